"""Checks shared by test_k1_chunk_layout_emu.py (emulated kernels) and test_k1_chunk_layout_gpu.py (the gfx950 build): K1
gathering from the chunk-major ligand copy (include/dlpd.h, dlpd_make_channel_chunks / dlpd_zfft_channel_chunks) against the
same kernel gathering from the channels-last copy.  Only addresses differ, so every comparison is bit for bit."""
import numpy as np
import torch

from oracle import docking_oracle as orc
from deeplocalproteindocking_amd.engine import DockingEngine, _ptr


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0


def chunk_width(L):
    """Channels per K1 block (K1ClCfg<2L>::CC): 8 at box 64, 16 at the other boxes."""
    return 8 if L == 64 else 16


def rotations(kind, nb):
    """'oblique': nb rotations with every axis tilted; 'z+oblique': one rotation about z, then oblique ones."""
    a = np.array([[0.4, 0.9, 1.7], [-1.3, 2.0, -0.2], [2.6, 0.6, -2.1]])[:nb]
    R = orc.euler_to_matrix(a[:, 0], a[:, 1], a[:, 2])
    if kind == "z+oblique":
        c, s = np.cos(0.7), np.sin(0.7)
        R[0] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return torch.from_numpy(np.ascontiguousarray(R)).float().contiguous()


def samples_reach_the_faces(R, L, c0, ext):
    """True if, for every rotation, some samples of the kernel's map p = c0 + M (v - c0) (columns r0..r2 | r3..r5 | r6..r8) have
    one corner inside and one outside the box: floor(p) = -1 occurs, and floor(p) = L - 1 too unless the volume is an embedded
    box (ext < L: its far side lies inside the large box, whose far face a rotation about the small pivot need not reach)."""
    v = np.arange(ext, dtype=np.float64) - c0
    d = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    for M in R.double().numpy():
        f = np.floor(c0 + d @ M)
        if not ((f == -1).any() and (ext < L or (f == L - 1).any())):
            return False
    return True


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_layout(lib, device, L, C):
    """buf.view(nchunk, L, L, L, CC)[k, ..., j] == vol[k CC + j]; padding channels zero; never larger than channels-last."""
    g = torch.Generator().manual_seed(31)
    CC = chunk_width(L)
    nchunk = (C + CC - 1) // CC
    vol = torch.randn(C, L, L, L, generator=g).to(device)
    n = lib.call("dlpd_channel_chunks_floats", C, L)
    assert n == nchunk * CC * L ** 3 and n <= lib.call("dlpd_channels_last_floats", C, L)
    buf = torch.full((n,), float("nan"), device=device)
    lib.call("dlpd_make_channel_chunks", _ptr(vol), _ptr(buf), C, L, _stream(device))
    b = buf.view(nchunk, L, L, L, CC)
    for k in range(nchunk):
        for j in range(CC):
            c = k * CC + j
            if c < C:
                assert torch.equal(b[k, ..., j], vol[c]), (k, j)
            else:
                assert not bool(b[k, ..., j].any()), (k, j)


def check_k1_equality(lib, device, L, C, R, extent=0, occupancy=False, c_base=0, extra=1, seed=33):
    """dlpd_zfft_channel_chunks == dlpd_zfft_channels_last_ext (dense / embedded extent) or dlpd_zfft_channels_last_occ (by the
    maps of dlpd_rotated_occupancy, skip_empty = 0) on the COMPLETE workspace: both start as NaN, so an element one of them
    leaves unwritten shows, and channels outside [c_base, c_base + C) must stay untouched."""
    from deeplocalproteindocking_amd import ops
    g = torch.Generator().manual_seed(seed)
    nb, NZ, CT = R.shape[0], L + 1, c_base + C + extra
    e = extent or L
    c0 = e / 2.0
    vol = torch.zeros(C, L, L, L)
    if occupancy:                                  # a blob off the centre: most cells of a rotated copy are empty
        lo, hi = e // 4, e // 4 + e // 3
        vol[:, lo:hi, lo + 2:hi + 2, lo - 1:hi - 1] = torch.randn(C, hi - lo, hi - lo, hi - lo, generator=g)
    else:
        vol[:, :e, :e, :e] = torch.randn(C, e, e, e, generator=g)
    vol, R, st = vol.to(device), R.to(device), _stream(device)
    assert samples_reach_the_faces(R.cpu(), L, c0, e)
    cl = torch.empty(lib.call("dlpd_channels_last_floats", C, L), device=device)
    lib.call("dlpd_make_channels_last", _ptr(vol), _ptr(cl), C, L, st)
    buf = torch.empty(lib.call("dlpd_channel_chunks_floats", C, L), device=device)
    lib.call("dlpd_make_channel_chunks", _ptr(vol), _ptr(buf), C, L, st)
    want = torch.full((nb * CT * NZ * L * L * 2,), float("nan"), device=device)
    got = torch.full_like(want, float("nan"))
    occ = 0
    if occupancy:
        nc = (L + 3) // 4
        occ_src = ops.tile_occupancy(vol.unsqueeze(0), lib=lib)
        occ_t = torch.empty(nb, nc, nc, nc, dtype=torch.uint8, device=device)
        lib.call("dlpd_rotated_occupancy", _ptr(occ_src), _ptr(R), _ptr(occ_t), 0, nb, L, c0, st)
        assert 0 < int(occ_t.sum()) < occ_t.numel()                       # both the gathered and the skipped cells occur
        occ = _ptr(occ_t)
        lib.call("dlpd_zfft_channels_last_occ", _ptr(cl), _ptr(R), occ, _ptr(want), nb, C, CT, c_base, L, c0, extent, 0, st)
    else:
        lib.call("dlpd_zfft_channels_last_ext", _ptr(cl), _ptr(R), _ptr(want), nb, C, CT, c_base, L, c0, extent, st)
    lib.call("dlpd_zfft_channel_chunks", _ptr(buf), _ptr(R), occ, _ptr(got), nb, C, CT, c_base, L, c0, extent, 0, st)
    assert bits_equal(got, want)
    w = got.view(nb, CT, NZ, L, L, 2)
    written = w[:, c_base:c_base + C]
    assert not bool(torch.isnan(written).any()) and float(written.abs().max()) > 1.0
    assert bool(torch.isnan(w[:, :c_base]).all()) and bool(torch.isnan(w[:, c_base + C:]).all())


def check_engine_lists(lib, device, L=32, C=8, nrot=32, batch=8, seed=35):
    """The same search with the layout on and off: identical ranked lists, entry for entry."""
    g = torch.Generator().manual_seed(seed)
    H = C // 2
    rec, lig = torch.randn(C, L, L, L, generator=g) * 0.1, torch.randn(C, L, L, L, generator=g) * 0.1
    recf, ligf = torch.rand(L, L, L, generator=g), torch.rand(L, L, L, generator=g)
    W = (torch.randn(H, C, generator=g), torch.randn(H, generator=g), torch.randn(1, H, generator=g), torch.randn(1, generator=g))
    ang = np.random.RandomState(seed).uniform(-np.pi, np.pi, size=(nrot, 3))
    R = torch.from_numpy(orc.euler_to_matrix(ang[:, 0], np.abs(ang[:, 1]), ang[:, 2])).float().contiguous()
    lists = {}
    for on in (True, False):
        eng = DockingEngine(L, C, *W, clip=5.0, threshold_clash=0.125 * L ** 3, max_conf=64, batch=batch, device=device, lib=lib,
                            k1_chunk_major=on)
        sw = eng.switches()
        assert sw["k1"] == "channels_last" and sw["k1_source_layout"]["fine"] == ("chunk_major" if on else "channels_last")
        assert eng.fine.ligcl.numel() <= lib.call("dlpd_channels_last_floats", C, L)
        eng.set_receptor(rec, recf)
        eng.set_ligand(lig, ligf)
        eng.reset_top()
        eng.search(R)
        lists[on] = eng.top_entries()
    for a, b in zip(lists[True], lists[False]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert len(lists[True][0]) == 64
