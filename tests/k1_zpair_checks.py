"""Checks shared by test_k1_zpair_emu.py (emulated kernels) and test_k1_zpair_gpu.py (the gfx950 build): K1's four-lane gather
from the chunk-major ligand copy at box 64 (csrc/dlpd_k1.h, ZPAIR: one 64-byte request for a sample's two z corners, the other
corner of a lane's row arriving by a quad exchange) against the channels-last entry, which keeps the two-lane gather.  The
sample is meant to be the same bits -- the sign of an all-zero sample included -- so every comparison is on raw 32-bit patterns.
Built on the helpers of k1_chunk_layout_checks.py; the cases here are the ones that module's rotations and volumes do not
reach: integer sample positions, whole planes outside the box on either z side, strictly negative volumes."""
import numpy as np
import torch

import k1_chunk_layout_checks as chk
from deeplocalproteindocking_amd.engine import _ptr

L = 64


def _mat(rows):
    return np.array(rows, dtype=np.float64)


def lattice_rotations():
    """The identity and a quarter turn about x, y and z: every sample position is an integer, every weight exactly 0 or 1.  About
    the centre L / 2 a quarter turn maps one coordinate to L - v, so one whole plane samples position L (outside, beyond the
    high face) and its neighbour position L - 1 (on the face)."""
    R = np.stack([np.eye(3),
                  _mat([[1, 0, 0], [0, 0, -1], [0, 1, 0]]),
                  _mat([[0, 0, 1], [0, 1, 0], [-1, 0, 0]]),
                  _mat([[0, -1, 0], [1, 0, 0], [0, 0, 1]])])
    return torch.from_numpy(R).float().contiguous()


def half_turns():
    """Half turns about x and about y: with the pivot c0 off the centre, p_z = 2 c0 - z leaves the box on one side for
    |2 c0 - L| whole planes (integer positions: floor(p_z) < -1 or > L - 1, all eight weights zero)."""
    R = np.stack([_mat([[1, 0, 0], [0, -1, 0], [0, 0, -1]]), _mat([[-1, 0, 0], [0, 1, 0], [0, 0, -1]])])
    return torch.from_numpy(R).float().contiguous()


def floor_z(R, c0, ext=L):
    """floor(p_z) of every sample of the kernel's map p = c0 + M (v - c0) (p_z uses r2, r5, r8), per rotation, in float64."""
    v = np.arange(ext, dtype=np.float64) - c0
    d = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    return [np.floor(c0 + d @ M[:, 2]) for M in R.double().numpy()]


def z_faces_reached(R, c0):
    """True if every rotation has samples straddling the LOW z face (floor = -1: only the z1 corner inside) and the HIGH one
    (floor = L - 1: only the z0 corner inside) -- the two cases in which the old code's clamped corners are one voxel twice."""
    return all((f == -1).any() and (f == L - 1).any() for f in floor_z(R, c0))


def planes_outside(R, c0, side):
    """True if every rotation has samples wholly outside in z on `side`: floor(p_z) < -1 ('low') or > L - 1 ('high')."""
    return all(((f < -1) if side == "low" else (f > L - 1)).any() for f in floor_z(R, c0))


def volume(kind, C, seed=41):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(C, L, L, L, generator=g)
    if kind == "negative":                         # strictly negative: an all-zero-weight sample is -0.0, not +0.0
        return -(v.abs() + 0.25)
    assert kind == "mixed"                         # both signs in every face layer
    for face in (v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1], v[:, :, :, 0], v[:, :, :, -1]):
        assert bool((face > 0).any()) and bool((face < 0).any())
    return v


def check_same_bits(lib, device, C, R, vol, c0=L / 2.0, c_base=0, extra=1):
    """dlpd_zfft_channel_chunks == dlpd_zfft_channels_last_ext on the complete workspace (both start as NaN), as raw bits."""
    nb, NZ, CT = R.shape[0], L + 1, c_base + C + extra
    vol, R, st = vol.to(device), R.to(device), chk._stream(device)
    cl = torch.empty(lib.call("dlpd_channels_last_floats", C, L), device=device)
    lib.call("dlpd_make_channels_last", _ptr(vol), _ptr(cl), C, L, st)
    buf = torch.empty(lib.call("dlpd_channel_chunks_floats", C, L), device=device)
    assert buf.numel() == -(-C // chk.chunk_width(L)) * chk.chunk_width(L) * L ** 3 <= cl.numel()
    lib.call("dlpd_make_channel_chunks", _ptr(vol), _ptr(buf), C, L, st)
    want = torch.full((nb * CT * NZ * L * L * 2,), float("nan"), device=device)
    got = torch.full_like(want, float("nan"))
    lib.call("dlpd_zfft_channels_last_ext", _ptr(cl), _ptr(R), _ptr(want), nb, C, CT, c_base, L, c0, 0, st)
    lib.call("dlpd_zfft_channel_chunks", _ptr(buf), _ptr(R), 0, _ptr(got), nb, C, CT, c_base, L, c0, 0, 0, st)
    assert chk.bits_equal(got, want)
    w = got.view(nb, CT, NZ, L, L, 2)
    written = w[:, c_base:c_base + C]
    assert not bool(torch.isnan(written).any()) and float(written.abs().max()) > 1.0
    assert bool(torch.isnan(w[:, :c_base]).all()) and bool(torch.isnan(w[:, c_base + C:]).all())
    return written


def check_lattice(lib, device, C, kind, nb=4):
    R = lattice_rotations()[:nb]
    for f in floor_z(R, L / 2.0):
        assert (f == np.floor(f)).all()
    assert (floor_z(R[1:2], L / 2.0)[0] == L).any()                 # the quarter turn about x: one whole plane beyond the high z face
    w = check_same_bits(lib, device, C, R, volume(kind, C))
    # the identity samples the voxels themselves: plane kz = 0 of the z transform is the sum over z
    vol = volume(kind, C).to(device)
    s = w[0, :, 0, :, :, 0]
    assert torch.allclose(s, vol.sum(-1), rtol=0, atol=1e-3)


def check_planes_outside(lib, device, C, kind, side, nb=2):
    """Half turns about a pivot four voxels off the centre (integer positions), then the oblique set about the same pivot."""
    c0 = L / 2.0 + (4.0 if side == "high" else -4.0)
    for R in (half_turns()[:nb], chk.rotations("oblique", nb)):
        assert planes_outside(R, c0, side)
        check_same_bits(lib, device, C, R, volume(kind, C), c0=c0)


def check_oblique_faces(lib, device, C, kind, c_base=0, extra=1, nb=2):
    R = chk.rotations("oblique", nb)
    assert z_faces_reached(R, L / 2.0) and chk.samples_reach_the_faces(R, L, L / 2.0, L)
    check_same_bits(lib, device, C, R, volume(kind, C), c_base=c_base, extra=extra)
