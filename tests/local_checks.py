"""Check bodies shared by tests/test_local_emu.py (the kernel sources on the fibre emulator) and tests/test_local_gpu.py (the
gfx950 build): the forward of local docking -- dlpd_local_correlate with one volume pair per pose and on a coarser grid,
dlpd_local_filter over its whole window, and the reference's recorded outputs G1 (MultiplyVolumes) and G8
(LocalDockingModel.forward on recorded volumes).  Signature (lib, device, ...): lib = the emulated library with device "cpu",
or None (the built library) with a GPU device.  Expected values are computed on the host.

Tolerances are derived, not chosen (as in test_local_emu.py): a correlation value is an f32 sum of K products in some order on
both sides, so |got - want| <= 2 (K + 1) 2^-24 sum|v1 v2| (the sum taken in float64 here)."""
import json
import os

import numpy as np
import torch

from oracle import docking_oracle as orc

TOL = 1e-4
EPS = 2.0 ** -24


def signed_index(t, N):
    return tuple(int(v) % N for v in t)


def direct64(v1, v2, t):
    """sum_x v1[c, x + t] v2[c, x] and sum |..| for ONE signed translation (the slices of orc.correlate_direct), float64,
    (C,) each; zero where a component reaches the box edge."""
    v1, v2 = np.asarray(v1, dtype=np.float64), np.asarray(v2, dtype=np.float64)
    L = v1.shape[-1]
    if max(abs(int(v)) for v in t) >= L:
        z = np.zeros(v1.shape[0])
        return z, z
    a, b = [], []
    for v in t:
        v = int(v)
        a.append(slice(v, L) if v >= 0 else slice(0, L + v))
        b.append(slice(0, L - v) if v >= 0 else slice(-v, L))
    prod = v1[:, a[0], a[1], a[2]] * v2[:, b[0], b[1], b[2]]
    return prod.sum(axis=(1, 2, 3)), np.abs(prod).sum(axis=(1, 2, 3))


# ---------------------------------------------------------------------------------------------- dlpd_local_correlate
def check_given_volumes_per_pose_and_coarse_modes(lib, device, L=6):
    """R = null (volumes as they are), one volume pair per pose, and the two coarse conventions on a half-resolution grid.
    T lives on the grid of 2L points: negative odd components (floor != trunc), a centre beyond the box, the last overlap."""
    from deeplocalproteindocking_amd import ops
    C, P = 2, 6
    g = torch.Generator().manual_seed(77)
    rec, lig = torch.randn(P, C, L, L, L, generator=g), torch.randn(P, C, L, L, L, generator=g)
    T = torch.tensor([[-3, 5, -1], [-(L + 1), 3, L + 3], [1, -1, -5], [0, 0, 0], [-(2 * L - 1), 2 * L - 1, -(2 * L - 3)], [-1, 1, -3]],
                     dtype=torch.int32)
    recd, ligd, Td = rec.to(device), lig.to(device), T.to(device)
    full = mag = None
    if L <= 6:                                           # the whole oracle volume where it is cheap: direct64 is its entry
        full = [orc.correlate_direct(rec[p:p + 1].numpy(), lig[p:p + 1].numpy())[0] for p in range(P)]
        mag = [orc.correlate_direct(np.abs(rec[p:p + 1].numpy()), np.abs(lig[p:p + 1].numpy()))[0] for p in range(P)]
    nonzero = 0
    for mode, fn in (("floor", np.floor), ("trunc", np.trunc)):
        got = ops.local_correlate(recd, ligd, Td, radius=0, scale=2, coarse=mode, lib=lib).reshape(P, C).cpu()
        for p in range(P):
            t = fn(T[p].numpy() / 2.0).astype(int)
            want, m = direct64(rec[p].numpy(), lig[p].numpy(), t)
            if full is not None:
                idx = (slice(None),) + signed_index(t, 2 * L)
                inside = (np.abs(t) < L).all()
                assert np.allclose(m, mag[p][idx] if inside else np.zeros(C), rtol=1e-13, atol=0.0)
                assert np.allclose(want, full[p][idx] if inside else np.zeros(C), rtol=0.0, atol=1e-13 * m.max())
            nonzero += int((want != 0).any())
            assert (np.abs(got[p].numpy() - want) <= 2 * (L ** 3 + 1) * EPS * m).all(), (mode, p, got[p].numpy(), want)
    assert nonzero >= 2 * (P - 1)                        # (one centre lies beyond the box under either convention, no more)
    a = ops.local_correlate(recd, ligd, Td, radius=0, scale=2, coarse="floor", lib=lib)
    b = ops.local_correlate(recd, ligd, Td, radius=0, scale=2, coarse="trunc", lib=lib)
    assert not torch.equal(a, b)                        # negative odd components tell the two apart


# ---------------------------------------------------------------------------------------------- dlpd_local_filter
def check_filter_minimum_per_pose(lib, device, r=2, coarse="floor", H=2):
    """dlpd_local_filter's per-pose minimum against numpy on the scores it wrote (argmin: first occurrence), with windows of
    more voxels than a wave has lanes (r = 2: 125, two trips of the 64-lane loop; r = 3: 343, six), the coarse window of scale
    2 under either convention, ties among masked (zero) scores, and a filter too wide for the kernel.
    The scores answer to local_features + orc.filter_mlp to 1e-6 of max|want|: a float32 MLP against a float32 MLP of at most
    H + 5 terms per score."""
    from deeplocalproteindocking_amd import ops
    g = torch.Generator().manual_seed(8)
    P, C0, C1 = 5, 3, 2
    W, Wc = 2 * r + 1, 2 * ops.local_coarse_radius(r, 2) + 1
    corr0, corr1 = torch.randn(P, C0, W, W, W, generator=g), torch.randn(P, C1, Wc, Wc, Wc, generator=g)
    clash = torch.rand(P, W, W, W, generator=g)
    clash[1] = 2.0                                       # every voxel of pose 1 masked: all scores 0, index 0 wins
    T = torch.tensor([[-3, 5, -1], [0, 0, 0], [1, -1, 7], [-7, -7, -7], [2, 4, 6]], dtype=torch.int32)
    W1, b1 = torch.randn(H, C0 + C1, generator=g), torch.randn(H, generator=g)
    W2, b2 = -torch.rand(1, H, generator=g), torch.tensor([0.5])
    dv = [t.to(device) for t in (corr0, corr1, clash, T)]
    score, best, besti = ops.local_filter(*dv, r, W1, b1, W2, b2, scale=2, coarse=coarse, clip=0.7, threshold=0.6, lib=lib)
    score, best, besti = score.cpu(), best.cpu(), besti.cpu()
    feat = ops.local_features(corr0, corr1, T, r, scale=2, coarse=coarse, clip=0.7)
    want = (orc.filter_mlp(feat, W1, b1, W2, b2).reshape(P, W, W, W) * (clash < 0.6).float()).numpy()
    print("local_filter r=%d %s H=%d: worst score error %.3g of max|want|" %
          (r, coarse, H, np.abs(score.numpy() - want).max() / np.abs(want).max()), flush=True)
    assert np.abs(score.numpy() - want).max() <= 1e-6 * np.abs(want).max()
    flat = score.numpy().reshape(P, -1)
    assert besti.tolist() == np.argmin(flat, axis=1).tolist() and besti[1] == 0
    assert best.numpy().tobytes() == flat[np.arange(P), np.argmin(flat, axis=1)].tobytes()
    assert (flat == 0).any() and (flat < 0).any()
    wide = ops.local_filter(*dv, r, torch.randn(40, C0 + C1), torch.randn(40), torch.randn(1, 40), b2, scale=2, lib=lib)
    assert wide is None                                   # hidden width beyond the kernel's: the caller applies its module
    return besti.tolist()


# ---------------------------------------------------------------------------------------------- G1: MultiplyVolumes
def check_multiply_volumes_g1(lib, device, g):
    """g: tests/golden/g1_multiply_volumes.npz, the reference module's recorded outputs at L = 4 and 6 (every whole translation
    of the (2L - 1)^3 grid) and at fractional rows."""
    from deeplocalproteindocking_amd.ops import MultiplyVolumes
    mv = MultiplyVolumes(lib=lib)
    for L, count in ((4, 343), (6, 1331)):
        v1, v2 = torch.from_numpy(g["v1_L%d" % L]), torch.from_numpy(g["v2_L%d" % L])
        T = torch.from_numpy(g["T_L%d" % L]).float()
        assert T.shape[0] == count
        B = T.shape[0]
        got = mv(v1.expand(B, -1, -1, -1, -1).contiguous().to(device), v2.expand(B, -1, -1, -1, -1).contiguous().to(device),
                 T.to(device)).cpu().numpy()
        mag = orc.correlate_direct(np.abs(v1.numpy()), np.abs(v2.numpy()))[0]                 # sum |v1 v2| per translation
        N = 2 * L
        bound = np.stack([mag[(slice(None),) + signed_index(t, N)] for t in g["T_L%d" % L]]) * 2 * (L ** 3 + 1) * EPS
        assert got.shape == g["out_L%d" % L].shape
        assert (np.abs(got - g["out_L%d" % L]) <= bound).all()
        assert np.abs(g["out_L%d" % L]).max() > 1.0
    # fractional rows: int() truncates toward zero
    v1 = torch.from_numpy(g["v1_L6"]).repeat(2, 1, 1, 1, 1)
    v2 = torch.from_numpy(g["v2_L6"]).repeat(2, 1, 1, 1, 1)
    got = mv(v1.to(device), v2.to(device), torch.from_numpy(g["Tfrac"]).to(device)).cpu().numpy()
    mag = orc.correlate_direct(np.abs(g["v1_L6"]), np.abs(g["v2_L6"]))[0]
    tt = np.trunc(g["Tfrac"]).astype(int)
    bound = np.stack([mag[(slice(None),) + signed_index(t, 12)] for t in tt]) * 2 * (6 ** 3 + 1) * EPS
    assert (np.abs(got - g["out_frac"]) <= bound).all()
    return v1, v2


# ---------------------------------------------------------------------------------------------- G8: LocalDockingModel
def g8():
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "local", "g8_local_forward.npz"))


def g8_filter(g):
    from deeplocalproteindocking_amd.Models import SimpleFilter
    filt = SimpleFilter(g["num_outputs"].tolist())
    keys = json.loads(bytes(g["filter_keys"]).decode())
    assert list(filt.state_dict().keys()) == keys
    filt.load_state_dict({k: torch.from_numpy(g["filter_sd_" + k]) for k in keys}, strict=True)
    return filt.eval()


def check_local_model_on_recorded_volumes(lib, device, g):
    """g: tests/golden/local/g8_local_forward.npz.  LocalDockingModel.forward with the reference's own representation volumes
    (boxes 12 and 6) in place of the representation: the correlation kernel, the trunc convention on fractional and
    out-of-box T, and the filter kernel against the reference's recorded scores, in the 1e-4 band."""
    from deeplocalproteindocking_amd.Models import LocalDockingModel
    rec, lig, T = (torch.from_numpy(g[k]).to(device) for k in ("receptor", "ligand", "T"))
    want = g["out"]
    band = TOL * np.abs(want).max()
    assert (np.abs(g["T"]) >= rec.shape[2]).any() and (g["T"] != np.trunc(g["T"])).any()

    class Recorded(torch.nn.Module):                     # isolates the new kernels and the trunc convention
        def forward(self, x):
            tag = "rec" if x is rec else "lig"
            return [torch.from_numpy(g["%s_vol%d" % (tag, i)]).to(device) for i in range(2)]
    stub = LocalDockingModel(Recorded(), g8_filter(g).to(device), lib=lib).eval()
    with torch.no_grad():
        got = stub(rec, lig, T).cpu().numpy()
    print("LocalDockingModel (recorded volumes): max error %.3g, band %.3g" % (np.abs(got - want).max(), band), flush=True)
    assert got.shape == want.shape == (rec.shape[0], 1)
    assert np.abs(got - want).max() <= band
    return band
