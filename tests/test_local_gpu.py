"""Local docking on the real gfx950 build: dlpd_local_correlate, Docker.score_poses and refine at the reference's shapes
([16@80^3, 32@40^3]) and at 48@64^3, on dense random and on protein-shaped (mostly zero) volumes.  Expected values are
float64 direct sums over the window (no 160^3 transform needed); the rotated ligand is the CPU oracle's.  Tolerances as in
test_local_emu.py: the f32 summation bound 2 (K + 1) 2^-24 sum|v1 v2| plus the parity band 1e-4 of the largest value
compared.  Beyond those shapes: the correlation at boxes 33 / 96 / 127 / 128 (the ends of its launch geometry), one volume
pair per pose and the coarse conventions, the filter kernel over windows of 5^3 and 7^3, and the reference's recorded outputs
G1 / G8 -- check bodies in tests/local_checks.py, shared with test_local_emu.py.  Nothing here reads the reference tree."""
import numpy as np
import pytest
import torch

from oracle import docking_oracle as orc
import local_checks as lc

pytestmark = pytest.mark.gpu
TOL = 1e-4
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    import __graft_entry__ as entry
    entry.build()
    return torch.device("cuda:0")


def _rots(n, seed=1):
    ang = np.random.RandomState(seed).uniform(-np.pi, np.pi, size=(n, 3))
    return orc.euler_to_matrix(ang[:, 0], np.abs(ang[:, 1]), ang[:, 2])


def _window(r):
    return [(dx, dy, dz) for dx in range(-r, r + 1) for dy in range(-r, r + 1) for dz in range(-r, r + 1)]


def _volume(C, L, seed, kind, amp=0.3):
    """dense: random everywhere; protein: zero outside an off-centre ellipsoid that fills about a sixth of the box."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(C, L, L, L, generator=g) * amp
    if kind == "protein":
        ax = torch.arange(L, dtype=torch.float32)
        x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
        c = L / 2.0
        inside = ((x - c - 2) / (0.42 * L)) ** 2 + ((y - c + 1) / (0.3 * L)) ** 2 + ((z - c) / (0.26 * L)) ** 2 <= 1.0
        v = v * inside.float()
    return v


def _direct(rec, lig, tau):
    """sum_x rec[c, x + tau] lig[c, x] and sum |..| for one signed translation, float64, (C,) each."""
    L = rec.shape[-1]
    if max(abs(int(t)) for t in tau) >= L:
        z = np.zeros(rec.shape[0])
        return z, z
    a, b = [], []
    for t in tau:
        t = int(t)
        a.append(slice(t, L) if t >= 0 else slice(0, L + t))
        b.append(slice(0, L - t) if t >= 0 else slice(-t, L))
    prod = rec[:, a[0], a[1], a[2]] * lig[:, b[0], b[1], b[2]]
    return prod.sum(axis=(1, 2, 3)), np.abs(prod).sum(axis=(1, 2, 3))


def _translations(P, L, seed):
    """Signed translations with negative odd components, inside the range where the volumes overlap well."""
    T = np.random.RandomState(seed).randint(-(L // 4), L // 4 + 1, size=(P, 3))
    T[0] = [-3, 5, -1]
    T[1] = [-(L // 4) | 1, 1, -5]
    return T


# (L, C, r, kind, P).  Beside the reference's shapes, the shapes the backward already has (test_local_grad_gpu.py) and the
# ends of the launch geometry (csrc/dlpd_local.h, local_xt): box 33 -> 7 x-planes per block, 231 of 256 threads, a last slab
# of 5 planes, r = 3 -> one dx per block (grid.y = 7); box 127 -> 2 planes, 254 threads, 64 slabs, the last of ONE plane;
# box 128 -> DLPD_LOCAL_MAXL.  Three poses at boxes >= 96: the float64 sums on the host are what a case costs.
CORRELATE_CASES = [(80, 16, 1, "dense", 8), (80, 16, 1, "protein", 8), (40, 32, 2, "dense", 8), (40, 32, 0, "protein", 8),
                   (64, 48, 1, "dense", 8), (64, 48, 1, "protein", 8), (40, 4, 3, "dense", 8), (64, 5, 2, "protein", 8),
                   (33, 3, 3, "dense", 8), (96, 2, 1, "protein", 3), (127, 2, 1, "dense", 3), (128, 2, 0, "dense", 3)]


@pytest.mark.parametrize("L,C,r,kind,P", CORRELATE_CASES, ids=["%d-%d-%d-%s" % c[:4] for c in CORRELATE_CASES])
def test_local_correlate_matches_float64_direct_sums(dev, L, C, r, kind, P):
    from deeplocalproteindocking_amd import ops
    rec, lig = _volume(C, L, 100 + L + C, kind), _volume(C, L, 200 + L + C, kind)
    R = torch.from_numpy(_rots(P, seed=L + r)).float().contiguous()
    T = _translations(P, L, seed=3 * L + r)
    T[2] = [L - 1, -(L - 1), 0]                         # part of the window at and beyond |tau| = L - 1
    got = ops.local_correlate(rec.to(dev), lig.to(dev), torch.from_numpy(T).int().to(dev), R=R.to(dev), radius=r).cpu().numpy()
    again = ops.local_correlate(rec.to(dev), lig.to(dev), torch.from_numpy(T).int().to(dev), R=R.to(dev), radius=r).cpu().numpy()
    assert got.tobytes() == again.tobytes()              # fixed-order reduction: the same bits run to run
    rec64 = rec.numpy().astype(np.float64)
    worst = 0.0
    for p in range(P):
        lr = orc.rotate_volume(lig[None], R[p:p + 1])[0].numpy().astype(np.float64)
        want = np.zeros((C, 2 * r + 1, 2 * r + 1, 2 * r + 1))
        mag = np.zeros_like(want)
        for d in _window(r):
            want[:, d[0] + r, d[1] + r, d[2] + r], mag[:, d[0] + r, d[1] + r, d[2] + r] = _direct(rec64, lr, T[p] + np.array(d))
        scale = np.abs(want).max()
        dead = mag == 0.0
        assert (got[p][dead] == 0.0).all()               # no overlap (or all-zero overlap): exactly zero
        bound = 2 * (L ** 3 + 1) * EPS * mag + TOL * scale
        err = np.abs(got[p] - want)
        assert (err <= bound).all(), (p, float(err.max()), float(scale))
        worst = max(worst, float(err.max() / scale)) if scale > 0 else worst
    print("local_correlate %s L=%d C=%d r=%d: worst error %.3g of max|corr|" % (kind, L, C, r, worst))


def test_local_correlate_batches_a_list_beyond_the_launch_grid_limit(dev):
    """More poses than one launch can hold (2^24 - 1 blocks): ops.local_correlate splits the list; the poses behind the split
    get the bits they get in a call of their own."""
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd._lib import get_lib
    L, C = 40, 32
    most = get_lib().call("dlpd_local_max_poses", C, L)
    assert most == (2 ** 32 - 1) // 256 // (C * 7)
    P = most + 5
    rec, lig = _volume(C, L, 1, "dense").to(dev), _volume(C, L, 2, "dense").to(dev)
    R = torch.from_numpy(_rots(64, seed=3)).float().to(dev).repeat((P + 63) // 64, 1, 1)[:P].contiguous()
    T = torch.from_numpy(np.random.RandomState(4).randint(-10, 11, size=(P, 3))).int().to(dev)
    got = ops.local_correlate(rec, lig, T, R=R, radius=0)
    tail = ops.local_correlate(rec, lig, T[-16:].contiguous(), R=R[-16:].contiguous(), radius=0)
    head = ops.local_correlate(rec, lig, T[:16].contiguous(), R=R[:16].contiguous(), radius=0)
    assert got[-16:].cpu().numpy().tobytes() == tail.cpu().numpy().tobytes()
    assert got[:16].cpu().numpy().tobytes() == head.cpu().numpy().tobytes()
    assert float(got.abs().min()) > 0.0


@pytest.mark.parametrize("L", [6, 33])
def test_local_correlate_given_volumes_per_pose_and_coarse_modes(dev, L):
    """One volume pair per pose, R = null, scale 2, "floor" against "trunc" on negative odd components: at the emulator's
    box 6 (36 of 256 threads active) and at box 33."""
    lc.check_given_volumes_per_pose_and_coarse_modes(None, dev, L=L)


@pytest.mark.parametrize("H", [2, 5, 32])
@pytest.mark.parametrize("coarse", ["floor", "trunc"])
@pytest.mark.parametrize("r", [2, 3])
def test_local_filter_minimum_per_pose_lowest_index_wins_a_tie(dev, r, coarse, H):
    """k_local_filter beyond one trip of its 64-lane loop: the coarse index of scale 2 under both conventions, hidden widths 2,
    5 (padded to 8) and 32, and the wave's lowest-index-wins reduction (an all-masked pose: 125 / 343 tied zeros, index 0)."""
    lc.check_filter_minimum_per_pose(None, dev, r=r, coarse=coarse, H=H)


def test_multiply_volumes_reproduces_the_reference_module(dev, golden):
    """G1 on the device: boxes 4 and 6, where 16 / 36 of a block's 256 threads are active."""
    lc.check_multiply_volumes_g1(None, dev, golden("g1_multiply_volumes.npz"))


def test_local_docking_model_reproduces_the_reference_forward_on_recorded_volumes(dev):
    """G8 on the device, the half that needs no representation: the reference's recorded volumes (boxes 12 and 6), fractional
    and out-of-box T, the trunc convention.  (The whole call stays on the emulator: the fixture's representation has 2 and 4
    output channels, which the HIP convolution rejects by design.)"""
    lc.check_local_model_on_recorded_volumes(None, dev, lc.g8())


def _model(sizes, thr, clip, dev, seed=3):
    from deeplocalproteindocking_amd.Models import GlobalDockingModel, SimpleFilter
    torch.manual_seed(seed)
    filt = SimpleFilter(sizes)
    with torch.no_grad():
        filt.fc[0].bias.normal_(0.0, 0.3)
        filt.fc[2].bias.normal_(0.0, 0.3)
    W = [w.detach().cpu().numpy().astype(np.float64) for w in filt.parameters_tuple()]
    return GlobalDockingModel(None, filt, threshold_clash=thr, clip=clip).to(dev).eval(), W


def _score64(rec, lig_rot, W, tau, clip):
    """The filter's value at one signed translation from float64 direct sums (floor on the coarse grid)."""
    feats = []
    for a, b in zip(rec, lig_rot):
        s = rec[0].shape[-1] // a.shape[-1]
        feats.append(np.clip(_direct(a, b, [int(np.floor(t / s)) for t in tau])[0], -clip, clip))
    W1, b1, W2, b2 = W
    return float(W2.reshape(-1) @ np.maximum(W1 @ np.concatenate(feats) + b1, 0.0) + b2.reshape(-1)[0])


# (sizes, L, kind, clip, r).  The last two: the whole window of the filter kernel (r = 2: 125 entries, two trips of its 64-lane
# loop; r = 3: 343, six) with the coarse window of the second resolution, on the smallest box that holds them.
SCORE_CASES = [([16, 32], 80, "dense", 5.0, 1), ([16, 32], 80, "protein", 0.5, 1), ([48], 64, "dense", 5.0, 1), ([48], 64, "protein", 5.0, 1),
               ([4, 6], 24, "dense", 0.5, 2), ([4, 6], 24, "dense", 0.5, 3)]
SCORE_IDS = ["sizes0-80-dense-5.0", "sizes1-80-protein-0.5", "sizes2-64-dense-5.0", "sizes3-64-protein-5.0", "sizes4-24-dense-0.5-r2",
             "sizes5-24-dense-0.5-r3"]


@pytest.mark.parametrize("sizes,L,kind,clip,r", SCORE_CASES, ids=SCORE_IDS)
def test_score_poses_matches_float64_direct_sums(dev, sizes, L, kind, clip, r):
    from deeplocalproteindocking_amd.Docker import Docker
    P = 8
    amp = 0.02 if kind == "dense" else 0.05
    rec = [_volume(c, L >> i, 300 + c, kind, amp) for i, c in enumerate(sizes)]
    lig = [_volume(c, L >> i, 400 + c, kind, amp) for i, c in enumerate(sizes)]
    g = torch.Generator().manual_seed(7)
    recf, ligf = torch.rand(L, L, L, generator=g), torch.rand(L, L, L, generator=g)
    if kind == "protein":
        recf, ligf = recf * (rec[0][0] != 0), ligf * (lig[0][0] != 0)
    R = _rots(P, seed=L)
    T = _translations(P, L, seed=L + 1)
    rec64, recf64 = [v.numpy().astype(np.float64) for v in rec], recf.numpy().astype(np.float64)
    rot = lambda v, p: orc.rotate_volume(v[None], torch.from_numpy(R[p:p + 1]).float())[0].numpy().astype(np.float64)
    # the clash sums of every compared translation in float64 first; the threshold goes into the middle of the widest gap of
    # their middle third, so that the float64 sums themselves keep clear of it
    ligf_rot = [rot(ligf[None], p)[0] for p in range(P)]
    norm = np.zeros((P, 2 * r + 1, 2 * r + 1, 2 * r + 1))
    for p in range(P):
        for d in _window(r):
            norm[p, d[0] + r, d[1] + r, d[2] + r] = _direct(recf64[None], ligf_rot[p][None], T[p] + np.array(d))[0][0]
    srt = np.sort(norm.reshape(-1))
    third = srt[len(srt) // 3: 2 * len(srt) // 3 + 1]
    k = int(np.argmax(np.diff(third)))
    thr = float(0.5 * (third[k] + third[k + 1]))
    model, W = _model(sizes, thr, clip, dev)
    dk = Docker(model, box_size=L, max_conf=10, rotations=R, device=dev)
    got = dk.score_poses(rec, lig, R, T, recf, ligf, radius=r).cpu().numpy()
    want = np.zeros_like(got, dtype=np.float64)
    sure = np.abs(norm - thr) > 1e-3 * thr
    for p in range(P):
        lig_rot = [rot(v, p) for v in lig]
        for d in _window(r):
            i = (p, d[0] + r, d[1] + r, d[2] + r)
            want[i] = _score64(rec64, lig_rot, W, T[p] + np.array(d), clip) if norm[i] < thr else 0.0
    band = TOL * np.abs(want).max()
    err = np.abs(got - want)
    print("score_poses %s %s L=%d clip %s: worst error %.3g of the band; %d of %d near the threshold, %d non-zero" %
          (sizes, kind, L, clip, err[sure].max() / band, (~sure).sum(), sure.size, (want[sure] != 0).sum()))
    assert (~sure).sum() <= 0.01 * sure.size
    assert (want[sure] != 0).sum() >= 0.3 * sure.sum()
    assert (err[sure] <= band).all()


def test_score_poses_returns_the_search_s_own_scores_and_refine_is_reproducible(dev):
    """The tie between the two GPU paths: every entry of the list the fused FFT search produced, re-scored by direct correlation
    at its own (rotation, translation), gets its score back."""
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Models import GlobalDockingModel, SimpleFilter, SyntheticRepr
    from deeplocalproteindocking_amd.Utils.Rotations import local_perturbations
    L, K = 80, 100
    torch.manual_seed(31)
    repr_ = SyntheticRepr(num_outputs=(16, 32), seed=5, amplitude=0.12)
    filt = SimpleFilter(repr_.get_num_outputs())
    rec, lig = repr_.make(L, "rec"), repr_.make(L, "lig")
    R = _rots(6, seed=15)
    recf, ligf = _volume(1, L, 32, "protein", 1.0)[0].abs(), _volume(1, L, 33, "protein", 1.0)[0].abs()
    recf64 = recf.numpy().astype(np.float64)
    ligf_rot = [orc.rotate_volume(ligf[None, None], torch.from_numpy(R[i:i + 1]).float())[0, 0].numpy().astype(np.float64)
                for i in range(6)]
    thr = 0.3 * float(_direct(recf64[None], ligf_rot[0][None], (0, 0, 0))[0][0])
    model = GlobalDockingModel(repr_, filt, threshold_clash=thr).to(dev)
    dk = Docker(model, box_size=L, max_conf=K, rotations=R, device=dev)
    top = list(dk.dock_volumes(rec, lig, recf, ligf, batch_size=2, write=False))
    assert dk.path == "fused" and len(top) == K
    T = [dk.signed_translation(x, y, z) for _, x, y, z, _ in top]
    got = dk.score_poses(rec, lig, R[[e[0] for e in top]], T, recf, ligf, radius=0).cpu().numpy().reshape(-1)
    band = TOL * max(abs(e[4]) for e in top)             # <= max|V|: a stricter band than the stated one
    near = [abs(float(_direct(recf64[None], ligf_rot[e[0]][None], t)[0][0]) - thr) <= 1e-3 * thr for e, t in zip(top, T)]
    errs = [abs(float(g) - e[4]) for g, e, n in zip(got, top, near) if not n]
    print("search vs score_poses: worst error %.3g of the band, %d of %d near the threshold, best score %.4g" %
          (max(errs) / band, sum(near), K, top[0][4]))
    assert sum(near) <= 0.01 * K and top[0][4] < 0
    assert max(errs) <= band
    assert dk.top_list == top
    # refine: never worse than the re-scored input (the identity and d = 0 are among the candidates); the same bits twice
    Q = local_perturbations(5.0, 1)
    a = [(e[0].tobytes(), e[1], np.float32(e[2]).tobytes(), e[3]) for e in dk.refine(rec, lig, recf, ligf, poses=top[:20], perturbations=Q)]
    b = [(e[0].tobytes(), e[1], np.float32(e[2]).tobytes(), e[3]) for e in dk.refine(rec, lig, recf, ligf, poses=top[:20], perturbations=Q)]
    assert a == b and dk.top_list == top
    for Rm, tt, score, n in dk.refined_list:
        assert score <= float(got[n]) + band
    dk.release_engine()
