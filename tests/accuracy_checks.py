"""Check bodies shared by tests/test_gpu_accuracy.py (the gfx950 build) and tests/test_accuracy_emu.py (the same kernel
sources on the fibre emulator): distance from the TRUTH, not from the 1e-4 contract band.

The yardstick.  For an output X of the kernels, X64 is the oracle evaluated in float64 throughout (rotation matrices
included) and X32 the oracle in float32 on the same inputs.  With e_k = X - X64 and e_o = X32 - X64 over the compared voxels

    rms(e_k) <= 2 * rms(e_o)        and        max|e_k| <= 3 * max|e_o|

The bound comes from the reference -- an independent float32 evaluation of the same mathematics, made inside the test for
every case -- never from the kernels.  Both sides are float32 transforms with correctly rounded twiddles, so their errors
are draws from one distribution; on the emulated library the largest ratios measured were 1.08 (RMS) and 1.31 (max), and
the margins are about twice that (the maximum of N^3 draws moves more than the RMS).  Every check prints both ratios
(EXPERIMENTS.md, section ACCURACY holds the values of an MI355X).

A case cannot hide a failure: voxels whose float64 clash correlation lies within 1e-3 * thr of the threshold are left out
(a mask flip there is not an arithmetic error), at most 1 % of a case -- thr is the median of the float64 clash
correlations of the compared rotations, so few voxels are near it --; the masked fraction of X64 lies between 0.2 and
0.7; rms(e_o) > 0.

Reading the fused pipeline channel by channel.  K3 never materialises the correlations.  A PROBE FILTER makes it
transparent at no cost in precision: W1 = [I_S; -I_S] on a subset S of the channels, b1 = 0, W2 = [w, -w] with w a vector
of +-1, b2 = 0.  relu(x) - relu(-x) = x exactly, so V = sum_{c in S} w_c clamp(corr_c): an error in any probed channel
appears at full weight, through the product K3 (role-split, hidden width up to 48 fused), not a diagnostic path.
"""
import itertools

import numpy as np
import torch

from oracle import docking_oracle as orc

RMS_MARGIN, MAX_MARGIN = 2.0, 3.0
NEAR_BAND, NEAR_CAP = 1e-3, 0.01


def _rms(e):
    return float(torch.sqrt((e * e).mean()))


def yardstick(label, X, X32, X64, keep=None, growth=1.0):
    """Assert the two inequalities over the voxels ``keep`` (all if None) and print the figures first.
    growth: factor on both margins for a path whose FORMULATION implies it (the caller derives it; 1 everywhere else)."""
    X, X32, X64 = (torch.as_tensor(t).detach().cpu().double().reshape(-1) for t in (X, X32, X64))
    assert X.shape == X32.shape == X64.shape, (label, X.shape, X32.shape, X64.shape)
    if keep is not None:
        keep = torch.as_tensor(keep).reshape(-1)
        X, X32, X64 = X[keep], X32[keep], X64[keep]
    ek, eo = X - X64, X32 - X64
    rk, ro, mk, mo = _rms(ek), _rms(eo), float(ek.abs().max()), float(eo.abs().max())
    scale = float(X64.abs().max())
    row = (label, rk / ro if ro > 0 else float("inf"), mk / mo if mo > 0 else float("inf"), mk / scale if scale > 0 else mk)
    print("ACCURACY | %-58s | rms %.3f | max %.3f | max|e_k|/max|X64| %.2e | oracle32 %.2e" %
          (label, row[1], row[2], row[3], mo / scale if scale > 0 else mo), flush=True)
    assert ro > 0 and mo > 0, (label, "the float32 oracle has no error here: the case measures nothing")
    assert rk <= growth * RMS_MARGIN * ro, (label, "rms", rk, ro, rk / ro)
    assert mk <= growth * MAX_MARGIN * mo, (label, "max", mk, mo, mk / mo)
    return row


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------

def rots(n, seed=1):
    ang = np.random.RandomState(seed).uniform(-np.pi, np.pi, size=(n, 3))
    return orc.euler_to_matrix(ang[:, 0], np.abs(ang[:, 1]), ang[:, 2])


def signed_permutations():
    """The 24 proper rotations that map the lattice to itself."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return np.stack(out)


def permuted(vol, R):
    """The exact result of rotating vol (..., L, L, L) by a signed permutation R about L/2: out[i] = vol[c0 + R^T (i - c0)],
    an index permutation; a source index L lies outside the box and gives zero.  Integer arithmetic only."""
    vol = torch.as_tensor(vol)
    L = vol.shape[-1]
    Ri = np.rint(np.asarray(R)).astype(np.int64)
    ar = torch.arange(L, dtype=torch.int64)
    i = torch.stack(torch.meshgrid(ar, ar, ar, indexing="ij"), dim=-1).reshape(-1, 3)          # output indices
    d2 = 2 * i - L                                                                             # 2 (i - c0): integers
    src2 = d2 @ torch.from_numpy(Ri) + L                                                       # 2 * source index
    assert bool((src2 % 2 == 0).all())
    src = src2 // 2
    ok = ((src >= 0) & (src < L)).all(dim=1)
    flat = (src[:, 0].clamp(0, L - 1) * L + src[:, 1].clamp(0, L - 1)) * L + src[:, 2].clamp(0, L - 1)
    out = vol.reshape(vol.shape[:-3] + (-1,))[..., flat] * ok.to(vol.dtype)
    return out.reshape(vol.shape)


def soi_rotations(golden_npz):
    """The 64 matrices of tests/golden/g2_rotations.npz in file order: head and tail of the 20 / 15 / 12 / 10 degree sets."""
    return np.concatenate([golden_npz["%s_%d" % (part, inc)] for inc in (20, 15, 12, 10) for part in ("first8", "last8")])


def axis_angle(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def face_rotations():
    """Turns that put samples within rounding distance of lattice points and of the faces of the box."""
    quarter = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return np.stack([axis_angle([1.0, 2.0, 3.0], 1e-4), axis_angle([3.0, -1.0, 2.0], 1e-2), axis_angle([2.0, 1.0, -1.0], 1e-4) @ quarter])


def face_mass(C, L, seed):
    """Non-negative volumes whose largest values lie on faces, edges and corners of the box: a face voxel counts 4 per
    face it lies on (a corner 64), the interior is at most 1."""
    g = torch.Generator().manual_seed(seed)
    ar = torch.arange(L)
    on = ((ar == 0) | (ar == L - 1)).float()
    nface = on[:, None, None] + on[None, :, None] + on[None, None, :]
    return torch.rand(C, L, L, L, generator=g) * (4.0 ** nface)


def protein_shaped(C, L, seed, amp=0.1):
    """Zero outside an off-centre ellipsoid that fills about a sixth of the box."""
    g = torch.Generator().manual_seed(seed)
    ax = torch.arange(L, dtype=torch.float32)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c = L / 2.0
    inside = ((x - c - 2) / (0.42 * L)) ** 2 + ((y - c + 1) / (0.3 * L)) ** 2 + ((z - c) / (0.26 * L)) ** 2 <= 1.0
    return torch.randn(C, L, L, L, generator=g) * amp * inside.float()


def extreme_ligands(C, L, seed):
    """Channel c takes pattern c mod 4: constant (energy at k = 0 and the padding's sidelobes), checkerboard (-1)^(x+y+z)
    (energy beside the Nyquist planes), constant along z only, constant along x only; amplitudes differ per channel."""
    g = torch.Generator().manual_seed(seed)
    ar = torch.arange(L)
    cb = (1.0 - 2.0 * ((ar[:, None, None] + ar[None, :, None] + ar[None, None, :]) % 2)).float()
    out = torch.empty(C, L, L, L)
    for c in range(C):
        amp = 0.05 + 0.1 * float(torch.rand(1, generator=g))
        k = c % 4
        if k == 0:
            out[c] = amp
        elif k == 1:
            out[c] = amp * cb
        elif k == 2:
            out[c] = (amp * torch.randn(L, L, 1, generator=g)).expand(L, L, L)
        else:
            out[c] = (amp * torch.randn(1, L, L, generator=g)).expand(L, L, L)
    return out


def impulse_positions(L):
    """The eight corners, a face centre and the box centre."""
    e = (0, L - 1)
    return [(x, y, z) for x in e for y in e for z in e] + [(0, L // 2, L // 2), (L // 2, L // 2, L // 2)]


def impulses(C, L, first=0):
    pos = impulse_positions(L)
    where = [pos[(first + c) % len(pos)] for c in range(C)]
    v = torch.zeros(C, L, L, L)
    for c, p in enumerate(where):
        v[c][p] = 1.0
    return v, where


def shifted(rec, b):
    """corr[t mod 2L] = rec[b + t] for a unit impulse at b, zero where b + t leaves the box: index arithmetic only."""
    L = rec.shape[-1]
    N = 2 * L
    out = torch.zeros(N, N, N, dtype=torch.float64)
    idx = []
    for a in range(3):
        t = torch.arange(-b[a], L - b[a])                      # translations that keep b + t inside
        idx.append(t % N)
    out[idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]] = rec.double()
    return out


def random_filter(C, H, seed, dead=2):
    """An ordinary SimpleFilter; ``dead`` hidden units get a bias that keeps them inactive on correlations of order 1."""
    g = torch.Generator().manual_seed(seed)
    W1, b1 = torch.randn(H, C, generator=g) * 0.3, torch.randn(H, generator=g) * 0.1
    b1[:dead] = -50.0
    return W1, b1, torch.randn(1, H, generator=g), torch.randn(1, generator=g)


def probe_width(lib, L, coarse=False):
    """The largest number of channels one probe can read at box L: hidden width 2 n must have a fused K3 (48 at boxes 32,
    64 and 80, less where the library says so)."""
    from deeplocalproteindocking_amd._lib import get_lib
    lib = lib or get_lib()
    return max(n for n in range(1, 25) if lib.call("dlpd_fused_hidden_pad", 2 * n, int(L), int(bool(coarse))) >= 0)


def probe_filters(C, width=24, signs=2, seed=0):
    """The probe filters that read C channels: subsets of at most ``width`` channels, ``signs`` sign vectors each; every
    filter has hidden width 2 * min(C, width), so they load into one live engine."""
    g = torch.Generator().manual_seed(1000 + seed)
    n = min(C, width)
    out = []
    for beg in range(0, C, n):
        S = list(range(beg, min(beg + n, C)))
        S = list(range(C - n, C)) if len(S) < n else S
        for _ in range(signs):
            w = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
            W1 = torch.zeros(2 * n, C)
            for j, c in enumerate(S):
                W1[j, c], W1[n + j, c] = 1.0, -1.0
            out.append((W1, torch.zeros(2 * n), torch.cat([w, -w])[None], torch.zeros(1)))
    return out


def single_channel_probe(C, c):
    W1 = torch.zeros(2, C)
    W1[0, c], W1[1, c] = 1.0, -1.0
    return W1, torch.zeros(2), torch.tensor([[1.0, -1.0]]), torch.zeros(1)


# ----------------------------------------------------------------------------------------------------------------------
# the oracle of one item (rotation or given volumes) in one precision
# ----------------------------------------------------------------------------------------------------------------------

def oracle_features(recs, ligs, clip, dtype):
    """The rows GlobalDockingModel.forward feeds its filter, by the oracle's own pieces: per-resolution correlate_fft,
    nearest upsample, channel concat (score_volumes, oracle/docking_oracle.py, up to its filter_mlp call -- so that several
    filters can read one set of correlations; test_accuracy_emu.py pins the two against each other)."""
    N = 2 * recs[0].shape[-1]
    conv = []
    for r, l in zip(recs, ligs):
        c = orc.correlate_fft(r[None], l[None], clip=clip, dtype=dtype)
        if c.shape[2] < N:
            s = N // c.shape[2]
            c = c.repeat_interleave(s, 2).repeat_interleave(s, 3).repeat_interleave(s, 4)
        conv.append(c)
    return torch.cat(conv, dim=1).permute(0, 2, 3, 4, 1).reshape(N * N * N, -1)


def oracle_scores(feat, filt, dtype):
    W1, b1, W2, b2 = (torch.as_tensor(t).to(dtype) for t in filt)
    return orc.filter_mlp(feat, W1, b1, W2, b2).reshape(-1)


class Case:
    """One receptor / ligand pair on one engine layout; items are rotations of the stored ligand or given volumes."""

    def __init__(self, lib, device, L, C, C1=0, seed=0, amp=0.05, has_clash=True, **engine_kw):
        self.lib, self.device, self.L, self.C, self.C1, self.has_clash = lib, torch.device(device), L, C, C1, has_clash
        self.engine_kw = engine_kw
        g = torch.Generator().manual_seed(seed)
        L1 = L // 2
        self.rec, self.lig = torch.randn(C, L, L, L, generator=g) * amp, torch.randn(C, L, L, L, generator=g) * amp
        self.recf, self.ligf = torch.rand(L, L, L, generator=g), torch.rand(L, L, L, generator=g)
        self.rec1 = torch.randn(C1, L1, L1, L1, generator=g) * 2 * amp if C1 else None
        self.lig1 = torch.randn(C1, L1, L1, L1, generator=g) * 2 * amp if C1 else None

    def _items(self, R, volumes, dtype):
        """-> per item (ligand volumes per resolution, forbidden volume) in ``dtype``."""
        if volumes is not None:
            vl, vf, vc = volumes
            for i in range(vl.shape[0]):
                yield [vl[i].to(dtype)] + ([vc[i].to(dtype)] if self.C1 else []), (vf[i].to(dtype) if self.has_clash else None)
            return
        for i in range(R.shape[0]):
            Rb = torch.from_numpy(np.ascontiguousarray(R[i:i + 1]))                  # float64; rotate_volume casts to dtype
            ligs = [orc.rotate_volume(self.lig[None], Rb, dtype=dtype)[0]]
            if self.C1:
                ligs.append(orc.rotate_volume(self.lig1[None], Rb, dtype=dtype)[0])
            yield ligs, (orc.rotate_volume(self.ligf[None, None], Rb, dtype=dtype)[0, 0] if self.has_clash else None)

    def oracle(self, filters, clip, R=None, volumes=None, exact_features=None):
        """-> thr, keep (n, N^3) bool, V64 and V32 as [filter] -> (n, N^3).  thr: the median of the float64 clash
        correlations of the items.  exact_features: optional callable(item) -> float64 feature rows from index arithmetic,
        used in place of the float64 transform (which must agree with it)."""
        recs = [self.rec] + ([self.rec1] if self.C1 else [])
        f64, f32 = torch.float64, torch.float32
        norms, feats64 = [], []
        V = {f64: [[] for _ in filters], f32: [[] for _ in filters]}
        for i, (ligs, forb) in enumerate(self._items(R, volumes, f64)):
            if self.has_clash:
                norms.append(orc.correlate_fft(self.recf[None, None], forb[None, None], dtype=f64)[0, 0].reshape(-1))
            feat = oracle_features(recs, ligs, clip, f64)
            if exact_features is not None:
                exact = exact_features(i)
                assert float((feat - exact).abs().max()) <= 1e-12 * max(1.0, float(exact.abs().max())), "index arithmetic vs float64 transform"
                feat = exact
            for k, filt in enumerate(filters):
                V[f64][k].append(oracle_scores(feat, filt, f64))
        thr, keep, mask64 = 0.0, None, None
        if self.has_clash:
            norms = torch.stack(norms)
            thr = float(norms.median())
            assert thr > 0
            keep = (norms - thr).abs() > NEAR_BAND * thr
            assert float((~keep).float().mean()) <= NEAR_CAP, ("voxels near the clash threshold", float((~keep).float().mean()))
            mask64 = (norms < thr).double()
            masked = float((mask64 == 0).double().mean())
            assert 0.2 <= masked <= 0.7, ("masked fraction", masked)
        for ligs, forb in self._items(R, volumes, f32):
            mask32 = None
            if self.has_clash:
                mask32 = (orc.correlate_fft(self.recf[None, None], forb[None, None], dtype=f32)[0, 0].reshape(-1) < thr).float()
            feat = oracle_features(recs, ligs, clip, f32)
            for k, filt in enumerate(filters):
                v = oracle_scores(feat, filt, f32)
                V[f32][k].append(v * mask32 if mask32 is not None else v)
        V64 = [torch.stack(v) * mask64 if mask64 is not None else torch.stack(v) for v in V[f64]]
        V32 = [torch.stack(v) for v in V[f32]]
        return thr, keep, V64, V32

    def engine(self, filt, clip, thr, batch):
        from deeplocalproteindocking_amd.engine import DockingEngine
        eng = DockingEngine(self.L, self.C, *filt, clip=clip, threshold_clash=thr, has_clash=self.has_clash, max_conf=16,
                            batch=batch, device=self.device, lib=self.lib, coarse_channels=self.C1, **self.engine_kw)
        eng.set_receptor(self.rec, self.recf if self.has_clash else None, self.rec1)
        eng.set_ligand(self.lig, self.ligf if self.has_clash else None, self.lig1)
        return eng

    def kernels(self, eng, filt, R=None, volumes=None, **batch_kw):
        """-> (n, N^3) scores of the engine, in batches of its size."""
        eng.set_filter(*filt)
        n = R.shape[0] if volumes is None else volumes[0].shape[0]
        dev, out = self.device, []
        for beg in range(0, n, eng.batch):
            end = min(beg + eng.batch, n)
            if volumes is None:
                Rd = torch.from_numpy(np.ascontiguousarray(R[beg:end])).float().to(dev).contiguous()
                V = eng.score_batch(Rd, **batch_kw)
            else:
                vl, vf, vc = volumes
                V = eng.score_batch(None, volumes=(vl[beg:end].to(dev), vf[beg:end].to(dev) if self.has_clash else None,
                                                   vc[beg:end].to(dev) if self.C1 else None))
            out.append(V.reshape(end - beg, -1).cpu().clone())
        return torch.cat(out)

    def run(self, label, filters, clip, R=None, volumes=None, exact_features=None, batch=2, eng=None, **batch_kw):
        """The whole check: oracle in both precisions, the engine, the yardstick per filter pooled over the items.
        -> (engine, [scores per filter], what ``oracle`` returned) for callers that compare further."""
        thr, keep, V64, V32 = self.oracle(filters, clip, R, volumes, exact_features)
        eng = eng or self.engine(filters[0], clip, thr, batch)
        assert eng.threshold == float(thr) or not self.has_clash
        got = []
        for k, filt in enumerate(filters):
            V = self.kernels(eng, filt, R, volumes, **batch_kw)
            got.append(V)
            yardstick("%s, filter %d" % (label, k) if len(filters) > 1 else label, V, V32[k], V64[k], keep)
        return eng, got, (thr, keep, V64, V32)

    def layout(self):
        return ("[%d @ %d, %d @ %d]" % (self.C, self.L, self.C1, self.L // 2)) if self.C1 else "%d @ %d" % (self.C, self.L)


# ----------------------------------------------------------------------------------------------------------------------
# section 3: cases through the fused engine
# ----------------------------------------------------------------------------------------------------------------------

def check_dense(lib, device, L, C, C1=0, nrot=2, seed=0, protein=False, expect_switches=None, label="", engine_kw=None, **batch_kw):
    """a. dense random volumes (or a protein-shaped, mostly zero ligand), oblique rotations, probe filters."""
    case = Case(lib, device, L, C, C1, seed=seed, **(engine_kw or {}))
    if protein:
        case.lig = protein_shaped(C, L, seed + 1)
        if C1:
            case.lig1 = protein_shaped(C1, L // 2, seed + 2, amp=0.2)
    R = rots(nrot, seed=seed + 5)
    eng, _, _ = case.run("%s, %s%s, probe" % (case.layout(), "protein-shaped ligand" if protein else "dense", label),
                         probe_filters(C + C1, probe_width(lib, L, C1), seed=seed), None, R=R, batch=min(nrot, 2), **batch_kw)
    if expect_switches is not None:
        expect_switches(eng.switches())
    return eng


def check_filter_and_clip(lib, device, L, C, C1=0, nrot=2, seed=0):
    """One ordinary random SimpleFilter (some units inactive), and the probe with the clip biting: clip near the RMS of the
    float64 correlations, chosen so that a third or more of them saturate (asserted on the float64 correlations)."""
    case = Case(lib, device, L, C, C1, seed=seed)
    R = rots(nrot, seed=seed + 7)
    H = max(2, (C + C1) // 2)
    filt = random_filter(C + C1, H, seed, dead=min(2, H - 1))
    # the inactive units are inactive: their pre-activation stays far below zero for correlations of this size
    case.run("%s, dense, random SimpleFilter, clip 5" % case.layout(), [filt], 5.0, R=R, batch=min(nrot, 2))
    Rb = torch.from_numpy(R[:1])
    corr = orc.correlate_fft(case.rec[None], orc.rotate_volume(case.lig[None], Rb, dtype=torch.float64), dtype=torch.float64)
    a = corr.abs().reshape(-1)
    clip = float(a.kthvalue(int(0.6 * a.numel())).values)               # the 60th percentile of |corr|: 0.6 - 0.8 of the RMS
    rms = float(torch.sqrt((corr * corr).mean()))
    assert 0.3 * rms < clip < 1.5 * rms, (clip, rms)
    sat = float((a >= clip).double().mean())
    assert sat >= 1.0 / 3.0, ("the clip does not bite", sat)
    case.run("%s, dense, probe, clip %.3g (%.0f %% saturated)" % (case.layout(), clip, 100 * sat), probe_filters(C + C1, probe_width(lib, L, C1), seed=seed),
             clip, R=R, batch=min(nrot, 2))


def check_impulses(lib, device, L, C, seed=0):
    """b. the volumes path (no rotation: the expectation is exact).  Ligand = unit impulses, receptor random:
    corr_c[t] = rec_c[b_c + t]; then impulse against impulse: 1 at (a - b) mod 2L, nothing elsewhere."""
    case = Case(lib, device, L, C, seed=seed)
    ligs, wheres = zip(*[impulses(C, L, first) for first in (0, 5)])
    vl = torch.stack(ligs)
    g = torch.Generator().manual_seed(seed + 3)
    vf = torch.rand(2, L, L, L, generator=g)
    filters = probe_filters(C, probe_width(lib, L), seed=seed)

    def exact(i):
        return torch.stack([shifted(case.rec[c], wheres[i][c]) for c in range(C)], dim=-1).reshape(-1, C)
    case.run("%s, impulse ligand, volumes path" % case.layout(), filters, None, volumes=(vl, vf, None), exact_features=exact)
    # impulse against impulse, no clash channel: the flat spectrum weighs every bin equally
    both = Case(lib, device, L, C, seed=seed, has_clash=False)
    both.rec, rwhere = impulses(C, L, 3)
    N = 2 * L

    def exact2(i):
        f = torch.zeros(N, N, N, C, dtype=torch.float64)
        for c in range(C):
            t = [(rwhere[c][a] - wheres[i][c][a]) % N for a in range(3)]
            f[t[0], t[1], t[2], c] = 1.0
        return f.reshape(-1, C)
    _, got, (_, _, V64, _) = both.run("%s, impulse x impulse, volumes path" % both.layout(), filters, None, volumes=(vl, None, None),
                                      exact_features=exact2)
    for V, want in zip(got, V64):
        peaks = want != 0
        assert bool(peaks.any()) and float((V[peaks].double() - want[peaks]).abs().max()) < 1e-5
        assert not bool(peaks.reshape(2, N, N, N)[:, L].any())          # (the planes |t| = L hold no peak and are under the bound)


def check_extreme_spectra(lib, device, L, C, seed=0):
    """c. constant, checkerboard, constant along z, constant along x -- through the volumes path, so that the structure
    reaches the transforms as it is."""
    case = Case(lib, device, L, C, seed=seed)
    g = torch.Generator().manual_seed(seed + 4)
    vl = torch.stack([extreme_ligands(C, L, seed + 10), extreme_ligands(C, L, seed + 11).roll(1, 0)])
    vf = torch.rand(2, L, L, L, generator=g)
    case.run("%s, constant / checkerboard / constant along z / along x" % case.layout(), probe_filters(C, probe_width(lib, L), seed=seed), None,
             volumes=(vl, vf, None))


def check_exact_rotations(lib, device, L, C, which, seed=0, launches=((),), engine_kw=None, C1=0):
    """d. signed permutation matrices through the fused K1: the rotated ligand is an exact index permutation, so
    score_batch(R) answers to float64 AND to score_batch(volumes = permuted ligand).  launches: score_batch switch sets."""
    case = Case(lib, device, L, C, C1, seed=seed, **(engine_kw or {}))
    R = signed_permutations()[list(which)]
    n = R.shape[0]
    vl = torch.stack([permuted(case.lig, R[i]) for i in range(n)])
    vf = torch.stack([permuted(case.ligf, R[i]) for i in range(n)])
    vc = torch.stack([permuted(case.lig1, R[i]) for i in range(n)]) if C1 else None
    for i in range(n):                      # the oracle's trilinear rotation gives the same permutation, exactly
        assert torch.equal(orc.rotate_volume(case.lig[None, :1], torch.from_numpy(R[i:i + 1]), dtype=torch.float64)[0].float(), vl[i, :1])
    filters = probe_filters(C + C1, probe_width(lib, L, C1), signs=1, seed=seed)
    eng, via_volumes, (thr, keep, V64, V32) = case.run("%s, signed permutations, volumes path" % case.layout(), filters, None,
                                                      volumes=(vl, vf, vc), batch=min(n, 4))
    for kw in launches:
        kw = dict(kw)
        tag = ", ".join(sorted(k for k, v in kw.items() if v)) or "default launch"
        for k, filt in enumerate(filters):
            V = case.kernels(eng, filt, R=R, **kw)
            yardstick("%s, signed permutations, fused K1 (%s), filter %d" % (case.layout(), tag, k), V, V32[k], V64[k], keep)
            # ... and against the volumes path: the same yardstick with the given-volumes scores as the expectation
            yardstick("%s, signed permutations, fused K1 (%s) vs volumes path, filter %d" % (case.layout(), tag, k), V,
                      V32[k], via_volumes[k], keep)
    return eng


def check_rotation_list(lib, device, label, R, seed=0):
    """A whole rotation set through ``search()`` at 4 @ 32 (so the grouping code -- slab orientation x gather layout --
    meets it) against the oracle's ranked list, as test_full_search_ranked_list_matches_oracle compares them."""
    from deeplocalproteindocking_amd.engine import DockingEngine
    L, C, K, thr = 32, 4, 100, 4000.0
    case = Case(lib, device, L, C, seed=seed, amp=0.1)
    W1, b1, W2, _ = random_filter(C, 2, seed, dead=0)
    # the best scores are the largest activations (W2 < 0, b2 = -1): distinct values, neither the zero-fill nor a plateau of
    # voxels whose hidden units are all inactive
    filt = (W1, b1, -W2.abs(), torch.tensor([-1.0]))
    eng = DockingEngine(L, C, *filt, clip=5.0, threshold_clash=thr, max_conf=K, batch=7, device=device, lib=lib)
    eng.set_receptor(case.rec, case.recf)
    eng.set_ligand(case.lig, case.ligf)
    eng.reset_top()
    eng.search(R)
    got = eng.top_list()
    want, Vs = orc.dock_volumes([case.rec[None]], [case.lig[None]], case.recf[None, None], case.ligf[None, None], R, *filt,
                                thr, K, clip=5.0, faithful_topk=False, return_V=True)
    band = 1e-4 * max(float(v.abs().max()) for v in Vs)
    assert len(got) == len(want) == K
    assert want[-1][4] < 0 and len({w[4] for w in want}) > K // 2, "the list must rank real scores, not the zero-fill"
    worst = max(abs(a[4] - b[4]) for a, b in zip(got, want))
    print("ACCURACY | %-58s | ranked list: worst score difference %.2e of the band, %d / %d poses identical" %
          (label, worst / band, sum(a[:4] == b[:4] for a, b in zip(got, want)), K), flush=True)
    assert worst <= band
    want_set, kth = {w[:4] for w in want}, want[-1][4]
    for a, b in zip(got, want):
        if a[:4] != b[:4]:
            assert abs(a[4] - b[4]) <= band and (a[:4] in want_set or abs(a[4] - kth) <= 2 * band)
    assert sum(a[:4] == b[:4] for a, b in zip(got, want)) >= int(0.97 * K)


def check_rotations(lib, device, L, C, R, label, C1=0, seed=0, ligand=None, engine_kw=None, launches=((),)):
    """e. / f. given rotation matrices (float64) on a dense pair, or on the ligand ``ligand(C, L, seed)`` builds."""
    case = Case(lib, device, L, C, C1, seed=seed, **(engine_kw or {}))
    if ligand is not None:
        case.lig, case.ligf = ligand(C, L, seed + 1), ligand(1, L, seed + 2)[0] / 64.0
        if C1:
            case.lig1 = ligand(C1, L // 2, seed + 3)
    filters = probe_filters(C + C1, probe_width(lib, L, C1), signs=1, seed=seed)
    eng, _, (thr, keep, V64, V32) = case.run("%s, %s%s" % (case.layout(), label, ", default launch" if len(launches) > 1 else ""),
                                            filters, None, R=R, batch=min(len(R), 4), **dict(launches[0]))
    for kw in launches[1:]:
        kw = dict(kw)
        tag = ", ".join(sorted(k for k, v in kw.items() if v))
        for k, filt in enumerate(filters):
            yardstick("%s, %s, %s, filter %d" % (case.layout(), label, tag, k), case.kernels(eng, filt, R=R, **kw), V32[k], V64[k], keep)


def check_unequal_scales(lib, device, L, C, probed, seed=0):
    """g. amplitudes from 1e-3 to 10 across the channels of one launch, clip off, one probed channel per run.  The yardstick
    holds for the errors pooled over the launch; per channel, max|e_k| / max|corr_c| is reported beside the oracle's."""
    case = Case(lib, device, L, C, seed=seed, amp=1.0)
    amps = torch.logspace(-3, 1, C)
    case.rec, case.lig = case.rec * 0.05, case.lig * amps[:, None, None, None]
    R = rots(1, seed=seed + 9)
    filters = [single_channel_probe(C, c) for c in probed]
    thr, keep, V64, V32 = case.oracle(filters, None, R=R)
    eng = case.engine(filters[0], None, thr, 1)
    got = [case.kernels(eng, f, R=R) for f in filters]
    rows = []
    for c, V, v32, v64 in zip(probed, got, V32, V64):
        scale = float(v64.abs().max())
        ek, eo = float((V.double() - v64)[keep].abs().max()) / scale, float((v32.double() - v64)[keep].abs().max()) / scale
        rows.append((c, float(amps[c]), ek, eo))
        print("ACCURACY | %s, channel %d of amplitude %.3g: max|e_k| / max|corr_c| %.2e, float32 oracle %.2e" %
              (case.layout(), c, float(amps[c]), ek, eo), flush=True)
    yardstick("%s, amplitudes 1e-3 .. 10, pooled over the launch" % case.layout(), torch.stack(got), torch.stack(V32),
              torch.stack(V64), torch.stack([keep] * len(probed)))
    return rows


# ----------------------------------------------------------------------------------------------------------------------
# section 4: stand-alone operators and the local path
# ----------------------------------------------------------------------------------------------------------------------

def check_volume_convolution(lib, device, L, C=2, embed=True, seed=0, inputs=None):
    """ops.VolumeConvolution on dense, impulse, impulse x impulse, spectrally extreme and face-mass inputs (``inputs``: the
    names of those to run, None: all five -- the largest boxes take three, the float64 transform on the host is what costs).

    The plan-free route (boxes without a compiled plan, embed=False) answers to a wider bound, by its formulation: every
    1-D transform there is a DIRECT sum (csrc/dlpd_generic.hip: O(n N), no radix plan) of n = L terms on the way in and
    n = N = 2L terms on the way back.  The rounding error of a float32 sum of n terms grows like sqrt(n) eps (a random walk
    of n roundings; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), that of an FFT like sqrt(log2 N) eps
    (one rounding per pass; Gentleman and Sande 1966): a direct transform may be sqrt(N / log2 N) further from the truth than
    the oracle's FFT -- 3.45 at box 37, 2.15 at box 10 -- and both margins are multiplied by exactly that.  (Measured on an
    MI355X at box 37: 1.6 RMS on dense input, 2.6 on impulse x impulse, whose error is all transform and no input; the
    oracle's own transform of length 74 = 2 x 37 holds a direct 37-point butterfly, so the full factor is not reached.)
    Those figures are of a single running sum per output.  At box 128 that missed the bound on impulse x impulse (11.49 RMS,
    19.58 max against 11.31 / 16.97): at the peak all 256 terms are in phase and the error of a running sum grows like
    n^1.5 eps, not like the random walk above.  The kernels now keep four partial sums per output (GEN_NACC)."""
    from deeplocalproteindocking_amd.ops import VolumeConvolution
    g = torch.Generator().manual_seed(seed)
    rec = torch.randn(C, L, L, L, generator=g)
    imp, where = impulses(C, L, 1)
    imp2, where2 = impulses(C, L, 4)
    route = "compiled" if lib_supports(lib, L) else ("embedded" if embed else "plan-free")
    conv = VolumeConvolution(clip=None, lib=lib, embed=embed)
    cases = [("dense", rec, torch.randn(C, L, L, L, generator=g), None),
             ("impulse ligand", rec, imp, torch.stack([shifted(rec[c], where[c]) for c in range(C)])),
             ("impulse x impulse", imp2, imp, None),
             ("extreme spectra", rec, extreme_ligands(C, L, seed + 1) * 10, None),
             ("mass on the faces", rec, face_mass(C, L, seed + 2), None)]
    assert inputs is None or set(inputs) <= {c[0] for c in cases}, inputs
    for name, v1, v2, exact in cases:
        if inputs is not None and name not in inputs:
            continue
        out = conv(v1[None].to(device), v2[None].to(device)).cpu()[0]
        x64 = orc.correlate_fft(v1[None], v2[None], dtype=torch.float64)[0]
        if exact is not None:
            assert float((x64 - exact).abs().max()) <= 1e-12 * float(exact.abs().max())
            x64 = exact
        if name == "impulse x impulse":
            N = 2 * L
            x64 = torch.zeros_like(x64)
            for c in range(C):
                x64[(c,) + tuple((where2[c][a] - where[c][a]) % N for a in range(3))] = 1.0
        growth = plan_free_growth(L) if route == "plan-free" else 1.0
        yardstick("VolumeConvolution box %d (%s), %s" % (L, route, name), out, orc.correlate_fft(v1[None], v2[None])[0], x64, growth=growth)


def plan_free_growth(L):
    """The formulation factor of the plan-free route at box L (derived in check_volume_convolution)."""
    return float(np.sqrt(2 * L / np.log2(2 * L)))


def check_plan_free_chunks(lib, device, L=128, C=12, seed=0):
    """ops._vc_generic keeps its scratch under 4 GB by taking the volumes in chunks: C volumes at a box where they exceed one
    chunk (asserted from the library's own workspace size).  The last channel is a copy of the first on both sides and lies
    behind the chunk boundary: its output must have the first's bytes (a chunk that read or wrote at the wrong volume
    offset cannot), and the first answers to float64 by the plan-free yardstick -- one transform on the host, not C."""
    from deeplocalproteindocking_amd._lib import get_lib
    from deeplocalproteindocking_amd.ops import VolumeConvolution
    per = (lib or get_lib()).call("dlpd_correlate_generic_ws_bytes", 1, int(L))
    assert C > (4 << 30) // per >= 1, ("the chunk loop must iterate twice", per, C)
    chunk = min((4 << 30) // per, 65535 // (2 * L))
    g = torch.Generator().manual_seed(seed)
    v1, v2 = torch.randn(1, C, L, L, L, generator=g), torch.randn(1, C, L, L, L, generator=g)
    v1[0, C - 1], v2[0, C - 1] = v1[0, 0], v2[0, 0]
    out = VolumeConvolution(clip=None, lib=lib, embed=False)(v1.to(device), v2.to(device))
    first, last, others = out[0, 0].cpu(), out[0, C - 1].cpu(), out[0, 1:C - 1].abs().amax(dim=(1, 2, 3)).cpu()
    del out
    assert first.numpy().tobytes() == last.numpy().tobytes(), "the volume behind the chunk boundary"
    assert bool((others > 0).all()) and bool(torch.isfinite(others).all())
    x64 = orc.correlate_fft(v1[:, :1], v2[:, :1], dtype=torch.float64)[0, 0]
    return yardstick("VolumeConvolution box %d (plan-free), %d volumes in chunks of %d, volume 0" % (L, C, chunk), first,
                     orc.correlate_fft(v1[:, :1], v2[:, :1])[0, 0], x64, growth=plan_free_growth(L))


def check_plan_free_clamp(lib, device, L=84, C=2, seed=0):
    """The clamp of the plan-free route is the last operation of its last kernel: with ``clip`` at the median of the
    unclipped |output| the clipped call equals torch.clamp of the unclipped one bit for bit, and about half the elements
    change."""
    from deeplocalproteindocking_amd.ops import VolumeConvolution
    g = torch.Generator().manual_seed(seed)
    v1, v2 = torch.randn(1, C, L, L, L, generator=g).to(device), torch.randn(1, C, L, L, L, generator=g).to(device)
    assert not lib_supports(lib, L)
    plain = VolumeConvolution(clip=None, lib=lib, embed=False)(v1, v2).cpu()
    clip = float(plain.abs().reshape(-1).median())
    clipped = VolumeConvolution(clip=clip, lib=lib, embed=False)(v1, v2).cpu()
    changed = float((clipped != plain).float().mean())
    print("ACCURACY | VolumeConvolution box %d (plan-free), clip %.4g: %.3f of the elements clamped" % (L, clip, changed), flush=True)
    assert clip > 0 and 0.3 <= changed <= 0.7, changed
    assert torch.equal(clipped, torch.clamp(plain, -clip, clip))


def lib_supports(lib, L):
    from deeplocalproteindocking_amd._lib import get_lib
    return bool((lib or get_lib()).call("dlpd_grid_supported", int(L)))


def check_volume_rotation(lib, device, L, C=3, seed=0):
    """ops.VolumeRotation: the 24 signed permutations are exact index permutations (bit for bit); oblique turns of a dense
    volume and near-lattice turns of mass on the faces answer to float64 by the yardstick."""
    from deeplocalproteindocking_amd.ops import VolumeRotation
    rot = VolumeRotation(lib=lib)
    g = torch.Generator().manual_seed(seed)
    vol = torch.randn(C, L, L, L, generator=g)
    P = signed_permutations()
    for beg in range(0, 24, 8):
        Rp = P[beg:beg + 8]
        out = rot(vol[None].repeat(8, 1, 1, 1, 1).to(device), torch.from_numpy(Rp).float().to(device).contiguous()).cpu()
        for i in range(8):
            assert torch.equal(out[i], permuted(vol, Rp[i])), ("signed permutation", beg + i)

    def turn(v, R, name):
        n = R.shape[0]
        Rt = torch.from_numpy(np.ascontiguousarray(R))
        out = rot(v[None].repeat(n, 1, 1, 1, 1).to(device), Rt.float().to(device).contiguous()).cpu()
        vb = v[None].repeat(n, 1, 1, 1, 1)
        yardstick("VolumeRotation box %d, %s" % (L, name), out, orc.rotate_volume(vb, Rt), orc.rotate_volume(vb, Rt, dtype=torch.float64))
    turn(vol, rots(2, seed=seed + 8), "dense, oblique")
    turn(face_mass(C, L, seed + 1), face_rotations(), "mass on the faces, 1e-4 / 1e-2 rad / quarter turn + 1e-4")


def check_local_window_is_the_receptor(lib, device, L, C, seed=0):
    """ops.local_correlate at radius 1 with an impulse ligand under signed permutations: every direct sum has one term, so
    the window equals the receptor's values bit for bit (zero where the index leaves the box)."""
    from deeplocalproteindocking_amd.ops import local_correlate
    g = torch.Generator().manual_seed(seed)
    rec = torch.randn(C, L, L, L, generator=g)
    lig, where = impulses(C, L, 8)                          # a face centre, the box centre, then corners
    P = signed_permutations()[[0, 5, 10, 13, 19, 23]]
    n = P.shape[0]
    T = torch.tensor([[0, 0, 0], [1, -2, 3], [-(L // 2), 1, 0], [L // 2 - 1, -1, -(L // 2)], [-1, -1, -1], [2, L // 2, -3]], dtype=torch.int32)
    out = local_correlate(rec.to(device), lig.to(device), T.to(device), R=torch.from_numpy(P).float().to(device).contiguous(),
                          radius=1, lib=lib).cpu()
    hits = 0
    for p in range(n):
        ligp = permuted(lig, P[p])
        for c in range(C):
            b = torch.nonzero(ligp[c])
            assert b.shape[0] <= 1                                   # (an impulse turned to index L has left the box)
            for d in itertools.product((-1, 0, 1), repeat=3):
                want = 0.0
                if b.shape[0]:
                    q = [int(b[0, a]) + int(T[p, a]) + d[a] for a in range(3)]
                    if all(0 <= x < L for x in q):
                        want = float(rec[c, q[0], q[1], q[2]])
                        hits += 1
                assert float(out[p, c, d[0] + 1, d[1] + 1, d[2] + 1]) == want, (p, c, d)
    assert hits >= 27 * n // 2                               # (the windows are not all outside the box)


# ----------------------------------------------------------------------------------------------------------------------
# section 5: the convolution kernel
# ----------------------------------------------------------------------------------------------------------------------

def conv_positions(D):
    """Corners, face centres, and both sides of the edges of the 4 x 4 patch and of the 16-voxel z tile."""
    m, e = D // 2, D - 1
    pos = [(0, 0, 0), (e, e, e), (0, e, 0), (e, 0, e), (0, m, m), (m, e, m), (m, m, 0), (m, m, e),
           (3, 4, 15), (4, 3, 16), (7, 8, 31), (8, 7, 32)]
    return [tuple(min(x, e) for x in p) for p in pos]


def check_conv3d_impulse_response(lib, device, cin, cout, ks, D, stride, precision, seed=0, positions=None):
    """Input = unit impulse in channel ci at p (one (ci, p) per batch item): y[co, p - k + ks // 2] = w[co, ci, k], zero
    elsewhere (stride 2: the even output positions) -- exactly for f32, to 2^-24 |w| per tap for split_bf16 (three bf16
    terms carry a float to that: test_three_bf16_terms_carry_a_float).  Every tap index and the padding, exactly."""
    from deeplocalproteindocking_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, ks, ks, ks, generator=g) * 0.1
    pos = conv_positions(D)
    pos = pos if positions is None else [pos[i] for i in positions]     # (the emulator takes a few of them)
    B, h = len(pos), ks // 2
    x = torch.zeros(B, cin, D, D, D)
    ci = [(3 * b + 1) % cin for b in range(B)]
    ci[0], ci[-1] = 0, cin - 1
    for b, p in enumerate(pos):
        x[b, ci[b]][p] = 1.0
    y = ops.conv3d(x.to(device), w.to(device), lib=lib, stride=stride, precision=precision).cpu()
    Do = (D - 1) // stride + 1
    want = torch.zeros(B, cout, Do, Do, Do)
    taps = 0
    for b, p in enumerate(pos):
        for k in itertools.product(range(ks), repeat=3):
            q = [p[a] - k[a] + h for a in range(3)]
            if all(0 <= v < D and v % stride == 0 for v in q):
                want[b, :, q[0] // stride, q[1] // stride, q[2] // stride] = w[:, ci[b], k[0], k[1], k[2]]
                taps += 1
    assert y.shape == want.shape and taps > 0
    if precision == "f32":
        assert torch.equal(y, want), float((y - want).abs().max())
    else:
        assert bool(((y - want).abs().double() <= 2.0 ** -24 * want.abs().double()).all()), \
            float(((y - want).abs().double() - 2.0 ** -24 * want.abs().double()).max())


def check_conv3d_yardstick(lib, device, cin, cout, ks, D, stride, precisions=("f32", "split_bf16"), seed=0):
    """randn input, and non-negative (post-ReLU-like) input: torch's float32 conv3d is X32, its float64 X64."""
    from deeplocalproteindocking_amd import ops
    g = torch.Generator().manual_seed(seed + 1)
    w = torch.randn(cout, cin, ks, ks, ks, generator=g) * 0.1
    for name, x in (("randn", torch.randn(1, cin, D, D, D, generator=g)), ("non-negative", torch.relu(torch.randn(1, cin, D, D, D, generator=g)))):
        x32 = torch.nn.functional.conv3d(x, w, padding=ks // 2, stride=stride)
        x64 = torch.nn.functional.conv3d(x.double(), w.double(), padding=ks // 2, stride=stride)
        for precision in precisions:
            y = ops.conv3d(x.to(device), w.to(device), lib=lib, stride=stride, precision=precision).cpu()
            yardstick("conv3d %s %d -> %d, k %d, D %d, stride %d, %s" % (precision, cin, cout, ks, D, stride, name), y, x32, x64)
