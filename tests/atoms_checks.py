"""Check bodies shared by tests/test_atoms_proj_gpu.py (the gfx950 build) and tests/test_atoms_proj_emu.py (the same kernel
sources on the fibre emulator): the atom projection of csrc/dlpd_atoms.hip -- k_project_atoms and the cell-wise path
(k_mark_atom_cells, k_marked_cells<0/1>) -- against float64, at box edges, odd boxes and non-default splats.

The yardstick.  X64 is oracle.docking_oracle.project_atoms (float64 throughout).  X32 is ``splat32`` below: the same formula
-- p = R x + s, floor(p / res - voff), exp(-d^2 / (2 sigma^2)) -- rounded to float32 at every operation, summed in float32;
it also returns n_v, the number of contributions each voxel received.  The kernel's documented contract is that every
contribution is rounded to a multiple of 2^-22, an error of at most 2^-23 each, so per case

    per voxel    |X - X64| <= 3 max|X32 - X64| + n_v 2^-23
    all voxels   rms(max(|X - X64| - n_v 2^-23, 0)) <= 2 rms(X32 - X64)

The margins 2 and 3 are those of tests/accuracy_checks.py; the bound comes from X32, never from the kernel.  Every check
prints its ratios (EXPERIMENTS.md, section ACCURACY holds the values of an MI355X).

The density is discontinuous where q = p' / res - voff crosses an integer (the window moves by a voxel), so the random cases
are redrawn until every q, computed in float64, is at least 1e-3 from an integer: float32 and float64 then bin every atom
alike and NO voxel is left out of a comparison.  The positions the random cases avoid -- q exactly integer, on the faces, one
voxel inside and outside the reach of the window -- are taken by ``check_exact_edges`` with dyadic inputs, where float32 is
exact.  Nothing here reads the reference tree."""
import functools

import numpy as np
import pytest
import torch

import accuracy_checks as acc
from oracle import docking_oracle as orc
from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend, NUM_ATOM_TYPES

T = NUM_ATOM_TYPES
STEP = 2.0 ** -23                      # the largest rounding error of one contribution (a multiple of 2^-22)
SCALE = 2.0 ** 22
PADDING = 7                            # NaN slots behind the atoms of every row
CLEAR = 1e-3                           # distance every q keeps from an integer in the random cases

# L, res, sigma, window, voxel_offset, norm, atoms, rotations -- the smallest shapes at which each edge exists
CASES = [
    dict(L=13, res=1.25, sigma=1.0, window=2, voxel_offset=0.0, norm=1.0, atoms=60, nrot=2),
    dict(L=11, res=1.0, sigma=0.8, window=3, voxel_offset=0.5, norm=1.5, atoms=80, nrot=2, empty_types=(0, 10)),
    dict(L=9, res=1.25, sigma=1.6, window=6, voxel_offset=0.5, norm=4.0, atoms=30, nrot=1),
    dict(L=6, res=2.0, sigma=0.5, window=0, voxel_offset=0.0, norm=1.0, atoms=50, nrot=2),
    dict(L=3, res=1.0, sigma=1.0, window=1, voxel_offset=0.25, norm=0.3, atoms=40, nrot=1),
]
CASE_IDS = ["L%d-w%d" % (c["L"], c["window"]) for c in CASES]


def splat_of(case):
    return {k: case[k] for k in ("sigma", "window", "voxel_offset", "norm")}


# ----------------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------------

def splat32(xyz, types, L, res, R=None, shift=None, sigma=1.0, window=2, voxel_offset=0.0, norm=1.0, sum_types=False,
            dtype=np.float32):
    """X32: the projection of atoms ``xyz`` (n, 3) of types ``types`` (n,), every operation rounded to ``dtype``.
    -> (volume (T or 1, L, L, L) in ``dtype``, n_v int64 of the same shape).  (dtype=float64 restates the oracle: the
    checks pin the two against each other, so that X32 differs from X64 by its rounding alone.)"""
    f = dtype
    xyz = np.asarray(xyz, dtype=f).reshape(-1, 3)
    types = np.asarray(types, dtype=np.int64)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if R is not None:
        r = np.asarray(R, dtype=f).reshape(9)
        x, y, z = ((r[0] * x + r[1] * y) + r[2] * z, (r[3] * x + r[4] * y) + r[5] * z, (r[6] * x + r[7] * y) + r[8] * z)
    s = np.zeros(3, dtype=f) if shift is None else np.asarray(shift, dtype=f).reshape(3)
    p = np.stack([x + s[0], y + s[1], z + s[2]], axis=1).astype(f)
    res, voff, nrm = f(res), f(voxel_offset), f(norm)
    inv2s2 = f(0.5) / (f(sigma) * f(sigma))
    c = np.floor(p / res - voff).astype(np.int64)
    off = np.arange(-int(window), int(window) + 1)
    di, dj, dk = (a.reshape(-1) for a in np.meshgrid(off, off, off, indexing="ij"))
    i, j, k = c[:, 0:1] + di[None], c[:, 1:2] + dj[None], c[:, 2:3] + dk[None]
    ok = (i >= 0) & (i < L) & (j >= 0) & (j < L) & (k >= 0) & (k < L)
    dx = p[:, 0:1] - (i.astype(f) + voff) * res
    dy = p[:, 1:2] - (j.astype(f) + voff) * res
    dz = p[:, 2:3] - (k.astype(f) + voff) * res
    assert dx.dtype == f
    w = nrm * np.exp(-inv2s2 * ((dx * dx + dy * dy) + dz * dz))
    assert w.dtype == f
    nch = 1 if sum_types else T
    ch = np.zeros_like(i) if sum_types else np.broadcast_to(types[:, None], i.shape)
    flat = ((ch * L + i) * L + j) * L + k
    vol, n_v = np.zeros(nch * L ** 3, dtype=f), np.zeros(nch * L ** 3, dtype=np.int64)
    np.add.at(vol, flat[ok], w[ok])                    # (one rounded addition per contribution, in atom order)
    np.add.at(n_v, flat[ok], 1)
    return vol.reshape(nch, L, L, L), n_v.reshape(nch, L, L, L)


def oracle64(row, L, res, R=None, shift=None, **splat):
    """X64 of one row (see ``Row``): the oracle's per-atom loop."""
    return orc.project_atoms(row.coords.astype(np.float64), row.counts, row.offsets, L, res,
                             R=None if R is None else np.asarray(R, dtype=np.float64),
                             shift=None if shift is None else np.asarray(shift, dtype=np.float64), **splat)


class Row:
    """One protein as the kernel takes it: float32 coordinates ordered by type in ``stride`` slots, the slots behind the
    atoms filled with NaN, counts and offsets per type."""

    def __init__(self, xyz, types, stride=None):
        xyz, types = np.asarray(xyz, dtype=np.float32).reshape(-1, 3), np.asarray(types, dtype=np.int64)
        order = np.argsort(types, kind="stable")
        self.xyz, self.types, self.n = xyz[order], types[order], len(types)
        self.stride = self.n + PADDING if stride is None else stride
        assert self.stride >= self.n
        self.coords = np.full(3 * self.stride, np.nan, dtype=np.float32)
        self.coords[:3 * self.n] = self.xyz.reshape(-1)
        self.counts = np.bincount(self.types, minlength=T).astype(np.int32)
        self.offsets = (np.cumsum(self.counts) - self.counts).astype(np.int32)

    def widened(self, stride):
        return Row(self.xyz, self.types, stride)


def tensors(rows, device):
    """-> coords (B, 3 * stride) f32, counts (B, T) i32, offsets (B, T) i32 on ``device``."""
    assert len({r.stride for r in rows}) == 1
    return (torch.from_numpy(np.stack([r.coords for r in rows])).to(device),
            torch.from_numpy(np.stack([r.counts for r in rows])).to(device),
            torch.from_numpy(np.stack([r.offsets for r in rows])).to(device))


def q_of(xyz, L, res, voff, R=None, shift=None):
    """q = p' / res - voff in float64 for float32 inputs (n, 3)."""
    p = np.asarray(xyz, dtype=np.float64)
    if R is not None:
        p = p @ np.asarray(R, dtype=np.float64).T
    if shift is not None:
        p = p + np.asarray(shift, dtype=np.float64)
    return p / res - voff


def clear_of_bins(q):
    return bool((np.abs(q - np.rint(q)) >= CLEAR).all())


def coverage(q, L, w):
    """What a set of atoms (q float64 (n, 3)) exercises.  -> (faces, outside): ``faces`` the set of (axis, side) whose face a
    CONTRIBUTING atom's window crosses (clipped there), ``outside`` the number of atoms whose window misses the box.  A window
    of 0 is a single voxel and cannot be clipped: there a face counts when one atom lies in its layer of voxels and another
    one voxel outside it (inside the box along the other two axes)."""
    c = np.floor(q).astype(np.int64)
    inside = (c + w >= 0) & (c - w < L)                         # per axis: the window meets the box
    contrib = inside.all(axis=1)
    faces = set()
    for a in range(3):
        others = np.delete(inside, a, axis=1).all(axis=1)
        for side, lo in ((0, True), (1, False)):
            if w > 0:
                hit = contrib & ((c[:, a] - w < 0) if lo else (c[:, a] + w >= L))
                if hit.any():
                    faces.add((a, side))
            else:
                layer, beyond = (0, -1) if lo else (L - 1, L)
                if (others & (c[:, a] == layer)).any() and (others & (c[:, a] == beyond)).any():
                    faces.add((a, side))
    return faces, int((~contrib).sum())


ALL_FACES = {(a, s) for a in range(3) for s in (0, 1)}


@functools.lru_cache(maxsize=None)
def random_case(index):
    """Inputs and both references of CASES[index], made once per process and shared (read-only) by the tests that use them.
    Atoms uniform over [-0.15, 1.15] L res per axis, random types, turned about the box centre by oblique rotations; coordinates
    and R rounded to float32 before either reference sees them; redrawn until every q is CLEAR of an integer and the atoms
    cover what ``check_yardstick`` asserts.  The last two of the atoms are OUTLIERS: 130 % of the box reaches 0.15 L voxels
    past a face (1.35 at box 9, 0.45 at box 3), less than the window there, so no uniform draw lies wholly outside the box at
    those shapes; the outliers do, under the first rotation, by less than a voxel -- one below and one above the box."""
    case = CASES[index]
    L, res, w, voff, n, nrot = case["L"], case["res"], case["window"], case["voxel_offset"], case["atoms"], case["nrot"]
    R = acc.rots(nrot, seed=40 + index).astype(np.float32)
    centre = np.full(3, np.float32(L * res / 2.0), dtype=np.float32)
    allowed = [t for t in range(T) if t not in case.get("empty_types", ())]
    for draw in range(2000):
        rng = np.random.RandomState(1000 * index + draw)
        xyz = rng.uniform(-0.15, 1.15, size=(n, 3)) * L * res - centre.astype(np.float64)
        for slot, q_out in ((n - 2, -w - 1 + rng.uniform(0.1, 0.9)), (n - 1, L + w + rng.uniform(0.1, 0.9))):
            p = xyz[slot] + centre                                       # the outliers: beyond the reach of the window
            p[rng.randint(3)] = (q_out + voff) * res                     # under the first rotation, low and high side
            xyz[slot] = (p - centre) @ R[0].astype(np.float64)
        xyz = xyz.astype(np.float32)
        types = np.asarray(allowed)[rng.randint(len(allowed), size=n)]
        qs = [q_of(xyz, L, res, voff, R[b], centre) for b in range(nrot)]
        if not all(clear_of_bins(q) for q in qs):
            continue
        faces, outside = coverage(np.concatenate(qs), L, w)
        if faces == ALL_FACES and outside > 0:
            break
    else:
        raise AssertionError("no admissible draw for case %d" % index)
    row = Row(xyz, types)
    splat = splat_of(case)
    x64 = np.stack([oracle64(row, L, res, R[b], centre, **splat) for b in range(nrot)])
    both = [splat32(row.xyz, row.types, L, res, R[b], centre, **splat) for b in range(nrot)]
    x32, n_v = np.stack([v for v, _ in both]), np.stack([m for _, m in both])
    # the restatement IS the oracle's formula: in float64 it gives the oracle's values and the same contributions per voxel
    for b in range(nrot):
        v, m = splat32(row.xyz, row.types, L, res, R[b], centre, dtype=np.float64, **splat)
        assert np.abs(v - x64[b]).max() <= 1e-12 * max(1.0, x64[b].max()) and np.array_equal(m, n_v[b])
    for a in (x64, x32, n_v, R, centre):
        a.setflags(write=False)
    return dict(case=case, row=row, R=R, shift=centre, qs=qs, x64=x64, x32=x32, n_v=n_v, draw=draw)


# ----------------------------------------------------------------------------------------------------------------------
# the bound
# ----------------------------------------------------------------------------------------------------------------------

def bound(label, X, X32, X64, n_v, keep=None):
    """Assert both inequalities of the module docstring over the voxels ``keep`` (all if None); print the figures first."""
    X, X32, X64 = (np.asarray(t, dtype=np.float64).reshape(-1) for t in (X, X32, X64))
    n_v = np.asarray(n_v, dtype=np.float64).reshape(-1)
    assert X.shape == X32.shape == X64.shape == n_v.shape, (label, X.shape, X32.shape, X64.shape, n_v.shape)
    if keep is not None:
        keep = np.asarray(keep, dtype=bool).reshape(-1)
        X, X32, X64, n_v = X[keep], X32[keep], X64[keep], n_v[keep]
    assert np.isfinite(X).all(), (label, "non-finite values among the compared voxels", int((~np.isfinite(X)).sum()))
    ek, eo = np.abs(X - X64), np.abs(X32 - X64)
    slack = n_v * STEP
    over = np.maximum(ek - slack, 0.0)
    mo, ro = float(eo.max()), float(np.sqrt((eo * eo).mean()))
    rk, rk_raw = float(np.sqrt((over * over).mean())), float(np.sqrt((ek * ek).mean()))
    worst = float((over / mo).max()) if mo > 0 else float("inf")
    scale = float(np.abs(X64).max())
    print("ACCURACY | %-58s | rms %.3f | max %.3f | without the 2^-23 term: rms %.3f max %.3f | max|e_k|/max|X64| %.2e | oracle32 %.2e" %
          (label, rk / ro if ro > 0 else float("inf"), worst, rk_raw / ro if ro > 0 else float("inf"),
           float(ek.max()) / mo if mo > 0 else float("inf"), float(ek.max()) / scale if scale > 0 else float(ek.max()),
           mo / scale if scale > 0 else mo), flush=True)
    assert mo > 0 and ro > 0, (label, "the float32 oracle has no error here: the case measures nothing")
    bad = ek > acc.MAX_MARGIN * mo + slack
    assert not bad.any(), (label, "max", int(bad.sum()), float(ek[bad].max()), mo)
    assert rk <= acc.RMS_MARGIN * ro, (label, "rms", rk, ro, rk / ro)
    return rk / ro, worst


# ----------------------------------------------------------------------------------------------------------------------
# running the kernels
# ----------------------------------------------------------------------------------------------------------------------

class nan_prefill:
    """Inside the block every floating-point torch.empty comes back full of NaN: CoordsBackend.project allocates its output
    with torch.empty, and what the cell-wise path does not write must still hold the NaN afterwards."""

    def __enter__(self):
        self.orig = orig = torch.empty

        def nan_empty(*a, **kw):
            t = orig(*a, **kw)
            return t.fill_(float("nan")) if t.is_floating_point() else t
        torch.empty = nan_empty

    def __exit__(self, *exc):
        torch.empty = self.orig


def project(lib, device, rows, L, res, splat, R=None, shift=None, cells=False, sum_types=False):
    """CoordsBackend.project of ``rows`` -> (volumes on the CPU as numpy, map (B, nc, nc, nc) uint8 or None); the cell-wise call
    runs with NaN-prefilled buffers."""
    be = CoordsBackend(lib=lib, splat=splat)
    c, nt, of = tensors(rows, device)
    Rt = None if R is None else torch.from_numpy(np.array(R, dtype=np.float32)).to(device)
    sh = None if shift is None else torch.from_numpy(np.array(shift, dtype=np.float32))
    if not cells:
        return be.project(c, nt, of, L, res, device, R=Rt, shift=sh, sum_types=sum_types).cpu().numpy(), None
    with nan_prefill():
        out = be.project(c, nt, of, L, res, device, R=Rt, shift=sh, cells=True)
    assert out.dlpd_unwritten
    return out.cpu().numpy(), out.dlpd_occupancy.cpu().numpy()


def live_voxels(occ, L, nch=T):
    """The voxel mask (B, nch, L, L, L) of a cell map (B, nc, nc, nc)."""
    m = np.asarray(occ).astype(bool).repeat(4, 1).repeat(4, 2).repeat(4, 3)[:, None, :L, :L, :L]
    return np.broadcast_to(m, (m.shape[0], nch, L, L, L))


def cellwise_agrees(label, sparse, occ, dense, x64, L):
    """The cell-wise contract: X64 is zero wherever the map is clear, the NaN-prefilled buffer still holds NaN there, and where
    the map is set the values are the dense path's bits.  -> the voxel mask."""
    nc = (L + 3) // 4
    assert occ.shape == (sparse.shape[0], nc, nc, nc) and set(np.unique(occ).tolist()) <= {0, 1}, (label, occ.shape)
    live = live_voxels(occ, L, sparse.shape[1])
    assert (np.asarray(x64)[~live] == 0).all(), (label, "the map leaves out a voxel that holds density")
    assert np.isnan(sparse[~live]).all(), (label, "written outside the map")
    if dense is not None:
        assert sparse[live].tobytes() == dense[live].tobytes(), (label, "cell-wise and dense values differ")
        assert (dense[~live] == 0).all(), label
    return live


# ----------------------------------------------------------------------------------------------------------------------
# 1. yardstick cases
# ----------------------------------------------------------------------------------------------------------------------

def check_yardstick(lib, device, index, cells):
    d = random_case(index)
    case, row = d["case"], d["row"]
    L, res, w = case["L"], case["res"], case["window"]
    # coverage, asserted on the float64 positions: a clipped window at each of the six faces, an atom wholly outside, types
    # 0 and 10 empty where the case says so, padding present, an oblique rotation, and a float32 oracle that errs
    assert all(clear_of_bins(q) for q in d["qs"])
    faces, outside = coverage(np.concatenate(d["qs"]), L, w)
    assert faces == ALL_FACES and outside >= 1, (faces, outside)
    assert row.stride == row.n + PADDING and np.isnan(row.coords[3 * row.n:]).all()
    for t in case.get("empty_types", ()):
        assert row.counts[t] == 0
    assert np.abs(d["R"]).max() < 0.999, "oblique rotations: no axis stays an axis"
    assert np.abs(d["x32"] - d["x64"]).max() > 0
    label = "projection L %d res %.4g sigma %.2g window %d voff %.2g norm %.2g, %s" % (
        L, res, case["sigma"], w, case["voxel_offset"], case["norm"], "cell-wise" if cells else "dense")
    X, occ = project(lib, device, [row], L, res, splat_of(case), R=d["R"], shift=d["shift"], cells=cells)
    assert X.shape == d["x64"].shape
    keep = None
    if cells:
        keep = cellwise_agrees(label, X, occ, None, d["x64"], L)
        assert 0 < int(occ.sum())
    return bound(label, X, d["x32"], d["x64"], d["n_v"], keep)


# ----------------------------------------------------------------------------------------------------------------------
# 2. exact edges
# ----------------------------------------------------------------------------------------------------------------------

# L, window, res, voxel_offset, sigma: both resolutions with both offsets, boxes that are no multiple of 4; sigma 1.5 beside
# window 3 keeps the far corner of a half-integer atom's window (3.5 voxels away per axis) above one accumulator step
EDGE_CASES = [(7, 2, 1.0, 0.0, 1.0), (7, 2, 1.25, 0.5, 1.0), (5, 1, 1.25, 0.0, 1.0), (6, 3, 1.0, 0.5, 1.5)]


def edge_atoms(L, w):
    """-> list of q (3 integers or half-integers per atom): the voxel centre in the middle of the box; per axis the faces
    (0 and L) and the four off-by-one places (-w: one plane, -w - 1: nothing, L + w - 1: one plane, L + w: nothing), the
    other two axes on the middle voxel; the eight corners of the box and the eight places whose window holds one corner
    voxel; two atoms half-way between voxel centres, one of them at a face."""
    m = L // 2
    out = [(m, m, m)]
    for a in range(3):
        for v in (-w - 1, -w, 0, L, L + w - 1, L + w):
            q = [m, m, m]
            q[a] = v
            out.append(tuple(q))
    out += [(x, y, z) for x in (0, L) for y in (0, L) for z in (0, L)]
    out += [(x, y, z) for x in (-w, L + w - 1) for y in (-w, L + w - 1) for z in (-w, L + w - 1)]
    out += [(m + 0.5, 0.5, L - 0.5), (-0.5, m - 0.5, m + 0.5)]
    return out


def check_exact_edges(lib, device, L, w, res, voff, sigma=1.0):
    """Every atom alone in a channel of its own ((row, type), 11 per row), every row turned by another signed permutation
    about a dyadic pivot: p' = R x + s is exact in float32, q is an integer or a half-integer."""
    qs = np.asarray(edge_atoms(L, w), dtype=np.float64)
    n = len(qs)
    B = (n + T - 1) // T
    P = acc.signed_permutations()[[1, 5, 10, 14, 19, 23][:B]]
    shift = np.full(3, L * res / 2.0)
    target = (qs + voff) * res                                           # p', dyadic
    assert (target * 64 == np.rint(target * 64)).all() and (shift * 64 == np.rint(shift * 64)).all()
    splat = dict(sigma=sigma, window=w, voxel_offset=voff, norm=1.0)
    rows, where = [], []
    for b in range(B):
        idx = np.arange(b * T, min((b + 1) * T, n))
        x = (target[idx] - shift) @ P[b]                                 # R^T (p' - s): a signed permutation of dyadics
        assert np.array_equal(q_of(x.astype(np.float32), L, res, voff, P[b], shift), qs[idx])
        rows.append(Row(x, np.arange(len(idx)), stride=T + PADDING))
        where += [(b, t) for t in range(len(idx))]
    x64 = np.stack([oracle64(r, L, res, P[b], shift, **splat) for b, r in enumerate(rows)])
    both = [splat32(r.xyz, r.types, L, res, P[b], shift, **splat) for b, r in enumerate(rows)]
    x32, n_v = np.stack([v for v, _ in both]), np.stack([m for _, m in both])
    # the expectation itself, from integers: an atom at q touches the voxels floor(q) - w .. floor(q) + w inside the box, each
    # once -- one plane at -w and L + w - 1, nothing at -w - 1 and L + w -- and every value is at least one accumulator step
    c = np.floor(qs).astype(int)
    for (b, t), ci, q in zip(where, c, qs):
        lo, hi = np.maximum(ci - w, 0), np.minimum(ci + w + 1, L)
        box = np.zeros((L, L, L), dtype=bool)
        if (hi > lo).all():
            box[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        assert np.array_equal(x64[b, t] != 0, box) and np.array_equal(n_v[b, t] == 1, box), (b, t, q)
        for a in range(3):
            planes = {-w - 1: 0, -w: 1, L + w - 1: 1, L + w: 0}
            if q[a] in planes and all(0 <= q[o] < L for o in range(3) if o != a):
                assert np.any(box, axis=tuple(o for o in range(3) if o != a)).sum() == planes[q[a]], (q, a)
    assert x64[x64 != 0].min() > 2.0 ** -22
    label = "exact edges L %d window %d res %.4g voff %.2g" % (L, w, res, voff)
    dense, _ = project(lib, device, rows, L, res, splat, R=P, shift=shift)
    sparse, occ = project(lib, device, rows, L, res, splat, R=P, shift=shift, cells=True)
    assert np.array_equal(dense != 0, x64 != 0), (label, "the set of non-zero voxels", np.argwhere((dense != 0) != (x64 != 0))[:5])
    bound(label + ", dense", dense, x32, x64, n_v)
    centres = 0
    for (b, t), q in zip(where, qs):
        if (q == np.rint(q)).all() and (q >= 0).all() and (q < L).all():
            i, j, k = (int(v) for v in q)
            assert dense[b, t, i, j, k] == np.float32(1.0), (label, "an atom on a voxel centre", q, dense[b, t, i, j, k])
            centres += 1
    assert centres >= 1 + 3 + 1                      # the middle, q = 0 per axis, the corner (0, 0, 0)
    # the cell map: exactly the cells that hold a non-zero voxel of X64 (every window voxel is non-zero, asserted above)
    nc = (L + 3) // 4
    pad = np.zeros((len(rows), 4 * nc, 4 * nc, 4 * nc), dtype=bool)
    pad[:, :L, :L, :L] = (x64 != 0).any(axis=1)
    want_occ = pad.reshape(len(rows), nc, 4, nc, 4, nc, 4).any(axis=(2, 4, 6))
    assert np.array_equal(occ.astype(bool), want_occ), (label, "the cell map")
    live = cellwise_agrees(label, sparse, occ, dense, x64, L)
    assert np.array_equal((sparse != 0) & live, x64 != 0)
    bound(label + ", cell-wise", sparse, x32, x64, n_v, live)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the type sum
# ----------------------------------------------------------------------------------------------------------------------

def check_type_sum(lib, device, index):
    """project(sum_types=True) adds all types into one integer accumulator; integer adds commute, so while every per-type
    density stays below 4 (accumulator below 2^24: its float conversion is exact, and rint(vol_t 2^22) recovers it) the sum
    equals float32(sum_t rint(vol_t 2^22)) 2^-22 bit for bit.  At 4 and above the per-type conversion rounds and it cannot."""
    d = random_case(index)
    case, row = d["case"], d["row"]
    assert d["x64"].max() < 3.9, "this identity needs per-type densities below 4"
    args = (lib, device, [row], case["L"], case["res"], splat_of(case))
    per_type, _ = project(*args, R=d["R"], shift=d["shift"])
    assert per_type.max() < 4.0
    summed, _ = project(*args, R=d["R"], shift=d["shift"], sum_types=True)
    fixed = np.rint(per_type.astype(np.float64) * SCALE)
    assert np.array_equal(fixed / SCALE, per_type.astype(np.float64))
    want = (fixed.astype(np.int64).sum(axis=1).astype(np.float32) * np.float32(1.0 / SCALE))
    assert summed.shape == (d["R"].shape[0], 1) + per_type.shape[2:]
    assert summed[:, 0].tobytes() == want.tobytes(), float(np.abs(summed[:, 0] - want).max())
    assert ((per_type > 0).sum(axis=1) >= 2).any()                   # (several types meet in a voxel)


# ----------------------------------------------------------------------------------------------------------------------
# 4. batches
# ----------------------------------------------------------------------------------------------------------------------

BATCH_L, BATCH_RES = 10, 1.25
BATCH_SPLAT = dict(sigma=0.9, window=2, voxel_offset=0.5, norm=1.0)


def _positions(n, seed, L, res, voff, R=None, shift=None):
    """n float32 positions over [-0.15, 1.15] L res whose q (under every R) is CLEAR of an integer."""
    for draw in range(2000):
        rng = np.random.RandomState(seed + 7919 * draw)
        xyz = (rng.uniform(-0.15, 1.15, size=(n, 3)) * L * res).astype(np.float32)
        if shift is not None:
            xyz = (xyz - np.asarray(shift, dtype=np.float32)).astype(np.float32)
        if all(clear_of_bins(q_of(xyz, L, res, voff, r, shift)) for r in ([None] if R is None else R)):
            return xyz, rng.randint(T, size=n)
    raise AssertionError("no admissible draw")


def check_distinct_proteins(lib, device):
    """Three proteins in one call without R, as LocalTrainer projects them: 41 atoms, 5 atoms, and an empty row (all counts
    zero); per-row counts and offsets, NaN in every unused slot."""
    L, res, splat = BATCH_L, BATCH_RES, BATCH_SPLAT
    stride = 41 + PADDING
    big, small = (Row(*_positions(n, seed, L, res, splat["voxel_offset"]), stride=stride) for n, seed in ((41, 5), (5, 6)))
    empty = Row(np.zeros((0, 3)), np.zeros(0, dtype=np.int64), stride=stride)
    rows = [big, small, empty]
    assert empty.counts.sum() == 0 and np.isnan(empty.coords).all() and np.isnan(small.coords[15:]).all()
    assert not np.array_equal(big.offsets, small.offsets)
    dense, _ = project(lib, device, rows, L, res, splat)
    sparse, occ = project(lib, device, rows, L, res, splat, cells=True)
    x64 = np.stack([oracle64(r, L, res, **splat) for r in rows])
    cellwise_agrees("distinct proteins", sparse, occ, dense, x64, L)
    for b, r in enumerate(rows):
        alone, _ = project(lib, device, [r], L, res, splat)
        assert dense[b].tobytes() == alone[0].tobytes(), ("row %d differs from the same protein projected alone" % b)
        alone_s, alone_occ = project(lib, device, [r], L, res, splat, cells=True)
        assert np.array_equal(occ[b], alone_occ[0])
        if r.n:
            x32, n_v = splat32(r.xyz, r.types, L, res, **splat)
            bound("distinct proteins, row %d (%d atoms), dense" % (b, r.n), dense[b], x32, x64[b], n_v)
            bound("distinct proteins, row %d (%d atoms), cell-wise" % (b, r.n), sparse[b], x32, x64[b], n_v, live_voxels(occ[b:b + 1], L)[0])
    assert (dense[2] == 0).all() and not occ[2].any() and np.isnan(sparse[2]).all()
    assert occ[0].any() and occ[1].any()


def check_repeated_rotation(lib, device):
    """One protein under five rotations, the first and the fourth equal: rows 0 and 3 carry the same bits."""
    L, res, splat = BATCH_L, BATCH_RES, BATCH_SPLAT
    R = acc.rots(5, seed=71).astype(np.float32)
    R[3] = R[0]
    shift = np.full(3, L * res / 2.0, dtype=np.float32)
    row = Row(*_positions(41, 8, L, res, splat["voxel_offset"], R, shift))
    dense, _ = project(lib, device, [row], L, res, splat, R=R, shift=shift)
    sparse, occ = project(lib, device, [row], L, res, splat, R=R, shift=shift, cells=True)
    assert dense.shape[0] == 5 and dense[0].tobytes() == dense[3].tobytes() and dense[0].any()
    assert np.array_equal(occ[0], occ[3]) and occ[0].any()
    live = live_voxels(occ, L)
    assert sparse[0][live[0]].tobytes() == sparse[3][live[3]].tobytes()
    assert sparse[live].tobytes() == dense[live].tobytes() and np.isnan(sparse[~live]).all()
    assert dense[0].tobytes() != dense[1].tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# 5. the second trip of the capped loop
# ----------------------------------------------------------------------------------------------------------------------

def check_second_trip(lib, device, L=128, B=5):
    """k_marked_cells is launched with at most 32768 blocks of 256 threads, 131072 cells per trip of its grid-stride loop.
    ntypes 1, box 128, five rows: 5 * 32768 cells, and row 4 is exactly the second trip.  A dozen atoms in rows 0 and 4 near
    the low and the high corner; through the C ABI, into NaN-prefilled buffers."""
    from deeplocalproteindocking_amd.engine import _ptr, _stream
    device = torch.device(device)
    nc = (L + 3) // 4
    assert B * nc ** 3 > 131072 and (B - 1) * nc ** 3 == 131072
    res, n = 1.25, 12
    rng = np.random.RandomState(3)
    lo, hi = rng.uniform(-1.0, 9.0, size=(n // 2, 3)), rng.uniform(L * res - 9.0, L * res + 1.0, size=(n // 2, 3))
    xyz = np.concatenate([lo, hi]).astype(np.float32)
    coords = np.full((B, 3 * n), np.nan, dtype=np.float32)
    coords[0], coords[B - 1] = xyz.reshape(-1), xyz[::-1].reshape(-1)
    counts = np.zeros((B, 1), dtype=np.int32)
    counts[0], counts[B - 1] = n, n
    c, nt = torch.from_numpy(coords).to(device), torch.from_numpy(counts).to(device)
    of = torch.zeros(B, 1, dtype=torch.int32, device=device)
    dense = torch.full((B, 1, L, L, L), float("nan"), dtype=torch.float32, device=device)
    sparse = torch.full((B, 1, L, L, L), float("nan"), dtype=torch.float32, device=device)
    occ = torch.full((B, nc, nc, nc), 255, dtype=torch.uint8, device=device)
    lib.call("dlpd_project_atoms_ext", _ptr(c), _ptr(nt), _ptr(of), 0, 0.0, 0.0, 0.0, _ptr(dense), B, n, 1, L, res, 0,
             1.0, 2, 0.0, 1.0, _stream(device))
    lib.call("dlpd_project_atoms_cells", _ptr(c), _ptr(nt), _ptr(of), 0, 0.0, 0.0, 0.0, _ptr(sparse), _ptr(occ), B, n, 1, L, res,
             1.0, 2, 0.0, 1.0, _stream(device))
    dense, sparse, occ = dense.cpu(), sparse.cpu(), occ.cpu()
    assert int(occ.max()) == 1 and int(occ[B - 1].sum()) > 0 and int(occ[0].sum()) > 0 and int(occ[1:B - 1].sum()) == 0
    live = occ.bool().repeat_interleave(4, 1).repeat_interleave(4, 2).repeat_interleave(4, 3)[:, None, :L, :L, :L]
    assert bool(torch.isfinite(dense).all()) and float(dense[B - 1].max()) > 0.5
    assert torch.equal(sparse[live], dense[live]), "the second trip: cell-wise and dense values differ where the map is set"
    assert bool(torch.isnan(sparse[~live]).all()) and bool((dense[~live] == 0).all())
    assert torch.equal(dense[0], dense[B - 1])               # (the same atoms in another order: integer adds commute)


# ----------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ----------------------------------------------------------------------------------------------------------------------

class _Recording:
    """Stands in for the library: any call is a launch that should not have happened."""

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append(name)
        raise AssertionError("launched %s" % name)


def check_project_refusals(lib, device):
    """CoordsBackend.project raises before any launch: R of nb rows with coords of B rows, B neither 1 nor nb (the kernel would
    read nb * stride atoms from a buffer of B * stride), and a shift that does not hold exactly three values."""
    L, res = 6, 1.25
    rows = [Row(*_positions(4, 20 + b, L, res, 0.0)) for b in range(2)]
    c, nt, of = tensors(rows, device)
    R = torch.from_numpy(acc.rots(3, seed=2).astype(np.float32)).to(device)
    for cells in (False, True):
        rec = _Recording()
        be = CoordsBackend(lib=rec)
        with pytest.raises(ValueError, match="rows"):
            be.project(c, nt, of, L, res, device, R=R, cells=cells)
        for shift in (torch.zeros(4), torch.zeros(2), torch.zeros(2, 3), torch.zeros(0)):
            with pytest.raises(ValueError, match="shift"):
                be.project(c, nt, of, L, res, device, shift=shift, cells=cells)
        assert rec.calls == []
    # what stays allowed: B == nb, B == 1, no R; a shift of any shape with three values
    be = CoordsBackend(lib=lib)
    assert be.project(c, nt, of, L, res, device, R=R[:2], shift=torch.zeros(1, 3)).shape[0] == 2
    assert be.project(c[:1], nt[:1], of[:1], L, res, device, R=R, shift=[0.0, 0.0, 0.0]).shape[0] == 3
    assert be.project(c, nt, of, L, res, device).shape[0] == 2


def check_abi_refusals(lib, device):
    """The C entry points return DLPD_ERR_ARG (the binding raises) for window 7, sigma 0, norm 65, box 0 and a null output, and
    leave a NaN-prefilled output untouched."""
    from deeplocalproteindocking_amd.engine import _ptr, _stream
    device = torch.device(device)
    L, res = 5, 1.0
    row = Row(*_positions(6, 30, L, res, 0.0))
    c, nt, of = tensors([row], device)
    nc = (L + 3) // 4
    good = dict(out=True, L=L, sigma=1.0, window=2, norm=1.0)
    bad = [dict(window=7), dict(sigma=0.0), dict(norm=65.0), dict(L=0), dict(out=False)]
    for cells in (False, True):
        for change in bad + [dict()]:
            a = dict(good, **change)
            out = torch.full((1, T, L, L, L), float("nan"), dtype=torch.float32, device=device)
            occ = torch.full((1, nc, nc, nc), 7, dtype=torch.uint8, device=device)
            po = _ptr(out) if a["out"] else 0
            if cells:
                args = ("dlpd_project_atoms_cells", _ptr(c), _ptr(nt), _ptr(of), 0, 0.0, 0.0, 0.0, po, _ptr(occ), 1, row.stride, T,
                        a["L"], res, a["sigma"], a["window"], 0.0, a["norm"], _stream(device))
            else:
                args = ("dlpd_project_atoms_ext", _ptr(c), _ptr(nt), _ptr(of), 0, 0.0, 0.0, 0.0, po, 1, row.stride, T,
                        a["L"], res, 0, a["sigma"], a["window"], 0.0, a["norm"], _stream(device))
            if change:
                with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
                    lib.call(*args)
                assert bool(torch.isnan(out).all().cpu()) and bool((occ == 7).all().cpu()), (cells, change)
            else:                                                      # (the same call without the defect runs)
                lib.call(*args)
                assert not bool(torch.isnan(out).all().cpu())
