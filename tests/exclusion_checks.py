"""Search with an exclusion radius (csrc/dlpd_suppress.h): check bodies shared by tests/test_exclusion_emu.py (the
emulated library) and tests/test_exclusion_gpu.py (the gfx950 build).

The oracle is the definition of include/dlpd.h written out in numpy: for every offset d of the ball, ``np.roll`` brings V[v + d]
to v and the (value, flat index) comparison says whether that neighbour beats v; a negative voxel that something beats becomes
+0.0, everything else keeps its bits.  The list is then ``oracle.docking_oracle.rotation_picks_fast`` / ``update_top`` on the
result, merged by (score, rotation, pick).  Every comparison is bit for bit on uint32 views: the kernels compare and copy, they
compute nothing, so there is no tolerance anywhere.  Nothing here reads the reference tree."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import docking_oracle as orc
from deeplocalproteindocking_amd.engine import DeviceTopList, DockingEngine

TILE = (8, 8, 32)                    # the kernel's tile (SUP_TX, SUP_TY, SUP_TZ): sizes one below and one above each edge are cases
SIZES = (3, 7, 8, 9, 10, 12, 20, 31, 33)
NAN_BITS = 0xFFFFFFFF


# ----------------------------------------------------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------------------------------------------------

def suppress_oracle(V, r):
    """suppress_r(V) of one (n, n, n) float32 volume, from the definition."""
    V = np.ascontiguousarray(V, dtype=np.float32)
    n = V.shape[0]
    assert V.shape == (n, n, n) and 2 * r + 1 <= n
    beaten = np.zeros(V.shape, dtype=bool)
    rolled = {}
    for dx, dy, dz in itertools.product(range(-r, r + 1), repeat=3):
        if (dx, dy, dz) == (0, 0, 0):
            continue
        if dz == -r:                                                     # (one roll per offset: the x and y rolls are shared)
            if dy == -r:
                rolled["x"] = np.roll(V, -dx, axis=0)
            rolled["xy"] = np.roll(rolled["x"], -dy, axis=1)
        U = np.roll(rolled["xy"], -dz, axis=2)                           # U[v] = V[(v + d) mod n]
        beaten |= U < V
        x, y, z = np.nonzero(U == V)                                     # equal values: the lower flat index beats
        if len(x):
            fv = (x * n + y) * n + z
            fu = (((x + dx) % n) * n + (y + dy) % n) * n + (z + dz) % n
            lost = fu < fv
            beaten[x[lost], y[lost], z[lost]] = True
    out = V.copy()
    out[(V < 0) & beaten] = np.float32(0.0)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expected_entries(Vs_by_rotation, K):
    """[(rotation id, suppressed volume)] -> the list's (rot, idx, score, pick), by the oracle's picks and the merge key."""
    parts = []
    for rid, Vs in Vs_by_rotation:
        idx, sc = orc.rotation_picks_fast(Vs, K)
        parts.append((np.full(K, rid, dtype=np.int64), idx.astype(np.int64), sc.astype(np.float32), np.arange(K, dtype=np.int64)))
    return DeviceTopList.merge_entries(parts, K)


def assert_same_entries(got, want):
    assert len(got[0]) == len(want[0])
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[3] == want[3]).all()
    assert (bits(got[2]) == bits(want[2])).all()


def assert_apart(entries, n, r):
    """No two negative entries of one rotation lie within r voxels of each other on the wrapped grid."""
    rot, idx, score, _ = entries
    for rid in np.unique(rot):
        sel = (rot == rid) & (score < 0)
        p = np.stack(orc.flat_to_xyz(idx[sel], n), axis=1)
        if len(p) < 2:
            continue
        d = np.abs(p[:, None, :] - p[None, :, :])
        d = np.minimum(d, n - d).max(axis=2)
        d[np.arange(len(p)), np.arange(len(p))] = n
        assert d.min() > r, (rid, int(d.min()))


# ----------------------------------------------------------------------------------------------------------------------
# calling the two entries
# ----------------------------------------------------------------------------------------------------------------------

def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0


def run_suppress(lib, device, V, r, ccount=None, cap=0):
    """V (nb, n, n, n) float32 numpy -> Vs numpy, from a NaN-filled output."""
    nb, n = V.shape[0], V.shape[1]
    Vd = torch.from_numpy(np.array(V, dtype=np.float32)).to(device)        # (a copy: on the CPU from_numpy shares the array)
    Vs = torch.full((nb, n * n * n), float("nan"), dtype=torch.float32, device=device)
    Vs.view(torch.int32).fill_(-1)                                        # (one NaN pattern: 0xFFFFFFFF)
    cc = None if ccount is None else torch.from_numpy(np.array(ccount, dtype=np.int32)).to(device)
    rc = lib.call("dlpd_topk_suppress", Vd.data_ptr(), Vs.data_ptr(), nb, n, r, 0 if cc is None else cc.data_ptr(), cap,
                  _stream(device))
    _sync(device)
    assert rc == 0 and (bits(Vd.cpu().numpy()) == bits(V)).all()          # the input is only read
    return Vs.cpu().numpy().reshape(nb, n, n, n)


def volumes(kind, nb, n, seed):
    rng = np.random.RandomState(seed)
    if kind == "normal":
        return rng.standard_normal((nb, n, n, n)).astype(np.float32)
    if kind == "integers":                                               # many ties, zeros of both signs among them
        V = rng.randint(-3, 3, size=(nb, n, n, n)).astype(np.float32)
        V[rng.rand(nb, n, n, n) < 0.05] = np.float32(-0.0)
        return V
    if kind == "sparse":                                                 # fewer negatives than any K of the tests
        V = np.abs(rng.standard_normal((nb, n, n, n))).astype(np.float32) + np.float32(0.5)
        for b in range(nb):
            for _ in range(5):
                V[(b,) + tuple(rng.randint(0, n, size=3))] = -np.float32(rng.rand() + 0.1)
        return V
    if kind == "nonnegative":
        V = np.abs(rng.standard_normal((nb, n, n, n))).astype(np.float32)
        V[rng.rand(nb, n, n, n) < 0.1] = np.float32(-0.0)
        V[rng.rand(nb, n, n, n) < 0.1] = np.float32(0.0)
        return V
    raise ValueError(kind)


def radii(n):
    return [r for r in (1, 2, 3, 4) if 2 * r + 1 <= n]


def check_suppress_volumes(lib, device, n, kinds=("normal", "integers"), rs=None):
    for r, nb, kind in itertools.product(rs or radii(n), (1, 3), kinds):
        V = volumes(kind, nb, n, 100 * n + 10 * r + nb)
        got = run_suppress(lib, device, V, r)
        for b in range(nb):
            want = suppress_oracle(V[b], r)
            assert (bits(got[b]) == bits(want)).all(), (n, r, nb, kind, b)
            gone = (V[b] < 0) & (bits(want) != bits(V[b]))
            assert (bits(got[b])[gone] == 0).all()                       # a suppressed voxel is +0.0, sign bit clear
            if kind == "normal":
                assert gone.any() and ((V[b] < 0) & ~gone).any()
            if n == 2 * r + 1:                                           # every voxel is every other's neighbour
                assert int((got[b] < 0).sum()) == int((V[b] < 0).any())


def check_planted(lib, device, n, rs=None):
    """Equal negatives across the cyclic faces, in a line and at the eight corners: the lowest flat index survives."""
    one = np.float32(1.0)
    for r in rs or radii(n):
        a, b = n // 2, n // 3
        cases = []
        for axis in range(3):                                            # two equal negatives facing each other across a face
            V = np.full((n, n, n), one, dtype=np.float32)
            lo, hi = [a, b, a], [a, b, a]
            lo[axis], hi[axis] = 0, n - 1
            V[tuple(lo)] = V[tuple(hi)] = np.float32(-2.0)
            cases.append((V, [tuple(lo)]))
        m = min(5, n)
        V = np.full((n, n, n), one, dtype=np.float32)                    # a line of equal negatives along z, off the origin
        z0 = 1 if n > m else 0
        V[a, b, z0:z0 + m] = np.float32(-3.0)
        cases.append((V, [(a, b, z0)]))
        V = np.full((n, n, n), one, dtype=np.float32)                    # ... and along x (the slowest axis)
        V[z0:z0 + m, b, a] = np.float32(-3.0)
        cases.append((V, [(z0, b, a)]))
        V = np.full((n, n, n), one, dtype=np.float32)                    # all eight corners
        for c in itertools.product((0, n - 1), repeat=3):
            V[c] = np.float32(-1.5)
        cases.append((V, [(0, 0, 0)]))
        got = run_suppress(lib, device, np.stack([c[0] for c in cases]), r)
        for k, (V, survivors) in enumerate(cases):
            want = suppress_oracle(V, r)
            assert (bits(got[k]) == bits(want)).all(), (n, r, k)
            assert [tuple(int(v) for v in p) for p in np.argwhere(got[k] < 0)] == survivors, (n, r, k)


def check_nonnegative_is_returned_as_is(lib, device, n):
    for r in radii(n):
        V = volumes("nonnegative", 2, n, 7 * n + r)
        assert (bits(V) == 0x80000000).any() and (bits(V) == 0).any()
        got = run_suppress(lib, device, V, r)
        assert (bits(got) == bits(V)).all()


def check_zero_fill(lib, device, n=10, K=16):
    """Fewer negatives than K: the select on Vs gives the oracle's zero-fill (through DeviceTopList.select, no cset)."""
    for r in radii(n):
        V = volumes("sparse", 3, n, 40 + r)
        V[1, 0, 0, 1] = np.float32(-0.0)                                 # an original zero in front of every pick ...
        V[2, n - 1, n - 1, n - 1] = np.float32(0.0)                      # ... and one behind them all
        top = DeviceTopList(K, 3, device, lib, exclusion=r)
        sc, idx = top.select(torch.from_numpy(V).to(device).reshape(3, -1), 3)
        _sync(device)
        sc, idx = sc.cpu().numpy(), idx.cpu().numpy()
        for b in range(3):
            wi, ws = orc.rotation_picks_fast(suppress_oracle(V[b], r), K)
            assert int((ws < 0).sum()) < K
            assert (idx[b] == wi).all() and (bits(sc[b]) == bits(ws)).all(), (r, b)


def check_rows_of_complete_lists_are_not_written(lib, device, n=12, cap=64):
    for r in radii(n):
        V = volumes("normal", 4, n, 60 + r)
        # rotation 0: complete (flag clear, count <= cap); 1: flagged; 2: over the cap; 3: complete with count == cap
        ccount = [5, 5, cap + 1, cap, 0, 1, 0, 0]
        got = run_suppress(lib, device, V, r, ccount=ccount, cap=cap)
        for b in (0, 3):
            assert (bits(got[b]) == NAN_BITS).all()                      # poison kept
        for b in (1, 2):
            assert (bits(got[b]) == bits(suppress_oracle(V[b], r))).all()


def check_suppress_on_the_device(lib, device, n, r, nb=2):
    """Guarded allocations, a NaN-filled output, sizes of the real grids."""
    from guard_alloc import GuardedAllocations
    V = volumes("normal", nb, n, n + r)
    V[0, 0, 0, 0] = V[0, n - 1, n - 1, n - 1] = np.float32(-9.0)          # a tie across all three faces, among the deepest
    with GuardedAllocations(empty_byte=0xFF) as g:
        Vd = torch.empty(nb, n * n * n, dtype=torch.float32, device=device)
        Vs = torch.empty(nb, n * n * n, dtype=torch.float32, device=device)
        Vd.copy_(torch.from_numpy(V).reshape(nb, -1))
        rc = lib.call("dlpd_topk_suppress", Vd.data_ptr(), Vs.data_ptr(), nb, n, r, 0, 0, _stream(device))
        assert rc == 0
        bad = g.check(release=False)
        got = Vs.cpu().numpy().reshape(nb, n, n, n)
        g.check()
    assert not bad, bad
    want = suppress_oracle(V[0], r)                                      # (the oracle is the slow side: one rotation by it ...)
    assert (bits(got[0]) == bits(want)).all()
    assert got[0, 0, 0, 0] == np.float32(-9.0) and bits(got[0])[n - 1, n - 1, n - 1] == 0
    for b in range(1, nb):                                               # ... the others by what the definition implies
        neg = got[b] < 0
        assert (bits(got[b])[neg] == bits(V[b])[neg]).all() and (bits(got[b])[~neg & (V[b] < 0)] == 0).all()
        assert (bits(got[b])[V[b] >= 0] == bits(V[b])[V[b] >= 0]).all()
        p = np.argwhere(neg)[:2000]
        for x, y, z in p[:: max(1, len(p) // 200)]:
            ball = V[b][np.ix_(*[np.arange(c - r, c + r + 1) % n for c in (x, y, z)])]
            assert V[b, x, y, z] == ball.min()


# ----------------------------------------------------------------------------------------------------------------------
# the candidate lists
# ----------------------------------------------------------------------------------------------------------------------

def f2key(v):
    u = bits(np.asarray(v, dtype=np.float32) + np.float32(0.0)).astype(np.uint64)
    return np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def check_suppress_cand(lib, device, n=12):
    rng = np.random.RandomState(5)
    for r, cap in itertools.product(radii(n), (64, 4096)):
        nb = 6
        V = volumes("normal", nb, n, 80 + r)
        V[4].reshape(-1)[:40] = np.float32(-1.25)                         # equal scores next to each other in list 4
        flat = V.reshape(nb, -1)
        lists = []
        for b in range(nb):
            few = cap == 64
            tau = np.sort(flat[b])[40 if few else 700]                    # what K3 appends: every voxel at or below a bound,
            ids = np.nonzero(flat[b] <= tau)[0]                           # in the order its blocks happened to finish
            lists.append(rng.permutation(ids))
        lists[3] = lists[3][:0]                                           # an empty list
        keys = np.full((nb, cap), 0x5555555555555555, dtype=np.uint64)
        count = np.zeros(2 * nb, dtype=np.int32)
        for b, ids in enumerate(lists):
            keys[b, :len(ids)] = (f2key(flat[b][ids]) << np.uint64(32)) | ids.astype(np.uint64)
            count[b] = len(ids)
        count[nb + 1] = 1                                                 # list 1: flagged
        count[2] = cap + 7                                                # list 2: over the cap (K3 counts on, stores cap keys)
        kd = torch.from_numpy(keys.view(np.int64).copy()).to(device)      # (copies: on the CPU from_numpy shares the array)
        cd = torch.from_numpy(count.copy()).to(device)
        Vd = torch.from_numpy(V.copy()).to(device)
        rc = lib.call("dlpd_topk_suppress_cand", Vd.data_ptr(), nb, n, r, kd.data_ptr(), cd.data_ptr(), cap, _stream(device))
        _sync(device)
        assert rc == 0
        k2, c2 = kd.cpu().numpy().view(np.uint64), cd.cpu().numpy()
        assert (c2[nb:] == count[nb:]).all()                             # flags left alone
        for b in (1, 2, 3):
            assert c2[b] == count[b] and (k2[b] == keys[b]).all()        # flagged, over the cap, empty: untouched
        for b in (0, 4, 5):
            keep = suppress_oracle(V[b], r).reshape(-1)[lists[b]] < 0
            want = keys[b, :len(lists[b])][keep]
            assert 0 < len(want) < len(lists[b]) and c2[b] == len(want)  # counts are lowered
            assert (k2[b, :len(want)] == want).all()                     # the survivors, in list order
        if cap == 4096:
            assert max(len(lists[b]) for b in (0, 4, 5)) > 256           # more than one round of the block


# ----------------------------------------------------------------------------------------------------------------------
# errors
# ----------------------------------------------------------------------------------------------------------------------

def check_errors(lib, device):
    n, nb, cap = 8, 2, 64
    V = torch.from_numpy(volumes("normal", nb, n, 3)).to(device)
    Vs = torch.full((nb, n ** 3), -7.0, dtype=torch.float32, device=device)
    keys = torch.full((nb, cap), -7, dtype=torch.int64, device=device)
    count = torch.tensor([3, 3, 0, 0], dtype=torch.int32, device=device)
    st = _stream(device)

    def sup(V_=V.data_ptr(), Vs_=Vs.data_ptr(), nb_=nb, n_=n, r=1, cc=0, cap_=0):
        return lib.call("dlpd_topk_suppress", V_, Vs_, nb_, n_, r, cc, cap_, st)

    def cand(V_=V.data_ptr(), nb_=nb, n_=n, r=1, k=keys.data_ptr(), c=count.data_ptr(), cap_=cap):
        return lib.call("dlpd_topk_suppress_cand", V_, nb_, n_, r, k, c, cap_, st)
    for fn, cases in ((sup, (dict(r=0), dict(r=-1), dict(r=5), dict(r=4), dict(n_=2, r=1), dict(nb_=0), dict(nb_=-2), dict(V_=0),
                             dict(Vs_=0), dict(Vs_=V.data_ptr()))),
                      (cand, (dict(r=0), dict(r=5), dict(r=4), dict(n_=2), dict(nb_=0), dict(V_=0), dict(k=0), dict(c=0)))):
        for kw in cases:
            with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
                fn(**kw)
    for fn in (sup, cand):
        for big in (1291, 2000, 1 << 30):
            with pytest.raises(RuntimeError, match="UNSUPPORTED"):
                fn(n_=big)                                                # (refused before anything is read)
    _sync(device)
    assert (Vs == -7.0).all() and (keys == -7).all() and count.tolist() == [3, 3, 0, 0]      # nothing was written
    top = DeviceTopList(4, 1, device, lib, exclusion=1)
    with pytest.raises(RuntimeError, match="cubic"):
        top.select(torch.zeros(1, 12, dtype=torch.float32, device=device), 1)
    assert sup() == 0 and cand() == 0


# ----------------------------------------------------------------------------------------------------------------------
# the engine, driven by hand
# ----------------------------------------------------------------------------------------------------------------------

L, NROT, BATCH = 32, 12, 4


def smooth(v, passes=2):
    """A (C, l, l, l) volume averaged over 5^3 neighbourhoods and brought back to unit scale: scores of smooth volumes have
    wells that are several voxels wide, which is what an exclusion radius is for (white noise has none)."""
    for _ in range(passes):
        v = torch.nn.functional.avg_pool3d(v[None], 5, stride=1, padding=2)[0]
    return v / v.abs().max()


def engine_case(C, seed, inner=None):
    import engine_reuse_checks as erc
    g = torch.Generator().manual_seed(seed)
    cut = (lambda v: erc.embed(v, inner)) if inner else (lambda v: v)
    rec = cut(smooth(torch.randn(C, L, L, L, generator=g)) * 0.3)
    lig = torch.zeros(C, L, L, L)
    a, b = (2, 10) if inner else (10, 22)
    lig[:, a:b, a:b, a:b] = smooth(torch.randn(C, b - a, b - a, b - a, generator=g))
    recf, ligf = erc.forbidden(g, L, inner)
    return rec, recf, lig, ligf, erc.rotations(NROT, seed + 1), erc.filter_weights(C, seed + 2)


def make_engine(lib, device, case, K, r, batch=BATCH, cap=None, **kw):
    rec, recf, lig, ligf, R, filt = case
    extent = kw.get("extent")
    thr = 0.3 * (extent or L) ** 3
    eng = DockingEngine(L, rec.shape[0], *filt, clip=5.0, threshold_clash=thr, max_conf=K, batch=batch, device=device, lib=lib,
                        exclusion=r, **kw)
    if cap is not None:
        eng.top.CAND_CAP = cap                                           # (on the instance: the sets made below are small)
    eng.set_receptor(rec, recf)
    eng.set_ligand(lig, ligf)
    return eng


def drive(eng, R, r, oracle=True):
    """score_batch / select_batch / merge_batch by hand -> (the engine's entries, the list expected from the engine's own V
    (None without ``oracle``), complete lists seen, overflows seen, n of the grid the top-K works on)."""
    dev = eng.device
    eng.reset_top()
    assert eng.top.exclusion == r
    cset = eng.top.new_candidate_set() if eng.prefilter else None
    seen, complete, overflow = [], 0, 0
    n = eng.N
    for beg in range(0, R.shape[0], eng.batch):
        Rb = R[beg:beg + eng.batch].to(dev).contiguous()
        nb = Rb.shape[0]
        tau = int(eng.top.tau[0])
        V = eng.score_batch(Rb, cset=cset)
        used = eng._cset_used if cset is not None else None
        G = eng.gather_window(V, nb) if eng.window is not None else V.reshape(nb, -1)
        n = int(round(G.shape[1] ** (1.0 / 3.0)))
        Gh = G.cpu().numpy().reshape(nb, n, n, n).copy()
        if used is not None:
            c = used["count"].cpu().numpy()
            flags, counts = c[eng.batch:eng.batch + nb], c[:nb]
            assert (flags == 0).all() == (tau != 0)                      # K3 flags a rotation iff it saw no filter
            complete += int(((flags == 0) & (counts <= used["cap"])).sum())
            overflow += int(((flags == 0) & (counts > used["cap"])).sum())
        eng.select_batch(V, nb, used)
        eng.merge_batch(torch.arange(beg, beg + nb, dtype=torch.int32, device=dev), nb)
        if oracle:
            seen += [(beg + i, suppress_oracle(Gh[i], r) if r else Gh[i]) for i in range(nb)]
    got = eng.top_entries()
    if cset is not None:
        assert (cset["count"] == 0).all()                                # consumed
    return got, (expected_entries(seen, eng.K) if oracle else None), complete, overflow, n


def check_engine(lib, device, K, r, C=3, cap=None):
    case = engine_case(C, 11 + C)
    eng = make_engine(lib, device, case, K, r, cap=cap)
    assert eng.switches()["exclusion"] == r and eng.prefilter
    got, want, complete, overflow, n = drive(eng, case[4], r)
    print("exclusion %d, K %d, cap %s: %d complete lists, %d overflows, %d negative entries" %
          (r, K, cap, complete, overflow, int((got[2] < 0).sum())))
    assert_same_entries(got, want)
    assert (got[2] < 0).sum() > K // 2
    assert_apart(got, n, r)
    if cap is None:
        assert complete >= 1                                             # the candidate path was live ...
    else:
        assert overflow >= 1                                             # ... and so was the radix select behind an overflow
    return got


def check_engine_variants(lib, device, K=16, r=2, C=2):
    """prefilter=False, launch batches 3 and 8 and the pipelined search() give the list of the hand-driven engine."""
    case = engine_case(C, 11 + C)
    base = drive(make_engine(lib, device, case, K, r), case[4], r)
    assert_same_entries(base[0], base[1])
    plain = make_engine(lib, device, case, K, r, prefilter=False)
    got = drive(plain, case[4], r, oracle=False)
    assert got[2] == 0 and got[3] == 0
    assert_same_entries(got[0], base[0])
    for batch in (3, 8):
        eng = make_engine(lib, device, case, K, r, batch=batch)
        eng.reset_top()
        eng.search(case[4])
        assert_same_entries(eng.top_entries(), base[0])


def check_engine_embedded(lib, device, K=16, r=2, C=2, inner=12):
    case = engine_case(C, 31, inner=inner)
    eng = make_engine(lib, device, case, K, r, extent=inner, center=inner / 2.0)
    assert eng.window is not None and not eng.prefilter
    got, want, _, _, n = drive(eng, case[4], r)
    assert n == 2 * inner
    assert_same_entries(got, want)
    assert (got[2] < 0).sum() > K // 2
    assert_apart(got, n, r)


# ----------------------------------------------------------------------------------------------------------------------
# Docker: the unfused loop, update_top, reuse, defaults, two ranks, the script
# ----------------------------------------------------------------------------------------------------------------------

class _UserModel(object):
    """A docking model of the user's own (Docker.py:229 calls it): circular correlation by torch's FFT, shifted below zero.
    What it returns IS the search's V (no clash channel), so it is kept for the oracle."""
    threshold_clash = 300.0

    def __init__(self):
        self.seen = []

    def __call__(self, receptor_volumes, ligand_volumes):
        r, l = receptor_volumes[0].double().cpu(), ligand_volumes[0].double().cpu()
        s = [2 * r.shape[-1]] * 3
        V = torch.fft.irfftn(torch.fft.rfftn(r, s=s).conj() * torch.fft.rfftn(l, s=s), s=s).sum(dim=1) - 0.05
        V = V.float().to(receptor_volumes[0].device)
        self.seen.append(V.cpu().numpy().copy())
        return V


def check_docker_unfused(lib, device, box=12, K=16, r=2):
    import engine_reuse_checks as erc
    from deeplocalproteindocking_amd.Docker import Docker
    g = torch.Generator().manual_seed(3)
    rec, lig = torch.randn(1, 2, box, box, box, generator=g) * 0.1, torch.randn(1, 2, box, box, box, generator=g) * 0.1
    R = erc.rotations(5, 9).double().numpy()
    model = _UserModel()
    dk = Docker(model, box_size=box, max_conf=K, rotations=R, device=device, lib=lib, exclusion=r)
    got = dk.dock_volumes([rec], [lig], write=False, model_batch=2)
    assert dk.path == "call" and dk.engine is None
    V = np.concatenate(model.seen)
    want = expected_entries([(i, suppress_oracle(V[i], r)) for i in range(len(V))], K)
    assert got == DeviceTopList.to_top_list(want, 2 * box)
    assert sum(e[4] < 0 for e in got) > K // 2
    assert_apart(want, 2 * box, r)


def check_update_top(lib, device, n=10, K=12):
    from deeplocalproteindocking_amd.Docker import Docker
    for r in (1, 2, 4):
        dk = Docker(None, box_size=n // 2, max_conf=K, rotations=np.eye(3)[None], device=device, lib=lib, exclusion=r)
        want = []
        for rid in (0, 1):
            Vh = volumes("normal" if rid == 0 else "sparse", 1, n, 50 + rid)[0]
            V = torch.from_numpy(Vh.copy()).to(device)
            dk.update_top(V, rid)
            Vo = torch.from_numpy(suppress_oracle(Vh, r))
            picks = orc.update_top([], Vo.clone(), rid, K)
            want = orc.update_top(want, Vo, rid, K)                      # the reference's own loop on suppress_r(V)
            assert [e[:4] for e in dk.top_list] == [e[:4] for e in want]
            assert (bits([e[4] for e in dk.top_list]) == bits([e[4] for e in want])).all()
            Vexp = Vh.copy()                                             # the picked voxels are zero in V, no other changed
            for e in picks:
                Vexp[e[1], e[2], e[3]] = np.float32(0.0)
            assert (bits(V.cpu().numpy()) == bits(Vexp)).all()


def _docker(lib, device, K, R, **kw):
    from cluster_checks import _Model
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Models import SimpleFilter
    torch.manual_seed(22)
    filt = SimpleFilter([2])
    with torch.no_grad():
        filt.fc[2].weight.copy_(-filt.fc[2].weight.abs())
        filt.fc[2].bias.fill_(-1.0)
    return Docker(_Model(filt.to(device)), box_size=L, resolution=1.25, max_conf=K, rotations=R, device=device, lib=lib,
                  launch_batch=BATCH, **kw)


def _volume_pair():
    g = torch.Generator().manual_seed(21)
    rec, lig = smooth(torch.randn(2, L, L, L, generator=g))[None] * 0.3, smooth(torch.randn(2, L, L, L, generator=g))[None] * 0.3
    return rec, lig, torch.rand(L, L, L, generator=g), torch.rand(L, L, L, generator=g)


def check_reuse_and_defaults(lib, device, K=16):
    """A live engine serves exclusion 0 -> 2 -> 0; each list is a fresh Docker's, the r = 0 lists those of a Docker built
    without the keyword -- and with exclusion 0 neither new entry is ever called."""
    import engine_reuse_checks as erc
    from deeplocalproteindocking_amd._lib import DlpdLib
    R = erc.rotations(4, 8).double().numpy()
    pair = _volume_pair()

    class Recording(object):
        def __init__(self, inner):
            self.inner, self.names = inner, []

        def call(self, name, *args):
            self.names.append(name)
            return self.inner.call(name, *args)

        def __getattr__(self, name):
            return getattr(self.inner, name)
    if lib is None:
        from deeplocalproteindocking_amd._lib import get_lib
        lib = get_lib()
    assert isinstance(lib, DlpdLib)
    rec_lib = Recording(lib)
    live = _docker(rec_lib, device, K, R)
    assert live.exclusion == 0
    lists = []
    for r in (0, 2, 0):
        live.exclusion = r
        seen = len(rec_lib.names)
        lists.append(list(live.dock_volumes([pair[0]], [pair[1]], pair[2], pair[3], write=False)))
        called = set(rec_lib.names[seen:])
        assert live.path == "fused" and live.engine.switches()["exclusion"] == r
        assert "dlpd_topk_select_cand" in called or "dlpd_topk_select" in called
        if r == 0:
            assert not [nm for nm in called if "suppress" in nm]          # exactly today's calls
        else:
            assert "dlpd_topk_suppress" in called and "dlpd_topk_suppress_cand" in called
    engine = live.engine
    for r, got in zip((0, 2, 0), lists):
        fresh = _docker(lib, device, K, R, exclusion=r)
        assert fresh.dock_volumes([pair[0]], [pair[1]], pair[2], pair[3], write=False) == got and fresh.engine is not engine
    plain = _docker(lib, device, K, R)
    assert plain.dock_volumes([pair[0]], [pair[1]], pair[2], pair[3], write=False) == lists[0] == lists[2]
    assert lists[1] != lists[0] and len(lists[1]) == K


def check_two_ranks(lib, device, K=16, r=2):
    import engine_reuse_checks as erc
    R = erc.rotations(7, 12).double().numpy()
    pair = _volume_pair()
    one = _docker(lib, device, K, R, exclusion=r)
    one.dock_volumes([pair[0]], [pair[1]], pair[2], pair[3], write=False)
    want = one.engine.top_entries()
    parts = []
    for rank in (0, 1):
        dk = _docker(lib, device, K, R, exclusion=r, rank=rank, world_size=2)
        dk._gather = lambda entries: (parts.append(entries), entries)[1]          # (the collective's place: it does not change)
        dk.dock_volumes([pair[0]], [pair[1]], pair[2], pair[3], write=False)
        assert set(parts[-1][0].tolist()) <= set(dk.shard(len(R)).tolist()) and len(parts[-1][0]) == K
    assert_same_entries(DeviceTopList.merge_entries(parts, K), want)
    assert_apart(want, 2 * L, r)


def check_dock_pair(lib, device, tmp_path):
    """The script's search step (``search``, what ``--exclusion R`` reaches) on two synthetic PDB files."""
    from synth_pdb import write_protein_like_pdb
    from test_atoms import _tiny_model
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend
    import engine_reuse_checks as erc
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import dock_pair
    assert dock_pair.parse_exclusion("0") == 0 and dock_pair.parse_exclusion("4") == 4
    for bad in ("5", "-1"):
        with pytest.raises(ValueError, match="exclusion"):
            dock_pair.parse_exclusion(bad)
    frec, flig = str(tmp_path / "r.pdb"), str(tmp_path / "l.pdb")
    write_protein_like_pdb(frec, 14, seed=5)
    write_protein_like_pdb(flig, 9, seed=6)
    K = 40
    R = erc.rotations(3, 2).double().numpy()
    dk = Docker(_tiny_model().to(device), box_size=L, resolution=1.25, max_conf=K, rotations=R, device=device, lib=lib,
                coords_backend=CoordsBackend(lib=lib))
    lists = {}
    with torch.no_grad():
        p = dk.prepare(frec, flig, "SE3")
        for r in (0, 2):
            out = str(tmp_path / ("pair%d.dat" % r))
            dk.new_log(out)
            lists[r] = list(dock_pair.search(dk, frec, flig, "SE3", 2, prepared=p, exclusion=r))
            dk.cleanup()
            assert dk.exclusion == r and len(open(out).read().strip().split("\n")) == K
    ent = lambda top: (np.array([e[0] for e in top]), np.array([(e[1] * 2 * L + e[2]) * 2 * L + e[3] for e in top]),
                       np.array([e[4] for e in top], dtype=np.float32), None)
    assert lists[2] != lists[0] and lists[2][0] == lists[0][0]           # the best pose is a local minimum
    assert_apart(ent(lists[2]), 2 * L, 2)
    with pytest.raises(AssertionError):
        assert_apart(ent(lists[0]), 2 * L, 2)                            # the plain list IS neighbours of a few minima
