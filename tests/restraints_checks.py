"""Search under distance restraints (csrc/dlpd_restrain.h): check bodies shared by tests/test_restraints_emu.py (the
emulated library) and tests/test_restraints_gpu.py (the gfx950 build).

The oracle is ``Utils.Restraints.allowed`` -- the definition of include/dlpd.h in numpy int64 -- applied to every voxel's signed
index: a negative voxel that is not allowed becomes +0.0, everything else keeps its bits.  The list is then
``oracle.docking_oracle.rotation_picks_fast`` / ``update_top`` on the result, merged by (score, rotation, pick).  Every comparison
is bit for bit on uint32 / uint64 views: the kernels compare integers and copy floats, they compute nothing that rounds, so there
is no tolerance anywhere.  Nothing here reads the reference tree."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import exclusion_checks as xc
from exclusion_checks import bits, f2key, assert_same_entries, expected_entries, _sync, _stream, NAN_BITS
from oracle import docking_oracle as orc
from deeplocalproteindocking_amd.engine import DeviceTopList, DockingEngine
from deeplocalproteindocking_amd.Utils import Restraints as rs

TILE = (8, 8, 32)                    # the kernel's tile (RST_TX, RST_TY, RST_TZ)
SIZES = (4, 6, 8, 10, 12, 34, 64)    # n % 4 != 0, partial tiles, one below and one above each tile edge
JNEED = ((1, 1), (5, 1), (5, 3), (5, 5), (32, 1), (32, 7), (32, 32))
U = rs.UNIT


# ----------------------------------------------------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------------------------------------------------

def signed_axis(n):
    t = np.arange(n, dtype=np.int64)
    return np.where(t >= n // 2, t - n, t)


def allowed_volume(table, rot, n):
    """(n, n, n) bool: the voxels of the grid of side n that are allowed for rotation ``rot``."""
    t = signed_axis(n)
    T = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1)
    return rs.allowed(table, rot, T)


def restrain_oracle(V, table, rot):
    """restrain(V) of one (n, n, n) float32 volume, from the definition."""
    V = np.ascontiguousarray(V, dtype=np.float32)
    out = V.copy()
    out[(V < 0) & ~allowed_volume(table, rot, V.shape[0])] = np.float32(0.0)
    return out


def table_of(centres, lo, hi, need):
    """centres (nrot, J, 3), lo, hi (J,) in 1/256 voxel -> RestraintTable"""
    return rs.RestraintTable(np.asarray(centres, dtype=np.int32), np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64), need)


def clustered_table(nrot, J, need, n, seed):
    """J balls per rotation whose centres lie within 0.4 voxel (per axis) of a point p inside the grid, radii 1.6 .. 2.0 voxels
    (shells with lo up to 0.5 voxel for every third restraint, none for need = J): the voxel nearest to p lies in every ball
    -- the nearest voxel is within 0.87 of p, 0.87 + 0.69 < 1.6 -- and the union is a few voxels wide.  -> (table, p)"""
    rng = np.random.RandomState(seed)
    half = n // 2
    span = (-half + 0.5, -half + 1.5) if n <= 6 else (-half + 1.0, half - 2.0)
    p = rng.uniform(span[0], span[1], size=(nrot, 1, 3))
    c = np.rint(U * (p + rng.uniform(-0.4, 0.4, size=(nrot, J, 3))))
    hi = np.rint(U * rng.uniform(1.6, 2.0, size=J))
    lo = np.where((np.arange(J) % 3 == 1) & (need < J), np.rint(U * rng.uniform(0.1, 0.5, size=J)), 0)
    return table_of(c, lo, hi, need), p[:, 0]


def run_restrain(lib, device, V, table, rot_ids, ccount=None, cap=0, inplace=False):
    """V (nb, n, n, n) float32 numpy -> restrain(V) numpy, from a NaN-filled output (or in place)."""
    nb, n = V.shape[0], V.shape[1]
    Vd = torch.from_numpy(np.array(V, dtype=np.float32)).to(device).reshape(nb, -1)
    Vs = torch.empty((nb, n * n * n), dtype=torch.float32, device=device)
    Vs.view(torch.int32).fill_(-1)                                        # (one NaN pattern: 0xFFFFFFFF)
    out = Vd if inplace else Vs
    cd, bd = torch.from_numpy(table.centres.copy()).to(device), torch.from_numpy(table.bounds.copy()).to(device)
    ids = torch.tensor(list(rot_ids), dtype=torch.int32, device=device)
    cc = None if ccount is None else torch.from_numpy(np.array(ccount, dtype=np.int32)).to(device)
    rc = lib.call("dlpd_topk_restrain", Vd.data_ptr(), out.data_ptr(), nb, n, ids.data_ptr(), cd.data_ptr(), bd.data_ptr(),
                  table.J, table.need, 0 if cc is None else cc.data_ptr(), cap, _stream(device))
    _sync(device)
    assert rc == 0
    if not inplace:
        assert (bits(Vd.cpu().numpy().reshape(V.shape)) == bits(V)).all()  # the input is only read
    return out.cpu().numpy().reshape(nb, n, n, n)


ROT_IDS = {1: (3,), 3: (5, 2, 6)}      # not in order, not starting at 0; the tables have 7 rotations


def check_restrain_volumes(lib, device, n, combos=None):
    """combos: (nb, (J, need), kind) triples (default: all of them; at n = 64, where the numpy oracle is the slow side, three
    rotations for J = 1 and 5 and one for J = 32)."""
    combos = combos or [c for c in itertools.product((1, 3), JNEED, ("normal", "integers")) if n < 64 or (c[0] == 3) == (c[1][0] < 32)]
    for nb, (J, need), kind in combos:
        ids = ROT_IDS[nb]
        table, p = clustered_table(7, J, need, n, 1000 * n + 10 * J + need)
        V = xc.volumes(kind, nb, n, 100 * n + J + nb)
        for b, rid in enumerate(ids):                                    # a negative in the voxel nearest to p: every ball holds it
            q = np.rint(p[rid]).astype(int) % n
            V[b, q[0], q[1], q[2]] = np.float32(-2.0) if kind == "integers" else -np.abs(V[b, q[0], q[1], q[2]]) - np.float32(0.5)
        got = run_restrain(lib, device, V, table, ids)
        same = run_restrain(lib, device, V, table, ids, inplace=True)
        assert (bits(got) == bits(same)).all(), (n, nb, J, need, kind)
        for b, rid in enumerate(ids):
            want = restrain_oracle(V[b], table, rid)
            assert (bits(got[b]) == bits(want)).all(), (n, nb, J, need, kind, b)
            gone = (V[b] < 0) & (bits(want) != bits(V[b]))
            assert (bits(got[b])[gone] == 0).all()                       # a masked voxel is +0.0, sign bit clear
            assert gone.any() and (got[b] < 0).any(), (n, nb, J, need, kind, b)      # some removed, some left


def check_nonnegative_is_returned_as_is(lib, device, n):
    for J, need in ((1, 1), (5, 3), (32, 32)):
        table, _ = clustered_table(7, J, need, n, 7 * n + J)
        V = xc.volumes("nonnegative", 3, n, 7 * n + J)
        assert (bits(V) == 0x80000000).any() and (bits(V) == 0).any()
        assert (bits(run_restrain(lib, device, V, table, ROT_IDS[3])) == bits(V)).all()
        assert (bits(run_restrain(lib, device, V, table, ROT_IDS[3], inplace=True)) == bits(V)).all()


def _negative(n, seed):
    """Every voxel negative: what comes back negative IS the allowed region."""
    return (-1.0 - np.random.RandomState(seed).rand(1, n, n, n)).astype(np.float32)


def _index(t, n):
    return tuple(int(v) % n for v in t)


def check_planted(lib, device, n):
    """Geometry by hand on a grid of side n >= 12: (table, voxels that must be allowed, voxels that must not) per case, and
    the oracle for the whole volume."""
    half = n // 2
    cases = []
    # a centre exactly on a voxel, hi = 0: that voxel alone
    cases.append((table_of([[[2 * U, -3 * U, 1 * U]]], [0], [0], 1), [(2, -3, 1)], [(2, -3, 0), (1, -3, 1), (2, -2, 1)], 1))
    # d^2 == hi^2 is kept, one unit beyond it is not: centre one unit off the origin, hi = 3 voxels
    cases.append((table_of([[[1, 0, 0]]], [0], [3 * U], 1), [(3, 0, 0), (0, 0, 0)], [(-3, 0, 0), (0, 3, 0), (0, 0, -3)], None))
    cases.append((table_of([[[0, 0, 0]]], [0], [3 * U], 1), [(3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, 0, -3)], [(4, 0, 0), (3, 1, 0)], None))
    # d^2 == lo^2 is kept, one unit below it is not: a shell from 3 to 4 voxels
    cases.append((table_of([[[0, 0, 0]]], [3 * U], [4 * U], 1), [(3, 0, 0), (0, -3, 0), (0, 0, 4), (-4, 0, 0)], [(0, 0, 0), (2, 0, 0), (2, 2, 0)], None))
    cases.append((table_of([[[0, 1, 0]]], [3 * U], [4 * U], 1), [(0, -3, 0), (3, 0, 0)], [(0, 3, 0), (0, -4, 0)], None))
    # the seam: a ball round t = -1/2 that ends exactly on index n/2 - 1 (t = n/2 - 1) and on index n/2 (t = -n/2), per axis
    for axis in range(3):
        c = [0, 0, 0]
        c[axis] = -U // 2
        ends = []
        for t in (half - 1, -half, -1, 0):
            v = [0, 0, 0]
            v[axis] = t
            ends.append(tuple(v))
        off = [1, 1, 1]
        off[axis] = half - 1
        cases.append((table_of([[c]], [0], [(half - 1) * U + U // 2], 1), ends, [tuple(off)], None))
    # a centre outside the grid: nothing is allowed
    cases.append((table_of([[[n * U, 0, 0]]], [0], [2 * U], 1), [], [(half - 1, 0, 0), (0, 0, 0)], 0))
    # two overlapping balls, need 2: the lens; need 1: the union
    two = [[[-U, 0, 0], [2 * U, 0, 0]]]
    cases.append((table_of(two, [0, 0], [2 * U, 2 * U], 2), [(0, 0, 0), (1, 0, 0)], [(-1, 0, 0), (2, 0, 0), (-3, 0, 0)], None))
    cases.append((table_of(two, [0, 0], [2 * U, 2 * U], 1), [(-3, 0, 0), (4, 0, 0), (0, 0, 0)], [(-4, 0, 0), (5, 0, 0)], None))
    # |c| at its limit, hi = floor(sqrt(3) 2^20): the origin is just outside (d^2 = 3 2^40 > hi^2), one voxel towards the centre
    # is inside
    lim = rs.MAX_CENTRE
    far = int(np.floor(np.sqrt(3.0) * lim))
    cases.append((table_of([[[lim, -lim, lim]]], [0], [far], 1), [(1, -1, 1), (half - 1, -half, half - 1)],
                  [(0, 0, 0), (-1, 0, 0), (0, 1, 0), (-half, half - 1, -half)], None))
    V = _negative(n, n)
    for k, (table, inside, outside, count) in enumerate(cases):
        for inplace in (False, True):
            got = run_restrain(lib, device, V, table, (0,), inplace=inplace)[0]
            assert (bits(got) == bits(restrain_oracle(V[0], table, 0))).all(), (n, k, inplace)
        for t in inside:
            assert got[_index(t, n)] < 0, (n, k, t)
        for t in outside:
            assert bits(got)[_index(t, n)] == 0, (n, k, t)
        if count is not None:
            assert int((got < 0).sum()) == count, (n, k)
        else:
            assert 0 < int((got < 0).sum()) < n ** 3


def check_restrain_on_the_device(lib, device, n, nb=3, J=4):
    """Guarded allocations, a NaN-filled output, sizes of the real grids; one rotation fully by the oracle, the others by
    sampled voxels."""
    from guard_alloc import GuardedAllocations
    rng = np.random.RandomState(n)
    V = xc.volumes("normal", nb, n, n + J)
    c = np.rint(U * rng.uniform(-n / 2 + 8, n / 2 - 9, size=(7, 1, 3)) + U * rng.uniform(-3, 3, size=(7, J, 3)))
    table = table_of(c, [0, 2 * U, 0, U], np.rint(U * rng.uniform(6.0, 9.0, size=J)), 2)
    ids = ROT_IDS[3]
    with GuardedAllocations(empty_byte=0xFF) as g:
        Vd = torch.empty(nb, n * n * n, dtype=torch.float32, device=device)
        Vs = torch.empty(nb, n * n * n, dtype=torch.float32, device=device)
        Vd.copy_(torch.from_numpy(V).reshape(nb, -1))
        cd, bd = torch.from_numpy(table.centres.copy()).to(device), torch.from_numpy(table.bounds.copy()).to(device)
        idd = torch.tensor(ids, dtype=torch.int32, device=device)
        rc = lib.call("dlpd_topk_restrain", Vd.data_ptr(), Vs.data_ptr(), nb, n, idd.data_ptr(), cd.data_ptr(), bd.data_ptr(), J, 2,
                      0, 0, _stream(device))
        assert rc == 0
        bad = g.check(release=False)
        got = Vs.cpu().numpy().reshape(nb, n, n, n)
        g.check()
    assert not bad, bad
    want = restrain_oracle(V[0], table, ids[0])
    assert (bits(got[0]) == bits(want)).all()
    assert (got[0] < 0).any() and ((V[0] < 0) & (got[0] == 0)).any()
    t = signed_axis(n)
    for b in range(1, nb):
        neg = got[b] < 0
        assert neg.any()
        assert (bits(got[b])[neg] == bits(V[b])[neg]).all() and (bits(got[b])[~neg & (V[b] < 0)] == 0).all()
        assert (bits(got[b])[V[b] >= 0] == bits(V[b])[V[b] >= 0]).all()
        p = np.concatenate([np.argwhere(neg)[::37], rng.randint(0, n, size=(3000, 3))])          # kept voxels and any voxels
        ok = rs.allowed(table, ids[b], t[p])
        assert (ok[V[b][tuple(p.T)] < 0] == neg[tuple(p.T)][V[b][tuple(p.T)] < 0]).all()


# ----------------------------------------------------------------------------------------------------------------------
# the candidate lists
# ----------------------------------------------------------------------------------------------------------------------

def _key_of(flat_scores, ids):
    return (f2key(flat_scores[ids]) << np.uint64(32)) | ids.astype(np.uint64)


def run_restrain_cand(lib, device, V, table, rot_ids, keys, count, cap, tau):
    """-> (keys, count) after the call.  tau: None (a null pointer) or the u32 the pointer points to."""
    nb, n = V.shape[0], V.shape[1]
    kd = torch.from_numpy(keys.view(np.int64).copy()).to(device)
    cd = torch.from_numpy(count.copy()).to(device)
    Vd = torch.from_numpy(V.copy()).to(device)
    cen, bnd = torch.from_numpy(table.centres.copy()).to(device), torch.from_numpy(table.bounds.copy()).to(device)
    ids = torch.tensor(list(rot_ids), dtype=torch.int32, device=device)
    td = None if tau is None else torch.from_numpy(np.array([tau, 0, 0, 0], dtype=np.uint32).view(np.int32).copy()).to(device)
    rc = lib.call("dlpd_topk_restrain_cand", Vd.data_ptr(), nb, n, ids.data_ptr(), cen.data_ptr(), bnd.data_ptr(), table.J,
                  table.need, 0 if td is None else td.data_ptr(), kd.data_ptr(), cd.data_ptr(), cap, _stream(device))
    _sync(device)
    assert rc == 0 and (bits(Vd.cpu().numpy()) == bits(V)).all()
    return kd.cpu().numpy().view(np.uint64), cd.cpu().numpy()


def check_restrain_cand(lib, device, n=20):
    """Lists 0, 4: complete (4 with equal scores side by side); 1: flagged; 2, 5: overflowed; 3: empty.  Two balls with a large
    overlap and need 1, so the cubes a rebuild walks share most of their voxels."""
    rng = np.random.RandomState(5)
    nb, rot_ids = 6, (4, 1, 7, 0, 9, 3)
    for cap in (64, 4096):
        V = xc.volumes("normal", nb, n, 80 + cap)
        V[4].reshape(-1)[:40] = np.float32(-1.25)
        flat = V.reshape(nb, -1)
        p = rng.uniform(-2.0, 1.0, size=(10, 1, 3))
        c = np.rint(U * (p + np.array([[0.0, 0.0, 0.0], [1.5, -1.0, 0.5]])[None]))
        table = table_of(c, [0, U], [int(8.5 * U), int(8.0 * U)], 1)
        big = table_of(c, [0, 0], [int(13.5 * U), int(13.0 * U)], 1)
        ok = [allowed_volume(table, rid, n).reshape(-1) for rid in rot_ids]
        lists = []
        for b in range(nb):
            bound = np.sort(flat[b])[40 if cap == 64 else 1500]
            lists.append(rng.permutation(np.nonzero(flat[b] <= bound)[0]))
        lists[3] = lists[3][:0]
        keys = np.full((nb, cap), 0x5555555555555555, dtype=np.uint64)
        count = np.zeros(2 * nb, dtype=np.int32)
        for b, ids in enumerate(lists):
            keys[b, :len(ids)] = _key_of(flat[b], ids)
            count[b] = len(ids)
        count[nb + 1] = 1                                                 # list 1: flagged
        count[2], count[5] = cap + 7, 3 * cap                             # over the cap (K3 counts on, stores cap keys)
        # tau: the list's K-th score.  The shallow one leaves at most cap allowed voxels below it, the deep one more than cap
        order = np.sort(flat, axis=1)
        tau_few = int(f2key(order[:, 100 if cap == 64 else 4000]).min())
        tau_many = int(f2key(order[:, -1]).max())

        def thinned(k2, c2):
            assert (c2[nb:] == count[nb:]).all()                         # flags left alone
            for b in (1, 3):
                assert c2[b] == count[b] and (k2[b] == keys[b]).all()    # flagged, empty: untouched
            for b in (0, 4):
                want = keys[b, :len(lists[b])][ok[b][lists[b]]]
                assert 0 < len(want) < len(lists[b]) and c2[b] == len(want)          # counts are lowered
                assert (k2[b, :len(want)] == want).all()                 # the survivors, in list order
        for tau in (None, 0):                                            # no rebuild: the overflowed lists are untouched
            k2, c2 = run_restrain_cand(lib, device, V, table, rot_ids, keys, count, cap, tau)
            thinned(k2, c2)
            for b in (2, 5):
                assert c2[b] == count[b] and (k2[b] == keys[b]).all()
        k2, c2 = run_restrain_cand(lib, device, V, table, rot_ids, keys, count, cap, tau_few)
        thinned(k2, c2)
        for b in (2, 5):
            ids = np.nonzero(ok[b] & (f2key(flat[b]) <= np.uint64(tau_few)))[0]
            assert 0 < len(ids) <= cap and c2[b] == len(ids), (cap, b, len(ids))     # rebuilt: complete, the count set
            got = np.sort(k2[b, :len(ids)])
            assert len(np.unique(got)) == len(got) and (got == np.sort(_key_of(flat[b], ids))).all()
        # the volume kernel, run with these counts, writes the rows of the flagged list only
        Vs = run_restrain(lib, device, V, table, rot_ids, ccount=c2, cap=cap)
        for b in range(nb):
            if b == 1:
                assert (bits(Vs[b]) == bits(restrain_oracle(V[b], table, rot_ids[b]))).all()
            else:
                assert (bits(Vs[b]) == NAN_BITS).all()                   # poison kept
        # more than cap allowed voxels below tau: the list stays over the cap, and the volume kernel writes its row
        wide = big if cap == 4096 else table
        k3, c3 = run_restrain_cand(lib, device, V, wide, rot_ids, keys, count, cap, tau_many)
        for b in (2, 5):
            assert int((allowed_volume(wide, rot_ids[b], n).reshape(-1) & (f2key(flat[b]) <= np.uint64(tau_many))).sum()) > cap
            assert c3[b] == count[b]
        assert (c3[nb:] == count[nb:]).all() and c3[1] == count[1] and c3[3] == 0
        Vs = run_restrain(lib, device, V, wide, rot_ids, ccount=c3, cap=cap)
        for b in (2, 5):
            assert (bits(Vs[b]) == bits(restrain_oracle(V[b], wide, rot_ids[b]))).all()
        if cap == 4096:
            assert max(len(lists[b]) for b in (0, 4)) > 512              # more than one round of the block


def check_zero_fill(lib, device, n=10, K=16):
    """Fewer allowed negatives than K: the select on restrain(V) gives the oracle's zero-fill (DeviceTopList.select, no cset)."""
    rng = np.random.RandomState(4)
    table = table_of(np.rint(U * rng.uniform(-2, 1, size=(7, 1, 3))), [0], [int(2.5 * U)], 1)
    ids = ROT_IDS[3]
    V = np.abs(rng.standard_normal((3, n, n, n))).astype(np.float32) + np.float32(0.5)
    for b, rid in enumerate(ids):
        ok = allowed_volume(table, rid, n)
        inside, outside = np.argwhere(ok), np.argwhere(~ok)
        for q in inside[rng.permutation(len(inside))[:4]]:
            V[(b,) + tuple(q)] = -np.float32(rng.rand() + 0.1)
        for q in outside[rng.permutation(len(outside))[:30]]:            # more negatives than K, but not allowed
            V[(b,) + tuple(q)] = -np.float32(rng.rand() + 0.1)
    V[1, 0, 0, 1] = np.float32(-0.0)
    V[2, n - 1, n - 1, n - 1] = np.float32(0.0)
    top = DeviceTopList(K, 3, device, lib)
    top.set_restraints(table)
    sc, idx = top.select(torch.from_numpy(V).to(device).reshape(3, -1), 3, None, torch.tensor(ids, dtype=torch.int32, device=device))
    _sync(device)
    sc, idx = sc.cpu().numpy(), idx.cpu().numpy()
    for b, rid in enumerate(ids):
        wi, ws = orc.rotation_picks_fast(restrain_oracle(V[b], table, rid), K)
        assert 0 < int((ws < 0).sum()) <= 4 and int((V[b] < 0).sum()) > K            # (the two planted zeros may have taken one)
        assert (idx[b] == wi).all() and (bits(sc[b]) == bits(ws)).all(), b


# ----------------------------------------------------------------------------------------------------------------------
# errors
# ----------------------------------------------------------------------------------------------------------------------

def check_errors(lib, device):
    n, nb, cap = 8, 2, 64
    table, _ = clustered_table(3, 2, 1, n, 1)
    V = torch.from_numpy(xc.volumes("normal", nb, n, 3)).to(device)
    Vs = torch.full((nb, n ** 3), -7.0, dtype=torch.float32, device=device)
    keys = torch.full((nb, cap), -7, dtype=torch.int64, device=device)
    count = torch.tensor([3, 3, 0, 0], dtype=torch.int32, device=device)
    cen, bnd = torch.from_numpy(table.centres.copy()).to(device), torch.from_numpy(table.bounds.copy()).to(device)
    ids = torch.tensor([2, 0], dtype=torch.int32, device=device)
    tau = torch.tensor([-5, 0, 0, 0], dtype=torch.int32, device=device)
    st = _stream(device)

    def vol(V_=V.data_ptr(), Vs_=Vs.data_ptr(), nb_=nb, n_=n, ids_=ids.data_ptr(), c=cen.data_ptr(), b=bnd.data_ptr(), J=2, need=1):
        return lib.call("dlpd_topk_restrain", V_, Vs_, nb_, n_, ids_, c, b, J, need, 0, 0, st)

    def cand(V_=V.data_ptr(), nb_=nb, n_=n, ids_=ids.data_ptr(), c=cen.data_ptr(), b=bnd.data_ptr(), J=2, need=1, k=keys.data_ptr(),
             cc=count.data_ptr(), cap_=cap):
        return lib.call("dlpd_topk_restrain_cand", V_, nb_, n_, ids_, c, b, J, need, tau.data_ptr(), k, cc, cap_, st)
    common = (dict(n_=7), dict(n_=9), dict(J=0), dict(J=33), dict(J=-1), dict(need=0), dict(need=3), dict(nb_=0), dict(nb_=-2),
              dict(V_=0), dict(ids_=0), dict(c=0), dict(b=0))
    for fn, cases in ((vol, common + (dict(Vs_=0),)),
                      (cand, common + (dict(k=0), dict(cc=0), dict(cap_=63), dict(cap_=8193), dict(cap_=0)))):
        for kw in cases:
            with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
                fn(**kw)
    for fn in (vol, cand):
        for big in (1292, 2000, 1 << 30):
            with pytest.raises(RuntimeError, match="UNSUPPORTED"):
                fn(n_=big)                                                # (refused before anything is read)
    _sync(device)
    assert (Vs == -7.0).all() and (keys == -7).all() and count.tolist() == [3, 3, 0, 0]      # nothing was written
    top = DeviceTopList(4, 1, device, lib)
    top.set_restraints(table)
    one = torch.tensor([0], dtype=torch.int32, device=device)
    with pytest.raises(RuntimeError, match="cubic"):
        top.select(torch.zeros(1, 12, dtype=torch.float32, device=device), 1, None, one)
    with pytest.raises(RuntimeError, match="even side"):
        top.select(torch.zeros(1, 27, dtype=torch.float32, device=device), 1, None, one)
    with pytest.raises(RuntimeError, match="rot_ids"):
        top.select(torch.zeros(1, 64, dtype=torch.float32, device=device), 1)
    assert vol() == 0 and cand() == 0


# ----------------------------------------------------------------------------------------------------------------------
# the host side
# ----------------------------------------------------------------------------------------------------------------------

def check_table_by_hand():
    R = np.stack([np.eye(3), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])])      # identity; 90 degrees about z
    r1 = rs.Restraint([5.0, 0.0, -2.5], [1.25, 2.5, 0.0], dmax=10.0, dmin=2.5)
    r2 = rs.Restraint([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], dmax=0.0)
    t = rs.restraint_table(R, [r1, r2], 1.25)
    assert t.J == 2 and t.need == 2 and t.nrot == 2 and t.centres.dtype == np.int32 and t.bounds.dtype == np.int64
    # rotation 0: (b - a) / 1.25 = (3, -2, -2) voxels; rotation 1: R a = (-2.5, 1.25, 0), (b - R a) / 1.25 = (6, -1, -2)
    assert t.centres.tolist() == [[[768, -512, -512], [0, 0, 0]], [[1536, -256, -512], [0, 0, 0]]]
    assert t.bounds.tolist() == [512 ** 2, 0, 2048 ** 2, 0]
    assert rs.restraint_table(R, [r1, r2], 1.25, need=1).need == 1
    # rounding at .5 goes to the even integer: 256 x / res = k + 0.5 for x = (k + 0.5) / 256 voxels
    for k, want in ((0, 0), (1, 2), (2, 2), (3, 4), (-1, 0), (-2, -2), (-3, -2)):
        tt = rs.restraint_table(np.eye(3)[None], [rs.Restraint([(k + 0.5) / 256.0, 0, 0], [0, 0, 0], dmax=(2.5 + k % 2) / 256.0)], 1.0)
        assert tt.centres[0, 0, 0] == want, (k, tt.centres[0, 0, 0])
    assert rs.restraint_table(np.eye(3)[None], [rs.Restraint([0, 0, 0], [0, 0, 0], dmax=2.5 / 256.0, dmin=0.5 / 256.0)], 1.0).bounds.tolist() == [0, 4]
    # allowed(): the definition on signed translations
    assert rs.allowed(t, 0, np.array([3, -2, -2])).item() is False                  # d = 0 < dmin of r1
    one = rs.restraint_table(R, [r1], 1.25)
    assert rs.allowed(one, 0, np.array([[5, -2, -2], [3, 6, -2], [3, -2, -10], [3, -2, -11], [4, -2, -2]])).tolist() == \
        [True, True, True, False, False]
    assert rs.satisfied(t, np.array([0, 1]), np.array([[0, 0, 0], [0, 0, 0]])).tolist() == [2, 2]
    assert t.cube_volume() == 17 ** 3 + 1
    # limits
    for bad in (dict(dmax=-1.0), dict(dmax=1.0, dmin=2.0), dict(dmax=float("inf")), dict(dmax=float("nan"))):
        with pytest.raises(ValueError, match="dmin"):
            rs.Restraint([0, 0, 0], [0, 0, 0], **bad)
    with pytest.raises(ValueError, match="1..32"):
        rs.restraint_table(R, [], 1.25)
    with pytest.raises(ValueError, match="1..32"):
        rs.restraint_table(R, [r2] * 33, 1.25)
    for need in (0, 3):
        with pytest.raises(ValueError, match="restraints_needed"):
            rs.restraint_table(R, [r1, r2], 1.25, need=need)
    with pytest.raises(ValueError, match="centre"):
        rs.restraint_table(R, [rs.Restraint([6000.0, 0, 0], [0, 0, 0], dmax=1.0)], 1.25)
    rs.restraint_table(R, [rs.Restraint([5120.0, 0, 0], [0, 0, 0], dmax=1.0)], 1.25)          # 4096 voxels: the limit itself
    with pytest.raises(ValueError, match="dmax"):
        rs.restraint_table(R, [r2, rs.Restraint([0, 0, 0], [0, 0, 0], dmax=10241.0)], 1.25)
    rs.restraint_table(R, [rs.Restraint([0, 0, 0], [0, 0, 0], dmax=10240.0)], 1.25)


def check_select_point(tmp_path):
    from deeplocalproteindocking_amd.Utils.FullAtom import read_pdb_atoms
    from synth_pdb import write_protein_like_pdb
    f = str(tmp_path / "p.pdb")
    write_protein_like_pdb(f, 8, seed=3)
    xyz, chains, _, resnums, names = read_pdb_atoms(f)
    chain, resnum = chains[0], int(resnums[0])
    sel = "%s:%d" % ("_" if chain == " " else chain, resnum)
    res = np.array([c == chain and int(r) == resnum for c, r in zip(chains, resnums)])
    ca = np.nonzero(res & (np.array(names) == "CA"))[0][0]
    assert (rs.select_point(f, sel) == xyz[ca]).all() and (rs.select_point(f, sel + ":CA") == xyz[ca]).all()
    other = [nm for nm, r in zip(names, res) if r and nm != "CA"][0]
    assert (rs.select_point(f, sel + ":" + other) == xyz[np.nonzero(res & (np.array(names) == other))[0][0]]).all()
    assert np.allclose(rs.select_point(f, sel + ":*"), xyz[res].mean(axis=0), rtol=0, atol=1e-12)
    g = str(tmp_path / "blank.pdb")                                      # the same file with blank chain identifiers
    with open(g, "w") as out:
        for line in open(f):
            out.write(line[:21] + " " + line[22:] if line.startswith("ATOM") else line)
    x2, c2, _, r2, n2 = read_pdb_atoms(g)
    hit = np.nonzero(np.array([int(r) == resnum for r in r2]) & (np.array(n2) == "CA"))[0][0]
    assert set(c2) == {" "} and (rs.select_point(g, "_:%d" % resnum) == x2[hit]).all()
    for bad, what in (("Q:%d" % resnum, "Q:"), ("%s:99999" % sel.split(":")[0], "99999"), (sel + ":XX", "XX"), ("A", "'A'"),
                      (sel.split(":")[0] + ":x", ":x"), (":5", ":5")):
        with pytest.raises(ValueError) as err:
            rs.select_point(f, bad)
        assert what in str(err.value) and bad in str(err.value), (bad, str(err.value))


# ----------------------------------------------------------------------------------------------------------------------
# the engine, driven by hand
# ----------------------------------------------------------------------------------------------------------------------

L, NROT, BATCH = xc.L, xc.NROT, xc.BATCH
RES = 1.25


def engine_restraints(two=True):
    """The deep scores of ``exclusion_checks.engine_case`` lie 7 to 25 voxels from t = 0, where the ligand block meets the
    receptor (nearer, the clash mask leaves zeros).  So: a shell of 11 .. 17 voxels round a centre next to t = 0, and a ball of 9
    voxels whose centre lies in that shell; ``need`` 1 asks for the union, 2 for the lens."""
    out = [rs.Restraint([1.0, 0.5, -1.0], [0.5, -0.3, 0.2], dmax=17 * RES, dmin=11 * RES)]
    if two:
        out.append(rs.Restraint([15.0, 1.0, 0.0], [-0.4, 0.2, 0.6], dmax=9 * RES))
    return out


def small_restraints():
    """Two balls of 1.9 voxels (about 30 voxels each) in that shell: however many voxels share the clipped minimum score, at most
    64 of them are allowed, so an overflowed list of cap 64 is always rebuilt."""
    return [rs.Restraint([15.0, 1.0, 0.0], [-0.4, 0.2, 0.6], dmax=1.9 * RES), rs.Restraint([-9.0, 1.5, 5.0], [0.5, -0.3, 0.2], dmax=1.9 * RES)]


class Spy(object):
    """The library, remembering every call's name."""

    def __init__(self, inner):
        self.inner, self.names = inner, []

    def call(self, name, *args):
        self.names.append(name)
        return self.inner.call(name, *args)

    def __getattr__(self, name):
        return getattr(self.inner, name)


def _real_lib(lib):
    if lib is None:
        from deeplocalproteindocking_amd._lib import get_lib
        lib = get_lib()
    return lib


def make_engine(lib, device, case, K, table, r=0, batch=BATCH, cap=None, **kw):
    rec, recf, lig, ligf, R, filt = case
    extent = kw.get("extent")
    thr = 0.3 * (extent or L) ** 3
    eng = DockingEngine(L, rec.shape[0], *filt, clip=5.0, threshold_clash=thr, max_conf=K, batch=batch, device=device, lib=lib,
                        exclusion=r, restraints=table, **kw)
    if cap is not None:
        eng.top.CAND_CAP = cap
    eng.set_receptor(rec, recf)
    eng.set_ligand(lig, ligf)
    return eng


def drive(eng, R, table, r=0, oracle=True):
    """score_batch / select_batch / merge_batch by hand -> (the engine's entries, the list expected from the engine's own V,
    {"complete", "rebuilt", "full"}: rotations seen on each selection path, n of the grid the top-K works on)."""
    dev = eng.device
    eng.reset_top()
    assert eng.top.exclusion == r and eng.top.restraints is table
    cset = eng.top.new_candidate_set() if eng.prefilter else None
    seen, free, paths = [], [], {"complete": 0, "rebuilt": 0, "full": 0}
    n = eng.N
    for beg in range(0, R.shape[0], eng.batch):
        Rb = R[beg:beg + eng.batch].to(dev).contiguous()
        nb = Rb.shape[0]
        V = eng.score_batch(Rb, cset=cset)
        used = eng._cset_used if cset is not None else None
        G = eng.gather_window(V, nb) if eng.window is not None else V.reshape(nb, -1)
        n = int(round(G.shape[1] ** (1.0 / 3.0)))
        Gh = G.cpu().numpy().reshape(nb, n, n, n).copy()
        before = None if used is None else used["count"].cpu().numpy().copy()
        ids = torch.arange(beg, beg + nb, dtype=torch.int32, device=dev)
        if used is not None and table is not None:                       # the counts as restrain_cand leaves them
            rid, cen, bnd = ids.data_ptr(), eng.top._rst[0].data_ptr(), eng.top._rst[1].data_ptr()
            probe_k, probe_c = used["keys"].clone(), used["count"].clone()
            eng.lib.call("dlpd_topk_restrain_cand", V.data_ptr(), nb, n, rid, cen, bnd, table.J, table.need, eng.top.tau.data_ptr(),
                         probe_k.data_ptr(), probe_c.data_ptr(), used["cap"], _stream(dev))
            after = probe_c.cpu().numpy()
            flags, c0, c1, cap = before[eng.batch:eng.batch + nb], before[:nb], after[:nb], used["cap"]
            paths["complete"] += int(((flags == 0) & (c0 <= cap)).sum())
            paths["rebuilt"] += int(((flags == 0) & (c0 > cap) & (c1 <= cap)).sum())
            paths["full"] += int(((flags != 0) | (c1 > cap)).sum())
        else:
            paths["full"] += nb
        eng.select_batch(V, nb, used, ids)
        eng.merge_batch(ids, nb)
        if oracle:
            for i in range(nb):
                Vo = xc.suppress_oracle(Gh[i], r) if r else Gh[i]
                seen.append((beg + i, restrain_oracle(Vo, table, beg + i) if table is not None else Vo))
                free.append((beg + i, Vo))
    got = eng.top_entries()
    if cset is not None:
        assert (cset["count"] == 0).all()                                # consumed
    eng.free_expected = expected_entries(free, eng.K) if oracle else None          # the unrestrained list of the same volumes
    return got, (expected_entries(seen, eng.K) if oracle else None), paths, n


def assert_negatives_allowed(entries, table, n):
    rot, idx, score, _ = entries
    neg = score < 0
    t = signed_axis(n)
    xyz = np.stack(orc.flat_to_xyz(idx[neg], n), axis=1)
    assert neg.any() and rs.allowed(table, rot[neg], t[xyz]).all()


def check_engine(lib, device, K, res, need, C=2, cap=None, r=0, prefilter=True, nrot=8, seen=None):
    case = xc.engine_case(C, 11 + C)
    R = case[4][:nrot]
    table = rs.restraint_table(case[4], res, RES, need)
    eng = make_engine(lib, device, case, K, table, r=r, cap=cap, prefilter=prefilter)
    assert eng.switches()["restraints"] == (len(res), need) and eng.switches()["exclusion"] == r and eng.prefilter == prefilter
    got, want, paths, n = drive(eng, R, table, r=r)
    print("need %d, K %d, cap %s, exclusion %d, prefilter %s: %s, %d negative entries" %
          (need, K, cap, r, prefilter, paths, int((got[2] < 0).sum())))
    assert_same_entries(got, want)
    assert_negatives_allowed(got, table, n)
    if r:
        xc.assert_apart(got, n, r)
    free = eng.free_expected
    assert (got[1] != free[1]).any() or (got[0] != free[0]).any()        # not the unrestrained list of the same volumes
    if seen is not None:
        for k, v in paths.items():
            seen[k] = seen.get(k, 0) + v
    return paths, got


_BASE = {}


def check_engine_paths(lib, device):
    """Complete lists, overflowing lists (cap 64), no prefilter, with an exclusion radius: across the cases every selection path
    -- complete (thinned), rebuilt, full -- was taken."""
    seen = {}
    p, _ = check_engine(lib, device, 16, engine_restraints(), 2, seen=seen)
    assert p["complete"] >= 1 and p["full"] >= 1 and p["rebuilt"] == 0
    p, got = check_engine(lib, device, 16, small_restraints(), 1, cap=64, seen=seen)
    assert p["rebuilt"] >= 1 and p["full"] >= 1 and p["complete"] == 0
    _BASE[id(lib)] = got
    p, _ = check_engine(lib, device, 16, engine_restraints(), 1, prefilter=False, nrot=4, seen=seen)
    assert p["complete"] == 0 and p["rebuilt"] == 0
    check_engine(lib, device, 16, small_restraints(), 1, cap=64, r=1, seen=seen)
    assert seen["complete"] >= 1 and seen["rebuilt"] >= 1 and seen["full"] >= 1, seen


def check_engine_search(lib, device, K=16):
    """The pipelined search() at launch batches 3 and 8, with and without the rebuild, gives the hand-driven list (that of
    check_engine_paths' cap-64 case, made here when that check has not run)."""
    case = xc.engine_case(2, 13)
    table = rs.restraint_table(case[4], small_restraints(), RES, 1)
    base = _BASE.get(id(lib))
    if base is None:
        base = drive(make_engine(lib, device, case, K, table, cap=64), case[4][:8], table, oracle=False)[0]
    for batch, limit in ((3, DeviceTopList.REBUILD_LIMIT), (8, None)):
        eng = make_engine(lib, device, case, K, table, batch=batch, cap=64)
        eng.top.REBUILD_LIMIT = limit
        eng.reset_top()
        eng.search(case[4][:8])
        assert_same_entries(eng.top_entries(), base)


def check_engine_embedded(lib, device, K=16, inner=12):
    case = xc.engine_case(2, 31, inner=inner)
    table = rs.restraint_table(case[4], engine_restraints(), RES, 1)
    eng = make_engine(lib, device, case, K, table, extent=inner, center=inner / 2.0)
    assert eng.window is not None and not eng.prefilter
    got, want, _, n = drive(eng, case[4][:8], table)
    assert n == 2 * inner
    assert_same_entries(got, want)
    assert_negatives_allowed(got, table, n)


# ----------------------------------------------------------------------------------------------------------------------
# Docker: update_top, the unfused loop, a live engine, two ranks, the script
# ----------------------------------------------------------------------------------------------------------------------

def check_update_top(lib, device, n=10, K=12):
    from deeplocalproteindocking_amd.Docker import Docker
    R = np.stack([np.eye(3), np.diag([1.0, -1.0, -1.0])])
    res = [rs.Restraint([1.0, -1.0, 0.5], [0.5, 1.0, 0.0], dmax=3.0)]
    for r in (0, 1):
        dk = Docker(None, box_size=n // 2, resolution=1.0, max_conf=K, rotations=R, device=device, lib=lib, exclusion=r, restraints=res)
        table = dk.restraint_table()
        want = []
        for rid in (0, 1):
            Vh = xc.volumes("normal", 1, n, 50 + rid)[0]
            V = torch.from_numpy(Vh.copy()).to(device)
            dk.update_top(V, rid)
            Vo = torch.from_numpy(restrain_oracle(xc.suppress_oracle(Vh, r) if r else Vh, table, rid))
            picks = orc.update_top([], Vo.clone(), rid, K)
            want = orc.update_top(want, Vo, rid, K)
            assert [e[:4] for e in dk.top_list] == [e[:4] for e in want]
            assert (bits([e[4] for e in dk.top_list]) == bits([e[4] for e in want])).all()
            Vexp = Vh.copy()                                             # the picked voxels are zero in V, no other changed
            for e in picks:
                Vexp[e[1], e[2], e[3]] = np.float32(0.0)
            assert (bits(V.cpu().numpy()) == bits(Vexp)).all()
        rep = dk.restraint_report()
        assert all(s == 1 for s, e in zip(rep, dk.top_list) if e[4] < 0) and sum(e[4] < 0 for e in dk.top_list) > 0
        # the report on list forms with their own matrices: the same counts; a fraction of a voxel moves a pose out
        as_refined = [(R[e[0]], dk.signed_translation(e[1], e[2], e[3]), e[4], i) for i, e in enumerate(dk.top_list)]
        assert (dk.restraint_report(as_refined) == rep).all()
        c = table.centres[0, 0] / 256.0
        edge = [(R[0], (c[0] + 3.0, c[1], c[2]), -1.0, 0), (R[0], (c[0] + 3.01, c[1], c[2]), -1.0, 0)]
        assert dk.restraint_report(edge).tolist() == [1, 0]
        dk.restraints = None
        with pytest.raises(RuntimeError, match="without restraints"):
            dk.restraint_report()


def check_docker_unfused(lib, device, box=12, K=16):
    import engine_reuse_checks as erc
    from deeplocalproteindocking_amd.Docker import Docker
    g = torch.Generator().manual_seed(3)
    rec, lig = torch.randn(1, 2, box, box, box, generator=g) * 0.1, torch.randn(1, 2, box, box, box, generator=g) * 0.1
    R = erc.rotations(5, 9).double().numpy()
    model = xc._UserModel()
    res = [rs.Restraint([2.0, 1.0, -3.0], [3.0, -2.0, 1.0], dmax=5.0), rs.Restraint([-20.0, 0.0, 0.0], [0.0, 0.0, 0.0], dmax=2.0)]
    dk = Docker(model, box_size=box, max_conf=K, rotations=R, device=device, lib=lib, restraints=res, restraints_needed=1)
    got = dk.dock_volumes([rec], [lig], write=False, model_batch=2)
    assert dk.path == "call" and dk.engine is None
    V = np.concatenate(model.seen)
    table = dk.restraint_table()
    want = expected_entries([(i, restrain_oracle(V[i], table, i)) for i in range(len(V))], K)
    assert got == DeviceTopList.to_top_list(want, 2 * box)
    assert sum(e[4] < 0 for e in got) > K // 2
    assert_negatives_allowed(want, table, 2 * box)
    assert all(s >= 1 for s, e in zip(dk.restraint_report(), got) if e[4] < 0)


def _restraints(k):
    return [engine_restraints(), [rs.Restraint([-4.0, 3.0, 1.0], [2.0, 2.0, -1.0], dmax=16 * RES, dmin=12 * RES)]][k]


def check_reuse_and_defaults(lib, device, K=16):
    """A live engine serves free -> restrained -> free -> another restraint set; each list is a fresh Docker's, the free lists
    those of a Docker built without the keywords -- and a free search never calls a restrain entry."""
    import engine_reuse_checks as erc
    R = erc.rotations(4, 8).double().numpy()
    pair = xc._volume_pair()
    spy = Spy(_real_lib(lib))
    live = xc._docker(spy, device, K, R)
    assert live.restraints is None and live.restraints_needed is None
    plans = (None, (_restraints(0), 1), None, (_restraints(1), None))
    lists, free_calls = [], None
    for plan in plans:
        live.restraints, live.restraints_needed = plan if plan else (None, None)
        seen = len(spy.names)
        lists.append(list(live.dock_volumes([pair[0]], [pair[1]], pair[2], pair[3], write=False)))
        called = spy.names[seen:]
        assert live.path == "fused"
        assert "dlpd_topk_select_cand" in called or "dlpd_topk_select" in called
        if plan is None:
            assert live.engine.switches()["restraints"] is None
            assert not [nm for nm in called if "restrain" in nm or "suppress" in nm]          # exactly today's calls
        else:
            assert live.engine.switches()["restraints"] == (len(plan[0]), plan[1] or len(plan[0]))
            assert "dlpd_topk_restrain" in called and "dlpd_topk_restrain_cand" in called
            neg = [e for e in lists[-1] if e[4] < 0]
            assert neg and all(s >= (plan[1] or len(plan[0])) for s, e in zip(live.restraint_report(), lists[-1]) if e[4] < 0)
        if plan is None:                                                 # ... one and the same sequence of them
            topk = [nm for nm in called if "topk" in nm and not nm.endswith("_bytes")]      # (sizes are asked once, at construction)
            assert free_calls in (None, topk)
            free_calls = topk
    for plan, got in zip(plans[1:], lists[1:]):                          # (the free list twice: one fresh engine for both)
        kw = dict(restraints=plan[0], restraints_needed=plan[1]) if plan else {}
        fresh = xc._docker(_real_lib(lib), device, K, R, **kw)
        assert fresh.dock_volumes([pair[0]], [pair[1]], pair[2], pair[3], write=False) == got and fresh.engine is not live.engine
    assert lists[0] == lists[2] and lists[1] != lists[0] and lists[3] != lists[0] and lists[3] != lists[1]


def check_two_ranks(lib, device, K=16):
    import engine_reuse_checks as erc
    R = erc.rotations(7, 12).double().numpy()
    pair = xc._volume_pair()
    kw = dict(restraints=_restraints(0), restraints_needed=1)
    one = xc._docker(lib, device, K, R, **kw)
    one.dock_volumes([pair[0]], [pair[1]], pair[2], pair[3], write=False)
    want = one.engine.top_entries()
    parts = []
    for rank in (0, 1):
        dk = xc._docker(lib, device, K, R, rank=rank, world_size=2, **kw)
        dk._gather = lambda entries: (parts.append(entries), entries)[1]          # (the collective's place: it does not change)
        dk.dock_volumes([pair[0]], [pair[1]], pair[2], pair[3], write=False)
        assert set(parts[-1][0].tolist()) <= set(dk.shard(len(R)).tolist()) and len(parts[-1][0]) == K
    assert_same_entries(DeviceTopList.merge_entries(parts, K), want)
    assert_negatives_allowed(want, one.restraint_table(), 2 * L)


def check_dock_pair(lib, device, tmp_path):
    """The script's search step (what ``--restraint`` reaches) on two synthetic PDB files, the receptor randomly rotated: every
    negative entry of the written list satisfies the restraint in the FILES' coordinates."""
    from synth_pdb import write_protein_like_pdb
    from test_atoms import _tiny_model
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend, read_pdb_atoms
    import engine_reuse_checks as erc
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import dock_pair
    assert dock_pair.parse_restraint_distance("8") == (8.0, 0.0) and dock_pair.parse_restraint_distance("10:8") == (10.0, 8.0)
    for bad in ("3:4", "-1", "inf"):
        with pytest.raises(ValueError, match="restraint"):
            dock_pair.parse_restraint_distance(bad)
    frec, flig = str(tmp_path / "r.pdb"), str(tmp_path / "l.pdb")
    write_protein_like_pdb(frec, 14, seed=5)
    write_protein_like_pdb(flig, 9, seed=6)
    K = 40
    R = erc.rotations(3, 2).double().numpy()
    dk = Docker(_tiny_model().to(device), box_size=L, resolution=1.25, max_conf=K, rotations=R, device=device, lib=lib,
                coords_backend=CoordsBackend(lib=lib), randomize_rot=True, rotation_seed=7)

    def sel_of(f, k):
        _, chains, _, resnums, _ = read_pdb_atoms(f)
        return "%s:%d" % ("_" if chains[k] == " " else chains[k], int(resnums[k]))
    spec = [(sel_of(frec, 0), sel_of(flig, -1), "12:2")]
    with torch.no_grad():
        p = dk.prepare(frec, flig, "SE3")
        out = str(tmp_path / "free.dat")
        dk.new_log(out)
        free = list(dock_pair.search(dk, frec, flig, "SE3", 2, prepared=p))
        dk.cleanup()
        assert dk.restraints is None
        out = str(tmp_path / "pair.dat")
        dk.new_log(out)
        got = list(dock_pair.search(dk, frec, flig, "SE3", 2, prepared=p, restraints=spec))
        dk.cleanup()
    assert len(dk.restraints) == 1 and got != free and len(got) == K
    rep = dk.restraint_report()
    neg = [i for i, e in enumerate(got) if e[4] < 0]
    assert neg and all(rep[i] == 1 for i in neg)
    # in file coordinates: the written line holds R and the translation in the receptor's ORIGINAL frame (randR undone); the
    # ligand atom, moved as the .dat says, lies within [2, 12] A of the receptor atom.  Slack 0.01 A: the centre is rounded to
    # 1/256 voxel (at most sqrt(3) / 2 units = 0.0042 A at 1.25 A), a bound to half a unit (0.0024 A), and the twelve %f
    # columns carry 5e-7 each (times a 40 A lever: 1e-4 A)
    rows = np.loadtxt(out).reshape(-1, 13)
    a = rs.select_point(flig, spec[0][1]) + np.asarray(p.ligand_shift, dtype=np.float64).reshape(3)
    b = rs.select_point(frec, spec[0][0]) + np.asarray(p.receptor_shift, dtype=np.float64).reshape(3)
    for i in neg:
        Rm, t = rows[i, :9].reshape(3, 3), rows[i, 9:12]
        d = np.linalg.norm(Rm @ a + t - b)
        assert 2.0 - 0.01 <= d <= 12.0 + 0.01, (i, d)
    far = [np.linalg.norm(rows_f[:9].reshape(3, 3) @ a + rows_f[9:12] - b) for rows_f in np.loadtxt(str(tmp_path / "free.dat")).reshape(-1, 13)]
    assert max(far) > 12.5 or min(far) < 1.5                            # the free list does not keep to it
    with pytest.raises(ValueError, match="restraints-needed"):
        dock_pair.set_restraints(dk, p, spec, needed=2)
    with pytest.raises(ValueError, match="no residue"):
        dock_pair.set_restraints(dk, p, [("Q:1", spec[0][1], "8")])
