"""Check bodies of the pose clustering (csrc/dlpd_cluster.h, ops.pose_*, Docker.cluster), shared by tests/test_cluster_emu.py
(the CPU-emulated kernels) and tests/test_cluster_gpu.py (the gfx950 build).  Nothing here reads the reference tree: the step
is build-defined.

THE TRUTH is float64 with explicit atoms: X_p = x R_p^T + t_p, d(i, j)^2 = sum_k w_k |X_i[k] - X_j[k]|^2, differenced directly
(``rmsd64``); the greedy reference (``greedy64``) is written from the definition on that matrix, not from the embedding:
pose i is a centre iff no earlier centre lies within the radius (d <= r), every other pose joins the first centre within the
radius, after ``m`` centres no new one is made and a pose none of them covers gets -1.

THE GENERATOR (``atoms``, ``poses``): atoms normal with sigma (9, 6, 4) Angstrom, re-centred on their bounding box; ``ns`` seed
poses (a random rotation, a translation on the 1.25 Angstrom grid within +-24 voxels); every pose a seed times a rotation
vector N(0, 4 degrees) per component, plus a shift of +-3 voxels.

TOLERANCE OF A DISTANCE (derived, not tuned).  u = 2^-24.  The embedding e (12 floats, |e_k| <= M) is rounded to float32:
each component moves by at most u M; the float32 difference of two components adds a relative u.  For the difference vector
delta (|delta| = d): |delta~ - delta| <= 2 sqrt(12) u M + u d.  The 12-term fma chain (each partial sum of non-negative terms
rounded once: relative 12 u on d^2, i.e. 6 u on d) and the root (u / 2, plus its own rounding u) add less than 7 u d.  So
|D32 - D64| <= u (7 M + 8 d)   (2 sqrt(12) < 7), and the tests allow TWICE that: 2^-23 (7 M + 8 d).

THE RADIUS OF A PREDICATE TEST (a condition on the inputs, checked on the truth alone).  The kernel's bit is d32^2 <= r32^2;
it equals the float64 predicate d <= r whenever no pair distance lies within the error band of r.  ``tuned_radius`` moves the
nominal radius to the middle of the widest gap between consecutive sorted pair distances within +-0.05 Angstrom of it (the
ends of that window count as distances: a gap they bound is no wider than the true one) and asserts half the gap
>= 2^-22 (7 M + 8 r): twice the distance bound above, which also covers the rounding of r and of r^2 (relative u each).

PLANTED SETS (any K, no K^2 reference): ``ns`` seed poses pairwise more than 3 r apart, every member within r / 4 of its seed,
both asserted in float64 on the atoms at cost O(K + ns^2).  Members of one seed are then within r / 2 of each other and
members of two seeds more than 2.5 r apart (triangle inequality), far from r on either side: the answer is exactly one
cluster per seed, its centre the seed's first member in list order, its size the seed's multiplicity."""
import functools
import os
import sys

import numpy as np
import torch

import pose_grad_checks as pg

U23, U22 = 2.0 ** -23, 2.0 ** -22
RES = 1.25
RADII = (3.0, 6.0, 9.0)
# (seed, K, ns) of the random sets: the half-gaps at the three radii were checked to lie between 5e-4 and 3e-2 Angstrom
SETS = {1: (1, 300, 12), 2: (2, 65, 5), 3: (3, 1000, 25), 4: (4, 200, 8), 5: (5, 1000, 10)}


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0


# ----------------------------------------------------------------------------------------------------------------------
# generator and truth
# ----------------------------------------------------------------------------------------------------------------------

def atoms(seed, n=60):
    rs = np.random.RandomState(1000 + seed)
    x = rs.normal(size=(n, 3)) * np.array([9.0, 6.0, 4.0])
    return x - 0.5 * (x.max(axis=0) + x.min(axis=0))


def _random_rotations(rs, n):
    q = rs.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def poses(seed, K, ns):
    """-> (R (K, 3, 3), t (K, 3) Angstrom), float64"""
    rs = np.random.RandomState(seed)
    Rs = _random_rotations(rs, ns)
    ts = rs.randint(-24, 25, size=(ns, 3)) * RES
    which = rs.randint(0, ns, size=K)
    rv = rs.normal(size=(K, 3)) * np.radians(4.0)
    R = np.stack([pg._expm(rv[k]) @ Rs[which[k]] for k in range(K)])
    t = ts[which] + rs.randint(-3, 4, size=(K, 3)) * RES
    return R, t


def weights_of(x, seed):
    w = np.random.RandomState(77 + seed).uniform(0.0, 1.0, size=x.shape[0])
    w[::5] = 0.0                                                         # (a subset switched off)
    return w


def rmsd64(x, Ra, ta, Rb=None, tb=None, w=None, chunk=64):
    x = np.asarray(x, dtype=np.float64)
    w = np.full(x.shape[0], 1.0 / x.shape[0]) if w is None else np.asarray(w, dtype=np.float64) / np.sum(w)
    Xa = np.einsum("kd,pcd->pkc", x, Ra) + ta[:, None, :]
    Xb = Xa if Rb is None else np.einsum("kd,pcd->pkc", x, Rb) + tb[:, None, :]
    D = np.zeros((Xa.shape[0], Xb.shape[0]))
    for i in range(0, Xa.shape[0], chunk):
        diff = Xa[i:i + chunk, None] - Xb[None]
        D[i:i + chunk] = np.sqrt(((diff ** 2).sum(axis=3) * w).sum(axis=2))
    return D


def greedy64(D, r, m=None):
    K = D.shape[0]
    centres, sizes, labels = [], [], np.full(K, -1, dtype=np.int32)
    for i in range(K):
        hit = [n for n, c in enumerate(centres) if D[c, i] <= r]
        if hit:
            labels[i] = hit[0]
            sizes[hit[0]] += 1
        elif m is None or len(centres) < m:
            labels[i] = len(centres)
            centres.append(i)
            sizes.append(1)
    return np.array(centres, dtype=np.int32), np.array(sizes, dtype=np.int32), labels


def tuned_radius(D, nominal, M, window=0.05):
    """The nominal radius moved into the widest gap of the pair distances near it; asserts the gap is wider than the band."""
    d = D[np.triu_indices(D.shape[0], 1)] if D.shape[0] == D.shape[1] else D.reshape(-1)
    near = np.sort(d[(d > nominal - window) & (d < nominal + window)])
    v = np.concatenate([[nominal - window], near, [nominal + window]])
    k = int(np.argmax(np.diff(v)))
    r, half = 0.5 * (v[k] + v[k + 1]), 0.5 * (v[k + 1] - v[k])
    band = U22 * (7 * M + 8 * r)
    assert half >= band, "pair distances too dense round %.1f: half-gap %.3g < band %.3g" % (nominal, half, band)
    return float(r), float(half), float(band)


class Case(object):
    pass


@functools.lru_cache(maxsize=None)
def case(key, K=None):
    """One random set (SETS[key], or its first K poses) with its float64 truth, computed once and shared."""
    from deeplocalproteindocking_amd import ops
    seed, Kfull, ns = SETS[key]
    c = Case()
    c.x = atoms(seed)
    c.R, c.t = poses(seed, Kfull, ns)
    if K is not None:
        c.R, c.t = c.R[:K], c.t[:K]
    c.K = c.R.shape[0]
    c.D = rmsd64(c.x, c.R, c.t)
    c.E, c.M = ops.pose_embedding(c.x, c.R, c.t)
    c.radii = {}
    for nominal in RADII:
        c.radii[nominal] = tuned_radius(c.D, nominal, c.M)
    c.D.setflags(write=False)
    return c


# ----------------------------------------------------------------------------------------------------------------------
# 1: the embedding (host only)
# ----------------------------------------------------------------------------------------------------------------------

def check_embedding():
    from deeplocalproteindocking_amd import ops
    for key in (2, 4):
        seed, K, ns = SETS[key]
        x = atoms(seed)
        R, t = poses(seed, K, ns)
        for w in (None, weights_of(x, seed)):
            D = rmsd64(x, R, t, w=w)
            E64 = _embedding64(x, R, t, w)
            De = np.sqrt(((E64[:, None] - E64[None]) ** 2).sum(axis=2))
            assert np.abs(De - D).max() <= 1e-9, np.abs(De - D).max()
            E, M = ops.pose_embedding(x, R, t, w)
            assert E.dtype == torch.float32 and tuple(E.shape) == (K, 12) and E.numpy().tobytes() == E64.astype(np.float32).tobytes()
            assert M == float(np.abs(E64).max())
            # a common rigid motion (Q, s) of all poses: X -> Q X + s
            Q, s = pg._expm([0.7, -1.1, 0.4]), np.array([3.0, -7.5, 11.25])
            Em = _embedding64(x, Q[None] @ R, t @ Q.T + s, w)
            Dm = np.sqrt(((Em[:, None] - Em[None]) ** 2).sum(axis=2))
            assert np.abs(Dm - D).max() <= 1e-9
    import pytest
    with pytest.raises(RuntimeError, match="weights"):
        ops.pose_embedding(x, R, t, -np.ones(x.shape[0]))
    with pytest.raises(RuntimeError, match="expects"):
        ops.pose_embedding(x, R, t[:-1])


def _embedding64(x, R, t, w):
    """ops.pose_embedding's own float64 values (the function rounds them to float32), restated."""
    w = np.full(x.shape[0], 1.0 / x.shape[0]) if w is None else w / w.sum()
    c = (w[:, None] * x).sum(axis=0)
    y = x - c
    lam, V = np.linalg.eigh((w[:, None, None] * y[:, :, None] * y[:, None, :]).sum(axis=0))
    B = V * np.sqrt(np.clip(lam, 0.0, None))[None, :]
    return np.concatenate([R @ c + t, (R @ B).reshape(-1, 9)], axis=1)


# ----------------------------------------------------------------------------------------------------------------------
# 2: the dense kernel
# ----------------------------------------------------------------------------------------------------------------------

def check_dense(lib, device, Ka, Kb):
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    a, b = case(3), case(5)
    x = a.x
    Ra, ta, Rb, tb = a.R[:Ka], a.t[:Ka], b.R[:Kb], b.t[:Kb]
    if Ka == Kb:
        Rb, tb = Ra, ta
    D64 = rmsd64(x, Ra, ta, Rb, tb)
    Ea, Ma = ops.pose_embedding(x, Ra, ta, device=dev)
    Eb, Mb = ops.pose_embedding(x, Rb, tb, device=dev)
    M = max(Ma, Mb)
    D = ops.pose_rmsd(Ea, Eb, lib=lib).cpu().numpy().astype(np.float64)
    err, bound = np.abs(D - D64), U23 * (7 * M + 8 * D64)
    print("pose_rmsd (%d, %d): M = %.1f, d <= %.1f, worst error %.3g of the bound" % (Ka, Kb, M, D64.max(), (err / bound).max()))
    assert D.shape == (Ka, Kb) and (err <= bound).all()
    if Ka == Kb:
        S = ops.pose_rmsd(Ea, lib=lib).cpu().numpy()
        assert S.tobytes() == S.T.copy().tobytes() and (np.diag(S) == 0).all()
        assert S.tobytes() == D.astype(np.float32).tobytes()


def check_duplicates(lib, device, K=70):
    from deeplocalproteindocking_amd import ops
    c = case(2)
    idx = np.arange(K) % 33                                               # every pose of the first 33 two or three times
    E = c.E[torch.from_numpy(idx)].to(device).contiguous()
    D = ops.pose_rmsd(E, lib=lib).cpu().numpy()
    same = idx[:, None] == idx[None]
    assert (D[same] == 0).all() and (D[~same] > 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 3: the bitmap
# ----------------------------------------------------------------------------------------------------------------------

def unpack(mask, K):
    """(K, W) int64 words -> (K, 64 W) bool"""
    m = np.ascontiguousarray(mask.cpu().numpy()).view(np.uint64)
    return ((m[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None]) & np.uint64(1)).astype(bool).reshape(K, -1)


def check_bitmap(lib, device, key, K, guard=False):
    from deeplocalproteindocking_amd import ops
    c = case(key, K)
    E = c.E.to(device)
    for nominal in RADII:
        r, half, band = c.radii[nominal]
        if guard:
            from guard_alloc import GuardedAllocations
            with GuardedAllocations(min_bytes=8) as g:
                mask = ops.pose_within(E, r, lib=lib)
                bad = g.check(release=False)
            assert not bad, bad
        else:
            mask = ops.pose_within(E, r, lib=lib)
        assert tuple(mask.shape) == (K, (K + 63) // 64)
        bits = unpack(mask, K)
        print("pose_within K = %d, r = %.4f: half-gap %.3g, band %.3g, %d bits" % (K, r, half, band, int(bits.sum())))
        assert not bits[:, K:].any()                                      # tail bits
        assert (bits[:, :K] == (c.D <= r)).all()
        assert bits[:, :K].diagonal().all() and (bits[:, :K] == bits[:, :K].T).all()


# ----------------------------------------------------------------------------------------------------------------------
# 4: clustering
# ----------------------------------------------------------------------------------------------------------------------

def _np(ts):
    return [t.cpu().numpy() for t in ts]


def check_cluster(lib, device, key, K=None):
    from deeplocalproteindocking_amd import ops
    c = case(key, K)
    E = c.E.to(device)
    for nominal in RADII:
        r = c.radii[nominal][0]
        want = greedy64(c.D, r)
        got = _np(ops.pose_cluster(E, r, lib=lib))
        again = _np(ops.pose_cluster(E, r, lib=lib))
        print("pose_cluster K = %d, r = %.4f: %d clusters, largest %d" % (c.K, r, len(want[0]), want[1].max()))
        for g, w, a in zip(got, want, again):
            assert g.dtype == np.int32 and g.tobytes() == w.tobytes() and a.tobytes() == g.tobytes()
        assert int(got[1].sum()) == c.K and (got[2] >= 0).all()
        m = 5
        want5 = greedy64(c.D, r, m)
        got5 = _np(ops.pose_cluster(E, r, max_clusters=m, lib=lib))
        for g, w in zip(got5, want5):
            assert g.tobytes() == w.tobytes()
        n = min(m, len(want[0]))
        assert (got5[0] == want[0][:n]).all() and (got5[1] == want[1][:n]).all()          # the first five, sizes unchanged
        assert (got5[2] == np.where(want[2] < n, want[2], -1)).all()


def check_cluster_edges(lib, device):
    from deeplocalproteindocking_amd import ops
    c = case(2)
    K = c.K
    E = c.E.to(device)
    # radius 0: every distinct pose a centre, an exact duplicate joins the first
    idx = np.concatenate([np.arange(K), [3, 0, 40]])
    Ed = c.E[torch.from_numpy(idx)].to(device).contiguous()
    cen, siz, lab = _np(ops.pose_cluster(Ed, 0.0, lib=lib))
    assert (cen == np.arange(K)).all() and (lab == idx).all()
    assert (siz == 1 + np.bincount([3, 0, 40], minlength=K)).all()
    # a radius above the diameter: one cluster of K (and an infinite one)
    for r in (float(c.D.max()) + 1.0, float("inf")):
        cen, siz, lab = _np(ops.pose_cluster(E, r, lib=lib))
        assert cen.tolist() == [0] and siz.tolist() == [K] and (lab == 0).all()
    # K = 1
    cen, siz, lab = _np(ops.pose_cluster(E[:1].contiguous(), 3.0, lib=lib))
    assert cen.tolist() == [0] and siz.tolist() == [1] and lab.tolist() == [0]
    D = ops.pose_rmsd(E[:1].contiguous(), lib=lib)
    assert tuple(D.shape) == (1, 1) and float(D[0, 0]) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# 5: planted sets
# ----------------------------------------------------------------------------------------------------------------------

def planted(K, ns, r, seed):
    """-> (x, R, t, which): ns seeds pairwise > 3 r apart, K members within r / 4 of theirs (both asserted on the atoms)."""
    rs = np.random.RandomState(seed)
    x = atoms(seed)
    Rs = _random_rotations(rs, ns)
    side = int(np.ceil(ns ** (1.0 / 3.0)))
    cell = np.stack(np.unravel_index(rs.permutation(side ** 3)[:ns], (side,) * 3), axis=1) - (side - 1) / 2.0
    ts = cell * (3.0 * r + 2.0 * np.linalg.norm(x, axis=1).max())      # |R_i x - R_j x| <= 2 max|x| for every atom
    Ds = rmsd64(x, Rs, ts)
    assert (Ds[np.triu_indices(ns, 1)] > 3.0 * r).all()
    which = np.concatenate([np.arange(ns), rs.randint(0, ns, size=K - ns)])[rs.permutation(K)]
    rv = rs.normal(size=(K, 3))
    rv *= (rs.uniform(0.0, np.radians(0.5), size=(K, 1)) / np.linalg.norm(rv, axis=1, keepdims=True))
    th = np.linalg.norm(rv, axis=1)[:, None, None]
    Kx = np.zeros((K, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -rv[:, 2], rv[:, 1], rv[:, 2], -rv[:, 0], -rv[:, 1], rv[:, 0]
    Q = np.eye(3)[None] + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)
    R = Q @ Rs[which]
    t = ts[which] + rs.uniform(-0.1 * r, 0.1 * r, size=(K, 3))
    w = 1.0 / x.shape[0]
    diff = np.einsum("kd,pcd->pkc", x, R) + t[:, None] - (np.einsum("kd,pcd->pkc", x, Rs[which]) + ts[which][:, None])
    dm = np.sqrt(((diff ** 2).sum(axis=2) * w).sum(axis=1))
    assert (dm <= 0.25 * r).all(), dm.max()
    return x, R, t, which


def check_planted(lib, device, K, ns, r=9.0, seed=11):
    from deeplocalproteindocking_amd import ops
    x, R, t, which = planted(K, ns, r, seed)
    E, _ = ops.pose_embedding(x, R, t, device=torch.device(device))
    cen, siz, lab = _np(ops.pose_cluster(E, r, lib=lib))
    _, first = np.unique(which, return_index=True)
    want_cen = np.sort(first)
    rank_of_seed = np.empty(ns, dtype=np.int64)
    rank_of_seed[which[want_cen]] = np.arange(ns)
    assert cen.tolist() == want_cen.tolist()
    assert siz.tolist() == np.bincount(which, minlength=ns)[which[want_cen]].tolist()
    assert (lab == rank_of_seed[which]).all()


# ----------------------------------------------------------------------------------------------------------------------
# 6: errors
# ----------------------------------------------------------------------------------------------------------------------

def check_errors(lib, device):
    import pytest
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    K = 70
    E = case(2).E[:K].to(dev).contiguous()
    st = _stream(dev)
    nbytes = lib.call("dlpd_pose_cluster_ws", K)
    assert nbytes == K * 2 * 8 and lib.call("dlpd_pose_cluster_ws", 0) == 0 and lib.call("dlpd_pose_cluster_ws", 65537) == 0
    assert lib.call("dlpd_pose_cluster_ws", 65536) == 65536 * 1024 * 8
    outs = dict(D=torch.full((K, K), -7.0, device=dev), mask=torch.full((K, 2), -7, dtype=torch.int64, device=dev),
                cen=torch.full((K,), -7, dtype=torch.int32, device=dev), siz=torch.full((K,), -7, dtype=torch.int32, device=dev),
                lab=torch.full((K,), -7, dtype=torch.int32, device=dev), cnt=torch.full((1,), -7, dtype=torch.int32, device=dev),
                ws=torch.full((K, 2), -7, dtype=torch.int64, device=dev))
    p = {k: v.data_ptr() for k, v in outs.items()}
    e = E.data_ptr()

    def rmsd(Ea=e, Eb=e, D=p["D"], Ka=K, Kb=K):
        return lib.call("dlpd_pose_rmsd", Ea, Eb, D, Ka, Kb, st)

    def within(E_=e, K_=K, r=3.0, mask=p["mask"]):
        return lib.call("dlpd_pose_within", E_, K_, r, mask, st)

    def cluster(E_=e, K_=K, r=3.0, m=0, cen=p["cen"], siz=p["siz"], lab=p["lab"], cnt=p["cnt"], ws=p["ws"], nb=nbytes):
        return lib.call("dlpd_pose_cluster", E_, K_, r, m, cen, siz, lab, cnt, ws, nb, st)
    bad = [(rmsd, (dict(Ea=None), dict(Eb=None), dict(D=None), dict(Ka=0), dict(Kb=-1))),
           (within, (dict(E_=None), dict(mask=None), dict(K_=0), dict(r=-1.0), dict(r=float("nan")))),
           (cluster, (dict(E_=None), dict(cen=None), dict(siz=None), dict(lab=None), dict(cnt=None), dict(ws=None), dict(K_=0),
                      dict(K_=-3), dict(r=-0.5), dict(r=float("nan")), dict(nb=nbytes - 1), dict(nb=0)))]
    for fn, cases in bad:
        for kw in cases:
            with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
                fn(**kw)
    for fn, kw in ((rmsd, dict(Ka=65537)), (rmsd, dict(Kb=65537)), (within, dict(K_=65537)), (cluster, dict(K_=65537, nb=1 << 40))):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            fn(**kw)                                                     # (refused before anything is read)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for k, v in outs.items():
        assert (v == -7).all(), k                                        # nothing was written
    assert rmsd() == 0 and within() == 0 and cluster() == 0
    # the ops' own refusals
    with pytest.raises(RuntimeError, match=r"\(K, 12\)"):
        ops.pose_cluster(E[:, :11], 3.0, lib=lib)
    with pytest.raises(RuntimeError, match="max_clusters"):
        ops.pose_cluster(E, 3.0, max_clusters=0, lib=lib)
    with pytest.raises(RuntimeError, match="float32"):
        ops.pose_rmsd(E.double(), lib=lib)


# ----------------------------------------------------------------------------------------------------------------------
# 7: Docker.cluster on a real list
# ----------------------------------------------------------------------------------------------------------------------

class _Model(object):
    threshold_clash = 4000.0
    clip = 5.0

    def __init__(self, filt):
        self.filter = filt

    def eval(self):
        return self


def _searched(lib, device, L, K=200, nrot=6, randomize=False):
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Models import SimpleFilter
    g = torch.Generator().manual_seed(21)
    C = 2
    rec, lig = torch.randn(1, C, L, L, L, generator=g) * 0.1, torch.randn(1, C, L, L, L, generator=g) * 0.1
    recf, ligf = torch.rand(L, L, L, generator=g), torch.rand(L, L, L, generator=g)
    torch.manual_seed(22)
    filt = SimpleFilter([C])
    with torch.no_grad():                                                # negative scores everywhere: with a positive output every
        filt.fc[2].weight.copy_(-filt.fc[2].weight.abs())                # pick of the search is a masked 0.0 at the same voxel
        filt.fc[2].bias.fill_(-1.0)
    R = _random_rotations(np.random.RandomState(8), nrot)
    dk = Docker(_Model(filt.to(device)), box_size=L, resolution=RES, max_conf=K, rotations=R, device=device, lib=lib,
                randomize_rot=randomize, rotation_seed=4)
    with torch.no_grad():
        dk.dock_volumes(rec, lig, recf, ligf, batch_size=2, write=False)
    assert len(dk.top_list) == K and max(e[4] for e in dk.top_list) < 0 and len(set(e[1:4] for e in dk.top_list)) > K // 2
    return dk


def check_docker_cluster(lib, device, L, tmp_path):
    dk = _searched(lib, device, L, randomize=True)
    top = list(dk.top_list)
    K = len(top)
    x = atoms(6, n=40)
    # the poses reconstructed from the list, and the truth on them
    R = np.stack([dk.rot.R[e[0]].double().cpu().numpy() for e in top])
    tv = np.array([dk.signed_translation(*e[1:4]) for e in top], dtype=np.float64)
    D = rmsd64(x, R, tv * RES)
    M = float(np.abs(_embedding64(x, R, tv * RES, None)).max())
    w = weights_of(x, 6)
    Dw = rmsd64(x, R, tv * RES, w=w)
    for nominal in RADII:
        r = tuned_radius(D, nominal, M)[0]
        cen, siz, lab = greedy64(D, r)
        got = dk.cluster(x, radius=r)
        assert got is dk.clustered_list and dk.top_list == top
        assert [e[3] for e in got] == cen.tolist() and [e[4] for e in got] == siz.tolist()
        assert dk.cluster_labels.dtype == np.int32 and (dk.cluster_labels == lab).all()
        for e in got:
            src = top[e[3]]
            assert e[0].dtype == np.float64 and e[0].tobytes() == R[e[3]].tobytes() and e[2] == src[4]
            assert e[1] == dk.signed_translation(*src[1:4])
        # the same poses as refined_list entries, on a tensor of atoms
        refined = [(R[n], tuple(int(v) for v in tv[n]), top[n][4], n) for n in range(K)]
        again = dk.cluster(torch.from_numpy(x), poses=refined, radius=r)
        assert [(e[0].tobytes(),) + tuple(e[1:]) for e in again] == [(e[0].tobytes(),) + tuple(e[1:]) for e in got]
        assert (dk.cluster_labels == lab).all()
        # keep
        kept = dk.cluster(x, radius=r, keep=3)
        cen3, siz3, lab3 = greedy64(D, r, 3)
        assert [e[3] for e in kept] == cen3.tolist() and [e[4] for e in kept] == siz3.tolist() and (dk.cluster_labels == lab3).all()
        # rank="size": the stable re-sort, then keep
        order = sorted(range(len(cen)), key=lambda n: -int(siz[n]))      # (sorted() is stable)
        by_size = dk.cluster(x, radius=r, rank="size")
        assert [e[3] for e in by_size] == [int(cen[n]) for n in order] and [e[4] for e in by_size] == [int(siz[n]) for n in order]
        place = {n: i for i, n in enumerate(order)}
        assert dk.cluster_labels.tolist() == [place[int(v)] for v in lab]
        cut = dk.cluster(x, radius=r, keep=2, rank="size")
        assert [e[3] for e in cut] == [int(cen[n]) for n in order[:2]]
        assert dk.cluster_labels.tolist() == [place[int(v)] if place[int(v)] < 2 else -1 for v in lab]
        # weights
        rw = tuned_radius(Dw, nominal, M)[0]
        cw, sw, lw = greedy64(Dw, rw)
        gw = dk.cluster(x, radius=rw, weights=w)
        assert [e[3] for e in gw] == cw.tolist() and [e[4] for e in gw] == sw.tolist() and (dk.cluster_labels == lw).all()
    # fractional translations (what minimize(translation=True) writes)
    frac = np.random.RandomState(3).uniform(-0.5, 0.5, size=(K, 3))
    Df = rmsd64(x, R, (tv + frac) * RES)
    rf = tuned_radius(Df, 6.0, M + 1.0)[0]
    cf, sf, lf = greedy64(Df, rf)
    gf = dk.cluster(x, poses=[(R[n], tuple(float(v) for v in tv[n] + frac[n]), top[n][4], n) for n in range(K)], radius=rf)
    assert [e[3] for e in gf] == cf.tolist() and [e[4] for e in gf] == sf.tolist() and (dk.cluster_labels == lf).all()
    # the writer: column for column write_conformations' text of the centre entries (randR undone the same way)
    got = dk.cluster(x, radius=tuned_radius(D, 6.0, M)[0])
    dk.new_log(str(tmp_path / "c.dat"))
    dk.write_clustered_conformations()
    dk.cleanup()
    dk.top_list = [top[e[3]] for e in got]
    dk.new_log(str(tmp_path / "t.dat"))
    dk.write_conformations()
    dk.cleanup()
    dk.top_list = top
    text = open(str(tmp_path / "c.dat")).read()
    assert text == open(str(tmp_path / "t.dat")).read() and len(text.strip().split("\n")) == len(got) > 1
    import pytest
    with pytest.raises(Exception, match="radius"):
        dk.cluster(x)
    with pytest.raises(Exception, match="ranking"):
        dk.cluster(x, radius=3.0, rank="cluspro")
    assert dk.cluster(x, poses=[], radius=3.0) == [] and len(dk.cluster_labels) == 0


# ----------------------------------------------------------------------------------------------------------------------
# 8: scripts/dock_pair.py --cluster
# ----------------------------------------------------------------------------------------------------------------------

def check_dock_pair(lib, device, tmp_path):
    """The script's own cluster step (``cluster_and_write``, what ``--cluster RADIUS[:KEEP]`` runs after the search) on a search
    of two synthetic PDB files."""
    from synth_pdb import write_protein_like_pdb
    from test_atoms import _tiny_model
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Results.DockerParser import DockerParser
    from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import dock_pair
    assert dock_pair.parse_cluster("9") == (9.0, None) and dock_pair.parse_cluster("4.5:20") == (4.5, 20)
    frec, flig = str(tmp_path / "r.pdb"), str(tmp_path / "l.pdb")
    write_protein_like_pdb(frec, 14, seed=5)
    write_protein_like_pdb(flig, 9, seed=6)
    L, K = 32, 40
    R = _random_rotations(np.random.RandomState(2), 3)
    dk = Docker(_tiny_model(), box_size=L, resolution=RES, max_conf=K, rotations=R, device=device, lib=lib,
                coords_backend=CoordsBackend(lib=lib))
    out = str(tmp_path / "pair.dat")
    with torch.no_grad():
        p = dk.prepare(frec, flig, "SE3")
        dk.new_log(out)
        dk.dockSE3(frec, flig, batch_size=2, prepared=p)
        dk.cleanup()
    top = list(dk.top_list)
    for spec, poses in (("6", None), ("6:3", None)):
        radius, keep = dock_pair.parse_cluster(spec)
        name, sizes_name = dock_pair.cluster_and_write(dk, p, out, radius, keep, poses=poses)
        assert name == str(tmp_path / "pair.clustered.dat") and sizes_name == str(tmp_path / "pair.clustered.sizes.txt")
        lines = [ln for ln in open(name).read().split("\n") if ln.strip()]
        sizes = [int(v) for v in open(sizes_name).read().split()]
        assert len(lines) == len(sizes) == len(dk.clustered_list) >= 1 and all(len(ln.split("\t")) == 13 for ln in lines)
        assert sum(sizes) == int((dk.cluster_labels >= 0).sum()) and sizes == [e[4] for e in dk.clustered_list]
        if keep is None:
            assert sum(sizes) == K
        else:
            assert len(sizes) <= keep
        confs = DockerParser(str(tmp_path), coords_backend=object()).parse_output("pair.clustered")["conformations"]
        assert len(confs) == len(sizes)
    assert dk.top_list == top and len(open(out).read().strip().split("\n")) == K
