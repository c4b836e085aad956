"""Check bodies of the pose evaluation (csrc/dlpd_evaluate.h, ops.pose_native_* / pose_capri / pose_evaluate, Docker.evaluate,
Results.evaluate_target_device), shared by tests/test_evaluate_emu.py (the CPU-emulated kernels) and tests/test_evaluate_gpu.py
(the gfx950 build).  Nothing here reads the reference tree.

THE TRUTH is float64 on explicit points: the mobile set [a ; y R^T + t] against the static set by numpy's SVD Kabsch,
e0 - 2 (s1 + s2 + d s3) with d = sign det(P^T Q) (``kabsch64``), the minimum over the interface pairs; the ligand RMSD by direct
differences (``lrmsd64``); a contact by the minimum atom-pair distance of its two residues under the pose (``min_distances``);
the class by the cascade written from its definition (``cascade``).

THE RMSD BAND (derived, not tuned).  u = 2^-53.  The kernel forms n rmsd^2 = Gp + Gq - 2 lambda; S = Gp + Gq, the two centred
energies, is the scale (both terms are non-negative and lambda <= sqrt(Gp Gq) <= S / 2).  Per source, in units of u S:
  moments    every point set is taken about its centroid (one rounding per coordinate: relative u), products are rounded once,
             sums are exact (math.fsum) and rounded once: 4 u on Saa, Syy, Gq (4 in all, they add up to S), and 4 u sum |x||q|
             <= 4 u sqrt(Gp Gq) on each of the 9 entries of A and Y, 12 u sqrt(Gp Gq) <= 6 u S in Frobenius norm.  The number of
             points does not enter.
  assembly   H = A + R Y + u s^T is four fma per entry (8 in Frobenius norm, as above); sum |R y|^2 from the second moments of
             y, Gp and the final Gp + Gq - 2 lambda are fifteen roundings of values <= S (15).
  lambda     is 1-Lipschitz in Horn's matrix N (Weyl) and |N|_F = 2 |H|_F <= S, so an error dH of H moves lambda by at most
             2 |dH|_F and the result by 4 |dH|_F: the 6 and 8 above count four times (56).  A Jacobi rotation writes six
             entries, each by two fma from c, s, tau that carry up to four roundings: at most 16 u |N|_F per rotation, six
             rotations a sweep, at most EVAL_SWEEPS = 12 sweeps, twice for the factor of lambda: 2 * 16 * 6 * 12 = 2304.
  the pose   its offset t + R cy - ca is rounded at the size T = |t| + |cy| + |ca| of its terms, not at its own: 4 u T.  It
             enters H through u s^T (|s| <= sqrt(nl Gq)) and Gp through (nl nr / n) |u|^2 <= Gp: at most 24 u kappa S with
             kappa = T / sqrt(S / n), the size of the coordinates over the size of the interface.  The float64 truth, which
             poses uncentred atoms, has this term too.
band = 2 u (4 + 56 + 15 + 2304 + 24 kappa): TWICE the bound, both sides carry float64 rounding.  kappa is a property of a case's
inputs and is computed from them; every case asserts band <= 2^-40 (kappa <= 70).  With kappa about 10 this is 2^-40.7: the
Jacobi term, counted at its cap, is nearly all of it.  For the ligand RMSD the scale is (Syy + Szz) / nl + |u|^2, what the kernel
adds up, and the same count without an eigenvalue gives band_L = 2 u (42 + 8 kappa_L).  n = 1 has S = 0: both sides must give an
exact zero, and do (the centred point is 0.0).

THE CONTACT BAND (float32).  v = 2^-24, M = the largest |coordinate sum| the chain of a posed atom passes through (|t|_inf +
|y|_2) or a receptor atom has.  A posed coordinate carries the rounding of t (1), of R and of the atom (2) and three fma (3):
6 v M; the receptor's atom 1 v M; their difference one more rounding v d: |dd| <= 7 sqrt(3) v M + v d over the three
coordinates.  The chain of d^2 adds 3 v d^2, i.e. 1.5 v d; r rounded and squared in float32 1.5 v r.  At d ~ r:
|d32 - d64| + |r32 - r| <= v (13 M + 4 r) = ``contact_band``.  ``tuned_cutoff`` moves the nominal 5.0 A to the middle of the
widest gap between the sorted atom-pair distances of all (pose, contact) pairs within +-0.05 A of it and asserts, on the truth
alone, half the gap >= 2 band; then the kernel's bit is the float64 predicate and ``count`` must match exactly.
Half-gaps of the seeds used below (checked on the CPU): 1.7e-4 A (C = 64 / 65 at K = 65) to 2.7e-2 A against bands of
2.1e-5 to 8.0e-5 A; 1.1e-4 A against 4.5e-5 A for the 512 reference poses of the 65,536-pose test."""
import functools
import os
import sys

import numpy as np
import torch

import pose_grad_checks as pg
from cluster_checks import _random_rotations, _stream

U = 2.0 ** -53
V = 2.0 ** -24
BAND_LIMIT = 2.0 ** -40
C_FIXED = 4 + 56 + 15 + 2304
THRESHOLDS = ((0.1, 10.0, 4.0), (0.3, 5.0, 2.0), (0.5, 1.0, 1.0))
worst = {"irmsd": 0.0, "lrmsd": 0.0}                 # worst error / band seen in this process (printed by the checks)


# ----------------------------------------------------------------------------------------------------------------------
# truth
# ----------------------------------------------------------------------------------------------------------------------

def kabsch64(mobile, static):
    """-> (n rmsd^2, S = Gp + Gq), float64 SVD"""
    P, Q = mobile - mobile.mean(axis=0), static - static.mean(axis=0)
    H = P.T @ Q
    s = np.linalg.svd(H, compute_uv=False)
    d = np.sign(np.linalg.det(H))
    S = float((P * P).sum() + (Q * Q).sum())
    return max(0.0, S - 2.0 * float(s[0] + s[1] + d * s[2])), S


def irmsd64(pairs, P):
    """-> (rmsd^2 (K), scale (K) = the largest S / n over the pairs, kappa (K)): |min a - min b| <= max |a - b| over the pairs"""
    K = P.shape[0]
    r2, scale, kappa = np.full(K, np.inf), np.zeros(K), np.zeros(K)
    for a, y, q in pairs:
        n = len(a) + len(y)
        ca = a.mean(axis=0) if len(a) else np.zeros(3)
        for k in range(K):
            R, t = P[k, :9].reshape(3, 3), P[k, 9:]
            e, S = kabsch64(np.concatenate([a, y @ R.T + t]), q)
            r2[k] = min(r2[k], e / n)
            scale[k] = max(scale[k], S / n)
            T = np.linalg.norm(t) + np.linalg.norm(y.mean(axis=0)) + np.linalg.norm(ca)
            kappa[k] = max(kappa[k], T / np.sqrt(S / n) if S > 0 else 0.0)
    return r2, scale, kappa


def lrmsd64(y, z, P):
    """-> (lrmsd^2 (K), scale (K), kappa (K)) by direct differences"""
    R, t = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
    X = np.einsum("kd,pcd->pkc", y, R) + t[:, None, :]
    l2 = ((X - z[None]) ** 2).sum(axis=2).mean(axis=1)
    cy, cz = y.mean(axis=0), z.mean(axis=0)
    u = t + cy @ np.transpose(R, (0, 2, 1)) - cz
    scale = (((y - cy) ** 2).sum() + ((z - cz) ** 2).sum()) / len(y) + (u ** 2).sum(axis=1)
    T = np.linalg.norm(t, axis=1) + np.linalg.norm(cy) + np.linalg.norm(cz)
    return l2, scale, T / np.sqrt(scale)


def band_i(kappa):
    b = 2.0 * U * (C_FIXED + 24.0 * float(np.max(kappa)))
    assert b <= BAND_LIMIT, (b / BAND_LIMIT, float(np.max(kappa)))
    return b


def band_l(kappa):
    b = 2.0 * U * (42.0 + 8.0 * float(np.max(kappa)))
    assert b <= BAND_LIMIT
    return b


def cascade(fnat, lrmsd, irmsd):
    cls = 0
    for a, b, c in THRESHOLDS:
        if (fnat >= a and lrmsd <= b) or irmsd <= c:
            cls = {0.1: 1, 0.3: 2, 0.5: 3}[a]
    return cls


def min_distances(rec, lig, ranges, P, near=None, window=0.05, nominal=5.0):
    """-> dmin (K, C): the least atom-pair distance of every contact under every pose; ``near`` (a list) collects every
    atom-pair distance within ``window`` of ``nominal``"""
    R, t = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
    X = np.einsum("kd,pcd->pkc", lig, R) + t[:, None, :]                  # (K, NLa, 3)
    out = np.zeros((P.shape[0], len(ranges)))
    for c, (r0, r1, l0, l1) in enumerate(ranges):
        d = np.sqrt(((rec[None, r0:r1, None, :] - X[:, None, l0:l1, :]) ** 2).sum(axis=3))
        out[:, c] = d.reshape(P.shape[0], -1).min(axis=1)
        if near is not None:
            near.append(d[np.abs(d - nominal) < window])
    return out


def contact_band(M, r):
    return V * (13.0 * M + 4.0 * r)


def tuned_cutoff(near, M, nominal=5.0, window=0.05):
    near = np.sort(np.concatenate(near)) if near else np.zeros(0)
    v = np.concatenate([[nominal - window], near, [nominal + window]])
    k = int(np.argmax(np.diff(v)))
    r, half = 0.5 * (v[k] + v[k + 1]), 0.5 * (v[k + 1] - v[k])
    band = contact_band(M, r)
    assert half >= 2.0 * band, "atom-pair distances too dense round %.1f: half-gap %.3g < 2 x band %.3g" % (nominal, half, band)
    return float(r), float(half), float(band)


# ----------------------------------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------------------------------

def pose_rows(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64).reshape(-1, 9), np.asarray(t, dtype=np.float64).reshape(-1, 3)], axis=1)


def perturbed(rs, Rn, tn, centre, K, angle=5.0, shift=2.0, far=True):
    """K poses: the native one, poses near it (a rotation N(0, angle degrees) per component about ``centre``, the ligand's
    interface centre in the docking frame, and a shift N(0, shift)), and -- ``far`` -- every third one anywhere"""
    out = np.zeros((K, 12))
    for k in range(K):
        if k == 0:
            R, t = Rn, tn
        elif far and k % 3 == 2:
            R, t = _random_rotations(rs, 1)[0], tn + rs.normal(size=3) * 10.0
        else:
            Q = pg._expm(rs.normal(size=3) * np.radians(angle))
            R, t = Q @ Rn, Q @ (tn - centre) + centre + rs.normal(size=3) * shift
        out[k] = pose_rows(R, t)[0]
    return out


class Case(object):
    pass


@functools.lru_cache(maxsize=None)
def rmsd_case(seed, nr, nl, nI, K, kind="random"):
    """One target for the RMSD kernel with its truth, computed once.  ``kind`` shapes the point sets: random | collinear |
    coplanar | mirror | exact | constant."""
    rs = np.random.RandomState(4000 + seed)
    c = Case()
    Rn, tn = _random_rotations(rs, 1)[0], np.array([31.0, -4.0, 6.0])
    c.pairs = []
    for p in range(nI):
        shape = {"collinear": (1.0, 0.0, 0.0), "coplanar": (1.0, 1.0, 0.0)}.get(kind, (1.0, 1.0, 1.0))
        frame = _random_rotations(rs, 1)[0]                                             # (the line / the plane: both parts lie in it)
        a = ((rs.normal(size=(nr, 3)) * 7.0 + [-6.0, 0.0, 0.0]) * shape) @ frame.T + 20.0
        yn = ((rs.normal(size=(nl, 3)) * 6.0 + [6.0, 0.0, 0.0]) * shape) @ frame.T + 20.0  # the ligand's points where the native has them
        Qp = pg._expm(rs.normal(size=3) * np.radians(3.0 * p))                          # (pair p: its own native, p degrees off)
        m = np.concatenate([a, (yn - 20.0) @ Qp.T + 20.0])
        if kind == "mirror":
            m = m * [1.0, 1.0, -1.0]
        elif kind == "constant":
            m = np.zeros_like(m) + [3.0, -8.0, 1.0]
        elif kind == "random":
            m = m + rs.normal(size=m.shape) * 0.4
        F, s = _random_rotations(rs, 1)[0], np.array([80.0, -35.0, 12.0])
        q = m if kind == "exact" else m @ F.T + s
        c.pairs.append((a, (yn - tn) @ Rn, q))                                          # y = Rn^T (yn - tn)
    nL = max(nl, 3) + 20
    c.lig = rs.normal(size=(nL, 3)) * 9.0
    c.target = c.lig @ Rn.T + tn + rs.normal(size=(nL, 3)) * 0.3
    c.P = perturbed(rs, Rn, tn, np.array([20.0, 20.0, 20.0]), K)
    if kind != "random":
        c.P[-1] = pose_rows(np.eye(3), np.zeros(3))[0]                                  # the identity pose
    c.i2, c.iscale, c.ikappa = irmsd64(c.pairs, c.P)
    c.l2, c.lscale, c.lkappa = lrmsd64(c.lig, c.target, c.P)
    for v in (c.P, c.i2, c.l2):
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def contact_case(seed, C, K, pad_to=None, far=True, nres=144):
    """Two facing layers of residues of 1 and of 14 atoms, the first C native contacts (residue pairs within 5 A in the native
    placement), the atoms of the residues they name packed residue after residue; poses round the native; the tuned cutoff."""
    rs = np.random.RandomState(7000 + seed)
    c = Case()

    def layer(z):
        side = int(np.ceil(np.sqrt(nres)))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:nres] * 3.0
        cen = np.concatenate([g - g.mean(axis=0), np.full((nres, 1), z)], axis=1) + rs.normal(size=(nres, 3)) * 0.4
        return [cen[i] + (rs.normal(size=(14, 3)) * 0.9 if i % 4 == 1 else np.zeros((1, 3))) for i in range(nres)]
    off = np.array([4.0, 3.0, -6.0])
    rec_res = [r + off for r in layer(0.0)]
    lig_res = [r + off for r in layer(3.6)]
    found = []
    for j, l in enumerate(lig_res):
        for i, r in enumerate(rec_res):
            if np.sqrt(((r[:, None] - l[None]) ** 2).sum(axis=2)).min() <= 4.6:
                found.append((i, j))
    found = [found[i] for i in rs.permutation(len(found))]
    assert len(found) >= C, (len(found), C)
    found = found[:C]
    Rn, tn = _random_rotations(rs, 1)[0], np.array([7.0, 2.0, -4.0])
    ri, li = sorted(set(f[0] for f in found)), sorted(set(f[1] for f in found))
    rstart, lstart = np.cumsum([0] + [len(rec_res[i]) for i in ri]), np.cumsum([0] + [len(lig_res[j]) for j in li])
    c.rec = np.concatenate([rec_res[i] for i in ri])
    lig_native = np.concatenate([lig_res[j] for j in li])
    if pad_to is not None:                                                              # atoms no contact names, far away
        assert pad_to >= len(lig_native)
        lig_native = np.concatenate([lig_native, rs.normal(size=(pad_to - len(lig_native), 3)) * 3.0 + [0.0, 0.0, 60.0]])
    c.lig = (lig_native - tn) @ Rn
    c.ranges = np.array([(rstart[ri.index(i)], rstart[ri.index(i) + 1], lstart[li.index(j)], lstart[li.index(j) + 1]) for i, j in found],
                        dtype=np.int32).reshape(-1, 4)
    c.C = C
    centre = lig_native[:lstart[-1]].mean(axis=0)
    c.P = perturbed(rs, Rn, tn, centre, K, angle=3.0, shift=1.0, far=far)
    if K >= 5:
        c.P[K - 1] = pose_rows(Rn, tn + [0.0, 0.0, 30.0])[0]                            # no contact holds
    near = []
    c.dmin = min_distances(c.rec, c.lig, c.ranges, c.P, near)
    M = max(np.abs(c.rec).max() * np.sqrt(3.0), np.abs(c.P[:, 9:]).max() + np.linalg.norm(c.lig, axis=1).max())
    c.r, c.half, c.band = tuned_cutoff(near, M)
    c.count = (c.dmin <= c.r).sum(axis=1).astype(np.int32)
    c.Rn, c.tn = Rn, tn
    return c


def reference_of(pairs, lig, target, rec_atoms, lig_atoms, ranges, cutoff, device):
    from deeplocalproteindocking_amd.Results.InterfaceSelection import native_reference_from_points
    return native_reference_from_points(pairs, lig, target, rec_atoms, lig_atoms, ranges, cutoff).to(device)


# ----------------------------------------------------------------------------------------------------------------------
# 1: the two RMSDs
# ----------------------------------------------------------------------------------------------------------------------

def _rmsd_on_device(lib, device, c, P=None):
    from deeplocalproteindocking_amd import ops
    mom, cnt = ops.native_moments(c.pairs, c.lig, c.target)
    P = c.P if P is None else P
    ir, lr = ops.pose_native_rmsd(torch.from_numpy(np.array(P)).to(device), torch.from_numpy(mom).to(device), cnt, lib=lib)
    return ir.cpu().numpy(), lr.cpu().numpy()


def _assert_rmsd(c, ir, lr, what):
    bi, bl = band_i(c.ikappa), band_l(c.lkappa)
    ei, el = np.abs(ir ** 2 - c.i2), np.abs(lr ** 2 - c.l2)
    ok = c.iscale > 0
    ri = float((ei[ok] / (bi * c.iscale[ok])).max()) if ok.any() else 0.0
    rl = float((el / (bl * c.lscale)).max())
    worst["irmsd"], worst["lrmsd"] = max(worst["irmsd"], ri), max(worst["lrmsd"], rl)
    print("%s: band_I 2^%.2f (kappa %.1f), worst I error %.3g of it; band_L 2^%.2f, worst L error %.3g of it" %
          (what, np.log2(bi), c.ikappa.max(), ri, np.log2(bl), rl))
    assert np.isfinite(ir).all() and np.isfinite(lr).all()
    assert (ei <= bi * c.iscale).all(), ri                                              # (scale 0: an exact zero on both sides)
    assert (el <= bl * c.lscale).all(), rl


def check_rmsd(lib, device, K, nI, nr, nl):
    c = rmsd_case(1, nr, nl, nI, K)
    ir, lr = _rmsd_on_device(lib, device, c)
    assert ir.shape == (K,) and lr.shape == (K,) and ir.dtype == np.float64
    _assert_rmsd(c, ir, lr, "pose_native_rmsd K = %d, nI = %d, (nr, nl) = (%d, %d)" % (K, nI, nr, nl))
    if nI > 1:                                                                          # the minimum picked a pair other than the first
        which = np.argmin(np.stack([irmsd64([pair], c.P)[0] for pair in c.pairs]), axis=0)
        assert K < 3 * nI or nr == 0 or len(set(which.tolist())) >= 2       # (nr = 0: the pose does not enter)


def _det_h(pair, pose):
    a, y, q = pair
    m = np.concatenate([a, y @ pose[:9].reshape(3, 3).T + pose[9:]])
    return float(np.linalg.det((m - m.mean(axis=0)).T @ (q - q.mean(axis=0))))


def check_rmsd_degenerate(lib, device, kind):
    """collinear | coplanar | mirror | exact | constant at (nr, nl) = (12, 9); tiny: n = 1 and n = 2, static = mobile.  65 poses
    and the identity pose each."""
    K = 66
    for nr, nl in (((0, 1), (1, 1), (0, 2)) if kind == "tiny" else ((12, 9),)):
        c = rmsd_case(2, nr, nl, 1, K, "exact" if kind == "tiny" else kind)
        ir, lr = _rmsd_on_device(lib, device, c)
        _assert_rmsd(c, ir, lr, "degenerate %s (nr, nl) = (%d, %d)" % (kind, nr, nl))
        if nr + nl == 1:
            assert (ir == 0.0).all() and (c.i2 == 0.0).all()
        if kind in ("exact", "tiny"):                                                   # the native pose: static = mobile
            limit = band_i(c.ikappa) * c.iscale[0]
            assert c.i2[0] <= limit and ir[0] ** 2 <= limit
        if kind == "mirror":
            assert _det_h(c.pairs[0], c.P[0]) < -1.0 and c.i2[0] > 1.0
        if kind == "constant":
            assert (c.iscale > 0).all() and np.allclose(ir ** 2, c.iscale, rtol=1e-9)   # H = 0: rmsd^2 = Gp / n


# ----------------------------------------------------------------------------------------------------------------------
# 2: contacts
# ----------------------------------------------------------------------------------------------------------------------

def _contacts_on_device(lib, device, c, guard=False, P=None):
    from deeplocalproteindocking_amd import ops
    P = c.P if P is None else P
    args = (torch.from_numpy(np.array(P)).to(device), torch.from_numpy(c.rec.astype(np.float32)).to(device),
            torch.from_numpy(c.lig.astype(np.float32)).to(device), torch.from_numpy(c.ranges).to(device), c.ranges, c.r)
    if guard:
        from guard_alloc import GuardedAllocations
        with GuardedAllocations(min_bytes=4) as g:
            count = ops.pose_native_contacts(*args, lib=lib)
            bad = g.check(release=False)
        assert not bad, bad
    else:
        count = ops.pose_native_contacts(*args, lib=lib)
    return count.cpu().numpy()


def check_contacts(lib, device, C, K, pad_to=None, guard=False):
    c = contact_case(1, C, K, pad_to)
    count = _contacts_on_device(lib, device, c, guard)
    print("pose_native_contacts C = %d, K = %d, NRa = %d, NLa = %d: cutoff %.5f, half-gap %.3g, band %.3g, counts %d..%d" %
          (C, K, len(c.rec), len(c.lig), c.r, c.half, c.band, c.count.min(), c.count.max()))
    assert count.dtype == np.int32 and count.shape == (K,)
    assert (count == c.count).all(), (count, c.count)
    assert c.count[0] == C                                                              # the native pose: every contact holds
    if K >= 5:
        assert c.count[K - 1] == 0 and len(set(c.count.tolist())) >= 3                 # none holds 30 A away; and in between


def check_contacts_limit(lib, device):
    """NLa = 2048 runs (and NLa = 512 / 513, either side of the small instance); 2049 is refused"""
    import pytest
    for pad in (512, 513, 2048):
        check_contacts(lib, device, 65, 5, pad_to=pad, guard=torch.device(device).type == "cuda")
    c = contact_case(1, 65, 5, 2048)
    c2 = Case()
    c2.__dict__.update(c.__dict__)
    c2.lig = np.concatenate([c.lig, np.zeros((1, 3))])
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        _contacts_on_device(lib, device, c2)


# ----------------------------------------------------------------------------------------------------------------------
# 3: the class
# ----------------------------------------------------------------------------------------------------------------------

# (count of C = 1000 contacts, lrmsd, irmsd) -> class: every branch of every if, the ``or irmsd`` branches with fnat < 0.1
TABLE = [((0, 50.0, 50.0), 0), ((99, 5.0, 50.0), 0), ((101, 10.0, 50.0), 1), ((101, 10.5, 50.0), 0), ((1000, 10.5, 4.5), 0),
         ((0, 50.0, 4.0), 1), ((0, 50.0, 4.5), 0), ((99, 0.5, 3.0), 1), ((301, 5.0, 50.0), 2), ((301, 5.5, 50.0), 1),
         ((299, 4.0, 50.0), 1), ((0, 50.0, 2.0), 2), ((0, 50.0, 2.5), 1), ((301, 12.0, 2.0), 2), ((501, 1.0, 50.0), 3),
         ((501, 1.5, 50.0), 2), ((499, 0.5, 50.0), 2), ((0, 50.0, 1.0), 3), ((0, 50.0, 0.5), 3), ((600, 12.0, 1.5), 2),
         ((501, 1.0, 0.5), 3), ((1000, 0.0, 0.0), 3), ((100, 10.0, 4.5), 0), ((300, 5.0, 2.5), 1), ((500, 1.0, 1.5), 2)]


def check_capri_table(lib, device):
    from deeplocalproteindocking_amd import ops
    C = 1000
    for (cnt, l, i), want in TABLE:
        assert cascade(cnt / (C + 0.001), l, i) == want, (cnt, l, i, want)              # the table against the definition
    count = torch.tensor([t[0][0] for t in TABLE], dtype=torch.int32).to(device)
    lr = torch.tensor([t[0][1] for t in TABLE], dtype=torch.float64).to(device)
    ir = torch.tensor([t[0][2] for t in TABLE], dtype=torch.float64).to(device)
    fnat, capri = ops.pose_capri(count, ir, lr, C, lib=lib)
    assert capri.dtype == torch.int32 and capri.cpu().tolist() == [t[1] for t in TABLE]
    assert fnat.cpu().numpy().tobytes() == (count.cpu().numpy().astype(np.float64) / (C + 0.001)).tobytes()
    f0, c0 = ops.pose_capri(count, ir, lr, 0, lib=lib)                                  # C = 0: fnat = 0
    assert (f0.cpu().numpy()[count.cpu().numpy() == 0] == 0).all()


def _assert_cascade(irmsd, lrmsd, fnat, capri):
    want = [cascade(f, l, i) for f, l, i in zip(fnat, lrmsd, irmsd)]
    assert capri.tolist() == want


def _target(c, device):
    """a NativeReference of a contact case: its residues' first atoms as the interface and ligand points of the RMSDs"""
    rfirst = sorted(set(int(r[0]) for r in c.ranges))
    lfirst = sorted(set(int(r[2]) for r in c.ranges))
    a, y = c.rec[rfirst], c.lig[lfirst]
    q = np.concatenate([a, y @ c.Rn.T + c.tn])
    return (a, y, q), reference_of([(a, y, q)], c.lig, c.lig @ c.Rn.T + c.tn, c.rec, c.lig, c.ranges, c.r, device)


def check_evaluate(lib, device, C=65, K=65):
    """pose_evaluate: the four outputs against the truth, and the class exactly the cascade of the device's own outputs"""
    from deeplocalproteindocking_amd import ops
    c = contact_case(1, C, K)
    pair, native = _target(c, device)
    ir, lr, fnat, capri = (v.cpu().numpy() for v in ops.pose_evaluate(c.P, native, lib=lib))
    _assert_cascade(ir, lr, fnat, capri)
    assert fnat.tobytes() == (c.count.astype(np.float64) / (C + 0.001)).tobytes()
    i2, iscale, ikappa = irmsd64([pair], c.P)
    l2, lscale, lkappa = lrmsd64(c.lig, c.lig @ c.Rn.T + c.tn, c.P)
    assert (np.abs(ir ** 2 - i2) <= band_i(ikappa) * iscale).all() and (np.abs(lr ** 2 - l2) <= band_l(lkappa) * lscale).all()
    assert capri[0] == 3 and capri[K - 1] == 0 and ir[0] ** 2 <= band_i(ikappa) * iscale[0]


def check_ladder(lib, device):
    """The native placement times rotations of 0, 1, 4, 12 and 40 degrees about the interface centroid: the float64 quantities
    lie away from every threshold by more than the bands, and the device's classes are the truth's."""
    from deeplocalproteindocking_amd import ops
    c = contact_case(3, 257, 1)
    lfirst = sorted(set(int(r[2]) for r in c.ranges))
    centre = (c.lig[lfirst] @ c.Rn.T + c.tn).mean(axis=0)
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    P = np.zeros((5, 12))
    for k, deg in enumerate((0.0, 1.0, 4.0, 12.0, 40.0)):
        Q = pg._expm(axis * np.radians(deg))
        P[k] = pose_rows(Q @ c.Rn, Q @ (c.tn - centre) + centre)[0]
    near = []
    dmin = min_distances(c.rec, c.lig, c.ranges, P, near)
    M = max(np.abs(c.rec).max() * np.sqrt(3.0), np.abs(P[:, 9:]).max() + np.linalg.norm(c.lig, axis=1).max())
    c2 = Case()
    c2.__dict__.update(c.__dict__)
    c2.r, c2.half, c2.band = tuned_cutoff(near, M)
    pair, native = _target(c2, device)
    count = (dmin <= c2.r).sum(axis=1)
    fnat = count / (c.C + 0.001)
    i2, iscale, ikappa = irmsd64([pair], P)
    l2, lscale, lkappa = lrmsd64(c.lig, c.lig @ c.Rn.T + c.tn, P)
    bi, bl = band_i(ikappa), band_l(lkappa)
    for a, b, cc in THRESHOLDS:                                                         # the truth keeps clear of every threshold
        assert (np.abs(i2 - cc * cc) > bi * iscale).all() and (np.abs(l2 - b * b) > bl * lscale).all()
        assert (np.abs(count - a * (c.C + 0.001)) > 0.5).all()
    want = [cascade(f, l, i) for f, l, i in zip(fnat, np.sqrt(l2), np.sqrt(i2))]
    print("ladder: irmsd", np.sqrt(i2).round(3), "lrmsd", np.sqrt(l2).round(3), "fnat", fnat.round(3), "classes", want)
    assert want[0] == 3 and want[-1] < 3 and len(set(want)) >= 3
    ir, lr, f, capri = (v.cpu().numpy() for v in ops.pose_evaluate(P, native, lib=lib))
    assert capri.tolist() == want and (f == fnat).all()
    _assert_cascade(ir, lr, f, capri)


def check_large(lib, device, K=65536, sub=512):
    """K poses, the truth on a fixed subset of ``sub`` positions; the class against the cascade everywhere"""
    from deeplocalproteindocking_amd import ops
    c = contact_case(6, 16, sub, far=True)                                              # (half-gap 1.1e-4 A against 2 x 4.5e-5)
    pair, native = _target(c, device)
    where = np.linspace(0, K - 1, sub).astype(np.int64)
    rs = np.random.RandomState(12)
    P = c.P[rs.randint(0, sub, size=K)]
    P[where] = c.P
    ir, lr, fnat, capri = (v.cpu().numpy() for v in ops.pose_evaluate(P, native, lib=lib))
    assert ir.shape == (K,) and capri.shape == (K,)
    _assert_cascade(ir, lr, fnat, capri)
    assert (fnat[where] * (c.C + 0.001)).round().astype(np.int32).tolist() == c.count.tolist()
    i2, iscale, ikappa = irmsd64([pair], c.P)
    l2, lscale, lkappa = lrmsd64(c.lig, c.lig @ c.Rn.T + c.tn, c.P)
    assert (np.abs(ir[where] ** 2 - i2) <= band_i(ikappa) * iscale).all()
    assert (np.abs(lr[where] ** 2 - l2) <= band_l(lkappa) * lscale).all()


# ----------------------------------------------------------------------------------------------------------------------
# 4: errors (through ctypes)
# ----------------------------------------------------------------------------------------------------------------------

def check_errors(lib, device):
    import pytest
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    c = contact_case(1, 65, 5)
    K = 5
    mom, cnt = ops.native_moments([(c.rec[:4], c.lig[:3], np.concatenate([c.rec[:4], c.lig[:3]]))], c.lig, c.lig)
    t = dict(P=torch.from_numpy(c.P.copy()).to(dev), mom=torch.from_numpy(mom).to(dev), rec=torch.from_numpy(c.rec.astype(np.float32)).to(dev),
             lig=torch.from_numpy(c.lig.astype(np.float32)).to(dev), ranges=torch.from_numpy(c.ranges).to(dev))
    outs = dict(ir=torch.full((K,), -7.0, dtype=torch.float64, device=dev), lr=torch.full((K,), -7.0, dtype=torch.float64, device=dev),
                cnt=torch.full((K,), -7, dtype=torch.int32, device=dev), fn=torch.full((K,), -7.0, dtype=torch.float64, device=dev),
                cl=torch.full((K,), -7, dtype=torch.int32, device=dev))
    p = {k: v.data_ptr() for k, v in list(t.items()) + list(outs.items())}
    st = _stream(dev)
    NRa, NLa, C = len(c.rec), len(c.lig), c.C
    zero_nl, neg_nr = cnt.copy(), cnt.copy()
    zero_nl[0, 1], neg_nr[0, 0] = 0, -1
    no_lig = cnt.copy()
    no_lig[1, 1] = 0
    empty, outside = c.ranges.copy(), c.ranges.copy()
    empty[7, 1] = empty[7, 0]
    outside[3, 3] = NLa + 1
    many = np.ascontiguousarray(np.tile(cnt[:1], (18, 1)))

    def rmsd(P=p["P"], K_=K, mom=p["mom"], counts=cnt, nI=1, ir=p["ir"], lr=p["lr"]):
        return lib.call("dlpd_pose_native_rmsd", P, K_, mom, None if counts is None else counts.ctypes.data, nI, ir, lr, st)

    def contacts(P=p["P"], K_=K, rec=p["rec"], NRa_=NRa, lig=p["lig"], NLa_=NLa, rg=p["ranges"], rh=c.ranges, C_=C, r=5.0, cnt_=p["cnt"]):
        return lib.call("dlpd_pose_native_contacts", P, K_, rec, NRa_, lig, NLa_, rg, None if rh is None else rh.ctypes.data, C_, r, cnt_, st)

    def capri(cnt_=p["cnt"], ir=p["ir"], lr=p["lr"], C_=C, K_=K, fn=p["fn"], cl=p["cl"]):
        return lib.call("dlpd_pose_capri", cnt_, ir, lr, C_, K_, fn, cl, st)
    bad = [(rmsd, (dict(P=None), dict(mom=None), dict(counts=None), dict(ir=None), dict(lr=None), dict(K_=0), dict(K_=-2), dict(nI=0),
                   dict(counts=zero_nl), dict(counts=neg_nr), dict(counts=no_lig))),
           (contacts, (dict(P=None), dict(cnt_=None), dict(rec=None), dict(lig=None), dict(rg=None), dict(rh=None), dict(K_=0), dict(C_=-1),
                       dict(r=float("nan")), dict(r=-1.0), dict(rh=empty), dict(rh=outside), dict(NRa_=-1))),
           (capri, (dict(cnt_=None), dict(ir=None), dict(lr=None), dict(fn=None), dict(cl=None), dict(K_=0), dict(C_=-1)))]
    for fn, cases in bad:
        for kw in cases:
            with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
                fn(**kw)
    for fn, kw in ((rmsd, dict(K_=65537)), (rmsd, dict(nI=17, counts=many)), (contacts, dict(K_=65537)), (contacts, dict(NLa_=2049)),
                   (contacts, dict(NRa_=65537)), (contacts, dict(C_=65537)), (capri, dict(K_=65537)), (capri, dict(C_=65537))):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            fn(**kw)                                                                    # (refused before anything is read)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for k, v in outs.items():
        assert (v == -7).all(), k                                                       # nothing was written
    assert rmsd() == 0 and contacts() == 0 and capri() == 0 and contacts(C_=0, rg=None, rh=None) == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert (outs["cnt"] == 0).all()                                                     # C = 0: every count 0
    with pytest.raises(RuntimeError, match="float64"):
        ops.pose_native_rmsd(t["P"].float(), t["mom"], cnt, lib=lib)
    with pytest.raises(RuntimeError, match="interface pairs"):
        ops.native_moments([], c.lig, c.lig)
    with pytest.raises(RuntimeError, match="nl >= 1"):
        ops.native_moments([(c.rec[:4], c.lig[:0], c.rec[:4])], c.lig, c.lig)


# ----------------------------------------------------------------------------------------------------------------------
# 5: end to end on synthetic PDB files
# ----------------------------------------------------------------------------------------------------------------------

def _files(tmp_path):
    from synth_pdb import write_protein_like_pdb
    frec, flig = str(tmp_path / "r.pdb"), str(tmp_path / "l.pdb")
    write_protein_like_pdb(frec, 40, seed=5, extras=False)
    write_protein_like_pdb(flig, 30, seed=6, offset=(6.0, 3.0, -2.0), extras=False)       # two globules in contact
    return frec, flig


def _docker(lib, device, randomize):
    from cluster_checks import RES, _Model
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Models import SimpleFilter
    R = _random_rotations(np.random.RandomState(8), 6)
    return Docker(_Model(SimpleFilter([2]).to(device)), box_size=16, resolution=RES, max_conf=10, rotations=R, device=device, lib=lib,
                  randomize_rot=randomize, rotation_seed=4)


def check_docker_evaluate(lib, device, tmp_path):
    from cluster_checks import RES
    from deeplocalproteindocking_amd.Results import InterfaceSelection as isel
    frec, flig = _files(tmp_path)
    native = isel.native_reference(frec, flig, frec, flig)                              # unbound = bound
    assert native.C > 0 and native.counts[0, 1] >= 1 and tuple(native.ranges_host.shape) == (native.C, 4)
    ur, ul = isel.read_structure(frec), isel.read_structure(flig)
    tn = isel.bbox_centre(ul) - isel.bbox_centre(ur)
    rs = np.random.RandomState(3)
    Rs = [np.eye(3), np.eye(3)] + [pg._expm(rs.normal(size=3) * np.radians(6.0)) for _ in range(6)]
    ts = [tn, tn + [30.0, 0.0, 0.0]] + [tn + rs.normal(size=3) * 1.5 for _ in range(6)]
    dk = _docker(lib, device, False)
    refined = [(Rs[k], tuple(float(v) for v in ts[k] / RES), -1.0 * k, k) for k in range(len(Rs))]
    ev = dk.evaluate(native, poses=refined)
    assert ev is dk.evaluation and sorted(ev) == ["capri", "fnat", "irmsd", "lrmsd"] and all(len(v) == len(Rs) for v in ev.values())
    assert round(ev["fnat"][0] * (native.C + 0.001)) == native.C and ev["capri"][0] == 3
    assert ev["capri"][1] == 0 and ev["fnat"][1] == 0 and ev["irmsd"][1] > 4.0          # 30 A away
    assert ev["capri"].dtype == np.int32 and ev["irmsd"].dtype == np.float64
    _assert_cascade(ev["irmsd"], ev["lrmsd"], ev["fnat"], ev["capri"])
    # against the truth on the reference's own point sets
    P = pose_rows(np.stack(Rs), np.stack(ts))
    assert np.abs(dk.dat_frame_poses(refined) - P).max() <= 1e-12
    i2, iscale, ikappa = irmsd64(native.pairs, P)
    l2, lscale, lkappa = lrmsd64(native.ligand_ca, native.target_ca, P)
    assert (np.abs(ev["irmsd"] ** 2 - i2) <= band_i(ikappa) * iscale).all() and (np.abs(ev["lrmsd"] ** 2 - l2) <= band_l(lkappa) * lscale).all()
    print("native pose: irmsd %.3g lrmsd %.3g fnat %.4f class %d (C = %d)" % (ev["irmsd"][0], ev["lrmsd"][0], ev["fnat"][0], ev["capri"][0], native.C))
    assert ev["irmsd"][0] ** 2 <= band_i(ikappa) * iscale[0] and ev["lrmsd"][0] ** 2 <= band_l(lkappa) * lscale[0]   # within the band of 0
    # the three list forms: grid poses as top_list entries, as refined_list entries and as clustered_list entries
    L = dk.box_size
    top = [(k % 6, (3 * k) % (2 * L), (5 * k + 17) % (2 * L), (7 * k + 30) % (2 * L), -float(k)) for k in range(9)]
    as_refined = [(dk.rot.R[e[0]].double().cpu().numpy(), dk.signed_translation(*e[1:4]), e[4], k) for k, e in enumerate(top)]
    as_clustered = [e + (1,) for e in as_refined]
    dk.top_list = list(top)
    a = {k: v.copy() for k, v in dk.evaluate(native).items()}
    b = {k: v.copy() for k, v in dk.evaluate(native, poses=as_refined).items()}
    cl = dk.evaluate(native, poses=as_clustered)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == cl[k].tobytes(), k
    assert dk.top_list == top
    # the frame: a Docker that searched a randomly rotated receptor holds (randR R, randR t); its .dat poses are the same
    dr = _docker(lib, device, True)
    Q = dr.randR.squeeze().double().numpy()
    assert np.abs(Q - np.eye(3)).max() > 0.1
    rotated = [(Q @ Rs[k], tuple(float(v) for v in Q @ ts[k] / RES), -1.0 * k, k) for k in range(len(Rs))]
    assert np.abs(dr.dat_frame_poses(rotated) - P).max() <= 1e-12
    er = dr.evaluate(native, poses=rotated)
    assert (np.abs(er["irmsd"] ** 2 - i2) <= band_i(ikappa) * iscale).all() and (np.abs(er["lrmsd"] ** 2 - l2) <= band_l(lkappa) * lscale).all()
    assert (er["capri"] == ev["capri"]).all() and (er["fnat"] == ev["fnat"]).all()
    # the written poses give the same four arrays, and write_evaluation one line per pose
    for d, poses, name in ((dk, refined, "a"), (dr, rotated, "b")):
        d.refined_list = list(poses)
        d.new_log(str(tmp_path / (name + ".dat")))
        d.write_refined_conformations()
        d.cleanup()
        d.evaluate(native, poses=poses)
        d.new_log(str(tmp_path / (name + ".eval.txt")))
        d.write_evaluation()
        d.cleanup()
    assert np.abs(np.loadtxt(str(tmp_path / "a.dat")) - np.loadtxt(str(tmp_path / "b.dat"))).max() <= 2e-6    # (%f: six decimals)
    rows = [ln.split("\t") for ln in open(str(tmp_path / "b.eval.txt")).read().strip().split("\n")]
    assert len(rows) == len(Rs) and all(len(r) == 4 for r in rows) and [int(r[3]) for r in rows] == ev["capri"].tolist()
    assert dk.evaluate(native, poses=[])["capri"].shape == (0,)
    return native


def check_evaluate_target_device(lib, device, tmp_path):
    """a .dat file through ``evaluate_target_device`` against the existing host loop (``evaluate_target``: one svdvals per
    pose), truncated translations included"""
    from deeplocalproteindocking_amd.Results import DockerParser
    from deeplocalproteindocking_amd.Results import InterfaceSelection as isel
    frec, flig = _files(tmp_path)
    ur, ul = isel.read_structure(frec), isel.read_structure(flig)
    tn = isel.bbox_centre(ul) - isel.bbox_centre(ur)
    rs = np.random.RandomState(9)
    rows = []
    for k in range(7):
        R = np.eye(3) if k == 0 else pg._expm(rs.normal(size=3) * np.radians(8.0 * k))
        t = tn + (0.0 if k == 0 else 1.0) * rs.normal(size=3) * 3.0
        rows.append("\t".join("%f" % v for v in list(R.reshape(-1)) + list(t) + [-float(k)]))
    (tmp_path / "T.dat").write_text("\n".join(rows) + "\n")
    dp = DockerParser(str(tmp_path), coords_backend=object())
    want = np.array(isel.evaluate_target(dp, "T", frec, flig, frec, flig))
    got = isel.evaluate_target_device(dp, "T", frec, flig, frec, flig, device=device, lib=lib)
    assert isel.evaluate_target_device(dp, "missing", frec, flig, frec, flig, device=device, lib=lib) is None
    P = isel.conformation_poses(dp.target_dict["conformations"])
    assert (P[:, 9:] == np.trunc(P[:, 9:])).all() and np.abs(P[0, 9:] - tn).max() > 0.01       # truncated as parse_output keeps them
    _, iscale, ikappa = irmsd64(got["native"].pairs, P)
    print("evaluate_target_device:", got["irmsd"], want, band_i(ikappa) * iscale)
    assert got["irmsd"].shape == (7,) and (np.abs(got["irmsd"] ** 2 - want ** 2) <= band_i(ikappa) * iscale).all()
    assert 0.0 < got["irmsd"][0] < 1.5                                                  # off by the truncated fraction of t only
    _assert_cascade(got["irmsd"], got["lrmsd"], got["fnat"], got["capri"])
    two = isel.evaluate_target_device(dp, "T", frec, flig, frec, flig, num_conf=2, device=device, lib=lib)
    assert two["capri"].tolist() == got["capri"][:2].tolist()


def check_dock_pair(lib, device, tmp_path):
    """the script's own --native step (``evaluate_and_write``) on a searched list: <out>.eval.txt, one line per pose"""
    import cluster_checks as cc
    from deeplocalproteindocking_amd.Results import InterfaceSelection as isel
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import dock_pair
    frec, flig = _files(tmp_path)
    native = isel.native_reference(frec, flig, frec, flig).to(device)
    dk = cc._searched(lib, device, 16, K=40)
    top = list(dk.top_list)
    out = str(tmp_path / "pair.dat")
    name = dock_pair.evaluate_and_write(dk, native, out)
    assert name == str(tmp_path / "pair.eval.txt") and dk.top_list == top
    rows = [ln.split("\t") for ln in open(name).read().strip().split("\n")]
    assert len(rows) == 40 and all(len(r) == 4 for r in rows)
    assert [int(r[3]) for r in rows] == dk.evaluation["capri"].tolist()
    assert np.allclose([float(r[0]) for r in rows], dk.evaluation["irmsd"], atol=1e-6)
    dk.cluster(cc.atoms(6, n=40), radius=6.0)
    name = dock_pair.evaluate_and_write(dk, native, out, poses=dk.clustered_list, tag="clustered")
    assert name == str(tmp_path / "pair.clustered.eval.txt") and len(open(name).read().strip().split("\n")) == len(dk.clustered_list)
    ev = {"capri": np.array([0, 0, 2, 1, 3] + [0] * 120, dtype=np.int32), "irmsd": np.array([9.0, 8.0, 1.5, 3.0, 0.5] + [20.0] * 120)}
    rows, first = dock_pair.evaluation_summary(ev)
    assert rows == [(1, 0, 9.0), (10, 3, 0.5), (100, 3, 0.5), (125, 3, 0.5)] and first == 3
    assert dock_pair.evaluation_summary({"capri": np.zeros(4, dtype=np.int32), "irmsd": np.ones(4)}) == ([(1, 0, 1.0), (4, 0, 1.0)], None)
