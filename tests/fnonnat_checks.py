"""Check bodies of the all-contacts kernel (csrc/dlpd_contacts.h, ops.pose_contact_counts / pose_fnonnat, Docker.evaluate with
``fnonnat=True``), shared by tests/test_fnonnat_emu.py (the CPU-emulated kernels) and tests/test_fnonnat_gpu.py (the gfx950
build).  Nothing here reads the reference tree.

THE EXACT CASE.  Atom coordinates and translations are multiples of 1/8 A with |x| < 64 and the rotations are the 24 signed
axis permutations of determinant +1: a posed coordinate is a sum of one coordinate and one translation, a multiple of 1/8 below
128 (11 bits); a difference is a multiple of 1/8 below 256, its square a multiple of 1/64 below 2^16 (22 bits), the sum of three
below 2^18 (24 bits).  Every float32 product and sum of the predicate is exact, 5^2 = 25 is exact, and n_dec / n_corr must equal
integer arithmetic on coordinates times 8 (``lattice_truth``).  The sphere filter works on centroids and rounded radii that are
NOT on the lattice: this case is also the check that it never drops a pair.

THE GENERIC CASE.  The float64 truth is the least atom-pair distance of every residue pair under every pose; with ``band`` =
evaluate_checks.contact_band(M, r) -- the distance by which the float32 predicate can differ from it -- n_lo counts the pairs at
dmin <= r - band and n_hi those at dmin <= r + band: n_lo <= n <= n_hi, exact where they agree.  The share of poses where they
differ is a property of the inputs; the seeds below were chosen on the CPU for none or few (asserted <= 10 %)."""
import functools
import itertools

import numpy as np
import torch

import evaluate_checks as ec
from cluster_checks import _random_rotations, _stream

R_CUT = 5.0


class Case(object):
    pass


def signed_permutations():
    """the 24 rotations that permute the axes with signs"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return out


def _lattice_residues(rs, sizes, spread):
    """residues of ``sizes`` atoms: a centre on the lattice inside +-spread, atoms within +-2 A of it, all multiples of 1/8"""
    rows, off = [], [0]
    for n in sizes:
        cen = rs.randint(-8 * spread, 8 * spread + 1, size=3)
        rows.append(cen + (rs.randint(-16, 17, size=(n, 3)) if n > 1 else np.zeros((1, 3), dtype=np.int64)))
        off.append(off[-1] + n)
    return np.concatenate(rows).astype(np.int64), np.asarray(off, dtype=np.int32)


def _mixed_sizes(nres):
    return [14 if i % 4 == 1 else 1 for i in range(nres)]


def sizes_for_atoms(total):
    """residues of 14 atoms, then of 1, that hold ``total`` atoms"""
    return [14] * (total // 14) + [1] * (total % 14)


@functools.lru_cache(maxsize=None)
def lattice_case(NRres, NLres, K, seed=0, lig_atoms=None):
    """integer coordinates (units of 1/8 A), poses from the 24 signed permutations, the native set a random third of the
    residue pairs (some named twice), and the integer truth"""
    rs = np.random.RandomState(9000 + seed)
    c = Case()
    lsizes = _mixed_sizes(NLres) if lig_atoms is None else sizes_for_atoms(lig_atoms)
    spread = 10 if lig_atoms is None else 30
    c.rec8, c.rec_off = _lattice_residues(rs, _mixed_sizes(NRres), min(spread, 10 + NRres // 20))
    c.lig8, c.lig_off = _lattice_residues(rs, lsizes, spread)
    assert np.abs(c.rec8).max() < 40 * 8 and np.abs(c.lig8).max() < 40 * 8
    rots = signed_permutations()
    c.P = np.zeros((K, 12))
    c.R8, c.t8 = [], []
    for k in range(K):
        R, t8 = rots[k % 24], rs.randint(-8 * 8, 8 * 8 + 1, size=3)                     # |t| <= 8 A: |posed| < 64
        c.P[k] = ec.pose_rows(R, t8 / 8.0)[0]
        c.R8.append(R.astype(np.int64))
        c.t8.append(t8.astype(np.int64))
    nl = len(c.lig_off) - 1
    allp = [(i, j) for i in range(NRres) for j in range(nl)]
    pick = [allp[i] for i in rs.permutation(len(allp))[:max(1, len(allp) // 3)]]
    c.native_pairs = pick + pick[:len(pick) // 4]                                        # duplicates: a set all the same
    c.n_dec, c.n_corr = lattice_truth(c)
    return c


def _residue_min(D, roff, loff):
    """(NRa, NLa) -> (NRres, NLres): the minimum over the atoms of every residue pair (no empty residues)"""
    return np.minimum.reduceat(np.minimum.reduceat(D, roff[:-1], axis=0), loff[:-1], axis=1)


def lattice_truth(c):
    nat = np.zeros((len(c.rec_off) - 1, len(c.lig_off) - 1), dtype=bool)
    for i, j in c.native_pairs:
        nat[i, j] = True
    n_dec, n_corr = [], []
    for R8, t8 in zip(c.R8, c.t8):
        X = c.lig8 @ R8.T + t8
        assert np.abs(X).max() < 64 * 8
        D = ((c.rec8[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)                      # int64, units of 1/64 A^2
        hit = _residue_min(D, c.rec_off, c.lig_off) <= int(R_CUT * 8) ** 2
        n_dec.append(int(hit.sum()))
        n_corr.append(int((hit & nat).sum()))
    return np.array(n_dec, dtype=np.int32), np.array(n_corr, dtype=np.int32)


def native_of(rec, rec_off, lig, lig_off, native_pairs, device, interface=True, cutoff=R_CUT):
    """a NativeReference with the all-contacts tables; ``interface``: the contact ranges of the native pairs over the same
    arrays (what pose_native_contacts reads), else one placeholder range"""
    from deeplocalproteindocking_amd.Results.InterfaceSelection import native_reference_from_points
    a, y = rec[:3], lig[:2]
    pairs = [(a, y, np.concatenate([a, y]))]
    if interface:
        ranges = [(rec_off[i], rec_off[i + 1], lig_off[j], lig_off[j + 1]) for i, j in native_pairs]
        ra, la = rec, lig
    else:
        ranges, ra, la = [(0, 1, 0, 1)], rec[:1], lig[:1]
    return native_reference_from_points(pairs, lig[:2], lig[:2], ra, la, ranges, cutoff, all_rec=(rec, rec_off), all_lig=(lig, lig_off),
                                        all_pairs=native_pairs).to(device)


def counts_on_device(lib, device, native, P, guard=False):
    from deeplocalproteindocking_amd import ops
    P = torch.from_numpy(np.array(P)).to(device)
    if guard:
        from guard_alloc import GuardedAllocations
        with GuardedAllocations(min_bytes=4) as g:
            nd, nc = ops.pose_contact_counts(P, native, lib=lib)
            bad = g.check(release=False)
        assert not bad, bad
    else:
        nd, nc = ops.pose_contact_counts(P, native, lib=lib)
    assert nd.dtype == torch.int32 and nc.dtype == torch.int32 and tuple(nd.shape) == (P.shape[0],) == tuple(nc.shape)
    return nd.cpu().numpy(), nc.cpu().numpy()


def _is_gpu(device):
    return torch.device(device).type == "cuda"


# ----------------------------------------------------------------------------------------------------------------------
# 1: the exact case
# ----------------------------------------------------------------------------------------------------------------------

def check_exact(lib, device, NRres, NLres, K):
    c = lattice_case(NRres, NLres, K)
    native = native_of(c.rec8 / 8.0, c.rec_off, c.lig8 / 8.0, c.lig_off, c.native_pairs, device, interface=False)
    nd, nc = counts_on_device(lib, device, native, c.P, guard=_is_gpu(device))
    print("exact (NRres, NLres, K) = (%d, %d, %d): NRa %d, NLa %d, n_dec %d..%d, n_corr %d..%d" %
          (NRres, NLres, K, len(c.rec8), len(c.lig8), c.n_dec.min(), c.n_dec.max(), c.n_corr.min(), c.n_corr.max()))
    assert (nd == c.n_dec).all(), (nd, c.n_dec)
    assert (nc == c.n_corr).all(), (nc, c.n_corr)
    if NRres * NLres >= 100:
        assert c.n_dec.max() > 0 and (c.n_corr < c.n_dec).any() and c.n_corr.max() > 0   # the case measures something


def check_exact_capacity(lib, device, lig_atoms):
    """a ligand of exactly ``lig_atoms`` atoms: either side of the small instance (2048), the large one's capacity (8192)"""
    c = lattice_case(5, 0, 3, seed=lig_atoms, lig_atoms=lig_atoms)
    assert len(c.lig8) == lig_atoms
    native = native_of(c.rec8 / 8.0, c.rec_off, c.lig8 / 8.0, c.lig_off, c.native_pairs, device, interface=False)
    nd, nc = counts_on_device(lib, device, native, c.P, guard=_is_gpu(device))
    print("exact, %d ligand atoms in %d residues: n_dec %s, n_corr %s" % (lig_atoms, len(c.lig_off) - 1, c.n_dec, c.n_corr))
    assert (nd == c.n_dec).all() and (nc == c.n_corr).all(), (nd, c.n_dec, nc, c.n_corr)
    assert c.n_dec.max() > 0


def check_over_capacity(lib, device):
    import pytest
    c = lattice_case(5, 0, 3, seed=8193, lig_atoms=8193)
    native = native_of(c.rec8 / 8.0, c.rec_off, c.lig8 / 8.0, c.lig_off, c.native_pairs, device, interface=False)
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        counts_on_device(lib, device, native, c.P)


# ----------------------------------------------------------------------------------------------------------------------
# 2: the sphere filter at its edge
# ----------------------------------------------------------------------------------------------------------------------

def check_sphere_edge(lib, device):
    """Two-atom residues 6 A long (radius 3) tip to tip along every axis and direction: closest atoms at r - 1/8 (counts) and
    r + 1/8 (does not); the centres are then 11 -+ 1/8 apart, the filter's bound r + 3 + 3 = 11 between them."""
    rots = signed_permutations()
    for gap8, want in ((int(R_CUT * 8) - 1, 1), (int(R_CUT * 8) + 1, 0)):
        rec8 = np.array([[-48, 8, -16], [0, 8, -16]], dtype=np.int64)                   # along x, its tip at x = 0
        lig8 = np.array([[0, 0, 0], [48, 0, 0]], dtype=np.int64)
        P, truth = [], []
        for R in rots:
            X = lig8 @ R.astype(np.int64).T
            # put the posed ligand's nearer tip ``gap8`` beyond the receptor's tip, on the receptor's axis
            tip = X[np.argmin(X[:, 0])] if abs(X[1, 0] - X[0, 0]) == 48 else None
            if tip is None:
                continue                                                                # (the ligand's axis left x: not tip to tip)
            t8 = np.array([gap8, 8, -16]) - tip
            P.append(ec.pose_rows(R, t8 / 8.0)[0])
            D = (((rec8[:, None] - (X + t8)[None]) ** 2).sum(axis=2)).min()
            truth.append(int(D <= int(R_CUT * 8) ** 2))
            cd = np.abs((rec8.mean(axis=0) - (X + t8).mean(axis=0)))[0] / 8.0
            assert abs(cd - 11.0) == 0.125
        assert len(P) == 8 and truth == [want] * 8
        native = native_of(rec8 / 8.0, np.array([0, 2], dtype=np.int32), lig8 / 8.0, np.array([0, 2], dtype=np.int32), [(0, 0)], device,
                           interface=False)
        nd, nc = counts_on_device(lib, device, native, np.array(P))
        assert nd.tolist() == truth and nc.tolist() == truth, (gap8, nd, nc)


# ----------------------------------------------------------------------------------------------------------------------
# 3, 4, 6: generic poses
# ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layers_case(seed, nres, K, far=True, extra=False):
    """Two facing layers of residues of 1 and of 14 atoms (as evaluate_checks.contact_case lays them out), every residue kept;
    the native pairs: the residue pairs within 4.6 A in the native placement; poses round the native one.  ``extra``: pose 1
    far away, pose 2 slid 12 A along both axes of the interface."""
    rs = np.random.RandomState(11000 + seed)
    c = Case()

    def layer(z):
        side = int(np.ceil(np.sqrt(nres)))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:nres] * 3.0
        cen = np.concatenate([g - g.mean(axis=0), np.full((nres, 1), z)], axis=1) + rs.normal(size=(nres, 3)) * 0.4
        return [cen[i] + (rs.normal(size=(14, 3)) * 0.9 if i % 4 == 1 else np.zeros((1, 3))) for i in range(nres)]
    off = np.array([4.0, 3.0, -6.0])
    rec_res, lig_res = [r + off for r in layer(0.0)], [r + off for r in layer(3.6)]
    Rn, tn = _random_rotations(rs, 1)[0], np.array([7.0, 2.0, -4.0])
    c.rec, lig_native = np.concatenate(rec_res), np.concatenate(lig_res)
    c.rec_off = np.cumsum([0] + [len(r) for r in rec_res]).astype(np.int32)
    c.lig_off = np.cumsum([0] + [len(r) for r in lig_res]).astype(np.int32)
    c.lig = (lig_native - tn) @ Rn
    c.P = ec.perturbed(rs, Rn, tn, lig_native.mean(axis=0), K, angle=3.0, shift=1.0, far=far)
    if extra:
        c.P[1] = ec.pose_rows(Rn, tn + [0.0, 0.0, 40.0])[0]
        c.P[2] = ec.pose_rows(Rn, tn + [12.0, 12.0, 0.0])[0]
    c.dmin = residue_distances(c.rec, c.rec_off, c.lig, c.lig_off, c.P)                 # (K, NRres, NLres)
    c.nat = c.dmin[0] <= 4.6
    c.native_pairs = [(int(i), int(j)) for i, j in zip(*np.nonzero(c.nat))]
    M = max(np.abs(c.rec).max() * np.sqrt(3.0), np.abs(c.P[:, 9:]).max() + np.linalg.norm(c.lig, axis=1).max())
    c.band = ec.contact_band(M, R_CUT)
    lo, hi = c.dmin <= R_CUT - c.band, c.dmin <= R_CUT + c.band
    c.dec_lo, c.dec_hi = lo.sum(axis=(1, 2)), hi.sum(axis=(1, 2))
    c.corr_lo, c.corr_hi = (lo & c.nat).sum(axis=(1, 2)), (hi & c.nat).sum(axis=(1, 2))
    c.Rn, c.tn = Rn, tn
    return c


def residue_distances(rec, rec_off, lig, lig_off, P):
    out = np.zeros((P.shape[0], len(rec_off) - 1, len(lig_off) - 1))
    for k in range(P.shape[0]):
        X = lig @ P[k, :9].reshape(3, 3).T + P[k, 9:]
        D = np.sqrt(((rec[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
        out[k] = _residue_min(D, rec_off, lig_off)
    return out


def _assert_between(c, nd, nc, where=slice(None)):
    open_share = float(((c.dec_lo != c.dec_hi) | (c.corr_lo != c.corr_hi)).mean())
    print("band %.3g A: %.1f %% of the %d poses have a pair inside it; n_dec %d..%d, n_corr %d..%d" %
          (c.band, 100.0 * open_share, len(c.dec_lo), c.dec_lo.min(), c.dec_hi.max(), c.corr_lo.min(), c.corr_hi.max()))
    assert open_share <= 0.10
    assert (c.dec_lo <= nd[where]).all() and (nd[where] <= c.dec_hi).all(), (nd[where], c.dec_lo, c.dec_hi)
    assert (c.corr_lo <= nc[where]).all() and (nc[where] <= c.corr_hi).all(), (nc[where], c.corr_lo, c.corr_hi)


def check_generic(lib, device, nres=144, K=65):
    c = layers_case(1, nres, K)
    native = native_of(c.rec, c.rec_off, c.lig, c.lig_off, c.native_pairs, device)
    nd, nc = counts_on_device(lib, device, native, c.P, guard=_is_gpu(device))
    _assert_between(c, nd, nc)
    assert len(set(c.dec_lo.tolist())) >= 5 and c.corr_lo[0] == len(c.native_pairs)


def check_agreement(lib, device, nres=144, K=65):
    """n_corr is the count of the existing kernel, pose for pose; the native, a far and a slid pose"""
    from deeplocalproteindocking_amd import ops
    c = layers_case(2, nres, K, extra=True)
    assert len(set(c.native_pairs)) == len(c.native_pairs)
    native = native_of(c.rec, c.rec_off, c.lig, c.lig_off, c.native_pairs, device)
    nd, nc = counts_on_device(lib, device, native, c.P)
    _assert_between(c, nd, nc)
    old = ops.pose_native_contacts(torch.from_numpy(c.P.copy()).to(device), native.rec_atoms, native.lig_atoms, native.ranges,
                                   native.ranges_host, native.contact_dist, lib=lib).cpu().numpy()
    assert (nc == old).all(), (nc, old)
    C = len(c.native_pairs)
    f = ops.pose_fnonnat(c.P, native, lib=lib)
    assert f.dtype == torch.float64 and f.device.type == torch.device(device).type
    f = f.cpu().numpy()
    assert f.tobytes() == ((nd - nc).astype(np.float64) / (nd.astype(np.float64) + 0.001)).tobytes()
    print("native pose: n_dec %d n_corr %d (C = %d) fnonnat %.4f; far: %d %d; slid: %d %d fnonnat %.4f" %
          (nd[0], nc[0], C, f[0], nd[1], nc[1], nd[2], nc[2], f[2]))
    assert nc[0] == C and nd[0] >= C
    assert nd[1] == 0 and nc[1] == 0 and f[1] == 0.0
    assert nc[2] == 0 and nd[2] > 0 and abs(f[2] - nd[2] / (nd[2] + 0.001)) < 1e-15


def check_large(lib, device, K=65536, sub=512):
    """K poses, the truth on a fixed subset of ``sub`` positions"""
    c = layers_case(3, 16, sub)
    native = native_of(c.rec, c.rec_off, c.lig, c.lig_off, c.native_pairs, device)
    where = np.linspace(0, K - 1, sub).astype(np.int64)
    P = c.P[np.random.RandomState(12).randint(0, sub, size=K)]
    P[where] = c.P
    nd, nc = counts_on_device(lib, device, native, P)
    assert nd.shape == (K,)
    _assert_between(c, nd, nc, where)
    assert (nc <= nd).all() and nd.max() <= 16 * 16


# ----------------------------------------------------------------------------------------------------------------------
# 5: the formula against the fixture
# ----------------------------------------------------------------------------------------------------------------------

def fixture():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_training_data.json")) as fin:
        return json.load(fin)


def check_formula():
    """ops.fnonnat_of on the fixture's (n_dec, n_corr): the numbers ``_get_fnat`` gave for sets of those sizes"""
    from deeplocalproteindocking_amd import ops
    rows = fixture()["fnat_cases"]
    assert len(rows) >= 8
    nd = torch.tensor([r["n_dec"] for r in rows], dtype=torch.int32)
    nc = torch.tensor([r["n_corr"] for r in rows], dtype=torch.int32)
    got = ops.fnonnat_of(nd, nc).numpy()
    assert got.dtype == np.float64
    assert got.tolist() == [r["fnonnat"] for r in rows]


# ----------------------------------------------------------------------------------------------------------------------
# 7: errors (through ctypes)
# ----------------------------------------------------------------------------------------------------------------------

def check_errors(lib, device):
    import pytest
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.Results.InterfaceSelection import native_reference_from_points
    dev = torch.device(device)
    c = layers_case(1, 16, 5)
    native = native_of(c.rec, c.rec_off, c.lig, c.lig_off, c.native_pairs, device)
    tb = native.all
    K = 5
    P = torch.from_numpy(c.P.copy()).to(dev)
    nd = torch.full((K,), -7, dtype=torch.int32, device=dev)
    nc = torch.full((K,), -7, dtype=torch.int32, device=dev)
    st = _stream(dev)
    NRa, NLa, NRres, NLres = len(c.rec), len(c.lig), len(c.rec_off) - 1, len(c.lig_off) - 1
    roh, loh = tb["rec_off_host"], tb["lig_off_host"]
    bad_r, bad_l, long_l = roh.copy(), loh.copy(), loh.copy()
    bad_r[2] = bad_r[3] + 1
    bad_l[0] = -1
    long_l[-1] = NLa + 1
    base = dict(P=P.data_ptr(), K_=K, ra=tb["rec_atoms"].data_ptr(), ro=tb["rec_off"].data_ptr(), rs=tb["rec_sph"].data_ptr(), NRa_=NRa,
                NRres_=NRres, la=tb["lig_atoms"].data_ptr(), lo=tb["lig_off"].data_ptr(), ls=tb["lig_sph"].data_ptr(), NLa_=NLa, NLres_=NLres,
                roh=roh, loh=loh, bits=tb["native_bits"].data_ptr(), ext=tb["lig_extent"], r=5.0, nd=nd.data_ptr(), nc=nc.data_ptr())

    def call(**kw):
        a = dict(base)
        a.update(kw)
        return lib.call("dlpd_pose_contacts_all", a["P"], a["K_"], a["ra"], a["ro"], a["rs"], a["NRa_"], a["NRres_"], a["la"], a["lo"], a["ls"],
                        a["NLa_"], a["NLres_"], None if a["roh"] is None else a["roh"].ctypes.data,
                        None if a["loh"] is None else a["loh"].ctypes.data, a["bits"], a["ext"], a["r"], a["nd"], a["nc"], st)
    for name in ("P", "ra", "ro", "rs", "la", "lo", "ls", "roh", "loh", "bits", "nd", "nc"):
        with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
            call(**{name: None})
    for kw in (dict(K_=-1), dict(NRa_=0), dict(NLa_=0), dict(NRres_=0), dict(NLres_=0), dict(r=float("nan")), dict(r=-1.0),
               dict(ext=float("nan")), dict(roh=bad_r), dict(loh=bad_l), dict(loh=long_l)):
        with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
            call(**kw)
    for kw in (dict(K_=65537), dict(NLa_=8193), dict(NLres_=1025), dict(NRa_=65537), dict(NRres_=8193)):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            call(**kw)                                                                  # (refused before anything is read)
    assert call(K_=0) == 0                                                              # a no-op
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert (nd == -7).all() and (nc == -7).all()                                        # nothing was written
    assert call() == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert (nd.cpu().numpy() >= c.dec_lo).all() and (nd.cpu().numpy() <= c.dec_hi).all()
    plain = native_reference_from_points([(c.rec[:3], c.lig[:2], np.concatenate([c.rec[:3], c.lig[:2]]))], c.lig[:2], c.lig[:2], c.rec[:1],
                                         c.lig[:1], [(0, 1, 0, 1)]).to(device)
    assert plain.all is None
    for fn in (ops.pose_contact_counts, ops.pose_fnonnat):
        with pytest.raises(RuntimeError, match="all_contacts"):
            fn(P, plain, lib=lib)
    with pytest.raises(RuntimeError, match="go together"):
        native_reference_from_points([(c.rec[:3], c.lig[:2], np.concatenate([c.rec[:3], c.lig[:2]]))], c.lig[:2], c.lig[:2], c.rec[:1],
                                     c.lig[:1], [(0, 1, 0, 1)], all_rec=(c.rec, c.rec_off))
    with pytest.raises(RuntimeError, match="outside"):
        ops.contact_tables(c.rec, c.rec_off, c.lig, c.lig_off, [(NRres, 0)])
