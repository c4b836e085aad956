"""Check bodies of the interface kernels (csrc/dlpd_interface.h, ops.pose_interface_bits / interface_profile / interface_within /
interface_cluster / unpack_bits, Docker.interface / cluster_interface), shared by tests/test_interface_emu.py (the CPU-emulated
kernels) and tests/test_interface_gpu.py (the gfx950 build).  Nothing here reads the reference tree: the step is build-defined.

THE EXACT CASE is fnonnat_checks' lattice: coordinates and translations multiples of 1/8 A, the 24 signed axis permutations, so every
float32 operation of the predicate is exact and a residue's bit must equal ``hit.any`` of the int64 residue-pair matrix.  The seeds
(``SEEDS``) were fixed after checking on the CPU that every case with NRres NLres >= 100 has, on each side, a set bit and a clear bit
below the residue count (asserted again in the check).

THE GENERIC CASE is fnonnat_checks' two layers with its float64 distances: bits_lo <= bits <= bits_hi at r -+ band, band =
evaluate_checks.contact_band.

THE PROFILE's reference is a host float64 sum in the documented order: np.cumsum (sequential) over where(bit, w, 0) within chunks of
1,024 poses, then np.cumsum over the chunk partials.  Adding 0.0 changes no partial, so this is the kernel's sum bit for bit.

THE SIMILARITY BITMAP's reference is the integer test in numpy on the unpacked fingerprints."""
import functools

import numpy as np
import torch

import evaluate_checks as ec
from cluster_checks import _stream, greedy64, unpack
from fnonnat_checks import R_CUT, _residue_min, lattice_case, layers_case, native_of, signed_permutations

# (NRres, NLres, K) or ligand atoms -> seed of lattice_case where the default leaves a side all set or all clear
SEEDS = {(3, 63, 1): 3, 8192: 2}
EXACT_SHAPES = [(1, 1), (31, 3), (32, 3), (33, 65), (3, 63), (3, 64), (65, 3), (129, 67), (130, 513)]
FULL = np.uint32(0xFFFFFFFF)


def _is_gpu(device):
    return torch.device(device).type == "cuda"


def _sync(device):
    if _is_gpu(device):
        torch.cuda.synchronize()


def tables_on(tb, device):
    """the dict of ops.contact_tables with its tensors on ``device``"""
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in tb.items()}


def tables_of(rec, rec_off, lig, lig_off, device):
    from deeplocalproteindocking_amd import ops
    return tables_on(ops.contact_tables(rec, rec_off, lig, lig_off, ()), device)


def pack(hit):
    """(K, n) bool -> (K, ceil(n / 32)) uint32, bit (i & 31) of word i >> 5"""
    K, n = hit.shape
    W = (n + 31) // 32
    padded = np.zeros((K, W * 32), dtype=np.uint64)
    padded[:, :n] = hit
    return (padded.reshape(K, W, 32) << np.arange(32, dtype=np.uint64)[None, None]).sum(axis=2).astype(np.uint32)


def unpack32(words, n):
    w = np.ascontiguousarray(words).view(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None]) & np.uint32(1)).astype(bool).reshape(w.shape[0], -1)[:, :n]


def popcount(words):
    w = np.ascontiguousarray(words).view(np.uint32)
    return unpack32(w, 32 * w.shape[1]).sum(axis=1)


def raw_bits(lib, device, tb, poses, cutoff=R_CUT, **kw):
    """dlpd_pose_residue_bits through ctypes into buffers that hold 0xFFFFFFFF everywhere: an unwritten word or a set padding bit
    shows -> (rc, rec_bits, lig_bits) uint32 numpy"""
    dev = torch.device(device)
    P = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float64))).to(dev)
    roh, loh = tb["rec_off_host"], tb["lig_off_host"]
    NRres, NLres = len(roh) - 1, len(loh) - 1
    K = P.shape[0]
    rb = torch.full((K, (NRres + 31) // 32), -1, dtype=torch.int32, device=dev)
    lb = torch.full((K, (NLres + 31) // 32), -1, dtype=torch.int32, device=dev)
    a = dict(P=P.data_ptr(), K_=K, ra=tb["rec_atoms"].data_ptr(), ro=tb["rec_off"].data_ptr(), rs=tb["rec_sph"].data_ptr(),
             NRa_=tb["rec_atoms"].shape[0], NRres_=NRres, la=tb["lig_atoms"].data_ptr(), lo=tb["lig_off"].data_ptr(), ls=tb["lig_sph"].data_ptr(),
             NLa_=tb["lig_atoms"].shape[0], NLres_=NLres, roh=roh, loh=loh, ext=tb["lig_extent"], r=cutoff, rb=rb.data_ptr(), lb=lb.data_ptr())
    a.update(kw)
    rc = lib.call("dlpd_pose_residue_bits", a["P"], a["K_"], a["ra"], a["ro"], a["rs"], a["NRa_"], a["NRres_"], a["la"], a["lo"], a["ls"],
                  a["NLa_"], a["NLres_"], None if a["roh"] is None else a["roh"].ctypes.data, None if a["loh"] is None else a["loh"].ctypes.data,
                  a["ext"], a["r"], a["rb"], a["lb"], _stream(dev))
    _sync(dev)
    return rc, rb.cpu().numpy().view(np.uint32), lb.cpu().numpy().view(np.uint32)


def ops_bits(lib, device, tb, P, cutoff=R_CUT):
    """ops.pose_interface_bits; on the GPU under guarded allocations whose ``empty`` holds 0xFF bytes"""
    from deeplocalproteindocking_amd import ops
    P = torch.from_numpy(np.ascontiguousarray(np.asarray(P, dtype=np.float64))).to(device)
    if _is_gpu(device):
        from guard_alloc import GuardedAllocations
        with GuardedAllocations(min_bytes=4, empty_byte=0xFF) as g:
            rb, lb = ops.pose_interface_bits(P, tb, cutoff, lib=lib)
            bad = g.check(release=False)
        assert not bad, bad
    else:
        rb, lb = ops.pose_interface_bits(P, tb, cutoff, lib=lib)
    assert rb.dtype == torch.int32 and lb.dtype == torch.int32 and rb.device.type == torch.device(device).type
    return rb.cpu().numpy().view(np.uint32), lb.cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------
# 1: bits are integer arithmetic
# ----------------------------------------------------------------------------------------------------------------------

def lattice_hits(c):
    """the int64 residue-pair matrix of every pose -> (K, NRres, NLres) bool"""
    out = []
    for R8, t8 in zip(c.R8, c.t8):
        X = c.lig8 @ R8.T + t8
        D = ((c.rec8[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)                      # int64, units of 1/64 A^2
        out.append(_residue_min(D, c.rec_off, c.lig_off) <= int(R_CUT * 8) ** 2)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def exact_case(NRres, NLres, K, lig_atoms=None):
    if lig_atoms is None:
        c = lattice_case(NRres, NLres, K, seed=SEEDS.get((NRres, NLres, K), 0))
    else:
        c = lattice_case(NRres, 0, K, seed=SEEDS.get(lig_atoms, lig_atoms), lig_atoms=lig_atoms)
    hit = lattice_hits(c)
    return c, hit.any(axis=2), hit.any(axis=1)


def measures_something(rt, lt):
    return bool(rt.any() and (~rt).any() and lt.any() and (~lt).any())


def check_exact(lib, device, NRres, NLres, K, lig_atoms=None):
    c, rt, lt = exact_case(NRres, NLres, K, lig_atoms)
    nl = len(c.lig_off) - 1
    assert lig_atoms is None or len(c.lig8) == lig_atoms
    tb = tables_of(c.rec8 / 8.0, c.rec_off, c.lig8 / 8.0, c.lig_off, device)
    rc, rb, lb = raw_bits(lib, device, tb, c.P)
    print("exact (NRres, NLres, K) = (%d, %d, %d), %d ligand atoms: %d / %d receptor and %d / %d ligand bits set" %
          (NRres, nl, K, len(c.lig8), rt.sum(), rt.size, lt.sum(), lt.size))
    assert rc == 0
    assert (rb == pack(rt)).all(), (rb, pack(rt))                                       # every word, padding bits included
    assert (lb == pack(lt)).all(), (lb, pack(lt))
    if NRres * nl >= 100:
        assert measures_something(rt, lt)
    rb2, lb2 = ops_bits(lib, device, tb, c.P)
    assert (rb2 == rb).all() and (lb2 == lb).all()


def check_unpack(lib, device):
    from deeplocalproteindocking_amd import ops
    rs = np.random.RandomState(5)
    hit = rs.rand(7, 70) < 0.3
    words = torch.from_numpy(pack(hit).view(np.int32)).to(device)
    got = ops.unpack_bits(words, 70)
    assert got.dtype == torch.bool and tuple(got.shape) == (7, 70) and got.device.type == torch.device(device).type
    assert (got.cpu().numpy() == hit).all() and (unpack32(pack(hit), 70) == hit).all()
    import pytest
    with pytest.raises(RuntimeError, match="hold no"):
        ops.unpack_bits(words, 97)


# ----------------------------------------------------------------------------------------------------------------------
# 2: agreement with the counting kernel
# ----------------------------------------------------------------------------------------------------------------------

def check_counts_agree(lib, device):
    from deeplocalproteindocking_amd import ops
    for NRres, NLres, side in ((33, 1, 0), (1, 33, 1)):
        c = lattice_case(NRres, NLres, 24)
        native = native_of(c.rec8 / 8.0, c.rec_off, c.lig8 / 8.0, c.lig_off, c.native_pairs, device, interface=False)
        P = torch.from_numpy(c.P.copy()).to(device)
        nd = ops.pose_contact_counts(P, native, lib=lib)[0].cpu().numpy()
        bits = ops.pose_interface_bits(P, native, R_CUT, lib=lib)
        pc = popcount(bits[side].cpu().numpy())
        print("one residue on the other side, %d x %d: n_dec %s" % (NRres, NLres, nd.tolist()))
        assert (pc == nd).all() and nd.max() > 0 and (nd == c.n_dec).all()
        assert (popcount(bits[1 - side].cpu().numpy()) == (nd > 0)).all()
    c = layers_case(2, 144, 65, extra=True)
    native = native_of(c.rec, c.rec_off, c.lig, c.lig_off, c.native_pairs, device)
    P = torch.from_numpy(c.P.copy()).to(device)
    nd = ops.pose_contact_counts(P, native, lib=lib)[0].cpu().numpy().astype(np.int64)
    rb, lb = ops.pose_interface_bits(P, native, R_CUT, lib=lib)
    pr, pl = popcount(rb.cpu().numpy()), popcount(lb.cpu().numpy())
    print("layers: n_dec %d..%d, receptor residues %d..%d, ligand residues %d..%d" % (nd.min(), nd.max(), pr.min(), pr.max(), pl.min(), pl.max()))
    assert (np.maximum(pr, pl) <= nd).all() and (nd <= pr * pl).all()
    assert ((nd == 0) == ((pr == 0) & (pl == 0))).all() and (nd == 0).any() and (nd > 0).any()


# ----------------------------------------------------------------------------------------------------------------------
# 3: generic poses, the sphere filter's edge
# ----------------------------------------------------------------------------------------------------------------------

def check_generic(lib, device, nres=144, K=65):
    c = layers_case(1, nres, K)
    tb = tables_of(c.rec, c.rec_off, c.lig, c.lig_off, device)
    rb, lb = ops_bits(lib, device, tb, c.P)
    lo, hi = c.dmin <= R_CUT - c.band, c.dmin <= R_CUT + c.band
    open_share = float((lo != hi).any(axis=(1, 2)).mean())
    print("band %.3g A: %.1f %% of the %d poses have a pair inside it" % (c.band, 100.0 * open_share, K))
    assert open_share <= 0.10
    for bits, axis, n in ((rb, 2, nres), (lb, 1, nres)):
        got = unpack32(bits, n)
        assert (bits == pack(got)).all()                                                # no padding bit
        assert (lo.any(axis=axis) <= got).all() and (got <= hi.any(axis=axis)).all()
    assert measures_something(lo.any(axis=2), lo.any(axis=1))


def check_sphere_edge(lib, device):
    """fnonnat_checks.check_sphere_edge's inputs: two-atom residues 6 A long tip to tip, the closest atoms at r - 1/8 (marked on
    both sides) and r + 1/8 (not marked); the centres are 11 -+ 1/8 apart, the filter's bound r + 3 + 3 = 11 between them"""
    rots = signed_permutations()
    for gap8, want in ((int(R_CUT * 8) - 1, 1), (int(R_CUT * 8) + 1, 0)):
        rec8 = np.array([[-48, 8, -16], [0, 8, -16]], dtype=np.int64)
        lig8 = np.array([[0, 0, 0], [48, 0, 0]], dtype=np.int64)
        P = []
        for R in rots:
            X = lig8 @ R.astype(np.int64).T
            if abs(X[1, 0] - X[0, 0]) != 48:
                continue
            t8 = np.array([gap8, 8, -16]) - X[np.argmin(X[:, 0])]
            P.append(ec.pose_rows(R, t8 / 8.0)[0])
            assert (((rec8[:, None] - (X + t8)[None]) ** 2).sum(axis=2)).min() == gap8 ** 2
        assert len(P) == 8
        tb = tables_of(rec8 / 8.0, np.array([0, 2], dtype=np.int32), lig8 / 8.0, np.array([0, 2], dtype=np.int32), device)
        rc, rb, lb = raw_bits(lib, device, tb, np.array(P))
        assert rc == 0 and rb.reshape(-1).tolist() == [want] * 8 and lb.reshape(-1).tolist() == [want] * 8, (gap8, rb, lb)


# ----------------------------------------------------------------------------------------------------------------------
# 4: the profile
# ----------------------------------------------------------------------------------------------------------------------

CHUNK = 1024


def profile_host(hit, w):
    """the documented order on the host"""
    parts = []
    for k0 in range(0, hit.shape[0], CHUNK):
        terms = np.where(hit[k0:k0 + CHUNK], w[k0:k0 + CHUNK, None], 0.0)
        parts.append(np.cumsum(terms, axis=0)[-1])
    return np.cumsum(np.stack(parts), axis=0)[-1]


@functools.lru_cache(maxsize=None)
def profile_case(K, NRres=70, NLres=33):
    rs = np.random.RandomState(400 + K)
    rh, lh = rs.rand(K, NRres) < 0.4, rs.rand(K, NLres) < 0.4
    rh[:, 3], rh[:, 4] = False, True
    w = 10.0 ** rs.uniform(-6.0, 6.0, size=K) * rs.choice([-1.0, 1.0], size=K)             # twelve orders of magnitude, both signs
    return rh, lh, w


def check_profile(lib, device, K):
    from deeplocalproteindocking_amd import ops
    rh, lh, w = profile_case(K)
    NRres, NLres = rh.shape[1], lh.shape[1]
    rb = torch.from_numpy(pack(rh).view(np.int32)).to(device)
    lb = torch.from_numpy(pack(lh).view(np.int32)).to(device)

    def run(weights):
        if _is_gpu(device):
            from guard_alloc import GuardedAllocations
            with GuardedAllocations(min_bytes=4, empty_byte=0xFF) as g:
                out = ops.interface_profile(rb, lb, NRres, NLres, weights, lib=lib)
                bad = g.check(release=False)
            assert not bad, bad
        else:
            out = ops.interface_profile(rb, lb, NRres, NLres, weights, lib=lib)
        assert out[0].dtype == torch.float64 and out[2].dtype == torch.int32 and tuple(out[0].shape) == (NRres,) and tuple(out[3].shape) == (NLres,)
        return [t.cpu().numpy() for t in out]
    rf, lf, rc, lc = run(w)
    assert (rc == rh.sum(axis=0)).all() and (lc == lh.sum(axis=0)).all()
    want_r, want_l = profile_host(rh, w), profile_host(lh, w)
    other = np.where(rh, w[:, None], 0.0).sum(axis=0)                                   # (numpy's pairwise order: not the same number)
    print("profile K = %d: %d of %d receptor frequencies differ from a pairwise sum" % (K, int((other != want_r).sum()), NRres))
    assert rf.tobytes() == want_r.tobytes() and lf.tobytes() == want_l.tobytes()
    again = run(torch.from_numpy(w))
    assert all(a.tobytes() == b.tobytes() for a, b in zip((rf, lf, rc, lc), again))
    uni = run(None)
    exp = run(np.full(K, 1.0 / K))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(uni, exp))
    assert uni[0][3] == 0.0 and abs(uni[0][4] - 1.0) < 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# 5: the similarity bitmap and the clustering on it
# ----------------------------------------------------------------------------------------------------------------------

QS = (0, 1, 512, 1023, 1024)
WORDS = ((1, 0), (1, 1), (6, 3))


@functools.lru_cache(maxsize=None)
def fingerprints(K, Wr, Wl):
    """(K, 32 (Wr + Wl)) bool: a few families with flipped bits, then planted rows -- empty ones, identical ones, pairs with
    |A & B| / |A | B| exactly 1 / 2 (q = 512), 1023 / 1024 is out of reach of so few bits, 1 (q = 1024: identical) and just above 0"""
    rs = np.random.RandomState(70 + K + 100 * Wr + Wl)
    n = 32 * (Wr + Wl)
    fam = rs.rand(5, n) < 0.25
    F = fam[rs.randint(0, 5, size=K)] ^ (rs.rand(K, n) < 0.02)
    planted = []
    a = np.zeros(n, dtype=bool)
    a[[1, 5]] = True
    b = a.copy()
    b[[7, n - 1]] = True                                                                 # |A & B| = 2, |A | B| = 4
    c = np.zeros(n, dtype=bool)
    c[n - 1] = True                                                                      # shares one bit with b, none with a
    for row in (np.zeros(n, dtype=bool), a, b, np.zeros(n, dtype=bool), a, c, fam[0], fam[0]):
        planted.append(row)
    where = rs.permutation(K)[:len(planted)]
    for p, row in zip(where, planted):
        F[p] = row
    return F


def within_numpy(F, q):
    f = F.astype(np.int64)
    inter = f @ f.T
    pop = f.sum(axis=1)
    uni = pop[:, None] + pop[None, :] - inter
    return inter * 1024 >= q * uni


def _bit_tensors(F, Wr, Wl, device):
    words = pack(F)
    rb = torch.from_numpy(np.ascontiguousarray(words[:, :Wr]).view(np.int32).reshape(F.shape[0], Wr)).to(device)
    lb = torch.from_numpy(np.ascontiguousarray(words[:, Wr:]).view(np.int32).reshape(F.shape[0], Wl)).to(device)
    return rb, lb


def check_within(lib, device, K):
    from deeplocalproteindocking_amd import ops
    for Wr, Wl in WORDS:
        F = fingerprints(K, Wr, Wl)
        rb, lb = _bit_tensors(F, Wr, Wl, device)
        for q in QS:
            want = within_numpy(F, q)
            if _is_gpu(device):
                from guard_alloc import GuardedAllocations
                with GuardedAllocations(min_bytes=4, empty_byte=0xFF) as g:
                    mask = ops.interface_within(rb, lb, q / 1024.0, lib=lib)
                    bad = g.check(release=False)
                assert not bad, bad
            else:
                mask = ops.interface_within(rb, lb, q / 1024.0, lib=lib)
            assert tuple(mask.shape) == (K, (K + 63) // 64) and mask.dtype == torch.int64
            bits = unpack(mask, K)
            assert not bits[:, K:].any()                                                # tail bits
            assert (bits[:, :K] == want).all(), (K, Wr, Wl, q)
            assert bits[:, :K].diagonal().all() and (bits[:, :K] == bits[:, :K].T).all()
            if K >= 63 and 0 < q:
                assert want.any() and (~want).any()
            if q == 0:
                assert want.all()
        if K >= 63:
            at = within_numpy(F, 512) & ~within_numpy(F, 513)                           # pairs exactly at 1 / 2 exist
            assert at.any()
        # the clustering is the greedy reference on that bitmap
        for q in (512, 1):
            D = 1.0 - within_numpy(F, q).astype(np.float64)
            for m in (None, 3):
                cen, siz, lab = greedy64(D, 0.5, m)
                got = [t.cpu().numpy() for t in ops.interface_cluster(rb, lb, q / 1024.0, max_clusters=m, lib=lib)]
                assert got[0].dtype == np.int32 and got[0].tolist() == cen.tolist() and got[1].tolist() == siz.tolist()
                assert (got[2] == lab).all(), (K, Wr, Wl, q, m)


# ----------------------------------------------------------------------------------------------------------------------
# 6: errors
# ----------------------------------------------------------------------------------------------------------------------

def check_errors(lib, device):
    import pytest
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    c = layers_case(1, 16, 5)
    tb = tables_of(c.rec, c.rec_off, c.lig, c.lig_off, device)
    roh, loh = tb["rec_off_host"], tb["lig_off_host"]
    NLa = len(c.lig)
    bad_r, bad_l, long_l = roh.copy(), loh.copy(), loh.copy()
    bad_r[2] = bad_r[3] + 1
    bad_l[0] = -1
    long_l[-1] = NLa + 1

    def untouched(out):
        return (out[1] == FULL).all() and (out[2] == FULL).all()
    for name in ("P", "ra", "ro", "rs", "la", "lo", "ls", "roh", "loh", "rb", "lb"):
        with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
            raw_bits(lib, device, tb, c.P, **{name: None})
    for kw in (dict(K_=-1), dict(NRa_=0), dict(NLa_=0), dict(NRres_=0), dict(NLres_=0), dict(r=float("nan")), dict(r=-1.0),
               dict(ext=float("nan")), dict(roh=bad_r), dict(loh=bad_l), dict(loh=long_l)):
        with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
            raw_bits(lib, device, tb, c.P, **kw)
    for kw in (dict(K_=65537), dict(NLa_=8193), dict(NLres_=1025), dict(NRa_=65537), dict(NRres_=8193)):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            raw_bits(lib, device, tb, c.P, **kw)                                        # (refused before anything is read)
    out = raw_bits(lib, device, tb, c.P, K_=0)
    assert out[0] == 0 and untouched(out)                                               # a no-op
    out = raw_bits(lib, device, tb, c.P)
    assert out[0] == 0 and not untouched(out)
    # tables that do not belong together; tables on another kind of object
    mixed = dict(tb)
    mixed["lig_sph"] = tb["lig_sph"][:-1]
    with pytest.raises(RuntimeError, match="belong together"):
        ops.pose_interface_bits(c.P, mixed, R_CUT, lib=lib)
    with pytest.raises(RuntimeError, match="contact_tables"):
        ops.pose_interface_bits(c.P, object(), R_CUT, lib=lib)
    rb, lb = ops.pose_interface_bits(np.zeros((0, 12)), tb, R_CUT, lib=lib)
    assert tuple(rb.shape) == (0, 1) and tuple(lb.shape) == (0, 1)
    # profile and similarity through ctypes
    st = _stream(dev)
    K, NRres, NLres = 5, 16, 16
    rb, lb = (t.contiguous() for t in ops.pose_interface_bits(c.P, tb, R_CUT, lib=lib))
    w = torch.full((K,), 0.2, dtype=torch.float64, device=dev)
    rf, lf = torch.full((NRres,), -7.0, dtype=torch.float64, device=dev), torch.full((NLres,), -7.0, dtype=torch.float64, device=dev)
    rc, lc = torch.full((NRres,), -7, dtype=torch.int32, device=dev), torch.full((NLres,), -7, dtype=torch.int32, device=dev)
    nbytes = lib.call("dlpd_interface_profile_ws", K, NRres, NLres)
    assert nbytes == 32 * 12 and lib.call("dlpd_interface_profile_ws", 1025, 3, 2) == 2 * 5 * 12
    assert lib.call("dlpd_interface_profile_ws", 0, 3, 2) == 0 and lib.call("dlpd_interface_profile_ws", 65537, 3, 2) == 0
    assert lib.call("dlpd_interface_profile_ws", 5, 8193, 2) == 0 and lib.call("dlpd_interface_profile_ws", 5, 3, 1025) == 0
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device=dev)
    base = dict(rb=rb.data_ptr(), lb=lb.data_ptr(), K_=K, NR=NRres, NL=NLres, w=w.data_ptr(), rf=rf.data_ptr(), lf=lf.data_ptr(), rc=rc.data_ptr(),
                lc=lc.data_ptr(), ws=ws.data_ptr(), nb=nbytes)

    def profile(**kw):
        a = dict(base)
        a.update(kw)
        return lib.call("dlpd_interface_profile", a["rb"], a["lb"], a["K_"], a["NR"], a["NL"], a["w"], a["rf"], a["lf"], a["rc"], a["lc"], a["ws"],
                        a["nb"], st)
    for name in ("rb", "lb", "w", "rf", "lf", "rc", "lc", "ws"):
        with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
            profile(**{name: None})
    for kw in (dict(K_=-1), dict(NR=0), dict(NL=0), dict(nb=nbytes - 1)):
        with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
            profile(**kw)
    for kw in (dict(K_=65537), dict(NR=8193), dict(NL=1025)):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            profile(**kw)
    assert profile(K_=0) == 0
    _sync(dev)
    assert (rf == -7.0).all() and (lc == -7).all()
    assert profile() == 0
    _sync(dev)
    assert (rc.cpu().numpy() == unpack32(rb.cpu().numpy(), NRres).sum(axis=0)).all()
    W = 1
    mask = torch.full((K, W), -7, dtype=torch.int64, device=dev)
    cen, siz, lab = (torch.full((K,), -7, dtype=torch.int32, device=dev) for _ in range(3))
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    cws = torch.zeros(K * W, dtype=torch.int64, device=dev)
    cb = dict(rb=rb.data_ptr(), lb=lb.data_ptr(), K_=K, Wr=1, Wl=1, q=512, mask=mask.data_ptr(), m=0, cen=cen.data_ptr(), siz=siz.data_ptr(),
              lab=lab.data_ptr(), cnt=cnt.data_ptr(), ws=cws.data_ptr(), nb=K * W * 8)

    def within(**kw):
        a = dict(cb)
        a.update(kw)
        return lib.call("dlpd_interface_within", a["rb"], a["lb"], a["K_"], a["Wr"], a["Wl"], a["q"], a["mask"], st)

    def cluster(**kw):
        a = dict(cb)
        a.update(kw)
        return lib.call("dlpd_interface_cluster", a["rb"], a["lb"], a["K_"], a["Wr"], a["Wl"], a["q"], a["m"], a["cen"], a["siz"], a["lab"], a["cnt"],
                        a["ws"], a["nb"], st)
    for fn, names in ((within, ("rb", "lb", "mask")), (cluster, ("rb", "lb", "cen", "siz", "lab", "cnt", "ws"))):
        for name in names:
            with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
                fn(**{name: None})
        for kw in (dict(K_=-1), dict(q=1025), dict(q=-1), dict(Wr=-1), dict(Wr=0, Wl=0)):
            with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
                fn(**kw)
        for kw in (dict(K_=65537), dict(Wr=257), dict(Wl=33)):
            with pytest.raises(RuntimeError, match="UNSUPPORTED"):
                fn(**kw)
        assert fn(K_=0) == 0
    with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
        cluster(nb=K * W * 8 - 1)
    _sync(dev)
    assert (mask == -7).all() and (lab == -7).all() and int(cnt.item()) == -7              # nothing was written
    assert within() == 0 and cluster() == 0
    _sync(dev)
    assert 1 <= int(cnt.item()) <= K and (lab.cpu().numpy() >= 0).all()
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(RuntimeError, match="Jaccard"):
            ops.interface_cluster(rb, lb, bad, lib=lib)
    with pytest.raises(RuntimeError, match="max_clusters"):
        ops.interface_cluster(rb, lb, 0.5, max_clusters=0, lib=lib)
    with pytest.raises(RuntimeError, match="same poses"):
        ops.interface_cluster(rb, lb[:3], 0.5, lib=lib)
    with pytest.raises(RuntimeError, match="widths"):
        ops.interface_profile(rb, lb, 40, 16, lib=lib)
    with pytest.raises(RuntimeError, match="one per pose"):
        ops.interface_profile(rb, lb, 16, 16, np.ones(4), lib=lib)
    empty = ops.interface_profile(rb[:0], lb[:0], 16, 16, lib=lib)
    assert float(empty[0].abs().sum()) == 0.0 and int(empty[2].sum()) == 0
    e3 = ops.interface_cluster(rb[:0], lb[:0], 0.5, lib=lib)
    assert all(t.numel() == 0 for t in e3)


# ----------------------------------------------------------------------------------------------------------------------
# 8: 65,536 poses (the device suite)
# ----------------------------------------------------------------------------------------------------------------------

def check_large(lib, device, K=65536, sub=512):
    """K poses on a 3 x 2-residue complex: the grid limits of all three kernels, the host's answer on ``sub`` fixed positions"""
    from deeplocalproteindocking_amd import ops
    c = lattice_case(3, 2, sub, seed=4)
    hit = lattice_hits(c)
    rt, lt = hit.any(axis=2), hit.any(axis=1)
    assert measures_something(rt, lt)
    tb = tables_of(c.rec8 / 8.0, c.rec_off, c.lig8 / 8.0, c.lig_off, device)
    where = np.linspace(0, K - 1, sub).astype(np.int64)
    src = np.random.RandomState(12).randint(0, sub, size=K)
    src[where] = np.arange(sub)
    P = torch.from_numpy(c.P[src]).to(device)
    rb, lb = ops.pose_interface_bits(P, tb, R_CUT, lib=lib)
    rbn, lbn = rb.cpu().numpy().view(np.uint32), lb.cpu().numpy().view(np.uint32)
    assert rbn.shape == (K, 1) and (rbn[where] == pack(rt)).all() and (lbn[where] == pack(lt)).all()
    assert (rbn == pack(rt)[src]).all() and (lbn == pack(lt)[src]).all()                # (every pose is one of the ``sub``)
    w = 10.0 ** np.random.RandomState(13).uniform(-6.0, 6.0, size=K)
    rf, lf, rc, lc = (t.cpu().numpy() for t in ops.interface_profile(rb, lb, 3, 2, w, lib=lib))
    assert (rc == rt[src].sum(axis=0)).all() and (lc == lt[src].sum(axis=0)).all()
    assert rf.tobytes() == profile_host(rt[src], w).tobytes() and lf.tobytes() == profile_host(lt[src], w).tobytes()
    F = np.concatenate([np.pad(rt, ((0, 0), (0, 29))), np.pad(lt, ((0, 0), (0, 30)))], axis=1)
    mask = ops.interface_within(rb, lb, 0.5, lib=lib)
    rows = unpack(mask[torch.from_numpy(where).to(device)], sub)                        # (sub, 64 W): the rows of the subsample
    assert rows.shape == (sub, K) and (rows[:, where] == within_numpy(F, 512)).all()
    assert (rows == within_numpy(F, 512)[:, src]).all()
    del mask
    cen, siz, lab = (t.cpu().numpy() for t in ops.interface_cluster(rb, lb, 0.5, lib=lib))
    full = within_numpy(F, 512)
    assert int(siz.sum()) == K and (lab >= 0).all() and len(cen) <= 2 ** 5
    assert all(full[src[cen[lab[k]]], src[k]] for k in where) and cen[0] == 0


# ----------------------------------------------------------------------------------------------------------------------
# 7: the Docker level
# ----------------------------------------------------------------------------------------------------------------------

def _guarded(device, fn):
    if not _is_gpu(device):
        return fn()
    from guard_alloc import GuardedAllocations
    with GuardedAllocations(min_bytes=4, empty_byte=0xFF) as g:
        out = fn()
        bad = g.check(release=False)
    assert not bad, bad
    return out


def _np_bits(bits):
    return [b.cpu().numpy().view(np.uint32) for b in bits]


def _score(e):
    return float(e[4]) if np.ndim(e[0]) == 0 else float(e[2])


def mixed_list(dk, native, n=12):
    """a hand-made list in the three entry forms: ``refined_list`` and ``clustered_list`` entries round the native pose, and
    ``top_list`` entries (a rotation index, grid indices) near the native translation -> (list, the poses of the first two
    forms in the frame of a .dat file)"""
    from deeplocalproteindocking_amd.Dataset import near_native_poses, pose_entries
    P = near_native_poses(native, n, angle=8.0, shift=3.0, seed=2)
    ent = [(e[0], e[1], -0.5 * (n - k) - 0.01 * k * k, k) for k, e in enumerate(pose_entries(P, dk))]
    ent[1] = (ent[1][0], tuple(v + 40.0 for v in ent[1][1]), ent[1][2], 1)               # far away: no interface
    N = 2 * dk.box_size
    t0 = np.round(P[0, 9:] / float(dk.resolution)).astype(int)
    top = [(k % 6, int(t0[0] + k) % N, int(t0[1] - k) % N, int(t0[2]) % N, -3.0 - k) for k in range(3)]
    return ent[:4] + [e + (1,) for e in ent[4:8]] + top + ent[8:], P


def check_docker_interface(lib, device, tmp_path):
    import pytest
    from types import SimpleNamespace
    import decoy_checks as dc
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.Results import InterfaceSelection as isel
    frec, flig = dc.files(tmp_path, "I")
    native = dc.native_of(frec, flig, device)
    cx = isel.complex_reference(frec, flig).to(device)
    assert cx.contact_dist == 5.0 and cx.rec_residues == native.rec_residues and cx.lig_residues == native.lig_residues
    assert len(cx.rec_residues) == len(cx.all["rec_off_host"]) - 1 and all(len(r) == 3 for r in cx.lig_residues)
    assert dc.native_of(frec, flig, device, all_contacts=False).rec_residues is None
    NR, NL = len(cx.rec_residues), len(cx.lig_residues)
    dk = ec._docker(lib, device, False)
    lst, _ = mixed_list(dk, native)
    K = len(lst)
    keep = list(lst)
    prof = _guarded(device, lambda: dk.interface(cx, poses=lst))
    assert prof is dk.interface_profile and prof["K"] == K and lst == keep and prof["rec_residues"] == cx.rec_residues
    P = dk.dat_frame_poses(lst)
    want = ops.pose_interface_bits(P, cx, 5.0, lib=lib)
    rb, lb = _np_bits(dk.interface_bits)
    assert (rb == _np_bits(want)[0]).all() and (lb == _np_bits(want)[1]).all() and rb.shape == (K, (NR + 31) // 32)
    rt, lt = unpack32(rb, NR), unpack32(lb, NL)
    assert rt[0].any() and lt[0].any() and not rt[1].any() and not lt[1].any() and measures_something(rt, lt)
    assert (ops.unpack_bits(dk.interface_bits[0], NR).cpu().numpy() == rt).all()
    assert (prof["rec_count"] == rt.sum(axis=0)).all() and (prof["lig_count"] == lt.sum(axis=0)).all() and prof["rec_count"].dtype == np.int32
    # a native reference with all_contacts is taken in its place and gives the same bits
    dk.interface(native, poses=lst)
    assert all((a == b).all() for a, b in zip(_np_bits(dk.interface_bits), (rb, lb)))
    # the weights are the host's float64 numbers
    s = np.array([_score(e) for e in lst])
    boltz = np.exp(-(s - s.min()) / 0.7)
    rank = 1.0 / (1.0 + np.arange(K))
    given = np.random.RandomState(4).uniform(0.0, 2.0, size=K)
    for kw, w in ((dict(weights="uniform"), np.full(K, 1.0 / K)), (dict(weights="boltzmann", temperature=0.7), boltz / boltz.sum()),
                  (dict(weights="rank"), rank / rank.sum()), (dict(weights=given), given), (dict(weights=torch.from_numpy(given)), given)):
        got = dk.interface(cx, poses=lst, **kw)
        ref = [t.cpu().numpy() for t in ops.interface_profile(want[0], want[1], NR, NL, w, lib=lib)]
        assert got["rec_freq"].tobytes() == ref[0].tobytes() and got["lig_freq"].tobytes() == ref[1].tobytes()
        assert got["rec_freq"].tobytes() == profile_host(rt, w).tobytes()
    assert len(set(boltz.tolist())) == K
    with pytest.raises(Exception, match="temperature"):
        dk.interface(cx, poses=lst, weights="boltzmann")
    with pytest.raises(Exception, match="Unknown interface weights"):
        dk.interface(cx, poses=lst, weights="softmax")
    with pytest.raises(Exception, match="one number per pose"):
        dk.interface(cx, poses=lst, weights=np.ones(K + 1))
    with pytest.raises(RuntimeError, match="all_contacts=True"):
        dk.interface(dc.native_of(frec, flig, device, all_contacts=False), poses=lst)
    with pytest.raises(RuntimeError, match="at most"):
        dk.interface(cx, poses=[lst[0]] * 65537)
    # the residues, sorted, as selections of a restrained search
    prof = dk.interface(cx, poses=lst)
    for side, key, residues in (("receptor", "rec", cx.rec_residues), ("ligand", "lig", cx.lig_residues)):
        order = sorted((i for i in range(len(residues)) if prof[key + "_count"][i] > 0), key=lambda i: (-prof[key + "_freq"][i], i))
        names = ["%s:%d" % (residues[i][0], residues[i][1]) for i in order]
        assert dk.interface_residues(side) == names and dk.interface_residues(side, n=3) == names[:3] and len(names) >= 3
        cut = float(prof[key + "_freq"][order[1]])
        assert dk.interface_residues(side, min_freq=cut) == [nm for nm, i in zip(names, order) if prof[key + "_freq"][i] >= cut]
    prepared = SimpleNamespace(ureceptor=frec, uligand=flig, receptor_shift=np.zeros(3), ligand_shift=np.zeros(3))
    sel = [(r, l, 8.0) for r, l in zip(dk.interface_residues("receptor", n=2), dk.interface_residues("ligand", n=2))]
    rst = dk.restraints_from_selections(prepared, sel)
    assert len(rst) == 2 and all(np.isfinite(r.receptor_point).all() and r.dmax == 8.0 for r in rst)
    with pytest.raises(Exception, match="Unknown side"):
        dk.interface_residues("both")
    # the writer
    dk.new_log(str(tmp_path / "i.txt"))
    dk.write_interface()
    dk.cleanup()
    rows = [ln.split("\t") for ln in open(str(tmp_path / "i.txt")).read().strip().split("\n")]
    assert all(len(r) == 6 for r in rows) and [r[0] for r in rows] == sorted((r[0] for r in rows), key="RL".index)
    for tag, key, residues in (("R", "rec", cx.rec_residues), ("L", "lig", cx.lig_residues)):
        mine = [r for r in rows if r[0] == tag]
        marked = [i for i in range(len(residues)) if prof[key + "_count"][i] > 0]
        assert [(r[1], int(r[2]), r[3]) for r in mine] == [tuple(residues[i]) for i in marked]
        assert [int(r[4]) for r in mine] == prof[key + "_count"][marked].tolist()
        assert np.allclose([float(r[5]) for r in mine], prof[key + "_freq"][marked], atol=1e-6)
    # clustering by interface: the greedy reference on the integer test; the bitmaps of interface() are reused
    F = np.concatenate([np.pad(rt, ((0, 0), (0, 32 * rb.shape[1] - NR))), np.pad(lt, ((0, 0), (0, 32 * lb.shape[1] - NL)))], axis=1)
    held = dk.interface_bits
    for thr in (0.5, 0.25):
        D = 1.0 - within_numpy(F, ops.interface_q(thr)).astype(np.float64)
        cen, siz, lab = greedy64(D, 0.5)
        got = _guarded(device, lambda: dk.cluster_interface(cx, poses=lst, threshold=thr))
        assert dk.interface_bits is held and got is dk.clustered_list and lst == keep
        assert [e[3] for e in got] == cen.tolist() and [e[4] for e in got] == siz.tolist() and (dk.cluster_labels == lab).all()
        assert dk.cluster_labels.dtype == np.int32 and 1 < len(cen) < K
        for e in got:
            assert e[0].dtype == np.float64 and e[2] == _score(lst[e[3]])
        assert np.abs(dk.dat_frame_poses(got) - P[cen]).max() == 0.0
        cen2, siz2, lab2 = greedy64(D, 0.5, 2)
        kept = dk.cluster_interface(cx, poses=lst, threshold=thr, keep=2)
        assert [e[3] for e in kept] == cen2.tolist() and [e[4] for e in kept] == siz2.tolist() and (dk.cluster_labels == lab2).all()
        order = sorted(range(len(cen)), key=lambda n: -int(siz[n]))
        by_size = dk.cluster_interface(cx, poses=lst, threshold=thr, rank="size", keep=2)
        assert [e[3] for e in by_size] == [int(cen[n]) for n in order[:2]]
    fresh = dk.cluster_interface(cx, poses=list(lst), threshold=0.5)                    # another list object: computed again
    assert dk.interface_bits is not held and [e[3] for e in fresh] == greedy64(1.0 - within_numpy(F, 512).astype(np.float64), 0.5)[0].tolist()
    # ... and its output goes through the writer and evaluate as cluster's does
    dk.new_log(str(tmp_path / "c.dat"))
    dk.write_clustered_conformations()
    dk.cleanup()
    text = np.loadtxt(str(tmp_path / "c.dat")).reshape(len(fresh), 13)
    assert np.abs(text[:, :12] - dk.dat_frame_poses(fresh)).max() <= 2e-6
    ev = dk.evaluate(native, poses=dk.clustered_list)
    assert len(ev["capri"]) == len(fresh) and ev["capri"][0] == 3
    with pytest.raises(Exception, match="threshold"):
        dk.cluster_interface(cx, poses=lst)
    with pytest.raises(Exception, match="threshold"):
        dk.cluster_interface(cx, poses=lst, threshold=1.5)
    with pytest.raises(Exception, match="ranking"):
        dk.cluster_interface(cx, poses=lst, threshold=0.5, rank="cluspro")
    # the empty list
    empty = dk.interface(cx, poses=[])
    assert empty["K"] == 0 and tuple(dk.interface_bits[0].shape) == (0, (NR + 31) // 32) and not empty["rec_count"].any() and not empty["lig_freq"].any()
    assert dk.interface_residues("receptor") == []
    assert dk.cluster_interface(cx, poses=[], threshold=0.5) == [] and len(dk.cluster_labels) == 0
    dk.new_log(str(tmp_path / "e.txt"))
    dk.write_interface()
    dk.cleanup()
    assert open(str(tmp_path / "e.txt")).read() == ""


def check_random_rotation(lib, device, tmp_path):
    """a Docker that searched a randomly rotated receptor holds (randR R, randR t): the same physical poses give the same bitmaps"""
    import decoy_checks as dc
    from deeplocalproteindocking_amd.Dataset import near_native_poses, pose_entries
    from deeplocalproteindocking_amd.Results import InterfaceSelection as isel
    frec, flig = dc.files(tmp_path, "Q")
    native = dc.native_of(frec, flig, device)
    cx = isel.complex_reference(frec, flig).to(device)
    P = near_native_poses(native, 10, angle=8.0, shift=3.0, seed=3)
    dk, dr = ec._docker(lib, device, False), ec._docker(lib, device, True)
    assert np.abs(dr.randR.squeeze().double().numpy() - np.eye(3)).max() > 0.1
    a = dk.interface(cx, poses=pose_entries(P, dk))
    bits = _np_bits(dk.interface_bits)
    b = dr.interface(cx, poses=pose_entries(P, dr))
    assert all((x == y).all() for x, y in zip(bits, _np_bits(dr.interface_bits))) and bits[0].any()
    assert a["rec_freq"].tobytes() == b["rec_freq"].tobytes() and (a["lig_count"] == b["lig_count"]).all()
    ca = dk.cluster_interface(cx, poses=pose_entries(P, dk), threshold=0.5)
    cb = dr.cluster_interface(cx, poses=pose_entries(P, dr), threshold=0.5)
    assert [e[3:] for e in ca] == [e[3:] for e in cb] and (dk.cluster_labels == dr.cluster_labels).all()
    for d, name in ((dk, "a"), (dr, "b")):
        d.new_log(str(tmp_path / (name + ".dat")))
        d.write_clustered_conformations()
        d.cleanup()
    assert np.abs(np.loadtxt(str(tmp_path / "a.dat")) - np.loadtxt(str(tmp_path / "b.dat"))).max() <= 2e-6


def check_dock_pair(lib, device, tmp_path):
    """the script's --interface and --cluster-interface steps on a search of two synthetic PDB files; the .dat of that search is
    byte for byte the .dat of a run without them"""
    import os
    import sys
    from cluster_checks import RES, _random_rotations
    from synth_pdb import write_protein_like_pdb
    from test_atoms import _tiny_model
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Results import InterfaceSelection as isel
    from deeplocalproteindocking_amd.Results.DockerParser import DockerParser
    from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import dock_pair
    assert dock_pair.parse_interface("") == (10, "uniform", None) and dock_pair.parse_interface("5") == (5, "uniform", None)
    assert dock_pair.parse_interface(":rank") == (10, "rank", None) and dock_pair.parse_interface("7:boltzmann:0.5") == (7, "boltzmann", 0.5)
    assert dock_pair.parse_cluster_interface("0.5") == (0.5, None) and dock_pair.parse_cluster_interface("0.25:4") == (0.25, 4)
    import pytest
    for bad in ("3:softmax", "3:boltzmann", "3:boltzmann:-1"):
        with pytest.raises(ValueError):
            dock_pair.parse_interface(bad)
    with pytest.raises(ValueError):
        dock_pair.parse_cluster_interface("1.5")
    frec, flig = str(tmp_path / "r.pdb"), str(tmp_path / "l.pdb")
    write_protein_like_pdb(frec, 14, seed=5)
    write_protein_like_pdb(flig, 9, seed=6)
    L, K = 32, 40
    R = _random_rotations(np.random.RandomState(2), 3)

    def run(out, steps):
        dk = Docker(_tiny_model().to(device), box_size=L, resolution=RES, max_conf=K, rotations=R, device=device, lib=lib, coords_backend=CoordsBackend(lib=lib))
        with torch.no_grad():
            p = dk.prepare(frec, flig, "SE3")
            dk.new_log(out)
            dk.dockSE3(frec, flig, batch_size=2, prepared=p)
            dk.cleanup()
        top = list(dk.top_list)
        if steps:
            cx = isel.complex_reference(frec, flig).to(device)
            name = dock_pair.interface_and_write(dk, cx, out, 4, "boltzmann", 2.0)
            assert name == out[:-4] + ".interface.txt"
            rows = [ln.split("\t") for ln in open(name).read().strip().split("\n") if ln]
            prof = dk.interface_profile
            assert len(rows) == int((prof["rec_count"] > 0).sum() + (prof["lig_count"] > 0).sum()) and prof["K"] == K
            names = dock_pair.cluster_interface_and_write(dk, cx, out, 0.5, 3)
            assert names == (out[:-4] + ".iclustered.dat", out[:-4] + ".iclustered.sizes.txt")
            sizes = [int(v) for v in open(names[1]).read().split()]
            lines = [ln for ln in open(names[0]).read().split("\n") if ln.strip()]
            assert len(lines) == len(sizes) == len(dk.clustered_list) <= 3 and sizes == [e[4] for e in dk.clustered_list]
            assert all(len(ln.split("\t")) == 13 for ln in lines) and sum(sizes) == int((dk.cluster_labels >= 0).sum())
            confs = DockerParser(str(tmp_path), coords_backend=object()).parse_output(os.path.basename(names[0])[:-4])["conformations"]
            assert len(confs) == len(sizes)
            assert dk.top_list == top
        return open(out, "rb").read()
    with_steps = run(str(tmp_path / "pair.dat"), True)
    without = run(str(tmp_path / "plain.dat"), False)
    assert with_steps == without and len(with_steps.strip().split(b"\n")) == K
    assert sorted(os.listdir(str(tmp_path))) == sorted(["r.pdb", "l.pdb", "pair.dat", "plain.dat", "pair.interface.txt", "pair.iclustered.dat",
                                                        "pair.iclustered.sizes.txt"])
