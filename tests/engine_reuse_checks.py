"""A live DockingEngine against fresh ones: check bodies shared by tests/test_engine_reuse_emu.py (the emulated library, one
stream, one V, one candidate set) and tests/test_engine_reuse_gpu.py (the gfx950 build: side stream, two V buffers, two
candidate sets).

Docker keeps one engine per shape and docks every pair of a sweep on it, so only the first pair sees a fresh engine.  What a
live engine carries from one pair to the next -- the candidate filter ``top.tau``, the candidate sets and the slot parity, the
per-ligand decisions of ``_ligand_occupancy`` (maps, pencil map), the receptor / ligand copies, filter / clip / threshold,
the double-buffered V -- must leave no trace: after every pair of a SEQUENCE pushed through one engine, ``top_entries()`` and
the bits of ``score_batch(R[:2])`` equal those of a fresh engine given that pair alone.  Equality is exact (the kernels are
deterministic; a fresh-against-fresh control per sequence says so, and a failure of THAT control is non-determinism, not
reuse).  The fresh engine's distance from float64 is held by tests/test_gpu_accuracy.py / test_gpu_parity.py; bit equality
chains the live engine to that.

``poison`` makes "no trace" testable: before a pair's inputs are set every stored copy of the previous pair is NaN, and
between ``set_ligand`` and ``reset_top`` (the order of Docker.dock_volumes) every workspace, score volume and top-K buffer is
NaN / 0xFF -- whatever the pair's kernels read they must have written first, or been told not to read (the pencil map).

Every case asserts on its own inputs what it claims to exercise: which grids go by occupancy maps and by the pencil map,
that a "strong" pair published a candidate filter (so the candidate path was live) and that the weaker pair after it scores
ABOVE that filter (a stale one would empty its list), that consecutive lists differ, and that K1 really left pencils
unwritten (NaNs still in wsA after the search).  Nothing here reads the reference tree."""
import numpy as np
import torch

from oracle import docking_oracle as orc
from deeplocalproteindocking_amd.engine import DockingEngine

H, CLIP, BATCH = 4, 5.0, 2
PENCIL_BOXES = (40, 80)                                    # where K2 reads the packed receptor and can go by a pencil map


# ---------------------------------------------------------------------------------------- inputs
def rotations(n, seed):
    ang = np.random.RandomState(seed).uniform(-np.pi, np.pi, size=(n, 3))
    return torch.from_numpy(orc.euler_to_matrix(ang[:, 0], np.abs(ang[:, 1]), ang[:, 2])).float().contiguous()


def filter_weights(cin, seed, w1_scale=0.3):
    """A filter whose score is +0.05 where the correlations vanish and negative where they are large: a weak dense ligand
    leaves nothing below zero (its list is the masked zeros, no candidate filter), a strong one fills the list with
    negative scores."""
    g = torch.Generator().manual_seed(seed)
    W1, b1 = torch.randn(H, cin, generator=g) * w1_scale, -torch.randn(H, generator=g).abs() * 0.1
    W2, b2 = -torch.randn(1, H, generator=g).abs(), torch.tensor([0.05])
    return W1, b1, W2, b2


def blob(g, C, L, lo, hi, amp):
    v = torch.zeros(C, L, L, L)
    v[:, lo:hi, lo:hi, lo:hi] = torch.randn(C, hi - lo, hi - lo, hi - lo, generator=g) * amp
    return v


class Pair(object):
    """One receptor / ligand pair, its rotations and what the case claims about it.
    sparse: per grid, whether K1 goes by occupancy maps; strong: the list fills with negative scores and publishes tau;
    quiet: nothing scores below zero (no tau)."""

    def __init__(self, name, rec, recf, lig, ligf, R, sparse, strong=False, quiet=False, rec1=None, lig1=None):
        self.name, self.rec, self.recf, self.lig, self.ligf, self.R = name, rec, recf, lig, ligf, R
        self.rec1, self.lig1, self.sparse, self.strong, self.quiet = rec1, lig1, tuple(sparse), strong, quiet


class Result(object):
    def __init__(self, entries, S, tau, switches, nan_left):
        self.entries, self.S, self.tau, self.switches, self.nan_left = entries, S, tau, switches, nan_left

    @property
    def score(self):
        return self.entries[2]


def forbidden(g, L, inner=None):
    """Receptor and ligand clash densities: overlaps above ~0.6 of the box exceed 0.3 L^3, so the central translations
    are masked (zeros in V) and the others are not."""
    recf, ligf = torch.rand(L, L, L, generator=g), torch.rand(L, L, L, generator=g) * 2.0
    if inner:
        recf, ligf = embed(recf, inner), embed(ligf, inner)
    return recf, ligf


def embed(v, e):
    """Zero outside the e^3 corner box (the volumes of an embedded extent)."""
    out = torch.zeros_like(v)
    out[..., :e, :e, :e] = v[..., :e, :e, :e]
    return out


def single_resolution_pairs(L=40, C=8, seed=41, inner=None, nrot=(5, 3, 4)):
    """Pairs A (strong sparse blob), C (weak sparse blob in a corner) and B (weak, dense) of the issue's case 1 on one
    receptor shape; inner: every volume is zero outside the inner^3 corner box."""
    g = torch.Generator().manual_seed(seed)
    cut = (lambda v: embed(v, inner)) if inner else (lambda v: v)
    rec = cut(torch.randn(C, L, L, L, generator=g) * 0.1)
    recB = cut(torch.randn(C, L, L, L, generator=g) * 0.1)
    recf, ligf = forbidden(g, L, inner)
    A = Pair("A", rec, recf, blob(g, C, L, 14, 24, 1.0), ligf, rotations(nrot[0], seed + 1), (True,), strong=True)
    Cc = Pair("C", recB, recf.flip(0), blob(g, C, L, 3, 12, 0.3), ligf.flip(1), rotations(nrot[1], seed + 2), (True,))
    B = Pair("B", rec, recf, cut(torch.randn(C, L, L, L, generator=g) * 1e-3), ligf, rotations(nrot[2], seed + 3), (False,),
             quiet=True)
    return A, Cc, B


def two_resolution_pairs(L, C=8, C1=8, seed=53, nrot=3):
    """Blobs on both grids (strong); dense on both (quiet); a fine blob with a coarse ligand whose cells, dilated by one,
    cover the coarse box -- the two grids decide differently."""
    g = torch.Generator().manual_seed(seed)
    L1 = L // 2
    rec, rec1 = torch.randn(C, L, L, L, generator=g) * 0.1, torch.randn(C1, L1, L1, L1, generator=g) * 0.1
    recf, ligf = forbidden(g, L)
    a, b = (3 * L) // 8, (5 * L) // 8
    P = Pair("blobs", rec, recf, blob(g, C, L, a, b, 1.0), ligf, rotations(nrot, seed + 1), (True, True), strong=True,
             rec1=rec1, lig1=blob(g, C1, L1, a // 2, b // 2, 1.0))
    Q = Pair("dense", rec.flip(1), recf, torch.randn(C, L, L, L, generator=g) * 1e-4, ligf, rotations(nrot, seed + 2),
             (False, False), quiet=True, rec1=rec1.flip(1), lig1=torch.randn(C1, L1, L1, L1, generator=g) * 1e-4)
    M = Pair("mixed", rec.flip(2), recf.flip(0), blob(g, C, L, a + 2, b + 1, 0.1), ligf.flip(1), rotations(nrot, seed + 3),
             (True, False), rec1=rec1.flip(2), lig1=blob(g, C1, L1, 4, L1 - 6, 0.03))
    return P, Q, M


# ---------------------------------------------------------------------------------------- engine, poison, one pair
def make_engine(lib, device, cfg, filt, clip=CLIP, threshold=None):
    L = cfg["L"]
    thr = 0.3 * L ** 3 if threshold is None else threshold
    return DockingEngine(L, cfg["C"], *filt, clip=clip, threshold_clash=thr, max_conf=cfg["K"], batch=BATCH, device=device,
                         lib=lib, coarse_channels=cfg.get("C1", 0), extent=cfg.get("extent"), center=cfg.get("center"),
                         coarse_center=cfg.get("coarse_center"))


def _fill(t):
    if t is None:
        return
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.view(torch.uint8).fill_(0xFF)


def candidate_sets(eng):
    return [cs for cs in (getattr(eng, "_csets", None) or []) if cs is not None]


def poison(eng, phase):
    """phase "inputs", before set_receptor / set_ligand: every stored copy of a pair's volumes and spectra is NaN.
    phase "work", after set_ligand and before reset_top: every workspace, score volume and top-K buffer is NaN / 0xFF,
    the list and the candidate filter included (reset_top restores those two).  The candidate sets' counters are never
    touched: they are an invariant of their own (all zero after every search)."""
    if phase == "inputs":
        for g in eng.grids:
            for t in (g.lig, g.ligcl, g.ligq, g.recF, g.recP):
                _fill(t)
    elif phase == "work":
        for g in eng.grids:
            _fill(g.wsA)
            _fill(g.wsB)
        for t in [eng.V] + list(eng._Vbuf or []) + [getattr(eng, "pre", None), getattr(eng, "conv", None)]:
            _fill(t)
        top = eng.top
        for t in (top.cand_score, top.cand_idx, top.ws, top.glist, top.tau):
            _fill(t)
        for cs in candidate_sets(eng):
            _fill(cs["keys"])
    else:
        raise ValueError(phase)


def _after_search(eng):
    """The invariants a finished search leaves: nothing pending, every candidate counter back at zero.  -> per grid, whether
    the score channels of rotation slot 0 of wsA still hold NaNs (K1 left pencils unwritten) and whether its clash
    channel does."""
    assert eng._pending is None
    for cs in candidate_sets(eng):
        assert int(cs["count"].abs().sum()) == 0, cs["count"].tolist()
    left = []
    for g in eng.grids:
        A = g.wsA.view(eng.batch, g.CT, g.NZ, g.L, g.L, 2)[0]
        left.append((bool(torch.isnan(A[: g.C]).any()), bool(torch.isnan(A[g.C:]).any())))
    return left


def _tau(eng):
    return int(eng.top.tau.cpu().numpy().view(np.uint32)[0])


def _reset_top(eng):
    """reset_top restores the two things of the top-K state that outlive a pair (and that the poison overwrote): an empty
    list and no candidate filter."""
    eng.reset_top()
    assert _tau(eng) == 0 and len(eng.top_entries()[0]) == 0, (hex(_tau(eng)), len(eng.top_entries()[0]))


def _finish(eng, S, left):
    entries = eng.top_entries()
    return Result(entries, S.detach().cpu().clone(), _tau(eng), eng.switches(), left)


def run_pair(eng, p, poisoned):
    """One pair through eng, as Docker.dock_volumes drives it: receptor, ligand, reset_top, search; then the scores of the
    pair's first batch once more."""
    if poisoned:
        poison(eng, "inputs")
    eng.set_receptor(p.rec, p.recf, p.rec1)
    eng.set_ligand(p.lig, p.ligf, p.lig1)
    if poisoned:
        poison(eng, "work")
    _reset_top(eng)
    eng.search(p.R)
    left = _after_search(eng)
    S = eng.score_batch(p.R[:2].to(eng.device).contiguous())
    return _finish(eng, S, left)


def assert_same(a, b, what):
    for x, y, name in zip(a.entries, b.entries, ("rotation", "index", "score", "pick")):
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), "%s: %s differs (%d / %d entries)" % (what, name, len(x), len(y))
    assert a.tau == b.tau, "%s: tau %#x / %#x" % (what, a.tau, b.tau)
    assert a.S.shape == b.S.shape and torch.equal(a.S.view(torch.int32), b.S.view(torch.int32)), "%s: score_batch bits differ" % what


def check_claims(eng_cfg, p, r, poisoned):
    """What pair p claims about itself, on the result r of one engine."""
    K = eng_cfg["K"]
    what = "pair %s" % p.name
    assert not np.isnan(r.score).any() and not bool(torch.isnan(r.S).any()), what
    assert len(r.score) == K, (what, len(r.score))
    assert float(r.S.abs().max()) > 0, what
    sw = r.switches["k1_occupancy_maps"]
    boxes = [eng_cfg["L"]] + ([eng_cfg["L"] // 2] if eng_cfg.get("C1") else [])
    for n, (grid, Lg, sparse) in enumerate(zip(("fine", "coarse"), boxes, p.sparse)):
        pencil = sparse and Lg in PENCIL_BOXES
        assert sw[grid] is sparse and sw["k2_pencil_map"][grid] is pencil, (what, grid, sw)
        if not sparse and p.quiet:
            assert sw["ligand_cells_occupied"][grid] == 1.0, (what, grid, sw)
        if poisoned:
            # K1 really left pencils unwritten where K2 goes by the map -- and wrote everything where it does not
            assert r.nan_left[n] == (pencil, False), (what, grid, r.nan_left)
    if p.strong:
        assert 0 < r.tau < 0x80000000, (what, hex(r.tau))
        assert r.score[K - 1] < 0 and r.score[0] != r.score[K - 1], (what, r.score[0], r.score[K - 1])
    if p.quiet:
        assert r.tau == 0 and r.score[0] >= 0, (what, hex(r.tau), r.score[0])
    if not (p.strong or p.quiet):                          # a weak pair with a list of its own
        assert r.score[0] < 0 and r.score[0] != r.score[K - 1], (what, r.score[0], r.score[K - 1])


def assert_stale_tau_would_bite(strong, weak, K):
    """The weak pair's best score lies above the strong pair's K-th: under the strong pair's candidate filter K3 would emit
    nothing for the weak one."""
    assert weak.score[0] > strong.score[K - 1], (weak.score[0], strong.score[K - 1])


def lists_differ(a, b):
    return not (len(a.entries[0]) == len(b.entries[0]) and all(np.array_equal(x, y) for x, y in zip(a.entries, b.entries)))


class Fresh(object):
    """Results of fresh engines, one per distinct pair, computed once and shared by the poisoned and the plain run of a
    sequence; the fresh-against-fresh control on the pairs asked for."""

    def __init__(self, lib, device, cfg, filt, clip=CLIP, threshold=None):
        self.args, self.done = (lib, device, cfg, filt, clip, threshold), {}

    def engine(self):
        return make_engine(*self.args)

    def of(self, p, control=False):
        if p.name not in self.done:
            self.done[p.name] = run_pair(self.engine(), p, False)
            check_claims(self.args[2], p, self.done[p.name], False)
            if control:
                assert_same(run_pair(self.engine(), p, False), self.done[p.name], "NON-DETERMINISM: two fresh engines on pair %s" % p.name)
        return self.done[p.name]


def check_sequence(lib, device, cfg, filt, seq, poisons, fresh=None):
    """seq through ONE engine per entry of poisons; after every pair the live engine equals the fresh one.  The control runs
    on every distinct pair on the device and on the first pair of the sequence on the emulator (a search costs seconds there).
    -> the live engine of the last run and the fresh results."""
    fresh = fresh or Fresh(lib, device, cfg, filt)
    every = torch.device(device).type == "cuda"
    for n, p in enumerate(seq):
        fresh.of(p, control=every or n == 0)
    for a, b in zip(seq, seq[1:]):
        assert a.name == b.name or lists_differ(fresh.of(a), fresh.of(b)), "pairs %s and %s have the same list" % (a.name, b.name)
    for poisoned in poisons:
        eng = make_engine(lib, device, cfg, filt)
        for n, p in enumerate(seq):
            r = run_pair(eng, p, poisoned)
            what = "pair %s, number %d of the sequence on a live engine (%s)" % (p.name, n, "poisoned" if poisoned else "plain")
            check_claims(cfg, p, r, poisoned)
            assert_same(r, fresh.of(p), what)
    return eng, fresh


# ---------------------------------------------------------------------------------------- the cases
CASE1 = dict(L=40, C=8, K=30)


def check_case1(lib, device, poisons, short=False):
    """Box 40, 8 channels: channels-last K1 from the library's source layout, occupancy maps, packed receptor, pencil map.
    A, C, B, A with 5, 3, 4, 5 rotations (partial last batches; an odd number of batches flips the slot parity); short: A, C,
    A with two rotations each."""
    A, C, B = single_resolution_pairs(nrot=(2, 2, 2) if short else (5, 3, 4))
    seq = [A, C, A] if short else [A, C, B, A]
    filt = filter_weights(8, 7)
    eng, fresh = check_sequence(lib, device, CASE1, filt, seq, poisons)
    sw = eng.switches()
    assert sw["k1"] == "channels_last" and sw["k2_packed_receptor"]["fine"] and eng.fine.recF is None
    assert sw["k1_source_layout"]["fine"] == ("chunk_major" if lib.call("dlpd_channel_chunks_default", 40) else "channels_last")
    assert_stale_tau_would_bite(fresh.of(A), fresh.of(C), CASE1["K"])
    # the decisions of _ligand_occupancy are per ligand: the dense one after a sparse one takes neither map
    eng.set_ligand(B.lig, B.ligf)
    occ = eng.switches()["k1_occupancy_maps"]
    assert occ["fine"] is False and occ["k2_pencil_map"]["fine"] is False and occ["ligand_cells_occupied"]["fine"] == 1.0, occ


def check_two_resolutions(lib, device, L, poisons):
    cfg = dict(L=L, C=8, C1=8, K=60)
    P, Q, M = two_resolution_pairs(L)
    eng, fresh = check_sequence(lib, device, cfg, filter_weights(16, 11), [P, Q, M, P], poisons)
    packed = L // 2 in PENCIL_BOXES
    assert eng.switches()["k2_packed_receptor"] == {"fine": packed, "coarse": packed}
    occ = fresh.of(M).switches["k1_occupancy_maps"]["ligand_cells_occupied"]
    assert occ["coarse"] < DockingEngine.SPARSE_K1_MAX_FILL                # it is the DILATED cells that cover the coarse box
    assert_stale_tau_would_bite(fresh.of(P), fresh.of(M), cfg["K"])


def check_per_channel(lib, device, poisons):
    """Box 32, 3 channels: the per-channel K1 (no channels-last copy, no maps), slab orientation and quad layout per group."""
    L, C = 32, 3
    cfg = dict(L=L, C=C, K=25)
    g = torch.Generator().manual_seed(67)
    rec, rec2 = torch.randn(C, L, L, L, generator=g) * 0.1, torch.randn(C, L, L, L, generator=g) * 0.1
    recf, ligf = forbidden(g, L)
    R = rotations(5, 68)
    groups = set(zip(DockingEngine.prefers_transposed(R.numpy()).tolist(), DockingEngine.prefers_quads(R.numpy()).tolist()))
    assert len(groups) >= 2, groups
    P = Pair("P", rec, recf, torch.randn(C, L, L, L, generator=g) * 0.15, ligf, R, (False,), strong=True)
    Q = Pair("Q", rec2, recf.flip(0), blob(g, C, L, 5, 14, 0.15), ligf.flip(2), rotations(3, 69), (False,))
    eng, fresh = check_sequence(lib, device, cfg, filter_weights(C, 13, 0.5), [P, Q, P], poisons)
    sw = eng.switches()
    assert sw["k1"] == "per_channel" and sw["k1_quad_layout"] and sw["k1_slab_orientation"] and eng.fine.ligq is not None
    assert_stale_tau_would_bite(fresh.of(P), fresh.of(Q), cfg["K"])


def check_embedded_extent(lib, device, poisons):
    """DockingEngine(40, 8, ..., extent=37): 37^3 volumes in the corner of the 40^3 box, the window gather in front of the
    top-K, no candidate lists."""
    cfg = dict(L=40, C=8, K=30, extent=37, center=18.5)
    A, C, _ = single_resolution_pairs(seed=71, inner=37, nrot=(3, 3, 2))
    eng, fresh = check_sequence(lib, device, cfg, filter_weights(8, 7), [A, C], poisons)
    sw = eng.switches()
    assert sw["embedded_extent"] == 37 and sw["topk_candidate_lists"] is False and candidate_sets(eng) == []
    idx = fresh.of(A).entries[1]
    assert idx.max() < 74 ** 3                                           # indices of the (2 * 37)^3 grid


def _given_pair(L, C, seed, device):
    """Pair D of case 5: three single-volume batches.  Each volume is a blob; its fine map marks the blob's cells, and the
    volume holds NaN in every cell the map marks empty (activations nobody wrote)."""
    g = torch.Generator().manual_seed(seed)
    rec, (recf, _) = torch.randn(C, L, L, L, generator=g) * 0.1, forbidden(g, L)
    batches = []
    for lo, hi in ((8, 20), (17, 29), (3, 15)):
        v = blob(g, C, L, lo, hi, 0.6)[None]
        c0, c1 = lo // 4, (hi + 3) // 4
        occ = torch.zeros(1, (L + 3) // 4, (L + 3) // 4, (L + 3) // 4, dtype=torch.uint8)
        occ[:, c0:c1, c0:c1, c0:c1] = 1
        live = occ.bool().repeat_interleave(4, 1).repeat_interleave(4, 2).repeat_interleave(4, 3)[:, None, :L, :L, :L]
        assert bool((v[~live.expand_as(v)] == 0).all()) and 0 < int(occ.sum()) < occ.numel() // 2
        v = torch.where(live, v, torch.full_like(v, float("nan")))
        vf = torch.rand(1, L, L, L, generator=g) * 2.0
        batches.append(((v.to(device), vf.to(device), None), (occ.to(device), None)))
    return rec, recf, batches


def _run_given(eng, rec, recf, batches, poisoned):
    if poisoned:
        poison(eng, "inputs")
    eng.set_receptor(rec, recf)
    if poisoned:
        poison(eng, "work")
    _reset_top(eng)
    for n, (vols, occ) in enumerate(batches):
        eng.step(None, torch.tensor([n], dtype=torch.int32, device=eng.device), volumes=vols, occupancy=occ)
    eng.finish()
    left = _after_search(eng)
    S = eng.score_batch(None, volumes=batches[0][0], occupancy=batches[0][1])
    return _finish(eng, S, left)


def check_given_volumes(lib, device, poisons):
    """On the engine of case 1: search A; three single-volume batches of given volumes with occupancy maps (the dockE3
    path: K1 on volumes whose empty cells are unwritten, K2 by the maps' pencil words); search C."""
    A, C, _ = single_resolution_pairs(nrot=(5, 3, 2))
    filt = filter_weights(8, 7)
    fresh = Fresh(lib, device, CASE1, filt)
    rec, recf, batches = _given_pair(40, 8, 83, device)
    fD = _run_given(fresh.engine(), rec, recf, batches, False)
    K = CASE1["K"]
    assert len(fD.score) == K and not np.isnan(fD.score).any() and not bool(torch.isnan(fD.S).any())
    assert fD.score[0] < 0 and fD.score[0] != fD.score[K - 1], (fD.score[0], fD.score[K - 1])
    assert len(set(fD.entries[0].tolist())) >= 2, fD.entries[0]          # (more than one of the three batches reached the list)
    assert_same(_run_given(fresh.engine(), rec, recf, batches, False), fD, "NON-DETERMINISM: two fresh engines on pair D")
    every = torch.device(device).type == "cuda"
    for poisoned in poisons:
        eng = make_engine(lib, device, CASE1, filt)
        for p in (A, None, C):
            what = "pair %s after %s (%s)" % (p.name if p else "D", "A" if p is not A else "nothing", "poisoned" if poisoned else "plain")
            if p is None:
                r = _run_given(eng, rec, recf, batches, poisoned)
                if poisoned:                                             # single-volume batches: pencils of empty x-planes unwritten
                    assert r.nan_left[0] == (True, False), r.nan_left
                assert_same(r, fD, what)
            else:
                r = run_pair(eng, p, poisoned)
                check_claims(CASE1, p, r, poisoned)
                assert_same(r, fresh.of(p, control=every), what)
        assert lists_differ(fresh.of(A), fD) and lists_differ(fD, fresh.of(C))


def check_live_filter_change(lib, device, poisons):
    """On the engine of case 1, after A: what Docker._make_engine does to a pooled engine -- set_filter with new weights of
    the same width, clip 0.4 (it bites), half the threshold -- then pair C against a fresh engine BUILT with those values."""
    A, C, _ = single_resolution_pairs(nrot=(2, 2, 2) if torch.device(device).type != "cuda" else (5, 3, 2))
    filt, filt2 = filter_weights(8, 7), filter_weights(8, 8, 1.5)
    thr = 0.3 * 40 ** 3
    fresh = Fresh(lib, device, CASE1, filt)
    fresh2 = Fresh(lib, device, CASE1, filt2, clip=0.4, threshold=thr / 2)
    e2 = fresh2.engine()
    fC = run_pair(e2, C, False)
    check_claims(CASE1, C, fC, False)
    # the clamp at 0.4 bites and so does the threshold: the same engine with the constructor's defaults scores differently
    e2.clip = CLIP
    S_unclipped = e2.score_batch(C.R[:1].to(e2.device).contiguous()).cpu().clone()
    e2.clip, e2.threshold = 0.4, thr
    S_full_thr = e2.score_batch(C.R[:1].to(e2.device).contiguous()).cpu().clone()
    assert not torch.equal(S_unclipped, fC.S[:1]) and not torch.equal(S_full_thr, fC.S[:1])
    for poisoned in poisons:
        eng = make_engine(lib, device, CASE1, filt)
        rA = run_pair(eng, A, poisoned)
        check_claims(CASE1, A, rA, poisoned)
        assert_same(rA, fresh.of(A, control=True), "pair A on a fresh engine (%s)" % ("poisoned" if poisoned else "plain"))
        eng.finish()
        eng.set_filter(*filt2)
        eng.clip, eng.threshold = 0.4, thr / 2
        r = run_pair(eng, C, poisoned)
        check_claims(CASE1, C, r, poisoned)
        assert_same(r, fC, "pair C after A and a live filter change (%s)" % ("poisoned" if poisoned else "plain"))
    assert lists_differ(fresh.of(A), fC)


class _Filter(object):
    def __init__(self, filt):
        self.filt = filt

    def parameters_tuple(self):
        return self.filt


class _Model(object):
    clip = CLIP

    def __init__(self, filt, threshold):
        self.filter, self.threshold_clash = _Filter(filt), threshold

    def eval(self):
        return self


def check_docker(lib, device):
    """One Docker docks A, then C, at the shapes of case 1: the second call keeps the engine, its list is a fresh Docker's,
    and after release_engine() a new engine gives it again."""
    from deeplocalproteindocking_amd.Docker import Docker
    A, C, _ = single_resolution_pairs()
    R = rotations(5, 97).double().numpy()
    model = _Model(filter_weights(8, 7), 0.3 * 40 ** 3)
    new = lambda: Docker(model, box_size=40, resolution=1.25, max_conf=CASE1["K"], rotations=R, device=device, lib=lib)
    dock = lambda dk, p: list(dk.dock_volumes([p.rec[None]], [p.lig[None]], p.recf, p.ligf, batch_size=BATCH, write=False))
    dk = new()
    with torch.no_grad():
        topA = dock(dk, A)
        eng = dk.engine
        assert eng is not None and dk.path == "fused"
        topC = dock(dk, C)
        assert dk.engine is eng
        fr = new()
        wantC = dock(fr, C)
        assert fr.engine is not eng
        K = CASE1["K"]
        assert len(topA) == len(wantC) == K and topA[K - 1][4] < 0 and wantC[0][4] > topA[K - 1][4] and wantC[0][4] < 0
        assert topC == wantC and topA != topC
        dk.release_engine()
        assert dk.engine is None
        assert dock(dk, C) == wantC and dk.engine is not None and dk.engine is not eng
