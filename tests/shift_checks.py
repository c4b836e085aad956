"""Check bodies shared by tests/test_shift_emu.py (the kernel sources on the fibre emulator) and tests/test_shift_gpu.py (the
gfx950 build): the trilinear rotation with a per-pose offset of the sample position (csrc/dlpd_rotate_shift.h) -- forward,
adjoint, pose gradient, the local correlation and its adjoint --, ``shift=`` of ops.VolumeRotation, ops.local_correlate and
ops.local_correlate_rotated, ``Docker.score_poses(shift=)`` and ``Docker.minimize(translation=True)``.

The expectation is a float64 gather with the offset IN THE POSITION, p(i) = (c0 + off) + (i - c0) M: in numpy for the values
and the scatter (``corners64``), in torch for the gradients (``rotate_torch``), differentiated by AUTOGRAD through
a = p - floor(p) -- independent of the kernels' closed forms -- and itself held to a central difference (check_expectation).

Bounds (derived, none tuned).  u = 2^-24; delta, the error of the kernels' float32 sample position per axis, is

  delta = 9 u (L + max|off|)

pose_grad_checks' 8 u L (three products and three additions of magnitude <= L) with the ONE extra addition c0 + off, and the
magnitudes now reaching L + |off|.

  forward, per output voxel     |got - want| <= 16 u sum_corners w |V| + delta sum_axes S_ax
      The value is eight terms V w_x w_y w_z: 1 - a, two products of weights, the product with V and at most seven additions
      -- 13 roundings of quantities bounded by sum w |V|; 16 covers them and the second order.  The value is trilinear in the
      fractions: its slope along an axis is a convex combination of the four corner differences V1 - V0 of that axis, at
      most S_ax = sum of the four |V1 - V0|.  It is CONTINUOUS across cell faces, so a float32 position that falls into the
      neighbouring cell adds no jump (no flip term); for a sample within delta of a face S_ax is the largest over the cells
      on both sides.
  adjoint                       rotate_grad_checks' bounds unchanged: 2 (K + 1) u sum|w g| + 1e-4 max|want| against the float64
      scatter; the transpose identity with (148 + 6 (L + max|off|)) u <Rot |v|, |g|> (one ulp of a coordinate that now
      reaches L + |off|).
  pose gradient                 gR[j][a]: pose_grad_checks.bound64's expression, (C + 16) u A + 2 delta B + flip [+ g_err], with
      this delta.  goff[a]: the same expression with |i_j - c0| replaced by 1 (goff is the same sum without that factor).
      Condition on the inputs, unchanged: fewer than 1 in 1,000 samples within delta of a cell face (check_face_fractions
      holds the chosen seeds to it at every shape of both suites, on the CPU).
  ops                           the kernel receives M and off as float32 tensors computed in plain torch; the float64
      expectation is evaluated AT those values and carried back to R and shift by the (linear) float64 chain, the bound with
      it; the float32 chain's own rounding is a dot product of three terms: 4 u sum|terms|.
  Docker.score_poses(shift=)    against float64: the ligand resampled in float64 at the displaced positions, correlated with
      the receptor at T by slices, summed by the filter.  Per resolution and channel the kernel's sample error (the forward
      bound above) enters through sum_x |rec(x + T)| bound(x); the correlation itself is a float32 sum whose longest chain
      of additions is L (a thread's column) + 6 (lanes) + 3 (waves) + L (slabs, at most) + the product: (2 L + 16) u
      sum|terms|; the filter of the planted model adds the channels: (C + 2) u sum|corr|.
"""
import functools
import itertools

import numpy as np
import torch

import local_grad_checks as lg
import pose_grad_checks as pg
import rotate_grad_checks as rg

EPS = pg.EPS
TOL = lg.TOL
OFF_MAX = 3.7                                                            # offsets: uniform in +-3.7 voxels per axis
S_STAR = np.array([0.37, -0.41, 0.22])                                   # the planted fraction (fine-grid voxels)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(dev):
    return lg._stream(dev)


def offsets(B, seed=0):
    return np.random.RandomState(4300 + seed).uniform(-OFF_MAX, OFF_MAX, size=(B, 3)).astype(np.float32)


def delta(L, off):
    return 9 * EPS * (L + float(np.abs(np.asarray(off, dtype=np.float64)).max()))


# ----------------------------------------------------------------------------------------------------------------------
# float64: positions, corners, gather, scatter, the differentiable gather
# ----------------------------------------------------------------------------------------------------------------------

def _geometry(M, off, c0, L):
    ar = np.arange(L, dtype=np.float64) - c0
    d = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), axis=-1).reshape(-1, 3)
    return d, (c0 + np.asarray(off, dtype=np.float64).reshape(1, 3)) + d @ np.asarray(M, dtype=np.float64).reshape(3, 3)


def corners64(M, off, c0, L):
    """rotate_grad_checks.corners64 with the offset in the position: flat source index, weight, in-box (8, L^3)."""
    _, p = _geometry(M, off, c0, L)
    f = np.floor(p)
    a = p - f
    i0 = f.astype(np.int64)
    idx, w, ok = [], [], []
    for o in itertools.product((0, 1), repeat=3):
        o = np.array(o)
        c = i0 + o
        ok.append(((c >= 0) & (c < L)).all(axis=1))
        w.append(np.where(o == 1, a, 1.0 - a).prod(axis=1))
        c = np.clip(c, 0, L - 1)
        idx.append((c[:, 0] * L + c[:, 1]) * L + c[:, 2])
    return np.stack(idx), np.stack(w), np.stack(ok)


def rotate64(v, M, off, c0):
    C, L = v.shape[0], v.shape[-1]
    idx, w, ok = corners64(M, off, c0, L)
    flat = v.reshape(C, -1)
    return sum(flat[:, idx[k]] * (w[k] * ok[k])[None, :] for k in range(8)).reshape(v.shape)


def scatter64(g, M, off, c0):
    """-> (adjoint (C, L, L, L), the sum of |terms|, terms per element (L, L, L))."""
    C, L = g.shape[0], g.shape[-1]
    idx, w, ok = corners64(M, off, c0, L)
    sel = ok & (w != 0)
    cnt = np.bincount(idx[sel], minlength=L ** 3)
    out, mag = np.zeros((C, L ** 3)), np.zeros((C, L ** 3))
    for c in range(C):
        t = w * g[c].reshape(1, -1)
        out[c] = np.bincount(idx[sel], weights=t[sel], minlength=L ** 3)
        mag[c] = np.bincount(idx[sel], weights=np.abs(t[sel]), minlength=L ** 3)
    return out.reshape(g.shape), mag.reshape(g.shape), cnt.reshape(L, L, L)


def rotate_torch(vol, M, off, c0):
    """rotate_grad_checks.rotate_torch with the offset: vol (C, L, L, L), M (P, 3, 3), off (P, 3) -> (P, C, L, L, L),
    differentiable in all three."""
    C, L = vol.shape[0], vol.shape[-1]
    ar = torch.arange(L, dtype=vol.dtype, device=vol.device) - c0
    d = torch.stack(torch.meshgrid(ar, ar, ar, indexing="ij"), dim=-1).reshape(-1, 3)
    p = (c0 + off[:, None, :]) + d @ M                                   # (P, L^3, 3)
    f = torch.floor(p)
    a, i0 = p - f, f.long()
    flat = vol.reshape(C, -1)
    out = 0
    for o in itertools.product((0, 1), repeat=3):
        o = torch.tensor(o, device=vol.device)
        c = i0 + o
        ok = ((c >= 0) & (c < L)).all(dim=-1)
        w = torch.where(o == 1, a, 1.0 - a).prod(dim=-1) * ok
        c = c.clamp(0, L - 1)
        out = out + flat[:, (c[..., 0] * L + c[..., 1]) * L + c[..., 2]] * w[None]
    return out.permute(1, 0, 2).reshape(M.shape[0], C, L, L, L)


def expect64(g, v, M, off, c0):
    """d/dM (3, 3) and d/doff (3,) of sum(g * rotate(v, M, off)) by autograd: element [j][a] is the kernel's gR[3j + a]."""
    Mt = torch.tensor(np.asarray(M, dtype=np.float64).reshape(1, 3, 3), requires_grad=True)
    ot = torch.tensor(np.asarray(off, dtype=np.float64).reshape(1, 3), requires_grad=True)
    out = rotate_torch(torch.from_numpy(np.ascontiguousarray(v)), Mt, ot, float(c0))[0]
    gM, go = torch.autograd.grad((out * torch.from_numpy(np.ascontiguousarray(g))).sum(), (Mt, ot))
    return gM[0].numpy(), go[0].numpy()


def _near_faces(d, p, off, dl):
    """(n, 3) bool: the float64 position is within dl of an integer along that axis (the pivot's own voxel with no offset
    sits ON an integer in either precision and cannot flip: pose_grad_checks.bound64)."""
    near = np.abs(p - np.rint(p)) <= dl
    if not np.asarray(off).any():
        near &= (np.abs(d).sum(axis=1) > 0)[:, None]
    return near


def face_fraction(M, off, c0, L):
    d, p = _geometry(M, off, c0, L)
    return float(_near_faces(d, p, off, delta(L, off)).any(axis=1).mean())


def forward_bound(v, M, off, c0):
    """-> (bound (C, L, L, L), sum_corners w |V|) of the module docstring."""
    C, L = v.shape[0], v.shape[-1]
    d, p = _geometry(M, off, c0, L)
    f = np.floor(p)
    a, i0 = p - f, f.astype(np.int64)
    slope = pg._axis_derivs(pg._corner_table(v, i0), a)[2].sum(axis=0)   # (C, n): sum over the axes of the four |V1 - V0|
    dl = delta(L, off)
    near = np.abs(p - np.rint(p)) <= dl
    sel = np.nonzero(near.any(axis=1))[0]
    if len(sel):
        q = np.rint(p[sel]).astype(np.int64)
        for e in itertools.product((-1, 0, 1), repeat=3):                # the cells on both sides of every near face
            if not any(e):
                continue
            cell = i0[sel] + np.array(e)
            ok = np.ones(len(sel), dtype=bool)
            for k in range(3):
                if e[k]:
                    ok &= near[sel, k] & ((cell[:, k] == q[:, k]) | (cell[:, k] == q[:, k] - 1))
            if ok.any():
                s2 = pg._axis_derivs(pg._corner_table(v, cell[ok]), a[sel][ok])[2].sum(axis=0)
                slope[:, sel[ok]] = np.maximum(slope[:, sel[ok]], s2)
    mag = rotate64(np.abs(v), M, off, c0)
    return 16 * EPS * mag + dl * slope.reshape(v.shape), mag


def bound64(g, v, M, off, c0, g_err=None):
    """pose_grad_checks.bound64 with the offset in the position and this module's delta.
    -> (bound of gR (3, 3), bound of goff (3,), A of gR, A of goff, fraction of samples within delta of a cell face)."""
    C, L = v.shape[0], v.shape[-1]
    d, p = _geometry(M, off, c0, L)
    f = np.floor(p)
    a, i0 = p - f, f.astype(np.int64)
    D, Dw, D4 = pg._axis_derivs(pg._corner_table(v, i0), a)
    ga, e = np.abs(g).reshape(C, -1), np.abs(d)
    sA, sB = (ga[None] * Dw).sum(axis=1), (ga[None] * D4).sum(axis=1)    # (3, n): per axis a, summed over the channels
    A_R, B_R, A_O, B_O = e.T @ sA.T, e.T @ sB.T, sA.sum(axis=1), sB.sum(axis=1)
    dl = delta(L, off)
    near = _near_faces(d, p, off, dl)
    flagged = np.nonzero(near.any(axis=1))[0]
    flipR, flipO = np.zeros((3, 3)), np.zeros(3)
    for k in range(3):
        sel = flagged[near[flagged, k]]
        if len(sel) == 0:
            continue
        q = np.rint(p[sel, k]).astype(np.int64)
        side = []
        for cell, frac in ((q, 0.0), (q - 1, 1.0)):                      # the cell on the right of the face, and on the left
            ic, ac = i0[sel].copy(), a[sel].copy()
            ic[:, k], ac[:, k] = cell, frac
            side.append(pg._axis_derivs(pg._corner_table(v, ic), ac)[0][k])
        jump = (ga[:, sel] * np.abs(side[0] - side[1])).sum(axis=0)
        flipR[:, k] += e[sel].T @ jump
        flipO[k] += jump.sum()
    bR = (C + 16) * EPS * A_R + 2 * dl * B_R + flipR
    bO = (C + 16) * EPS * A_O + 2 * dl * B_O + flipO
    if g_err is not None:
        sE = (np.abs(g_err).reshape(C, -1)[None] * np.abs(D)).sum(axis=1)
        bR, bO = bR + e.T @ sE.T, bO + sE.sum(axis=1)
    return bR, bO, A_R, A_O, len(flagged) / float(L ** 3)


def check_expectation(L=9, C=2, h=1e-6):
    """The autograd expectation against a central difference of rotate64, in M and in off (CPU, float64).  Tolerance as
    pose_grad_checks.check_expectation derives it (1e-7 of sum |g| |corner values|); no sample may lie within 2 h L of a cell
    face (asserted), where the difference would straddle a kink."""
    g_ = torch.Generator().manual_seed(93)
    g, v = torch.randn(C, L, L, L, generator=g_, dtype=torch.float64).numpy(), torch.randn(C, L, L, L, generator=g_, dtype=torch.float64).numpy()
    M, off, c0 = lg.rots(1, seed=12)[0].astype(np.float64), offsets(1, seed=5)[0].astype(np.float64), L / 2.0
    _, p = _geometry(M, off, c0, L)
    assert (np.abs(p - np.rint(p)) > 2 * h * L).all()
    wantM, wantO = expect64(g, v, M, off, c0)
    scale = float((np.abs(g) * rotate64(np.abs(v), M, off, c0)).sum())

    def f(Mx, ox):
        return (g * rotate64(v, Mx, ox, c0)).sum()
    for j in range(3):
        E = np.zeros(3)
        E[j] = h
        fd = (f(M, off + E) - f(M, off - E)) / (2 * h)
        assert abs(fd - wantO[j]) <= 1e-7 * scale, (j, fd, wantO[j], scale)
        for a in range(3):
            E = np.zeros((3, 3))
            E[j, a] = h
            fd = (f(M + E, off) - f(M - E, off)) / (2 * h)
            assert abs(fd - wantM[j, a]) <= 1e-7 * scale, (j, a, fd, wantM[j, a], scale)
    assert np.abs(wantM).max() > 1e-3 * scale and np.abs(wantO).max() > 1e-3 * scale


# ----------------------------------------------------------------------------------------------------------------------
# the entry points
# ----------------------------------------------------------------------------------------------------------------------

def rotate_shift(lib, dev, v, R, off, L, C, B, stride, c0):
    out = torch.full((B, C, L, L, L), float("nan"), dtype=torch.float32, device=dev)
    lib.call("dlpd_rotate_trilinear_shift", _ptr(v), _ptr(R), _ptr(off), _ptr(out), B, C, L, stride, c0, _stream(dev))
    return out


def adjoint_shift(lib, dev, g, R, off, L, C, B, stride, c0, accumulate=0, out=None):
    if out is None:
        out = torch.full((B if stride else 1, C, L, L, L), float("nan"), dtype=torch.float32, device=dev)
    lib.call("dlpd_rotate_trilinear_shift_grad", _ptr(g), _ptr(R), _ptr(off), _ptr(out), B, C, L, stride, c0, accumulate, _stream(dev))
    return out


def pgrad(lib, dev, g, v, R, off, L, C, B, stride, c0, want=("R", "off")):
    """dlpd_rotate_trilinear_pgrad -> (gR (B, 3, 3) or None, goff (B, 3) or None); the outputs start as NaN."""
    gR = torch.full((B, 9), float("nan"), dtype=torch.float32, device=dev) if "R" in want else None
    go = torch.full((B, 3), float("nan"), dtype=torch.float32, device=dev) if "off" in want else None
    n = lib.call("dlpd_rotate_trilinear_pgrad_ws_bytes", B, L)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    lib.call("dlpd_rotate_trilinear_pgrad", _ptr(g), _ptr(v), _ptr(R), _ptr(off), _ptr(gR), _ptr(go), _ptr(ws), B, C, L, stride, c0,
             _stream(dev))
    return (None if gR is None else gR.cpu().numpy().reshape(B, 3, 3)), (None if go is None else go.cpu().numpy())


def local_corr(lib, dev, rec, lig, R, off, T, r, scale, mode, shared, entry):
    """dlpd_local_correlate (entry "plain") or dlpd_local_correlate_shift; corr starts as NaN."""
    P, C, L, W = T.shape[0], rec.shape[-4], rec.shape[-1], 2 * r + 1
    out = torch.full((P, C, W, W, W), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.call("dlpd_local_ws_bytes", P, C, L, r), dtype=torch.uint8, device=dev)
    st = 0 if shared else C * L ** 3
    tail = (_ptr(T), _ptr(out), _ptr(ws), P, C, L, r, scale, lg.MODES[mode], float(L) / 2.0, st, st, _stream(dev))
    if entry == "plain":
        lib.call("dlpd_local_correlate", _ptr(rec), _ptr(lig), _ptr(R), *tail)
    else:
        lib.call("dlpd_local_correlate_shift", _ptr(rec), _ptr(lig), _ptr(R), _ptr(off), *tail)
    return out.cpu().numpy()


def local_grec(lib, dev, rec, lig, R, off, T, g, r, scale, mode, shared, entry):
    P, C, L = T.shape[0], rec.shape[-4], rec.shape[-1]
    out = torch.full(tuple(rec.shape), float("nan"), dtype=torch.float32, device=dev)
    st = 0 if shared else C * L ** 3
    tail = (_ptr(T), _ptr(g), _ptr(out), None, P, C, L, r, scale, lg.MODES[mode], float(L) / 2.0, st, st, _stream(dev))
    if entry == "plain":
        lib.call("dlpd_local_correlate_grad", _ptr(rec), _ptr(lig), _ptr(R), *tail)
    else:
        lib.call("dlpd_local_correlate_shift_grad", _ptr(rec), _ptr(lig), _ptr(R), _ptr(off), *tail)
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(L, C, B, seed=0):
    g_ = torch.Generator().manual_seed(8000 * L + 10 * C + B + seed)
    g = torch.randn(B, C, L, L, L, generator=g_)
    v = torch.randn(B, C, L, L, L, generator=g_)
    R = torch.from_numpy(lg.rots(B, seed=seed + L + 7)).float().contiguous()
    off = torch.from_numpy(offsets(B, seed=seed + L)).contiguous()
    return g, v, R, off, float(L) / 2.0


def check_face_fractions(shapes):
    """The chosen seeds keep the float64 reference under the cap -- fewer than 1 in 1,000 samples within delta of a cell face
    -- at every shape (CPU only: the positions, no volume)."""
    for L, C, B in shapes:
        _, _, R, off, c0 = case(L, C, B)
        for b in range(B):
            frac = face_fraction(R[b].numpy(), off[b].numpy(), c0, L)
            print("L=%d b=%d: %.3g of the samples within delta = %.3g of a face" % (L, b, frac, delta(L, off[b].numpy())))
            assert frac < 1e-3, (L, b, frac)


# ----------------------------------------------------------------------------------------------------------------------
# 1: off = 0 (and off = NULL) is the plain call, bit for bit
# ----------------------------------------------------------------------------------------------------------------------

def check_zero_offset(lib, device, L, C, B, r=1):
    dev = torch.device(device)
    g, v, R, _, c0 = case(L, C, B)
    d_g, d_v, d_R = g.to(dev).contiguous(), v.to(dev).contiguous(), R.to(dev).contiguous()
    zero = torch.zeros(B, 3, device=dev)
    for stride in (0, C * L ** 3):
        fwd = rg.rotate(lib, dev, d_v, d_R, L, C, B, stride, c0).cpu().numpy()
        adj = rg.adjoint(lib, dev, d_g, d_R, L, C, B, stride, c0).cpu().numpy()
        nine = pg.rgrad(lib, dev, d_g, d_v, d_R, L, C, B, stride, c0)
        assert np.abs(fwd).max() > 0 and np.abs(adj).max() > 0 and np.abs(nine).max() > 0
        for o in (zero, None):
            assert rotate_shift(lib, dev, d_v, d_R, o, L, C, B, stride, c0).cpu().numpy().tobytes() == fwd.tobytes()
            assert adjoint_shift(lib, dev, d_g, d_R, o, L, C, B, stride, c0).cpu().numpy().tobytes() == adj.tobytes()
            gR, go = pgrad(lib, dev, d_g, d_v, d_R, o, L, C, B, stride, c0)
            assert gR.tobytes() == nine.tobytes() and np.isfinite(go).all() and np.abs(go).max() > 0
    P = 4
    for shared in (True, False):
        rec, lig, T, Rp, gout = [t.to(dev).contiguous() for t in pg._correlate_inputs(dev, L, C, P, r, 1, "floor", shared)]
        zero = torch.zeros(P, 3, device=dev)
        corr = local_corr(lib, dev, rec, lig, Rp, None, T, r, 1, "floor", shared, "plain")
        grec = local_grec(lib, dev, rec, lig, Rp, None, T, gout, r, 1, "floor", shared, "plain")
        assert np.abs(corr).max() > 0 and np.abs(grec).max() > 0
        for o in (zero, None):
            assert local_corr(lib, dev, rec, lig, Rp, o, T, r, 1, "floor", shared, "shift").tobytes() == corr.tobytes()
            assert local_grec(lib, dev, rec, lig, Rp, o, T, gout, r, 1, "floor", shared, "shift").tobytes() == grec.tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# 2: exact cases
# ----------------------------------------------------------------------------------------------------------------------

def check_signed_permutations(lib, device, L, C=2):
    """The 24 signed permutations about L / 2 with integer offsets in +-3: every sample position is an exact integer q.  The
    forward is V(q), zeros where q leaves the box; the adjoint scatters g(i) to q(i), one term per element; the derivative
    along a is the forward difference V(q + e_a) - V(q) of the volume continued by zeros (pose_grad_checks'
    check_signed_permutations: no position error, no flip, the bound is its first term alone)."""
    from accuracy_checks import signed_permutations
    dev = torch.device(device)
    perms = signed_permutations()
    B = len(perms)
    g_ = torch.Generator().manual_seed(L + 1)
    g, v = torch.randn(B, C, L, L, L, generator=g_), torch.randn(C, L, L, L, generator=g_)
    offs = np.random.RandomState(L).randint(-3, 4, size=(B, 3)).astype(np.float32)
    assert (offs != 0).any(axis=1).sum() >= B - 2 and np.abs(offs).max() == 3
    R, off = torch.from_numpy(perms).float().contiguous(), torch.from_numpy(offs)
    c0 = float(L) / 2.0
    d_g, d_v, d_R, d_o = g.to(dev), v.to(dev), R.to(dev), off.to(dev)
    fwd = rotate_shift(lib, dev, d_v, d_R, d_o, L, C, B, 0, c0).cpu().numpy()
    adj = adjoint_shift(lib, dev, d_g, d_R, d_o, L, C, B, C * L ** 3, c0).cpu().numpy()
    gR, go = pgrad(lib, dev, d_g, d_v, d_R, d_o, L, C, B, 0, c0)
    pad = np.zeros((C, L + 10, L + 10, L + 10))
    pad[:, 4:L + 4, 4:L + 4, 4:L + 4] = v.numpy().astype(np.float64)                    # pad[q + 4] = V(q), -4 <= q <= L + 5
    outside = 0
    for b in range(B):
        d, p = _geometry(perms[b], offs[b], c0, L)
        q = np.rint(p).astype(np.int64)
        assert (p == q).all() and q.min() >= -4 and q.max() <= L + 3
        inside = ((q >= 0) & (q < L)).all(axis=1)
        outside += int((~inside).sum())
        V0 = pad[:, q[:, 0] + 4, q[:, 1] + 4, q[:, 2] + 4]
        assert np.array_equal(fwd[b].reshape(C, -1), V0.astype(np.float32)), b                   # exactly, zeros outside
        want = np.zeros((C, L ** 3), dtype=np.float32)
        flat = (q[inside, 0] * L + q[inside, 1]) * L + q[inside, 2]
        assert len(np.unique(flat)) == len(flat)
        want[:, flat] = g[b].numpy().reshape(C, -1)[:, inside]
        assert np.array_equal(adj[b].reshape(C, -1), want), b                                    # the inverse scatter, exactly
        gb = g[b].numpy().astype(np.float64).reshape(C, -1)
        wR, AR, wO, AO = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3), np.zeros(3)
        for a in range(3):
            qa = q.copy()
            qa[:, a] += 1
            Da = pad[:, qa[:, 0] + 4, qa[:, 1] + 4, qa[:, 2] + 4] - V0
            s, sa = (gb * Da).sum(axis=0), (np.abs(gb) * np.abs(Da)).sum(axis=0)
            wR[:, a], AR[:, a], wO[a], AO[a] = d.T @ s, np.abs(d).T @ sa, s.sum(), sa.sum()
        assert (np.abs(gR[b] - wR) <= (C + 16) * EPS * AR).all(), (b, gR[b], wR)
        assert (np.abs(go[b] - wO) <= (C + 16) * EPS * AO).all(), (b, go[b], wO)
        assert (np.abs(wO) > 1e-5 * AO).any()
    assert outside > 0


def check_offset_of_a_whole_box(lib, device, L, C=2):
    """An offset of L along one axis under signed permutations (positions i or L - i, both >= 0, plus L): every sample leaves
    the box: the forward is all zeros and so is the volume's gradient."""
    from accuracy_checks import signed_permutations
    dev = torch.device(device)
    perms = signed_permutations()[:6]
    B = len(perms)
    g_ = torch.Generator().manual_seed(L + 2)
    g, v = torch.randn(B, C, L, L, L, generator=g_).to(dev), torch.randn(C, L, L, L, generator=g_).to(dev)
    R = torch.from_numpy(perms).float().contiguous().to(dev)
    off = torch.zeros(B, 3)
    for b in range(B):
        off[b, b % 3] = L
    off = off.to(dev)
    c0 = float(L) / 2.0
    fwd = rotate_shift(lib, dev, v, R, off, L, C, B, 0, c0).cpu().numpy()
    assert (fwd == 0).all()
    for stride in (0, C * L ** 3):
        assert (adjoint_shift(lib, dev, g, R, off, L, C, B, stride, c0).cpu().numpy() == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 3, 4: forward and adjoint against float64, the transpose identity, accumulate
# ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def forward_reference(L, C, B, b, vb, seed=0):
    _, v, R, off, c0 = case(L, C, B, seed)
    v64, M, o = v[vb].numpy().astype(np.float64), R[b].numpy().astype(np.float64), off[b].numpy().astype(np.float64)
    want = rotate64(v64, M, o, c0)
    bound, mag = forward_bound(v64, M, o, c0)
    for t in (want, bound, mag):
        t.setflags(write=False)
    return want, bound, mag


def check_forward(lib, device, L, C, B, seed=0):
    dev = torch.device(device)
    _, v, R, off, c0 = case(L, C, B, seed)
    d_v, d_R, d_o = v.to(dev).contiguous(), R.to(dev).contiguous(), off.to(dev).contiguous()
    for shared in (True, False):
        stride = 0 if shared else C * L ** 3
        got = rotate_shift(lib, dev, d_v, d_R, d_o, L, C, B, stride, c0).cpu().numpy()
        assert got.tobytes() == rotate_shift(lib, dev, d_v, d_R, d_o, L, C, B, stride, c0).cpu().numpy().tobytes()
        assert np.isfinite(got).all(), "every element is written"
        for b in range(B):
            want, bound, mag = forward_reference(L, C, B, b, 0 if shared else b, seed)
            err = np.abs(got[b] - want)
            print("rotate_trilinear_shift L=%d C=%d b=%d%s: worst error %.3g of the bound, %.3g of sum w|V|; non-zero %.2f" %
                  (L, C, b, ", shared volume" if shared else "", float((err / np.maximum(bound, 1e-300)).max()),
                   float((err / np.maximum(mag, 1e-300)).max()), float((want != 0).mean())))
            assert (want != 0).any() and (err <= bound).all(), (b, float((err - bound).max()))


@functools.lru_cache(maxsize=None)
def adjoint_reference(L, C, B, seed=0):
    g, _, R, off, c0 = case(L, C, B, seed)
    want, mag = np.zeros((B, C, L, L, L)), np.zeros((B, C, L, L, L))
    cnt = np.zeros((B, L, L, L), dtype=np.int64)
    for b in range(B):
        want[b], mag[b], cnt[b] = scatter64(g[b].numpy().astype(np.float64), R[b].numpy(), off[b].numpy(), c0)
    for a in (want, mag, cnt):
        a.setflags(write=False)
    return want, mag, cnt


def check_adjoint(lib, device, L, C, B, summed, seed=0):
    """rotate_grad_checks.check_kernel with the offsets."""
    dev = torch.device(device)
    g, _, R, off, c0 = case(L, C, B, seed)
    want, mag, cnt = adjoint_reference(L, C, B, seed)
    d_g, d_R, d_o = g.to(dev).contiguous(), R.to(dev).contiguous(), off.to(dev).contiguous()
    stride = 0 if summed else C * L ** 3
    got = adjoint_shift(lib, dev, d_g, d_R, d_o, L, C, B, stride, c0).cpu().numpy()
    assert got.tobytes() == adjoint_shift(lib, dev, d_g, d_R, d_o, L, C, B, stride, c0).cpu().numpy().tobytes()
    assert not np.isnan(got).any(), "every element is written"
    if summed:
        w64, m64, K = want.sum(axis=0, keepdims=True), mag.sum(axis=0, keepdims=True), int(cnt.max()) * B
    else:
        w64, m64, K = want, mag, int(cnt.max())
    assert (w64 != 0).mean() > 0.05                                      # (an offset of 3.7 voxels empties a box of 5 on one side)
    bound = 2 * (K + 1) * EPS * m64 + TOL * np.abs(w64).max()
    err = np.abs(got - w64)
    print("rotate_trilinear_shift_grad L=%d C=%d B=%d%s: non-zero %.2f, K=%d, worst error %.3g of max|want|" %
          (L, C, B, ", summed" if summed else "", float((w64 != 0).mean()), K, err.max() / np.abs(w64).max()))
    assert (err <= bound).all(), (float((err - bound).max()), float(np.abs(w64).max()))
    # what the plain adjoint would give is NOT this: the offsets are seen (they move a source voxel's candidates by > 1)
    plain = rg.adjoint(lib, dev, d_g, d_R, L, C, B, stride, c0).cpu().numpy()
    assert (np.abs(plain - w64) > bound).any()


def check_transpose(lib, device, L, C, B, summed, seed=0):
    """<shift_rotate(v), g> = <v, shift_grad(g)>, the forward KERNEL on the other side (rotate_grad_checks.check_transpose)."""
    dev = torch.device(device)
    g, v, R, off, c0 = case(L, C, B, seed)
    if summed:
        v = v[:1]
    d_g, d_v, d_R, d_o = g.to(dev).contiguous(), v.to(dev).contiguous(), R.to(dev).contiguous(), off.to(dev).contiguous()
    stride = 0 if summed else C * L ** 3
    rot = rotate_shift(lib, dev, d_v, d_R, d_o, L, C, B, stride, c0).cpu().double()
    rot_abs = rotate_shift(lib, dev, d_v.abs().contiguous(), d_R, d_o, L, C, B, stride, c0).cpu().double()
    adj = adjoint_shift(lib, dev, d_g, d_R, d_o, L, C, B, stride, c0).cpu().double()
    lhs, rhs = float((rot * g.double()).sum()), float((v.double() * adj).sum())
    bound = (148 + 6 * (L + OFF_MAX)) * EPS * float((rot_abs * g.double().abs()).sum())
    print("transpose identity with offsets L=%d C=%d B=%d%s: <Rot v, g> %.9g, <v, Adj g> %.9g, difference %.3g, bound %.3g" %
          (L, C, B, ", summed" if summed else "", lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 0 and abs(lhs - rhs) <= bound, (lhs, rhs, bound)


def check_accumulate(lib, device, L=9, C=3):
    """B = 5 in one call equals 2 + 3 with accumulate, bit for bit (the summed form), with the offsets."""
    dev = torch.device(device)
    g, _, R, off, c0 = case(L, C, 5)
    d_g, d_R, d_o = g.to(dev).contiguous(), R.to(dev).contiguous(), off.to(dev).contiguous()
    one = adjoint_shift(lib, dev, d_g, d_R, d_o, L, C, 5, 0, c0)
    two = adjoint_shift(lib, dev, d_g[:2].contiguous(), d_R[:2].contiguous(), d_o[:2].contiguous(), L, C, 2, 0, c0)
    two = adjoint_shift(lib, dev, d_g[2:].contiguous(), d_R[2:].contiguous(), d_o[2:].contiguous(), L, C, 3, 0, c0, accumulate=1, out=two)
    assert one.cpu().numpy().tobytes() == two.cpu().numpy().tobytes() and float(one.abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------------
# 5, 6, 7: the pose gradient against float64 autograd, a ramp, determinism and independence
# ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pose_reference(L, C, B, b, vb, seed=0):
    g, v, R, off, c0 = case(L, C, B, seed)
    g64, v64 = g[b].numpy().astype(np.float64), v[vb].numpy().astype(np.float64)
    M, o = R[b].numpy().astype(np.float64), off[b].numpy().astype(np.float64)
    wM, wO = expect64(g64, v64, M, o, c0)
    res = (wM, wO) + bound64(g64, v64, M, o, c0)
    for t in res[:6]:
        t.setflags(write=False)
    return res


def check_pose_gradient(lib, device, L, C, B, seed=0):
    """gR and goff against float64 autograd, one volume for all poses and one per pose; the same bytes twice; either output
    alone has the bytes it has beside the other; a pose alone has the bytes it has among the others."""
    dev = torch.device(device)
    g, v, R, off, c0 = case(L, C, B, seed)
    d_g, d_v, d_R, d_o = g.to(dev).contiguous(), v.to(dev).contiguous(), R.to(dev).contiguous(), off.to(dev).contiguous()
    for shared in (True, False):
        stride = 0 if shared else C * L ** 3
        gR, go = pgrad(lib, dev, d_g, d_v, d_R, d_o, L, C, B, stride, c0)
        again = pgrad(lib, dev, d_g, d_v, d_R, d_o, L, C, B, stride, c0)
        assert gR.tobytes() == again[0].tobytes() and go.tobytes() == again[1].tobytes(), "the same bits run to run"
        assert pgrad(lib, dev, d_g, d_v, d_R, d_o, L, C, B, stride, c0, want=("R",))[0].tobytes() == gR.tobytes()
        assert pgrad(lib, dev, d_g, d_v, d_R, d_o, L, C, B, stride, c0, want=("off",))[1].tobytes() == go.tobytes()
        for b in range(B):
            vb = 0 if shared else b
            alone = pgrad(lib, dev, d_g[b:b + 1].contiguous(), d_v[vb:vb + 1].contiguous(), d_R[b:b + 1].contiguous(),
                          d_o[b:b + 1].contiguous(), L, C, 1, stride, c0)
            assert alone[0][0].tobytes() == gR[b].tobytes() and alone[1][0].tobytes() == go[b].tobytes(), "independent of the other poses"
            wM, wO, bR, bO, AR, AO, frac = pose_reference(L, C, B, b, vb, seed)
            assert (np.abs(wM) > 1e-4 * AR).any() and (np.abs(wO) > 1e-4 * AO).any()          # (something to measure)
            label = "L=%d C=%d b=%d%s" % (L, C, b, ", shared volume" if shared else "")
            pg._compare("rotate_trilinear_pgrad gR " + label, gR[b], wM, bR, AR, frac)
            pg._compare("rotate_trilinear_pgrad goff " + label, go[b], wO, bO, AO, frac)


def check_ramp(lib, device, L, C=3):
    """vol_c = al_c x + be_c y + ga_c z + const_c, g >= 0 and zero on the samples that have a corner outside the box: the
    derivative is the constant slope on every sample that counts, goff[a] = sum_c slope[c][a] sum_i g_c(i) in closed form
    (pose_grad_checks.check_ramp's argument; gR[j][a] with the factor (i_j - c0)).  Pose 0 is a PURE offset (the identity
    map), pose 1 a rotation with an offset."""
    dev = torch.device(device)
    B = 2
    g_ = torch.Generator().manual_seed(79 + L)
    slope = torch.randn(C, 3, generator=g_, dtype=torch.float64).numpy()
    const = torch.randn(C, generator=g_, dtype=torch.float64).numpy()
    ar = np.arange(L, dtype=np.float64)
    X, Y, Z = np.meshgrid(ar, ar, ar, indexing="ij")
    v64 = (slope[:, 0, None, None, None] * X + slope[:, 1, None, None, None] * Y + slope[:, 2, None, None, None] * Z +
           const[:, None, None, None])
    v = torch.from_numpy(v64).float()
    Rn = np.stack([np.eye(3), lg.rots(1, seed=L + 6)[0]])
    R = torch.from_numpy(Rn).float().contiguous()
    offs = np.array([[0.37, -1.41, 0.72], [-0.6, 0.3, 1.2]], dtype=np.float32)
    c0 = float(L) / 2.0
    g = torch.rand(B, C, L, L, L, generator=g_)
    wantR, wantO = np.zeros((B, 3, 3)), np.zeros((B, 3))
    for b in range(B):
        d, p = _geometry(R[b].numpy(), offs[b], c0, L)
        inside = ((np.floor(p) >= 0) & (np.floor(p) + 1 <= L - 1)).all(axis=1)
        assert 0.1 < inside.mean() < 1.0
        g[b] *= torch.from_numpy(inside.reshape(1, L, L, L)).float()
        s = g[b].numpy().astype(np.float64).reshape(C, -1).T @ slope                        # (n, 3): sum_c g_c slope[c][a]
        wantR[b], wantO[b] = d.T @ s, s.sum(axis=0)
    gR, go = pgrad(lib, dev, g.to(dev).contiguous(), v.to(dev).contiguous(), R.to(dev), torch.from_numpy(offs).to(dev), L, C, B, 0, c0)
    for b in range(B):
        bR, bO, AR, AO, frac = bound64(g[b].numpy().astype(np.float64), v.numpy().astype(np.float64), R[b].numpy(), offs[b], c0)
        assert (np.abs(wantO[b]) > 1e-2 * AO).any()
        pg._compare("ramp goff L=%d b=%d" % (L, b), go[b], wantO[b], bO, AO, frac)
        pg._compare("ramp gR L=%d b=%d" % (L, b), gR[b], wantR[b], bR, AR, frac)


def _run_rotated(ops, lib, d, kw, rotation_grad, with_shift=True):
    a, b, Rg, sg = d[0].clone().requires_grad_(), d[1].clone().requires_grad_(), d[3].clone().requires_grad_(), d[5].clone().requires_grad_()
    out = ops.local_correlate_rotated(a, b, d[2], Rg, rotation_grad=rotation_grad, shift=sg if with_shift else None, **kw)
    out.backward(d[4])
    return [out.detach().cpu().numpy(), a.grad.cpu().numpy(), b.grad.cpu().numpy(), None if Rg.grad is None else Rg.grad.cpu().numpy(),
            None if sg.grad is None else sg.grad.cpu().numpy()]


def _correlate_inputs(dev, L, C, P, r, scale, mode, shared, seed=0):
    rec, lig, T, R, gout = pg._correlate_inputs(dev, L, C, P, r, scale, mode, shared, seed)
    shift = torch.from_numpy(np.random.RandomState(77 + L + seed).uniform(-0.9, 0.9, size=(P, 3)).astype(np.float32))
    return rec, lig, T, R, gout, shift


def check_chunking(lib, device, monkeypatch, L=8, C=2, P=5, r=1):
    """LOCAL_WS_BYTES of one pose's volume: five chunks of one pose.  Every gradient -- receptor, ligand, R, shift -- has the
    bytes of the unsplit call (pose_grad_checks.check_chunking with the shifts)."""
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    for shared in (True, False):
        d = [t.to(dev).contiguous() for t in _correlate_inputs(dev, L, C, P, r, 1, "floor", shared)]
        kw = dict(radius=r, lib=lib)
        whole = _run_rotated(ops, lib, d, kw, True)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "LOCAL_WS_BYTES", 4 * C * L ** 3)
            split = _run_rotated(ops, lib, d, kw, True)
        assert whole[3].shape == (P, 3, 3) and whole[4].shape == (P, 3) and np.abs(whole[3]).max() > 0 and np.abs(whole[4]).max() > 0
        for k in range(5):
            assert whole[k].tobytes() == split[k].tobytes(), k


# ----------------------------------------------------------------------------------------------------------------------
# 8: ops under autograd
# ----------------------------------------------------------------------------------------------------------------------

def _chain(R64, shift64, fold):
    """The float64 chain of ops: R -> M (kernel_matrices), (M, shift) -> off = -shift M."""
    from deeplocalproteindocking_amd.Utils.Conventions import kernel_matrices
    M = kernel_matrices(R64, *fold) if fold is not None else R64
    return M, -torch.matmul(shift64.unsqueeze(1), M).squeeze(1)


def _carry(R, shift, fold, b, wM, wO, bM, bO):
    """One pose's expectation (wM, wO) and bound (bM, bO) for (gM, goff), computed AT the float32 M and off the kernel took,
    carried to (R.grad, shift.grad) through the float64 chain -- linear: gM' = gM - shift (x) goff, then kernel_matrices'
    transpose; shift.grad = -M goff -- and the bound through the same maps in absolute value, plus the float32 chain's own
    rounding, 4 u sum|terms| (dot products of three terms)."""
    R64, s64 = R[b:b + 1].double().requires_grad_(), shift[b:b + 1].double().requires_grad_()
    M, off = _chain(R64, s64, fold)
    wR, wS = torch.autograd.grad((M * torch.from_numpy(wM)).sum() + (off * torch.from_numpy(wO)).sum(), (R64, s64))
    Ma, sa = M.detach().abs()[0].numpy(), s64.detach().abs()[0].numpy()
    bMt = bM + sa[:, None] * bO[None, :] + 4 * EPS * (np.abs(wM) + sa[:, None] * np.abs(wO)[None, :])
    bS = Ma @ (bO + 4 * EPS * np.abs(wO))
    AS = Ma @ np.abs(wO)
    # kernel_matrices is a permutation of the entries times a positive scale: the bound maps as the value does
    R1 = R[b:b + 1].double().requires_grad_()
    (bR,) = torch.autograd.grad((_chain(R1, s64.detach(), fold)[0] * torch.from_numpy(bMt)).sum(), R1)
    return wR[0].numpy(), wS[0].numpy(), np.abs(bR[0].numpy()), bS, AS


def check_volume_rotation_autograd(lib, device, L=9, C=3, B=3, **conv):
    """ops.VolumeRotation(rotation_grad=True)(v, R, shift): the forward's bytes; the volume's gradient is the offset adjoint's
    bytes; R.grad and shift.grad against float64 through off = -M^T shift and kernel_matrices.  Without the flag: the same
    forward bytes, the same volume gradient, no gradient for R or shift."""
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.Utils.Conventions import kernel_matrices, rotation_scale
    dev = torch.device(device)
    g_ = torch.Generator().manual_seed(59 + L)
    vol, gout = torch.randn(B, C, L, L, L, generator=g_).to(dev), torch.randn(B, C, L, L, L, generator=g_).to(dev)
    R = torch.from_numpy(lg.rots(B, seed=L + 4)).float().contiguous().to(dev)
    shift = torch.from_numpy(np.random.RandomState(L).uniform(-2.5, 2.5, size=(B, 3)).astype(np.float32)).to(dev)
    c0 = float(L) / 2.0 if conv.get("center") is None else float(conv["center"])
    fold = (rotation_scale(conv.get("scale"), L), conv.get("axis_order", "xyz"), conv.get("transpose", False))
    M = kernel_matrices(R, *fold)
    off = ops._kernel_offset(M, shift)                                   # (what the operator hands the kernel)
    off_op, on = ops.VolumeRotation(lib=lib, **conv), ops.VolumeRotation(lib=lib, rotation_grad=True, **conv)
    plain = off_op(vol, R, shift)
    direct = rotate_shift(lib, dev, vol.contiguous(), M.contiguous(), off, L, C, B, C * L ** 3, c0)
    assert not plain.requires_grad and plain.cpu().numpy().tobytes() == direct.cpu().numpy().tobytes()
    # shift = 0 is the operator without a shift; the displaced volume is not
    assert off_op(vol, R, torch.zeros_like(shift)).cpu().numpy().tobytes() == off_op(vol, R).cpu().numpy().tobytes()
    assert float((plain - off_op(vol, R)).abs().max()) > 0
    res = {}
    for name, op in (("off", off_op), ("on", on)):
        a, Rg, sg = vol.clone().requires_grad_(), R.clone().requires_grad_(), shift.clone().requires_grad_()
        out = op(a, Rg, sg)
        assert out.requires_grad and out.detach().cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
        out.backward(gout)
        res[name] = (a.grad.cpu().numpy(), Rg.grad, sg.grad)
    gv = adjoint_shift(lib, dev, gout.contiguous(), M.contiguous(), off, L, C, B, C * L ** 3, c0).cpu().numpy()
    assert res["off"][1] is None and res["off"][2] is None
    assert res["off"][0].tobytes() == gv.tobytes() == res["on"][0].tobytes()
    gotR, gotS = res["on"][1], res["on"][2]
    assert gotR is not None and gotR.shape == R.shape and gotS is not None and gotS.shape == shift.shape and gotS.dtype == torch.float32
    gotR, gotS = gotR.cpu().numpy(), gotS.cpu().numpy()
    M64, off64 = M.cpu().double().numpy(), off.cpu().double().numpy()    # (the maps and offsets the kernel took, as float64)
    Rc, sc = R.cpu(), shift.cpu()
    for b in range(B):
        g64, v64 = gout[b].cpu().numpy().astype(np.float64), vol[b].cpu().numpy().astype(np.float64)
        wM, wO = expect64(g64, v64, M64[b], off64[b], c0)
        bM, bO, AM, AO, frac = bound64(g64, v64, M64[b], off64[b], c0)
        wR, wS, bR, bS, AS = _carry(Rc, sc, fold, b, wM, wO, bM, bO)
        label = "L=%d b=%d %s" % (L, b, conv or "")
        pg._compare("VolumeRotation(shift) R.grad " + label, gotR[b], wR, bR, np.maximum(np.abs(wR), 1e-300), frac)
        pg._compare("VolumeRotation(shift) shift.grad " + label, gotS[b], wS, bS, AS, frac)
        assert np.abs(wS).max() > 0
    # shift alone asks for a gradient; no graph under no_grad, none without the flag
    sg = shift.clone().requires_grad_()
    out = on(vol, R, sg)
    assert out.requires_grad
    out.backward(gout)
    assert sg.grad.cpu().numpy().tobytes() == res["on"][2].cpu().numpy().tobytes()
    assert not off_op(vol, R, sg).requires_grad
    with torch.no_grad():
        assert not on(vol.clone().requires_grad_(), R, sg).requires_grad
    # one (C, L, L, L) volume for all B matrices
    sg = shift.clone().requires_grad_()
    shared = on(vol[0], R, sg)
    assert shared.cpu().detach().numpy().tobytes() == rotate_shift(lib, dev, vol[0].contiguous(), M.contiguous(), off, L, C, B, 0, c0).cpu().numpy().tobytes()
    shared.backward(gout)
    assert float(sg.grad.abs().max()) > 0


def check_local_correlate_rotated(lib, device, L, C, P, r, scale, mode, shared, seed=0):
    """ops.local_correlate_rotated(..., shift=, rotation_grad=True) against the float64 model: the receptor's and the ligand's
    gradient with rotate_grad_checks' bounds, R.grad and shift.grad with bound64 and the ``g_err`` term
    (pose_grad_checks.check_local_correlate_rotated), carried through off = -shift R."""
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    W = 2 * r + 1
    rec, lig, T, R, gout, shift = _correlate_inputs(dev, L, C, P, r, scale, mode, shared, seed)
    tau = lg.coarse(T.numpy(), scale, mode)
    c0 = float(L) / 2.0
    d = [t.to(dev).contiguous() for t in (rec, lig, T, R, gout, shift)]
    kw = dict(radius=r, scale=scale, coarse=mode, lib=lib)
    off = ops._kernel_offset(d[3], d[5])
    off64 = off.cpu().double().numpy()
    plain = ops.local_correlate(d[0], d[1], d[2], R=d[3], shift=d[5], **kw)
    direct = local_corr(lib, dev, d[0], d[1], d[3], off, d[2], r, scale, mode, shared, "shift")
    assert not plain.requires_grad and plain.cpu().numpy().tobytes() == direct.tobytes()
    assert ops.local_correlate(d[0], d[1], d[2], R=d[3], shift=torch.zeros_like(d[5]), **kw).cpu().numpy().tobytes() == \
        ops.local_correlate(d[0], d[1], d[2], R=d[3], **kw).cpu().numpy().tobytes()
    on = _run_rotated(ops, lib, d, kw, True)
    no = _run_rotated(ops, lib, d, kw, False)
    assert on[0].tobytes() == plain.cpu().numpy().tobytes() == no[0].tobytes()
    assert on[1].tobytes() == no[1].tobytes() and on[2].tobytes() == no[2].tobytes() and no[3] is None and no[4] is None
    assert on[3].shape == (P, 3, 3) and on[4].shape == (P, 3)
    # the receptor's gradient of ops.local_correlate(shift=) is the same kernel call
    a = d[0].clone().requires_grad_()
    ops.local_correlate(a, d[1], d[2], R=d[3], shift=d[5], **kw).backward(d[4])
    assert a.grad.cpu().numpy().tobytes() == on[1].tobytes()
    # shift alone: the same three numbers per pose
    sg = d[5].clone().requires_grad_()
    o = ops.local_correlate_rotated(d[0], d[1], d[2], d[3], rotation_grad=True, shift=sg, **kw)
    assert o.requires_grad
    o.backward(d[4])
    assert sg.grad.cpu().numpy().tobytes() == on[4].tobytes()
    with torch.no_grad():
        assert not ops.local_correlate_rotated(d[0], d[1], d[2], d[3], rotation_grad=True, shift=sg, **kw).requires_grad
    want = {k: np.zeros((P, C, L, L, L)) for k in ("rec", "lig", "mrec", "mlig")}
    Krot, measured = 0, 0
    for p in range(P):
        vsel = () if shared else (p,)
        l64, M = lig[vsel].numpy().astype(np.float64), R[p].numpy().astype(np.float64)
        lrot = rotate64(l64, M, off64[p], c0)
        want["rec"][p], G, want["mrec"][p], mG = lg.adjoint64(rec[vsel].numpy().astype(np.float64), lrot, gout[p].numpy().astype(np.float64),
                                                               tau[p], r)
        want["lig"][p], _, cnt = scatter64(G, M, off64[p], c0)
        idx, w, ok = corners64(M, off64[p], c0, L)
        for c in range(C):
            want["mlig"][p, c] = np.bincount(idx[ok], weights=(np.abs(w) * mG[c].reshape(1, -1))[ok], minlength=L ** 3).reshape(L, L, L)
        Krot = max(Krot, int(cnt.max()))
        if not G.any():
            assert (on[3][p] == 0).all() and (on[4][p] == 0).all(), p    # (no overlap anywhere in the window: exactly zero)
            continue
        wM, wO = expect64(G, l64, M, off64[p], c0)
        bM, bO, AM, AO, frac = bound64(G, l64, M, off64[p], c0, g_err=2 * (W ** 3 + 1) * EPS * mG)
        wR, wS, bR, bS, AS = _carry(R, shift, None, p, wM, wO, bM, bO)
        measured += int((np.abs(wS) > 1e-4 * AS).any())
        label = "L=%d r=%d scale %d %s%s pose %d" % (L, r, scale, mode, ", shared" if shared else "", p)
        pg._compare("local_correlate_rotated(shift) R.grad " + label, on[3][p], wR, bR, np.maximum(np.abs(wR), 1e-300), frac)
        pg._compare("local_correlate_rotated(shift) shift.grad " + label, on[4][p], wS, bS, AS, frac)
    assert measured >= 2
    for k, got, K in (("rec", on[1], W ** 3), ("lig", on[2], Krot * W ** 3)):
        w64, mag = (want[k].sum(axis=0), want["m" + k].sum(axis=0)) if shared else (want[k], want["m" + k])
        K = K * (P if shared else 1)
        assert got.shape == w64.shape and np.abs(w64).max() > 0
        err = np.abs(got - w64)
        bound = 2 * (K + 1) * EPS * mag + TOL * np.abs(w64).max()
        print("local_correlate_rotated(shift) g%s L=%d r=%d%s: worst error %.3g of max|want|" %
              (k, L, r, ", shared" if shared else "", err.max() / np.abs(w64).max()))
        assert (err <= bound).all(), (k, float((err - bound).max()), float(np.abs(w64).max()))


# ----------------------------------------------------------------------------------------------------------------------
# 9: errors
# ----------------------------------------------------------------------------------------------------------------------

def check_errors(lib, device):
    import pytest
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    x = torch.zeros(8 ** 3, device=dev)
    R = torch.eye(3, device=dev).reshape(1, 9).contiguous()
    o3, out9, out3 = torch.zeros(3, device=dev), torch.zeros(9, device=dev), torch.zeros(3, device=dev)
    T = torch.zeros(1, 3, dtype=torch.int32, device=dev)
    corr = torch.zeros(27, device=dev)
    ws = torch.empty(max(lib.call("dlpd_rotate_trilinear_pgrad_ws_bytes", 1, 8), lib.call("dlpd_local_ws_bytes", 1, 1, 8, 1)),
                     dtype=torch.uint8, device=dev)
    p, r, o, w, st = x.data_ptr(), R.data_ptr(), o3.data_ptr(), ws.data_ptr(), _stream(dev)

    def fwd(vol=p, Rm=r, off=o, out=p, B=1, C=1, L=8, stride=0):
        return lib.call("dlpd_rotate_trilinear_shift", vol, Rm, off, out, B, C, L, stride, L / 2.0, st)

    def adj(gout=p, Rm=r, off=o, gvol=p, B=1, C=1, L=8, stride=0):
        return lib.call("dlpd_rotate_trilinear_shift_grad", gout, Rm, off, gvol, B, C, L, stride, L / 2.0, 0, st)

    def pose(gout=p, vol=p, Rm=r, off=o, gR=out9.data_ptr(), goff=out3.data_ptr(), ws_=w, B=1, C=1, L=8, stride=0):
        return lib.call("dlpd_rotate_trilinear_pgrad", gout, vol, Rm, off, gR, goff, ws_, B, C, L, stride, L / 2.0, st)

    def corr_(rec=p, lig=p, Rm=r, off=o, T_=T.data_ptr(), out=corr.data_ptr(), ws_=w, P=1, C=1, L=8, rr=1):
        return lib.call("dlpd_local_correlate_shift", rec, lig, Rm, off, T_, out, ws_, P, C, L, rr, 1, 0, L / 2.0, 0, 0, st)

    def cgrad(rec=p, lig=p, Rm=r, off=o, T_=T.data_ptr(), g=corr.data_ptr(), grec=p, glig=None, P=1, C=1, L=8, rr=1):
        return lib.call("dlpd_local_correlate_shift_grad", rec, lig, Rm, off, T_, g, grec, glig, P, C, L, rr, 1, 0, L / 2.0, 0, 0, st)
    bad = [(fwd, (dict(vol=None), dict(Rm=None), dict(out=None), dict(B=0), dict(C=0), dict(stride=-1))),
           (adj, (dict(gout=None), dict(Rm=None), dict(gvol=None), dict(B=0), dict(C=-1), dict(stride=-1))),
           (pose, (dict(gout=None), dict(vol=None), dict(Rm=None), dict(gR=None, goff=None), dict(ws_=None), dict(B=0), dict(C=0),
                   dict(stride=-1))),
           (corr_, (dict(rec=None), dict(lig=None), dict(T_=None), dict(out=None), dict(ws_=None), dict(P=0), dict(Rm=None))),
           (cgrad, (dict(rec=None), dict(g=None), dict(grec=None), dict(P=0), dict(Rm=None)))]
    for fn, cases in bad:
        for kw in cases:
            with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
                fn(**kw)                                                 # (off with R == NULL among them: dict(Rm=None))
        for L in (1, 129):
            with pytest.raises(RuntimeError, match="UNSUPPORTED"):
                fn(L=L)                                                  # (refused before anything is read)
        assert fn() == 0
        assert fn(off=None) == 0                                         # off == NULL means zeros
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        corr_(rr=4)
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        cgrad(glig=p)                                                    # glig with R: as the plain entry
    assert pose(gR=None) == 0 and pose(goff=None) == 0
    for L in (1, 129):
        assert lib.call("dlpd_rotate_trilinear_pgrad_ws_bytes", 1, L) == 0
    assert lib.call("dlpd_rotate_trilinear_pgrad_ws_bytes", 0, 8) == 0
    assert lib.call("dlpd_rotate_trilinear_pgrad_ws_bytes", 3, 128) == 3 * lib.call("dlpd_rotate_trilinear_pgrad_ws_bytes", 1, 128) > 0
    assert 3 * lib.call("dlpd_rotate_trilinear_pgrad_ws_bytes", 1, 33) == 4 * lib.call("dlpd_rotate_trilinear_rgrad_ws_bytes", 1, 33)
    # ops: a shift without rotations is refused; so is a shift of the wrong shape
    v = torch.zeros(1, 8, 8, 8, device=dev)
    s = torch.zeros(1, 3, device=dev)
    with pytest.raises(RuntimeError, match="needs the rotations"):
        ops.local_correlate(v, v, T, shift=s, lib=lib)
    with pytest.raises(RuntimeError, match="needs the rotations"):
        ops.local_correlate_rotated(v, v, T, None, shift=s, lib=lib)
    with pytest.raises(RuntimeError, match="shift must be"):
        ops.local_correlate(v, v, T, R=R.reshape(1, 3, 3), shift=torch.zeros(2, 3, device=dev), lib=lib)
    with pytest.raises(RuntimeError, match="shift must be"):
        ops.VolumeRotation(lib=lib)(v, R.reshape(1, 3, 3), torch.zeros(3, device=dev))


# ----------------------------------------------------------------------------------------------------------------------
# 10, 11: Docker
# ----------------------------------------------------------------------------------------------------------------------

def planted_shifted(Ls, s_star=S_STAR, C=2, nblob=6, sigma=1.5, seed=3):
    """pose_grad_checks.planted with the ligand's blob centres displaced ANALYTICALLY so that the rotated ligand lies on the
    receptor at the translation s* (fine-grid voxels; s* L / Ls[0] on a coarser grid): the rotated ligand's blobs sit at the
    receptor's minus s*, i.e. the ligand's at c0 + (x - s*) M* (the kernel's map, out(i) = lig(c0 + (i - c0) M*))."""
    rs = np.random.RandomState(seed)
    dirs = rs.normal(size=(C, nblob, 3))
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    rad = rs.uniform(0.25, 0.37, size=(C, nblob, 1))
    Mstar = pg._expm([0.9, -1.7, 0.6])
    rec, lig = [], []
    for L in Ls:
        c0 = L / 2.0
        ar = np.arange(L, dtype=np.float64)
        X = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), axis=-1)
        vols = []
        for carry, disp in ((np.eye(3), np.zeros(3)), (Mstar.T, np.asarray(s_star, dtype=np.float64) * L / Ls[0])):
            cen = c0 + (dirs * rad * L - disp) @ carry.T
            v = np.zeros((C, L, L, L))
            for c in range(C):
                for k in range(nblob):
                    v[c] += np.exp(-((X - cen[c, k]) ** 2).sum(axis=-1) / (2 * (sigma * L / Ls[0]) ** 2))
            vols.append(torch.from_numpy(v).float()[None])
        rec.append(vols[0])
        lig.append(vols[1])
    return rec, lig, Mstar


def _docker(lib, device, L, R):
    from deeplocalproteindocking_amd.Docker import Docker
    return Docker(pg.PlantedModel(1e30), box_size=L, max_conf=10, rotations=R, device=device, lib=lib)


def check_score_poses(lib, device, Ls):
    """shift = 0 has the bytes of the call without it (a window, with a stored clash channel too); a fractional shift gives,
    within the derived bound, the float64 score of the ligand resampled at the displaced positions and correlated at T."""
    from deeplocalproteindocking_amd import ops
    L = Ls[0]
    rec, lig, _ = planted_shifted(Ls)
    P = 3
    R = lg.rots(P, seed=21)
    T = np.array([[0, 0, 0], [1, -2, 1], [-3, 2, 0]])
    s = np.random.RandomState(9).uniform(-0.9, 0.9, size=(P, 3))
    dk = _docker(lib, device, L, R)
    dev = dk.device
    ones = torch.ones(L, L, L)
    for kw in (dict(), dict(receptor_forbidden=ones, ligand_forbidden=ones)):
        a = dk.score_poses(rec, lig, R, T, radius=1, **kw)
        b = dk.score_poses(rec, lig, R, T, radius=1, shift=np.zeros((P, 3)), **kw)
        assert a.shape == (P, 3, 3, 3) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    got = dk.score_poses(rec, lig, R, T, shift=s).cpu().numpy().reshape(P).astype(np.float64)
    plain = dk.score_poses(rec, lig, R, T).cpu().numpy().reshape(P).astype(np.float64)
    R32, s32 = torch.from_numpy(R).float(), torch.from_numpy(s).float()
    want, bound = np.zeros(P), np.zeros(P)
    for k, Lk in enumerate(Ls):
        scale = L // Lk
        M = dk.conventions.matrices(R32.to(dev), Lk)
        off = ops._kernel_offset(M, (s32 / float(scale)).to(dev)).cpu().double().numpy()
        M, c0 = M.cpu().double().numpy(), dk.rotation_pivot(Lk)
        r64, l64 = rec[k][0].numpy().astype(np.float64), lig[k][0].numpy().astype(np.float64)
        C = r64.shape[0]
        for p in range(P):
            lrot = rotate64(l64, M[p], off[p], c0)
            lb, _ = forward_bound(l64, M[p], off[p], c0)
            a, b = lg._slices(np.floor(T[p] / float(scale)).astype(int), Lk)
            corr = (r64[a] * lrot[b]).sum(axis=(1, 2, 3))
            mag = np.abs(r64[a] * lrot[b]).sum()
            want[p] -= corr.sum()
            bound[p] += (np.abs(r64[a]) * lb[b]).sum() + (2 * Lk + 16) * EPS * mag + (C + 2) * EPS * np.abs(corr).sum()
    bound += 2 * EPS * np.abs(want)                                      # (the two resolutions' features, added by the filter)
    print("score_poses(shift) boxes %s: scores %s, without the shift %s; worst error %.3g of the bound" %
          (Ls, got, plain, float((np.abs(got - want) / bound).max())))
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)
    assert (np.abs(plain - want) > bound).all()                          # (the shift is seen)


def check_minimize_unchanged(lib, device, Ls, tmp_path):
    """translation=False is the descent as it was: pose_grad_checks.check_minimize's own assertions, called unchanged."""
    return pg.check_minimize(lib, device, Ls, tmp_path)


def check_minimize_translation(lib, device, Ls, tmp_path, steps=20):
    """The planted pose with a planted fraction: the ligand lies on the receptor at M* and the translation s* = (0.37, -0.41,
    0.22) voxels; the start is 6 degrees from M* at T = 0.  Inequalities only; the residuals are printed."""
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Results.DockerParser import DockerParser
    L = Ls[0]
    rec, lig, Mstar = planted_shifted(Ls)
    axis = np.array([0.5, -0.7, 0.4])
    start = pg._expm(np.radians(6.0) * axis / np.linalg.norm(axis)) @ Mstar
    R = np.stack([start, start])
    dk = _docker(lib, device, L, R)
    poses = [(0, 0, 0, 0, 0.0)]
    top_before = list(dk.top_list)
    rot = [tuple(e) for e in dk.minimize(rec, lig, poses=poses, steps=steps)]
    got = [tuple(e) for e in dk.minimize(rec, lig, poses=poses, steps=steps, translation=True)]
    again = dk.minimize(rec, lig, poses=poses, steps=steps, translation=True)
    assert dk.top_list == top_before and len(got) == 1 and len(rot) == 1
    assert [(e[0].tobytes(), e[1], e[2], e[3]) for e in got] == [(e[0].tobytes(), e[1], e[2], e[3]) for e in again]   # the same bytes
    (Rr, tr, fr, _), (Rt, tt, ft, n) = rot[0], got[0]
    assert all(isinstance(v, int) for v in tr) and all(isinstance(v, float) for v in tt) and n == 0
    a0, ar, at = pg.angle_between(start, Mstar), pg.angle_between(Rr, Mstar), pg.angle_between(Rt, Mstar)
    res_r, res_t = float(np.linalg.norm(np.array(tr) - S_STAR)), float(np.linalg.norm(np.array(tt) - S_STAR))
    print("minimize(translation=True), boxes %s: start %.2f deg from M* at T = 0; rotation only: %.3f deg, t %s, |t - s*| %.3f, "
          "score %.4f; rigid body: %.3f deg, t (%.3f, %.3f, %.3f), |t - s*| %.3f, score %.4f" %
          (Ls, a0, ar, tr, res_r, fr, at, tt[0], tt[1], tt[2], res_t, ft))
    assert ft < fr                                                       # a strictly lower score than the rotation alone reaches
    assert res_t < res_r                                                 # closer to the planted translation
    assert at <= ar                                                      # and no further from the planted rotation
    assert Rt.dtype == np.float64 and Rt.shape == (3, 3) and np.abs(Rt @ Rt.T - np.eye(3)).max() < 1e-12
    Tn, sn = Docker.split_translation(tt)
    assert all(abs(v) <= 0.5 for v in sn)
    assert float(dk.score_poses(rec, lig, Rt[None], [Tn], shift=[sn])[0, 0, 0, 0]) == ft     # the list's score is score_poses' own
    # a clash mask over the whole window: the source comes back (as a translation of floats)
    ones = torch.ones(L, L, L)
    dk.docking_model.threshold_clash = 1.0
    masked = dk.minimize(rec, lig, ones, ones, poses=[(1, 1, 2 * L - 1, 0, 0.0)], steps=steps, translation=True)
    assert len(masked) == 1 and masked[0][0].tobytes() == R[1].astype(np.float64).tobytes()
    assert masked[0][1] == (1.0, -1.0, 0.0) and masked[0][2] == 0.0 and masked[0][3] == 0
    dk.docking_model.threshold_clash = 1e30
    # a clash channel that never bites changes nothing (the stored volume is displaced with the ligand)
    free = dk.minimize(rec, lig, ones, ones, poses=poses, steps=steps, translation=True)
    assert free[0][0].tobytes() == Rt.tobytes() and tuple(free[0][1:]) == (tt, ft, 0)
    # the .dat round trip through the consumer: the fractional translation times the resolution
    dk.refined_list = got
    dk.new_log(str(tmp_path / "P2.dat"))
    dk.write_refined_conformations()
    dk.cleanup()
    confs = DockerParser(str(tmp_path), coords_backend=object()).parse_output("P2")["conformations"]
    assert len(confs) == 1 and np.abs(confs[0][0][0].numpy() - Rt).max() < 1e-6 and abs(confs[0][2] - ft) < 1e-6 * max(1.0, abs(ft))
    # the file's own columns are (T + s) * resolution; parse_output keeps their int(), as of every .dat (DockerParser.py:51)
    cols = np.array([float(c) for c in open(str(tmp_path / "P2.dat")).read().split()[9:12]])
    want_t = np.array(tt) * dk.resolution
    assert np.abs(cols - want_t).max() < 1e-6 and np.abs(cols / dk.resolution - np.rint(cols / dk.resolution)).max() > 1e-3
    assert confs[0][1].reshape(-1).tolist() == [float(int(v)) for v in cols]
    return dict(start=a0, rot_angle=ar, rot_res=res_r, rot_score=fr, rigid_angle=at, rigid_res=res_t, rigid_score=ft, t=tt)
