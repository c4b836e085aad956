"""Check bodies shared by tests/test_pose_grad_emu.py (the kernel sources on the fibre emulator) and
tests/test_pose_grad_gpu.py (the gfx950 build): the gradient of the trilinear rotation with respect to its matrices
(csrc/dlpd_rotate_rgrad.h), ``rotation_grad=True`` of ops.VolumeRotation and ops.local_correlate_rotated, Docker.minimize.

The expectation is rotate_grad_checks' float64 gather (``rotate_torch``: the corners of corners64 as index gathers in torch)
differentiated by AUTOGRAD through a = p - floor(p) -- independent of the kernel's closed form -- and itself held to a
central difference of ``rotate64`` (check_expectation).

The bound, per element [j][a] of a pose's nine numbers (derived, not tuned; ``bound64``):

  |got - want| <= (C + 16) 2^-24 A + 2 delta B + flip

  A     = sum_i,c |g| (sum over the four corner pairs of w |V1 - V0|) |i_j - c0|: the sum of |terms|.  The kernel's value of one
          term carries ~8 f32 roundings (1 - a, the weight product, the difference, the product, three additions), the chain
          over the channels C more, the cast of the float64 total one: (C + 16) covers them.
  B     = sum_i,c |g| (sum over the four corner pairs of |V1 - V0|) |i_j - c0|: the derivative along a is linear in the fractions
          of the two other axes with slopes bounded by that sum, and the kernel's f32 sample position is off by at most
          delta = 8 2^-24 L per axis (three products and three additions of magnitude <= L).
  flip  = for every sample whose float64 position lies within delta of an integer along axis a: |g| |D+ - D-| |i_j - c0| summed
          over the channels -- the f32 and the f64 floor may pick different cells there and the derivative ALONG that axis jumps
          (across a face the derivatives along the other two axes are continuous).  Fewer than 1 in 1,000 samples may be such.
  With ``g_err`` (the error bound of a g that was itself computed in f32: local_correlate_rotated) the term
  sum_i,c g_err |d_a vol| |i_j - c0| is added."""
import functools
import itertools

import numpy as np
import torch

import local_grad_checks as lg
import rotate_grad_checks as rg

EPS = lg.EPS


def _ptr(t):
    return t.data_ptr()


# ----------------------------------------------------------------------------------------------------------------------
# float64: the expectation (autograd) and the pieces of the bound (numpy)
# ----------------------------------------------------------------------------------------------------------------------

def expect64(g, v, M, c0):
    """g, v (C, L, L, L) float64, M (3, 3) -> d/dM of sum(g * rotate(v, M)) (3, 3): element [j][a] is the kernel's gR[3j + a]."""
    Mt = torch.tensor(np.asarray(M, dtype=np.float64).reshape(1, 3, 3), requires_grad=True)
    out = rg.rotate_torch(torch.from_numpy(np.ascontiguousarray(v)), Mt, float(c0))[0]
    (gM,) = torch.autograd.grad((out * torch.from_numpy(np.ascontiguousarray(g))).sum(), Mt)
    return gM[0].numpy()


def _geometry(M, c0, L):
    ar = np.arange(L, dtype=np.float64) - c0
    d = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), axis=-1).reshape(-1, 3)
    return d, c0 + d @ np.asarray(M, dtype=np.float64).reshape(3, 3)


def _corner_table(v, i0):
    """v (C, L, L, L), cells i0 (n, 3) -> the eight corner values (C, 2, 2, 2, n), zero outside the box."""
    C, L = v.shape[0], v.shape[-1]
    flat = v.reshape(C, -1)
    V = np.zeros((C, 2, 2, 2, i0.shape[0]))
    for o in itertools.product((0, 1), repeat=3):
        c = i0 + np.array(o)
        ok = ((c >= 0) & (c < L)).all(axis=1)
        c = np.clip(c, 0, L - 1)
        V[:, o[0], o[1], o[2]] = flat[:, (c[:, 0] * L + c[:, 1]) * L + c[:, 2]] * ok
    return V


def _axis_derivs(V, a):
    """Corner values (C, 2, 2, 2, n), fractions a (n, 3) -> per axis (3, C, n): the derivative of the trilinear cell, the same sum
    with |V1 - V0| (weighted), and the plain sum of the four |V1 - V0|."""
    w = [np.stack([1.0 - a[:, k], a[:, k]]) for k in range(3)]
    D, Dw, D4 = [], [], []
    for ax in range(3):
        Vm = np.moveaxis(V, 1 + ax, 1)
        delta = Vm[:, 1] - Vm[:, 0]                                      # (C, 2, 2, n): the two other axes in order
        o1, o2 = [k for k in range(3) if k != ax]
        ww = w[o1][:, None, :] * w[o2][None, :, :]
        D.append((delta * ww).sum(axis=(1, 2)))
        Dw.append((np.abs(delta) * ww).sum(axis=(1, 2)))
        D4.append(np.abs(delta).sum(axis=(1, 2)))
    return np.stack(D), np.stack(Dw), np.stack(D4)


def bound64(g, v, M, c0, g_err=None):
    """-> (bound (3, 3), A (3, 3), fraction of samples within delta of a cell face)."""
    C, L = v.shape[0], v.shape[-1]
    d, p = _geometry(M, c0, L)
    f = np.floor(p)
    a, i0 = p - f, f.astype(np.int64)
    D, Dw, D4 = _axis_derivs(_corner_table(v, i0), a)
    ga, e = np.abs(g).reshape(C, -1), np.abs(d)
    A = e.T @ (ga[None] * Dw).sum(axis=1).T                              # [j][a]
    B = e.T @ (ga[None] * D4).sum(axis=1).T
    delta = 8 * EPS * L
    # (the pivot's own voxel, i = c0 for an even box, sits ON an integer in either precision -- c0 + 0 -- and cannot flip)
    near = (np.abs(p - np.rint(p)) <= delta) & (np.abs(d).sum(axis=1) > 0)[:, None]
    flagged = np.nonzero(near.any(axis=1))[0]
    flip = np.zeros((3, 3))
    for k in range(3):
        sel = flagged[near[flagged, k]]
        if len(sel) == 0:
            continue
        q = np.rint(p[sel, k]).astype(np.int64)
        side = []
        for cell, frac in ((q, 0.0), (q - 1, 1.0)):                      # the cell on the right of the face, and on the left
            ic, ac = i0[sel].copy(), a[sel].copy()
            ic[:, k], ac[:, k] = cell, frac
            side.append(_axis_derivs(_corner_table(v, ic), ac)[0][k])
        flip[:, k] += e[sel].T @ (ga[:, sel] * np.abs(side[0] - side[1])).sum(axis=0)
    bound = (C + 16) * EPS * A + 2 * delta * B + flip
    if g_err is not None:
        bound = bound + e.T @ (np.abs(g_err).reshape(C, -1)[None] * np.abs(D)).sum(axis=1).T
    return bound, A, len(flagged) / float(L ** 3)


def check_expectation(L=9, C=2, h=1e-6):
    """The autograd expectation against a central difference of rotate64 (CPU, float64).  Tolerance: f is a sum of products
    of magnitude <= A' = sum |g| |corner values|; its float64 rounding (~K 2^-53 A', K ~ 100 operations deep) divided by 2 h
    gives 1e-8 A' at h = 1e-6; within a cell f is multilinear in M, the central difference's error is second order
    (h^2 L^2 A'), far below.  No sample may lie within 2 h L of a cell face (asserted), where the difference would straddle
    a kink."""
    g_ = torch.Generator().manual_seed(91)
    g, v = torch.randn(C, L, L, L, generator=g_, dtype=torch.float64).numpy(), torch.randn(C, L, L, L, generator=g_, dtype=torch.float64).numpy()
    M, c0 = lg.rots(1, seed=12)[0].astype(np.float64), L / 2.0
    d, p = _geometry(M, c0, L)
    assert (np.abs(p - np.rint(p))[np.abs(d).sum(axis=1) > 0] > 2 * h * L).all()
    want = expect64(g, v, M, c0)
    scale = float((np.abs(g) * rg.rotate64(np.abs(v), M, c0)).sum())
    for j in range(3):
        for a in range(3):
            E = np.zeros((3, 3))
            E[j, a] = h
            fd = ((g * rg.rotate64(v, M + E, c0)).sum() - (g * rg.rotate64(v, M - E, c0)).sum()) / (2 * h)
            assert abs(fd - want[j, a]) <= 1e-7 * scale, (j, a, fd, want[j, a], scale)
    assert np.abs(want).max() > 1e-3 * scale


# ----------------------------------------------------------------------------------------------------------------------
# 1: the kernel against float64
# ----------------------------------------------------------------------------------------------------------------------

def rgrad(lib, dev, g, v, R, L, C, B, stride, c0):
    """dlpd_rotate_trilinear_rgrad; gR starts as NaN (every element must be written)."""
    out = torch.full((B, 9), float("nan"), dtype=torch.float32, device=dev)
    n = lib.call("dlpd_rotate_trilinear_rgrad_ws_bytes", B, L)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    lib.call("dlpd_rotate_trilinear_rgrad", _ptr(g), _ptr(v), _ptr(R), _ptr(out), _ptr(ws), B, C, L, stride, c0, lg._stream(dev))
    return out.cpu().numpy().reshape(B, 3, 3)


@functools.lru_cache(maxsize=None)
def case(L, C, B, seed=0):
    g_ = torch.Generator().manual_seed(9000 * L + 10 * C + B + seed)
    g = torch.randn(B, C, L, L, L, generator=g_)
    v = torch.randn(B, C, L, L, L, generator=g_)
    R = torch.from_numpy(lg.rots(B, seed=seed + L + 3)).float().contiguous()
    return g, v, R, float(L) / 2.0


@functools.lru_cache(maxsize=None)
def reference(L, C, B, b, vb, seed=0):
    """The float64 expectation and its bound for gradient b of the case against volume vb: computed once (read only)."""
    g, v, R, c0 = case(L, C, B, seed)
    g64, v64, M = g[b].numpy().astype(np.float64), v[vb].numpy().astype(np.float64), R[b].numpy().astype(np.float64)
    want = expect64(g64, v64, M, c0)
    bound, A, frac = bound64(g64, v64, M, c0)
    for t in (want, bound, A):
        t.setflags(write=False)
    return want, bound, A, frac


def _compare(label, got, want, bound, A, frac=0.0):
    err = np.abs(got - want)
    print("%s: worst error %.3g of the bound, %.3g of sum|terms|; max|want| / sum|terms| %.3g; near a face %.2g" %
          (label, float((err / np.maximum(bound, 1e-300)).max()), float((err / np.maximum(A, 1e-300)).max()),
           float((np.abs(want) / np.maximum(A, 1e-300)).max()), frac))
    assert frac < 1e-3, frac
    assert np.isfinite(got).all(), "every element is written"
    assert (err <= bound).all(), (got, want, bound)


def check_kernel(lib, device, L, C, B, seed=0):
    """One volume for all poses (stride 0) and one per pose; the same bytes twice."""
    dev = torch.device(device)
    g, v, R, c0 = case(L, C, B, seed)
    d_g, d_v, d_R = g.to(dev).contiguous(), v.to(dev).contiguous(), R.to(dev).contiguous()
    for shared in (True, False):
        stride = 0 if shared else C * L ** 3
        got = rgrad(lib, dev, d_g, d_v, d_R, L, C, B, stride, c0)
        assert got.tobytes() == rgrad(lib, dev, d_g, d_v, d_R, L, C, B, stride, c0).tobytes(), "the same bits run to run"
        for b in range(B):
            want, bound, A, frac = reference(L, C, B, b, 0 if shared else b, seed)
            assert (np.abs(want) > 1e-4 * A).any()                       # (something to measure)
            _compare("rotate_trilinear_rgrad L=%d C=%d b=%d%s" % (L, C, b, ", shared volume" if shared else ""), got[b], want,
                     bound, A, frac)


# ----------------------------------------------------------------------------------------------------------------------
# 2: cases with teeth
# ----------------------------------------------------------------------------------------------------------------------

def check_ramp(lib, device, L, C=3, B=2):
    """vol_c = al_c x + be_c y + ga_c z, g >= 0 and zero on the samples that have a corner outside the box: the derivative is
    the constant slope on every sample that counts, gR[j][a] = sum_c slope[c][a] sum_i g_c(i) (i_j - c0) in closed form."""
    dev = torch.device(device)
    g_ = torch.Generator().manual_seed(77 + L)
    slope = torch.randn(C, 3, generator=g_, dtype=torch.float64).numpy()
    ar = np.arange(L, dtype=np.float64)
    X, Y, Z = np.meshgrid(ar, ar, ar, indexing="ij")
    v64 = slope[:, 0, None, None, None] * X + slope[:, 1, None, None, None] * Y + slope[:, 2, None, None, None] * Z
    v = torch.from_numpy(v64).float()
    R = torch.from_numpy(lg.rots(B, seed=L + 5)).float().contiguous()
    c0 = float(L) / 2.0
    g = torch.rand(B, C, L, L, L, generator=g_)
    want = np.zeros((B, 3, 3))
    for b in range(B):
        d, p = _geometry(R[b].numpy(), c0, L)
        inside = ((np.floor(p) >= 0) & (np.floor(p) + 1 <= L - 1)).all(axis=1)
        assert 0.2 < inside.mean() < 1.0
        g[b] *= torch.from_numpy(inside.reshape(1, L, L, L)).float()
        want[b] = d.T @ (g[b].numpy().astype(np.float64).reshape(C, -1).T @ slope)       # [j][a]
    got = rgrad(lib, dev, g.to(dev).contiguous(), v.to(dev).contiguous(), R.to(dev), L, C, B, 0, c0)
    for b in range(B):
        bound, A, frac = bound64(g[b].numpy().astype(np.float64), v.numpy().astype(np.float64), R[b].numpy(), c0)
        assert (np.abs(want[b]) > 1e-2 * A).any()
        _compare("ramp L=%d b=%d" % (L, b), got[b], want[b], bound, A, frac)


def check_signed_permutations(lib, device, L=33, C=2):
    """The 24 signed permutations about L / 2: every sample position is an exact integer q, the fractions are zero, and the
    derivative along a is the forward difference of the cell floorf picks: V(q + e_a) - V(q), V the volume continued by zeros
    (index L is outside).  No position error and no flip: the bound is the first term alone."""
    from accuracy_checks import signed_permutations
    dev = torch.device(device)
    perms = signed_permutations()
    B = len(perms)
    g_ = torch.Generator().manual_seed(L)
    g, v = torch.randn(B, C, L, L, L, generator=g_), torch.randn(C, L, L, L, generator=g_)
    R = torch.from_numpy(perms).float().contiguous()
    c0 = float(L) / 2.0
    got = rgrad(lib, dev, g.to(dev), v.to(dev), R.to(dev), L, C, B, 0, c0)
    pad = np.zeros((C, L + 3, L + 3, L + 3))
    pad[:, 1:L + 1, 1:L + 1, 1:L + 1] = v.numpy().astype(np.float64)                    # pad[q + 1] = V(q), -1 <= q <= L + 1
    seen_outside = False
    for b in range(B):
        d, p = _geometry(perms[b], c0, L)
        q = np.rint(p).astype(np.int64)
        assert (p == q).all() and q.min() >= -1 and q.max() <= L
        seen_outside |= bool((q >= L).any())
        V0 = pad[:, q[:, 0] + 1, q[:, 1] + 1, q[:, 2] + 1]
        gb = g[b].numpy().astype(np.float64).reshape(C, -1)
        want, A = np.zeros((3, 3)), np.zeros((3, 3))
        for a in range(3):
            qa = q.copy()
            qa[:, a] += 1
            Da = pad[:, qa[:, 0] + 1, qa[:, 1] + 1, qa[:, 2] + 1] - V0
            want[:, a] = d.T @ (gb * Da).sum(axis=0)
            A[:, a] = np.abs(d).T @ (np.abs(gb) * np.abs(Da)).sum(axis=0)
        err = np.abs(got[b] - want)
        assert (err <= (C + 16) * EPS * A).all(), (b, got[b], want)
        assert (np.abs(want) > 1e-5 * A).any()
    assert seen_outside


def check_zero_and_scaling(lib, device, L=9, C=3, B=2):
    dev = torch.device(device)
    g, v, R, c0 = case(L, C, B)
    d_g, d_v, d_R = g.to(dev).contiguous(), v.to(dev).contiguous(), R.to(dev).contiguous()
    zero = rgrad(lib, dev, torch.zeros_like(d_g), d_v, d_R, L, C, B, C * L ** 3, c0)
    assert (zero == 0).all()
    one = rgrad(lib, dev, d_g, d_v, d_R, L, C, B, C * L ** 3, c0)
    for k in (-7, 5):
        scaled = rgrad(lib, dev, (d_g * 2.0 ** k).contiguous(), d_v, d_R, L, C, B, C * L ** 3, c0)
        assert scaled.tobytes() == (one * np.float32(2.0 ** k)).tobytes() and np.abs(one).min() > 0


# ----------------------------------------------------------------------------------------------------------------------
# 3, 4: chunking and the autograd surface
# ----------------------------------------------------------------------------------------------------------------------

def _correlate_inputs(dev, L, C, P, r, scale, mode, shared, seed=0):
    g_ = torch.Generator().manual_seed(700 * L + 10 * r + seed)
    W = 2 * r + 1
    nv = () if shared else (P,)
    rec, lig = torch.randn(*nv, C, L, L, L, generator=g_), torch.randn(*nv, C, L, L, L, generator=g_)
    gout = torch.randn(P, C, W, W, W, generator=g_)
    T = torch.from_numpy(lg.translations(P, L, scale, seed)).int()
    R = torch.from_numpy(lg.rots(P, seed=seed + L + 1)).float().contiguous()
    return rec, lig, T, R, gout


def _run_rotated(ops, lib, d, kw, rotation_grad):
    a, b, Rg = d[0].clone().requires_grad_(), d[1].clone().requires_grad_(), d[3].clone().requires_grad_()
    out = ops.local_correlate_rotated(a, b, d[2], Rg, rotation_grad=rotation_grad, **kw) if rotation_grad is not None else \
        ops.local_correlate_rotated(a, b, d[2], Rg, **kw)
    out.backward(d[4])
    return out.detach().cpu().numpy(), a.grad.cpu().numpy(), b.grad.cpu().numpy(), None if Rg.grad is None else Rg.grad.cpu().numpy()


def check_chunking(lib, device, monkeypatch, L=8, C=2, P=5, r=1):
    """LOCAL_WS_BYTES of one pose's volume: five chunks of one pose.  R.grad has the bytes of the unsplit call; so have the
    volumes' gradients, which are also the bytes of the call without the flag."""
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    for shared in (True, False):
        d = [t.to(dev).contiguous() for t in _correlate_inputs(dev, L, C, P, r, 1, "floor", shared)]
        kw = dict(radius=r, lib=lib)
        whole = _run_rotated(ops, lib, d, kw, True)
        plain = _run_rotated(ops, lib, d, kw, None)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "LOCAL_WS_BYTES", 4 * C * L ** 3)
            split = _run_rotated(ops, lib, d, kw, True)
        assert whole[3].shape == (P, 3, 3) and np.abs(whole[3]).max() > 0 and plain[3] is None
        for k in range(4):
            assert whole[k].tobytes() == split[k].tobytes(), k
        for k in range(3):
            assert whole[k].tobytes() == plain[k].tobytes(), k


def check_volume_rotation_autograd(lib, device, L=9, C=3, B=3, **conv):
    """Flag off: today's bytes and no gradient for R.  Flag on: R.grad against float64 through kernel_matrices."""
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.Utils.Conventions import kernel_matrices, rotation_scale
    dev = torch.device(device)
    g_ = torch.Generator().manual_seed(57 + L)
    vol, gout = torch.randn(B, C, L, L, L, generator=g_).to(dev), torch.randn(B, C, L, L, L, generator=g_).to(dev)
    R = torch.from_numpy(lg.rots(B, seed=L + 2)).float().contiguous().to(dev)
    c0 = float(L) / 2.0 if conv.get("center") is None else float(conv["center"])
    fold = (rotation_scale(conv.get("scale"), L), conv.get("axis_order", "xyz"), conv.get("transpose", False))
    M = kernel_matrices(R, *fold)
    off, on = ops.VolumeRotation(lib=lib, **conv), ops.VolumeRotation(lib=lib, rotation_grad=True, **conv)
    plain = off(vol, R)
    res = {}
    for name, op in (("off", off), ("on", on)):
        a, Rg = vol.clone().requires_grad_(), R.clone().requires_grad_()
        out = op(a, Rg)
        assert out.requires_grad and out.detach().cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
        out.backward(gout)
        res[name] = (a.grad.cpu().numpy(), Rg.grad)
    direct = rg.adjoint(lib, dev, gout.contiguous(), M.contiguous(), L, C, B, C * L ** 3, c0).cpu().numpy()
    assert res["off"][1] is None and res["off"][0].tobytes() == direct.tobytes() == res["on"][0].tobytes()
    got = res["on"][1]
    assert got is not None and got.shape == R.shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    R64 = R.cpu().double().requires_grad_()
    M64 = M.cpu().double().numpy()                                       # (the maps the kernel took, as float64)
    for b in range(B):
        g64, v64 = gout[b].cpu().numpy().astype(np.float64), vol[b].cpu().numpy().astype(np.float64)
        wantM = expect64(g64, v64, M64[b], c0)
        boundM, A, frac = bound64(g64, v64, M64[b], c0)
        # back through kernel_matrices (a signed permutation times a positive scale: linear, the bound maps the same way; the
        # f32 product with the scale is one more rounding of the value)
        folded = kernel_matrices(R64[b:b + 1], *fold)
        want = torch.autograd.grad(folded, R64, torch.from_numpy(wantM)[None], retain_graph=True)[0][b].numpy()
        bound = torch.autograd.grad(folded, R64, torch.from_numpy(boundM)[None], retain_graph=True)[0][b].numpy()
        AR = torch.autograd.grad(folded, R64, torch.from_numpy(A)[None])[0][b].numpy()
        _compare("VolumeRotation R.grad L=%d b=%d %s" % (L, b, conv or ""), got[b], want, bound + 2 * EPS * np.abs(want), AR, frac)
    # R alone asks for a gradient; no graph under no_grad, none without the flag
    Rg = R.clone().requires_grad_()
    out = on(vol, Rg)
    assert out.requires_grad
    out.backward(gout)
    assert Rg.grad.cpu().numpy().tobytes() == res["on"][1].cpu().numpy().tobytes()
    assert not off(vol, Rg).requires_grad
    with torch.no_grad():
        assert not on(vol.clone().requires_grad_(), Rg).requires_grad
    # one (C, L, L, L) volume for all B matrices: the stride-0 kernel call's bytes
    Rg = R.clone().requires_grad_()
    on(vol[0], Rg).backward(gout)
    if not conv:
        want0 = rgrad(lib, dev, gout.contiguous(), vol[0].contiguous(), R.contiguous(), L, C, B, 0, c0)
        assert Rg.grad.cpu().numpy().tobytes() == want0.tobytes()
    assert float(Rg.grad.abs().max()) > 0


def check_local_correlate_rotated(lib, device, L, C, P, r, scale, mode, shared, seed=0):
    """R.grad of ops.local_correlate_rotated(rotation_grad=True) against float64: the correlation's adjoint on the float64
    rotated ligand gives the gradient G of every pose's rotated ligand (local_grad_checks.adjoint64), the expectation above
    carries it to the matrix.  The bound is bound64's with G, plus the f32 error of the kernel's own G -- local_grad_checks'
    bound for the correlation's adjoint, 2 (W^3 + 1) 2^-24 sum|terms| per voxel -- carried through |d_a vol| |i_j - c0|."""
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    W = 2 * r + 1
    rec, lig, T, R, gout = _correlate_inputs(dev, L, C, P, r, scale, mode, shared, seed)
    tau = lg.coarse(T.numpy(), scale, mode)
    c0 = float(L) / 2.0
    d = [t.to(dev).contiguous() for t in (rec, lig, T, R, gout)]
    kw = dict(radius=r, scale=scale, coarse=mode, lib=lib)
    plain = ops.local_correlate(d[0], d[1], d[2], R=d[3], **kw)
    out, grec, glig, gR = _run_rotated(ops, lib, d, kw, True)
    off = _run_rotated(ops, lib, d, kw, False)
    assert out.tobytes() == plain.cpu().numpy().tobytes() == off[0].tobytes()
    assert grec.tobytes() == off[1].tobytes() and glig.tobytes() == off[2].tobytes() and off[3] is None
    assert gR.shape == (P, 3, 3)
    # R alone: the same nine numbers per pose
    Rg = d[3].clone().requires_grad_()
    o = ops.local_correlate_rotated(d[0], d[1], d[2], Rg, rotation_grad=True, **kw)
    assert o.requires_grad
    o.backward(d[4])
    assert Rg.grad.cpu().numpy().tobytes() == gR.tobytes()
    with torch.no_grad():
        assert not ops.local_correlate_rotated(d[0], d[1], d[2], Rg, rotation_grad=True, **kw).requires_grad
    measured = 0
    for p in range(P):
        vsel = () if shared else (p,)
        l64, M = lig[vsel].numpy().astype(np.float64), R[p].numpy().astype(np.float64)
        lrot = rg.rotate64(l64, M, c0)
        _, G, _, mG = lg.adjoint64(rec[vsel].numpy().astype(np.float64), lrot, gout[p].numpy().astype(np.float64), tau[p], r)
        if not G.any():
            assert (gR[p] == 0).all(), p                                 # (no overlap anywhere in the window: exactly zero)
            continue
        want = expect64(G, l64, M, c0)
        bound, A, frac = bound64(G, l64, M, c0, g_err=2 * (W ** 3 + 1) * EPS * mG)
        measured += int((np.abs(want) > 1e-4 * A).any())
        _compare("local_correlate_rotated R.grad L=%d r=%d scale %d %s%s pose %d" % (L, r, scale, mode, ", shared" if shared else "", p),
                 gR[p], want, bound, A, frac)
    assert measured >= 2


# ----------------------------------------------------------------------------------------------------------------------
# 5: errors
# ----------------------------------------------------------------------------------------------------------------------

def check_errors(lib, device):
    import pytest
    dev = torch.device(device)
    x = torch.zeros(8 ** 3, device=dev)
    R = torch.eye(3, device=dev).reshape(1, 9).contiguous()
    out = torch.zeros(9, device=dev)
    ws = torch.empty(lib.call("dlpd_rotate_trilinear_rgrad_ws_bytes", 1, 8), dtype=torch.uint8, device=dev)
    p, r, o, w = x.data_ptr(), R.data_ptr(), out.data_ptr(), ws.data_ptr()

    def call(gout=p, vol=p, Rm=r, gR=o, ws_=w, B=1, C=1, L=8, stride=0):
        return lib.call("dlpd_rotate_trilinear_rgrad", gout, vol, Rm, gR, ws_, B, C, L, stride, L / 2.0, lg._stream(dev))
    for kw in (dict(gout=None), dict(vol=None), dict(Rm=None), dict(gR=None), dict(ws_=None), dict(B=0), dict(C=0), dict(C=-1),
               dict(stride=-1)):
        with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
            call(**kw)
    for L in (1, 129):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            call(L=L)                                                    # (refused before anything is read)
        assert lib.call("dlpd_rotate_trilinear_rgrad_ws_bytes", 1, L) == 0
    assert lib.call("dlpd_rotate_trilinear_rgrad_ws_bytes", 0, 8) == 0
    assert lib.call("dlpd_rotate_trilinear_rgrad_ws_bytes", 3, 128) == 3 * lib.call("dlpd_rotate_trilinear_rgrad_ws_bytes", 1, 128) > 0
    assert call() == 0 and call(stride=512) == 0


# ----------------------------------------------------------------------------------------------------------------------
# 6: Docker.minimize on a planted pose
# ----------------------------------------------------------------------------------------------------------------------

def _expm(w):
    w = np.asarray(w, dtype=np.float64)
    t = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) if t == 0 else np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / t ** 2 * (K @ K)


def angle_between(A, B):
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(A) @ np.asarray(B).T) - 1.0) / 2.0, -1.0, 1.0))))


class NegativeSum(torch.nn.Module):
    """A user filter: rows (n, C) -> -sum_c, what the planted case scores with (low = good overlap)."""

    def forward(self, feat):
        return -feat.sum(dim=1, keepdim=True)


class PlantedModel(torch.nn.Module):
    def __init__(self, threshold_clash):
        super().__init__()
        self.filter = NegativeSum()
        self.clip = 1e30
        self.threshold_clash = threshold_clash


def planted(Ls, C=2, nblob=6, sigma=1.5, seed=3):
    """Receptor: ``nblob`` Gaussian blobs per channel at radius 0.25-0.37 L round the pivot L / 2; ligand: the same blobs
    evaluated ANALYTICALLY (no interpolation) at centres carried by M* -- so that rotating the ligand's volume by M* (the
    kernel's map, out(i) = lig(c0 + M*^T (i - c0))) lays it on the receptor.  One volume pair per edge of ``Ls`` (the blobs
    scaled to each grid).  -> (receptor volumes, ligand volumes, M*)."""
    rs = np.random.RandomState(seed)
    dirs = rs.normal(size=(C, nblob, 3))
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    rad = rs.uniform(0.25, 0.37, size=(C, nblob, 1))
    Mstar = _expm([0.9, -1.7, 0.6])
    rec, lig = [], []
    for L in Ls:
        c0 = L / 2.0
        ar = np.arange(L, dtype=np.float64)
        X = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), axis=-1)                   # (L, L, L, 3)
        vols = []
        for carry in (np.eye(3), Mstar.T):
            cen = c0 + (dirs * rad * L) @ carry.T                                       # x' = carry x
            v = np.zeros((C, L, L, L))
            for c in range(C):
                for k in range(nblob):
                    v[c] += np.exp(-((X - cen[c, k]) ** 2).sum(axis=-1) / (2 * (sigma * L / Ls[0]) ** 2))
            vols.append(torch.from_numpy(v).float()[None])
        rec.append(vols[0])
        lig.append(vols[1])
    return rec, lig, Mstar


def check_minimize(lib, device, Ls, tmp_path, steps=20):
    """The planted case: conditions (a)-(f) of the minimiser, inequalities only.  Pose 0 starts 6 degrees from M*; pose 1 is
    the same start behind a clash mask that covers its whole window."""
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Results.DockerParser import DockerParser
    L = Ls[0]
    rec, lig, Mstar = planted(Ls)
    axis = np.array([0.5, -0.7, 0.4])
    start = _expm(np.radians(6.0) * axis / np.linalg.norm(axis)) @ Mstar
    R = np.stack([start, start])
    dk = Docker(PlantedModel(1e30), box_size=L, max_conf=10, rotations=R, device=device, lib=lib)
    poses = [(0, 0, 0, 0, 0.0)]
    source = dk.score_poses(rec, lig, R[:1], [(0, 0, 0)])
    refined = [list(e) for e in dk.refine(rec, lig, poses=poses)]
    top_before = list(dk.top_list)
    got = dk.minimize(rec, lig, poses=poses, steps=steps)
    again = dk.minimize(rec, lig, poses=poses, steps=steps)
    assert dk.top_list == top_before and len(got) == 1
    assert [(e[0].tobytes(), e[1], e[2], e[3]) for e in got] == [(e[0].tobytes(), e[1], e[2], e[3]) for e in again]
    Rm, tt, score, n = got[0]
    a0, a1, a2 = angle_between(start, Mstar), angle_between(Rm, Mstar), angle_between(refined[0][0], Mstar)
    print("minimize, boxes %s: start %.2f deg from M*, descent %.2f deg (score %.4f, t %s), best of the 5 deg lattice %.2f deg "
          "(score %.4f); source score %.4f" % (Ls, a0, a1, score, tt, a2, refined[0][2], float(source[0, 0, 0, 0])))
    assert Rm.dtype == np.float64 and Rm.shape == (3, 3) and np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and n == 0
    assert score <= float(source[0, 0, 0, 0])                            # (a)
    assert a1 < a0                                                       # (b)
    assert a1 < a2                                                       # (c)
    assert score <= refined[0][2]                                        # (d)
    assert float(dk.score_poses(rec, lig, Rm[None], [tt])[0, 0, 0, 0]) == score          # the list's score is score_poses' own
    # (e) a clash mask over the whole window: forbidden volumes of ones correlate to (L - |t|)^3 > threshold everywhere
    ones = torch.ones(L, L, L)
    dk.docking_model.threshold_clash = 1.0
    masked = dk.minimize(rec, lig, ones, ones, poses=[(1, 1, 2 * L - 1, 0, 0.0)], steps=steps)
    assert len(masked) == 1 and masked[0][0].tobytes() == R[1].astype(np.float64).tobytes()
    assert masked[0][1] == (1, -1, 0) and masked[0][2] == 0.0 and masked[0][3] == 0
    dk.docking_model.threshold_clash = 1e30
    # the same descent with a clash channel that never bites (stored volume, and a provider of per-pose volumes in batches)
    free = dk.minimize(rec, lig, ones, ones, poses=poses, steps=steps)
    assert free[0][0].tobytes() == Rm.tobytes() and free[0][1:] == (tt, score, 0)
    calls = []

    def provider(Rb):
        calls.append(Rb.shape[0])
        return ones.to(Rb.device)[None, None].expand(Rb.shape[0], -1, -1, -1, -1).contiguous()
    prov = dk.minimize(rec, lig, ones, None, clash_provider=provider, poses=poses + poses, steps=2)
    assert len(prov) == 2 and prov[0][0].tobytes() == prov[1][0].tobytes() and len(calls) >= 3
    # (f) the .dat round trip through the consumer
    dk.refined_list = got
    dk.new_log(str(tmp_path / "P1.dat"))
    dk.write_refined_conformations()
    dk.cleanup()
    confs = DockerParser(str(tmp_path), coords_backend=object()).parse_output("P1")["conformations"]
    assert len(confs) == 1 and np.abs(confs[0][0][0].numpy() - Rm).max() < 1e-6 and abs(confs[0][2] - score) < 1e-6 * max(1.0, abs(score))
    return a0, a1, a2
