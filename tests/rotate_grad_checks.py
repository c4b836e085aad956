"""Check bodies shared by tests/test_rotate_grad_emu.py (the kernel sources on the fibre emulator) and
tests/test_rotate_grad_gpu.py (the gfx950 build): the adjoint of the trilinear rotation (csrc/dlpd_rotate_grad.h), the
differentiable ops.VolumeRotation, ops.local_correlate_rotated and LocalDockingModel.forward_poses.

The expectation is the SCATTER definition of the adjoint in numpy float64 -- the sample position p(i) = c0 + (i - c0) M in
float64, its eight corners, corners outside the box dropped, every (weight * g) added to its corner with np.bincount --
independent of the kernel, which gathers over the output voxels that can reach a source voxel.

Tolerances (derived):
  kernel vs float64   |got - want| <= 2 (K + 1) 2^-24 sum|w g| + 1e-4 max|want|: an element is an f32 sum of at most K products
                      in some order (K the largest number of terms any element collects, counted by the expectation; times B
                      where one gradient collects every rotation); the 1e-4 term is the repository's band for an f32 rotated
                      sample (its weights come from an f32 position), as local_grad_checks uses it.
  transpose identity  |<Rot v, g> - <v, Adj g>| <= (148 + 6 L) 2^-24 <Rot |v|, |g|>: 9 + 65 rounding steps per side, doubled,
                      plus one ulp (of a coordinate up to L) of the sample position per axis -- the compiler may contract the
                      two kernels' position arithmetic differently.
  local_correlate_rotated: the two bounds of the correlation's adjoint (local_grad_checks) and of the rotation's combined: the
                      ligand's gradient is a nested f32 sum of K_rot * W^3 products."""
import functools
import itertools

import numpy as np
import torch

import local_grad_checks as lg

TOL = lg.TOL
EPS = lg.EPS


def _ptr(t):
    return t.data_ptr()


def _stream(dev):
    return lg._stream(dev)


# ----------------------------------------------------------------------------------------------------------------------
# float64: the forward's weights, the scatter (adjoint) and the gather (forward)
# ----------------------------------------------------------------------------------------------------------------------

def corners64(M, c0, L):
    """For every output voxel i (flat, z fastest) of the map M (3, 3): flat source index (8, L^3), weight (8, L^3), in-box
    (8, L^3) of the eight corners of p(i) = c0 + (i - c0) M  (p_a = c0 + sum_b M[b][a] (i_b - c0): k_rotate's expression)."""
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    ar = np.arange(L, dtype=np.float64) - c0
    d = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), axis=-1).reshape(-1, 3)
    p = c0 + d @ M
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


def scatter64(g, M, c0):
    """g (C, L, L, L) float64 -> (adjoint (C, L, L, L), the sum of |terms|, terms per element (L, L, L))."""
    C, L = g.shape[0], g.shape[-1]
    idx, w, ok = corners64(M, c0, L)
    sel = ok & (w != 0)
    cnt = np.bincount(idx[sel], minlength=L ** 3)
    out, mag = np.zeros((C, L ** 3)), np.zeros((C, L ** 3))
    for c in range(C):
        t = w * g[c].reshape(1, -1)
        out[c] = np.bincount(idx[sel], weights=t[sel], minlength=L ** 3)
        mag[c] = np.bincount(idx[sel], weights=np.abs(t[sel]), minlength=L ** 3)
    return out.reshape(g.shape), mag.reshape(g.shape), cnt.reshape(L, L, L)


def rotate64(v, M, c0):
    """The forward in float64: v (C, L, L, L) -> (C, L, L, L)."""
    C, L = v.shape[0], v.shape[-1]
    idx, w, ok = corners64(M, c0, L)
    flat = v.reshape(C, -1)
    return sum(flat[:, idx[k]] * (w[k] * ok[k])[None, :] for k in range(8)).reshape(v.shape)


@functools.lru_cache(maxsize=None)
def case(L, C, B, seed=0, center=None):
    """Inputs and the float64 expectation of one shape, computed once and shared by the checks that need it (read only)."""
    g_ = torch.Generator().manual_seed(7000 * L + 10 * C + B + seed)
    g = torch.randn(B, C, L, L, L, generator=g_)
    v = torch.randn(B, C, L, L, L, generator=g_)
    R = torch.from_numpy(lg.rots(B, seed=seed + L)).float().contiguous()
    c0 = float(L) / 2.0 if center is None else float(center)
    want, mag = np.zeros((B, C, L, L, L)), np.zeros((B, C, L, L, L))
    cnt = np.zeros((B, L, L, L), dtype=np.int64)
    for b in range(B):
        want[b], mag[b], cnt[b] = scatter64(g[b].numpy().astype(np.float64), R[b].numpy(), c0)
    for a in (want, mag, cnt):
        a.setflags(write=False)
    return g, v, R, c0, want, mag, cnt


def adjoint(lib, dev, g, R, L, C, B, stride, c0, accumulate=0, out=None):
    """dlpd_rotate_trilinear_grad; the output starts as NaN (every element must be written)."""
    if out is None:
        out = torch.full((B if stride else 1, C, L, L, L), float("nan"), dtype=torch.float32, device=dev)
    lib.call("dlpd_rotate_trilinear_grad", _ptr(g), _ptr(R), _ptr(out), B, C, L, stride, c0, accumulate, _stream(dev))
    return out


def rotate(lib, dev, v, R, L, C, B, stride, c0):
    out = torch.full((B, C, L, L, L), float("nan"), dtype=torch.float32, device=dev)
    lib.call("dlpd_rotate_trilinear", _ptr(v), _ptr(R), _ptr(out), B, C, L, stride, c0, _stream(dev))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# 1, 2: the kernel against float64, and against the forward kernel (transpose identity)
# ----------------------------------------------------------------------------------------------------------------------

def check_kernel(lib, device, L, C, B, summed, seed=0):
    dev = torch.device(device)
    g, _, R, c0, want, mag, cnt = case(L, C, B, seed)
    d_g, d_R = g.to(dev).contiguous(), R.to(dev).contiguous()
    stride = 0 if summed else C * L ** 3
    got = adjoint(lib, dev, d_g, d_R, L, C, B, stride, c0).cpu().numpy()
    again = adjoint(lib, dev, d_g, d_R, L, C, B, stride, c0).cpu().numpy()
    assert got.tobytes() == again.tobytes(), "fixed summation order: the same bits run to run"
    assert not np.isnan(got).any(), "every element is written"
    if summed:
        w64, m64, K = want.sum(axis=0, keepdims=True), mag.sum(axis=0, keepdims=True), int(cnt.max()) * B
    else:
        w64, m64, K = want, mag, int(cnt.max())
    frac = float((w64 != 0).mean())
    assert frac >= 0.5, ("at least half of the expected elements must be non-zero", frac)
    bound = 2 * (K + 1) * EPS * m64 + TOL * np.abs(w64).max()
    err = np.abs(got - w64)
    print("rotate_trilinear_grad L=%d C=%d B=%d%s: non-zero %.2f, K=%d, worst error %.3g of max|want|" %
          (L, C, B, ", summed" if summed else "", frac, K, err.max() / np.abs(w64).max()))
    assert (err <= bound).all(), (float((err - bound).max()), float(np.abs(w64).max()))


def check_transpose(lib, device, L, C, B, summed, seed=0):
    """<Rot v, g> = <v, Adj g> with the forward KERNEL on the other side, the dot products in float64 over the kernels'
    float32 outputs.  summed: one v for all B rotations (the forward's stride 0) against the adjoint's sum over b."""
    dev = torch.device(device)
    g, v, R, c0, _, _, _ = case(L, C, B, seed)
    if summed:
        v = v[:1]
    d_g, d_v, d_R = g.to(dev).contiguous(), v.to(dev).contiguous(), R.to(dev).contiguous()
    stride = 0 if summed else C * L ** 3
    rot = rotate(lib, dev, d_v, d_R, L, C, B, stride, c0).cpu().double()
    rot_abs = rotate(lib, dev, d_v.abs().contiguous(), d_R, L, C, B, stride, c0).cpu().double()
    adj = adjoint(lib, dev, d_g, d_R, L, C, B, stride, c0).cpu().double()
    lhs, rhs = float((rot * g.double()).sum()), float((v.double() * adj).sum())
    bound = (148 + 6 * L) * EPS * float((rot_abs * g.double().abs()).sum())
    print("transpose identity L=%d C=%d B=%d%s: <Rot v, g> %.9g, <v, Adj g> %.9g, difference %.3g, bound %.3g" %
          (L, C, B, ", summed" if summed else "", lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 0 and abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ----------------------------------------------------------------------------------------------------------------------
# 3: exact cases
# ----------------------------------------------------------------------------------------------------------------------

def check_exact(lib, device, L, C=2):
    """Identity: Adj g is g, bit for bit.  The 24 signed permutations: Adj_R g is dlpd_rotate_trilinear of g with R^T, bit
    for bit -- both are one index permutation, with zeros where the index leaves the box (pivot L / 2: index L is outside)."""
    from accuracy_checks import signed_permutations
    dev = torch.device(device)
    perms = signed_permutations()
    B = len(perms)
    g = torch.randn(B, C, L, L, L, generator=torch.Generator().manual_seed(L)).to(dev)
    c0, stride = float(L) / 2.0, C * L ** 3
    eye = torch.eye(3).reshape(1, 3, 3).repeat(B, 1, 1).contiguous().to(dev)
    assert adjoint(lib, dev, g, eye, L, C, B, stride, c0).cpu().numpy().tobytes() == g.cpu().numpy().tobytes()
    R = torch.from_numpy(perms).float().contiguous().to(dev)
    Rt = R.transpose(1, 2).contiguous()
    adj = adjoint(lib, dev, g, R, L, C, B, stride, c0).cpu().numpy()
    fwd = rotate(lib, dev, g, Rt, L, C, B, stride, c0).cpu().numpy()
    # (where the index leaves the box the forward kernel adds eight products value * 0 of clamped neighbours: its zero is -0.0
    # when they are all negative; the adjoint's empty sum is +0.0.  "+ 0.0" makes every zero +0.0 and changes no other bit.)
    assert not np.signbit(adj[adj == 0]).any()
    assert adj.tobytes() == (fwd + np.float32(0.0)).tobytes()
    assert (adj == 0).any() and (adj != 0).mean() > 0.5
    # the summed form of the identity: B copies of one value added in order -- what a float32 running sum gives
    acc = np.zeros((1, C, L, L, L), dtype=np.float32)
    for b in range(B):
        acc = acc + g[b:b + 1].cpu().numpy()
    assert adjoint(lib, dev, g, eye, L, C, B, 0, c0).cpu().numpy().tobytes() == acc.tobytes()


def check_singular(lib, device, L=6, C=2):
    """A map that is not invertible (and one full of zeros): the bounds are not finite, the kernel walks the whole box --
    still the scatter definition, no hang, nothing read outside."""
    dev = torch.device(device)
    g = torch.randn(2, C, L, L, L, generator=torch.Generator().manual_seed(5))
    R = torch.tensor([[[1.0, 0.5, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[0.0] * 3] * 3]).contiguous()
    c0 = float(L) / 2.0
    got = adjoint(lib, dev, g.to(dev), R.to(dev), L, C, 2, C * L ** 3, c0).cpu().numpy()
    for b in range(2):
        want, mag, cnt = scatter64(g[b].numpy().astype(np.float64), R[b].numpy(), c0)
        assert np.abs(want).max() > 0
        assert (np.abs(got[b] - want) <= 2 * (int(cnt.max()) + 1) * EPS * mag + TOL * np.abs(want).max()).all()


# ----------------------------------------------------------------------------------------------------------------------
# 4: chunking
# ----------------------------------------------------------------------------------------------------------------------

def check_accumulate(lib, device, L=9, C=3):
    """At the ABI: B = 5 in one call equals 2 + 3 with accumulate, bit for bit (the summed form)."""
    dev = torch.device(device)
    g, _, R, c0, _, _, _ = case(L, C, 5)
    d_g, d_R = g.to(dev).contiguous(), R.to(dev).contiguous()
    one = adjoint(lib, dev, d_g, d_R, L, C, 5, 0, c0)
    two = adjoint(lib, dev, d_g[:2].contiguous(), d_R[:2].contiguous(), L, C, 2, 0, c0)
    two = adjoint(lib, dev, d_g[2:].contiguous(), d_R[2:].contiguous(), L, C, 3, 0, c0, accumulate=1, out=two)
    assert one.cpu().numpy().tobytes() == two.cpu().numpy().tobytes() and float(one.abs().max()) > 0


def check_backward_split(lib, device):
    """13 poses through ops.local_correlate_rotated with a library wrapper that answers 5 to dlpd_local_max_poses (the idea of
    local_grad_checks.check_backward_split): chunks of 5, 5 and 3; the gradients have the bits of the unsplit call, for a
    ligand shared by the poses (accumulate from the second chunk on) and for one ligand per pose."""
    from deeplocalproteindocking_amd import ops

    class Limited:
        def call(self, name, *args):
            return 5 if name == "dlpd_local_max_poses" else lib.call(name, *args)
    L, C, P = 8, 2, 13
    dev = torch.device(device)
    g_ = torch.Generator().manual_seed(2)
    T = torch.randint(-2, 3, (P, 3), generator=g_).int().to(dev)
    R = torch.from_numpy(lg.rots(P, seed=4)).float().contiguous().to(dev)
    gout = torch.randn(P, C, 3, 3, 3, generator=g_).to(dev)
    for nv in ((), (P,)):
        rec, lig = torch.randn(*nv, C, L, L, L, generator=g_).to(dev), torch.randn(*nv, C, L, L, L, generator=g_).to(dev)
        res = []
        for lib_ in (Limited(), lib):
            a, b = rec.clone().requires_grad_(), lig.clone().requires_grad_()
            ops.local_correlate_rotated(a, b, T, R, radius=1, lib=lib_).backward(gout)
            res.append((a.grad.cpu().numpy(), b.grad.cpu().numpy()))
        assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()
        assert np.abs(res[0][0]).max() > 0 and np.abs(res[0][1]).max() > 0 and res[0][1].shape == tuple(lig.shape)


# ----------------------------------------------------------------------------------------------------------------------
# 5: errors and the autograd surface of VolumeRotation
# ----------------------------------------------------------------------------------------------------------------------

def check_errors(lib, device):
    import pytest
    dev = torch.device(device)
    x = torch.zeros(8 ** 3, device=dev)
    R = torch.eye(3, device=dev).reshape(1, 9).contiguous()
    p, r = x.data_ptr(), R.data_ptr()

    def call(gout=p, Rm=r, gvol=p, B=1, C=1, L=8, stride=0):
        return lib.call("dlpd_rotate_trilinear_grad", gout, Rm, gvol, B, C, L, stride, L / 2.0, 0, _stream(dev))
    for kw in (dict(gout=None), dict(Rm=None), dict(gvol=None), dict(B=0), dict(C=0), dict(C=-1), dict(stride=-1)):
        with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
            call(**kw)
    for L in (1, 129):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            call(L=L)                                                    # (refused before anything is read)
    assert call() == 0 and call(stride=512) == 0


def check_volume_rotation_autograd(lib, device, L=9, C=3, B=4, **conv):
    """ops.VolumeRotation under autograd, with the conventions ``conv`` (folded into the kernel's maps before the Function:
    the backward uses the same maps)."""
    import pytest
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.Utils.Conventions import kernel_matrices, rotation_scale
    dev = torch.device(device)
    g_ = torch.Generator().manual_seed(31 + L)
    vol, gout = torch.randn(B, C, L, L, L, generator=g_).to(dev), torch.randn(B, C, L, L, L, generator=g_).to(dev)
    R = torch.from_numpy(lg.rots(B, seed=L)).float().contiguous().to(dev)
    op = ops.VolumeRotation(lib=lib, **conv)
    c0 = float(L) / 2.0 if conv.get("center") is None else float(conv["center"])
    M = kernel_matrices(R, rotation_scale(conv.get("scale"), L), conv.get("axis_order", "xyz"), conv.get("transpose", False))
    plain = op(vol, R)
    assert not plain.requires_grad
    a, Rg = vol.clone().requires_grad_(), R.clone().requires_grad_()
    out = op(a, Rg)
    assert out.requires_grad and out.detach().cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    out.backward(gout)
    assert Rg.grad is None and a.grad.shape == a.shape
    got = a.grad.cpu().numpy()
    for b in range(B):
        want, mag, cnt = scatter64(gout[b].cpu().numpy().astype(np.float64), M[b].cpu().numpy(), c0)
        assert float((want != 0).mean()) >= 0.5
        assert (np.abs(got[b] - want) <= 2 * (int(cnt.max()) + 1) * EPS * mag + TOL * np.abs(want).max()).all(), b
    # a gradient only when the volume asks for one; no graph under no_grad
    assert not op(vol, Rg).requires_grad
    with torch.no_grad():
        assert not op(a, R).requires_grad
    # first order only
    a2 = vol.clone().requires_grad_()
    (g1,) = torch.autograd.grad(op(a2, R).sum(), a2, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()
    # ONE (C, L, L, L) volume for all B matrices: the expanded call's bytes; its gradient the stride-0 kernel call's bytes
    s = vol[0].clone().requires_grad_()
    shared = op(s, R)
    expanded = op(vol[0:1].expand(B, -1, -1, -1, -1).contiguous(), R)
    assert shared.shape == (B, C, L, L, L) and shared.detach().cpu().numpy().tobytes() == expanded.cpu().numpy().tobytes()
    with torch.no_grad():
        assert op(vol[0], R).cpu().numpy().tobytes() == expanded.cpu().numpy().tobytes()
    shared.backward(gout)
    direct = adjoint(lib, dev, gout.contiguous(), M.contiguous(), L, C, B, 0, c0)
    assert s.grad.shape == s.shape and s.grad.cpu().numpy().tobytes() == direct[0].cpu().numpy().tobytes()
    assert float(s.grad.abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------------
# 6: local_correlate_rotated
# ----------------------------------------------------------------------------------------------------------------------

def check_local_correlate_rotated(lib, device, L, C, P, r, scale, mode, shared, seed=0):
    from deeplocalproteindocking_amd import ops
    dev = torch.device(device)
    g_ = torch.Generator().manual_seed(900 * L + 10 * r + seed)
    W = 2 * r + 1
    nv = () if shared else (P,)
    rec, lig = torch.randn(*nv, C, L, L, L, generator=g_), torch.randn(*nv, C, L, L, L, generator=g_)
    gout = torch.randn(P, C, W, W, W, generator=g_)
    T = torch.from_numpy(lg.translations(P, L, scale, seed)).int()
    R = torch.from_numpy(lg.rots(P, seed=seed + L)).float().contiguous()
    tau = lg.coarse(T.numpy(), scale, mode)
    c0 = float(L) / 2.0
    d = [t.to(dev).contiguous() for t in (rec, lig, T, R, gout)]
    kw = dict(radius=r, scale=scale, coarse=mode, lib=lib)
    plain = ops.local_correlate(d[0], d[1], d[2], R=d[3], **kw)
    assert not ops.local_correlate_rotated(d[0], d[1], d[2], d[3], **kw).requires_grad
    a, b = d[0].clone().requires_grad_(), d[1].clone().requires_grad_()
    out = ops.local_correlate_rotated(a, b, d[2], d[3], **kw)
    assert out.requires_grad and out.detach().cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    # the same value with the rotated ligand in memory
    ligp = d[1] if not shared else d[1][None].expand(P, -1, -1, -1, -1).contiguous()
    stored = ops.local_correlate(d[0], ops.VolumeRotation(lib=lib)(ligp, d[3]), d[2], **kw)
    print("local_correlate_rotated L=%d r=%d scale %d %s%s: the value %s the correlation with the stored rotated ligand" %
          (L, r, scale, mode, ", shared" if shared else "",
           "IS bit for bit" if stored.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes() else "is NOT bit for bit"))
    assert float((stored - plain).abs().max()) <= TOL * float(plain.abs().max()) and float(plain.abs().max()) > 0
    out.backward(d[4])
    # float64: the correlation's adjoint on the float64-rotated ligand, then the scatter of the rotated ligand's gradient
    want = {k: np.zeros((P, C, L, L, L)) for k in ("rec", "lig", "mrec", "mlig")}
    Krot = 0
    for p in range(P):
        v = () if shared else (p,)
        lrot = rotate64(lig[v].numpy().astype(np.float64), R[p].numpy(), c0)
        want["rec"][p], glrot, want["mrec"][p], mlrot = lg.adjoint64(rec[v].numpy().astype(np.float64), lrot,
                                                                      gout[p].numpy().astype(np.float64), tau[p], r)
        want["lig"][p], _, cnt = scatter64(glrot, R[p].numpy(), c0)
        idx, w, ok = corners64(R[p].numpy(), c0, L)
        for c in range(C):
            want["mlig"][p, c] = np.bincount(idx[ok], weights=(np.abs(w) * mlrot[c].reshape(1, -1))[ok], minlength=L ** 3).reshape(L, L, L)
        Krot = max(Krot, int(cnt.max()))
    for k, t, K in (("rec", a, W ** 3), ("lig", b, Krot * W ** 3)):
        w64, mag = (want[k].sum(axis=0), want["m" + k].sum(axis=0)) if shared else (want[k], want["m" + k])
        K = K * (P if shared else 1)
        got = t.grad.cpu().numpy()
        # (the poses that overlap well -- |tau| <= L / 4 -- must fill a quarter of the gradient: (3/4)^3 of the box overlaps,
        # less the corners a rotation leaves empty)
        small = [p for p in range(P) if (np.abs(tau[p]) <= L / 4.0).all()]
        body = want[k][small].sum(axis=0) if shared else want[k][small]
        assert got.shape == w64.shape and len(small) >= 1 and float((body != 0).mean()) >= 0.25, float((body != 0).mean())
        err = np.abs(got - w64)
        bound = 2 * (K + 1) * EPS * mag + TOL * np.abs(w64).max()
        print("local_correlate_rotated g%s L=%d r=%d%s: worst error %.3g of max|want|" %
              (k, L, r, ", shared" if shared else "", err.max() / np.abs(w64).max()))
        assert (err <= bound).all(), (k, float((err - bound).max()), float(np.abs(w64).max()))


# ----------------------------------------------------------------------------------------------------------------------
# 7: LocalDockingModel.forward_poses against the same modules in pure torch
# ----------------------------------------------------------------------------------------------------------------------

def rotate_torch(vol, M, c0):
    """Differentiable trilinear rotation written as index gathers: vol (C, L, L, L), M (P, 3, 3) in vol's dtype ->
    (P, C, L, L, L); out[p, c, i] = vol[c]( c0 + (i - c0) M_p ), zeros outside."""
    C, L = vol.shape[0], vol.shape[-1]
    ar = torch.arange(L, dtype=vol.dtype, device=vol.device) - c0
    d = torch.stack(torch.meshgrid(ar, ar, ar, indexing="ij"), dim=-1).reshape(-1, 3)
    p = c0 + d @ M                                                       # (P, L^3, 3)
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


def model_poses_torch(representation, filt, receptor, ligand, R, T):
    """forward_poses in plain torch, in the dtype of its arguments: the ligand's representation rotated P times."""
    edge, P = float(receptor.shape[2]), R.shape[0]
    feats = []
    for rv, lv in zip(representation(receptor), representation(ligand)):
        Li = rv.shape[2]
        lrot = rotate_torch(lv[0], R, float(Li) / 2.0)
        feats.append(lg.multiply_torch(rv.expand(P, -1, -1, -1, -1), lrot, T * float(Li) / edge))
    return filt(torch.cat(feats, dim=1))


def check_model_pose_gradients(label, model, receptor, ligand, R, T, device="cpu"):
    """out.sum().backward() through forward_poses (kernels) against the same modules in pure torch -- the pattern of
    local_grad_checks.check_model_gradients: float64 on the CPU is the truth, float32 pure torch on ``device`` the yardstick."""
    import copy
    from accuracy_checks import yardstick
    dev = torch.device(device)
    model = model.to(dev).train()
    model.zero_grad()
    out = model.forward_poses(receptor.to(dev), ligand.to(dev), R.to(dev), T.to(dev))
    out.sum().backward()
    names = [n for n, _ in model.named_parameters()]
    got = {n: p.grad for n, p in model.named_parameters()}
    assert all(got[n] is not None for n in names), [n for n in names if got[n] is None]
    grads = {}
    for dtype, where in ((torch.float64, torch.device("cpu")), (torch.float32, dev)):
        rep = copy.deepcopy(model.representation).to(device=where, dtype=dtype)
        filt = copy.deepcopy(model.filter).to(device=where, dtype=dtype)
        for m in (rep, filt):
            m.zero_grad()
        o = model_poses_torch(rep, filt, receptor.to(device=where, dtype=dtype), ligand.to(device=where, dtype=dtype),
                              R.to(device=where, dtype=dtype), T)
        o.sum().backward()
        grads[dtype] = {**{"representation." + n: p.grad for n, p in rep.named_parameters()},
                        **{"filter." + n: p.grad for n, p in filt.named_parameters()}}
        if dtype == torch.float64:
            out64 = o.detach()
    assert sorted(grads[torch.float64]) == sorted(names)
    for n in names:
        g64 = grads[torch.float64][n]
        assert float(g64.abs().max()) > 0, (n, "a gradient that is zero measures nothing")
        g32 = grads[torch.float32][n].detach().cpu().double()
        if torch.equal(g32, g64):          # (a last layer's bias: twice no error is no error)
            assert torch.equal(got[n].detach().cpu().double(), g64), (n, "float32 torch is exact here, the kernel path is not")
            continue
        yardstick("%s, d/d %s" % (label, n), got[n], g32, g64)
    with torch.no_grad():
        plain = model.forward_poses(receptor.to(dev), ligand.to(dev), R.to(dev), T.to(dev))
    assert not plain.requires_grad and out.requires_grad
    print("%s: no_grad against the autograd path, max difference %.3g, max|value| %.3g" %
          (label, float((plain - out.detach()).abs().max()), float(out.detach().abs().max())))
    assert float((plain - out.detach()).abs().max()) <= TOL * float(out.detach().abs().max())
    return out.detach().cpu(), out64
