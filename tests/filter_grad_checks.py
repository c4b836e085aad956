"""Check bodies of the differentiable grid filter (csrc/dlpd_filter_grad.h, ops.filter_volumes_autograd,
GlobalDockingModel(fused_filter_grad=True)), shared by tests/test_filter_grad_emu.py (the kernel sources on the fibre emulator)
and tests/test_filter_grad_gpu.py (the gfx950 build).

Truth and tolerance.  ``restatement`` is the module path in plain torch on the CPU -- interpolate, cat, permute, matmul, relu,
matmul -- under torch autograd.  In float64 it is the truth; in float32 it is the oracle of ``accuracy_checks.yardstick``: the
kernel may sit no further from float64 than the float32 restatement does, times 2 (RMS) and 3 (max), the project's standing
rule and no number of this file's own.  The exact case needs no tolerance: its inputs are dyadic, every product and every
partial sum in any order is exact in float32, and the kernel must give the float64 bits.

ReLU's derivative jumps at pre = 0, so in the random case the voxels where some |pre_j| (float64) lies below
``BAND`` x rms(pre) carry no incoming gradient: g is set to zero there BEFORE the kernel is called, so their contribution
vanishes on all three sides, for the parameter gradients too.  At most ``CAP`` of the voxels may be left out.
"""
import torch

import corr_grad_checks as cg
from accuracy_checks import yardstick

BAND, CAP = 1e-4, 0.01
NAMES = ("gconv0", "gconv1", "gW1", "gb1", "gW2", "gb2")

# (B, C0, C1, H, N0, N1); N1 = 0: one resolution
EXACT_SHAPES = [(2, 3, 5, 4, 16, 8),        # the vectorised forward, s = 2
                (1, 2, 2, 3, 10, 5),        # N0 not a multiple of 4, H not a compiled width
                (1, 3, 2, 4, 12, 12),       # s = 1
                (2, 9, 0, 8, 20, 0),        # one resolution, C0 not a multiple of 8, voxels not a multiple of a tile
                (1, 3, 18, 33, 8, 4),       # three hidden tiles, two coarse channel tiles: the kernel's wide instantiation
                (1, 100, 28, 64, 4, 2)]     # the widest filter: 128 channels, H = 64, every gW1 tile a wave can own, 143 KB of LDS
RANDOM_SHAPES = [(2, 3, 5, 4, 16, 8), (1, 16, 32, 24, 32, 16), (1, 2, 2, 3, 10, 5), (1, 3, 18, 33, 8, 4)]
RANDOM_SHAPE_GPU = (1, 2, 2, 4, 64, 32)     # 262 K voxels: the cross-block reduction and the grid-stride loop


def restatement(convs, params, g, dtype):
    """The module path in ``dtype`` on the CPU -> (V, [gconv0, (gconv1,) gW1, gb1, gW2, gb2], pre)."""
    convs = [c.detach().cpu().to(dtype).requires_grad_() for c in convs]
    W1, b1, W2, b2 = (p.detach().cpu().to(dtype).requires_grad_() for p in params)
    B, N = convs[0].shape[0], convs[0].shape[2]
    same = [c if c.shape[2] == N else torch.nn.functional.interpolate(c, size=(N, N, N)) for c in convs]
    rows = torch.cat(same, dim=1).permute(0, 2, 3, 4, 1).reshape(B * N * N * N, -1)
    pre = torch.matmul(rows, W1.t()) + b1
    V = (torch.matmul(torch.relu(pre), W2.t()) + b2).reshape(B, N, N, N)
    grads = torch.autograd.grad(V, convs + [W1, b1, W2, b2], g.detach().cpu().to(dtype))
    return V.detach(), [t.detach() for t in grads], pre.detach()


def kernel(lib, device, convs, params, g, inputs=True, parameters=True):
    """ops.filter_volumes_autograd and autograd -> (V, gradients in the order of ``restatement``; None where not asked for)."""
    from deeplocalproteindocking_amd import ops
    cs = [c.detach().clone().to(device).requires_grad_(inputs) for c in convs]
    ps = [p.detach().clone().to(device).requires_grad_(parameters) for p in params]
    V = ops.filter_volumes_autograd(cs, *ps, lib=lib)
    V.backward(g.to(device))
    return V.detach().cpu(), [None if t.grad is None else t.grad.cpu() for t in cs + ps]


def _names(convs):
    return NAMES if len(convs) == 2 else (NAMES[0],) + NAMES[2:]


def exact_inputs(shape, seed=0):
    """conv in {-1, -0.75, .., 1}; W1, W2, g in {-1, -0.5, 0, 0.5, 1}; b1 an odd multiple of 1/16 (pre is never 0)."""
    B, C0, C1, H, N0, N1 = shape
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *size: torch.randint(lo, hi, size, generator=gen).float()      # noqa: E731
    convs = [ri(-4, 5, B, C0, N0, N0, N0) / 4] + ([ri(-4, 5, B, C1, N1, N1, N1) / 4] if C1 else [])
    params = [ri(-2, 3, H, C0 + C1) / 2, (2 * ri(-4, 4, H) + 1) / 16, ri(-2, 3, 1, H) / 2, torch.tensor([0.25])]
    return convs, params, ri(-2, 3, B, N0, N0, N0) / 2


def random_inputs(shape, seed=1):
    """Normal volumes and g, Xavier weights, b1 uniform in +-0.5."""
    B, C0, C1, H, N0, N1 = shape
    gen = torch.Generator().manual_seed(seed)
    convs = [torch.randn(B, C0, N0, N0, N0, generator=gen)] + ([torch.randn(B, C1, N1, N1, N1, generator=gen)] if C1 else [])
    C = C0 + C1
    xavier = lambda o, i: (torch.rand(o, i, generator=gen) * 2 - 1) * (6.0 / (i + o)) ** 0.5      # noqa: E731
    params = [xavier(H, C), torch.rand(H, generator=gen) - 0.5, xavier(1, H), torch.rand(1, generator=gen) - 0.5]
    return convs, params, torch.randn(B, N0, N0, N0, generator=gen)


def check_exact(lib, device, shape):
    """Dyadic inputs: float32 and float64 restatements agree exactly; then the kernel equals float64 bit for bit."""
    convs, params, g = exact_inputs(shape)
    V64, g64, pre = restatement(convs, params, g, torch.float64)
    V32, g32, _ = restatement(convs, params, g, torch.float32)
    assert float(pre.abs().min()) >= 1.0 / 16
    print("exact case %s: %.0f %% of the hidden units active" % (shape, 100 * float((pre > 0).double().mean())))
    assert torch.equal(V32.double(), V64)
    for name, a, b in zip(_names(convs), g32, g64):
        assert torch.equal(a.double(), b), name
    V, got = kernel(lib, device, convs, params, g)
    assert torch.equal(V.double(), V64), "forward"
    for name, k, b in zip(_names(convs), got, g64):
        assert k.dtype == torch.float32 and k.shape == b.shape, name
        assert torch.equal(k.double(), b), (name, float((k.double() - b).abs().max()))


def check_random(lib, device, shape):
    """Random inputs through the yardstick: one call per output (gconv0, gconv1, the concatenated parameter gradients)."""
    convs, params, g = random_inputs(shape)
    B, N0 = shape[0], shape[4]
    _, _, pre = restatement(convs, params, torch.zeros_like(g), torch.float64)
    band = BAND * float(pre.pow(2).mean().sqrt())
    near = (pre.abs() < band).any(dim=1).reshape(B, N0, N0, N0)
    frac = float(near.double().mean())
    print("random case %s: %.4f %% of the voxels lie in the band and carry no gradient" % (shape, 100 * frac))
    assert frac <= CAP
    g = g * (~near).float()
    _, g64, _ = restatement(convs, params, g, torch.float64)
    _, g32, _ = restatement(convs, params, g, torch.float32)
    _, got = kernel(lib, device, convs, params, g)
    nin = len(convs)
    for i in range(nin):
        yardstick("filter backward %s, %s" % (shape, _names(convs)[i]), got[i], g32[i], g64[i])
    cat = lambda ts: torch.cat([t.double().reshape(-1) for t in ts])      # noqa: E731
    yardstick("filter backward %s, parameter gradients" % (shape,), cat(got[nin:]), cat(g32[nin:]), cat(g64[nin:]))


def check_surface(lib, device, shape=(2, 3, 5, 4, 8, 4)):
    """The forward's bits are filter_volumes'; two backward calls give equal bits; only the requested gradients are computed;
    a non-contiguous incoming gradient is accepted."""
    from deeplocalproteindocking_amd import ops
    convs, params, g = random_inputs(shape, seed=4)
    dconvs, dparams, gd = [c.to(device) for c in convs], [p.to(device) for p in params], g.to(device)
    plain = ops.filter_volumes(dconvs, dparams[0], dparams[1], dparams[2], float(dparams[3][0]), lib=lib)
    cs, ps = [c.clone().requires_grad_() for c in dconvs], [p.clone().requires_grad_() for p in dparams]
    V = ops.filter_volumes_autograd(cs, *ps, lib=lib)
    assert V.grad_fn is not None and V.shape == plain.shape and torch.equal(V.detach(), plain)
    first = torch.autograd.grad(V, cs + ps, gd, retain_graph=True)
    again = torch.autograd.grad(V, cs + ps, gd)
    for name, a, b in zip(NAMES, first, again):
        assert torch.equal(a, b), name                                  # no atomics: the same bits
    for t, a in zip(cs + ps, first):
        assert a.shape == t.shape and a.dtype == t.dtype
    # parameters frozen / inputs detached / one volume only: null pointers for what is not asked for, the same bits for the rest
    for inputs, parameters in ((True, False), (False, True)):
        rec = cg.Recorder(lib)
        cs = [c.clone().requires_grad_(inputs) for c in dconvs]
        ps = [p.clone().requires_grad_(parameters) for p in dparams]
        ops.filter_volumes_autograd(cs, *ps, lib=rec).backward(gd)
        calls = [args for name, args in rec.calls if name == "dlpd_filter_grad"]
        assert len(calls) == 1                                          # (g, conv0, C0, N0, conv1, C1, N1, W1t, b1, W2, H, gconv0, gconv1, gparams, ws, ..)
        assert (calls[0][11] != 0) == inputs and (calls[0][12] != 0) == inputs
        assert (calls[0][13] != 0) == parameters and (calls[0][14] != 0) == parameters
        for t, a in zip(cs + ps, first):
            assert (t.grad is None) if not t.requires_grad else torch.equal(t.grad, a)
    rec = cg.Recorder(lib)
    cs = [dconvs[0].clone(), dconvs[1].clone().requires_grad_()]
    ops.filter_volumes_autograd(cs, *dparams, lib=rec).backward(gd)
    args = [a for name, a in rec.calls if name == "dlpd_filter_grad"][0]
    assert args[11] == 0 and args[12] != 0 and args[13] == 0
    assert cs[0].grad is None and torch.equal(cs[1].grad, first[1])
    # V.sum().backward() hands in an expanded gradient; a transposed one is not contiguous either
    x = dconvs[0].clone().requires_grad_()
    V = ops.filter_volumes_autograd([x, dconvs[1]], *dparams, lib=lib)
    gt = gd.transpose(1, 3)
    assert not gt.is_contiguous()
    got = torch.autograd.grad(V, [x], gt)[0]
    x2 = dconvs[0].clone().requires_grad_()
    want = torch.autograd.grad(ops.filter_volumes_autograd([x2, dconvs[1]], *dparams, lib=lib), [x2], gt.contiguous())[0]
    assert torch.equal(got, want)
    x = dconvs[0].clone().requires_grad_()
    ops.filter_volumes_autograd([x, dconvs[1]], *dparams, lib=lib).sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


def check_unsupported(lib, device):
    """s = 4 and H = 65: the library says no, the operator raises, the model calls the module."""
    import pytest
    from deeplocalproteindocking_amd import ops
    assert lib.call("dlpd_filter_grad_supported", 3, 16, 5, 8, 4) == 1 and lib.call("dlpd_filter_grad_supported", 2, 10, 0, 0, 3) == 1
    assert lib.call("dlpd_filter_grad_supported", 3, 16, 5, 4, 4) == 0          # s = 4
    assert lib.call("dlpd_filter_grad_supported", 3, 16, 0, 0, 65) == 0         # H = 65
    assert lib.call("dlpd_filter_grad_supported", 3, 15, 2, 7, 4) == 0          # N0 odd with a coarse grid
    assert lib.call("dlpd_filter_grad_supported", 100, 16, 29, 8, 4) == 0       # more than 128 channels
    assert lib.call("dlpd_filter_grad_supported", 3, 15, 2, 15, 64) == 1
    assert lib.call("dlpd_filter_grad_ws_bytes", 3, 16, 5, 4, 4, 1) == 0
    assert lib.call("dlpd_filter_grad_ws_bytes", 3, 16, 5, 8, 4, 2) == 128 * (8 * 4 + 2 * 4 + 1) * 4      # 2 x 8 x 8 x 1 tiles
    buf = torch.zeros(1 << 14, dtype=torch.float32, device=device)     # (never reached: every call below returns before a launch)
    p = buf.data_ptr()
    fg = lib._dlpd_filter_grad
    assert fg(p, p, 3, 16, p, 5, 4, p, p, p, 4, p, p, p, p, 1, None) == 2
    assert fg(p, p, 3, 16, None, 0, 0, p, p, p, 65, p, None, p, p, 1, None) == 2
    assert fg(None, p, 3, 16, p, 5, 8, p, p, p, 4, p, p, p, p, 1, None) == 1
    assert fg(p, p, 3, 16, p, 5, 8, p, p, p, 4, None, None, None, None, 1, None) == 1       # nothing asked for
    assert fg(p, p, 3, 16, p, 5, 8, p, p, p, 4, None, None, p, None, 1, None) == 1          # parameters without the workspace
    assert fg(p, p, 3, 16, None, 5, 8, p, p, p, 4, p, None, None, None, 1, None) == 1       # coarse channels without conv1
    assert fg(p, p, 3, 16, p, 5, 8, p, p, p, 4, p, p, p, p, 0, None) == 1
    gen = torch.Generator().manual_seed(2)
    c0, c1 = torch.randn(1, 2, 8, 8, 8, generator=gen).to(device), torch.randn(1, 2, 2, 2, 2, generator=gen).to(device)
    W1, b1, W2, b2 = (torch.randn(2, 4), torch.randn(2), torch.randn(1, 2), torch.randn(1))
    with pytest.raises(RuntimeError, match="no filter backward kernel"):
        ops.filter_volumes_autograd([c0, c1], W1.requires_grad_(), b1, W2, b2, lib=lib)
    with pytest.raises(RuntimeError, match="no filter backward kernel"):
        ops.filter_volumes_autograd([c0], torch.randn(65, 2).requires_grad_(), torch.randn(65), torch.randn(1, 65), b2, lib=lib)

    # the model: a filter wider than the kernel (130 channels -> hidden 65) is called as a module, as with the flag off
    from deeplocalproteindocking_amd.Models import GlobalDockingModel, SimpleFilter
    torch.manual_seed(3)
    filt = SimpleFilter([130])
    assert filt.fc[0].out_features == 65
    rec_lib = cg.Recorder(lib)
    model = GlobalDockingModel(None, filt, clip=None, lib=rec_lib, differentiable=True, fused_filter_grad=True).to(device)
    model.convolve.embed = False
    rv, lv = torch.rand(1, 130, 2, 2, 2, generator=gen).to(device), torch.rand(1, 130, 2, 2, 2, generator=gen).to(device)
    out = model([rv], [lv])
    assert out.grad_fn is not None and "FilterVolumes" not in type(out.grad_fn).__name__
    out.sum().backward()
    assert filt.fc[0].weight.grad is not None
    assert not [1 for name, _ in rec_lib.calls if name in ("dlpd_filter_grad", "dlpd_filter_mask")]


def _module_scores(model, rec, lig):
    """The graph branch of the parent's forward, spelled out: correlations, interpolate, cat, permute, the filter module."""
    rv, lv = model.representation(rec), model.representation(lig)
    corr = [model.convolve(a, b) for a, b in zip(rv, lv)]
    B, N = corr[0].shape[0], corr[0].shape[2]
    same = [c if c.shape[2] == N else torch.nn.functional.interpolate(c, size=(N, N, N)) for c in corr]
    V = torch.cat(same, dim=1).permute(0, 2, 3, 4, 1).reshape(B * N * N * N, -1)
    return model.filter(V).reshape(B, N, N, N)


def check_model(lib, device, L=32, channels=2, embed=True):
    """GlobalDockingModel(differentiable=True) with fused_filter_grad set: parameter gradients against the float64 restatement
    of the whole model (the float32 one as the oracle), scores equal to the no_grad fused path bit for bit; with the flag off
    the graph and the bits of the module path."""
    import inspect
    from deeplocalproteindocking_amd.Models import GlobalDockingModel
    sig = inspect.signature(GlobalDockingModel.__init__).parameters
    assert list(sig)[-1] == "fused_filter_grad" and sig["fused_filter_grad"].default is False
    rec_lib = cg.Recorder(lib)
    model, rec, lig, target = cg.make_model(rec_lib, device, L, True, channels=channels, embed=embed)
    assert model.fused_filter_grad is False
    # flag off: the module path, no filter kernel in the graph
    loss0, scores0 = cg.model_loss(model, rec, lig, target)
    assert "FilterVolumes" not in type(scores0.grad_fn).__name__
    assert not [1 for name, _ in rec_lib.calls if name in ("dlpd_filter_grad", "dlpd_filter_mask")]
    assert torch.equal(scores0.detach(), _module_scores(model, rec, lig).detach())
    params = list(model.representation.parameters()) + list(model.filter.parameters())
    # flag on
    model.fused_filter_grad = True                                      # a public attribute
    loss, scores = cg.model_loss(model, rec, lig, target)
    assert scores.shape == (1, 2 * L, 2 * L, 2 * L) and "FilterVolumes" in type(scores.grad_fn).__name__
    got = torch.autograd.grad(loss, params)
    assert len([1 for name, _ in rec_lib.calls if name == "dlpd_filter_grad"]) == 1
    with torch.no_grad():
        fused = model(model.representation(rec), model.representation(lig))
    assert fused.grad_fn is None and torch.equal(fused, scores.detach())
    l64, g64 = cg._restatement(model.representation, model.filter, rec, lig, target, torch.float64)
    l32, g32 = cg._restatement(model.representation, model.filter, rec, lig, target, torch.float32)
    assert abs(float(loss.detach()) - float(l64)) <= 1e-5 * abs(float(l64))
    cat = lambda gs: torch.cat([t.detach().cpu().double().reshape(-1) for t in gs])      # noqa: E731
    yardstick("GlobalDockingModel(fused_filter_grad=True) box %d + %d, parameter gradients" % (L, L // 2), cat(got), cat(g32), cat(g64))
    # differentiable=False: the inference path, whatever the new flag says
    model.differentiable = False
    out = model(model.representation(rec), model.representation(lig))
    assert out.grad_fn is None and torch.equal(out, fused)
