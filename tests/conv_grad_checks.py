"""Check bodies of the convolution's backward (csrc/dlpd_conv_grad.h, ops.conv3d_weight_grad / conv3d_input_grad /
conv3d_autograd, the plugins' ``hip_autograd``), shared by tests/test_conv_grad_emu.py (the kernel sources on the fibre
emulator) and tests/test_conv_grad_gpu.py (the gfx950 build).

The weight gradient answers to float64 by the project's yardstick (accuracy_checks.yardstick): X64 is
torch.nn.grad.conv3d_weight in float64 on the CPU, X32 the same call in float32 on the CPU, and the kernel's error may be
at most 2 x (RMS) and 3 x (max) the float32 run's.  No growth factor: the kernel keeps one short running sum per patch (at
most 16 rows x D voxels), adds the patches of a part in float32 and the parts in float64 (EXPERIMENTS.md, CONV-GRAD).
Inputs: X non-negative and smooth (|accuracy_checks.protein_shaped|, 3^3 box mean), gY signed random.  Every reference is
computed once per case and shared by the tests that need it."""
import copy
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import accuracy_checks as ac

# (B, cin, cout, ks, D, nparts): the smallest shapes at which each thing can go wrong, on the emulator AND the device (an
# emulated case costs its number of matrix instructions: each of these takes 1-5 s there)
SMALL_CASES = [
    (2, 11, 16, 5, 9, 3),      # padded channels (11 -> 12: three chunks); D below one z tile and no multiple of the patch
    (1, 16, 32, 3, 13, 4),     # two output-channel tiles; a z tail of one voxel (13 = 3 x 4 + 1); four patches per block
    (1, 32, 32, 3, 6, 7),      # more parts than patches (4): idle parts must contribute zeros; two groups of 16 input channels
    (1, 16, 16, 5, 10, 2),     # k = 5 with all four chunks resident, 4 or 5 patches per block, patches that hang over the box
]
# on the device only, at the default nparts: the reference's boxes
LARGE_CASES = [(1, 16, 16, 3, 80, None), (1, 11, 16, 5, 80, None), (2, 16, 32, 5, 40, None), (2, 32, 32, 3, 40, None)]

_REF = {}


def smooth_nonneg(n, D, seed):
    """(n, D, D, D): non-negative, zero away from an ellipsoid, smooth (3^3 box mean)."""
    return F.avg_pool3d(ac.protein_shaped(n, D, seed, amp=1.0).abs()[None], 3, 1, 1)[0].contiguous()


def reference(B, cin, cout, ks, D):
    """x, gy, the float32 and the float64 weight gradient of torch on the CPU -- made once per shape."""
    key = (B, cin, cout, ks, D)
    if key not in _REF:
        g = torch.Generator().manual_seed(100 + 7 * cin + cout + ks + D)
        x = smooth_nonneg(B * cin, D, 11 + D).reshape(B, cin, D, D, D)
        gy = torch.randn(B, cout, D, D, D, generator=g)
        size = (cout, cin, ks, ks, ks)
        w32 = torch.nn.grad.conv3d_weight(x, size, gy, padding=ks // 2)
        w64 = torch.nn.grad.conv3d_weight(x.double(), size, gy.double(), padding=ks // 2)
        assert float(x.min()) >= 0 and float(x.max()) > 0
        _REF[key] = (x, gy, w32, w64)
    return _REF[key]


def check_weight_grad(lib, device, B, cin, cout, ks, D, nparts, where=""):
    from deeplocalproteindocking_amd import ops
    x, gy, w32, w64 = reference(B, cin, cout, ks, D)
    gw = ops.conv3d_weight_grad(x.to(device), gy.to(device), ks, lib=lib, nparts=nparts).cpu()
    assert gw.shape == w64.shape
    ac.yardstick("conv3d_weight_grad B %d, %d -> %d, k %d, D %d, nparts %s%s" % (B, cin, cout, ks, D, nparts or "default", where),
                 gw, w32, w64)
    return gw


def check_index_exactness(lib, device, ks, far):
    """X = one 1.0 per input channel at p(ci), gY = one 1.0 per output channel at q(co): gW[co, ci] is exactly 1.0 at tap
    p(ci) - q(co) + ks // 2 where that tap exists and exactly 0.0 everywhere else -- all 32 x 16 pairs of one launch at once.
    p: the corner of the box (near: (0, 0, 0); far: (5, 5, 5)) and the seven voxels next to it inwards, eight channels
    without an impulse; q: up to ks // 2 away from the corner along each axis (every combination), and offsets of
    ks // 2 + 1, which no tap reaches."""
    from deeplocalproteindocking_amd import ops
    D, cin, cout, h = 6, 16, 32, ks // 2
    corner, s = ((D - 1,) * 3, -1) if far else ((0, 0, 0), 1)
    offs = list(itertools.product(range(h + 1), repeat=3)) + [(h + 1, 0, 0), (0, h + 1, h), (h + 1, h + 1, h + 1)]
    offs = [offs[i % len(offs)] for i in range(cout)]
    q = [tuple(corner[a] + s * o[a] for a in range(3)) for o in offs]
    p = [tuple(corner[a] + s * ((ci >> a) & 1) for a in range(3)) if ci < 8 else None for ci in range(cin)]
    x, gy = torch.zeros(1, cin, D, D, D), torch.zeros(1, cout, D, D, D)
    for ci, v in enumerate(p):
        if v is not None:
            x[0, ci][v] = 1.0
    for co, v in enumerate(q):
        gy[0, co][v] = 1.0
    want = torch.zeros(cout, cin, ks, ks, ks)
    ones = zeros = 0
    for co, ci in itertools.product(range(cout), range(cin)):
        if p[ci] is None:
            continue
        t = [p[ci][a] - q[co][a] + h for a in range(3)]
        if all(0 <= v < ks for v in t):
            want[co, ci, t[0], t[1], t[2]] = 1.0
            ones += 1
        else:
            zeros += 1
    assert ones >= (h + 1) ** 3 and zeros > 0                      # (the corner pairs, and pairs no tap connects)
    gw = ops.conv3d_weight_grad(x.to(device), gy.to(device), ks, lib=lib, nparts=3).cpu()
    assert torch.equal(gw, want), (int((gw != want).sum()), float((gw - want).abs().max()))


def check_determinism(lib, device, B, cin, cout, ks, D, nparts, other):
    """Two calls: equal bits.  Another nparts: another order of the same sum -- the yardstick, not the bits."""
    from deeplocalproteindocking_amd import ops
    x, gy, w32, w64 = reference(B, cin, cout, ks, D)
    xd, gd = x.to(device), gy.to(device)
    a = ops.conv3d_weight_grad(xd, gd, ks, lib=lib, nparts=nparts).cpu()
    b = ops.conv3d_weight_grad(xd, gd, ks, lib=lib, nparts=nparts).cpu()
    assert torch.equal(a, b)
    c = ops.conv3d_weight_grad(xd, gd, ks, lib=lib, nparts=other).cpu()
    ac.yardstick("conv3d_weight_grad B %d, %d -> %d, k %d, D %d, nparts %d (after %d)" % (B, cin, cout, ks, D, other, nparts), c, w32, w64)


def check_input_grad(lib, device, B, cin, cout, ks, D, precision):
    """The forward kernel on gY with the flipped, transposed weights: its contract, 1e-5 of the largest value, against
    torch.nn.grad.conv3d_input in float64."""
    from deeplocalproteindocking_amd import ops
    g = torch.Generator().manual_seed(3 + cin + ks)
    w = torch.randn(cout, cin, ks, ks, ks, generator=g) * 0.1
    gy = torch.randn(B, cout, D, D, D, generator=g)
    want = torch.nn.grad.conv3d_input((B, cin, D, D, D), w.double(), gy.double(), padding=ks // 2)
    got = ops.conv3d_input_grad(gy.to(device), w.to(device), lib=lib, precision=precision).cpu()
    err, scale = float((got.double() - want).abs().max()), float(want.abs().max())
    print("conv3d_input_grad %s %d -> %d, k %d, D %d: max error %.2e of the largest value" % (precision, cin, cout, ks, D, err / scale))
    assert got.shape == want.shape and err <= 1e-5 * scale


def check_input_grad_refuses(lib, device, monkeypatch):
    """A layer with 11 input channels has no input-gradient kernel: an error, unless DLPD_ALLOW_TORCH_CONV=1 (then torch's,
    with a warning)."""
    import pytest
    from deeplocalproteindocking_amd import ops
    g = torch.Generator().manual_seed(5)
    w, gy = torch.randn(16, 11, 3, 3, 3, generator=g).to(device), torch.randn(1, 16, 6, 6, 6, generator=g).to(device)
    monkeypatch.delenv("DLPD_ALLOW_TORCH_CONV", raising=False)
    with pytest.raises(RuntimeError, match="has no HIP kernel"):
        ops.conv3d_input_grad(gy, w, lib=lib)
    monkeypatch.setenv("DLPD_ALLOW_TORCH_CONV", "1")
    with pytest.warns(UserWarning, match="torch/MIOpen"):
        got = ops.conv3d_input_grad(gy, w, lib=lib)
    want = torch.nn.grad.conv3d_input((1, 11, 6, 6, 6), w.cpu().double(), gy.cpu().double(), padding=1)
    assert float((got.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def check_function(lib, device, relu, cin=16, cout=16, ks=3, D=6):
    """ops.conv3d_autograd: the forward's bits are conv3d's at ``ops.CONV_GRAD_PRECISION``; the gradients of sum(y * g) follow float64 autograd of
    [relu] F.conv3d -- gX by the forward kernel's 1e-5 contract, gW by the yardstick (X32: torch's float32 autograd on the
    CPU).  g is non-zero where y <= 0 too: those entries must not contribute.  (g is zero in a band of 1e-4 of the largest
    pre-activation around zero, where the sign of y is a matter of rounding.)"""
    from deeplocalproteindocking_amd import ops
    gen = torch.Generator().manual_seed(21 + int(relu))
    x = torch.rand(1, cin, D, D, D, generator=gen) - 0.3
    w = torch.randn(cout, cin, ks, ks, ks, generator=gen) * 0.1
    g = torch.randn(1, cout, D, D, D, generator=gen)
    pre64 = F.conv3d(x.double(), w.double(), padding=ks // 2)
    g = g * (pre64.abs() > 1e-4 * pre64.abs().max()).float()
    if relu:
        dead = (pre64 <= 0) & (g != 0)
        assert int(dead.sum()) > g.numel() // 10 and int(((pre64 > 0) & (g != 0)).sum()) > g.numel() // 10

    def torch_grads(dtype):
        a, b = x.to(dtype).clone().requires_grad_(), w.to(dtype).clone().requires_grad_()
        y = F.conv3d(a, b, padding=ks // 2)
        ((torch.relu(y) if relu else y) * g.to(dtype)).sum().backward()
        return a.grad, b.grad
    gx64, gw64 = torch_grads(torch.float64)
    _, gw32 = torch_grads(torch.float32)
    a, b = x.clone().to(device).requires_grad_(), w.clone().to(device).requires_grad_()
    y = ops.conv3d_autograd(a, b, relu=relu, lib=lib)
    with torch.no_grad():
        assert torch.equal(y.detach(), ops.conv3d(a, b, relu=relu, lib=lib, precision=ops.CONV_GRAD_PRECISION)) and y.requires_grad
        assert not ops.conv3d_autograd(a, b, relu=relu, lib=lib).requires_grad
    (y * g.to(device)).sum().backward()
    assert float((a.grad.cpu().double() - gx64).abs().max()) <= 1e-5 * float(gx64.abs().max())
    ac.yardstick("conv3d_autograd %s, %d -> %d, k %d, D %d: gW" % ("relu" if relu else "linear", cin, cout, ks, D), b.grad.cpu(), gw32, gw64)
    # only what is asked for
    a2 = x.clone().to(device).requires_grad_()
    ops.conv3d_autograd(a2, w.to(device), relu=relu, lib=lib).backward(g.to(device))
    assert torch.equal(a2.grad, a.grad)


# ---------------------------------------------------------------------------------------------------------------- plugins
def set_lib(net, lib):
    from deeplocalproteindocking_amd.Models.ProteinRepresentationModels import IsotropicConv3d
    net.hip_lib = lib
    for m in net.modules():
        if isinstance(m, IsotropicConv3d):
            m.hip_lib = lib


def plain_torch_forward(net, vol):
    """The plugin's layer plan by torch's own calls: what the module is under autograd without ``hip_autograd``."""
    from deeplocalproteindocking_amd.Models import E3MultiResRepr4x4
    from deeplocalproteindocking_amd.Models.ProteinRepresentationModels import IsotropicConv3d
    if isinstance(net, E3MultiResRepr4x4):
        v1 = net.conv1(vol)
        return [v1, net.conv2(v1)]
    outs, x = [], vol
    for seq in (net.sequence_res0, net.sequence_res1):
        for m in seq:
            x = F.conv3d(x, m.kernel(), padding=m.padding, stride=m.stride) if isinstance(m, IsotropicConv3d) else m(x)
        outs.append(x)
    return outs


def _param_grads(net, outs, proj):
    net.zero_grad()
    sum((o * p.to(device=o.device, dtype=o.dtype)).sum() for o, p in zip(outs, proj)).backward()
    return {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()}


def check_plugin(lib, device, cls, D, monkeypatch, where=""):
    """Parameter gradients of a fixed random projection of both outputs with ``hip_autograd`` on: every parameter by the
    yardstick (X64: the module in float64 on the CPU, X32: in float32 on the CPU), while torch's stride-1 conv3d and
    conv3d_weight raise.  With ``hip_autograd`` off: the bits of plain torch."""
    torch.manual_seed(31)
    net = cls(multiplier=8)
    vol = smooth_nonneg(11, D, 41)[None].contiguous()
    gen = torch.Generator().manual_seed(43)
    shapes = [o.shape for o in net(vol)]
    proj = [torch.randn(s, generator=gen) for s in shapes]
    g32 = _param_grads(net, net(vol), proj)
    net64 = copy.deepcopy(net).double()
    g64 = _param_grads(net64, net64(vol.double()), proj)
    dnet = copy.deepcopy(net).to(device)
    set_lib(dnet, lib)
    dvol = vol.to(device)
    # off: the module under autograd IS plain torch.  No entry of ops may be reached, and the gradients have the bits of
    # torch's own calls wherever torch reproduces its own bits: on the CPU everywhere (asserted).  On an MI355X MIOpen's
    # weight gradient differs between two identical calls for some layers (E3MultiResRepr4x4 at box 16: five of nine
    # parameters, with and without torch.backends.cudnn.deterministic); a parameter whose two plain runs differ cannot be
    # compared by bits and answers to the yardstick instead, as the HIP path does below.
    assert dnet.hip_autograd is False
    from deeplocalproteindocking_amd import ops

    def unreachable(*a, **k):
        raise AssertionError("an ops entry was reached with hip_autograd off")
    plain_a = _param_grads(dnet, plain_torch_forward(dnet, dvol), proj)          # (also the warm-up of torch's algorithm choice)
    plain_a = _param_grads(dnet, plain_torch_forward(dnet, dvol), proj)
    with monkeypatch.context() as mp:
        for name in ("conv3d", "conv3d_autograd", "conv3d_weight_grad", "conv3d_input_grad", "maxpool3d_5s2"):
            mp.setattr(ops, name, unreachable)
        off = _param_grads(dnet, dnet(dvol), proj)
    plain_b = _param_grads(dnet, plain_torch_forward(dnet, dvol), proj)
    same = [n for n in plain_a if torch.equal(plain_a[n], plain_b[n])]
    print("hip_autograd off: torch reproduces its own bits for %d of %d parameters" % (len(same), len(plain_a)))
    assert same and (len(same) == len(plain_a) or torch.device(device).type != "cpu")
    for n in plain_a:
        if n in same:
            assert torch.equal(off[n], plain_a[n]), n
        else:
            ac.yardstick("%s(8) hip_autograd off, D %d%s: d/d %s" % (cls.__name__, D, where, n), off[n], g32[n], g64[n])
    # on: HIP forward and backward; torch's stride-1 convolution is out of reach
    conv3d, conv3d_weight = F.conv3d, torch.nn.grad.conv3d_weight

    def guarded(fn, at):
        def call(*a, **k):
            stride = k.get("stride", a[at] if len(a) > at else 1)
            if stride in (1, (1,), (1, 1, 1), [1, 1, 1]):
                raise AssertionError("torch's stride-1 %s was called on the hip_autograd path" % fn.__name__)
            return fn(*a, **k)
        return call
    dnet.hip_autograd = True
    with monkeypatch.context() as mp:
        mp.setattr(torch.nn.functional, "conv3d", guarded(conv3d, 3))
        mp.setattr(torch.nn.grad, "conv3d_weight", guarded(conv3d_weight, 3))
        outs = dnet(dvol)
        on = _param_grads(dnet, outs, proj)
    for o, s in zip(outs, shapes):
        assert o.shape == s and o.requires_grad
    for n in g64:
        assert float(g64[n].abs().max()) > 0, n
        ac.yardstick("%s(8) hip_autograd, D %d%s: d/d %s" % (cls.__name__, D, where, n), on[n], g32[n], g64[n])


def synthetic_pairs(tmp_path, n=4):
    from synth_pdb import write_protein_like_pdb
    recs, ligs = [], []
    for i in range(n):
        recs.append(str(tmp_path / ("r%d.pdb" % i)))
        ligs.append(str(tmp_path / ("l%d.pdb" % i)))
        write_protein_like_pdb(recs[-1], 30 + i, 20 + i, extras=False)
        write_protein_like_pdb(ligs[-1], 24 + i, 40 + i, extras=False)
    return recs, ligs, torch.tensor([0.1, 0.9, 0.5, 0.3][:n])


def check_trainer(lib, device, tmp_path, monkeypatch):
    """One LocalTrainer.optimize step at box 16 with hip_conv=True: a finite loss, equal to the identically seeded
    hip_conv=False trainer's to 1e-5 relative (the forward differs by summation order), every representation parameter moved,
    and the backward went through the kernels: one weight gradient per Conv3d and protein (9 x 2), one input gradient for
    every layer but the first (8 x 2) -- none without hip_conv."""
    from deeplocalproteindocking_amd import ops
    calls = {"conv3d_weight_grad": 0, "conv3d_input_grad": 0}

    def counted(name):
        fn = getattr(ops, name)

        def call(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return call
    for name in calls:
        monkeypatch.setattr(ops, name, counted(name))
    from deeplocalproteindocking_amd.Models import BatchRankingLoss, E3MultiResRepr4x4, LocalDockingModel, SimpleFilter
    from deeplocalproteindocking_amd.Training import LocalTrainer
    data = synthetic_pairs(tmp_path)
    losses = {}
    for hip in (False, True):
        torch.manual_seed(11)
        net = E3MultiResRepr4x4(multiplier=8)
        model = LocalDockingModel(representation=net, filter=SimpleFilter(net.get_num_outputs()), lib=lib).to(device)
        set_lib(net, lib)
        with torch.no_grad():
            model.filter.fc[0].bias.fill_(0.5)                     # (hidden units active: every weight has a gradient)
            model.filter.fc[0].weight.abs_()
        trainer = LocalTrainer(model, BatchRankingLoss(), lr=0.01, box_size=16, resolution=2.0, randomize_rot=False, lib=lib, hip_conv=hip)
        assert net.hip_autograd is hip
        before = {n: p.detach().clone() for n, p in net.named_parameters()}
        losses[hip] = trainer.optimize(data)
        trainer.cleanup()
        assert np.isfinite(losses[hip]) and losses[hip] > 0
        assert calls == ({"conv3d_weight_grad": 18, "conv3d_input_grad": 16} if hip else {"conv3d_weight_grad": 0, "conv3d_input_grad": 0}), calls
        if hip:
            for n, p in net.named_parameters():
                assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[n]), n
    print("LocalTrainer box 16: loss %.8g with hip_conv, %.8g without" % (losses[True], losses[False]))
    assert abs(losses[True] - losses[False]) <= 1e-5 * abs(losses[False])
