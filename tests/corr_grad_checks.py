"""Check bodies of the differentiable VolumeConvolution (csrc/dlpd_corr_grad.h, dlpd_correlate_generic_grad), shared by
tests/test_corr_grad_emu.py (the kernel sources on the fibre emulator) and tests/test_corr_grad_gpu.py (the gfx950 build).

Truth and tolerance.  With N = 2L, g the incoming gradient over the whole (N, N, N) grid and G, V1, V2 the N^3 spectra of g
and of the zero-padded volumes,

    grad_v1 = IDFT3(G . V2)[:L, :L, :L]            grad_v2 = IDFT3(V1 . conj(G))[:L, :L, :L]

evaluated in float64 ``torch.fft`` on the CPU is the truth, and the same two lines in float32 ``torch.fft`` are the oracle of
``accuracy_checks.yardstick``: the kernels may sit no further from float64 than that float32 evaluation does, times 2 (RMS)
and 3 (max) -- the project's standing rule, no number of this file's own, on every route (the plan-free one included).
A case in which the float32 evaluation shows no error at all measures nothing and is dropped (yardstick's own rule); the
exact cases are then still held to their closed form to float32 rounding of a sum of N^3 terms.
"""
import numpy as np
import torch

import accuracy_checks as ac
from accuracy_checks import yardstick


def formulas(g, v1, v2, dtype):
    """(grad_v1, grad_v2) of the module docstring for g (.., N, N, N), v1, v2 (.., L, L, L), in ``dtype`` on the CPU."""
    g, v1, v2 = (t.detach().cpu().to(dtype) for t in (g, v1, v2))
    L = v1.shape[-1]
    N = 2 * L
    G = torch.fft.rfftn(g, dim=(-3, -2, -1))
    V1, V2 = (torch.fft.rfftn(v, s=(N, N, N), dim=(-3, -2, -1)) for v in (v1, v2))
    g1 = torch.fft.irfftn(G * V2, s=(N, N, N), dim=(-3, -2, -1))[..., :L, :L, :L]
    g2 = torch.fft.irfftn(V1 * G.conj(), s=(N, N, N), dim=(-3, -2, -1))[..., :L, :L, :L]
    return g1.contiguous(), g2.contiguous()


def correlate(v1, v2, dtype):
    """The forward in ``dtype`` torch.fft on the CPU: (.., N, N, N)."""
    v1, v2 = (t.detach().cpu().to(dtype) for t in (v1, v2))
    N = 2 * v1.shape[-1]
    V1, V2 = (torch.fft.rfftn(v, s=(N, N, N), dim=(-3, -2, -1)) for v in (v1, v2))
    return torch.fft.irfftn(V1 * V2.conj(), s=(N, N, N), dim=(-3, -2, -1))


def route(lib, L, embed=True):
    return "compiled" if ac.lib_supports(lib, L) else ("embedded" if embed else "plan-free")


def kernel_grads(lib, device, g, v1, v2, embed=True, clip=None, want=(True, True)):
    """(out, grad_v1, grad_v2) through ops.VolumeConvolution and autograd."""
    from deeplocalproteindocking_amd.ops import VolumeConvolution
    a = v1.detach().clone().to(device).requires_grad_(want[0])
    b = v2.detach().clone().to(device).requires_grad_(want[1])
    out = VolumeConvolution(clip=clip, lib=lib, embed=embed)(a, b)
    out.backward(g.to(device))
    return out.detach().cpu(), (a.grad.cpu() if want[0] else None), (b.grad.cpu() if want[1] else None)


def volumes(L, B, C, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, L, L, L, generator=gen), torch.randn(B, C, L, L, L, generator=gen), gen


def check_dense(lib, device, L, B, C, embed=True, seed=0):
    """Both gradients for a dense normal g against float64."""
    v1, v2, gen = volumes(L, B, C, seed)
    g = torch.randn(B, C, 2 * L, 2 * L, 2 * L, generator=gen)
    _, k1, k2 = kernel_grads(lib, device, g, v1, v2, embed=embed)
    x64, x32 = formulas(g, v1, v2, torch.float64), formulas(g, v1, v2, torch.float32)
    r = route(lib, L, embed)
    for name, k, a32, a64 in (("grad_v1", k1, x32[0], x64[0]), ("grad_v2", k2, x32[1], x64[1])):
        assert k.shape == (B, C, L, L, L)
        yardstick("VolumeConvolution backward box %d (%s) %dx%d, dense g, %s" % (L, r, B, C, name), k, a32, a64)


def special_gradients(L, reps):
    """g (2 + 2 reps, N, N, N), one volume per case: an impulse at a translation with negative components (stored at
    N + t), an impulse with a component equal to L (no overlap: both gradients are zero), ``reps`` copies of (-1)^tz (only
    the Nyquist plane kz = L of the spectrum) and ``reps`` of a constant (only DC)."""
    N = 2 * L
    g = torch.zeros(2 + 2 * reps, N, N, N)
    t_neg, t_edge = (-3, 5, -(L - 1)), (2, L, -1)
    g[0][tuple(c % N for c in t_neg)] = 1.0
    g[1][tuple(c % N for c in t_edge)] = 1.0
    g[2:2 + reps] = torch.tensor([1.0, -1.0]).repeat(L).reshape(1, 1, 1, N)
    g[2 + reps:] = 0.75
    return g, t_neg, t_edge


def _shift_crop(v, t, sign):
    """w[s] = v[s + sign t] where that lies in the box, zero elsewhere (float64)."""
    L = v.shape[-1]
    w = torch.zeros(L, L, L, dtype=torch.float64)
    src, dst = [], []
    for c in t:
        d = sign * c
        lo, hi = max(0, -d), min(L, L - d)
        if lo >= hi:
            return w
        dst.append(slice(lo, hi))
        src.append(slice(lo + d, hi + d))
    w[tuple(dst)] = v.double()[tuple(src)]
    return w


def check_special_gradients(lib, device, L, reps=1, seed=3, float64_check=True):
    """The g of ``special_gradients`` as the channels of one call, every channel with volumes of its own; each kind against
    its closed form through the yardstick.  The closed forms ARE the truth; float64_check also holds the float64 formulas to
    them on one volume of each kind (left out at the two largest boxes, where that transform on the host is what costs).
    reps.  For (-1)^tz and for a constant every element of a gradient is the same ONE number (+-sum (-1)^rz v[r], c sum v): a
    volume holds a single draw of the rounding error, on either side, and the ratio of two single draws is anything.  The
    yardstick's premise is many draws from one distribution, so these two kinds are measured over ``reps`` volumes with
    different v1, v2, pooled (an RMS ratio of 2 between two samples of 16 equal-variance draws has a probability of 0.4 %,
    of 8 draws 3 %).  On the power-of-two plans both kinds are exact up to the one final rounding on both sides, so one
    volume is enough there (the emulator's box 32)."""
    N, C = 2 * L, 2 + 2 * reps
    v1, v2, _ = volumes(L, 1, C, seed)
    g, t_neg, t_edge = special_gradients(L, reps)
    _, k1, k2 = kernel_grads(lib, device, g[None], v1, v2)
    x32 = formulas(g[None], v1, v2, torch.float32)
    first = [0, 1] + ([2, 2 + reps] if reps else [])            # one volume of each kind: the closed forms against float64
    x64 = formulas(g[None][:, first], v1[:, first], v2[:, first], torch.float64) if float64_check else None
    # grad_v1[s] = v2[s - t], grad_v2[r] = v1[r + t] for an impulse at t;  (-1)^tz: grad_v1[s] = (-1)^sz sum_r (-1)^rz v2[r],
    # grad_v2[r] = (-1)^rz sum_s (-1)^sz v1[s];  a constant c: grad_v1 = c sum v2, grad_v2 = c sum v1
    sgn = torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(L // 2 + 1)[:L].reshape(1, 1, L)
    closed = [(_shift_crop(v2[0, 0], t_neg, -1), _shift_crop(v1[0, 0], t_neg, +1)),
              (torch.zeros(L, L, L, dtype=torch.float64), torch.zeros(L, L, L, dtype=torch.float64))]
    closed += [tuple((sgn * (v[0, c].double() * sgn).sum()).expand(L, L, L) for v in (v2, v1)) for c in range(2, 2 + reps)]
    closed += [tuple((0.75 * v[0, c].double().sum()).expand(L, L, L) for v in (v2, v1)) for c in range(2 + reps, C)]
    kinds = [("impulse at negative t", [0]), ("impulse with a component L", [1])]
    if reps:
        kinds += [("(-1)^tz: Nyquist plane only", list(range(2, 2 + reps))), ("constant: DC only", list(range(2 + reps, C)))]
    vmax = float(v1.abs().max())
    eps = 2.0 ** -23
    for name, chans in kinds:
        for which, k in ((0, k1), (1, k2)):
            exact = torch.stack([closed[c][which] for c in chans])
            scale = max(float(exact.abs().max()), vmax)
            if x64 is not None:
                assert float((x64[which][0, first.index(chans[0])] - exact[0]).abs().max()) <= 1e-11 * scale, (name, which)
            label = "VolumeConvolution backward box %d, %s (%d), grad_v%d" % (L, name, len(chans), which + 1)
            # The bound that stands when the yardstick has nothing to measure.  An impulse: every output is ONE term v[s -+ t]
            # carried through three transforms of log2(N^3) butterfly stages and one product, a rounding of at most eps max|v|
            # per stage (Higham, Accuracy and Stability of Numerical Algorithms, section 24.1, the worst case: linear in the
            # stages) -- 4 log2(N^3) eps max|v|, 1e-5 relative at N = 160.  The two sums of L^3 terms: sqrt(N^3) eps scale.
            bound = (4.0 * np.log2(float(N) ** 3) if len(chans) == 1 and chans[0] < 2 else np.sqrt(float(N) ** 3)) * eps * scale
            assert float((k[0, chans].double() - exact).abs().max()) <= bound, label
            if float((x32[which][0, chans].double() - exact).abs().max()) == 0.0:
                print("ACCURACY | %-58s | dropped: the float32 evaluation is exact here" % label)
                continue
            yardstick(label, k[0, chans], x32[which][0, chans], exact)


def check_transpose(lib, device, L, B, C, seed=5):
    """<VolumeConvolution(v1, v2), g> = <v1, grad_v1> = <v2, grad_v2> with the FORWARD kernel on the left, per volume, the sums
    in float64.  The RMS over the volumes of the two discrepancies may be no larger than 3 x what the float32 torch.fft pair
    (``correlate`` and ``formulas`` in float32) shows on the same inputs."""
    v1, v2, gen = volumes(L, B, C, seed)
    g = torch.randn(B, C, 2 * L, 2 * L, 2 * L, generator=gen)
    out, k1, k2 = kernel_grads(lib, device, g, v1, v2)
    o32 = correlate(v1, v2, torch.float32)
    f1, f2 = formulas(g, v1, v2, torch.float32)

    def gaps(o, a, b):
        dot = lambda x, y: (x.double() * y.double()).reshape(B * C, -1).sum(1)      # noqa: E731
        lhs = dot(o, g)
        return torch.cat([lhs - dot(v1, a), lhs - dot(v2, b)]), float(lhs.abs().max())
    ek, scale = gaps(out, k1, k2)
    eo, _ = gaps(o32, f1, f2)
    rk, ro = float(ek.pow(2).mean().sqrt()), float(eo.pow(2).mean().sqrt())
    print("ACCURACY | %-58s | kernel %.3e | float32 torch.fft %.3e | ratio %.3f | scale %.3e" %
          ("transpose identity box %d, %d volumes" % (L, B * C), rk, ro, rk / ro if ro > 0 else float("inf"), scale), flush=True)
    assert ro > 0
    assert rk <= 3.0 * ro, (rk, ro)


CLIP_BAND, CLIP_CAP = 1e-4, 0.01


def check_clip(lib, device, L=32, seed=7):
    """clip = 0.25 max|corr| on uniform random volumes: the incoming gradient is zeroed where the correlation was clamped.
    Translations whose float64 correlation lies within 1e-4 max|corr| of +-clip (the forward's parity band: a float32
    correlation may fall on the other side there) carry no incoming gradient; they are at most 1 % of the grid."""
    gen = torch.Generator().manual_seed(seed)
    v1, v2 = torch.rand(1, 2, L, L, L, generator=gen), torch.rand(1, 2, L, L, L, generator=gen)
    c64 = correlate(v1, v2, torch.float64)
    top = float(c64.abs().max())
    clip = 0.25 * top
    near = ((c64.abs() - clip).abs() <= CLIP_BAND * top)
    clamped = float((c64.abs() >= clip).double().mean())
    print("clip %.4g: clamped %.2f %%, left out %.4f %%" % (clip, 100 * clamped, 100 * float(near.double().mean())))
    assert float(near.double().mean()) <= CLIP_CAP
    assert 0.05 <= clamped <= 0.5
    g = torch.randn(1, 2, 2 * L, 2 * L, 2 * L, generator=gen) * (~near).float()
    out, k1, k2 = kernel_grads(lib, device, g, v1, v2, clip=clip)
    assert float(out.abs().max()) <= np.float32(clip)
    x64 = formulas(g.double() * (c64.abs() < clip), v1, v2, torch.float64)
    c32 = correlate(v1, v2, torch.float32)
    x32 = formulas(g * (c32.abs() < clip), v1, v2, torch.float32)
    for name, k, a32, a64 in (("grad_v1", k1, x32[0], x64[0]), ("grad_v2", k2, x32[1], x64[1])):
        yardstick("VolumeConvolution(clip) backward box %d, %s" % (L, name), k, a32, a64)


class Recorder:
    """Wraps a library: records (name, args) of every call."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def call(self, name, *args):
        self.calls.append((name, args))
        return self._lib.call(name, *args)

    def __getattr__(self, name):
        return getattr(self._lib, name)


def check_autograd_surface(lib, device, L=32, C=1, seed=9):
    """needs_input_grad decides which gradient is computed (null pointers for the other); sum().backward(); the forward's bits
    with and without a graph; two backward calls."""
    from deeplocalproteindocking_amd import ops
    v1, v2, gen = volumes(L, 1, C, seed)
    N = 2 * L
    g = torch.randn(1, C, N, N, N, generator=gen)
    conv = ops.VolumeConvolution(lib=lib)
    a, b = v1.to(device), v2.to(device)
    with torch.no_grad():
        plain = conv(a, b)
    assert plain.grad_fn is None and not plain.requires_grad
    # both inputs; the forward's bits do not depend on the graph
    ra, rb = a.clone().requires_grad_(), b.clone().requires_grad_()
    out = conv(ra, rb)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    out.backward(g.to(device), retain_graph=True)
    first = (ra.grad.clone(), rb.grad.clone())
    ra.grad = rb.grad = None
    out.backward(g.to(device))
    assert torch.equal(ra.grad, first[0]) and torch.equal(rb.grad, first[1])          # no atomics: the same bits
    # one input only: None for the other, and its kernels are not asked for
    for which in (0, 1):
        rec = Recorder(lib)
        x = (a if which == 0 else b).clone().requires_grad_()
        o = ops.VolumeConvolution(lib=rec)(x if which == 0 else a, b if which == 0 else x)
        o.backward(g.to(device))
        assert torch.equal(x.grad, first[which]) and a.grad is None and b.grad is None
        grads = [args for name, args in rec.calls if name == "dlpd_correlate_grad"]
        assert len(grads) >= 1
        for args in grads:                   # (gout, spec1, spec2, g1, g2, ...): g1 reads spec2, g2 reads spec1
            assert (args[3] is None) == (which == 1) and (args[4] is None) == (which == 0)
            assert (args[2] is None) == (which == 1) and (args[1] is None) == (which == 0)
        ffts = [1 for name, _ in rec.calls if name == "dlpd_rfft3d_padded"]
        assert len(ffts) == 1 + len(grads)                                              # the forward's, and ONE per backward chunk
    x = a.clone().requires_grad_()
    got = torch.autograd.grad(conv(x, b), [x], g.to(device))
    assert torch.equal(got[0], first[0])
    # sum().backward() hands in an expanded (non-contiguous) gradient: grad_v1 = sum v2 everywhere
    x = a.clone().requires_grad_()
    conv(x, b).sum().backward()
    want = v2.double().reshape(C, -1).sum(1).reshape(1, C, 1, 1, 1).expand(1, C, L, L, L)
    assert float((x.grad.cpu().double() - want).abs().max()) <= np.sqrt(float(N) ** 3) * 2.0 ** -23 * float(v2.abs().max())


def check_chunks(lib, device, L=32, seed=10):
    """5 volumes in chunks of 2, 2, 1 give the bits of one chunk."""
    from deeplocalproteindocking_amd import ops
    v1, v2, gen = volumes(L, 1, 5, seed)
    gd = torch.randn(1, 5, 2 * L, 2 * L, 2 * L, generator=gen).to(device)
    a, b = v1.to(device), v2.to(device)
    rec = Recorder(lib)
    one = ops._vc_grad(lib, gd, a, b, True, True, True)
    many = ops._vc_grad(rec, gd, a, b, True, True, True, chunk=2)
    assert [args[6] for name, args in rec.calls if name == "dlpd_correlate_grad"] == [2, 2, 1]
    assert torch.equal(one[0], many[0]) and torch.equal(one[1], many[1])


def check_errors(lib, device):
    """Argument errors of the two new entry points: the library's error codes (1 = DLPD_ERR_ARG, 2 = DLPD_ERR_UNSUPPORTED)."""
    L = 32
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=device)      # (never reached: every call below returns before a launch)
    p = buf.data_ptr()
    grad, gen = lib._dlpd_correlate_grad, lib._dlpd_correlate_generic_grad
    assert lib.call("dlpd_correlate_grad_supported", 32) == 1 and lib.call("dlpd_correlate_grad_supported", 33) == 0
    assert lib.call("dlpd_correlate_grad_ws_bytes", 1, 33) == 0 and lib.call("dlpd_correlate_grad_ws_bytes", 0, 32) == 0
    assert lib.call("dlpd_correlate_grad_ws_bytes", 2, 32) == 2 * 33 * (64 * 64 + 2 * 32 * 64 + 32 * 32) * 8
    assert lib.call("dlpd_correlate_generic_grad_ws_bytes", 1, 129) == 0
    assert lib.call("dlpd_correlate_generic_grad_ws_bytes", 1, 9) == (3 * 18 ** 3 + 81 * 18 + 9 * 324) * 8
    assert grad(None, p, p, p, p, p, 1, L, None) == 1
    assert grad(p, p, p, p, p, None, 1, L, None) == 1
    assert grad(p, p, p, None, None, p, 1, L, None) == 1               # neither gradient
    assert grad(p, p, None, p, None, p, 1, L, None) == 1               # g1 without the spectrum it reads
    assert grad(p, None, p, None, p, p, 1, L, None) == 1
    assert grad(p, p, p, p, p, p, 0, L, None) == 1
    assert grad(p, p, p, p, p, p, 1, 33, None) == 2
    assert gen(None, p, p, p, p, 1, 9, p, None) == 1
    assert gen(p, p, p, p, p, 1, 9, None, None) == 1
    assert gen(p, p, p, None, None, 1, 9, p, None) == 1
    assert gen(p, p, None, p, None, 1, 9, p, None) == 1
    assert gen(p, p, p, p, p, 0, 9, p, None) == 1
    assert gen(p, p, p, p, p, 1, 129, p, None) == 2


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------

class TwoResolutions(torch.nn.Module):
    """A small representation in plain torch: one Conv3d on the input grid and the same features pooled to half of it."""

    def __init__(self, channels=2):
        super().__init__()
        self.conv = torch.nn.Conv3d(1, channels, 3, padding=1)
        self.channels = channels

    def get_num_outputs(self):
        return [self.channels, self.channels]

    def forward(self, x):
        y = torch.tanh(self.conv(x))
        return [y, torch.nn.functional.avg_pool3d(y, 2)]


def _restatement(net, filt, rec, lig, target, dtype):
    """The model in pure torch on the CPU in ``dtype``: representation, torch.fft correlations, nearest upsampling, the filter
    on channels-last rows, softmax cross-entropy over the N^3 translations.  -> (loss, parameter gradients)."""
    import copy
    net, filt = copy.deepcopy(net).cpu().to(dtype), copy.deepcopy(filt).cpu().to(dtype)
    rv, lv = net(rec.cpu().to(dtype)), net(lig.cpu().to(dtype))
    corr = []
    for a, b in zip(rv, lv):
        n = 2 * a.shape[-1]
        A, Bs = (torch.fft.rfftn(v, s=(n, n, n), dim=(-3, -2, -1)) for v in (a, b))
        corr.append(torch.fft.irfftn(A * Bs.conj(), s=(n, n, n), dim=(-3, -2, -1)))
    N = corr[0].shape[-1]
    same = [c if c.shape[-1] == N else torch.nn.functional.interpolate(c, size=(N, N, N)) for c in corr]
    V = torch.cat(same, dim=1).permute(0, 2, 3, 4, 1).reshape(-1, sum(c.shape[1] for c in corr))
    loss = torch.nn.functional.cross_entropy(filt(V).reshape(1, -1), target.cpu())
    params = list(net.parameters()) + list(filt.parameters())
    return loss.detach(), torch.autograd.grad(loss, params)


def make_model(lib, device, L, differentiable, embed=True, channels=2, seed=21):
    from deeplocalproteindocking_amd.Models import GlobalDockingModel, SimpleFilter
    torch.manual_seed(seed)
    net = TwoResolutions(channels)
    filt = SimpleFilter(net.get_num_outputs())
    with torch.no_grad():
        filt.fc[0].bias.fill_(0.5)                  # (hidden units active: every weight has a gradient)
    model = GlobalDockingModel(net, filt, clip=None, lib=lib, differentiable=differentiable).to(device)
    model.convolve.embed = embed
    gen = torch.Generator().manual_seed(seed + 1)
    rec, lig = torch.rand(1, 1, L, L, L, generator=gen).to(device), torch.rand(1, 1, L, L, L, generator=gen).to(device)
    N = 2 * L
    target = torch.tensor([(3 * N + (N - 2)) * N + 5])              # translation (3, -2, 5)
    return model, rec, lig, target.to(device)


def model_loss(model, rec, lig, target):
    scores = model(model.representation(rec), model.representation(lig))
    return torch.nn.functional.cross_entropy(scores.reshape(1, -1), target), scores


def check_model_gradients(lib, device, L=32, channels=2):
    """Parameter gradients of GlobalDockingModel(differentiable=True) -- a Conv3d at box L and its pooled copy at L / 2, which
    is embedded in the next compiled box -- against the float64 restatement, the float32 one as the yardstick's oracle."""
    model, rec, lig, target = make_model(lib, device, L, True, channels=channels)
    loss, scores = model_loss(model, rec, lig, target)
    assert scores.shape == (1, 2 * L, 2 * L, 2 * L) and scores.grad_fn is not None
    params = list(model.representation.parameters()) + list(model.filter.parameters())
    got = torch.autograd.grad(loss, params)
    l64, g64 = _restatement(model.representation, model.filter, rec, lig, target, torch.float64)
    l32, g32 = _restatement(model.representation, model.filter, rec, lig, target, torch.float32)
    assert abs(float(loss.detach()) - float(l64)) <= 1e-5 * abs(float(l64))
    cat = lambda gs: torch.cat([t.detach().cpu().double().reshape(-1) for t in gs])      # noqa: E731
    names = [n for n, _ in model.representation.named_parameters()] + ["filter." + n for n, _ in model.filter.named_parameters()]
    print("parameters:", names)
    yardstick("GlobalDockingModel(differentiable=True) box %d + %d, parameter gradients" % (L, L // 2), cat(got), cat(g32), cat(g64))
    # under no_grad the differentiable model takes the fused filter path: the same scores to float32 rounding
    with torch.no_grad():
        fused = model(model.representation(rec), model.representation(lig))
    assert fused.grad_fn is None
    assert float((fused - scores.detach()).abs().max()) <= 1e-4 * float(scores.detach().abs().max())


def check_model_flag(lib, device, L=32, channels=2):
    """differentiable=False is the inference path whatever requires a gradient: no graph, and the bits of the fused path."""
    model, rec, lig, target = make_model(lib, device, L, False, channels=channels)
    assert model.differentiable is False
    rv, lv = model.representation(rec), model.representation(lig)
    assert rv[0].requires_grad
    out = model(rv, lv)                                                 # autograd enabled: it does not raise
    assert out.grad_fn is None and not out.requires_grad
    with torch.no_grad():
        ref = model([v.detach() for v in rv], [v.detach() for v in lv])
    assert torch.equal(out, ref)
    model.differentiable = True                                         # a public attribute
    with torch.no_grad():
        assert torch.equal(model(rv, lv), ref)
    assert model(rv, lv).grad_fn is not None


def check_model_trains(lib, device, L, embed=True, steps=5):
    """Five Adam steps on the softmax cross-entropy over the translation grid lower it."""
    model, rec, lig, target = make_model(lib, device, L, True, embed=embed)
    opt = torch.optim.Adam(model.parameters(), lr=2e-4)         # (the logits are sums of L^3 products: a small step)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss, _ = model_loss(model, rec, lig, target)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("losses:", " ".join("%.5f" % v for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
