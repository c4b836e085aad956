"""torch-facing operator objects with the call signatures the reference uses for
TorchProteinLibrary's volume ops, backed by libdlpd.so.

    VolumeRotation()(volume (B,C,L,L,L) f32 cuda, R (B,3,3) f32 cuda) -> (B,C,L,L,L)
        reference call: src/Docker/Docker.py:40,218
    VolumeConvolution(clip=None)(v1 (B,C,L,L,L), v2 same) -> (B,C,2L,2L,2L)
        reference calls: src/Docker/Docker.py:32,225 ; src/Models/DockingModels.py:48,71

    VolumeRotation also takes ONE (C,L,L,L) volume set for all B matrices, and is differentiable with respect to the
    volume (csrc/dlpd_rotate_grad.h), as the local correlations below are (local_correlate, local_correlate_rotated,
    MultiplyVolumes: csrc/dlpd_local_grad.h).  First order; T receives no gradient, and R only where it is asked for:
    ``VolumeRotation(rotation_grad=True)`` and ``local_correlate_rotated(..., rotation_grad=True)`` also return the gradient
    of the rotation matrices (csrc/dlpd_rotate_rgrad.h), what ``Docker.minimize`` descends.
    The same three calls take ``shift=``: a per-pose translation by a FRACTION of a voxel (csrc/dlpd_rotate_shift.h), which
    ``rotation_grad=True`` differentiates as well -- the three translational degrees of freedom of ``Docker.minimize(translation=True)``.
    ``conv3d_autograd`` is the plugins' stride-1 convolution with both gradients on the HIP kernels
    (``conv3d_input_grad``, ``conv3d_weight_grad``: csrc/dlpd_conv_grad.h); plain ``conv3d`` stays inference only.
    ``VolumeConvolution`` is differentiable with respect to both volumes wherever it runs (csrc/dlpd_corr_grad.h: the full
    transform of the incoming gradient, the products with the other volume's spectrum, inverses pruned to the L^3 corner;
    dlpd_correlate_generic_grad on a box without a compiled plan) -- what ``GlobalDockingModel(differentiable=True)`` trains through.
    ``filter_volumes_autograd`` is the grid filter (nearest upsample + concat + MLP over the correlations) with a graph: the
    inference kernel forward, one fused backward kernel for the correlations' and the four parameters' gradients
    (csrc/dlpd_filter_grad.h: the hidden layer recomputed, f32 matrix cores, fixed-order sums); plain ``filter_volumes`` and the
    clash mask stay inference only.  ``GlobalDockingModel(fused_filter_grad=True)`` uses it.

Everything else (the filter fused into the search pipeline, the max-pool, the fused search pipeline) is inference only (the docking search
runs under torch.no_grad(), local_test.py:67).
Box sizes 32 / 40 / 64 / 80 run the compiled FFT pipeline, any other box (<= 128) a plan-free slow path.
Build-defined conventions (TPL source absent, parity unpinned): rotation about index L/2 with
trilinear interpolation and zeros outside; ``clip`` clamps the correlation OUTPUT to +-clip.
"""
import torch
from torch import nn

from ._lib import get_lib
from .engine import _ptr, _stream
from .Utils.Conventions import CLIP_MODES, kernel_matrices, rotation_scale


def _check(t, name, lib=None):
    """lib: None -> the product library, GPU tensors only (no CPU path); the test-suite passes the
    emulated library, which takes host pointers."""
    if not (isinstance(t, torch.Tensor) and (t.is_cuda or lib is not None) and t.dtype == torch.float32):
        raise RuntimeError("dlpd: %s must be a float32 CUDA (ROCm) tensor; there is no CPU path" % name)
    return t.contiguous()


class VolumeRotation(nn.Module):
    """``center`` / ``scale`` / ``axis_order``: the conventions of Utils/Conventions.py (pivot index; stretch of the
    sample offset -- a number or "(L-1)/L" / "L/(L-1)"; "xyz" | "zyx"), folded into the 3x3 maps the kernel samples with."""

    def __init__(self, center=None, lib=None, scale=None, axis_order="xyz", transpose=False, rotation_grad=False):
        super().__init__()
        self.rotation_grad = bool(rotation_grad)
        self.center = center
        self.lib = lib
        self.scale = scale
        self.axis_order = axis_order
        self.transpose = bool(transpose)

    def forward(self, volume, R, shift=None):
        """volume (B, C, L, L, L) with R (B, 3, 3), or ONE (C, L, L, L) volume set for all B matrices -> (B, C, L, L, L).
        Differentiable with respect to ``volume`` (first order; csrc/dlpd_rotate_grad.h): when autograd is enabled and the
        volume requires a gradient the call is recorded -- the shared form's gradient is the sum over the B rotations.  ``R``
        receives a gradient only from an operator built with ``rotation_grad=True`` (csrc/dlpd_rotate_rgrad.h: the derivative
        of the trilinear sample, the right-hand one on a cell face; the conventions are folded into the kernel's maps in
        plain torch, so autograd carries it back to ``R``).  In every other case the call is the plain forward (the same
        bits either way).
        ``shift`` (B, 3) float32, voxels of the OUTPUT grid in index order [x][y][z]: the result is the rotated volume
        displaced by it, out(x) = rotated(x - shift), sampled in one trilinear gather (csrc/dlpd_rotate_shift.h: the kernel's
        offset off = -M^T shift, folded in plain torch after the conventions -- autograd carries its gradient back to
        ``shift`` and, through M, to ``R``).  ``shift`` receives a gradient only with ``rotation_grad=True``, as ``R``; zeros
        give the bits of the call without it."""
        volume, R = _check(volume, "volume", self.lib), _check(R, "R", self.lib)
        if volume.dim() not in (4, 5):
            raise RuntimeError("dlpd: VolumeRotation expects (B, C, L, L, L) or (C, L, L, L), got %s" % (tuple(volume.shape),))
        L = volume.shape[-1]
        if volume.dim() == 5 and R.shape[0] != volume.shape[0]:
            raise RuntimeError("dlpd: VolumeRotation batch mismatch: volume %d vs R %d" % (volume.shape[0], R.shape[0]))
        c0 = float(L) / 2.0 if self.center is None else float(self.center)
        if self.scale is not None or self.axis_order != "xyz" or self.transpose:
            R = kernel_matrices(R, rotation_scale(self.scale, L), self.axis_order, self.transpose)
        if shift is not None:
            off = _kernel_offset(R, _check(shift, "shift", self.lib))
            if self.rotation_grad and torch.is_grad_enabled() and (R.requires_grad or off.requires_grad):
                return _VolumeRotateShift.apply(volume, R, off, c0, self.lib, True)
            if torch.is_grad_enabled() and volume.requires_grad:
                return _VolumeRotateShift.apply(volume, R.detach(), off.detach(), c0, self.lib, False)
            return _volume_rotate_shift_forward(volume, R.detach(), off.detach(), c0, self.lib)
        if self.rotation_grad and torch.is_grad_enabled() and R.requires_grad:
            return _VolumeRotate.apply(volume, R, c0, self.lib, True)
        if torch.is_grad_enabled() and volume.requires_grad:
            return _VolumeRotate.apply(volume, R, c0, self.lib)
        return _volume_rotate_forward(volume, R, c0, self.lib)


def _volume_rotate_forward(volume, M, c0, lib):
    """M: the kernel's 3x3 maps (the conventions folded in)."""
    B, C, L = M.shape[0], volume.shape[-4], volume.shape[-1]
    out = torch.empty(B, C, L, L, L, dtype=torch.float32, device=volume.device)
    (lib or get_lib()).call("dlpd_rotate_trilinear", _ptr(volume), _ptr(M), _ptr(out), B, C, L,
                            C * L ** 3 if volume.dim() == 5 else 0, c0, _stream(volume.device))
    return out


class _VolumeRotate(torch.autograd.Function):
    """VolumeRotation under autograd: the forward is the plain call, the backward dlpd_rotate_trilinear_grad with the same maps
    and, for ``rgrad``, dlpd_rotate_trilinear_rgrad: the gradient of the maps themselves."""

    @staticmethod
    def forward(ctx, volume, M, c0, lib, rgrad=False):
        ctx.save_for_backward(M, *((volume,) if rgrad else ()))
        ctx.args = (tuple(volume.shape), c0, lib)
        return _volume_rotate_forward(volume.detach(), M.detach(), c0, lib)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        M = ctx.saved_tensors[0]
        shape, c0, lib = ctx.args
        lib_ = lib or get_lib()
        g = _check(gout, "the gradient", lib)
        B, C, L = M.shape[0], shape[-4], shape[-1]
        stride = C * L ** 3 if len(shape) == 5 else 0
        gvol = gM = None
        if ctx.needs_input_grad[0]:
            gvol = torch.empty(shape, dtype=torch.float32, device=g.device)
            lib_.call("dlpd_rotate_trilinear_grad", _ptr(g), _ptr(M), _ptr(gvol), B, C, L, stride, c0, 0, _stream(g.device))
        if len(ctx.saved_tensors) == 2 and ctx.needs_input_grad[1]:
            vol = ctx.saved_tensors[1].detach()
            gM = torch.empty(B, 3, 3, dtype=torch.float32, device=g.device)
            ws = torch.empty(_rgrad_ws_bytes(lib_, B, L), dtype=torch.uint8, device=g.device)
            lib_.call("dlpd_rotate_trilinear_rgrad", _ptr(g), _ptr(vol), _ptr(M), _ptr(gM), _ptr(ws), B, C, L, stride, c0,
                      _stream(g.device))
        return gvol, gM, None, None, None


def _kernel_offset(M, shift):
    """The kernels' source-space offset of a displacement by ``shift`` voxels of the output grid: the sample of output voxel x
    is taken at p(x - shift) = c0 + (x - shift - c0) M, so off = -shift M (``off = -M^T shift``).  Plain torch: differentiable
    in both."""
    if shift.dim() != 2 or shift.shape[1] != 3 or shift.shape[0] != M.shape[0]:
        raise RuntimeError("dlpd: shift must be (%d, 3), one row per matrix, got %s" % (M.shape[0], tuple(shift.shape)))
    return -torch.matmul(shift.unsqueeze(1), M).squeeze(1).contiguous()


def _volume_rotate_shift_forward(volume, M, off, c0, lib):
    B, C, L = M.shape[0], volume.shape[-4], volume.shape[-1]
    out = torch.empty(B, C, L, L, L, dtype=torch.float32, device=volume.device)
    (lib or get_lib()).call("dlpd_rotate_trilinear_shift", _ptr(volume), _ptr(M), _ptr(off), _ptr(out), B, C, L,
                            C * L ** 3 if volume.dim() == 5 else 0, c0, _stream(volume.device))
    return out


class _VolumeRotateShift(torch.autograd.Function):
    """VolumeRotation(shift=) under autograd: the forward is dlpd_rotate_trilinear_shift, the backward
    dlpd_rotate_trilinear_shift_grad for the volume and, for ``pgrad``, dlpd_rotate_trilinear_pgrad for the maps and the offsets."""

    @staticmethod
    def forward(ctx, volume, M, off, c0, lib, pgrad):
        M, off = M.contiguous(), off.contiguous()
        ctx.save_for_backward(M, off, *((volume,) if pgrad else ()))
        ctx.args = (tuple(volume.shape), c0, lib)
        return _volume_rotate_shift_forward(volume.detach(), M.detach(), off.detach(), c0, lib)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        M, off = ctx.saved_tensors[0].detach(), ctx.saved_tensors[1].detach()
        shape, c0, lib = ctx.args
        lib_ = lib or get_lib()
        g = _check(gout, "the gradient", lib)
        B, C, L = M.shape[0], shape[-4], shape[-1]
        stride = C * L ** 3 if len(shape) == 5 else 0
        gvol = gM = goff = None
        if ctx.needs_input_grad[0]:
            gvol = torch.empty(shape, dtype=torch.float32, device=g.device)
            lib_.call("dlpd_rotate_trilinear_shift_grad", _ptr(g), _ptr(M), _ptr(off), _ptr(gvol), B, C, L, stride, c0, 0,
                      _stream(g.device))
        if len(ctx.saved_tensors) == 3 and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            vol = ctx.saved_tensors[2].detach()
            gM = torch.empty(B, 3, 3, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[1] else None
            goff = torch.empty(B, 3, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[2] else None
            ws = torch.empty(_pgrad_ws_bytes(lib_, B, L), dtype=torch.uint8, device=g.device)
            lib_.call("dlpd_rotate_trilinear_pgrad", _ptr(g), _ptr(vol), _ptr(M), _ptr(off), _ptr(gM), _ptr(goff), _ptr(ws), B, C, L,
                      stride, c0, _stream(g.device))
        return gvol, gM, goff, None, None, None


def _pgrad_ws_bytes(lib_, B, L):
    n = lib_.call("dlpd_rotate_trilinear_pgrad_ws_bytes", B, L)
    if n == 0:
        raise RuntimeError("dlpd: the pose gradient supports boxes 2..128 (box %d)" % L)
    return n


def _rgrad_ws_bytes(lib_, B, L):
    n = lib_.call("dlpd_rotate_trilinear_rgrad_ws_bytes", B, L)
    if n == 0:
        raise RuntimeError("dlpd: the rotation's gradient supports boxes 2..128 (box %d)" % L)
    return n


class VolumeConvolution(nn.Module):
    """Per-channel circular cross-correlation on the 2L zero-padded grid:
    out[b,c,t mod 2L] = sum_r v1[b,c,r+t] * v2[b,c,r]  (semantics: MultiplyVolumes.py:13-47)."""

    def __init__(self, clip=None, lib=None, embed=True, clip_mode="output"):
        """clip_mode (Utils/Conventions.py): "output" clamps the correlation to +-clip (this build's definition),
        "input" clamps both input volumes instead, "none" ignores ``clip``."""
        super().__init__()
        if clip_mode not in CLIP_MODES:
            raise RuntimeError("dlpd: clip_mode must be one of %s" % (CLIP_MODES,))
        self.clip_mode = clip_mode
        self.clip = clip
        self.lib = lib
        self.embed = embed          # boxes without a compiled plan: inside the next compiled box (False: plan-free transforms)

    @property
    def out_clip(self):
        """The clamp the kernels apply to the correlation OUTPUT (None: no clamp)."""
        return self.clip if self.clip_mode == "output" else None

    def forward(self, input_volume1, input_volume2):
        """Differentiable with respect to both volumes (first order; csrc/dlpd_corr_grad.h, and dlpd_correlate_generic_grad on
        a box without a compiled plan): when autograd is enabled and one of them requires a gradient the call is recorded, and
        only the gradients that are needed are computed.  The forward is the same call either way (the same bits).  With
        ``clip`` in "output" mode the gradient is zero where the correlation was clamped (|out| >= clip); "input" mode clamps
        in plain torch before the operator and an embedded box is cut out in plain torch after it: autograd carries both."""
        v1, v2 = _check(input_volume1, "volume1", self.lib), _check(input_volume2, "volume2", self.lib)
        if v1.shape != v2.shape:
            raise RuntimeError("dlpd: VolumeConvolution shape mismatch %s vs %s" % (tuple(v1.shape), tuple(v2.shape)))
        if self.clip is not None and self.clip_mode == "input":
            c = float(self.clip)
            v1, v2 = v1.clamp(-c, c), v2.clamp(-c, c)
        B, C, L = v1.shape[0], v1.shape[1], v1.shape[2]
        lib = self.lib or get_lib()
        graph = torch.is_grad_enabled() and (v1.requires_grad or v2.requires_grad)
        if not lib.call("dlpd_grid_supported", L):
            Lc = next((c for c in (32, 40, 64, 80) if c > L and lib.call("dlpd_grid_supported", c)), None) if self.embed else None
            if Lc is None:
                if graph:
                    return _VolumeConvolve.apply(v1, v2, self, lib, False)
                return self._forward_generic(v1, v2, lib)
            # the L^3 volumes in the corner of the next compiled box: the correlation of two L-sized volumes is linear
            # for every |t| < L on any grid of >= 2L points, so the (2L)^3 result sits inside the (2Lc)^3 one at index t
            # (0 <= t <= L; t = L: no overlap, zero) and 2Lc + t (-L < t < 0)
            e1, e2 = (torch.zeros(B, C, Lc, Lc, Lc, dtype=torch.float32, device=v1.device) for _ in range(2))
            e1[:, :, :L, :L, :L], e2[:, :, :L, :L, :L] = v1, v2
            big = self.forward(e1, e2)
            idx = torch.tensor(list(range(0, L + 1)) + list(range(2 * Lc - (L - 1), 2 * Lc)), dtype=torch.long, device=v1.device)
            return big.index_select(2, idx).index_select(3, idx).index_select(4, idx).contiguous()
        if graph:
            return _VolumeConvolve.apply(v1, v2, self, lib, True)
        return self._forward_compiled(v1, v2, lib)

    def _forward_compiled(self, v1, v2, lib):
        B, C, L = v1.shape[0], v1.shape[1], v1.shape[2]
        N, NZ, nvol = 2 * L, L + 1, B * C
        dev, st = v1.device, _stream(v1.device)
        wsA = torch.empty(nvol * NZ * L * L * 2, dtype=torch.float32, device=dev)
        spec = torch.empty(nvol * NZ * N * N * 2, dtype=torch.float32, device=dev)
        lib.call("dlpd_rfft3d_padded", _ptr(v1), _ptr(spec), _ptr(wsA), nvol, L, 1.0 / float(N) ** 3, st)
        lib.call("dlpd_zfft", _ptr(v2), 0, _ptr(wsA), 1, nvol, L, 0, 0, 0.0, st)
        wsB = torch.empty(nvol * NZ * N * N * 2, dtype=torch.float32, device=dev)
        lib.call("dlpd_xy_correlate", _ptr(wsA), _ptr(spec), _ptr(wsB), 1, nvol, L, 0, st)
        out = torch.empty(B, C, N, N, N, dtype=torch.float32, device=dev)
        oc = self.out_clip
        lib.call("dlpd_zifft_real", _ptr(wsB), _ptr(out), 1, nvol, L, 0 if oc is None else 1, float(oc or 0.0), st)
        return out


def _vc_generic(self, v1, v2, lib):
    """Any other box size (the reference's ``box_size`` is free, Docker.py:18): the plan-free correlation of
    dlpd_correlate_generic, in chunks of volumes that keep the scratch below ~4 GB."""
    B, C, L = v1.shape[0], v1.shape[1], v1.shape[2]
    if not lib.call("dlpd_generic_box_supported", L):
        raise RuntimeError("dlpd: VolumeConvolution box size %d exceeds the generic path (box <= 128)" % L)
    N, nvol = 2 * L, B * C
    dev, st = v1.device, _stream(v1.device)
    out = torch.empty(B, C, N, N, N, dtype=torch.float32, device=dev)
    per = lib.call("dlpd_correlate_generic_ws_bytes", 1, L)
    chunk = max(1, min(nvol, (4 << 30) // per, 65535 // N))
    ws = torch.empty(per * chunk, dtype=torch.uint8, device=dev)
    a, b, o = v1.reshape(nvol, -1), v2.reshape(nvol, -1), out.reshape(nvol, -1)
    for beg in range(0, nvol, chunk):
        n = min(chunk, nvol - beg)
        lib.call("dlpd_correlate_generic", _ptr(a[beg]), _ptr(b[beg]), _ptr(o[beg]), n, L, 0 if self.out_clip is None else 1,
                 float(self.out_clip or 0.0), _ptr(ws), st)
    return out


VolumeConvolution._forward_generic = _vc_generic

CORR_GRAD_WS_BYTES = 2 << 30        # cap of the backward's scratch (workspace and the two spectra): volumes go in chunks that fit it


def _vc_grad(lib, g, v1, v2, want1, want2, compiled, chunk=None):
    """The two input gradients of VolumeConvolution for the incoming gradient ``g`` (B, C, N, N, N), contiguous: (g1, g2), None
    for one that is not wanted -- its kernels are not launched, its output pointer is null.  compiled: dlpd_correlate_grad with
    the spectra of the volumes recomputed here by dlpd_rfft3d_padded(scale = 1) (none is kept alive between forward and
    backward); otherwise dlpd_correlate_generic_grad.  ``chunk``: volumes per call (None: what keeps the scratch below
    ``CORR_GRAD_WS_BYTES``); the volumes are independent, so the bits do not depend on it."""
    B, C, L = v1.shape[0], v1.shape[1], v1.shape[2]
    N, NZ, nvol = 2 * L, L + 1, B * C
    dev, st = v1.device, _stream(v1.device)
    g1 = torch.empty_like(v1) if want1 else None
    g2 = torch.empty_like(v2) if want2 else None
    spec_bytes = NZ * N * N * 8
    if compiled:
        per = lib.call("dlpd_correlate_grad_ws_bytes", 1, L)
        if per == 0:
            raise RuntimeError("dlpd: no VolumeConvolution backward kernel for box %d" % L)
        most = max(1, CORR_GRAD_WS_BYTES // (per + (want1 + want2) * spec_bytes + NZ * L * L * 8))
    else:
        per = lib.call("dlpd_correlate_generic_grad_ws_bytes", 1, L)
        if per == 0:
            raise RuntimeError("dlpd: VolumeConvolution box size %d exceeds the generic path (box <= 128)" % L)
        most = max(1, min((4 << 30) // per, 65535 // N))
    chunk = max(1, min(nvol, most if chunk is None else int(chunk)))
    ws = torch.empty(per * chunk, dtype=torch.uint8, device=dev)
    if compiled:
        wsA = torch.empty(chunk * NZ * L * L * 2, dtype=torch.float32, device=dev)
        spec1 = torch.empty(chunk * spec_bytes, dtype=torch.uint8, device=dev) if want2 else None      # (g2 reads V1, g1 reads V2)
        spec2 = torch.empty(chunk * spec_bytes, dtype=torch.uint8, device=dev) if want1 else None
    vol, big = 4 * L ** 3, 4 * N ** 3
    for beg in range(0, nvol, chunk):
        n = min(chunk, nvol - beg)
        p1, p2 = (_ptr(g1) + vol * beg) if want1 else None, (_ptr(g2) + vol * beg) if want2 else None
        if compiled:
            if want2:
                lib.call("dlpd_rfft3d_padded", _ptr(v1) + vol * beg, _ptr(spec1), _ptr(wsA), n, L, 1.0, st)
            if want1:
                lib.call("dlpd_rfft3d_padded", _ptr(v2) + vol * beg, _ptr(spec2), _ptr(wsA), n, L, 1.0, st)
            lib.call("dlpd_correlate_grad", _ptr(g) + big * beg, _ptr(spec1) or None, _ptr(spec2) or None, p1, p2, _ptr(ws), n, L, st)
        else:
            lib.call("dlpd_correlate_generic_grad", _ptr(g) + big * beg, _ptr(v1) + vol * beg, _ptr(v2) + vol * beg, p1, p2, n, L,
                     _ptr(ws), st)
    return g1, g2


class _VolumeConvolve(torch.autograd.Function):
    """VolumeConvolution under autograd: the forward is the plain call (compiled box or plan-free), the backward ``_vc_grad``
    for the inputs that need a gradient.  Saved: the two inputs, and the output where it was clamped (the clamp's mask)."""

    @staticmethod
    def forward(ctx, v1, v2, op, lib, compiled):
        a, b = v1.detach(), v2.detach()
        out = op._forward_compiled(a, b, lib) if compiled else op._forward_generic(a, b, lib)
        clip = op.out_clip
        ctx.save_for_backward(v1, v2, *((out,) if clip is not None else ()))
        ctx.args = (lib, op.lib, compiled, clip)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        v1, v2 = ctx.saved_tensors[0].detach(), ctx.saved_tensors[1].detach()
        lib, given, compiled, clip = ctx.args
        g = _check(gout, "the gradient", given)                # (contiguous: out.sum().backward() hands in an expanded tensor)
        if clip is not None:
            g = g * (ctx.saved_tensors[2].abs() < float(clip)).to(g.dtype)
        g1, g2 = _vc_grad(lib, g, v1, v2, ctx.needs_input_grad[0], ctx.needs_input_grad[1], compiled)
        return g1, g2, None, None, None


def filter_volumes(conv_list, W1, b1, W2, b2, mask_norm=None, threshold=0.0, lib=None):
    """Nearest-upsample + concat + SimpleFilter MLP (+ optional clash mask) on materialised
    correlation volumes -- DockingModels.py:74-83, Docker.py:226,232.  conv_list: one or two
    tensors (B,C_i,N_i,N_i,N_i), N_0 the finest."""
    c0 = _check(conv_list[0], "conv0", lib)
    B, C0, N0 = c0.shape[0], c0.shape[1], c0.shape[2]
    if len(conv_list) > 2:
        raise RuntimeError("dlpd: at most two resolutions are supported")
    c1 = _check(conv_list[1], "conv1", lib) if len(conv_list) == 2 else None
    C1, N1 = (c1.shape[1], c1.shape[2]) if c1 is not None else (0, 0)
    dev = c0.device
    H = W1.shape[0]
    W1t = W1.detach().to(dev, torch.float32).t().contiguous()       # (C, H)
    b1 = b1.detach().to(dev, torch.float32).contiguous()
    W2 = W2.detach().to(dev, torch.float32).reshape(-1).contiguous()
    V = torch.empty(B, N0, N0, N0, dtype=torch.float32, device=dev)
    has_clash = mask_norm is not None
    if has_clash:
        mask_norm = _check(mask_norm, "mask_norm", lib)
    (lib or get_lib()).call("dlpd_filter_mask", _ptr(c0), C0, N0, _ptr(c1), C1, N1, _ptr(mask_norm), float(threshold),
                   int(has_clash), _ptr(W1t), _ptr(b1), _ptr(W2), float(b2), H, _ptr(V), B, _stream(dev))
    return V


def filter_grad_supported(C0, N0, C1, N1, H, lib=None):
    """True where the filter's backward kernel (csrc/dlpd_filter_grad.h) exists for conv0 (B, C0, N0^3), conv1 (B, C1, N1^3)
    and hidden width H."""
    return bool((lib or get_lib()).call("dlpd_filter_grad_supported", int(C0), int(N0), int(C1), int(N1), int(H)))


def _filter_shapes(conv_list):
    if not 1 <= len(conv_list) <= 2:
        raise RuntimeError("dlpd: one or two resolutions are supported")
    c0 = conv_list[0]
    c1 = conv_list[1] if len(conv_list) == 2 else None
    return (c0.shape[1], c0.shape[2]) + ((c1.shape[1], c1.shape[2]) if c1 is not None else (0, 0))


class _FilterVolumes(torch.autograd.Function):
    """filter_volumes under autograd: the forward is the inference kernel (no clash mask), the backward ONE dlpd_filter_grad
    call for the gradients that are asked for.  Saved: the correlations and the four parameters -- `pre` is recomputed."""

    @staticmethod
    def forward(ctx, c0, c1, W1, b1, W2, b2, lib):
        convs = [c0.detach()] + ([c1.detach()] if c1 is not None else [])
        V = filter_volumes(convs, W1.detach(), b1.detach(), W2.detach(), float(b2.detach().reshape(-1)[0]), lib=lib)
        ctx.save_for_backward(c0, W1, b1, W2, b2, *((c1,) if c1 is not None else ()))
        ctx.lib = lib
        return V

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        c0, W1, b1, W2, b2 = (t.detach() for t in ctx.saved_tensors[:5])
        c1 = ctx.saved_tensors[5].detach() if len(ctx.saved_tensors) == 6 else None
        given = ctx.lib
        lib = given or get_lib()
        g = _check(gout, "the gradient", given)                # (contiguous: V.sum().backward() hands in an expanded tensor)
        need = ctx.needs_input_grad
        B, C0, N0 = c0.shape[0], c0.shape[1], c0.shape[2]
        C1, N1 = (c1.shape[1], c1.shape[2]) if c1 is not None else (0, 0)
        H, C, dev = W1.shape[0], C0 + C1, c0.device
        W1t = W1.to(dev, torch.float32).t().contiguous()       # (C, H), as the forward passes it
        b1c = b1.to(dev, torch.float32).contiguous()
        W2c = W2.to(dev, torch.float32).reshape(-1).contiguous()
        g0 = torch.empty_like(c0) if need[0] else None
        g1 = torch.empty_like(c1) if (c1 is not None and need[1]) else None
        want_params = any(need[2:6])
        gp = ws = None
        if want_params:
            gp = torch.empty(C * H + 2 * H + 1, dtype=torch.float32, device=dev)
            ws = torch.empty(lib.call("dlpd_filter_grad_ws_bytes", C0, N0, C1, N1, H, B), dtype=torch.uint8, device=dev)
        if g0 is not None or g1 is not None or want_params:
            lib.call("dlpd_filter_grad", _ptr(g), _ptr(c0), C0, N0, _ptr(c1), C1, N1, _ptr(W1t), _ptr(b1c), _ptr(W2c), H,
                     _ptr(g0), _ptr(g1), _ptr(gp), _ptr(ws), B, _stream(dev))
        gW1 = gb1 = gW2 = gb2 = None
        if want_params:
            if need[2]:
                gW1 = gp[:C * H].reshape(C, H).t().to(W1).contiguous()
            if need[3]:
                gb1 = gp[C * H:C * H + H].to(b1).clone()
            if need[4]:
                gW2 = gp[C * H + H:C * H + 2 * H].to(W2).reshape(W2.shape).clone()
            if need[5]:
                gb2 = gp[C * H + 2 * H:].to(b2).reshape(b2.shape).clone()
        return g0, g1, gW1, gb1, gW2, gb2, None


def filter_volumes_autograd(conv_list, W1, b1, W2, b2, lib=None):
    """``filter_volumes`` (no clash mask) with a graph: conv_list as there, the parameters as ``nn.Linear`` holds them -- W1 (H, C),
    b1 (H), W2 (1, H), b2 (1), live tensors -- -> V (B, N0, N0, N0), the bits of ``filter_volumes``.  The backward is the fused
    kernel of csrc/dlpd_filter_grad.h: the gradients of the correlations and of the four parameters that are asked for, from one
    call that recomputes the hidden layer (first order only).  RuntimeError where the kernel does not exist
    (``filter_grad_supported``)."""
    conv_list = list(conv_list)
    C0, N0, C1, N1 = _filter_shapes(conv_list)
    H = W1.shape[0]
    if W1.dim() != 2 or W1.shape[1] != C0 + C1 or b1.numel() != H or W2.numel() != H or b2.numel() != 1:
        raise RuntimeError("dlpd: filter parameters do not match the correlations: W1 (H, C0 + C1), b1 (H), W2 (1, H), b2 (1)")
    if not filter_grad_supported(C0, N0, C1, N1, H, lib):
        raise RuntimeError("dlpd: no filter backward kernel for %d @ %d^3 + %d @ %d^3, hidden width %d" % (C0, N0, C1, N1, H))
    c0 = _check(conv_list[0], "conv0", lib)
    c1 = _check(conv_list[1], "conv1", lib) if len(conv_list) == 2 else None
    return _FilterVolumes.apply(c0, c1, W1, b1, W2, b2, lib)


def conv3d_supported(weight, D, lib=None):
    cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[2]
    cubic = weight.dim() == 5 and weight.shape[2] == weight.shape[3] == weight.shape[4]
    return bool(cubic and (lib or get_lib()).call("dlpd_conv3d_supported", int(cin), int(cout), int(ks), int(D)))


CONV_PRECISION = "split_bf16"      # default arithmetic of conv3d: "split_bf16" (3 x bf16 terms, six products: f32-grade) | "f32"


def tile_occupancy(x, lib=None):
    """Which 4 x 4 x 4 cells of x (B, C, D, D, D) hold a non-zero value: uint8 (B, ceil(D/4), ceil(D/4), ceil(D/4)), the
    ``occupancy`` argument of conv3d."""
    lib = lib or get_lib()
    x = x.contiguous()
    B, cin, D = x.shape[0], x.shape[1], x.shape[2]
    occ = torch.empty(B, (D + 3) // 4, (D + 3) // 4, (D + 3) // 4, dtype=torch.uint8, device=x.device)
    assert occ.numel() == lib.call("dlpd_conv3d_tile_occupancy_bytes", B, D)
    lib.call("dlpd_conv3d_tile_occupancy", _ptr(x), _ptr(occ), B, cin, D, _stream(x.device))
    return occ


def conv3d(x, weight, relu=False, lib=None, stride=1, precision=None, occupancy=None, return_occupancy=False, unwritten=False):
    """[relu] Conv3d(x, weight, padding=k//2, stride=1|2, bias=None) of the representation plugins
    (ProteinRepresentationModels.py:38-61,85-114) on the matrix cores (inference only: no autograd).
    x (B, cin, D, D, D) float32; weight (cout, cin, k, k, k).
    precision: "f32" = exact f32 products on the f32-input matrix instruction; "split_bf16" = every value as three
    bf16 terms, six bf16 products per f32 product, f32 accumulation (equal to the f32 form to a few 1e-7 relative,
    2-3x faster); None = ``ops.CONV_PRECISION``.
    occupancy (split_bf16 only): ``tile_occupancy(x)`` -- output tiles whose neighbouring input tiles are all empty are
    written as zeros without being computed (there is no bias: they ARE zero; same bits).  return_occupancy: -> (y, the
    occupancy of y or None), which the next layer takes -- a representation network pays for one map, of its input.
    unwritten (needs occupancy, return_occupancy, stride 1): the tensors travel WITH their maps -- cells that ``occupancy``
    marks empty are never read (they count as zeros, whatever the memory holds) and skipped output tiles are not written:
    y is undefined wherever the returned map is 0.  Only for consumers that go by the map (the next layer, maxpool3d_5s2,
    the engine's volumes path)."""
    lib = lib or get_lib()
    x = x.contiguous()
    if unwritten and not (occupancy is not None and return_occupancy and stride == 1 and (precision or CONV_PRECISION) == "split_bf16"):
        raise RuntimeError("dlpd: conv3d(unwritten=True) needs the input's occupancy, return_occupancy, stride 1 and split_bf16")
    if x.dtype != torch.float32 or x.dim() != 5 or not (x.shape[2] == x.shape[3] == x.shape[4]):
        raise RuntimeError("dlpd: conv3d expects (B, C, D, D, D) float32, got %s %s" % (x.dtype, tuple(x.shape)))
    B, cin, D = x.shape[0], x.shape[1], x.shape[2]
    w = weight.detach().to(device=x.device, dtype=torch.float32).contiguous()
    cout, ks = w.shape[0], w.shape[2]
    if w.shape[1] != cin:
        raise RuntimeError("dlpd: conv3d channel mismatch %d vs %d" % (w.shape[1], cin))
    precision = precision or CONV_PRECISION
    if precision not in ("f32", "split_bf16"):
        raise RuntimeError("dlpd: conv3d precision %r" % (precision,))
    split = precision == "split_bf16"
    wp = _packed_weights(weight, w, lib, x.device, split)
    if stride not in (1, 2):
        raise RuntimeError("dlpd: conv3d stride %r not supported (1 or 2)" % (stride,))
    Do = (D - 1) // stride + 1
    y = torch.empty(B, cout, Do, Do, Do, dtype=torch.float32, device=x.device)
    occ_out = None
    if split and (occupancy is not None or return_occupancy):
        if occupancy is not None and (occupancy.dtype != torch.uint8 or occupancy.device != x.device or
                                      occupancy.numel() != lib.call("dlpd_conv3d_tile_occupancy_bytes", B, D)):
            raise RuntimeError("dlpd: conv3d occupancy does not belong to this input (shape %s)" % (tuple(occupancy.shape),))
        if return_occupancy and stride == 1:
            occ_out = torch.empty(B, (D + 3) // 4, (D + 3) // 4, (D + 3) // 4, dtype=torch.uint8, device=x.device)
        lib.call("dlpd_conv3d_split_sparse", _ptr(x), _ptr(wp), _ptr(y),
                 _ptr(occupancy.contiguous()) if occupancy is not None else None, _ptr(occ_out) if occ_out is not None else None,
                 B, cin, cout, D, ks, int(bool(relu)), int(stride), int(bool(unwritten)), _stream(x.device))
    else:
        lib.call("dlpd_conv3d_split" if split else "dlpd_conv3d_strided", _ptr(x), _ptr(wp), _ptr(y), B, cin, cout, D, ks,
                 int(bool(relu)), int(stride), _stream(x.device))
    return (y, occ_out) if return_occupancy else y


_PACKED = {}


def _packed_weights(weight, w, lib, device, split=False):
    """dlpd_conv3d_pack; cached per (parameter, version) for nn.Parameters -- inference weights do not
    change between batches.  Other tensors (e.g. kernels composed on the fly) are packed per call: their
    storage may be recycled with new contents under the same address."""
    cacheable = isinstance(weight, torch.nn.Parameter)
    key = (id(weight), weight.data_ptr(), weight._version, tuple(weight.shape), str(device), id(lib), bool(split))
    if cacheable and key in _PACKED:
        return _PACKED[key]
    cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
    if split:
        wp = torch.empty(lib.call("dlpd_conv3d_split_packed_bytes", cin, cout, ks), dtype=torch.uint8, device=device)
        lib.call("dlpd_conv3d_split_pack", _ptr(w), _ptr(wp), cin, cout, ks, _stream(device))
    else:
        wp = torch.empty(lib.call("dlpd_conv3d_packed_floats", cin, cout, ks), dtype=torch.float32, device=device)
        lib.call("dlpd_conv3d_pack", _ptr(w), _ptr(wp), cin, cout, ks, _stream(device))
    if cacheable:
        if device.type == "cuda":
            # the packed copy outlives this call and may next be used from ANOTHER stream (a sweep prepares the next target
            # on a stream of its own, Docker.prepare): it must be complete before it is published -- once per weight
            torch.cuda.current_stream(device).synchronize()
        if len(_PACKED) > 64:
            _PACKED.clear()
        _PACKED[key] = wp
    return wp


# Arithmetic of conv3d_autograd's forward and input gradient (None there = this).  Exact f32, not conv3d's split_bf16: the three
# bf16 terms reproduce an f32 product to a few 1e-7, which inference does not see but a parameter gradient, held to twice
# the error of a float32 evaluation, does (EXPERIMENTS.md, CONV-GRAD: 4.6-8.8 x that error at box 16 against 1.5-2.2 x).
CONV_GRAD_PRECISION = "f32"
CONV_WGRAD_PARTS = 256             # blocks the weight gradient's voxels are split over: a constant, so the bits are the machine's neighbour's too


def _conv_volumes(t, name, lib):
    t = _check(t, name, lib)
    if t.dim() != 5 or not (t.shape[2] == t.shape[3] == t.shape[4]):
        raise RuntimeError("dlpd: %s must be (B, C, D, D, D), got %s" % (name, tuple(t.shape)))
    return t


def conv3d_weight_grad(x, gy, ks, lib=None, nparts=None):
    """gW (cout, cin, ks, ks, ks) of y = conv3d(x, w, padding=ks//2, stride=1, bias=None) for the upstream gradient gy:
    gW[co, ci, d] = sum_b sum_v gy[b, co, v] x[b, ci, v + d - ks//2] (csrc/dlpd_conv_grad.h: exact f32 products on the matrix
    cores, f32 accumulation).  x (B, cin, D, D, D), gy (B, cout, D, D, D) float32.  The sum runs over ``nparts`` fixed parts
    of the voxels added in a fixed order (None: ``CONV_WGRAD_PARTS``): the same bits for the same nparts, on any device."""
    lib_ = lib or get_lib()
    x, gy = _conv_volumes(x, "x", lib), _conv_volumes(gy, "gy", lib)
    B, cin, D, cout, ks = x.shape[0], x.shape[1], x.shape[2], gy.shape[1], int(ks)
    if gy.shape[0] != B or gy.shape[2] != D or gy.device != x.device:
        raise RuntimeError("dlpd: conv3d_weight_grad shape mismatch %s vs %s" % (tuple(x.shape), tuple(gy.shape)))
    if not lib_.call("dlpd_conv3d_supported", cin, cout, ks, D):
        raise RuntimeError("dlpd: conv3d_weight_grad has no HIP kernel for %d -> %d channels, kernel %d, box %d (supported: "
                           "kernel 3 or 5, output channels a multiple of 16, box <= 80)" % (cin, cout, ks, D))
    nparts = int(CONV_WGRAD_PARTS if nparts is None else nparts)
    ws = torch.empty(lib_.call("dlpd_conv3d_wgrad_ws_floats", cin, cout, ks, nparts), dtype=torch.float32, device=x.device)
    gw = torch.empty(cout, cin, ks, ks, ks, dtype=torch.float32, device=x.device)
    lib_.call("dlpd_conv3d_wgrad", _ptr(x), _ptr(gy), _ptr(gw), _ptr(ws), B, cin, cout, D, ks, nparts, _stream(x.device))
    return gw


CONV_GX_GROUP = 8                  # output channels of the layer summed by one call of the forward kernel in conv3d_input_grad


def conv3d_input_grad(gy, weight, lib=None, precision=None):
    """gX (B, cin, D, D, D) of the same stride-1 layer: the FORWARD kernel applied to gy with the taps flipped and the channel
    axes exchanged (any ``precision`` of ``conv3d``; the weights are packed per call).  The forward kernel adds all its
    cout * k^3 terms in one running sum; here the layer's output channels go through it in groups of ``CONV_GX_GROUP`` whose
    results are added in ascending order -- a sum of sums, which is what holds a plugin's parameter gradients to the error
    of a float32 evaluation (EXPERIMENTS.md, CONV-GRAD).  It needs the layer's cin to be a multiple of 16 -- every layer of
    both plugins but the first, whose input needs no gradient.  Where it cannot run it is an error, unless
    DLPD_ALLOW_TORCH_CONV=1: then ``torch.nn.grad.conv3d_input`` does it, with a warning."""
    gy = _conv_volumes(gy, "gy", lib)
    w = weight.detach().to(device=gy.device, dtype=torch.float32)
    if w.dim() != 5 or w.shape[0] != gy.shape[1]:
        raise RuntimeError("dlpd: conv3d_input_grad channel mismatch %s vs %s" % (tuple(w.shape), tuple(gy.shape)))
    wt = w.flip(2, 3, 4).transpose(0, 1).contiguous()               # (cin, cout, k, k, k): a layer from cout to cin channels
    if not conv3d_supported(wt, gy.shape[2], lib):
        from .Models.ProteinRepresentationModels import _torch_conv_allowed
        _torch_conv_allowed("the input gradient of Conv3d%s on %s" % (tuple(w.shape), tuple(gy.shape)))      # (raises unless allowed)
        size = (gy.shape[0], w.shape[1]) + tuple(gy.shape[2:])
        return torch.nn.grad.conv3d_input(size, w, gy, padding=w.shape[2] // 2)
    gx = None
    for beg in range(0, w.shape[0], CONV_GX_GROUP):
        part = conv3d(gy[:, beg:beg + CONV_GX_GROUP].contiguous(), wt[:, beg:beg + CONV_GX_GROUP].contiguous(), lib=lib, precision=precision)
        gx = part if gx is None else gx.add_(part)
    return gx


class _Conv3d(torch.autograd.Function):
    """conv3d_autograd: the forward is the plain call; the backward masks the upstream gradient by the ReLU and runs
    conv3d_input_grad / conv3d_weight_grad for the inputs that need a gradient."""

    @staticmethod
    def forward(ctx, x, weight, relu, lib, precision):
        # (weight.detach(): not the nn.Parameter, so packed per call -- conv3d's cache of packed parameters, which synchronises
        #  the stream when it publishes an entry, would be refilled after every optimizer step)
        y = conv3d(x.detach(), weight.detach(), relu=relu, lib=lib, precision=precision)
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.args = (relu, lib, precision)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        relu, lib, precision = ctx.args
        gy = _check(gy, "the gradient", lib)
        if relu:
            gy = gy * (y > 0).to(gy.dtype)
        gx = conv3d_input_grad(gy, weight, lib=lib, precision=precision) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            gw = conv3d_weight_grad(x.detach(), gy, weight.shape[2], lib=lib).to(device=weight.device, dtype=weight.dtype)
        return gx, gw, None, None, None


def conv3d_autograd(x, weight, relu=False, lib=None, precision=None):
    """``conv3d(x, weight, relu=relu)`` (stride 1) that autograd can differentiate: first order, with respect to ``x`` and
    ``weight``, both on the HIP kernels (the forward kernel for gX, csrc/dlpd_conv_grad.h for gW).  Plain ``conv3d`` stays
    inference only; this is the call the plugins make with ``hip_autograd`` set.  precision: of the forward and of gX, None =
    ``CONV_GRAD_PRECISION`` (gW is always exact f32).  Without autograd it is ``conv3d`` at that precision."""
    precision = precision or CONV_GRAD_PRECISION
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        x = _conv_volumes(x, "x", lib)
        if weight.dim() != 5 or not conv3d_supported(weight, x.shape[2], lib):
            raise RuntimeError("dlpd: conv3d_autograd has no HIP kernel for weights %s on %s" % (tuple(weight.shape), tuple(x.shape)))
        return _Conv3d.apply(x, weight, bool(relu), lib, precision)
    return conv3d(x, weight, relu=relu, lib=lib, precision=precision)


def maxpool3d_5s2(x, lib=None, occupancy=None, return_occupancy=False, unwritten=False):
    """MaxPool3d(kernel_size=5, stride=2, padding=2) of the E3 plugin, (B, C, D, D, D) float32 (inference).
    occupancy: ``tile_occupancy(x)`` (or what the convolution that made x handed on) -- output tiles whose inputs lie in
    empty cells are zeros and are written without reading them; return_occupancy: -> (y, the occupancy of y).
    unwritten (needs occupancy and return_occupancy): as conv3d -- empty input cells are not read, empty output tiles not written."""
    lib = lib or get_lib()
    if unwritten and not (occupancy is not None and return_occupancy):
        raise RuntimeError("dlpd: maxpool3d_5s2(unwritten=True) needs the input's occupancy and return_occupancy")
    x = x.contiguous()
    B, C, D = x.shape[0], x.shape[1], x.shape[2]
    Do = (D - 1) // 2 + 1
    y = torch.empty(B, C, Do, Do, Do, dtype=torch.float32, device=x.device)
    if occupancy is None and not return_occupancy:
        lib.call("dlpd_maxpool3d_5s2", _ptr(x), _ptr(y), B * C, D, _stream(x.device))
        return y
    if occupancy is not None and (occupancy.dtype != torch.uint8 or occupancy.device != x.device or
                                  occupancy.numel() != lib.call("dlpd_conv3d_tile_occupancy_bytes", B, D)):
        raise RuntimeError("dlpd: maxpool3d_5s2 occupancy does not belong to this input (shape %s)" % (tuple(occupancy.shape),))
    occ_out = torch.empty(B, (Do + 3) // 4, (Do + 3) // 4, (Do + 3) // 4, dtype=torch.uint8, device=x.device) if return_occupancy else None
    lib.call("dlpd_maxpool3d_5s2_sparse", _ptr(x), _ptr(y), _ptr(occupancy.contiguous()) if occupancy is not None else None,
             _ptr(occ_out), B, C, D, int(bool(unwritten)), _stream(x.device))
    return (y, occ_out) if return_occupancy else y


# ------------------------------------------------------------------------------------------------------------------
# Local docking: direct correlation at given poses (csrc/dlpd_local.h)
# ------------------------------------------------------------------------------------------------------------------
COARSE_MODES = {"floor": 0, "trunc": 1}
LOCAL_WS_BYTES = 256 << 20          # cap of the partial-sum workspace: poses are processed in batches that fit it


def _pose_volumes(v, P, name, lib):
    """(C, L, L, L) shared by all poses -> stride 0; (P, C, L, L, L) -> one set per pose."""
    v = _check(v, name, lib)
    if v.dim() == 4:
        return v, 0
    if v.dim() != 5 or v.shape[0] != P:
        raise RuntimeError("dlpd: %s must be (C, L, L, L) or (P, C, L, L, L) with P = %d, got %s" % (name, P, tuple(v.shape)))
    return v, v.shape[1] * v.shape[2] ** 3


def local_correlate(receptor, ligand, T, R=None, radius=0, scale=1, coarse="floor", center=None, lib=None, shift=None):
    """corr (P, C, W, W, W), W = 2 radius + 1: corr[p, c, d] = sum_x receptor[c, x + coarse(T_p) + d] * ligand'[c, x], ligand' the
    ligand rotated by R_p (the 3x3 maps ``VolumeRotation`` samples with; None: as it is) -- the slices of
    MultiplyVolumes.multiply (MultiplyVolumes.py:13-47) summed directly.  receptor / ligand: (C, L, L, L) for all poses or
    (P, C, L, L, L); T (P, 3) int32 signed translations on the grid of ``scale`` * L points; coarse(t) = floor(t / scale)
    ("floor": the global search's index) or trunc(t / scale) ("trunc": Python's int()).
    Differentiable with respect to ``receptor`` and ``ligand`` (first order; csrc/dlpd_local_grad.h): when autograd is enabled and
    one of them requires a gradient the call is recorded, and the gradient of a volume shared by all poses is the sum over the
    poses.  ``T`` and ``R`` receive no gradient, and the ligand's gradient THROUGH a rotation (``R`` given) is not this
    function's: that combination raises -- ``local_correlate_rotated`` is the call that has it.  In every other case the call
    is the plain forward.
    ``shift`` (P, 3) float32, voxels of THIS call's grid (needs ``R``): the rotated ligand is displaced by it, so that the
    effective translation of pose p is coarse(T_p) + d + shift_p (csrc/dlpd_rotate_shift.h); it receives no gradient here."""
    off = None
    if shift is not None:
        if R is None:
            raise RuntimeError("dlpd: local_correlate(shift=) needs the rotations R (a fractional translation is a resampling)")
        off = _kernel_offset(_check(R, "R", lib).detach(), _check(shift, "shift", lib).detach())
    if torch.is_grad_enabled() and any(isinstance(v, torch.Tensor) and v.requires_grad for v in (receptor, ligand)):
        if R is not None and ligand.requires_grad:
            raise RuntimeError("dlpd: local_correlate has no gradient with respect to a ROTATED ligand (R given) -- call "
                               "local_correlate_rotated, which has it, or detach the ligand")
        return _LocalCorrelate.apply(receptor, ligand, T, R, int(radius), int(scale), coarse, center, lib, off)
    return _local_correlate_forward(receptor, ligand, T, R, radius, scale, coarse, center, lib, off)


def _local_correlate_forward(receptor, ligand, T, R, radius, scale, coarse, center, lib, off=None):
    lib_ = lib or get_lib()
    T = T.contiguous()
    if T.dtype != torch.int32 or T.dim() != 2 or T.shape[1] != 3:
        raise RuntimeError("dlpd: T must be a (P, 3) int32 tensor")
    P = T.shape[0]
    rec, rs = _pose_volumes(receptor, P, "receptor", lib)
    lig, ls = _pose_volumes(ligand, P, "ligand", lib)
    C, L = rec.shape[-4], rec.shape[-1]
    if tuple(lig.shape[-4:]) != tuple(rec.shape[-4:]):
        raise RuntimeError("dlpd: local_correlate shape mismatch %s vs %s" % (tuple(rec.shape), tuple(lig.shape)))
    if R is not None:
        R = _check(R, "R", lib)
        if R.shape[0] != P:
            raise RuntimeError("dlpd: local_correlate needs one matrix per pose")
    r, W = int(radius), 2 * int(radius) + 1
    per = lib_.call("dlpd_local_ws_bytes", 1, C, L, r)
    if per == 0:
        raise RuntimeError("dlpd: local_correlate supports boxes 2..128 and radius 0..3 (box %d, radius %d)" % (L, r))
    if off is not None:
        off = _check(off, "the offset", lib)
    dev = rec.device
    if T.device != dev or lig.device != dev or (R is not None and R.device != dev) or (off is not None and off.device != dev):
        raise RuntimeError("dlpd: local_correlate arguments must be on one device")
    out = torch.empty(P, C, W, W, W, dtype=torch.float32, device=dev)
    chunk = max(1, min(P, LOCAL_WS_BYTES // per, lib_.call("dlpd_local_max_poses", C, L)))      # workspace and launch-grid limits
    ws = torch.empty(per * chunk, dtype=torch.uint8, device=dev)
    c0 = float(L) / 2.0 if center is None else float(center)
    st = _stream(dev)
    for beg in range(0, P, chunk):
        n = min(chunk, P - beg)
        if off is not None:
            lib_.call("dlpd_local_correlate_shift", _ptr(rec) + 4 * rs * beg, _ptr(lig) + 4 * ls * beg, _ptr(R) + 36 * beg,
                      _ptr(off) + 12 * beg, _ptr(T) + 12 * beg, _ptr(out) + 4 * C * W ** 3 * beg, _ptr(ws), n, C, L, r, int(scale),
                      COARSE_MODES[coarse], c0, rs, ls, st)
            continue
        lib_.call("dlpd_local_correlate", _ptr(rec) + 4 * rs * beg, _ptr(lig) + 4 * ls * beg,
                  (_ptr(R) + 36 * beg) if R is not None else None, _ptr(T) + 12 * beg, _ptr(out) + 4 * C * W ** 3 * beg, _ptr(ws),
                  n, C, L, r, int(scale), COARSE_MODES[coarse], c0, rs, ls, st)
    return out


class _LocalCorrelate(torch.autograd.Function):
    """local_correlate under autograd: the forward is the plain call, the backward dlpd_local_correlate_grad for the gradients
    that are needed.  Per-pose volumes go in batches of dlpd_local_max_poses, as in the forward; a volume shared by all poses
    takes every pose in one call (its gradient's grid does not grow with P)."""

    @staticmethod
    def forward(ctx, receptor, ligand, T, R, radius, scale, coarse, center, lib, off=None):
        ctx.save_for_backward(receptor, ligand, T, R, off)
        ctx.args = (radius, scale, coarse, center, lib)
        return _local_correlate_forward(receptor.detach(), ligand.detach(), T, R, radius, scale, coarse, center, lib, off)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gcorr):
        receptor, ligand, T, R, off = ctx.saved_tensors
        r, scale, coarse, center, lib = ctx.args
        lib_ = lib or get_lib()
        T = T.contiguous()
        P = T.shape[0]
        rec, rs = _pose_volumes(receptor.detach(), P, "receptor", lib)
        lig, ls = _pose_volumes(ligand.detach(), P, "ligand", lib)
        if R is not None:
            R = _check(R, "R", lib)
        g = _check(gcorr, "the gradient", lib)
        C, L, W = rec.shape[-4], rec.shape[-1], 2 * r + 1
        want_rec, want_lig = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grec = torch.empty_like(rec) if want_rec else None
        glig = torch.empty_like(lig) if want_lig else None
        c0 = float(L) / 2.0 if center is None else float(center)
        st = _stream(rec.device)
        most = lib_.call("dlpd_local_max_poses", C, L)

        def run(out_rec, out_lig, beg, n):
            if off is not None:                       # (with R; only the receptor's gradient is asked for then)
                lib_.call("dlpd_local_correlate_shift_grad", _ptr(rec) + 4 * rs * beg, _ptr(lig) + 4 * ls * beg, _ptr(R) + 36 * beg,
                          _ptr(off) + 12 * beg, _ptr(T) + 12 * beg, _ptr(g) + 4 * C * W ** 3 * beg,
                          (_ptr(grec) + 4 * rs * beg) if out_rec else None, (_ptr(glig) + 4 * ls * beg) if out_lig else None,
                          n, C, L, r, int(scale), COARSE_MODES[coarse], c0, rs, ls, st)
                return
            lib_.call("dlpd_local_correlate_grad", _ptr(rec) + 4 * rs * beg, _ptr(lig) + 4 * ls * beg,
                      (_ptr(R) + 36 * beg) if R is not None else None, _ptr(T) + 12 * beg, _ptr(g) + 4 * C * W ** 3 * beg,
                      (_ptr(grec) + 4 * rs * beg) if out_rec else None, (_ptr(glig) + 4 * ls * beg) if out_lig else None,
                      n, C, L, r, int(scale), COARSE_MODES[coarse], c0, rs, ls, st)
        # a gradient per pose: batches of at most one launch's poses; a shared volume's gradient: all poses, one call
        per_rec, per_lig = want_rec and rs != 0, want_lig and ls != 0
        if per_rec or per_lig:
            for beg in range(0, P, most):
                run(per_rec, per_lig, beg, min(most, P - beg))
        if (want_rec and rs == 0) or (want_lig and ls == 0):
            run(want_rec and rs == 0, want_lig and ls == 0, 0, P)
        return grec, glig, None, None, None, None, None, None, None, None


def local_correlate_rotated(receptor, ligand, T, R, radius=0, scale=1, coarse="floor", center=None, lib=None, rotation_grad=False,
                            shift=None):
    """``local_correlate(receptor, ligand, T, R=R, ...)`` -- the same call, the same bits, no rotated volume in memory --
    differentiable in BOTH volumes: what trains a model on the poses of a search's top list (rotations of one ligand).
    The receptor's gradient is the correlation's adjoint kernel with R (it recomputes the sample).  The ligand's goes in two
    steps: the correlation's adjoint without R writes the gradient of every pose's ROTATED ligand into a workspace of at most
    ``LOCAL_WS_BYTES`` (chunks of poses), and the rotation's adjoint (csrc/dlpd_rotate_grad.h) carries each chunk back through
    its rotations -- summed over the poses, in pose order, for a ligand shared by all of them.  First order; ``T`` receives
    no gradient, and ``R`` only with ``rotation_grad=True``: the same workspace contracted with the derivative of the trilinear
    sample (csrc/dlpd_rotate_rgrad.h) gives the nine numbers of every pose, each from one kernel call -- chunking does not
    change their bits.
    ``shift`` (P, 3) float32, voxels of this call's grid: the rotated ligand displaced by a fraction of a voxel, as
    ``local_correlate`` takes it -- the effective translation of pose p is coarse(T_p) + d + shift_p.  Every gradient above goes
    through the offset kernels (csrc/dlpd_rotate_shift.h), and ``rotation_grad=True`` also differentiates ``shift`` (three more
    numbers per pose from the same kernel call; through off = -M^T shift they reach R too)."""
    if R is None:
        raise RuntimeError("dlpd: local_correlate_rotated needs the rotations R (without them: local_correlate)")
    if shift is not None:
        pose = rotation_grad and torch.is_grad_enabled()
        off = _kernel_offset(_check(R, "R", lib), _check(shift, "shift", lib))
        if pose and (R.requires_grad or off.requires_grad):
            return _LocalCorrelateRotated.apply(receptor, ligand, T, R, int(radius), int(scale), coarse, center, lib, True, off)
        if torch.is_grad_enabled() and any(isinstance(v, torch.Tensor) and v.requires_grad for v in (receptor, ligand)):
            return _LocalCorrelateRotated.apply(receptor, ligand, T, R.detach(), int(radius), int(scale), coarse, center, lib, False,
                                                off.detach())
        return _local_correlate_forward(receptor, ligand, T, R.detach(), radius, scale, coarse, center, lib, off.detach())
    if rotation_grad and torch.is_grad_enabled() and R.requires_grad:
        return _LocalCorrelateRotated.apply(receptor, ligand, T, R, int(radius), int(scale), coarse, center, lib, True)
    if torch.is_grad_enabled() and any(isinstance(v, torch.Tensor) and v.requires_grad for v in (receptor, ligand)):
        return _LocalCorrelateRotated.apply(receptor, ligand, T, R, int(radius), int(scale), coarse, center, lib)
    return _local_correlate_forward(receptor, ligand, T, R, radius, scale, coarse, center, lib)


class _LocalCorrelateRotated(torch.autograd.Function):
    """local_correlate_rotated under autograd (its docstring).  Batching as _LocalCorrelate; the ligand's chunks are bounded by
    the workspace and by dlpd_local_max_poses, and from the second chunk on a shared ligand's sums start at the stored values
    (``accumulate``): the chunked result has the bits of the unsplit one."""

    @staticmethod
    def forward(ctx, receptor, ligand, T, R, radius, scale, coarse, center, lib, rgrad=False, off=None):
        ctx.save_for_backward(receptor, ligand, T, R, off)
        ctx.args = (radius, scale, coarse, center, lib, rgrad)
        return _local_correlate_forward(receptor.detach(), ligand.detach(), T, R.detach(), radius, scale, coarse, center, lib,
                                        None if off is None else off.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gcorr):
        receptor, ligand, T, R, off = ctx.saved_tensors
        r, scale, coarse, center, lib, rgrad = ctx.args
        lib_ = lib or get_lib()
        T = T.contiguous()
        P = T.shape[0]
        rec, rs = _pose_volumes(receptor.detach(), P, "receptor", lib)
        lig, ls = _pose_volumes(ligand.detach(), P, "ligand", lib)
        R = _check(R.detach(), "R", lib)
        g = _check(gcorr, "the gradient", lib)
        C, L, W = rec.shape[-4], rec.shape[-1], 2 * r + 1
        vol = C * L ** 3
        want_rec, want_lig, want_R = ctx.needs_input_grad[0], ctx.needs_input_grad[1], rgrad and ctx.needs_input_grad[3]
        want_off = off is not None and rgrad and ctx.needs_input_grad[10]
        goff = torch.empty(P, 3, dtype=torch.float32, device=rec.device) if want_off else None
        if off is not None:
            off = _check(off.detach(), "the offset", lib)
        gR = torch.empty(P, 3, 3, dtype=torch.float32, device=rec.device) if want_R else None
        grec = torch.empty_like(rec) if want_rec else None
        glig = torch.empty_like(lig) if want_lig else None
        c0 = float(L) / 2.0 if center is None else float(center)
        st = _stream(rec.device)
        most = lib_.call("dlpd_local_max_poses", C, L)

        def run(Rp, out_rec, out_lig, lig_stride, beg, n):
            if off is not None and Rp is not None:
                lib_.call("dlpd_local_correlate_shift_grad", _ptr(rec) + 4 * rs * beg, _ptr(lig) + 4 * ls * beg, Rp,
                          _ptr(off) + 12 * beg, _ptr(T) + 12 * beg, _ptr(g) + 4 * C * W ** 3 * beg, out_rec, out_lig, n, C, L, r,
                          int(scale), COARSE_MODES[coarse], c0, rs, lig_stride, st)
                return
            lib_.call("dlpd_local_correlate_grad", _ptr(rec) + 4 * rs * beg, _ptr(lig) + 4 * ls * beg, Rp, _ptr(T) + 12 * beg,
                      _ptr(g) + 4 * C * W ** 3 * beg, out_rec, out_lig, n, C, L, r, int(scale), COARSE_MODES[coarse], c0, rs,
                      lig_stride, st)
        if want_rec:
            step = most if rs != 0 else P             # a gradient per pose: one launch's poses; a shared receptor: all in one call
            for beg in range(0, P, step):
                run(_ptr(R) + 36 * beg, _ptr(grec) + 4 * rs * beg, None, ls, beg, min(step, P - beg))
        if want_lig or want_R or want_off:
            chunk = max(1, min(P, LOCAL_WS_BYTES // (4 * vol), most))
            ws = torch.empty(chunk * vol, dtype=torch.float32, device=rec.device)
            if off is not None and (want_R or want_off):
                ws_r = torch.empty(_pgrad_ws_bytes(lib_, chunk, L), dtype=torch.uint8, device=rec.device)
            elif want_R:
                ws_r = torch.empty(_rgrad_ws_bytes(lib_, chunk, L), dtype=torch.uint8, device=rec.device)
            for beg in range(0, P, chunk):
                n = min(chunk, P - beg)
                run(None, None, _ptr(ws), vol, beg, n)             # the gradient of each pose's rotated ligand (no ligand is read)
                if off is not None:                                # the same two steps through the offset kernels
                    if want_lig:
                        lib_.call("dlpd_rotate_trilinear_shift_grad", _ptr(ws), _ptr(R) + 36 * beg, _ptr(off) + 12 * beg,
                                  _ptr(glig) + 4 * ls * beg, n, C, L, ls, c0, 1 if (ls == 0 and beg > 0) else 0, st)
                    if want_R or want_off:                         # 12 numbers per pose: the nine of R, the three of the offset
                        lib_.call("dlpd_rotate_trilinear_pgrad", _ptr(ws), _ptr(lig) + 4 * ls * beg, _ptr(R) + 36 * beg,
                                  _ptr(off) + 12 * beg, (_ptr(gR) + 36 * beg) if want_R else None,
                                  (_ptr(goff) + 12 * beg) if want_off else None, _ptr(ws_r), n, C, L, ls, c0, st)
                    continue
                if want_lig:
                    lib_.call("dlpd_rotate_trilinear_grad", _ptr(ws), _ptr(R) + 36 * beg, _ptr(glig) + 4 * ls * beg, n, C, L, ls,
                              c0, 1 if (ls == 0 and beg > 0) else 0, st)
                if want_R:                                         # ... contracted with the sample's derivative: 9 numbers per pose
                    lib_.call("dlpd_rotate_trilinear_rgrad", _ptr(ws), _ptr(lig) + 4 * ls * beg, _ptr(R) + 36 * beg,
                              _ptr(gR) + 36 * beg, _ptr(ws_r), n, C, L, ls, c0, st)
        return grec, glig, None, gR, None, None, None, None, None, None, goff


def local_coarse_radius(radius, scale):
    """Window radius on the coarser grid that covers coarse(t + d) for every |d| <= radius (either convention)."""
    return int(radius) if int(scale) == 1 else (int(radius) + 1) // 2


def local_features(corr0, corr1, T, radius, scale=1, coarse="floor", clip=None):
    """The filter's input rows (P * W^3, C0 + C1) from the window correlations, in torch: for a filter module that has to be
    CALLED (not the reference MLP, or wider than the kernel's hidden widths)."""
    P, C0, W = corr0.shape[0], corr0.shape[1], corr0.shape[2]
    feats = [corr0.reshape(P, C0, -1)]
    if corr1 is not None:
        r, rc = int(radius), local_coarse_radius(radius, scale)
        d = torch.arange(-r, r + 1, device=corr0.device)
        t = T.to(torch.int64)

        def co(v):
            return torch.div(v, int(scale), rounding_mode="floor" if coarse == "floor" else "trunc")
        k = co(t[:, :, None] + d[None, None, :]) - co(t)[:, :, None] + rc               # (P, 3, W)
        Wc = 2 * rc + 1
        flat = ((k[:, 0, :, None, None] * Wc + k[:, 1, None, :, None]) * Wc + k[:, 2, None, None, :]).reshape(P, 1, -1)
        c1 = corr1.reshape(P, corr1.shape[1], -1)
        feats.append(torch.gather(c1, 2, flat.expand(-1, c1.shape[1], -1)))
    f = torch.cat(feats, dim=1)
    if clip is not None:
        f = f.clamp(-float(clip), float(clip))
    return f.permute(0, 2, 1).reshape(P * W ** 3, -1)


def local_filter(corr0, corr1, clash, T, radius, W1, b1, W2, b2, scale=1, coarse="floor", clip=None, threshold=0.0, lib=None):
    """score (P, W, W, W), best score (P), best flat window index (P) int32 from the window correlations of
    ``local_correlate``: clamp, coarse index, SimpleFilter MLP (DockingModels.py:28-32), clash mask (Docker.py:226,232).
    None when the hidden width is beyond the kernel's (the caller then applies its module to ``local_features``)."""
    lib_ = lib or get_lib()
    H = W1.shape[0]
    HP = lib_.call("dlpd_hidden_pad", int(H))
    if HP < 0:
        return None
    corr0 = _check(corr0, "corr0", lib)
    dev = corr0.device
    P, C0, W = corr0.shape[0], corr0.shape[1], corr0.shape[2]
    C1 = 0
    if corr1 is not None:
        corr1 = _check(corr1, "corr1", lib)
        C1 = corr1.shape[1]
    if clash is not None:
        clash = _check(clash, "clash", lib)
    if W1.shape[1] != C0 + C1:
        raise RuntimeError("dlpd: filter width %d does not match %d + %d channels" % (W1.shape[1], C0, C1))
    W1t = torch.zeros(C0 + C1, HP, dtype=torch.float32, device=dev)
    W1t[:, :H] = W1.detach().to(dev, torch.float32).t()
    b1p, W2p = (torch.zeros(HP, dtype=torch.float32, device=dev) for _ in range(2))
    b1p[:H] = b1.detach().to(dev, torch.float32)
    W2p[:H] = W2.detach().to(dev, torch.float32).reshape(-1)
    score = torch.empty(P, W, W, W, dtype=torch.float32, device=dev)
    best = torch.empty(P, dtype=torch.float32, device=dev)
    besti = torch.empty(P, dtype=torch.int32, device=dev)
    T = T.contiguous()
    lib_.call("dlpd_local_filter", _ptr(corr0), C0, _ptr(corr1), C1, _ptr(clash), _ptr(T), P, int(radius), int(scale),
              COARSE_MODES[coarse], _ptr(W1t), _ptr(b1p), _ptr(W2p), float(b2.reshape(-1)[0]), HP, 0 if clip is None else 1,
              float(clip or 0.0), float(threshold), _ptr(score), _ptr(best), _ptr(besti), _stream(dev))
    return score, best, besti


class MultiplyVolumes(nn.Module):
    """The reference's module (src/Models/MultiplyVolumes.py): ``forward(receptor (B, C, L, L, L), ligand (B, C, L, L, L),
    T (B, 3))`` -> (B, C), pair i at translation int(T[i]) (truncation toward zero), by the direct-correlation kernel.
    Differentiable with respect to the two volumes, as ``local_correlate`` is (the adjoint kernel; first order only); T is
    detached and truncated, it has no gradient.  Device tensors (``lib=``: the emulated library of the test-suite, host tensors)."""

    def __init__(self, lib=None):
        super().__init__()
        self.lib = lib

    def forward(self, receptor, ligand, T):
        rec, lig = _check(receptor, "receptor", self.lib), _check(ligand, "ligand", self.lib)
        if rec.dim() != 5 or rec.shape != lig.shape or T.shape[0] != rec.shape[0]:
            raise RuntimeError("dlpd: MultiplyVolumes expects (B, C, L, L, L) pairs and T (B, 3)")
        Ti = torch.as_tensor(T).detach().trunc().to(torch.int32).to(rec.device)
        return local_correlate(rec, lig, Ti, radius=0, scale=1, coarse="trunc", lib=self.lib).reshape(rec.shape[0], rec.shape[1])


# ----------------------------------------------------------------------------------------------------------------------
# Pose clustering (csrc/dlpd_cluster.h; build-defined, the reference has no counterpart)
# ----------------------------------------------------------------------------------------------------------------------
POSE_CLUSTER_MAX = 65536


def pose_embedding(coords, R, t, weights=None, device=None):
    """Rigid poses of ONE ligand as points whose Euclidean distance is the pose RMSD: ``coords`` (n, 3) in Angstrom (centred on
    the origin: the frame the poses ``x -> R x + t`` act in), ``R`` (K, 3, 3), ``t`` (K, 3) in Angstrom, ``weights`` (n) >= 0
    (normalised here to sum 1; None: every atom alike).  With c = sum w x, S = sum w (x - c)(x - c)^T = V L V^T and
    B = V L^(1/2), e_p = (R_p c + t_p, vec(R_p B)) and
        sum_k w_k |(R_i x_k + t_i) - (R_j x_k + t_j)|^2 = |e_i - e_j|^2:
    a translation part and a rotation part, both non-negative (no cancellation between them).  Computed in float64 on the
    host -> (E (K, 12) float32 on ``device`` (default: where ``coords`` lives), M = max|e| -- what the float32 error of a
    distance scales with)."""
    import numpy as np

    def host(a):
        return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)
    if device is None:
        device = coords.device if torch.is_tensor(coords) else "cpu"
    x, Rm, tt = host(coords).reshape(-1, 3), host(R).reshape(-1, 3, 3), host(t).reshape(-1, 3)
    if x.shape[0] == 0 or Rm.shape[0] != tt.shape[0]:
        raise RuntimeError("dlpd: pose_embedding expects coords (n, 3), R (K, 3, 3) and t (K, 3)")
    if weights is None:
        w = np.full(x.shape[0], 1.0 / x.shape[0])
    else:
        w = host(weights).reshape(-1)
        if w.shape[0] != x.shape[0] or (w < 0).any() or not w.sum() > 0:
            raise RuntimeError("dlpd: pose_embedding weights must be (n) non-negative numbers with a positive sum")
        w = w / w.sum()
    c = (w[:, None] * x).sum(axis=0)
    y = x - c
    lam, V = np.linalg.eigh((w[:, None, None] * y[:, :, None] * y[:, None, :]).sum(axis=0))
    B = V * np.sqrt(np.clip(lam, 0.0, None))[None, :]
    E = np.concatenate([Rm @ c + tt, (Rm @ B).reshape(-1, 9)], axis=1)
    M = float(np.abs(E).max()) if E.size else 0.0
    return torch.from_numpy(E.astype(np.float32)).to(device), M


def _embedded(E, name, lib):
    E = _check(E, name, lib)
    if E.dim() != 2 or E.shape[1] != 12 or E.shape[0] == 0:
        raise RuntimeError("dlpd: %s must be (K, 12) embedded poses (ops.pose_embedding), K > 0" % name)
    return E


def pose_rmsd(Ea, Eb=None, lib=None):
    """(Ka, Kb) float32: the RMSD between every pose of ``Ea`` and every pose of ``Eb`` (default: ``Ea`` itself -- then
    symmetric bit for bit, with an exact zero wherever two poses are equal)."""
    lib_ = lib or get_lib()
    Ea = _embedded(Ea, "Ea", lib)
    Eb = Ea if Eb is None else _embedded(Eb, "Eb", lib)
    D = torch.empty(Ea.shape[0], Eb.shape[0], dtype=torch.float32, device=Ea.device)
    lib_.call("dlpd_pose_rmsd", _ptr(Ea), _ptr(Eb), _ptr(D), Ea.shape[0], Eb.shape[0], _stream(Ea.device))
    return D


def pose_within(E, radius, lib=None):
    """The neighbour bitmap alone: (K, ceil(K / 64)) int64 words, bit (j & 63) of word [i, j >> 6] set iff pose j lies
    within ``radius`` of pose i.  For analysis and the tests: it is K^2 / 8 bytes, and ``pose_cluster`` never shows it."""
    lib_ = lib or get_lib()
    E = _embedded(E, "E", lib)
    K = E.shape[0]
    mask = torch.empty(K, (K + 63) // 64, dtype=torch.int64, device=E.device)
    lib_.call("dlpd_pose_within", _ptr(E), K, float(radius), _ptr(mask), _stream(E.device))
    return mask


def pose_cluster(E, radius, max_clusters=None, lib=None):
    """Greedy clustering of a list of embedded poses in ITS order (best first): pose i is a centre iff no earlier centre lies
    within ``radius`` (d <= radius) of it, every other pose joins the first centre within ``radius``; after ``max_clusters``
    centres the scan stops and what they do not cover is labelled -1.  -> (centres (n) list positions, sizes (n), the centre
    included, labels (K) index into centres) int32 on E's device.  The K x K bitmap lives in a workspace on the device
    (K^2 / 8 bytes: 512 MB at K = 65,536, the limit) and is never copied to the host."""
    lib_ = lib or get_lib()
    E = _embedded(E, "E", lib)
    K, dev = E.shape[0], E.device
    if K > POSE_CLUSTER_MAX:
        raise RuntimeError("dlpd: pose_cluster takes at most %d poses, got %d" % (POSE_CLUSTER_MAX, K))
    m = K if max_clusters is None else int(max_clusters)
    if m <= 0:
        raise RuntimeError("dlpd: pose_cluster max_clusters must be positive")
    m = min(m, K)
    nbytes = lib_.call("dlpd_pose_cluster_ws", K)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    centres = torch.empty(m, dtype=torch.int32, device=dev)
    sizes = torch.empty(m, dtype=torch.int32, device=dev)
    labels = torch.empty(K, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    lib_.call("dlpd_pose_cluster", _ptr(E), K, float(radius), m, _ptr(centres), _ptr(sizes), _ptr(labels), _ptr(count), _ptr(ws),
              nbytes, _stream(dev))
    n = int(count.item())
    return centres[:n], sizes[:n], labels


# ----------------------------------------------------------------------------------------------------------------------
# Pose evaluation against a native complex (csrc/dlpd_evaluate.h)
# ----------------------------------------------------------------------------------------------------------------------
EVAL_REC = 48                     # doubles per record of the moment block
EVAL_MAX_INTERFACES = 16
EVAL_MAX_LIGAND_ATOMS = 2048


def _fsum_columns(X):
    import math
    import numpy as np
    return np.array([math.fsum(X[:, j]) for j in range(X.shape[1])], dtype=np.float64)


def _centred(X):
    """(n, 3) float64 -> (X about its mean, the mean).  Two passes: the first mean is exact to a rounding of its size, the second
    removes what that rounding left, so the rows sum to zero to a rounding of a CENTRED coordinate."""
    import numpy as np
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    if X.shape[0] == 0:
        return X, np.zeros(3)
    c1 = _fsum_columns(X) / X.shape[0]
    X1 = X - c1
    c2 = _fsum_columns(X1) / X.shape[0]
    return X1 - c2, c1 + c2


def _moment(X, Y):
    """sum_k X[k, i] Y[k, j] -> (3, 3): every product rounded once, the sum exact (math.fsum) and rounded once"""
    import math
    import numpy as np
    out = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            out[i, j] = math.fsum(X[:, i] * Y[:, j])
    return out


def native_moments(pairs, ligand_ca, target_ca):
    """The moment block of a target for ``pose_native_rmsd``: host float64 packing, no device work.
    ``pairs``: [(a (nr, 3), y (nl, 3), q (nr + nl, 3))], one entry per interface pair -- the receptor's interface points in the
    docking frame, the ligand's in ITS frame (a pose carries y to R y + t) and the static points of the native complex,
    receptor rows first, in any frame (nr >= 0, nl >= 1, at most 16 pairs).  ``ligand_ca`` (m, 3) / ``target_ca`` (m, 3): the
    points of the ligand RMSD in the ligand's frame and where the native puts them in the docking frame.
    Every point set is taken about its own centroid (two-pass, so the centred rows sum to zero to a rounding of themselves):
    a common shift of the mobile set changes no superposed RMSD, and the centroids go into the block so that the kernel adds
    R cy - ca to a pose's translation.  Sums of products are exact sums (math.fsum) of once-rounded products: the error of a
    moment does not grow with the number of points.
    -> (moments (nI + 1, 48) float64: nI interface records  A[9] Y[9] s[3] sa[3] sy[3] Saa Syy Gq ca[3] cy[3] Cyy[6]  with
    A = sum a q^T, Y = sum y q^T, s = sum_lig q, sa = sum a, sy = sum y, Cyy = sum y y^T (xx xy xz yy yz zz: a pose's matrix
    need not be a rotation to the last bit, the kernel takes sum |R y|^2 from it), then the ligand record  M[9] sy[3] sz[3] Syy
    Szz cy[3] cz[3] Cyy[6]  with M = sum z y^T;  counts (nI + 1, 2) int32: (nr, nl) of every record)."""
    import math
    import numpy as np
    pairs = list(pairs)
    if not 1 <= len(pairs) <= EVAL_MAX_INTERFACES:
        raise RuntimeError("dlpd: native_moments takes 1 to %d interface pairs, got %d" % (EVAL_MAX_INTERFACES, len(pairs)))
    nI = len(pairs)
    mom, counts = np.zeros((nI + 1, EVAL_REC)), np.zeros((nI + 1, 2), dtype=np.int32)
    for p, (a, y, q) in enumerate(pairs):
        a, ca = _centred(a)
        y, cy = _centred(y)
        q, _ = _centred(q)
        nr, nl = a.shape[0], y.shape[0]
        if nl < 1 or q.shape[0] != nr + nl:
            raise RuntimeError("dlpd: interface pair %d needs nl >= 1 ligand points and nr + nl static points" % p)
        rec = mom[p]
        rec[0:9] = _moment(a, q[:nr]).reshape(-1)
        rec[9:18] = _moment(y, q[nr:]).reshape(-1)
        rec[18:21] = _fsum_columns(q[nr:])
        rec[21:24] = _fsum_columns(a) if nr else 0.0
        rec[24:27] = _fsum_columns(y)
        rec[27], rec[28], rec[29] = math.fsum((a * a).reshape(-1)), math.fsum((y * y).reshape(-1)), math.fsum((q * q).reshape(-1))
        rec[30:33], rec[33:36] = ca, cy
        rec[36:42] = _moment(y, y)[np.triu_indices(3)]
        counts[p] = (nr, nl)
    y, cy = _centred(ligand_ca)
    z, cz = _centred(target_ca)
    if y.shape[0] < 1 or y.shape != z.shape:
        raise RuntimeError("dlpd: native_moments needs ligand_ca and target_ca of one shape (m, 3), m >= 1")
    rec = mom[nI]
    rec[0:9] = _moment(z, y).reshape(-1)
    rec[9:12], rec[12:15] = _fsum_columns(y), _fsum_columns(z)
    rec[15], rec[16] = math.fsum((y * y).reshape(-1)), math.fsum((z * z).reshape(-1))
    rec[17:20], rec[20:23] = cy, cz
    rec[23:29] = _moment(y, y)[np.triu_indices(3)]
    counts[nI] = (0, y.shape[0])
    return mom, counts


def _poses64(poses, lib, device=None):
    import numpy as np
    if not torch.is_tensor(poses):
        poses = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float64)))
    if device is not None:
        poses = poses.to(device)
    if not ((poses.is_cuda or lib is not None) and poses.dtype == torch.float64 and poses.dim() == 2 and poses.shape[1] == 12
            and poses.shape[0] > 0):
        raise RuntimeError("dlpd: poses must be (K, 12) float64 (R row-major, then t) on the device, K > 0; there is no CPU path")
    return poses.contiguous()


def _on(t, dtype, dev, name, lib):
    if not (torch.is_tensor(t) and t.dtype == dtype and t.device == dev and (t.is_cuda or lib is not None)):
        raise RuntimeError("dlpd: %s must be a %s tensor on the poses' device" % (name, str(dtype).replace("torch.", "")))
    return t.contiguous()


def pose_native_rmsd(poses, moments, counts, lib=None):
    """(irmsd (K), lrmsd (K)) float64 on the poses' device: the interface RMSD (minimum over the interface pairs of the RMSD
    after the best rigid superposition) and the ligand RMSD (no superposition) of K poses, from the moment block of
    ``native_moments`` -- ``moments`` (nI + 1, 48) float64 on the device, ``counts`` (nI + 1, 2) host integers."""
    import numpy as np
    lib_ = lib or get_lib()
    poses = _poses64(poses, lib)
    moments = _on(moments, torch.float64, poses.device, "moments", lib)
    counts = np.ascontiguousarray(np.asarray(counts, dtype=np.int32))
    nI = counts.shape[0] - 1
    if counts.ndim != 2 or counts.shape[1] != 2 or tuple(moments.shape) != (nI + 1, EVAL_REC):
        raise RuntimeError("dlpd: pose_native_rmsd expects moments (nI + 1, %d) and counts (nI + 1, 2)" % EVAL_REC)
    K = poses.shape[0]
    irmsd = torch.empty(K, dtype=torch.float64, device=poses.device)
    lrmsd = torch.empty(K, dtype=torch.float64, device=poses.device)
    lib_.call("dlpd_pose_native_rmsd", _ptr(poses), K, _ptr(moments), counts.ctypes.data, nI, _ptr(irmsd), _ptr(lrmsd),
              _stream(poses.device))
    return irmsd, lrmsd


def pose_native_contacts(poses, rec_atoms, lig_atoms, ranges, ranges_host, cutoff, lib=None):
    """count (K) int32: how many of the C native contacts hold under each pose.  ``rec_atoms`` (NRa, 3) / ``lig_atoms`` (NLa, 3)
    float32 on the device, residue-contiguous (the receptor's in the docking frame, the ligand's in its own); contact c is the
    atom ranges rec [r0, r1) x lig [l0, l1): ``ranges`` (C, 4) int32 on the device, ``ranges_host`` the same array on the host
    (the library checks that one); it holds iff some atom pair lies within ``cutoff`` (d^2 <= cutoff^2 in float32)."""
    import numpy as np
    lib_ = lib or get_lib()
    poses = _poses64(poses, lib)
    dev = poses.device
    rec_atoms = _on(rec_atoms, torch.float32, dev, "rec_atoms", lib).reshape(-1, 3)
    lig_atoms = _on(lig_atoms, torch.float32, dev, "lig_atoms", lib).reshape(-1, 3)
    ranges = _on(ranges, torch.int32, dev, "ranges", lib).reshape(-1, 4)
    ranges_host = np.ascontiguousarray(np.asarray(ranges_host, dtype=np.int32)).reshape(-1, 4)
    C = ranges_host.shape[0]
    if ranges.shape[0] != C:
        raise RuntimeError("dlpd: ranges and ranges_host must hold the same (C, 4) contacts")
    K = poses.shape[0]
    count = torch.empty(K, dtype=torch.int32, device=dev)
    lib_.call("dlpd_pose_native_contacts", _ptr(poses), K, _ptr(rec_atoms), rec_atoms.shape[0], _ptr(lig_atoms), lig_atoms.shape[0],
              _ptr(ranges), ranges_host.ctypes.data, C, float(cutoff), _ptr(count), _stream(dev))
    return count


def pose_capri(count, irmsd, lrmsd, C, lib=None):
    """(fnat (K) float64 = count / (C + 0.001), capri (K) int32): the class starts at 0 and is set to 1, 2, 3 by three
    successive ifs ``(fnat >= a and lrmsd <= b) or irmsd <= c`` with (a, b, c) = (0.1, 10, 4), (0.3, 5, 2), (0.5, 1, 1)."""
    lib_ = lib or get_lib()
    dev = count.device
    count = _on(count, torch.int32, dev, "count", lib)
    irmsd, lrmsd = _on(irmsd, torch.float64, dev, "irmsd", lib), _on(lrmsd, torch.float64, dev, "lrmsd", lib)
    K = count.shape[0]
    if K == 0 or irmsd.shape[0] != K or lrmsd.shape[0] != K:
        raise RuntimeError("dlpd: pose_capri expects count, irmsd and lrmsd of one length K > 0")
    fnat = torch.empty(K, dtype=torch.float64, device=dev)
    capri = torch.empty(K, dtype=torch.int32, device=dev)
    lib_.call("dlpd_pose_capri", _ptr(count), _ptr(irmsd), _ptr(lrmsd), int(C), K, _ptr(fnat), _ptr(capri), _stream(dev))
    return fnat, capri


def pose_evaluate(poses, native, lib=None):
    """(irmsd, lrmsd, fnat, capri) of K poses ((K, 12) float64: R row-major, then t in Angstrom, in the frame of a .dat file)
    against ``native``, a ``Results.InterfaceSelection.NativeReference`` on the device the poses are on (an array of poses is
    moved there).  Three launches on one stream; only K-sized results exist."""
    poses = _poses64(poses, lib, device=native.device)
    irmsd, lrmsd = pose_native_rmsd(poses, native.moments, native.counts, lib=lib)
    count = pose_native_contacts(poses, native.rec_atoms, native.lig_atoms, native.ranges, native.ranges_host, native.contact_dist,
                                 lib=lib)
    fnat, capri = pose_capri(count, irmsd, lrmsd, native.C, lib=lib)
    return irmsd, lrmsd, fnat, capri


# ----------------------------------------------------------------------------------------------------------------------
# Every residue contact of a posed complex: n_dec, n_corr and fnonnat (csrc/dlpd_contacts.h)
# ----------------------------------------------------------------------------------------------------------------------
CONT_MAX_LIGAND_ATOMS, CONT_MAX_LIGAND_RESIDUES = 8192, 1024
CONT_MAX_RECEPTOR_ATOMS, CONT_MAX_RECEPTOR_RESIDUES = 65536, 8192


def _round_up32(x):
    """the least float32 >= x that is safely above it (a float32 conversion rounds down by half a step at most)"""
    import numpy as np
    return np.nextafter(np.asarray(x, dtype=np.float64).astype(np.float32), np.float32(np.inf))


def _bounding_spheres(atoms32, off):
    """(nres, 4) float32: the centroid of every residue's float32 atoms, rounded to float32, and a radius, rounded UP, that
    covers them about that rounded centre (float64 on the float32 values); an empty residue: zeros"""
    import numpy as np
    a64 = atoms32.astype(np.float64)
    out = np.zeros((len(off) - 1, 4), dtype=np.float32)
    for i in range(len(off) - 1):
        x = a64[off[i]:off[i + 1]]
        if len(x):
            c = x.mean(axis=0).astype(np.float32)
            out[i, :3] = c
            out[i, 3] = _round_up32(np.sqrt(((x - c.astype(np.float64)) ** 2).sum(axis=1)).max())
    return out


def contact_tables(rec_atoms, rec_off, lig_atoms, lig_off, native_pairs):
    """What ``pose_contact_counts`` reads of one target, packed once on the host: ``rec_atoms`` (NRa, 3) / ``lig_atoms``
    (NLa, 3) float32, every atom, residue-contiguous (receptor in the docking frame, ligand in its own); ``rec_off`` /
    ``lig_off`` int32 residue offsets with their host copies; ``rec_sph`` (NRres, 4) / ``lig_sph`` (NLres + 1, 4) bounding
    spheres (the last ligand row: the whole ligand); ``lig_extent``; ``native_bits``: the native pairs -- (receptor residue,
    ligand residue) indices, a pair named twice counts once -- as a bitmap over (lambda, rho), int32 words.  -> dict (tensors
    on the CPU)."""
    import numpy as np
    ra = np.ascontiguousarray(np.asarray(rec_atoms, dtype=np.float64).reshape(-1, 3).astype(np.float32))
    la = np.ascontiguousarray(np.asarray(lig_atoms, dtype=np.float64).reshape(-1, 3).astype(np.float32))
    ro = np.ascontiguousarray(np.asarray(rec_off, dtype=np.int32).reshape(-1))
    lo = np.ascontiguousarray(np.asarray(lig_off, dtype=np.int32).reshape(-1))
    nr, nl = len(ro) - 1, len(lo) - 1
    if nr < 1 or nl < 1 or ro[0] != 0 or lo[0] != 0 or ro[-1] != len(ra) or lo[-1] != len(la) or (np.diff(ro) < 0).any() or (np.diff(lo) < 0).any() \
            or not len(ra) or not len(la):
        raise RuntimeError("dlpd: contact_tables needs non-empty atom arrays and offsets 0 = off[0] <= ... <= off[nres] = natoms")
    rs, ls = _bounding_spheres(ra, ro), _bounding_spheres(la, lo)
    ls = np.concatenate([ls, _bounding_spheres(la, np.array([0, len(la)]))])
    extent = float(_round_up32(max(np.sqrt((la.astype(np.float64) ** 2).sum(axis=1)).max(), np.sqrt((ls[:, :3].astype(np.float64) ** 2).sum(axis=1)).max())))
    W = (nr + 31) // 32
    bits = np.zeros(nl * W, dtype=np.uint32)
    for rho, lam in native_pairs:
        if not (0 <= rho < nr and 0 <= lam < nl):
            raise RuntimeError("dlpd: native pair (%d, %d) outside the %d x %d residues" % (rho, lam, nr, nl))
        bits[lam * W + (rho >> 5)] |= np.uint32(1 << (rho & 31))
    t = torch.from_numpy
    return {"rec_atoms": t(ra), "rec_off": t(ro), "rec_sph": t(rs), "lig_atoms": t(la), "lig_off": t(lo), "lig_sph": t(np.ascontiguousarray(ls)),
            "native_bits": t(bits.view(np.int32)), "rec_off_host": ro.copy(), "lig_off_host": lo.copy(), "lig_extent": extent,
            "n_native": int(sum(bin(int(w)).count("1") for w in bits))}


def pose_contact_counts(poses, native, lib=None):
    """(n_dec (K), n_corr (K)) int32 on the poses' device: under each pose the number of residue pairs of the two unbound
    structures with an atom pair within ``native.contact_dist`` -- every atom of both, the predicate of ``pose_native_contacts``
    bit for bit -- and how many of them are native pairs.  ``native``: a NativeReference built with ``all_contacts=True``."""
    tb = getattr(native, "all", None)
    if tb is None:
        raise RuntimeError("dlpd: pose_contact_counts needs a native reference built with all_contacts=True")
    lib_ = lib or get_lib()
    poses = _poses64(poses, lib, device=native.device)
    dev = poses.device
    ra, la = _on(tb["rec_atoms"], torch.float32, dev, "rec_atoms", lib), _on(tb["lig_atoms"], torch.float32, dev, "lig_atoms", lib)
    ro, lo = _on(tb["rec_off"], torch.int32, dev, "rec_off", lib), _on(tb["lig_off"], torch.int32, dev, "lig_off", lib)
    rs, ls = _on(tb["rec_sph"], torch.float32, dev, "rec_sph", lib), _on(tb["lig_sph"], torch.float32, dev, "lig_sph", lib)
    bits = _on(tb["native_bits"], torch.int32, dev, "native_bits", lib)
    roh, loh = tb["rec_off_host"], tb["lig_off_host"]
    NRa, NLa, NRres, NLres = ra.shape[0], la.shape[0], roh.shape[0] - 1, loh.shape[0] - 1
    if ro.numel() != NRres + 1 or lo.numel() != NLres + 1 or tuple(rs.shape) != (NRres, 4) or tuple(ls.shape) != (NLres + 1, 4) \
            or bits.numel() != NLres * ((NRres + 31) // 32) or int(roh[-1]) != NRa or int(loh[-1]) != NLa:
        raise RuntimeError("dlpd: the all-contacts tables of this native reference do not belong together")
    K = poses.shape[0]
    n_dec = torch.empty(K, dtype=torch.int32, device=dev)
    n_corr = torch.empty(K, dtype=torch.int32, device=dev)
    lib_.call("dlpd_pose_contacts_all", _ptr(poses), K, _ptr(ra), _ptr(ro), _ptr(rs), NRa, NRres, _ptr(la), _ptr(lo), _ptr(ls), NLa, NLres,
              roh.ctypes.data, loh.ctypes.data, _ptr(bits), float(tb["lig_extent"]), float(native.contact_dist), _ptr(n_dec), _ptr(n_corr),
              _stream(dev))
    return n_dec, n_corr


def fnonnat_of(n_dec, n_corr):
    """(n_dec - n_corr) / (n_dec + 0.001) in float64: ``_get_fnat``'s second value (processing_utils.py:219-224)"""
    return (n_dec - n_corr).double() / (n_dec.double() + 0.001)


def pose_fnonnat(poses, native, lib=None):
    """fnonnat (K) float64 on the poses' device: the share of a pose's residue contacts that the native complex does not have"""
    return fnonnat_of(*pose_contact_counts(poses, native, lib=lib))


# ----------------------------------------------------------------------------------------------------------------------
# The interface of every pose as residue bitmaps: frequencies over a list, clustering by interface (csrc/dlpd_interface.h;
# DESIGN.md 4n; build-defined)
# ----------------------------------------------------------------------------------------------------------------------
INTERFACE_Q_ONE = 1024


def _contact_tables_on(tables, dev, lib):
    """the tensors of ``contact_tables`` (a dict, or an object that carries one as ``.all``) checked against each other"""
    tb = tables if isinstance(tables, dict) else getattr(tables, "all", None)
    if tb is None:
        raise RuntimeError("dlpd: pose_interface_bits needs the tables of ops.contact_tables (a ComplexReference, or a native "
                           "reference built with all_contacts=True)")
    ra, la = _on(tb["rec_atoms"], torch.float32, dev, "rec_atoms", lib), _on(tb["lig_atoms"], torch.float32, dev, "lig_atoms", lib)
    ro, lo = _on(tb["rec_off"], torch.int32, dev, "rec_off", lib), _on(tb["lig_off"], torch.int32, dev, "lig_off", lib)
    rs, ls = _on(tb["rec_sph"], torch.float32, dev, "rec_sph", lib), _on(tb["lig_sph"], torch.float32, dev, "lig_sph", lib)
    roh, loh = tb["rec_off_host"], tb["lig_off_host"]
    NRa, NLa, NRres, NLres = ra.shape[0], la.shape[0], roh.shape[0] - 1, loh.shape[0] - 1
    if ro.numel() != NRres + 1 or lo.numel() != NLres + 1 or tuple(rs.shape) != (NRres, 4) or tuple(ls.shape) != (NLres + 1, 4) \
            or int(roh[-1]) != NRa or int(loh[-1]) != NLa:
        raise RuntimeError("dlpd: these contact tables do not belong together")
    return tb, ra, ro, rs, la, lo, ls, roh, loh


def pose_interface_bits(poses, tables, cutoff, lib=None):
    """(rec_bits (K, ceil(NRres / 32)), lig_bits (K, ceil(NLres / 32))) int32 on the poses' device: bit (i & 31) of word i >> 5 of
    row k is set iff residue i of that protein has an atom within ``cutoff`` of some atom of the partner under pose k -- every
    atom of both, the predicate of ``pose_contact_counts`` bit for bit; the bits past the last residue are zero.  ``tables``:
    the dict of ``contact_tables`` (its native pairs are not read) or an object that carries it as ``.all``, on the poses'
    device (an array of poses is moved to the tables').  No poses: empty bitmaps, no launch."""
    import numpy as np
    tb = tables if isinstance(tables, dict) else getattr(tables, "all", None)
    if not torch.is_tensor(poses):
        poses = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 12)))
        if tb is not None:
            poses = poses.to(tb["rec_atoms"].device)
    dev = poses.device
    tb, ra, ro, rs, la, lo, ls, roh, loh = _contact_tables_on(tables, dev, lib)
    NRres, NLres = roh.shape[0] - 1, loh.shape[0] - 1
    K = poses.shape[0]
    if K > POSE_CLUSTER_MAX:
        raise RuntimeError("dlpd: pose_interface_bits takes at most %d poses, got %d" % (POSE_CLUSTER_MAX, K))
    rec_bits = torch.empty(K, (NRres + 31) // 32, dtype=torch.int32, device=dev)
    lig_bits = torch.empty(K, (NLres + 31) // 32, dtype=torch.int32, device=dev)
    if K == 0:
        return rec_bits, lig_bits
    lib_ = lib or get_lib()
    poses = _poses64(poses, lib)
    lib_.call("dlpd_pose_residue_bits", _ptr(poses), K, _ptr(ra), _ptr(ro), _ptr(rs), ra.shape[0], NRres, _ptr(la), _ptr(lo), _ptr(ls),
              la.shape[0], NLres, roh.ctypes.data, loh.ctypes.data, float(tb["lig_extent"]), float(cutoff), _ptr(rec_bits), _ptr(lig_bits),
              _stream(dev))
    return rec_bits, lig_bits


def _interface_bits(rec_bits, lig_bits, lib):
    if not (torch.is_tensor(rec_bits) and torch.is_tensor(lig_bits) and rec_bits.dtype == torch.int32 and lig_bits.dtype == torch.int32
            and rec_bits.dim() == 2 and lig_bits.dim() == 2 and rec_bits.shape[0] == lig_bits.shape[0]
            and rec_bits.device == lig_bits.device and (rec_bits.is_cuda or lib is not None)):
        raise RuntimeError("dlpd: rec_bits (K, Wr) and lig_bits (K, Wl) must be int32 bitmaps of the same poses on one device "
                           "(ops.pose_interface_bits); there is no CPU path")
    return rec_bits.contiguous(), lig_bits.contiguous()


def unpack_bits(bits, n):
    """(K, W) int32 bitmap words -> (K, n) bool on the same device: column i is bit (i & 31) of word i >> 5"""
    K = bits.shape[0]
    if n > 32 * bits.shape[1]:
        raise RuntimeError("dlpd: unpack_bits: %d words hold no %d bits" % (bits.shape[1], n))
    shifts = torch.arange(32, dtype=torch.int32, device=bits.device)
    return ((bits[:, :, None] >> shifts[None, None, :]) & 1).bool().reshape(K, -1)[:, :n]


def interface_profile(rec_bits, lig_bits, NRres, NLres, weights=None, lib=None):
    """Over the K poses of the two bitmaps -> (rec_freq (NRres), lig_freq (NLres) float64, rec_count, lig_count int32) on
    their device: how many poses mark a residue, and the sum of ``weights`` (K numbers, any values; None: 1 / K each) over
    those poses.  The sum's order depends on K alone -- chunks of 1,024 poses, ascending inside a chunk, the chunk partials
    added in ascending order -- so two runs give the same bytes and a host loop in that order reproduces them.  No poses:
    zeros, no launch."""
    import numpy as np
    rec_bits, lig_bits = _interface_bits(rec_bits, lig_bits, lib)
    NRres, NLres = int(NRres), int(NLres)
    K, dev = rec_bits.shape[0], rec_bits.device
    if NRres < 1 or NLres < 1 or rec_bits.shape[1] != (NRres + 31) // 32 or lig_bits.shape[1] != (NLres + 31) // 32:
        raise RuntimeError("dlpd: interface_profile: the bitmaps' widths are not those of %d and %d residues" % (NRres, NLres))
    rec_freq, lig_freq = torch.zeros(NRres, dtype=torch.float64, device=dev), torch.zeros(NLres, dtype=torch.float64, device=dev)
    rec_count, lig_count = torch.zeros(NRres, dtype=torch.int32, device=dev), torch.zeros(NLres, dtype=torch.int32, device=dev)
    if K == 0:
        return rec_freq, lig_freq, rec_count, lig_count
    if weights is None:
        w = torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev)
    else:
        if not torch.is_tensor(weights):
            weights = torch.from_numpy(np.ascontiguousarray(np.asarray(weights, dtype=np.float64)))
        w = weights.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(w.shape) != (K,):
            raise RuntimeError("dlpd: interface_profile weights must be %d numbers, one per pose" % K)
    lib_ = lib or get_lib()
    nbytes = lib_.call("dlpd_interface_profile_ws", K, NRres, NLres)
    if nbytes == 0:
        raise RuntimeError("dlpd: interface_profile takes at most %d poses, %d and %d residues" %
                           (POSE_CLUSTER_MAX, CONT_MAX_RECEPTOR_RESIDUES, CONT_MAX_LIGAND_RESIDUES))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    lib_.call("dlpd_interface_profile", _ptr(rec_bits), _ptr(lig_bits), K, NRres, NLres, _ptr(w), _ptr(rec_freq), _ptr(lig_freq),
              _ptr(rec_count), _ptr(lig_count), _ptr(ws), nbytes, _stream(dev))
    return rec_freq, lig_freq, rec_count, lig_count


def interface_q(threshold):
    """the integer the kernels compare with: poses i, j are neighbours iff |F_i & F_j| * 1024 >= q * |F_i | F_j|,
    q = round(1024 * threshold), threshold (a Jaccard index) in [0, 1]"""
    t = float(threshold)
    if not 0.0 <= t <= 1.0:
        raise RuntimeError("dlpd: the interface similarity threshold is a Jaccard index in [0, 1], got %r" % (threshold,))
    return int(round(t * INTERFACE_Q_ONE))


def interface_within(rec_bits, lig_bits, threshold, lib=None):
    """The neighbour bitmap of interface similarity alone, in the layout of ``pose_within``: (K, ceil(K / 64)) int64 words, bit
    (j & 63) of word [i, j >> 6] set iff the residue sets of poses i and j (both proteins' together) have a Jaccard index
    >= ``threshold`` (``interface_q``); two empty sets are neighbours.  For analysis and the tests."""
    rec_bits, lig_bits = _interface_bits(rec_bits, lig_bits, lib)
    q = interface_q(threshold)
    K, dev = rec_bits.shape[0], rec_bits.device
    mask = torch.empty(K, (K + 63) // 64, dtype=torch.int64, device=dev)
    if K == 0:
        return mask
    (lib or get_lib()).call("dlpd_interface_within", _ptr(rec_bits) if rec_bits.shape[1] else None, _ptr(lig_bits) if lig_bits.shape[1] else None,
                            K, rec_bits.shape[1], lig_bits.shape[1], q, _ptr(mask), _stream(dev))
    return mask


def interface_cluster(rec_bits, lig_bits, threshold, max_clusters=None, lib=None):
    """Greedy clustering of a list, in ITS order, by the similarity of the poses' interfaces (``interface_within``): pose i is
    a centre iff no earlier centre is its neighbour, every other pose joins the first centre that is.  -> (centres, sizes,
    labels) as ``pose_cluster`` returns them; the K x K bitmap stays in a workspace on the device."""
    rec_bits, lig_bits = _interface_bits(rec_bits, lig_bits, lib)
    q = interface_q(threshold)
    K, dev = rec_bits.shape[0], rec_bits.device
    if K > POSE_CLUSTER_MAX:
        raise RuntimeError("dlpd: interface_cluster takes at most %d poses, got %d" % (POSE_CLUSTER_MAX, K))
    m = K if max_clusters is None else int(max_clusters)
    if max_clusters is not None and m <= 0:
        raise RuntimeError("dlpd: interface_cluster max_clusters must be positive")
    m = min(m, K)
    centres = torch.empty(m, dtype=torch.int32, device=dev)
    sizes = torch.empty(m, dtype=torch.int32, device=dev)
    labels = torch.empty(K, dtype=torch.int32, device=dev)
    if K == 0:
        return centres, sizes, labels
    lib_ = lib or get_lib()
    nbytes = lib_.call("dlpd_pose_cluster_ws", K)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    lib_.call("dlpd_interface_cluster", _ptr(rec_bits) if rec_bits.shape[1] else None, _ptr(lig_bits) if lig_bits.shape[1] else None, K,
              rec_bits.shape[1], lig_bits.shape[1], q, m, _ptr(centres), _ptr(sizes), _ptr(labels), _ptr(count), _ptr(ws), nbytes,
              _stream(dev))
    n = int(count.item())
    return centres[:n], sizes[:n], labels
