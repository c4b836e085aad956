"""Scoring model with the reference's plugin surface.

Surface kept from /root/reference/src/Models/DockingModels.py:23-84 so that checkpoints and callers
carry over: ``SimpleFilter(inputs_sizes)`` owns ``fc = [Linear(C, C//2), ReLU, Linear(C//2, 1)]``
(state-dict keys ``fc.0.*`` / ``fc.2.*``, Xavier-uniform weights); ``GlobalDockingModel`` exposes
``.representation``, ``.filter``, ``.threshold_clash``, ``forward(receptor_volumes, ligand_volumes)``
and ``save/load(directory, epoch)`` writing ``<name>_repr_epochN.th`` / ``<name>_filter_epochN.th``.

What differs is where the arithmetic runs: ``forward`` is one VolumeConvolution(clip) per resolution
(HIP K1+K2+K3) and, for the reference's MLP filter, ONE kernel for nearest-upsample + concat + MLP
instead of interpolate / cat / three transposes / two GEMMs (DockingModels.py:74-83).  ``filter`` may
be ANY module mapping (voxels, channels) -> (voxels, 1) (DockingModels.py:82): a filter that is not
that MLP is called on the reference's own channels-last layout.
``GlobalDockingModel(differentiable=True)`` is the model that is trained: under autograd its correlations are the
differentiable ``VolumeConvolution`` (the adjoint FFT kernels of csrc/dlpd_corr_grad.h) and its filter is called, so a loss
over the whole (2L)^3 translation grid reaches the filter's and the representation's parameters.  With ``fused_filter_grad=True``
as well, the reference's MLP filter is not called there either: it runs as ``ops.filter_volumes_autograd``, the inference
kernel with the backward kernel of csrc/dlpd_filter_grad.h.
"""
import os

import torch
from torch import nn

from deeplocalproteindocking_amd.ops import (MultiplyVolumes, VolumeConvolution, VolumeRotation, filter_grad_supported,
                                             filter_volumes, filter_volumes_autograd, local_correlate_rotated, local_filter)
from deeplocalproteindocking_amd.Utils.Conventions import rotation_pivot


def init_weights(module):
    """Xavier-uniform on every Linear / Conv3d weight (DockingModels.py:17-21)."""
    if isinstance(module, (nn.Linear, nn.Conv3d)):
        nn.init.xavier_uniform_(module.weight)


class SimpleFilter(nn.Module):
    """Per-translation scorer: concatenated correlation channels -> hidden (half as wide) -> score."""

    def __init__(self, inputs_sizes):
        super().__init__()
        width = int(sum(int(c) for c in inputs_sizes))
        hidden = width // 2
        self.fc_input_size = width
        self.fc = nn.Sequential(nn.Linear(width, hidden), nn.ReLU(), nn.Linear(hidden, 1))
        self.fc.apply(init_weights)

    def forward(self, input):
        return self.fc(input)

    def parameters_tuple(self):
        """(W1 (H,C), b1 (H), W2 (1,H), b2 (1)), detached, for the fused kernels."""
        first, last = self.fc[0], self.fc[2]
        return tuple(t.detach() for t in (first.weight, first.bias, last.weight, last.bias))


def mlp_parameters(filt):
    """(W1 (H,C), b1 (H), W2 (1,H), b2 (1)) when ``filt`` is the reference's SimpleFilter
    (DockingModels.py:23-37: ``fc = [Linear(C,H), ReLU, Linear(H,1)]`` applied as is) -- this build's
    class or a same-named class of the same structure, e.g. the reference's own; None for any other
    module, which then has to be called."""
    if hasattr(filt, "parameters_tuple"):
        return filt.parameters_tuple()
    fc = getattr(filt, "fc", None)
    if (type(filt).__name__ == "SimpleFilter" and isinstance(fc, nn.Sequential) and len(fc) == 3
            and isinstance(fc[0], nn.Linear) and isinstance(fc[1], nn.ReLU) and isinstance(fc[2], nn.Linear)
            and fc[2].out_features == 1 and fc[0].bias is not None and fc[2].bias is not None):
        return tuple(t.detach() for t in (fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias))
    return None


def live_mlp_parameters(filt):
    """The test of ``mlp_parameters`` with the LIVE parameters (W1, b1, W2, b2) of ``fc[0]`` / ``fc[2]``, for the filter kernel
    that has a backward (ops.filter_volumes_autograd); None for any other module."""
    fc = getattr(filt, "fc", None)
    if (type(filt).__name__ == "SimpleFilter" and isinstance(fc, nn.Sequential) and len(fc) == 3
            and isinstance(fc[0], nn.Linear) and isinstance(fc[1], nn.ReLU) and isinstance(fc[2], nn.Linear)
            and fc[2].out_features == 1 and fc[0].bias is not None and fc[2].bias is not None):
        return fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias
    return None


def fused_filter_parameters(model):
    """Filter parameters when ``model(receptor_volumes, ligand_volumes)`` (Docker.py:229) IS the
    reference's ``GlobalDockingModel.forward`` (DockingModels.py:63-84: per-channel correlation,
    nearest upsample, concat) followed by an MLP filter -- what the fused kernels compute; None when
    the model brings a forward of its own or another filter, and therefore must be called."""
    cls = type(model)
    fwd = getattr(cls, "forward", None)
    has_own_call = (isinstance(model, nn.Module) and fwd is not None and fwd is not nn.Module.forward
                    and fwd is not getattr(nn.Module, "_forward_unimplemented", None)) or \
                   (not isinstance(model, nn.Module) and callable(model))
    # (a marker on the function, not a class identity test: the package is importable both as
    # ``Models`` -- the reference's import path -- and as ``deeplocalproteindocking_amd.Models``)
    if has_own_call and not getattr(fwd, "dlpd_reference_forward", False):
        return None
    filt = getattr(model, "filter", None)
    return None if filt is None else mlp_parameters(filt)


class GlobalDockingModel(nn.Module):
    FILES = ("%s_repr_epoch%d.th", "%s_filter_epoch%d.th")

    def __init__(self, representation, filter, threshold_clash=300, normalize=False, rotate_ligand=False,
                 exclude_clashes=True, clip=5.0, lib=None, differentiable=False, fused_filter_grad=False):
        """lib: None -> the product library (GPU); the test-suite passes the emulated one.
        differentiable (a public attribute, as on ``LocalDockingModel``): False -- ``forward`` is the inference path: the
        correlations carry no graph and the reference's MLP filter runs in the fused kernel.  True -- the model that is
        trained (the reference trains this model through VolumeConvolution's backward, DockingModels.py:48,71): under
        autograd, with an input volume or a filter parameter requiring a gradient, the correlations go through the
        differentiable ``VolumeConvolution`` (csrc/dlpd_corr_grad.h), the filter MODULE is called on the channels-last rows
        and the nearest upsampling is ``interpolate``; under ``torch.no_grad()`` it takes the fused path like the other.
        fused_filter_grad (a public attribute, opt-in as ``hip_autograd`` is on the plugins): True -- where ``forward`` builds a
        graph and the filter is the reference's MLP on one or two resolutions the backward kernel supports
        (``ops.filter_grad_supported``), the filter stage is ``ops.filter_volumes_autograd`` on the live ``fc[0]`` / ``fc[2]``
        parameters: the inference kernel forward, csrc/dlpd_filter_grad.h backward, no interpolate / cat / permute and no saved
        activations.  Any other filter or shape is called as a module, as with False."""
        super().__init__()
        self.differentiable = bool(differentiable)
        self.fused_filter_grad = bool(fused_filter_grad)
        self.representation, self.filter = representation, filter
        self.threshold_clash, self.clip = threshold_clash, clip
        self.normalize, self.rotate_ligand, self.exclude = normalize, rotate_ligand, exclude_clashes
        self.convolve = VolumeConvolution(clip=clip, lib=lib)
        self.vol_rotate = VolumeRotation(lib=lib)
        self._lib = lib

    def _paths(self, directory, epoch, model_name):
        return [os.path.join(directory, pattern % (model_name, epoch)) for pattern in self.FILES]

    def save(self, directory, epoch, model_name="DPD_Model"):
        for part, path in zip((self.representation, self.filter), self._paths(directory, epoch, model_name)):
            torch.save(part.state_dict(), path)

    def load(self, directory, epoch, model_name="DPD_Model"):
        for part, path in zip((self.representation, self.filter), self._paths(directory, epoch, model_name)):
            part.load_state_dict(torch.load(path))

    def forward(self, receptor_volumes, ligand_volumes):
        """Lists of (B, C_i, L_i, L_i, L_i) per resolution -> scores (B, 2L_0, 2L_0, 2L_0)."""
        receptor_volumes, ligand_volumes = list(receptor_volumes), list(ligand_volumes)
        graph = self.differentiable and torch.is_grad_enabled() and (
            any(v.requires_grad for v in receptor_volumes + ligand_volumes) or
            (isinstance(self.filter, nn.Module) and any(p.requires_grad for p in self.filter.parameters())))
        if graph:
            correlations = [self.convolve(rec, lig) for rec, lig in zip(receptor_volumes, ligand_volumes)]
        else:       # the inference path: no graph through the correlation, whatever the inputs require
            correlations = [self.convolve(rec.detach(), lig.detach()) for rec, lig in zip(receptor_volumes, ligand_volumes)]
        if graph and self.fused_filter_grad and 1 <= len(correlations) <= 2:
            live = live_mlp_parameters(self.filter)
            fine, coarse = correlations[0], (correlations[1] if len(correlations) == 2 else None)
            if live is not None and live[0].shape[1] == sum(c.shape[1] for c in correlations) and filter_grad_supported(
                    fine.shape[1], fine.shape[2], 0 if coarse is None else coarse.shape[1],
                    0 if coarse is None else coarse.shape[2], live[0].shape[0], self._lib):
                return filter_volumes_autograd(correlations, *live, lib=self._lib)
        params = None if graph else mlp_parameters(self.filter)
        if params is not None and params[0].shape[0] <= 64 and len(correlations) <= 2:
            W1, b1, W2, b2 = params
            return filter_volumes(correlations, W1, b1, W2, float(b2.reshape(-1)[0]), lib=self._lib)
        # any other filter module: the reference's data movement (DockingModels.py:74-83), then the module
        B, N = correlations[0].shape[0], correlations[0].shape[2]
        same = [c if c.shape[2] == N else nn.functional.interpolate(c, size=(N, N, N)) for c in correlations]
        V = torch.cat(same, dim=1).permute(0, 2, 3, 4, 1).reshape(B * N * N * N, -1)
        return self.filter(V).reshape(B, N, N, N)

    forward.dlpd_reference_forward = True      # what the fused kernels compute (fused_filter_parameters)


class LocalDockingModel(nn.Module):
    """Scores GIVEN poses -- one receptor / ligand pair, one translation, one number per batch entry: the reference's
    ``LocalDockingModel`` (DockingModels.py:86-120; driven by LocalTrainer.score, LocalTrainer.py:146-177) with the same
    surface: ``.representation``, ``.filter``, ``.mult``, ``save`` / ``load`` with the reference's file names,
    ``forward(receptor, ligand, T)`` -> (B, 1).

    ``differentiable=False`` (the default) is INFERENCE ONLY: ``forward`` raises when autograd is enabled and a parameter
    requires a gradient (call it under ``torch.no_grad()``), rather than return a tensor that silently has no graph.
    ``differentiable=True`` (a public attribute; ``Training.LocalTrainer`` sets it on the model it is given) is the model that
    is trained: under autograd the correlation goes through the differentiable ``MultiplyVolumes`` (the adjoint kernel of
    csrc/dlpd_local_grad.h), the representation runs as the plain torch modules it is made of (with its ``hip_autograd`` set: its stride-1
    convolutions on ``ops.conv3d_autograd``), and the filter is CALLED -- the
    fused filter kernel has no graph and serves ``torch.no_grad()`` only, as before.
    A filter that is not the reference's MLP (or is wider than the kernel's hidden widths) is called on the (B, sum C) features.
    ``forward_poses(receptor, ligand, R, T)`` scores P poses of ONE pair with one representation pass per protein (its docstring)."""
    FILES = GlobalDockingModel.FILES

    def __init__(self, representation, filter, lib=None, differentiable=False):
        super().__init__()
        self.representation, self.filter = representation, filter
        self.mult = MultiplyVolumes(lib=lib)
        self._lib = lib
        self.differentiable = bool(differentiable)

    _paths = GlobalDockingModel._paths
    save = GlobalDockingModel.save
    load = GlobalDockingModel.load

    def forward(self, receptor, ligand, T):
        graph = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if graph and not self.differentiable:
            raise RuntimeError("dlpd: LocalDockingModel is inference only (no backward through the correlation kernel): "
                               "call it under torch.no_grad(), or construct it with differentiable=True")
        edge = float(receptor.shape[2])
        # one correlation value per channel of every resolution: T lives on the input grid, each resolution reads it
        # scaled to its own edge (MultiplyVolumes truncates the scaled value toward zero)
        pairs = zip(self.representation(receptor), self.representation(ligand))
        # (T * edge_i / edge in this order, in T's own precision: where the product is a whole number the truncation must see it)
        features = torch.cat([self.mult(rv.contiguous(), lv.contiguous(), T * float(rv.shape[2]) / edge) for rv, lv in pairs],
                             dim=1).contiguous()
        return self._filter_features(features, graph)

    def forward_poses(self, receptor, ligand, R, T, vol_rotate_center=None):
        """ONE pair at P poses -- what a search's top list is: ``receptor`` / ``ligand`` (1, 11, L, L, L), ``R`` (P, 3, 3) the
        maps ``VolumeRotation`` samples with, ``T`` (P, 3) on the input grid (scaled and truncated per resolution as ``forward``
        does) -> (P, 1).  The representation runs ONCE per protein; per resolution the P rotated ligands are correlated with
        the receptor by ``ops.local_correlate_rotated`` (no rotated volume in memory, differentiable in both volumes), where
        the reference rotates the coordinates and pays one representation pass per pose.  ``vol_rotate_center``: the pivot on
        the input grid (None: index L / 2), scaled to every resolution.  ``differentiable`` governs it as it governs ``forward``."""
        graph = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if graph and not self.differentiable:
            raise RuntimeError("dlpd: LocalDockingModel is inference only (no backward through the correlation kernel): "
                               "call it under torch.no_grad(), or construct it with differentiable=True")
        if receptor.shape[0] != 1 or ligand.shape[0] != 1 or R.dim() != 3 or T.shape[0] != R.shape[0]:
            raise RuntimeError("dlpd: forward_poses expects one (1, C, L, L, L) pair, R (P, 3, 3) and T (P, 3)")
        edge, P = receptor.shape[2], R.shape[0]
        feats = []
        for rv, lv in zip(self.representation(receptor), self.representation(ligand)):
            Li = rv.shape[2]
            Ti = (torch.as_tensor(T) * float(Li) / float(edge)).detach().trunc().to(torch.int32).to(rv.device)
            Ri = R.detach().to(device=rv.device, dtype=torch.float32).contiguous()
            corr = local_correlate_rotated(rv[0].contiguous(), lv[0].contiguous(), Ti, Ri, radius=0, scale=1, coarse="trunc",
                                           center=rotation_pivot(vol_rotate_center, Li, edge), lib=self._lib)
            feats.append(corr.reshape(P, -1))
        return self._filter_features(torch.cat(feats, dim=1).contiguous(), graph)

    def _filter_features(self, features, graph):
        """(B, sum C) -> (B, 1): the fused filter kernel where there is no graph, the module otherwise."""
        params = None if graph else mlp_parameters(self.filter)
        if params is not None:
            W1, b1, W2, b2 = params
            B = features.shape[0]
            zero_t = torch.zeros(B, 3, dtype=torch.int32, device=features.device)
            out = local_filter(features.reshape(B, -1, 1, 1, 1), None, None, zero_t, 0, W1, b1, W2, b2, lib=self._lib)
            if out is not None:
                return out[0].reshape(B, 1)
        return self.filter(features)
