"""Check bodies of the scoring entry points of include/dlpd.h that neither DockingEngine nor ops calls, shared by
tests/test_abi_scoring_emu.py (the kernel sources on the fibre emulator) and tests/test_abi_scoring_gpu.py (the gfx950 build):

  1. dlpd_zifft_filter_aux / _cand / _form with RAW coarse channels (aux_is_preact = 0): the raw-aux branch of the
     channel-owning K3 (k_zifft_filter<N, HP, 1>, csrc/dlpd_corr.hip) -- its own gather, channel chunks and W1t row offset;
  2. dlpd_filter_preact (k_filter_preact) and its two consumers, dlpd_filter_volumes(conv1_is_preact = 1) and
     dlpd_zifft_filter_aux(aux_is_preact = 1);
  3. dlpd_score_rotations / dlpd_score_rotations_oriented, the one-call K1 + K2 + K3 driver, and through it the plain
     dlpd_zifft_filter.

Every entry point is called through ``lib.call`` with the argument lists of deeplocalproteindocking_amd/_lib.py, as a ctypes
integrator would; wsB of the K3 cases comes from the public stages dlpd_rfft3d_padded (scale 1 / N^3),
dlpd_zfft and dlpd_xy_correlate, as in tests/c_abi/client.c.

Truth and tolerance.  ``accuracy_checks.yardstick``, unchanged: the kernel output X against X64, the restatement by the
oracle's own pieces (orc.correlate_fft, orc.filter_mlp, acc.oracle_features) in float64, with X32, the same restatement in
float32, as the measure; margins 2 (RMS) and 3 (max), the project's standing rule and no number of this file's own.  Where a
clash mask is on, thr is the median of the float64 clash correlation, voxels within NEAR_BAND * thr of it are left out (at most
NEAR_CAP of a case, asserted) and the masked fraction lies between 0.2 and 0.7 (asserted) -- all of it on the float64
restatement alone, before a kernel runs.  The exact cases carry no tolerance: their inputs are dyadic or index-only and the
kernel must give the float64 bits.  Nothing here reads the reference tree.
"""
import functools

import numpy as np
import torch

import accuracy_checks as acc
from oracle import docking_oracle as orc

ERR_ARG, ERR_UNSUPPORTED = 1, 2
AMP = 0.05                                   # amplitude of the random score volumes, as acc.Case
AUX_CHANNELS = (1, 5, 9)                     # a lone channel, a partial second chunk of 4, a partial second chunk of 8
HIDDEN = {1: 3, 5: 8, 9: 6}                  # Caux -> H: dlpd_hidden_pad(3) = 4 != 3, dlpd_hidden_pad(8) = 8, dlpd_hidden_pad(6) = 8
GUARD = 1024                                 # floats of sentinel behind every buffer the driver writes


def _get(lib):
    from deeplocalproteindocking_amd._lib import get_lib
    return lib or get_lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(device):
    device = torch.device(device)
    return torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else None


def _dev(t, device):
    return torch.as_tensor(t).to(torch.float32).contiguous().to(device)


def hidden_table(lib):
    """The compiled hidden widths, probed: the values dlpd_hidden_pad takes."""
    table = sorted({lib.call("dlpd_hidden_pad", H) for H in range(1, 65)} - {-1})
    assert table and all(lib.call("dlpd_hidden_pad", w) == w for w in table), table
    return table


def padded_filter(lib, filt, device):
    """(W1 (H, C), b1, W2 (1, H), b2) -> W1t (C, HP), b1 (HP), W2 (HP) zero padded on ``device``, b2, HP = dlpd_hidden_pad(H)."""
    W1, b1, W2, b2 = (torch.as_tensor(t).float() for t in filt)
    H, C = W1.shape
    HP = lib.call("dlpd_hidden_pad", int(H))
    assert HP >= H
    W1t, b1p, W2p = torch.zeros(C, HP), torch.zeros(HP), torch.zeros(HP)
    W1t[:, :H], b1p[:H], W2p[:H] = W1.t(), b1, W2.reshape(-1)
    return W1t.to(device), b1p.to(device), W2p.to(device), float(b2.reshape(-1)[0]), HP


def k2_output(lib, device, rec, ligs):
    """wsB (nb, CT, NZ, N, N) complex64 of the given volumes (no rotation) by the public stages: rec (CT, L^3), ligs (nb, CT, L^3)."""
    nb, CT, L = ligs.shape[0], ligs.shape[1], ligs.shape[-1]
    N, NZ, st = 2 * L, L + 1, _stream(device)
    recd, ligd = _dev(rec, device), _dev(ligs, device)
    wsA = torch.empty(nb * CT * NZ * L * L * 2, dtype=torch.float32, device=device)
    spec = torch.empty(CT * NZ * N * N * 2, dtype=torch.float32, device=device)
    wsB = torch.empty(nb * CT * NZ * N * N * 2, dtype=torch.float32, device=device)
    lib.call("dlpd_rfft3d_padded", _ptr(recd), _ptr(spec), _ptr(wsA), CT, L, 1.0 / N ** 3, st)
    lib.call("dlpd_zfft", _ptr(ligd), None, _ptr(wsA), nb, CT, L, CT * L ** 3, 0, 0.0, st)
    lib.call("dlpd_xy_correlate", _ptr(wsA), _ptr(spec), _ptr(wsB), nb, CT, L, 0, st)
    return wsB


def k3(lib, device, wsB, nb, C, has_clash, L, pf, clip, thr, aux=None, Caux=0, preact=0, spelling="aux"):
    """One fused K3 call in the named spelling -> V (nb, N^3) on the host."""
    W1t, b1, W2, b2, HP = pf
    N = 2 * L
    V = torch.full((nb, N * N * N), float("nan"), dtype=torch.float32, device=device)
    head = (_ptr(wsB), _ptr(V), nb, C, int(has_clash), L, _ptr(W1t), _ptr(b1), _ptr(W2), b2, HP, int(clip is not None),
            float(clip or 0.0), float(thr))
    tail = (_ptr(aux), int(Caux), int(preact))
    st = _stream(device)
    if spelling == "plain":
        assert Caux == 0
        lib.call("dlpd_zifft_filter", *head, st)
    elif spelling == "aux":
        lib.call("dlpd_zifft_filter_aux", *head, *tail, st)
    elif spelling == "cand":
        lib.call("dlpd_zifft_filter_cand", *head, *tail, None, None, None, 0, st)
    else:
        form = {"form0": 0, "form1": 1}[spelling]
        lib.call("dlpd_zifft_filter_form", *head, *tail, None, None, None, 0, form, st)
    return V.cpu()


def upsample(a, s=2):
    """Nearest upsample by index of the last three dimensions (DockingModels.py:74-76: fine index // s)."""
    return a.repeat_interleave(s, -3).repeat_interleave(s, -2).repeat_interleave(s, -1)


# ----------------------------------------------------------------------------------------------------------------------
# 1. K3 with raw coarse channels
# ----------------------------------------------------------------------------------------------------------------------

def planted_positions(Na, item):
    """Coarse voxels of one batch item: the eight corners, one face centre (another face per item), and (1, 2, 3)."""
    e, m = (0, Na - 1), Na // 2
    face = [(0, m, m), (m, Na - 1, m), (m, m, 0)][item % 3]
    return [(x, y, z) for x in e for y in e for z in e] + [face, (1, 2, 3)]


def check_raw_aux_index_exact(lib, device, L, Caux, nb=2, seed=0):
    """Zero ligand (every correlation is 0), aux zero but for single ones, a probe filter over the aux channels:
    V = sum_c w_c upsample(aux_c), +-1 on the eight fine children of each planted voxel and 0 elsewhere, exactly."""
    lib = _get(lib)
    N, Na, C = 2 * L, L, 1
    g = torch.Generator().manual_seed(seed)
    rec = torch.randn(C, L, L, L, generator=g) * AMP
    ligs = torch.zeros(nb, C, L, L, L)
    chans = [0, Caux - 1, Caux // 2]                                   # first, last, middle
    aux = torch.zeros(nb, Caux, Na, Na, Na)
    for b in range(nb):
        for k, p in enumerate(planted_positions(Na, b)):
            aux[(b, chans[(b + k) % 3]) + p] = 1.0
    assert nb < 2 or not torch.equal(aux[0], aux[1])                   # (a dropped batch stride shows)
    # the probe reads the aux channels only: rows [C, C + Caux) of W1t; the fine channel's column stays zero
    W1p, b1p, W2p, b2p = acc.probe_filters(Caux, width=Caux, signs=1, seed=seed)[0]
    W1 = torch.cat([torch.zeros(2 * Caux, C), W1p], dim=1)
    w = W2p[0, :Caux].double()
    assert bool((w.abs() == 1).all())
    want = (upsample(aux.double()) * w[None, :, None, None, None]).sum(1).reshape(nb, -1)
    assert int((want != 0).sum()) == nb * 10 * 8 and bool((want.abs()[want != 0] == 1).all())
    pf = padded_filter(lib, (W1, b1p, W2p, b2p), device)
    assert pf[4] == lib.call("dlpd_hidden_pad", 2 * Caux)
    wsB = k2_output(lib, device, rec, ligs)
    V = k3(lib, device, wsB, nb, C, 0, L, pf, None, 0.0, _dev(aux, device), Caux, 0)
    bad = torch.nonzero(V.double() != want)
    assert bad.shape[0] == 0, ("box %d, Caux %d" % (L, Caux), bad.shape[0],
                               [(int(b), np.unravel_index(int(i), (N, N, N)), float(V[b, i]), float(want[b, i])) for b, i in bad[:8]])


class FusedCase:
    """Inputs and both restatements of one two-resolution K3 case on given volumes: C fine channels (+ a clash channel) at box
    L, Caux coarse channels that arrive as clipped real volumes on the grid L^3, one random SimpleFilter.  Building it runs the
    float64 restatement and asserts the caps of the module docstring; no kernel is involved."""

    def __init__(self, L, Caux, has_clash, C=3, nb=2, seed=0):
        self.L, self.C, self.Caux, self.has_clash, self.nb = L, C, Caux, bool(has_clash), nb
        N = 2 * L
        g = torch.Generator().manual_seed(1000 * L + 10 * Caux + int(has_clash) + seed)
        self.rec, self.lig = torch.randn(C, L, L, L, generator=g) * AMP, torch.randn(nb, C, L, L, L, generator=g) * AMP
        self.recf, self.ligf = torch.rand(L, L, L, generator=g), torch.rand(nb, L, L, L, generator=g)
        self.filt = acc.random_filter(C + Caux, HIDDEN[Caux], seed + Caux, dead=1)
        f64, f32 = torch.float64, torch.float32
        corr = torch.cat([orc.correlate_fft(self.rec[None], self.lig[b:b + 1], dtype=f64) for b in range(nb)])
        # a clip that saturates a few percent of the fine correlations; aux arrives already clipped: drawn inside +-clip
        a = corr.abs().reshape(-1)
        self.clip = float(a.kthvalue(int(0.97 * a.numel())).values)
        sat = float((a >= self.clip).double().mean())
        assert 0.01 <= sat <= 0.10, ("saturated fraction", sat)
        self.aux = ((torch.rand(nb, Caux, L, L, L, generator=g) * 2 - 1) * self.clip).float()
        assert float(self.aux.abs().max()) <= self.clip
        self.thr, self.keep, mask64, self.left_out = 0.0, None, None, 0.0
        if self.has_clash:
            norm = torch.cat([orc.correlate_fft(self.recf[None, None], self.ligf[b:b + 1, None], dtype=f64)[:, 0] for b in range(nb)])
            norm = norm.reshape(nb, -1)
            self.thr = float(norm.median())
            assert self.thr > 0
            self.keep = (norm - self.thr).abs() > acc.NEAR_BAND * self.thr
            self.left_out = float((~self.keep).double().mean())
            assert self.left_out <= acc.NEAR_CAP, ("voxels near the clash threshold", self.left_out)
            mask64 = (norm < self.thr).double()
            masked = float((mask64 == 0).double().mean())
            assert 0.2 <= masked <= 0.7, ("masked fraction", masked)
        self.X64 = self._restate(f64, mask64)
        self.X32 = self._restate(f32, None)
        print("ACCURACY | [%d @ %d, %d raw @ %d]%s: clip %.4g saturates %.2f %% of the fine correlations, %.4f %% of the voxels left out "
              "near the threshold" % (C, L, Caux, L // 2, ", clash" if has_clash else "", self.clip, 100 * sat, 100 * self.left_out), flush=True)
        assert N ** 3 * nb == self.X64.numel()

    def _restate(self, dtype, mask):
        """features [clamp(corr), nearest-upsample(aux)] -> filter_mlp -> times (clash < thr), all in ``dtype``."""
        N, out = 2 * self.L, []
        for b in range(self.nb):
            feat = acc.oracle_features([self.rec], [self.lig[b].to(dtype)], self.clip, dtype)                 # (N^3, C)
            up = upsample(self.aux[b].to(dtype)).permute(1, 2, 3, 0).reshape(N * N * N, self.Caux)
            v = acc.oracle_scores(torch.cat([feat, up], dim=1), self.filt, dtype)
            if self.has_clash:
                m = mask[b] if mask is not None else \
                    (orc.correlate_fft(self.recf[None, None], self.ligf[b:b + 1, None], dtype=dtype)[0, 0].reshape(-1) < self.thr).to(dtype)
                v = v * m
            out.append(v)
        return torch.stack(out)

    def label(self, what):
        return "[%d @ %d, %d @ %d] %s%s" % (self.C, self.L, self.Caux, self.L // 2, what, ", clash" if self.has_clash else "")

    def k2(self, lib, device):
        rec = torch.cat([self.rec, self.recf[None]]) if self.has_clash else self.rec
        lig = torch.cat([self.lig, self.ligf[:, None]], dim=1) if self.has_clash else self.lig
        return k2_output(lib, device, rec, lig)

    def raw(self, lib, device, wsB=None, spelling="aux"):
        pf = padded_filter(lib, self.filt, device)
        assert (pf[4] != HIDDEN[self.Caux]) == (self.Caux != 5)          # one case with padding, one without
        wsB = self.k2(lib, device) if wsB is None else wsB
        return k3(lib, device, wsB, self.nb, self.C, self.has_clash, self.L, pf, self.clip, self.thr, _dev(self.aux, device), self.Caux, 0,
                  spelling)

    def preact(self, lib, device):
        """The same features with the coarse half of the first layer made by dlpd_filter_preact: planes (nb, HP, L^3)."""
        pf = padded_filter(lib, self.filt, device)
        W1t, b1, HP = pf[0], pf[1], pf[4]
        planes = filter_preact(lib, device, _dev(self.aux, device), W1t[self.C:].contiguous(), b1, HP)
        return k3(lib, device, self.k2(lib, device), self.nb, self.C, self.has_clash, self.L, pf, self.clip, self.thr, planes, self.Caux, 1)


@functools.lru_cache(maxsize=4)
def fused_case(L, Caux, has_clash):
    """One restatement per case, shared by the tests that run it (raw form, the three spellings, the pre-activation form)."""
    return FusedCase(L, Caux, has_clash)


def check_raw_aux_yardstick(lib, device, L, Caux, has_clash):
    lib = _get(lib)
    case = fused_case(L, Caux, int(has_clash))
    V = case.raw(lib, device)
    return acc.yardstick(case.label("raw coarse channels"), V, case.X32, case.X64, case.keep)


def check_raw_aux_spellings(lib, device, L=32, Caux=5, has_clash=1):
    """dlpd_zifft_filter_aux, dlpd_zifft_filter_cand without lists, dlpd_zifft_filter_form(form 0) and (form 1): equal bits."""
    lib = _get(lib)
    case = fused_case(L, Caux, int(has_clash))
    wsB = case.k2(lib, device)
    got = {s: case.raw(lib, device, wsB, s) for s in ("aux", "cand", "form0", "form1")}
    assert bool(torch.isfinite(got["aux"]).all()) and float(got["aux"].abs().max()) > 0
    for s in ("cand", "form0", "form1"):
        assert got[s].numpy().tobytes() == got["aux"].numpy().tobytes(), s


def check_raw_aux_refusals(lib, product, device):
    """Caux > 0 without aux: DLPD_ERR_ARG (any library).  Raw aux at boxes 64 and 80 on the PRODUCT library:
    DLPD_ERR_UNSUPPORTED, as include/dlpd.h states.  Neither launches: the buffers are a few floats."""
    lib, product = _get(lib), _get(product)
    buf = torch.zeros(1 << 10, dtype=torch.float32, device=device)       # (never reached: every call returns before a launch)
    p, st = buf.data_ptr(), _stream(device)
    for lb in (lib, product):
        for L in (32, 40, 64, 80):
            assert lb._dlpd_zifft_filter_aux(p, p, 1, 3, 0, L, p, p, p, 0.0, 4, 0, 0.0, 0.0, None, 5, 0, st) == ERR_ARG
        assert lb._dlpd_zifft_filter_cand(p, p, 1, 3, 0, 32, p, p, p, 0.0, 4, 0, 0.0, 0.0, None, 5, 0, None, None, None, 0, st) == ERR_ARG
        assert lb._dlpd_zifft_filter_form(p, p, 1, 3, 0, 32, p, p, p, 0.0, 4, 0, 0.0, 0.0, None, 5, 0, None, None, None, 0, 1, st) == ERR_ARG
    for L in (64, 80):
        assert product._dlpd_zifft_filter_aux(p, p, 1, 3, 0, L, p, p, p, 0.0, 4, 0, 0.0, 0.0, p, 5, 0, st) == ERR_UNSUPPORTED
        for form in (0, 1, 2):
            assert product._dlpd_zifft_filter_form(p, p, 1, 3, 0, L, p, p, p, 0.0, 4, 0, 0.0, 0.0, p, 5, 0, None, None, None, 0, form,
                                                   st) == ERR_UNSUPPORTED
    if device != "cpu":
        torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# 2. dlpd_filter_preact and its consumers
# ----------------------------------------------------------------------------------------------------------------------

PREACT_SHAPES = [(2, 5, 8, 8),               # (nb, C1, N1, HP)
                 (1, 1, 4, 2),               # the smallest: one partial block
                 (3, 9, 12, 24)]             # nb * n / 4 = 1296: not a multiple of 256


def filter_preact(lib, device, conv1, W1rows, b1, HP):
    """conv1 (nb, C1, N1^3), W1rows (C1, HP), b1 (HP) on ``device`` -> pre (nb, HP, N1^3) on ``device``."""
    nb, C1, N1 = conv1.shape[0], conv1.shape[1], conv1.shape[-1]
    assert W1rows.shape == (C1, HP) and b1.shape == (HP,) and W1rows.is_contiguous() and conv1.is_contiguous()
    pre = torch.full((nb, HP, N1, N1, N1), float("nan"), dtype=torch.float32, device=device)
    lib.call("dlpd_filter_preact", _ptr(conv1), C1, N1, _ptr(W1rows), _ptr(b1), HP, _ptr(pre), nb, _stream(device))
    return pre


def preact_restatement(conv1, W1rows, b1, dtype):
    """b1 + W1rows^T conv1 in ``dtype``."""
    return torch.einsum("ch,bcxyz->bhxyz", W1rows.to(dtype), conv1.to(dtype)) + b1.to(dtype)[None, :, None, None, None]


def _dyadic(gen, lo, hi, div, *size):
    return torch.randint(lo, hi, size, generator=gen).float() / div


def check_preact_exact(lib, device, shape, seed=0):
    """Dyadic inputs (value sets as filter_grad_checks.exact_inputs): every product and partial sum is exact in float32, so
    pre equals the float64 b1 + W1rows^T conv1 bit for bit."""
    lib = _get(lib)
    nb, C1, N1, HP = shape
    assert HP in hidden_table(lib)
    gen = torch.Generator().manual_seed(seed + HP)
    conv1 = _dyadic(gen, -4, 5, 4, nb, C1, N1, N1, N1)                  # {-1, -0.75, .., 1}
    W1rows = _dyadic(gen, -2, 3, 2, C1, HP)                            # {-1, -0.5, 0, 0.5, 1}
    b1 = (2 * torch.randint(-4, 4, (HP,), generator=gen).float() + 1) / 16   # odd multiples of 1/16
    assert nb < 2 or not torch.equal(conv1[0], conv1[1])
    want = preact_restatement(conv1, W1rows, b1, torch.float64)
    assert torch.equal(preact_restatement(conv1, W1rows, b1, torch.float32).double(), want)
    pre = filter_preact(lib, device, _dev(conv1, device), _dev(W1rows, device), _dev(b1, device), HP).cpu()
    assert torch.equal(pre.double(), want), (shape, float((pre.double() - want).abs().max()))


def check_preact_random(lib, device, shape, seed=1):
    lib = _get(lib)
    nb, C1, N1, HP = shape
    gen = torch.Generator().manual_seed(seed + HP)
    conv1, W1rows, b1 = torch.randn(nb, C1, N1, N1, N1, generator=gen), torch.randn(C1, HP, generator=gen), torch.randn(HP, generator=gen)
    pre = filter_preact(lib, device, _dev(conv1, device), _dev(W1rows, device), _dev(b1, device), HP).cpu()
    return acc.yardstick("dlpd_filter_preact (nb, C1, N1, HP) = %s" % (shape,), pre, preact_restatement(conv1, W1rows, b1, torch.float32),
                         preact_restatement(conv1, W1rows, b1, torch.float64))


def check_preact_refusals(lib, device):
    lib = _get(lib)
    buf = torch.zeros(1 << 10, dtype=torch.float32, device=device)       # (never reached: every call returns before a launch)
    p, st, fp = buf.data_ptr(), _stream(device), lib._dlpd_filter_preact
    for N1 in (5, 6, 7):
        assert fp(p, 2, N1, p, p, 4, p, 1, st) == ERR_ARG
    for k in range(4):
        ptrs = [p, p, p, p]
        ptrs[k] = None
        assert fp(ptrs[0], 2, 4, ptrs[1], ptrs[2], 4, ptrs[3], 1, st) == ERR_ARG
    table = hidden_table(lib)
    for HP in (1, 3, 12, 48, 64):
        assert HP not in table
        assert fp(p, 2, 4, p, p, HP, p, 1, st) == ERR_UNSUPPORTED
    if device != "cpu":
        torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


def _filter_volumes(lib, device, conv0m, C0, conv1, C1, is_preact, thr, pf):
    """dlpd_filter_volumes with the mask as channel C0 of conv0m (nb, C0 + 1, N0^3): the layout include/dlpd.h advertises."""
    W1t, b1, W2, b2, HP = pf
    nb, N0, N1 = conv0m.shape[0], conv0m.shape[-1], conv1.shape[-1]
    bs = (C0 + 1) * N0 ** 3
    V = torch.full((nb, N0, N0, N0), float("nan"), dtype=torch.float32, device=device)
    lib.call("dlpd_filter_volumes", _ptr(conv0m), C0, bs, N0, _ptr(conv1), C1, N1, int(is_preact), conv0m.data_ptr() + 4 * C0 * N0 ** 3, bs,
             float(thr), 1, _ptr(W1t), _ptr(b1), _ptr(W2), b2, HP, _ptr(V), nb, _stream(device))
    return V.cpu()


def _volumes_restatement(conv0, conv1, mask, thr, filt, dtype, s):
    nb, N0 = conv0.shape[0], conv0.shape[-1]
    feat = torch.cat([conv0.to(dtype), upsample(conv1.to(dtype), s) if s > 1 else conv1.to(dtype)], dim=1)
    v = acc.oracle_scores(feat.permute(0, 2, 3, 4, 1).reshape(nb * N0 ** 3, -1), filt, dtype).reshape(nb, N0, N0, N0)
    return v * (mask.to(dtype) < thr).to(dtype)


def check_filter_volumes_preact(lib, device, N0, N1, nb=2, C0=3, C1=5, seed=0):
    """dlpd_filter_volumes(conv1_is_preact = 1) on the planes of dlpd_filter_preact: bit for bit the raw-conv1 call on dyadic
    inputs (and the float64 restatement), through the yardstick on random ones; the clash mask is a channel of conv0."""
    lib = _get(lib)
    s = N0 // N1
    gen = torch.Generator().manual_seed(seed + N0)
    # dyadic
    H = 4
    conv0, conv1 = _dyadic(gen, -4, 5, 4, nb, C0, N0, N0, N0), _dyadic(gen, -4, 5, 4, nb, C1, N1, N1, N1)
    mask = _dyadic(gen, 0, 9, 8, nb, 1, N0, N0, N0)                     # {0, 1/8, .., 1} against thr = 0.5: nothing near it but ties
    filt = (_dyadic(gen, -2, 3, 2, H, C0 + C1), (2 * torch.randint(-4, 4, (H,), generator=gen).float() + 1) / 16,
            _dyadic(gen, -2, 3, 2, 1, H), torch.tensor([0.25]))
    thr = 0.5
    want = _volumes_restatement(conv0, conv1, mask[:, 0], thr, filt, torch.float64, s)
    masked = float((mask[:, 0] >= thr).double().mean())
    assert 0.2 <= masked <= 0.7 and float(want.abs().max()) > 0
    pf = padded_filter(lib, filt, device)
    conv0m, conv1d = _dev(torch.cat([conv0, mask], dim=1), device), _dev(conv1, device)
    planes = filter_preact(lib, device, conv1d, pf[0][C0:].contiguous(), pf[1], pf[4])
    via_planes = _filter_volumes(lib, device, conv0m, C0, planes, C1, 1, thr, pf)
    via_raw = _filter_volumes(lib, device, conv0m, C0, conv1d, C1, 0, thr, pf)
    assert via_planes.numpy().tobytes() == via_raw.numpy().tobytes(), float((via_planes - via_raw).abs().max())
    assert torch.equal(via_planes.double(), want)
    # random
    H = 6
    conv0, conv1 = torch.randn(nb, C0, N0, N0, N0, generator=gen) * 0.5, torch.randn(nb, C1, N1, N1, N1, generator=gen) * 0.5
    mask = torch.rand(nb, 1, N0, N0, N0, generator=gen)
    filt = acc.random_filter(C0 + C1, H, seed + 1, dead=1)
    thr = float(mask.double().median())
    keep = (mask[:, 0].double() - thr).abs() > acc.NEAR_BAND * thr
    left_out = float((~keep).double().mean())
    assert left_out <= acc.NEAR_CAP, ("voxels near the threshold", left_out)
    masked = float((mask.double() >= thr).double().mean())
    assert 0.2 <= masked <= 0.7
    X64 = _volumes_restatement(conv0, conv1, mask[:, 0], thr, filt, torch.float64, s)
    X32 = _volumes_restatement(conv0, conv1, mask[:, 0], thr, filt, torch.float32, s)
    pf = padded_filter(lib, filt, device)
    assert pf[4] != H
    conv0m, conv1d = _dev(torch.cat([conv0, mask], dim=1), device), _dev(conv1, device)
    planes = filter_preact(lib, device, conv1d, pf[0][C0:].contiguous(), pf[1], pf[4])
    V = _filter_volumes(lib, device, conv0m, C0, planes, C1, 1, thr, pf)
    print("ACCURACY | dlpd_filter_volumes(conv1_is_preact = 1) (%d, %d): %.4f %% of the voxels left out near the threshold" %
          (N0, N1, 100 * left_out), flush=True)
    return acc.yardstick("dlpd_filter_volumes(conv1_is_preact = 1), [%d @ %d, %d @ %d]" % (C0, N0, C1, N1), V, X32, X64, keep)


def check_filter_volumes_preact_refusal(lib, device):
    """Pre-activation planes with N0 / N1 = 4: DLPD_ERR_ARG (the kernel reads them by halves or as they are)."""
    lib = _get(lib)
    buf = torch.zeros(1 << 10, dtype=torch.float32, device=device)       # (never reached)
    p, st, fv = buf.data_ptr(), _stream(device), lib._dlpd_filter_volumes
    assert fv(p, 3, 4 * 16 ** 3, 16, p, 5, 4, 1, p, 4 * 16 ** 3, 0.5, 1, p, p, p, 0.0, 4, p, 1, st) == ERR_ARG
    assert fv(p, 3, 4 * 16 ** 3, 16, p, 0, 16, 1, p, 4 * 16 ** 3, 0.5, 1, p, p, p, 0.0, 4, p, 1, st) == ERR_ARG     # planes of no channels
    if device != "cpu":
        torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


def check_k3_preact_from_filter_preact(lib, device, L, Caux, has_clash):
    """dlpd_zifft_filter_aux(aux_is_preact = 1) on the planes of dlpd_filter_preact against the X64 of the raw form.  (The two
    forms are not compared with each other: they sum in different orders, each answers to float64.)"""
    lib = _get(lib)
    case = fused_case(L, Caux, int(has_clash))
    V = case.preact(lib, device)
    return acc.yardstick(case.label("planes of dlpd_filter_preact"), V, case.X32, case.X64, case.keep)


# ----------------------------------------------------------------------------------------------------------------------
# 3. dlpd_score_rotations / dlpd_score_rotations_oriented
# ----------------------------------------------------------------------------------------------------------------------

class Driver:
    """One receptor / ligand pair (acc.Case's volumes) behind the one-call driver: lig (CT, L^3), the score channels and then the
    ligand's forbidden volume; recF from dlpd_rfft3d_padded(scale 1 / N^3)."""

    def __init__(self, lib, device, L, C, has_clash, R, filt, seed=0):
        self.lib, self.device, self.L, self.C, self.has_clash = _get(lib), device, L, C, bool(has_clash)
        self.case = acc.Case(self.lib, device, L, C, seed=seed, has_clash=self.has_clash)
        self.R64, self.filt = R, filt
        self.nb, self.CT = R.shape[0], C + int(self.has_clash)
        N, NZ, CT, c = 2 * L, L + 1, self.CT, self.case
        self.lig = _dev(torch.cat([c.lig, c.ligf[None]]) if self.has_clash else c.lig, device)
        rec = _dev(torch.cat([c.rec, c.recf[None]]) if self.has_clash else c.rec, device)
        self.R = _dev(torch.from_numpy(np.ascontiguousarray(R)).reshape(self.nb, 9), device)
        self.recF = torch.empty(CT * NZ * N * N * 2, dtype=torch.float32, device=device)
        scratch = torch.empty(CT * NZ * L * L * 2, dtype=torch.float32, device=device)
        self.lib.call("dlpd_rfft3d_padded", _ptr(rec), _ptr(self.recF), _ptr(scratch), CT, L, 1.0 / N ** 3, _stream(device))
        self.pf = padded_filter(self.lib, filt, device)
        self.nA, self.nB, self.nV = self.nb * CT * NZ * L * L * 2, self.nb * CT * NZ * N * N * 2, self.nb * N ** 3

    def buffers(self, fill):
        """wsA, wsB of exactly the documented sizes, pre-filled with ``fill``, and V, each with a guard of sentinels behind it."""
        out = []
        for n, f in ((self.nA, fill), (self.nB, fill), (self.nV, float("nan"))):
            t = torch.full((n + GUARD,), f, dtype=torch.float32, device=self.device)
            t[n:] = -7.0
            out.append(t)
        return out

    def _tail(self, thr, clip):
        W1t, b1, W2, b2, HP = self.pf
        return (_ptr(W1t), _ptr(b1), _ptr(W2), b2, HP, int(clip is not None), float(clip or 0.0), float(thr))

    def _guards(self, bufs):
        for t, n in zip(bufs, (self.nA, self.nB, self.nV)):
            assert bool((t[n:] == -7.0).all()), "written behind the end of a buffer of the documented size"

    def run(self, thr, clip=None, transposed=None, fill=float("nan")):
        """transposed None: dlpd_score_rotations; 0 / 1: dlpd_score_rotations_oriented -> V (nb, N^3) on the host."""
        wsA, wsB, V = bufs = self.buffers(fill)
        head = (_ptr(self.lig), _ptr(self.recF), _ptr(self.R), self.nb, self.C, int(self.has_clash), self.L, self.L / 2.0)
        st = _stream(self.device)
        if transposed is None:
            self.lib.call("dlpd_score_rotations", *head, *self._tail(thr, clip), _ptr(wsA), _ptr(wsB), _ptr(V), st)
        else:
            self.lib.call("dlpd_score_rotations_oriented", *head, *self._tail(thr, clip), _ptr(wsA), _ptr(wsB), _ptr(V), int(transposed), st)
        self._guards(bufs)
        return V[:self.nV].reshape(self.nb, -1).cpu()

    def staged(self, thr, clip=None, transposed=0):
        """The three calls the driver is documented to be, with the same ``transposed``."""
        wsA, wsB, V = bufs = self.buffers(0.0)
        lib, st, nb, CT, L = self.lib, _stream(self.device), self.nb, self.CT, self.L
        lib.call("dlpd_zfft_oriented", _ptr(self.lig), _ptr(self.R), _ptr(wsA), nb, CT, CT, 0, L, 0, 1, L / 2.0, int(transposed), st)
        lib.call("dlpd_xy_correlate_oriented", _ptr(wsA), _ptr(self.recF), _ptr(wsB), nb, CT, L, 0, int(transposed), st)
        lib.call("dlpd_zifft_filter", _ptr(wsB), _ptr(V), nb, self.C, int(self.has_clash), L, *self._tail(thr, clip), st)
        self._guards(bufs)
        return V[:self.nV].reshape(self.nb, -1).cpu()


def _same_bits(a, b, what):
    assert a.numpy().tobytes() == b.numpy().tobytes(), (what, float((a.double() - b.double()).abs().max()))


def check_driver_box32(lib, device, seed=3):
    """C = 3 plus a clash channel, two oblique rotations, a probe filter at box 32 (the per-channel K1): the driver equals its
    three stages bit for bit for transposed = 0 and 1, dlpd_score_rotations equals the oriented driver with transposed = 0,
    NaN-filled workspaces change nothing, and V answers to float64."""
    lib = _get(lib)
    L, C = 32, 3
    R = acc.rots(2, seed=seed + 5)
    filt = acc.probe_filters(C, acc.probe_width(lib, L), signs=1, seed=seed)[0]
    drv = Driver(lib, device, L, C, True, R, filt, seed=seed)
    thr, keep, V64, V32 = drv.case.oracle([filt], None, R=R)            # (asserts the clash caps on float64 before any kernel)
    plain = drv.run(thr)
    assert bool(torch.isfinite(plain).all())
    for transposed in (0, 1):
        assert lib.call("dlpd_orientation_supported", L) == 1
        V = drv.run(thr, transposed=transposed)
        _same_bits(V, drv.staged(thr, transposed=transposed), "driver vs its stages, transposed = %d" % transposed)
        _same_bits(V, drv.run(thr, transposed=transposed, fill=0.0), "NaN-filled vs zero-filled workspaces, transposed = %d" % transposed)
        acc.yardstick("dlpd_score_rotations_oriented(transposed = %d), %d @ %d + clash, probe" % (transposed, C, L), V, V32[0], V64[0], keep)
        if transposed == 0:
            _same_bits(plain, V, "dlpd_score_rotations vs dlpd_score_rotations_oriented(transposed = 0)")
    print("ACCURACY | dlpd_score_rotations %d @ %d + clash: %.4f %% of the voxels left out near the threshold" %
          (C, L, 100 * float((~keep).double().mean())), flush=True)


def check_driver_yardstick(lib, device, L, C, has_clash, nrot, seed=4):
    """One yardstick case of dlpd_score_rotations: a random SimpleFilter with the clip on, NaN-filled workspaces."""
    lib = _get(lib)
    R = acc.rots(nrot, seed=seed + L)
    filt = acc.random_filter(C, max(2, C), seed + L, dead=1)
    drv = Driver(lib, device, L, C, has_clash, R, filt, seed=seed + L)
    thr, keep, V64, V32 = drv.case.oracle([filt], 5.0, R=R)
    V = drv.run(thr, clip=5.0)
    if has_clash:
        print("ACCURACY | dlpd_score_rotations %d @ %d + clash: %.4f %% of the voxels left out near the threshold" %
              (C, L, 100 * float((~keep).double().mean())), flush=True)
    return acc.yardstick("dlpd_score_rotations, %d @ %d%s, random SimpleFilter, clip 5" % (C, L, " + clash" if has_clash else ""), V, V32[0],
                         V64[0], keep)


def check_driver_errors(lib, device):
    """A null ligand is DLPD_ERR_ARG from the first stage, box 33 DLPD_ERR_UNSUPPORTED; V stays untouched in both."""
    lib = _get(lib)
    buf = torch.zeros(1 << 10, dtype=torch.float32, device=device)       # (never reached: every call returns before a launch)
    V = torch.full((1 << 10,), -7.0, dtype=torch.float32, device=device)
    p, v, st = buf.data_ptr(), V.data_ptr(), _stream(device)
    tail = (p, p, p, 0.0, 2, 0, 0.0, 0.0, p, p, v)
    assert lib._dlpd_score_rotations(None, p, p, 1, 1, 0, 32, 16.0, *tail, st) == ERR_ARG
    assert lib._dlpd_score_rotations(p, p, p, 1, 1, 0, 33, 16.5, *tail, st) == ERR_UNSUPPORTED
    for transposed in (0, 1):
        assert lib._dlpd_score_rotations_oriented(None, p, p, 1, 1, 0, 32, 16.0, *tail, transposed, st) == ERR_ARG
        assert lib._dlpd_score_rotations_oriented(p, p, p, 1, 1, 0, 33, 16.5, *tail, transposed, st) == ERR_UNSUPPORTED
    if device != "cpu":
        torch.cuda.synchronize()
    assert bool((V == -7.0).all()) and float(buf.abs().max()) == 0.0
