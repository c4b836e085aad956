"""Checks shared by test_k2_set_order_emu.py (emulated kernels) and test_k2_set_order_gpu.py (the gfx950 build): the slab
kernel K2 (csrc/dlpd_k2.hip, k_xy_corr) with the SET PING-PONG -- with a shared receptor a wave visits its two column sets in
alternating order from rotation to rotation and fetches the receptor values of one set per rotation, keeping the other's in
registers.  Called directly (dlpd_xy_correlate_oriented on random wsA and receptor spectra; no K1, no K3).

The reference is not the kernel: per slab, the L x L block zero-padded to N x N, numpy's forward 2-D FFT, rec * conj(.), the
unnormalised inverse, all in float64.  The bar is the yardstick of accuracy_checks.py: with e_k = kernel - float64 and
e_o = (the same computation in float32 with torch) - float64, pooled over the whole launch,

    rms(e_k) <= 2 * rms(e_o)        and        max|e_k| <= 3 * max|e_o|

e_o is measured inside every check and both ratios are printed.  The receptor slabs are random with no symmetry between
columns, so a column set multiplied with the other set's values -- or with the values of another rotation, where the receptor
differs per rotation -- is an error of the size of the output itself, not a rounding error.

The float64 transform of a launch is made one rotation at a time and dropped again (a launch of nine rotations at box 64 is
230 MB of output; its float64 image would be twice that), so nothing is cached between the cases: a rotation costs 0.1 - 0.3 s
on the host."""
import numpy as np
import torch

from accuracy_checks import MAX_MARGIN, RMS_MARGIN
from deeplocalproteindocking_amd.engine import _ptr


def _stream(device):
    return 0 if str(device) == "cpu" else torch.cuda.current_stream().cuda_stream


def _sync(device):
    if str(device) != "cpu":
        torch.cuda.synchronize()


def _crandn(shape, g):
    return torch.view_as_complex(torch.randn(*shape, 2, generator=g))


def inputs(L, CT, nb, per_rotation, seed):
    """A (nb, CT, NZ, L, L) complex64 in [x][y] order, rec (CT, NZ, N, N) or (nb, CT, NZ, N, N) in [kx][ky] order."""
    g = torch.Generator().manual_seed(seed)
    N, NZ = 2 * L, L + 1
    A = _crandn((nb, CT, NZ, L, L), g)
    rec = _crandn(((nb,) if per_rotation else ()) + (CT, NZ, N, N), g) / float(N * N)
    return A, rec


def reference(A_b, rec_b, dtype):
    """IFFT2(rec * conj(FFT2(pad(A)))) of one rotation's slabs, unnormalised inverse.  float64: numpy; float32: torch."""
    N = rec_b.shape[-1]
    L = A_b.shape[-1]
    if dtype == "f64":
        pad = np.zeros(A_b.shape[:-2] + (N, N), dtype=np.complex128)
        pad[..., :L, :L] = A_b.numpy()
        F = np.fft.fft2(pad, axes=(-2, -1))
        return np.fft.ifft2(rec_b.numpy().astype(np.complex128) * np.conj(F), axes=(-2, -1), norm="forward")
    pad = torch.zeros(A_b.shape[:-2] + (N, N), dtype=torch.complex64)
    pad[..., :L, :L] = A_b
    F = torch.fft.fft2(pad, dim=(-2, -1))
    return torch.fft.ifft2(rec_b * torch.conj(F), dim=(-2, -1), norm="forward").numpy()


def correlate(lib, device, A, rec, transposed, per_rotation):
    """dlpd_xy_correlate_oriented (dlpd_xy_correlate for untransposed slabs) into a buffer of NaN -> (nb, CT, NZ, N, N) complex64."""
    nb, CT, NZ, L, _ = A.shape
    N = 2 * L
    stored = A.transpose(-1, -2).contiguous() if transposed else A.contiguous()
    wsA = torch.view_as_real(stored).contiguous().to(device)
    r = torch.view_as_real(rec).contiguous().to(device)
    out = torch.full((nb, CT, NZ, N, N, 2), float("nan"), device=device)
    rbs = CT * NZ * N * N if per_rotation else 0
    if transposed:
        assert lib.call("dlpd_orientation_supported", L) == 1
        lib.call("dlpd_xy_correlate_oriented", _ptr(wsA), _ptr(r), _ptr(out), nb, CT, L, rbs, 1, _stream(device))
    else:
        lib.call("dlpd_xy_correlate", _ptr(wsA), _ptr(r), _ptr(out), nb, CT, L, rbs, _stream(device))
    _sync(device)
    return torch.view_as_complex(out.cpu())


class Pool:
    """Error sums of a launch, one rotation at a time."""

    def __init__(self):
        self.n, self.sk, self.so, self.mk, self.mo, self.scale = 0, 0.0, 0.0, 0.0, 0.0, 0.0

    def add(self, X, X32, X64):
        # over the real and imaginary parts as separate numbers, as accuracy_checks.yardstick sees an interleaved buffer
        ek, eo = X.astype(np.complex128) - X64, X32.astype(np.complex128) - X64
        self.n += 2 * ek.size
        self.sk += float((ek.real ** 2).sum() + (ek.imag ** 2).sum())
        self.so += float((eo.real ** 2).sum() + (eo.imag ** 2).sum())
        self.mk = max(self.mk, float(np.abs(ek.real).max()), float(np.abs(ek.imag).max()))
        self.mo = max(self.mo, float(np.abs(eo.real).max()), float(np.abs(eo.imag).max()))
        self.scale = max(self.scale, float(np.abs(X64.real).max()), float(np.abs(X64.imag).max()))

    def judge(self, label):
        rk, ro = np.sqrt(self.sk / self.n), np.sqrt(self.so / self.n)
        print("K2 SET ORDER | %-62s | rms %.3f | max %.3f | max|e_k|/max|X64| %.2e | float32 %.2e" %
              (label, rk / ro, self.mk / self.mo, self.mk / self.scale, self.mo / self.scale), flush=True)
        assert ro > 0 and self.mo > 0 and self.scale > 0, (label, "the float32 evaluation has no error here: the case measures nothing")
        assert rk <= RMS_MARGIN * ro, (label, "rms", rk, ro, rk / ro)
        assert self.mk <= MAX_MARGIN * self.mo, (label, "max", self.mk, self.mo, self.mk / self.mo)
        return rk / ro, self.mk / self.mo


def check_against_float64(lib, device, L, CT, nb, transposed, per_rotation=False, seed=7):
    """One launch against float64 by the yardstick; every element of the output is written (it starts as NaN)."""
    A, rec = inputs(L, CT, nb, per_rotation, seed + 100 * L + nb)
    X = correlate(lib, device, A, rec, transposed, per_rotation)
    assert not bool(torch.isnan(torch.view_as_real(X)).any()), "elements of the output left unwritten"
    pool = Pool()
    for b in range(nb):
        rec_b = rec[b] if per_rotation else rec
        pool.add(X[b].numpy(), reference(A[b], rec_b, "f32"), reference(A[b], rec_b, "f64"))
    return pool.judge("box %d, CT %d, nb %d, %s slabs, %s" % (L, CT, nb, "transposed" if transposed else "natural",
                                                             "receptor per rotation" if per_rotation else "shared receptor"))


def check_position_in_the_batch_changes_no_bit(lib, device, L, CT, nb, transposed, seed=11):
    """Shared receptor, the SAME A slabs at every batch position: the nb outputs are the same bits -- neither the position in
    the batch nor the order in which a wave visits its column sets (which alternates with it) reaches the arithmetic.  An
    invariant beside check_against_float64, whose inputs differ per rotation."""
    A, rec = inputs(L, CT, 1, False, seed + 100 * L)
    X = correlate(lib, device, A.expand(nb, -1, -1, -1, -1), rec, transposed, False)
    first = torch.view_as_real(X[0]).contiguous().view(torch.int32)
    assert float(X[0].abs().max()) > 0 and not bool(torch.isnan(torch.view_as_real(X)).any())
    for b in range(1, nb):
        assert torch.equal(torch.view_as_real(X[b]).contiguous().view(torch.int32), first), ("batch position", b)


def check_forward_only(lib, device, L=32, nvol=3, seed=5):
    """MODE 0 of the same kernel (no receptor, nothing to keep or to re-order) through its entry in the C ABI,
    dlpd_rfft3d_padded: the entry has no batch axis (nb = 1, the volumes are the channels), and it leaves K1's z-transformed
    slabs in wsA -- the reference transforms those, so the check is of K2 alone: out = scale * FFT2(pad(wsA)).
    MODE 0 with more than one rotation per block (dlpd_k2_forward with nb > 1) has no caller and no entry in the C ABI, so
    it is not run here; by the source it takes the written-out passes with `pingpong` false and `par` 0, i.e. the fixed
    order, and has no receptor to fetch."""
    N, NZ = 2 * L, L + 1
    g = torch.Generator().manual_seed(seed)
    vol = torch.randn(nvol, L, L, L, generator=g).to(device)
    wsA = torch.full((nvol, NZ, L, L, 2), float("nan"), device=device)
    spec = torch.full((nvol, NZ, N, N, 2), float("nan"), device=device)
    scale = 1.0 / N ** 3
    lib.call("dlpd_rfft3d_padded", _ptr(vol), _ptr(spec), _ptr(wsA), nvol, L, scale, _stream(device))
    _sync(device)
    A, X = torch.view_as_complex(wsA.cpu()), torch.view_as_complex(spec.cpu()).numpy()
    assert not bool(torch.isnan(torch.view_as_real(A)).any()) and not np.isnan(X.view(np.float32)).any()
    pad = np.zeros((nvol, NZ, N, N), dtype=np.complex128)
    pad[..., :L, :L] = A.numpy()
    X64 = np.fft.fft2(pad, axes=(-2, -1)) * np.float64(np.float32(scale))
    pad32 = torch.zeros(nvol, NZ, N, N, dtype=torch.complex64)
    pad32[..., :L, :L] = A
    X32 = (torch.fft.fft2(pad32, dim=(-2, -1)) * scale).numpy()
    pool = Pool()
    pool.add(X, X32, X64)
    return pool.judge("box %d, forward only, %d volumes" % (L, nvol))


def check_same_bits_as(lib, other, device, L, CT, nb, transposed, per_rotation=False, seed=7):
    """The same launch through two libraries (the build with the ping-pong and the one without): the same bits."""
    A, rec = inputs(L, CT, nb, per_rotation, seed + 100 * L + nb)
    X, Y = (torch.view_as_real(correlate(l, device, A, rec, transposed, per_rotation)).contiguous().view(torch.int32) for l in (lib, other))
    assert torch.equal(X, Y)
