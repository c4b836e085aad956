"""Time the backward of VolumeConvolution (csrc/dlpd_corr_grad.h) at the reference's shapes [16 @ 80^3], [32 @ 40^3] and at
48 @ 64^3: the library call (five passes), the whole backward as autograd runs it (+ the two spectra it recomputes), the
forward VolumeConvolution at the same shape, and the backward of a pure torch.fft restatement under torch autograd on the
same device.  Prints one JSON line per shape, with the bytes each pass moves (computed from the shapes, below) and the
fraction of the HBM peak the library call reaches.

    python scripts/bench_corr_grad.py [--repeats 20]            # device-event timing
    python scripts/bench_corr_grad.py --profile prof/corr_grad  # + time per pass: a child process under
                                                                #   rocprofv3 --kernel-trace --stats
    python scripts/bench_corr_grad.py --kernel-only             # what that child runs

Needs a GPU: no CPU fallback."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as entry

SHAPES = ((16, 80), (32, 40), (48, 64))
STEPS = 10
HBM_PEAK = 8.0e12                   # bytes / s, the specification (a float4 copy reaches 6.3e12)
PASSES = ("a: z R2C", "b: y forward", "c: x forward, products, x inverse", "d: y inverse (x2)", "e: z C2R (x2)")


def pass_bytes(nvol, L):
    """Bytes each pass reads + writes for both gradients, from the shapes (complex64 = 8, float32 = 4)."""
    N, NZ = 2 * L, L + 1
    spec = nvol * NZ * N * N * 8
    h, d = nvol * NZ * L * N * 8, nvol * NZ * L * L * 8
    return [nvol * N ** 3 * 4 + spec, 2 * spec, 3 * spec + 2 * h, 2 * (h + d), 2 * (d + nvol * L ** 3 * 4)]


def _timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def setup(lib, dev, nvol, L):
    from deeplocalproteindocking_amd.engine import _stream
    N, NZ = 2 * L, L + 1
    gen = torch.Generator().manual_seed(3)
    v1, v2 = torch.randn(1, nvol, L, L, L, generator=gen).to(dev), torch.randn(1, nvol, L, L, L, generator=gen).to(dev)
    g = torch.randn(1, nvol, N, N, N, generator=gen).to(dev)
    st = _stream(dev)
    spec1, spec2 = (torch.empty(nvol * NZ * N * N * 2, dtype=torch.float32, device=dev) for _ in range(2))
    wsA = torch.empty(nvol * NZ * L * L * 2, dtype=torch.float32, device=dev)
    lib.call("dlpd_rfft3d_padded", v1.data_ptr(), spec1.data_ptr(), wsA.data_ptr(), nvol, L, 1.0, st)
    lib.call("dlpd_rfft3d_padded", v2.data_ptr(), spec2.data_ptr(), wsA.data_ptr(), nvol, L, 1.0, st)
    ws = torch.empty(lib.call("dlpd_correlate_grad_ws_bytes", nvol, L), dtype=torch.uint8, device=dev)
    g1, g2 = torch.empty_like(v1), torch.empty_like(v2)

    def call():
        lib.call("dlpd_correlate_grad", g.data_ptr(), spec1.data_ptr(), spec2.data_ptr(), g1.data_ptr(), g2.data_ptr(), ws.data_ptr(),
                 nvol, L, st)
    return v1, v2, g, call


def torch_fft_backward(v1, v2, g):
    N = 2 * v1.shape[-1]
    a, b = v1.clone().requires_grad_(), v2.clone().requires_grad_()
    A, B = (torch.fft.rfftn(v, s=(N, N, N), dim=(-3, -2, -1)) for v in (a, b))
    out = torch.fft.irfftn(A * B.conj(), s=(N, N, N), dim=(-3, -2, -1))
    return lambda: torch.autograd.grad(out, (a, b), g, retain_graph=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 kernel trace")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_corr_grad.py needs a GPU"
    entry.build()
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd._lib import get_lib
    lib, dev = get_lib(), torch.device("cuda:0")
    if args.kernel_only:
        for nvol, L in SHAPES:
            call = setup(lib, dev, nvol, L)[3]
            for _ in range(STEPS):
                call()
            torch.cuda.synchronize()
        return
    conv = ops.VolumeConvolution()
    for nvol, L in SHAPES:
        v1, v2, g, call = setup(lib, dev, nvol, L)
        by = pass_bytes(nvol, L)
        row = {"part": "VolumeConvolution backward %d @ %d^3, both gradients (device events)" % (nvol, L),
               "dlpd_correlate_grad_ms": _timed(call, args.repeats), "pass_bytes": dict(zip(PASSES, by)), "bytes": sum(by)}
        a, b = v1.clone().requires_grad_(), v2.clone().requires_grad_()
        out = conv(a, b)
        row["autograd_backward_ms"] = _timed(lambda: torch.autograd.grad(out, (a, b), g, retain_graph=True), args.repeats)
        del out
        with torch.no_grad():
            row["forward_ms"] = _timed(lambda: conv(v1, v2), args.repeats)
        row["torch_fft_backward_ms"] = _timed(torch_fft_backward(v1, v2, g), args.repeats)
        sec = row["dlpd_correlate_grad_ms"]["median"] * 1e-3
        row["achieved_TB_per_s"] = sum(by) / sec / 1e12
        row["fraction_of_hbm_peak"] = sum(by) / sec / HBM_PEAK
        row["backward_over_torch_fft"] = row["autograd_backward_ms"]["median"] / row["torch_fft_backward_ms"]["median"]
        row["backward_over_forward"] = row["autograd_backward_ms"]["median"] / row["forward_ms"]["median"]
        print(json.dumps(row), flush=True)
        del v1, v2, g, call, a, b
        torch.cuda.empty_cache()
    if args.profile:
        os.makedirs(args.profile, exist_ok=True)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.profile, "--",
                        sys.executable, os.path.abspath(__file__), "--kernel-only"], check=True, timeout=600, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(args.profile, "**", "*kernel_stats.csv"), recursive=True)
        assert files, "rocprofv3 wrote no kernel statistics under %s" % args.profile
        rows = list(csv.DictReader(open(files[0])))
        for nvol, L in SHAPES:
            N = 2 * L
            needles = ("k_cg_z_r2c<%d>" % N, "k_cg_rows<%d, -1>" % N, "k_cg_x<%d>" % N, "k_cg_rows<%d, 1>" % N, "k_cg_z_c2r<%d>" % N)
            ms = [sum(float(r["TotalDurationNs"]) for r in rows if n in r["Name"]) / 1e6 / STEPS for n in needles]
            by = pass_bytes(nvol, L)
            print(json.dumps({"part": "passes of the backward %d @ %d^3 (rocprofv3 --kernel-trace --stats, %d calls)" % (nvol, L, STEPS),
                              "passes": {p: {"ms": m, "bytes": b, "TB_per_s": (b / (m * 1e-3) / 1e12) if m > 0 else None,
                                             "fraction_of_hbm_peak": (b / (m * 1e-3) / HBM_PEAK) if m > 0 else None}
                                         for p, m, b in zip(PASSES, ms, by)}, "kernel_ms": sum(ms)}), flush=True)


if __name__ == "__main__":
    main()
