"""Time one forward + backward of the differentiable ``ops.MultiplyVolumes`` (the local model's correlation and its adjoint
kernel, csrc/dlpd_local.h + csrc/dlpd_local_grad.h) on 8 pairs at the reference's shapes [16 @ 80^3, 32 @ 40^3], beside a
pure-torch-autograd statement of the same slices on the same device.  Prints one JSON line per part.

    python scripts/bench_local_train.py [--pairs 8] [--repeats 50]           # device-event timing of both paths
    python scripts/bench_local_train.py --profile prof/local_train           # + the adjoint kernel alone: a child process
                                                                             #   under rocprofv3 --kernel-trace --stats
    python scripts/bench_local_train.py --kernel-only                        # what that child runs

The kernel's floor at radius 0 is memory traffic: each gradient reads one volume and writes one, 4 P C L^3 4 bytes for the
two of them.  The achieved rate printed is that figure over the kernel time of the trace.  Needs a GPU: no CPU fallback."""
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

SHAPES = ((16, 80), (32, 40))


def _timed(fn, repeats, warmup=5):
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
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def _slices(t, L):
    a, b = [], []
    for v in t:
        a.append(slice(v, L) if v >= 0 else slice(0, L + v))
        b.append(slice(0, L - v) if v >= 0 else slice(-v, L))
    return (slice(None),) + tuple(a), (slice(None),) + tuple(b)


def multiply_torch(rec, lig, T):
    """MultiplyVolumes in plain torch (autograd's own backward): per pair one product of two slices whose bounds are computed
    arithmetically from int(T[i]), summed over the box."""
    L = rec.shape[-1]
    rows = []
    for i in range(rec.shape[0]):
        t = [int(v) for v in T[i]]
        if max(abs(v) for v in t) >= L:
            rows.append(rec[i, :, 0, 0, 0] * 0.0)
            continue
        a, b = _slices(t, L)
        rows.append((rec[i][a] * lig[i][b]).sum(dim=(1, 2, 3)))
    return torch.stack(rows)


def inputs(B, dev):
    g = torch.Generator().manual_seed(7)
    vols = [(torch.randn(B, C, L, L, L, generator=g).to(dev).requires_grad_(), torch.randn(B, C, L, L, L, generator=g).to(dev).requires_grad_())
            for C, L in SHAPES]
    T = torch.from_numpy(np.random.RandomState(8).randint(-20, 21, size=(B, 3))).double()
    T[0] = torch.tensor([-3.0, 5.0, -1.0])
    return vols, T


def step(mult, vols, T):
    """Forward of both resolutions, one scalar, backward into the four volumes -- what a training step asks of the correlation."""
    edge = float(vols[0][0].shape[2])
    total = 0.0
    for rec, lig in vols:
        rec.grad = lig.grad = None
        total = total + mult(rec, lig, T * float(rec.shape[2]) / edge).sum()
    total.backward()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 run of the kernel path")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_local_train.py needs a GPU"
    entry.build()
    from deeplocalproteindocking_amd.ops import MultiplyVolumes
    dev = torch.device("cuda:0")
    B = args.pairs
    vols, T = inputs(B, dev)
    mult = MultiplyVolumes()

    def torch_mult(rec, lig, Ts):
        return multiply_torch(rec, lig, Ts.trunc().tolist())
    if args.kernel_only:
        for _ in range(20):
            step(mult, vols, T)
        torch.cuda.synchronize()
        return
    # the two paths agree (values and gradients) before either is timed
    a = step(mult, vols, T).item()
    ga = [v.grad.clone() for pair in vols for v in pair]
    b = step(torch_mult, vols, T).item()
    gb = [v.grad.clone() for pair in vols for v in pair]
    worst = max(float((x - y).abs().max()) / float(y.abs().max()) for x, y in zip(ga, gb))
    assert abs(a - b) <= 1e-4 * abs(b) and worst <= 1e-5, (a, b, worst)
    k_ms = _timed(lambda: step(mult, vols, T), args.repeats)
    t_ms = _timed(lambda: step(torch_mult, vols, T), args.repeats)
    floor_bytes = sum(4 * B * C * L ** 3 * 4 for C, L in SHAPES)
    out = {"part": "forward+backward", "pairs": B, "shapes": [list(s) for s in SHAPES],
           "kernel_path_ms": {"median": k_ms[0], "min": k_ms[1], "max": k_ms[2]},
           "torch_path_ms": {"median": t_ms[0], "min": t_ms[1], "max": t_ms[2]},
           "kernel_over_torch": k_ms[0] / t_ms[0], "gradients_worst_relative_difference": worst,
           "adjoint_floor_bytes": floor_bytes}
    print(json.dumps(out), flush=True)
    if args.profile:
        os.makedirs(args.profile, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.profile, "--",
               sys.executable, os.path.abspath(__file__), "--kernel-only", "--pairs", str(B)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(args.profile, "**", "*kernel_stats.csv"), recursive=True)
        assert files, "rocprofv3 wrote no kernel statistics under %s" % args.profile
        rows = list(csv.DictReader(open(files[0])))
        fwd = [r for r in rows if "k_local_corr<" in r["Name"] or "k_local_reduce" in r["Name"]]
        bwd = [r for r in rows if "k_local_corr_grad" in r["Name"]]
        assert bwd, "the trace holds no k_local_corr_grad"
        steps = 20
        bwd_ms = sum(float(r["TotalDurationNs"]) for r in bwd) / 1e6 / steps
        fwd_ms = sum(float(r["TotalDurationNs"]) for r in fwd) / 1e6 / steps
        print(json.dumps({"part": "kernels alone (rocprofv3 --kernel-trace --stats)", "steps": steps,
                          "adjoint_ms_per_step": bwd_ms, "adjoint_launches_per_step": sum(int(r["Calls"]) for r in bwd) / steps,
                          "forward_ms_per_step": fwd_ms, "adjoint_floor_bytes": floor_bytes,
                          "adjoint_achieved_TB_per_s": floor_bytes / (bwd_ms * 1e-3) / 1e12}), flush=True)


if __name__ == "__main__":
    main()
