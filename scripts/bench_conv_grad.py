"""Time the backward of the representation plugin's convolutions on the HIP kernels beside torch's on the same device.

Per layer shape of ``E3MultiResRepr4x4(multiplier=8)`` at box 80 with 20 volumes (the reference trains 10 pairs per batch
at box 80: twenty 11 @ 80^3 volumes through nine convolutions): the weight gradient (k_conv3d_wgrad + its reduce,
csrc/dlpd_conv_grad.h) and the input gradient (the forward kernel on gY, ops.conv3d_input_grad) against torch's
conv3d backward for the same layer; then one plugin forward + backward with ``hip_autograd`` on and off.  Device events,
median and min-max, the two paths alternating in one process and checked against each other before either is timed.
Prints one JSON line per layer and one for the step; a path that is slower than torch's is marked in its line
(``"slower_than_torch": true``), not hidden.

    python scripts/bench_conv_grad.py [--volumes 20] [--box 80] [--repeats 10] [--nparts 256]

Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as entry


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternating(fns, repeats, warmup=2):
    """Each fn in turn, ``repeats`` rounds -> per fn (median, min, max) ms."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            ms[i].append(_event_ms(fn))
    return [dict(median=float(np.median(m)), min=float(min(m)), max=float(max(m))) for m in ms]


def wgrad_truth_subset(x, gy, ks, cos, cis):
    """gW[co, ci] for a few (co, ci) pairs in float64 on the device: the definition, tap by tap."""
    D, h = x.shape[2], ks // 2
    out = torch.zeros(len(cos), len(cis), ks, ks, ks, dtype=torch.float64, device=x.device)
    for i, co in enumerate(cos):
        g = gy[:, co].double()
        for j, ci in enumerate(cis):
            xp = F.pad(x[:, ci].double(), (h,) * 6)
            for dx in range(ks):
                for dy in range(ks):
                    for dz in range(ks):
                        out[i, j, dx, dy, dz] = (g * xp[:, dx:dx + D, dy:dy + D, dz:dz + D]).sum()
    return out


def layer_shapes(net, box):
    """(name, cin, cout, ks, D, needs_input_grad) of every Conv3d of the plugin, in order."""
    out = []
    for seq_name, D in (("conv1", box), ("conv2", (box - 1) // 2 + 1)):
        for i, m in enumerate(getattr(net, seq_name)):
            if isinstance(m, torch.nn.Conv3d):
                out.append(("%s.%d" % (seq_name, i), m.in_channels, m.out_channels, m.kernel_size[0], D, len(out) > 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=20)
    ap.add_argument("--box", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--nparts", type=int, default=None)
    ap.add_argument("--part", choices=("all", "layers", "step"), default="all", help="torch's side takes seconds per call: the two parts can run apart")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_grad.py needs a GPU"
    entry.build()
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.Models import E3MultiResRepr4x4
    dev = torch.device("cuda:0")
    B = args.volumes
    torch.manual_seed(5)
    net = E3MultiResRepr4x4(multiplier=8).to(dev)
    g = torch.Generator().manual_seed(7)
    seen = set()
    for name, cin, cout, ks, D, want_gx in (layer_shapes(net, args.box) if args.part != "step" else []):
        if (cin, cout, ks, D) in seen:
            continue
        seen.add((cin, cout, ks, D))
        x = torch.rand(B, cin, D, D, D, generator=g).to(dev)
        gy = torch.randn(B, cout, D, D, D, generator=g).to(dev)
        w = (torch.randn(cout, cin, ks, ks, ks, generator=g) * 0.05).to(dev)

        def torch_backward():
            a, b = x.detach().requires_grad_(want_gx), w.detach().requires_grad_()
            F.conv3d(a, b, padding=ks // 2).backward(gy)
            return a.grad, b.grad

        def torch_wgrad():
            return torch.nn.grad.conv3d_weight(x, w.shape, gy, padding=ks // 2)

        def hip_wgrad():
            return ops.conv3d_weight_grad(x, gy, ks, nparts=args.nparts)

        def hip_xgrad():
            return ops.conv3d_input_grad(gy, w)

        def hip_backward():
            return (hip_xgrad() if want_gx else None), hip_wgrad()
        # the two paths agree before either is timed
        tx, tw = torch_backward()
        hx, hw = hip_backward()
        dw = float((hw - tw).abs().max()) / float(tw.abs().max())
        dx = float((hx - tx).abs().max()) / float(tx.abs().max()) if want_gx else 0.0
        # ... and the weight gradients of both against float64 on a few (co, ci) pairs (the whole tensor in float64 is hours)
        cos, cis = [0, cout - 1], [0, cin - 1]
        truth = wgrad_truth_subset(x, gy, ks, cos, cis)
        scale = float(truth.abs().max())
        hip_err = float((hw[cos][:, cis].double() - truth).abs().max()) / scale
        torch_err = float((tw[cos][:, cis].double() - truth).abs().max()) / scale
        assert hip_err <= 1e-5 and dw <= 1e-2 and dx <= 1e-4, (name, hip_err, torch_err, dw, dx)
        fns = [hip_wgrad, torch_wgrad, hip_backward, torch_backward] + ([hip_xgrad] if want_gx else [])
        t = _alternating(fns, args.repeats, warmup=1)
        flop = 2.0 * B * D ** 3 * cin * cout * ks ** 3
        row = {"layer": name, "cin": cin, "cout": cout, "ks": ks, "D": D, "volumes": B,
               "hip_wgrad_ms": t[0], "torch_wgrad_ms": t[1], "hip_backward_ms": t[2], "torch_backward_ms": t[3],
               "hip_input_grad_ms": t[4] if want_gx else None,
               "wgrad_TFLOP_per_s": flop / (t[0]["median"] * 1e-3) / 1e12,
               "wgrad_max_rel_difference": dw, "input_grad_max_rel_difference": dx,
               "hip_wgrad_error_vs_float64": hip_err, "torch_wgrad_error_vs_float64": torch_err,
               "slower_than_torch": bool(t[2]["median"] > t[3]["median"]),
               "wgrad_slower_than_torch": bool(t[0]["median"] > t[1]["median"])}
        print(json.dumps(row), flush=True)
        del x, gy, w
        torch.cuda.empty_cache()
    if args.part == "layers":
        return
    # one plugin forward + backward, hip_autograd on and off
    vol = torch.rand(B, 11, args.box, args.box, args.box, generator=g).to(dev)

    def step(hip):
        net.hip_autograd = hip
        net.zero_grad()
        outs = net(vol)
        sum(o.square().mean() for o in outs).backward()
        return [p.grad.clone() for p in net.parameters()]
    ga, gb = step(True), step(False)
    worst = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(ga, gb))
    assert worst <= 1e-2, worst
    del ga, gb
    t = _alternating([lambda: step(True), lambda: step(False)], max(3, args.repeats // 3), warmup=1)
    print(json.dumps({"part": "E3MultiResRepr4x4(8) forward + backward", "volumes": B, "box": args.box,
                      "hip_autograd_ms": t[0], "torch_ms": t[1], "hip_over_torch": t[0]["median"] / t[1]["median"],
                      "gradients_worst_relative_difference": worst,
                      "slower_than_torch": bool(t[0]["median"] > t[1]["median"])}), flush=True)


if __name__ == "__main__":
    main()
