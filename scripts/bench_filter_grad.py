"""Time the filter stage of a global training step -- forward + backward of the per-voxel MLP over the correlation volumes -- at
the reference's shapes [16 @ 160^3 + 32 @ 80^3] and at 48 @ 128^3, hidden width 24, one batch entry: the fused path
(ops.filter_volumes_autograd: the inference kernel forward, csrc/dlpd_filter_grad.h backward) against the module path
(interpolate, cat, permute + reshape, Linear, ReLU, Linear under torch autograd -- the graph branch of
GlobalDockingModel.forward), in one session on one device.  All six gradients are asked for on both paths.  Prints one JSON line
per shape: device-event times (median of --repeats after 3 warm-ups), the ratio, the peak of torch.cuda.max_memory_allocated
over a step of each path (above what the inputs and parameters hold), the bytes the fused passes move (counted from the shapes,
below) and the fraction of the HBM peak they reach.

    python scripts/bench_filter_grad.py [--repeats 20]

Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as entry

# (C0, N0, C1, N1, H)
SHAPES = ((16, 160, 32, 80, 24), (48, 128, 0, 0, 24))
HBM_PEAK = 8.0e12                   # bytes / s, the specification (a float4 copy reaches 6.3e12)


def fused_bytes(C0, N0, C1, N1):
    """Bytes the two fused passes read + write, from the shapes (float32): the forward reads the volumes and writes V; the
    backward reads the volumes and g and writes the two gradients (the parameters and their partial sums are kilobytes)."""
    vol = (C0 * N0 ** 3 + C1 * N1 ** 3) * 4
    grid = N0 ** 3 * 4
    return {"forward": vol + grid, "backward": 2 * vol + grid}


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


def _peak(fn):
    """Peak of the allocator over one call of fn, above what is allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_filter_grad.py needs a GPU"
    entry.build()
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.Models import SimpleFilter
    dev = torch.device("cuda:0")
    for C0, N0, C1, N1, H in SHAPES:
        gen = torch.Generator().manual_seed(5)
        convs = [torch.randn(1, C0, N0, N0, N0, generator=gen).to(dev).requires_grad_()]
        if C1:
            convs.append(torch.randn(1, C1, N1, N1, N1, generator=gen).to(dev).requires_grad_())
        torch.manual_seed(6)
        filt = SimpleFilter([2 * H]).to(dev)            # Linear(C0 + C1 = 2 H, H), ReLU, Linear(H, 1)
        assert filt.fc[0].in_features == C0 + C1 and filt.fc[0].out_features == H
        params = [filt.fc[0].weight, filt.fc[0].bias, filt.fc[2].weight, filt.fc[2].bias]
        g = torch.randn(1, N0, N0, N0, generator=gen).to(dev)

        def fused_forward():
            return ops.filter_volumes_autograd(convs, *params)

        def module_forward():
            same = [c if c.shape[2] == N0 else torch.nn.functional.interpolate(c, size=(N0, N0, N0)) for c in convs]
            V = torch.cat(same, dim=1).permute(0, 2, 3, 4, 1).reshape(N0 * N0 * N0, -1)
            return filt(V).reshape(1, N0, N0, N0)

        def step(forward):
            return lambda: torch.autograd.grad(forward(), convs + params, g)

        # the two paths compute the same thing: max |fused - module| / max |module| per gradient goes into the row.  (Two float32
        # evaluations of `pre` differ in the last bits, so among millions of voxels a few ReLU gates fall on different sides
        # and the volumes' gradients differ THERE by a whole term; what the kernel owes float64 is the tests' business,
        # tests/filter_grad_checks.py, which leave those voxels out.)
        a, b = step(fused_forward)(), step(module_forward)()
        names = ["gconv0"] + (["gconv1"] if C1 else []) + ["gW1", "gb1", "gW2", "gb2"]
        gap = {n: float((x - y).abs().max()) / float(y.abs().max()) for n, x, y in zip(names, a, b)}
        del a, b
        by = fused_bytes(C0, N0, C1, N1)
        row = {"part": "filter stage forward + backward, [%d @ %d^3%s], H = %d (device events)" %
                       (C0, N0, " + %d @ %d^3" % (C1, N1) if C1 else "", H)}
        row["fused_minus_module_over_max"] = gap
        with torch.no_grad():
            row["fused_forward_ms"] = _timed(lambda: ops.filter_volumes([c.detach() for c in convs], *[p.detach() for p in params[:3]],
                                                                        float(params[3].detach()[0])), args.repeats)
        row["fused_step_ms"] = _timed(step(fused_forward), args.repeats)
        V = fused_forward()
        row["fused_backward_ms"] = _timed(lambda: torch.autograd.grad(V, convs + params, g, retain_graph=True), args.repeats)
        del V
        row["module_step_ms"] = _timed(step(module_forward), args.repeats)
        row["module_over_fused"] = row["module_step_ms"]["median"] / row["fused_step_ms"]["median"]
        row["fused_peak_bytes"] = _peak(step(fused_forward))
        row["module_peak_bytes"] = _peak(step(module_forward))
        row["fused_bytes"] = by
        sec = row["fused_step_ms"]["median"] * 1e-3
        row["fused_TB_per_s"] = sum(by.values()) / sec / 1e12
        row["fused_fraction_of_hbm_peak"] = sum(by.values()) / sec / HBM_PEAK
        print(json.dumps(row), flush=True)
        del convs, g, filt, params
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
