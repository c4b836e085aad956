"""Time the adjoint of the trilinear volume rotation (csrc/dlpd_rotate_grad.h) at the reference's shapes [16 @ 80^3, 32 @ 40^3]
for 64 poses of ONE shared ligand, beside the forward kernel (k_rotate) on the same shapes and the backward of torch's
affine_grid + grid_sample (trilinear, zeros) into its input -- what a user would otherwise write -- and one
LocalDockingModel.forward_poses step (forward + backward).  Prints one JSON line per part.

    python scripts/bench_rotate_grad.py [--poses 64] [--repeats 30]          # device-event timing
    python scripts/bench_rotate_grad.py --profile prof/rotate_grad           # + the kernels alone: a child process under
                                                                             #   rocprofv3 --kernel-trace --stats
    python scripts/bench_rotate_grad.py --counters prof/rotate_grad_pmc      # + hardware counters of the adjoint kernel, in
                                                                             #   a run of their own (no tracing beside them)
    python scripts/bench_rotate_grad.py --kernel-only | --step-only          # what those children run
    python scripts/bench_rotate_grad.py --pose-grad [--minimize-poses 32]    # the rotation's gradient with respect to its
                                                                             #   matrices (csrc/dlpd_rotate_rgrad.h): the backward
                                                                             #   of local_correlate_rotated with and without
                                                                             #   rotation_grad, the new kernel beside the adjoint on
                                                                             #   one workspace, the twelve-number kernel
                                                                             #   (csrc/dlpd_rotate_shift.h: + the offset's gradient)
                                                                             #   beside it, Docker.minimize with and without
                                                                             #   translation=True beside Docker.refine

The adjoint's floor is memory traffic: it reads B C L^3 4 bytes (the gradient of every rotated copy) and writes C L^3 4.
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

SHAPES = ((16, 80), (32, 40))
STEPS = 10


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


def rotations(P, seed=3):
    """P proper rotations (QR of a normal matrix, the sign fixed), float32 (P, 3, 3)."""
    q, r = np.linalg.qr(np.random.RandomState(seed).randn(P, 3, 3))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    return torch.from_numpy(q).float().contiguous()


def floor_bytes(P, C, L):
    return (P + 1) * C * L ** 3 * 4


def kernels(lib, dev, P):
    """Per shape: closures that launch the adjoint (stride 0: the sum over the poses) and the forward (one shared volume)."""
    from deeplocalproteindocking_amd.engine import _stream
    out = []
    R = rotations(P).to(dev)
    g_ = torch.Generator().manual_seed(5)
    for C, L in SHAPES:
        vol = torch.randn(C, L, L, L, generator=g_).to(dev)
        gout = torch.randn(P, C, L, L, L, generator=g_).to(dev)
        gvol, rot = torch.empty_like(vol), torch.empty_like(gout)
        st, c0 = _stream(dev), L / 2.0

        def adj(gout=gout, gvol=gvol, C=C, L=L, c0=c0):
            lib.call("dlpd_rotate_trilinear_grad", gout.data_ptr(), R.data_ptr(), gvol.data_ptr(), P, C, L, 0, c0, 0, st)

        def fwd(vol=vol, rot=rot, C=C, L=L, c0=c0):
            lib.call("dlpd_rotate_trilinear", vol.data_ptr(), R.data_ptr(), rot.data_ptr(), P, C, L, 0, c0, st)
        out.append((C, L, adj, fwd, vol, gout, R))
    return out


def torch_backward(vol, gout, R):
    """The backward of affine_grid + grid_sample into ONE shared input (expanded over the poses): autograd's scatter with
    float atomics, then the sum over the poses."""
    P = R.shape[0]
    v = vol.detach().clone().requires_grad_()
    theta = torch.cat([R.flip(1).flip(2), torch.zeros(P, 3, 1, device=R.device)], dim=2)
    grid = torch.nn.functional.affine_grid(theta, (P,) + tuple(vol.shape), align_corners=True)
    out = torch.nn.functional.grid_sample(v[None].expand(P, -1, -1, -1, -1), grid, mode="bilinear", padding_mode="zeros",
                                          align_corners=True)
    return lambda: torch.autograd.grad(out, v, gout, retain_graph=True)


def model_step(dev, P):
    from deeplocalproteindocking_amd.Models import E3MultiResRepr4x4, LocalDockingModel, SimpleFilter
    torch.manual_seed(1)
    net = E3MultiResRepr4x4()
    model = LocalDockingModel(net, SimpleFilter(net.get_num_outputs()), differentiable=True).to(dev).train()
    g_ = torch.Generator().manual_seed(2)
    L = SHAPES[0][1]
    rec, lig = torch.rand(1, 11, L, L, L, generator=g_).to(dev), torch.rand(1, 11, L, L, L, generator=g_).to(dev)
    R = rotations(P).to(dev)
    T = torch.from_numpy(np.random.RandomState(8).randint(-20, 21, size=(P, 3))).float().to(dev)

    def step():
        model.zero_grad()
        model.forward_poses(rec, lig, R, T).sum().backward()
    return step


def pose_grad_rows(lib, dev, P, repeats, variants=()):
    """Per shape: the backward of ops.local_correlate_rotated (radius 1, one shared ligand) with rotation_grad=True against the
    same call without it, and dlpd_rotate_trilinear_rgrad beside dlpd_rotate_trilinear_grad on the same workspace."""
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.engine import _stream
    R = rotations(P).to(dev)
    g_ = torch.Generator().manual_seed(6)
    T = torch.from_numpy(np.random.RandomState(9).randint(-10, 11, size=(P, 3))).int().to(dev)
    for C, L in SHAPES:
        rec, lig = torch.randn(C, L, L, L, generator=g_).to(dev), torch.randn(C, L, L, L, generator=g_).to(dev)
        gcorr = torch.randn(P, C, 3, 3, 3, generator=g_).to(dev)
        row = {"part": "pose gradient %d @ %d^3, %d poses of one ligand, radius 1 (device events)" % (C, L, P)}
        for name, flag in (("backward_ms", False), ("backward_rotation_grad_ms", True), ("backward_ms_again", False),
                           ("backward_rotation_grad_ms_again", True)):
            a, b, Rg = rec.clone().requires_grad_(), lig.clone().requires_grad_(), R.clone().requires_grad_()
            out = ops.local_correlate_rotated(a, b, T, Rg, radius=1, rotation_grad=flag)
            row[name] = _timed(lambda: torch.autograd.grad(out, (a, b, Rg) if flag else (a, b), gcorr, retain_graph=True), repeats)
        ws = torch.randn(P, C, L, L, L, generator=g_).to(dev)
        gvol, gR = torch.empty_like(lig), torch.empty(P, 9, device=dev)
        part = torch.empty(lib.call("dlpd_rotate_trilinear_rgrad_ws_bytes", P, L), dtype=torch.uint8, device=dev)
        st, c0 = _stream(dev), L / 2.0
        row["k_rotate_adjoint_ms"] = _timed(lambda: lib.call("dlpd_rotate_trilinear_grad", ws.data_ptr(), R.data_ptr(), gvol.data_ptr(),
                                                             P, C, L, 0, c0, 0, st), repeats)
        row["k_rotate_rgrad_ms"] = _timed(lambda: lib.call("dlpd_rotate_trilinear_rgrad", ws.data_ptr(), lig.data_ptr(), R.data_ptr(),
                                                           gR.data_ptr(), part.data_ptr(), P, C, L, 0, c0, st), repeats)
        row["k_rotate_adjoint_us_per_pose"] = 1e3 * row["k_rotate_adjoint_ms"]["median"] / P
        row["k_rotate_rgrad_us_per_pose"] = 1e3 * row["k_rotate_rgrad_ms"]["median"] / P
        row["rgrad_floor_bytes"] = (P + 1) * C * L ** 3 * 4
        row["rgrad_achieved_TB_per_s"] = row["rgrad_floor_bytes"] / (row["k_rotate_rgrad_ms"]["median"] * 1e-3) / 1e12
        print(json.dumps(row), flush=True)
        # the twelve-number kernel (gR and goff) beside the nine-number one, without and with a non-zero offset: each twice,
        # alternating
        goff = torch.empty(P, 3, device=dev)
        part12 = torch.empty(lib.call("dlpd_rotate_trilinear_pgrad_ws_bytes", P, L), dtype=torch.uint8, device=dev)
        offs = {"zero_offset": torch.zeros(P, 3, device=dev),
                "offset": torch.from_numpy(np.random.RandomState(11).uniform(-0.5, 0.5, size=(P, 3)).astype(np.float32)).to(dev)}
        row = {"part": "nine numbers (dlpd_rotate_trilinear_rgrad) beside twelve (dlpd_rotate_trilinear_pgrad) %d @ %d^3, %d poses "
                       "(device events, kernel + reduce, alternating)" % (C, L, P)}
        for rnd in range(2):
            row["rgrad_ms_round%d" % rnd] = _timed(lambda: lib.call(
                "dlpd_rotate_trilinear_rgrad", ws.data_ptr(), lig.data_ptr(), R.data_ptr(), gR.data_ptr(), part.data_ptr(), P, C, L, 0, c0,
                st), repeats)["median"]
            for name, off in offs.items():
                row["pgrad_%s_ms_round%d" % (name, rnd)] = _timed(lambda: lib.call(
                    "dlpd_rotate_trilinear_pgrad", ws.data_ptr(), lig.data_ptr(), R.data_ptr(), off.data_ptr(), gR.data_ptr(), goff.data_ptr(),
                    part12.data_ptr(), P, C, L, 0, c0, st), repeats)["median"]
        print(json.dumps(row), flush=True)
        if variants:                                          # A/B builds of the kernel: every library twice, alternating
            row = {"part": "k_rotate_rgrad variants %d @ %d^3, %d poses (device events, alternating)" % (C, L, P)}
            for rnd in range(2):
                for name, l in [("product", lib)] + list(variants):
                    pv = torch.empty(l.call("dlpd_rotate_trilinear_rgrad_ws_bytes", P, L), dtype=torch.uint8, device=dev)
                    row["%s_ms_round%d" % (name, rnd)] = _timed(lambda: l.call(
                        "dlpd_rotate_trilinear_rgrad", ws.data_ptr(), lig.data_ptr(), R.data_ptr(), gR.data_ptr(), pv.data_ptr(), P, C, L,
                        0, c0, st), repeats)["median"]
            print(json.dumps(row), flush=True)
        del ws, rec, lig


def minimize_row(dev, npose, steps=20, rounds=3):
    """Docker.minimize(steps) beside Docker.refine (default perturbations) on the top ``npose`` poses of a short search over
    bench.py's real_protein volumes: wall time per pose (``rounds`` times each, alternating, after one warm-up) and scores."""
    import time
    import bench
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Models import GlobalDockingModel, SimpleFilter
    from deeplocalproteindocking_amd.Utils.Rotations import Rotations
    L = 80
    rec, lig, recf, ligf = bench.protein_pair_volumes(dev, L)
    thr = bench.clash_threshold(recf, ligf)
    torch.manual_seed(1)
    filt = SimpleFilter([rec[0].shape[0], rec[1].shape[0]])
    with torch.no_grad():                                 # a pose without contact scores 0, as in bench.py's real_protein
        W1, b1, W2, b2 = filt.parameters_tuple()
        filt.fc[2].bias -= float((W2.reshape(1, -1) @ torch.relu(b1.reshape(-1, 1))).reshape(-1)[0] + b2.reshape(-1)[0])
    model = GlobalDockingModel(None, filt, threshold_clash=thr).to(dev).eval()
    rot = Rotations(angle_inc=15, allow_generated=True, verbose=False)
    dk = Docker(model, box_size=L, max_conf=npose, rotations=rot.R.numpy()[:256], device=dev)
    with torch.no_grad():
        top = list(dk.dock_volumes(rec, lig, recf, ligf, write=False))
    dk.release_engine()
    calls = {"refine": lambda: dk.refine(rec, lig, recf, ligf, poses=top), "minimize": lambda: dk.minimize(rec, lig, recf, ligf, poses=top, steps=steps),
             "minimize_translation": lambda: dk.minimize(rec, lig, recf, ligf, poses=top, steps=steps, translation=True)}
    ms, lists = {name: [] for name in calls}, {}
    for rnd in range(rounds + 1):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lists[name] = list(fn())
            torch.cuda.synchronize()
            if rnd > 0:
                ms[name].append(1e3 * (time.perf_counter() - t0) / len(top))
    row = {"part": "Docker.minimize(steps=%d), without and with translation=True, beside Docker.refine(5 degrees, 1), %d poses of a 256-rotation search, real_protein "
                   "volumes [16 @ 80^3, 32 @ 40^3] (wall time)" % (steps, len(top)), "search_scores": [top[0][4], float(np.mean([t[4] for t in top]))]}
    for name in calls:
        sc = [e[2] for e in lists[name]]
        row[name] = {"ms_per_pose": {"median": float(np.median(ms[name])), "min": min(ms[name]), "max": max(ms[name])},
                     "best_score": min(sc), "mean_score": float(np.mean(sc)),
                     "improved": int(sum(e[2] < top[e[3]][4] for e in lists[name]))}
    by = {e[3]: e[2] for e in lists["refine"]}
    row["minimize_below_refine"] = int(sum(e[2] < by[e[3]] for e in lists["minimize"]))
    row["minimize_translation_below_refine"] = int(sum(e[2] < by[e[3]] for e in lists["minimize_translation"]))
    by = {e[3]: e[2] for e in lists["minimize"]}
    row["minimize_translation_below_minimize"] = int(sum(e[2] < by[e[3]] for e in lists["minimize_translation"]))
    print(json.dumps(row), flush=True)


def _variant_lib(path):
    """An A/B build for --pose-grad, which may be the library of ANOTHER commit (the parent's build, to hold a kernel's time to
    what it was): bound to the entry points it has, not to the whole of today's header."""
    import ctypes
    from deeplocalproteindocking_amd._lib import SIGNATURES, DlpdLib

    class Partial(DlpdLib):
        def __init__(self, path):
            self.path = path
            self._dll = ctypes.CDLL(path)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(self._dll, name, None)
                if fn is not None:
                    fn.restype, fn.argtypes = res, args
                    setattr(self, "_" + name, fn)
    return Partial(path)


def _stats(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    assert files, "rocprofv3 wrote no kernel statistics under %s" % directory
    return list(csv.DictReader(open(files[0])))


def _ms(rows, *needles):
    return sum(float(r["TotalDurationNs"]) for r in rows if any(n in r["Name"] for n in needles)) / 1e6 / STEPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 kernel traces")
    ap.add_argument("--counters", default=None, help="directory for the counter run of the adjoint kernel")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--adjoint-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--pose-grad", action="store_true", help="only the rows of the rotation's gradient with respect to its matrices")
    ap.add_argument("--minimize-poses", type=int, default=32)
    ap.add_argument("--variants", default="", help="name=library,... : A/B builds of the adjoint kernel (scripts/build_variant.py "
                    "NAME --generic=-DDLPD_ROT_GRAD_CC=8 | -DDLPD_ROT_GRAD_SKIP=0; with --pose-grad: -DDLPD_ROT_RGRAD_VT=1 | 2 | 8), "
                    "timed beside the product library")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rotate_grad.py needs a GPU"
    entry.build()
    from deeplocalproteindocking_amd._lib import get_lib
    lib, dev, P = get_lib(), torch.device("cuda:0"), args.poses
    if args.step_only:
        step = model_step(dev, P)
        for _ in range(2 + STEPS):
            step()
        torch.cuda.synchronize()
        return
    if args.pose_grad:
        pose_grad_rows(lib, dev, P, args.repeats,
                       [(nv.split("=")[0], _variant_lib(nv.split("=")[1])) for nv in args.variants.split(",") if nv])
        torch.cuda.empty_cache()
        if args.minimize_poses > 0:
            minimize_row(dev, args.minimize_poses)
        return
    ks = kernels(lib, dev, P)
    if args.kernel_only or args.adjoint_only:
        for _ in range(STEPS):
            for _, _, adj, fwd, _, _, _ in ks:
                adj()
                if not args.adjoint_only:
                    fwd()
        torch.cuda.synchronize()
        return
    for C, L, adj, fwd, vol, gout, R in ks:
        row = {"part": "rotation %d @ %d^3, %d poses of one volume (device events)" % (C, L, P), "adjoint_ms": _timed(adj, args.repeats),
               "forward_ms": _timed(fwd, args.repeats), "torch_grid_sample_backward_ms": _timed(torch_backward(vol, gout, R), args.repeats),
               "adjoint_floor_bytes": floor_bytes(P, C, L)}
        row["adjoint_over_torch"] = row["adjoint_ms"]["median"] / row["torch_grid_sample_backward_ms"]["median"]
        row["adjoint_achieved_TB_per_s"] = row["adjoint_floor_bytes"] / (row["adjoint_ms"]["median"] * 1e-3) / 1e12
        print(json.dumps(row), flush=True)
    if args.variants:
        from deeplocalproteindocking_amd._lib import DlpdLib
        libs = [("product", lib)] + [(nv.split("=")[0], DlpdLib(nv.split("=")[1])) for nv in args.variants.split(",")]
        sets = [(name, kernels(l, dev, P)) for name, l in libs]
        for i, (C, L) in enumerate(SHAPES):
            row = {"part": "adjoint variants %d @ %d^3, %d poses (device events, alternating)" % (C, L, P)}
            for rnd in range(2):                                  # every variant twice, alternating: the spread between rounds
                for name, k in sets:
                    row["%s_ms_round%d" % (name, rnd)] = _timed(k[i][2], args.repeats)["median"]
            print(json.dumps(row), flush=True)
        del sets, libs
    del ks
    torch.cuda.empty_cache()
    if not args.skip_step:
        print(json.dumps({"part": "forward_poses step, 11 @ %d^3, %d poses (device events)" % (SHAPES[0][1], P),
                          "step_ms": _timed(model_step(dev, P), max(5, args.repeats // 3), warmup=2)}), flush=True)
    me = [sys.executable, os.path.abspath(__file__), "--poses", str(P)]
    if args.profile:
        for name, flag in (("kernels", "--kernel-only"), ("step", "--step-only")):
            if name == "step" and args.skip_step:
                continue
            d = os.path.join(args.profile, name)
            os.makedirs(d, exist_ok=True)
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + [flag],
                           check=True, timeout=900, stdout=subprocess.DEVNULL)
            rows = _stats(d)
            if name == "kernels":
                adj_ms, fwd_ms = _ms(rows, "k_rotate_adjoint"), _ms(rows, "k_rotate(")
                fl = sum(floor_bytes(P, C, L) for C, L in SHAPES)
                print(json.dumps({"part": "kernels alone, both shapes (rocprofv3 --kernel-trace --stats)", "launches": STEPS,
                                  "adjoint_ms": adj_ms, "forward_ms": fwd_ms, "adjoint_floor_bytes": fl,
                                  "adjoint_achieved_TB_per_s": fl / (adj_ms * 1e-3) / 1e12}), flush=True)
            else:
                n = (2 + STEPS) / float(STEPS)                    # (the child's two warm-up steps are in the trace)
                total = sum(float(r["TotalDurationNs"]) for r in rows) / 1e6 / STEPS
                adj_ms, corr_ms = _ms(rows, "k_rotate_adjoint"), _ms(rows, "k_local_corr", "k_local_reduce")
                print(json.dumps({"part": "forward_poses step by kernel (rocprofv3 --kernel-trace --stats)", "steps": 2 + STEPS,
                                  "rotation_adjoint_ms_per_step": adj_ms / n, "correlation_ms_per_step": corr_ms / n,
                                  "representation_and_rest_ms_per_step": (total - adj_ms - corr_ms) / n,
                                  "kernel_time_ms_per_step": total / n}), flush=True)
    if args.counters:
        os.makedirs(args.counters, exist_ok=True)
        subprocess.run(["rocprofv3", "--pmc", "SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_VMEM_RD", "SQ_WAIT_INST_ANY", "SQ_BUSY_CYCLES",
                        "--output-format", "csv", "-d", args.counters, "--"] + me + ["--adjoint-only"],
                       check=True, timeout=900, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(args.counters, "**", "*counter_collection.csv"), recursive=True)
        assert files, "rocprofv3 wrote no counters under %s" % args.counters
        sums = {}
        for r in csv.DictReader(open(files[0])):
            if "k_rotate_adjoint" in r.get("Kernel_Name", ""):
                key = (r.get("Grid_Size", "?"), r["Counter_Name"])
                sums[key] = sums.get(key, 0.0) + float(r["Counter_Value"])
        print(json.dumps({"part": "adjoint kernel counters, summed over %d launches (rocprofv3 --pmc, a run of its own)" % STEPS,
                          "counters": {"grid %s %s" % k: v for k, v in sorted(sums.items())}}), flush=True)


if __name__ == "__main__":
    main()
