"""Measure the exclusion radius of the search (csrc/dlpd_suppress.h).  One JSON line per result.

    python scripts/bench_exclusion.py kernel [--repeats 9]
        dlpd_topk_suppress alone, nb = 32 rotations at n = 128 and n = 160, r = 1..4, every rotation (no candidate counts):
        device-event time (median after 2 warm-ups), the algorithmic bytes 2 nb n^3 4 (one read and one write of the volume),
        their share of 8 TB/s and the kernel's LDS bytes per block.
    python scripts/bench_exclusion.py step [--workload config2|real] [--steps 24] [--rounds 3]
        the pipelined step of bench.py's workload with exclusion 0, 1, 2, 3, ALTERNATING in one process (--rounds times each,
        each measurement a fresh search of the same stratified batches): wall ms per 16 rotations, and the share of rotations
        that went through dlpd_topk_suppress + the radix select instead of the candidate lists.
    python scripts/bench_exclusion.py buys [--max_conf 2000] [--box 80] [--angle_inc 20]
        what it buys: a synthetic protein-sized PDB pair docked with Docker.dockSE3 at r = 0..3, then the number of
        Docker.cluster centres (radius 9 Angstrom), of distinct rotations and of distinct minima (entries no other entry of the
        same rotation lies within 3 voxels of) in the list.

Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as entry

HBM_PEAK = 8.0e12


def bench_kernel(args, dev, lib):
    nb = 32
    for n in (128, 160):
        g = torch.Generator(device="cpu").manual_seed(n)
        V = torch.randn(nb, n * n * n, generator=g).to(dev)
        Vs = torch.empty_like(V)
        for r in (1, 2, 3, 4):
            call = lambda: lib.call("dlpd_topk_suppress", V.data_ptr(), Vs.data_ptr(), nb, n, r, 0, 0,
                                    torch.cuda.current_stream(dev).cuda_stream)
            times = []
            for i in range(args.repeats + 2):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                torch.cuda.synchronize()
                if i >= 2:
                    times.append(a.elapsed_time(b))
            ms = float(np.median(times))
            alg = 2.0 * nb * n ** 3 * 4
            lds = ((8 + 2 * r) * (8 + 2 * r) * (32 + 2 * r + 32) + (8 + 2 * r) * 8 * 32) * 4
            halo = (8 + 2 * r) * (8 + 2 * r) * (32 + 2 * r) / (8.0 * 8 * 32)
            print(json.dumps({"bench": "kernel", "n": n, "nb": nb, "r": r, "ms": ms, "ms_min": float(min(times)), "ms_max": float(max(times)),
                              "algorithmic_bytes": alg, "alg_GBps": alg / (ms * 1e-3) / 1e9, "share_of_8TBps": alg / (ms * 1e-3) / HBM_PEAK,
                              "lds_bytes_per_block": lds, "blocks_per_CU_by_lds": int(160 * 1024 // lds),
                              "voxels_staged_per_voxel_written": halo,
                              "surviving_negatives_per_rotation": float((Vs < 0).sum()) / nb}), flush=True)


class FullPathCounter(object):
    """Counts, on the device and without a synchronisation, the rotations whose candidate list was NOT complete when
    DeviceTopList.select consumed it (they take dlpd_topk_suppress and the radix select)."""

    def __init__(self, top):
        self.top, self.inner = top, top.select
        self.full = torch.zeros((), dtype=torch.int64, device=top.device)
        self.total = 0
        top.select = self

    def __call__(self, V, nb, cset=None, rot_ids=None):
        if cset is None:
            self.full += nb
        else:
            c = cset["count"]
            self.full += ((c[self.top.batch:self.top.batch + nb] != 0) | (c[:nb] > cset["cap"])).sum()
        self.total += nb
        return self.inner(V, nb, cset, rot_ids)


def bench_step(args, dev):
    import bench
    from deeplocalproteindocking_amd.engine import DockingEngine
    from deeplocalproteindocking_amd.Utils.Rotations import Rotations
    nb = 32
    bargs = types.SimpleNamespace(workload=args.workload, channels=None, box=None, max_conf=2000, batch=nb, k3_form=0, k1_form=0,
                                  hidden=None, natural_receptor=False, k1_occupancy="auto")
    eng, wl = bench.build_workload(args.workload, bargs, dev)
    R_all = Rotations(wl["angle"], allow_generated=True, verbose=False).R
    seq_ids, seq_key = bench.visiting_sequence(DockingEngine, R_all, np.arange(R_all.shape[0]), nb)
    nbat = len(seq_ids) // nb
    pick = np.linspace(0, nbat - 1, args.steps + 2).astype(int)
    rows = np.concatenate([np.arange(j * nb, (j + 1) * nb) for j in pick])
    ids, key_of = seq_ids[rows], seq_key[rows]
    tr_of, qd_of = key_of >= 2, (key_of % 2) == 1
    Rd = R_all[ids].to(device=dev, dtype=torch.float32).contiguous()
    idd = torch.as_tensor(ids, dtype=torch.int32).to(dev)
    counter = FullPathCounter(eng.top)
    results = {}
    for rnd in range(args.rounds + 1):                                    # (round 0 warms every radius up: Vs, the side stream)
        for r in (0, 1, 2, 3):
            eng.exclusion = r
            eng.reset_top()
            bench.time_steps(eng, Rd, idd, tr_of, qd_of, nb, 0, 2)
            eng.finish()
            torch.cuda.synchronize()
            counter.full.zero_()
            counter.total = 0
            t0 = time.perf_counter()
            bench.time_steps(eng, Rd, idd, tr_of, qd_of, nb, 2, args.steps)
            eng.finish()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            if rnd:
                results.setdefault(r, []).append((ms * 16.0 / nb, float(counter.full) / max(1, counter.total)))
    for r, v in sorted(results.items()):
        ms = [x[0] for x in v]
        print(json.dumps({"bench": "step", "workload": wl["desc"], "exclusion": r, "steps": args.steps, "rotations_per_step": nb,
                          "ms_per_16_rotations": ms, "median": float(np.median(ms)), "spread": float(max(ms) - min(ms)),
                          "share_of_rotations_on_the_full_path": [x[1] for x in v]}), flush=True)


def bench_buys(args, dev):
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from synth_pdb import write_protein_like_pdb
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Models import GlobalDockingModel, SE3MultiResReprScalar, SimpleFilter
    from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend
    torch.manual_seed(3)
    repr_ = SE3MultiResReprScalar(multiplier=8)
    filt = SimpleFilter(repr_.get_num_outputs())
    model = GlobalDockingModel(repr_, filt, threshold_clash=300.0).to(dev)
    with tempfile.TemporaryDirectory(prefix="dlpd_excl_") as tmp, torch.no_grad():
        frec, flig = os.path.join(tmp, "rec.pdb"), os.path.join(tmp, "lig.pdb")
        write_protein_like_pdb(frec, 160, 31)
        write_protein_like_pdb(flig, 110, 32)
        from deeplocalproteindocking_amd.Utils.Rotations import Rotations
        R = Rotations(args.angle_inc, allow_generated=True, verbose=False).R
        dk = Docker(model, rotations=R, box_size=args.box, resolution=1.25, max_conf=args.max_conf, device=dev,
                    coords_backend=CoordsBackend())
        W = [w.detach().clone() for w in filt.parameters_tuple()]
        # (the seeded random filter, shifted so that a pose without contact scores 0: bench.py's real_protein workload)
        c0 = float((W[2].reshape(1, -1) @ torch.relu(W[1].reshape(-1, 1))).reshape(-1)[0] + W[3].reshape(-1)[0])
        filt.fc[2].bias.sub_(c0)
        p = dk.prepare(frec, flig, "SE3")
        N = 2 * args.box
        for r in (0, 1, 2, 3):
            dk.exclusion = r
            dk.new_log(os.path.join(tmp, "pair%d.dat" % r))
            t0 = time.perf_counter()
            dk.dockSE3(frec, flig, 2, prepared=p)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            dk.cleanup()
            top = list(dk.top_list)
            dk.cluster_prepared(p, radius=9.0)
            centres = dk.clustered_list
            rot = np.array([e[0] for e in top])
            xyz = np.array([e[1:4] for e in top])
            minima = 0
            for rid in np.unique(rot):
                q = xyz[rot == rid]
                d = np.abs(q[:, None, :] - q[None, :, :])
                d = np.minimum(d, N - d).max(axis=2)
                first = np.array([not (d[i, :i] <= 3).any() for i in range(len(q))])
                minima += int(first.sum())
            print(json.dumps({"bench": "buys", "exclusion": r, "max_conf": args.max_conf, "rotations": int(dk.rot.R.shape[0]),
                              "negative_entries": int(sum(e[4] < 0 for e in top)), "cluster_centres_9A": len(centres),
                              "distinct_rotations": int(len(np.unique(rot))), "entries_3_voxels_apart_per_rotation": minima,
                              "best_score": float(top[0][4]), "kth_score": float(top[-1][4]), "search_wall_s": wall}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "step", "buys"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--workload", default="config2", choices=("config2", "real"))
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max_conf", type=int, default=2000)
    ap.add_argument("--box", type=int, default=80)
    ap.add_argument("--angle_inc", type=int, default=20)
    args = ap.parse_args()
    entry.build()
    from deeplocalproteindocking_amd._lib import get_lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    {"kernel": lambda: bench_kernel(args, dev, get_lib()), "step": lambda: bench_step(args, dev), "buys": lambda: bench_buys(args, dev)}[args.what]()


if __name__ == "__main__":
    main()
