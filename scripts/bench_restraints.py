"""Measure the search under distance restraints (csrc/dlpd_restrain.h).  One JSON line per result.

    python scripts/bench_restraints.py kernel [--repeats 9]
        dlpd_topk_restrain alone, nb = 32 rotations at n = 128 and n = 160, J = 1, 8, 32 (need = 1: no restraint is skipped),
        every rotation (no candidate counts): device-event time (median after 2 warm-ups), the algorithmic bytes 2 nb n^3 4
        (one read and one write of the volume), their share of 8 TB/s.  Balls of 8 voxels spread over the grid, on Gaussian
        scores (half the voxels negative: the predicate runs for every thread of a live tile).
    python scripts/bench_restraints.py step [--workload config2|real] [--steps 24] [--rounds 3]
        the pipelined step of bench.py's workload, ALTERNATING in one process (--rounds times each, each measurement a fresh
        search of the same stratified batches): no restraints; one restraint of 8, 16, 24, 32 voxels with the rebuild of
        overflowed candidate lists and without it.  Wall ms per 16 rotations, the share of rotations that went through
        dlpd_topk_restrain + the radix select, and the share whose list was rebuilt.
    python scripts/bench_restraints.py buys [--max_conf 2000] [--box 80] [--angle_inc 20]
        what it buys: the synthetic protein-sized PDB pair of bench_exclusion.py docked with Docker.dockSE3 three ways -- free,
        free and then filtered by Docker.restraint_report, restrained -- under ONE restraint of 8 .. 10 Angstrom between the two
        C-alpha atoms that lie nearest to 9 Angstrom apart in the free search's best pose (the pair has no native complex: that
        pose stands in for the known interface).  Entries that satisfy it, the rank of the first, the wall time.

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
    from deeplocalproteindocking_amd.Utils.Restraints import RestraintTable
    nb = 32
    for n in (128, 160):
        g = torch.Generator(device="cpu").manual_seed(n)
        V = torch.randn(nb, n * n * n, generator=g).to(dev)
        Vs = torch.empty_like(V)
        ids = torch.arange(nb, dtype=torch.int32, device=dev)
        rng = np.random.RandomState(n)
        for J in (1, 8, 32):
            c = np.rint(256 * rng.uniform(-n / 2 + 8, n / 2 - 9, size=(nb, J, 3)))
            tab = RestraintTable(c, np.zeros(J), np.full(J, 8 * 256), 1)
            cen, bnd = torch.from_numpy(tab.centres).to(dev), torch.from_numpy(tab.bounds).to(dev)
            call = lambda: lib.call("dlpd_topk_restrain", V.data_ptr(), Vs.data_ptr(), nb, n, ids.data_ptr(), cen.data_ptr(),
                                    bnd.data_ptr(), J, 1, 0, 0, torch.cuda.current_stream(dev).cuda_stream)
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
            print(json.dumps({"bench": "kernel", "n": n, "nb": nb, "J": J, "ms": ms, "ms_min": float(min(times)), "ms_max": float(max(times)),
                              "algorithmic_bytes": alg, "alg_GBps": alg / (ms * 1e-3) / 1e9, "share_of_8TBps": alg / (ms * 1e-3) / HBM_PEAK,
                              "allowed_negatives_per_rotation": float((Vs < 0).sum()) / nb}), flush=True)


class PathCounter(object):
    """Counts, on the device and without a synchronisation, the rotations whose candidate list was not complete when the
    select consumed it (they take dlpd_topk_restrain and the radix select), and those whose overflowed list
    dlpd_topk_restrain_cand rebuilt."""

    def __init__(self, top):
        self.top, self.inner, self.lib = top, top.select, top.lib
        self.full = torch.zeros((), dtype=torch.int64, device=top.device)
        self.rebuilt = torch.zeros((), dtype=torch.int64, device=top.device)
        self.total, self.now = 0, None
        top.select, top.lib = self, self

    def call(self, name, *args):
        rc = self.lib.call(name, *args)
        if name == "dlpd_topk_restrain_cand" and self.now is not None:
            cset, nb, before = self.now
            c, B = cset["count"], self.top.batch
            over = (c[B:B + nb] != 0) | (c[:nb] > cset["cap"])
            self.full += over.sum()
            self.rebuilt += ((before[B:B + nb] == 0) & (before[:nb] > cset["cap"]) & ~over).sum()
        return rc

    def __getattr__(self, name):
        return getattr(self.lib, name)

    def __call__(self, V, nb, cset=None, rot_ids=None):
        self.total += nb
        if cset is None:
            self.full += nb
        elif self.top.restraints is None:
            c = cset["count"]
            self.full += ((c[self.top.batch:self.top.batch + nb] != 0) | (c[:nb] > cset["cap"])).sum()
        else:
            self.now = (cset, nb, cset["count"].clone())
        out = self.inner(V, nb, cset, rot_ids)
        self.now = None
        return out

    def reset(self):
        self.full.zero_()
        self.rebuilt.zero_()
        self.total = 0


def bench_step(args, dev):
    import bench
    from deeplocalproteindocking_amd.engine import DeviceTopList, DockingEngine
    from deeplocalproteindocking_amd.Utils.Restraints import Restraint, restraint_table
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
    counter = PathCounter(eng.top)
    res, L = 1.25, wl["L"]
    # one restraint: a ligand point off its centre against a receptor point a third of the box away; dmax in voxels
    variants = [("free", None, DeviceTopList.REBUILD_LIMIT)]
    for vox in (8, 16, 24, 32):
        tab = restraint_table(R_all, [Restraint([0.35 * L * res, -0.2 * L * res, 0.1 * L * res], [4.0, -3.0, 2.0], dmax=vox * res)], res)
        variants += [("dmax %d voxels, rebuild" % vox, tab, 1 << 30), ("dmax %d voxels, no rebuild" % vox, tab, None)]
    results = {}
    for rnd in range(args.rounds + 1):                                    # (round 0 warms every variant up: Vs, the side stream)
        for name, tab, limit in variants:
            eng.restraints = tab
            eng.top.REBUILD_LIMIT = limit
            eng.reset_top()
            bench.time_steps(eng, Rd, idd, tr_of, qd_of, nb, 0, 2)
            eng.finish()
            torch.cuda.synchronize()
            counter.reset()
            t0 = time.perf_counter()
            bench.time_steps(eng, Rd, idd, tr_of, qd_of, nb, 2, args.steps)
            eng.finish()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            if rnd:
                neg = int((eng.top_entries()[2] < 0).sum())
                results.setdefault(name, []).append((ms * 16.0 / nb, float(counter.full) / max(1, counter.total),
                                                     float(counter.rebuilt) / max(1, counter.total), neg,
                                                     0 if tab is None else tab.cube_volume()))
    for name, _, _ in variants:
        v = results[name]
        ms = [x[0] for x in v]
        print(json.dumps({"bench": "step", "workload": wl["desc"], "variant": name, "steps": args.steps, "rotations_per_step": nb,
                          "cube_voxels": v[0][4], "ms_per_16_rotations": ms, "median": float(np.median(ms)),
                          "spread": float(max(ms) - min(ms)), "share_of_rotations_on_the_full_path": [x[1] for x in v],
                          "share_of_rotations_rebuilt": [x[2] for x in v], "negative_entries": [x[3] for x in v]}), flush=True)


def bench_buys(args, dev):
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from synth_pdb import write_protein_like_pdb
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Models import GlobalDockingModel, SE3MultiResReprScalar, SimpleFilter
    from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend, read_pdb_atoms
    from deeplocalproteindocking_amd.Utils.Restraints import Restraint
    from deeplocalproteindocking_amd.Utils.Rotations import Rotations
    torch.manual_seed(3)
    repr_ = SE3MultiResReprScalar(multiplier=8)
    filt = SimpleFilter(repr_.get_num_outputs())
    model = GlobalDockingModel(repr_, filt, threshold_clash=300.0).to(dev)
    with tempfile.TemporaryDirectory(prefix="dlpd_rst_") as tmp, torch.no_grad():
        frec, flig = os.path.join(tmp, "rec.pdb"), os.path.join(tmp, "lig.pdb")
        write_protein_like_pdb(frec, 160, 31)
        write_protein_like_pdb(flig, 110, 32)
        R = Rotations(args.angle_inc, allow_generated=True, verbose=False).R
        dk = Docker(model, rotations=R, box_size=args.box, resolution=1.25, max_conf=args.max_conf, device=dev,
                    coords_backend=CoordsBackend())
        W = [w.detach().clone() for w in filt.parameters_tuple()]
        # (the seeded random filter, shifted so that a pose without contact scores 0: bench.py's real_protein workload)
        c0 = float((W[2].reshape(1, -1) @ torch.relu(W[1].reshape(-1, 1))).reshape(-1)[0] + W[3].reshape(-1)[0])
        filt.fc[2].bias.sub_(c0)
        p = dk.prepare(frec, flig, "SE3")

        def search(tag):
            dk.new_log(os.path.join(tmp, tag + ".dat"))
            t0 = time.perf_counter()
            dk.dockSE3(frec, flig, 2, prepared=p)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            dk.cleanup()
            return list(dk.top_list), wall
        search("warm")
        free, wall_free = search("free")
        # the interface of the free search's best pose: the C-alpha pair nearest to 9 Angstrom apart
        ca = lambda f, sh: np.array([x for x, nm in zip(*[read_pdb_atoms(f)[i] for i in (0, 4)]) if nm == "CA"]) + \
            np.asarray(torch.as_tensor(sh).detach().cpu(), dtype=np.float64).reshape(3)
        rec_ca, lig_ca = ca(frec, p.receptor_shift), ca(flig, p.ligand_shift)
        Rm, t, _, _ = dk._pose_arrays(free[:1])
        posed = lig_ca @ Rm[0].T + t[0] * dk.resolution
        d = np.linalg.norm(rec_ca[:, None, :] - posed[None, :, :], axis=2)
        i, j = np.unravel_index(np.argmin(np.abs(d - 9.0)), d.shape)
        dk.restraints = [Restraint(rec_ca[i], lig_ca[j], dmax=10.0, dmin=8.0)]
        t0 = time.perf_counter()
        rep_free = dk.restraint_report(free)
        wall_filter = time.perf_counter() - t0
        restrained, wall_rst = search("restrained")
        rep_rst = dk.restraint_report(restrained)

        def row(way, top, rep, wall):
            ok = [k for k, (e, s) in enumerate(zip(top, rep)) if s >= 1 and e[4] < 0]
            print(json.dumps({"bench": "buys", "way": way, "max_conf": args.max_conf, "rotations": int(dk.rot.R.shape[0]),
                              "pair_distance_in_best_free_pose": float(d[i, j]), "entries": len(top),
                              "negative_entries": int(sum(e[4] < 0 for e in top)), "entries_satisfying": len(ok),
                              "rank_of_first_satisfying": (ok[0] + 1) if ok else None,
                              "best_satisfying_score": float(top[ok[0]][4]) if ok else None,
                              "worst_satisfying_score": float(top[ok[-1]][4]) if ok else None, "wall_s": wall}), flush=True)
        row("free search", free, rep_free, wall_free)
        row("free search, then restraint_report as a filter", [e for e, s in zip(free, rep_free) if s >= 1],
            [s for s in rep_free if s >= 1], wall_free + wall_filter)
        row("restrained search", restrained, rep_rst, wall_rst)


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
