"""Time the all-contacts kernel (csrc/dlpd_contacts.h, ops.pose_contact_counts) at K = 2,000 and 65,536 poses on the synthetic
target of scripts/bench_evaluate.py extended to whole proteins: behind each of its two facing interface layers lie
``--layers`` - 1 more layers of full-atom residues (5 or 14 atoms), so most residues are away from the interface, as in a
real complex.  One JSON line per K:

    hip_contacts_all_ms {median, min, max}    the kernel alone, CUDA events round the C-ABI call
    hip_fnonnat_ms                            ops.pose_fnonnat as a caller sees it (wall clock, synchronised, poses on the device)
    host_ms                                   the host's per-pose loop -- a cKDTree of the receptor's atoms queried with the posed
                                              ligand's, the route ``native_contact_pairs`` takes -- measured on --host-poses
                                              poses and SCALED to K (host_measured_ms is what was measured)
    host_over_hip                             host_ms / hip_fnonnat_ms
    counts_differing                          poses of the host subset whose (n_dec, n_corr) differ (float64 against float32 at
                                              the cutoff: a pair within the band of tests/fnonnat_checks.py may differ)

    python scripts/bench_fnonnat.py [--repeats 5] [--host-poses 200] [--layers 4]

Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import __graft_entry__ as entry
from bench_evaluate import CUTOFF, _events, _rotations, poses

SIZES = (2000, 65536)


def target(seed=0, nres=49, layers=4):
    rs = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(nres)))

    def layer(z):
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:nres] * 3.8
        cen = np.concatenate([g - g.mean(axis=0), np.full((nres, 1), z)], axis=1) + rs.normal(size=(nres, 3)) * 0.4
        return [cen[i] + np.concatenate([np.zeros((1, 3)), rs.normal(size=(13 if i % 4 == 1 else 4, 3)) * 0.9]) for i in range(nres)]
    off = np.array([4.0, 3.0, -6.0])
    rec_res = [r + off for k in range(layers) for r in layer(-3.8 * k)]
    lig_res = [r + off for k in range(layers) for r in layer(3.6 + 3.8 * k)]
    Rn, tn = _rotations(rs.normal(size=(1, 3)))[0], np.array([7.0, 2.0, -4.0])
    rec, lig_native = np.concatenate(rec_res), np.concatenate(lig_res)
    rec_off, lig_off = np.cumsum([0] + [len(r) for r in rec_res]).astype(np.int32), np.cumsum([0] + [len(r) for r in lig_res]).astype(np.int32)
    from scipy.spatial import cKDTree
    rec_residue, lig_residue = np.repeat(np.arange(len(rec_res)), np.diff(rec_off)), np.repeat(np.arange(len(lig_res)), np.diff(lig_off))
    pairs = sorted(set((int(rec_residue[i]), int(lig_residue[j])) for j, hits in enumerate(cKDTree(rec).query_ball_point(lig_native, CUTOFF))
                       for i in hits))
    lig = (lig_native - tn) @ Rn
    a, y = rec[rec_off[:nres]], lig[lig_off[:nres]]
    return dict(rec=rec, lig=lig, rec_off=rec_off, lig_off=lig_off, residue_pairs=pairs, rec_residue=rec_residue, lig_residue=lig_residue,
                pair=(a, y, np.concatenate([a, y @ Rn.T + tn])), Rn=Rn, tn=tn, centre=lig_native[:lig_off[nres]].mean(axis=0))


def host_counts(tg, P):
    from scipy.spatial import cKDTree
    tree, native = cKDTree(tg["rec"]), set(tg["residue_pairs"])
    out = []
    for p in P:
        posed = tg["lig"] @ p[:9].reshape(3, 3).T + p[9:]
        found = set()
        for j, hits in enumerate(tree.query_ball_point(posed, CUTOFF)):
            for i in hits:
                found.add((int(tg["rec_residue"][i]), int(tg["lig_residue"][j])))
        out.append((len(found), len(found & native)))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-poses", type=int, default=200)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fnonnat.py needs a GPU"
    entry.build()
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd._lib import get_lib
    from deeplocalproteindocking_amd.engine import _ptr, _stream
    from deeplocalproteindocking_amd.Results.InterfaceSelection import native_reference_from_points
    lib, dev = get_lib(), torch.device("cuda:0")
    tg = target(layers=args.layers)
    native = native_reference_from_points([tg["pair"]], tg["pair"][1], tg["pair"][1], tg["rec"][:1], tg["lig"][:1], [(0, 1, 0, 1)], CUTOFF,
                                          all_rec=(tg["rec"], tg["rec_off"]), all_lig=(tg["lig"], tg["lig_off"]),
                                          all_pairs=tg["residue_pairs"]).to(dev)
    tb = native.all
    NRa, NLa, NRres, NLres = len(tg["rec"]), len(tg["lig"]), len(tg["rec_off"]) - 1, len(tg["lig_off"]) - 1
    for K in args.sizes:
        Ph = poses(tg, K)
        P = torch.from_numpy(Ph).to(dev)
        nd, nc = (torch.empty(K, dtype=torch.int32, device=dev) for _ in range(2))
        st = _stream(dev)

        def kernel():
            lib.call("dlpd_pose_contacts_all", _ptr(P), K, _ptr(tb["rec_atoms"]), _ptr(tb["rec_off"]), _ptr(tb["rec_sph"]), NRa, NRres,
                     _ptr(tb["lig_atoms"]), _ptr(tb["lig_off"]), _ptr(tb["lig_sph"]), NLa, NLres, tb["rec_off_host"].ctypes.data,
                     tb["lig_off_host"].ctypes.data, _ptr(tb["native_bits"]), float(tb["lig_extent"]), CUTOFF, _ptr(nd), _ptr(nc), st)
        row = {"part": "all contacts, K = %d (device %s)" % (K, torch.cuda.get_device_name(0)), "K": K, "native_pairs": len(tg["residue_pairs"]),
               "rec_atoms": NRa, "lig_atoms": NLa, "rec_residues": NRres, "lig_residues": NLres, "library": os.path.basename(lib.path)}
        row["hip_contacts_all_ms"] = _events(kernel, args.repeats)
        wall = []
        for _ in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = ops.pose_fnonnat(P, native)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        row["hip_fnonnat_ms"] = float(np.median(wall[1:]))
        n = min(args.host_poses, K)
        t0 = time.perf_counter()
        h = host_counts(tg, Ph[:n])
        row["host_poses"], row["host_measured_ms"] = n, (time.perf_counter() - t0) * 1e3
        row["host_ms"] = row["host_measured_ms"] * K / n                    # SCALED from the subset
        row["host_over_hip"] = row["host_ms"] / row["hip_fnonnat_ms"]
        d = np.stack([nd[:n].cpu().numpy(), nc[:n].cpu().numpy()], axis=1)
        row["counts_differing"] = int((d != h).any(axis=1).sum())
        row["n_dec_range"] = [int(nd.min()), int(nd.max())]
        row["fnonnat_native_pose"] = float(f[0])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
