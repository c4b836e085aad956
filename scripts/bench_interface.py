"""Time the interface kernels (csrc/dlpd_interface.h) at K = 2,000 and 65,536 poses on the synthetic target and poses of
scripts/bench_fnonnat.py (196 residues and 1,412 atoms a side).  One JSON line per K:

    hip_residue_bits_ms {median, min, max}    k_pose_residue_bits alone, CUDA events round the C-ABI call
    hip_contacts_all_ms                       k_pose_contacts_all on the same inputs in the same run: it makes the same pair tests
    bits_over_contacts                        the ratio of the two medians
    hip_profile_ms                            dlpd_interface_profile (both launches), buffers allocated outside
    hip_within_ms                             dlpd_interface_within, the K x K bitmap alone
    hip_cluster_ms                            dlpd_interface_cluster: bitmap + greedy scan (threshold 0.5)
    docker_interface_ms                       ops.pose_interface_bits + ops.interface_profile as Docker.interface calls them (wall clock,
                                              synchronised, poses on the device)
    host_ms                                   the host's route -- per pose a cKDTree of the receptor's atoms queried with the posed
                                              ligand's, hits reduced to the two residue sets -- on --host-poses poses spread over
                                              --host-workers processes, SCALED to K (host_measured_ms is what was measured)
    host_over_hip                             host_ms / docker_interface_ms
    bits_differing                            poses of the host subset whose residue sets differ (float64 against float32 at the cutoff)

and one line for k_interface_within at K = 65,536 on random fingerprints of the largest size, 256 + 32 words.

    python scripts/bench_interface.py [--repeats 5] [--host-poses 200] [--host-workers 16] [--layers 4]

Needs a GPU: no CPU fallback."""
import argparse
import json
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import __graft_entry__ as entry
from bench_evaluate import CUTOFF, _events, poses
from bench_fnonnat import target

SIZES = (2000, 65536)
_TG = None


def _host_sets(P):
    """the two residue sets of every pose of ``P`` as bool rows (a worker's share)"""
    from scipy.spatial import cKDTree
    tg = _TG
    tree = cKDTree(tg["rec"])
    nr, nl = len(tg["rec_off"]) - 1, len(tg["lig_off"]) - 1
    rec, lig = np.zeros((len(P), nr), dtype=bool), np.zeros((len(P), nl), dtype=bool)
    for k, p in enumerate(P):
        posed = tg["lig"] @ p[:9].reshape(3, 3).T + p[9:]
        for j, hits in enumerate(tree.query_ball_point(posed, CUTOFF)):
            if hits:
                lig[k, tg["lig_residue"][j]] = True
                rec[k, tg["rec_residue"][hits]] = True
    return rec, lig


def host_route(tg, P, workers):
    """-> (rec (n, NRres) bool, lig (n, NLres) bool, wall ms): forked workers, started before the GPU is touched"""
    global _TG
    _TG = tg
    shares = [s for s in np.array_split(P, workers) if len(s)]
    with multiprocessing.get_context("fork").Pool(len(shares)) as pool:
        pool.map(_host_sets, [s[:1] for s in shares])                  # (workers up, scipy imported)
        t0 = time.perf_counter()
        out = pool.map(_host_sets, shares)
        ms = (time.perf_counter() - t0) * 1e3
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), ms


def unpack32(words, n):
    w = np.ascontiguousarray(words).view(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None]) & np.uint32(1)).astype(bool).reshape(w.shape[0], -1)[:, :n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-poses", type=int, default=200)
    ap.add_argument("--host-workers", type=int, default=16)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    args = ap.parse_args()
    tg = target(layers=args.layers)
    workers = max(1, min(args.host_workers, len(os.sched_getaffinity(0))))
    host = {K: host_route(tg, poses(tg, K)[:args.host_poses], workers) for K in args.sizes}      # before the first GPU call: the workers are forks
    assert torch.cuda.is_available(), "bench_interface.py needs a GPU"
    entry.build()
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd._lib import get_lib
    from deeplocalproteindocking_amd.engine import _ptr, _stream
    lib, dev = get_lib(), torch.device("cuda:0")
    tb = ops.contact_tables(tg["rec"], tg["rec_off"], tg["lig"], tg["lig_off"], tg["residue_pairs"])
    tb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in tb.items()}
    NRa, NLa, NRres, NLres = len(tg["rec"]), len(tg["lig"]), len(tg["rec_off"]) - 1, len(tg["lig_off"]) - 1
    Wr, Wl = (NRres + 31) // 32, (NLres + 31) // 32
    st = _stream(dev)
    name = torch.cuda.get_device_name(0)
    for K in args.sizes:
        Ph = poses(tg, K)
        P = torch.from_numpy(Ph).to(dev)
        nd, nc = (torch.empty(K, dtype=torch.int32, device=dev) for _ in range(2))
        rb, lb = torch.empty(K, Wr, dtype=torch.int32, device=dev), torch.empty(K, Wl, dtype=torch.int32, device=dev)
        head = (_ptr(P), K, _ptr(tb["rec_atoms"]), _ptr(tb["rec_off"]), _ptr(tb["rec_sph"]), NRa, NRres, _ptr(tb["lig_atoms"]), _ptr(tb["lig_off"]),
                _ptr(tb["lig_sph"]), NLa, NLres, tb["rec_off_host"].ctypes.data, tb["lig_off_host"].ctypes.data)

        def bits():
            lib.call("dlpd_pose_residue_bits", *head, float(tb["lig_extent"]), CUTOFF, _ptr(rb), _ptr(lb), st)

        def contacts():
            lib.call("dlpd_pose_contacts_all", *head, _ptr(tb["native_bits"]), float(tb["lig_extent"]), CUTOFF, _ptr(nd), _ptr(nc), st)
        row = {"part": "interface, K = %d (device %s)" % (K, name), "K": K, "rec_atoms": NRa, "lig_atoms": NLa, "rec_residues": NRres,
               "lig_residues": NLres, "fingerprint_words": Wr + Wl, "library": os.path.basename(lib.path)}
        row["hip_contacts_all_ms"] = _events(contacts, args.repeats)
        row["hip_residue_bits_ms"] = _events(bits, args.repeats)
        row["bits_over_contacts"] = row["hip_residue_bits_ms"]["median"] / row["hip_contacts_all_ms"]["median"]
        w = torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev)
        rf, lf = torch.empty(NRres, dtype=torch.float64, device=dev), torch.empty(NLres, dtype=torch.float64, device=dev)
        rc, lc = torch.empty(NRres, dtype=torch.int32, device=dev), torch.empty(NLres, dtype=torch.int32, device=dev)
        pbytes = lib.call("dlpd_interface_profile_ws", K, NRres, NLres)
        pws = torch.empty((pbytes + 7) // 8, dtype=torch.int64, device=dev)
        row["hip_profile_ms"] = _events(lambda: lib.call("dlpd_interface_profile", _ptr(rb), _ptr(lb), K, NRres, NLres, _ptr(w), _ptr(rf), _ptr(lf),
                                                         _ptr(rc), _ptr(lc), _ptr(pws), pbytes, st), args.repeats)
        cbytes = lib.call("dlpd_pose_cluster_ws", K)
        cws = torch.empty((cbytes + 7) // 8, dtype=torch.int64, device=dev)
        cen, siz, lab = (torch.empty(K, dtype=torch.int32, device=dev) for _ in range(3))
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        row["hip_within_ms"] = _events(lambda: lib.call("dlpd_interface_within", _ptr(rb), _ptr(lb), K, Wr, Wl, 512, _ptr(cws), st), args.repeats)
        row["hip_cluster_ms"] = _events(lambda: lib.call("dlpd_interface_cluster", _ptr(rb), _ptr(lb), K, Wr, Wl, 512, 0, _ptr(cen), _ptr(siz),
                                                         _ptr(lab), _ptr(cnt), _ptr(cws), cbytes, st), args.repeats)
        row["clusters"] = int(cnt.item())
        wall = []
        for _ in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b = ops.pose_interface_bits(P, tb, CUTOFF)
            prof = ops.interface_profile(b[0], b[1], NRres, NLres)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        row["docker_interface_ms"] = float(np.median(wall[1:]))
        host_rec, host_lig, host_measured = host[K]
        n = len(host_rec)
        row["host_poses"], row["host_workers"], row["host_measured_ms"] = n, workers, host_measured
        row["host_ms"] = host_measured * K / n                               # SCALED from the subset
        row["host_over_hip"] = row["host_ms"] / row["docker_interface_ms"]
        got_r, got_l = unpack32(b[0][:n].cpu().numpy(), NRres), unpack32(b[1][:n].cpu().numpy(), NLres)
        row["bits_differing"] = int(((got_r != host_rec).any(axis=1) | (got_l != host_lig).any(axis=1)).sum())
        row["interface_residues"] = [int((prof[2] > 0).sum()), int((prof[3] > 0).sum())]
        print(json.dumps(row), flush=True)
        del cws
    K = 65536
    g = torch.Generator(device="cpu").manual_seed(0)

    def sparse(shape, ands):                                               # random words, a bit set with probability 2^-ands
        out = torch.randint(0, 2 ** 32, shape, generator=g)
        for _ in range(ands - 1):
            out &= torch.randint(0, 2 ** 32, shape, generator=g)
        return out
    words = (sparse((32, 288), 3)[torch.randint(0, 32, (K,), generator=g)] ^ sparse((K, 288), 6)).to(torch.int32)   # 32 families, flipped bits
    rb, lb = words[:, :256].contiguous().to(dev), words[:, 256:].contiguous().to(dev)
    mask = torch.empty(K, K // 64, dtype=torch.int64, device=dev)
    row = {"part": "interface_within on 288-word fingerprints, K = %d (device %s)" % (K, name), "K": K, "fingerprint_words": 288}
    row["hip_within_ms"] = _events(lambda: lib.call("dlpd_interface_within", _ptr(rb), _ptr(lb), K, 256, 32, 512, _ptr(mask), st), args.repeats)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
