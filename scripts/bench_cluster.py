"""Time the pose clustering (csrc/dlpd_cluster.h) at K = 2,000 / 16,384 / 65,536 poses and a radius of 9 Angstrom, on seeded
poses (not a search): atoms normal with sigma (9, 6, 4) Angstrom, ``ns`` seed poses (a random rotation, a translation on the
1.25 Angstrom grid within +-24 voxels), every pose a seed times a rotation vector N(0, 4 degrees) plus a shift of +-3 voxels.

Per K one JSON line with device-event times (median of --repeats after 2 warm-ups):
    hip_within_ms     the neighbour bitmap alone (dlpd_pose_within)
    hip_cluster_ms    bitmap + greedy scan (dlpd_pose_cluster), buffers allocated once outside the timing
    hip_scan_ms       their difference: the scan (it has no entry point of its own)
    torch_ms          the same clustering from torch.cdist in row chunks, thresholded to a bool matrix on the same device,
                      and a greedy loop on the host that reads one row per centre (wall clock, synchronised)
    numpy_ms          chunked NumPy on the CPU: the bool matrix chunk by chunk, then the same loop (K <= --cpu-max-k)
and the cluster count, the largest cluster and whether the three agree (they may differ where a pair distance falls within
float32 rounding of the radius: the count of differing labels is printed, not asserted).

    python scripts/bench_cluster.py [--repeats 5] [--cpu-max-k 16384]

Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as entry

SIZES = (2000, 16384, 65536)
RADIUS = 9.0
RES = 1.25


def _rotations(rv):
    """Rodrigues: rotation vectors (n, 3) -> matrices"""
    th = np.linalg.norm(rv, axis=1)[:, None, None]
    Kx = np.zeros((rv.shape[0], 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -rv[:, 2], rv[:, 1], rv[:, 2], -rv[:, 0], -rv[:, 1], rv[:, 0]
    th = np.maximum(th, 1e-12)
    return np.eye(3)[None] + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)


def seeded(K, seed=0, natoms=200):
    rs = np.random.RandomState(seed)
    x = rs.normal(size=(natoms, 3)) * np.array([9.0, 6.0, 4.0])
    x -= 0.5 * (x.max(axis=0) + x.min(axis=0))
    ns = max(12, K // 40)
    axis = rs.normal(size=(ns, 3))
    axis *= rs.uniform(0, np.pi, size=(ns, 1)) / np.linalg.norm(axis, axis=1, keepdims=True)
    Rs, ts = _rotations(axis), rs.randint(-24, 25, size=(ns, 3)) * RES
    which = rs.randint(0, ns, size=K)
    R = _rotations(rs.normal(size=(K, 3)) * np.radians(4.0)) @ Rs[which]
    t = ts[which] + rs.randint(-3, 4, size=(K, 3)) * RES
    return x, R, t


def greedy_rows(row_of, K):
    """The greedy loop over rows of a bool neighbour matrix, one row per centre: row_of(c) -> (K) bool numpy"""
    removed = np.zeros(K, dtype=bool)
    labels = np.full(K, -1, dtype=np.int32)
    centres, sizes = [], []
    c = 0
    while c < K:
        fresh = row_of(c) & ~removed
        fresh[c] = True
        labels[fresh] = len(centres)
        centres.append(c)
        sizes.append(int(fresh.sum()))
        removed |= fresh
        rest = np.flatnonzero(~removed[c:])
        c = c + int(rest[0]) if len(rest) else K
    return np.array(centres), np.array(sizes), labels


def torch_cluster(E, r, chunk=8192):
    K = E.shape[0]
    B = torch.empty(K, K, dtype=torch.bool, device=E.device)
    for i in range(0, K, chunk):
        B[i:i + chunk] = torch.cdist(E[i:i + chunk], E) <= r
    return greedy_rows(lambda c: B[c].cpu().numpy(), K)


def numpy_cluster(E, r, chunk=256):
    K = E.shape[0]
    B = np.empty((K, K), dtype=bool)
    r2 = np.float32(r * r)
    for i in range(0, K, chunk):
        d = E[i:i + chunk, None, :] - E[None, :, :]
        B[i:i + chunk] = np.einsum("ijk,ijk->ij", d, d) <= r2
    return greedy_rows(lambda c: B[c], K)


def _events(fn, repeats, warmup=2):
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


def _wall(fn, repeats):
    ms, out = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-max-k", type=int, default=16384)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cluster.py needs a GPU"
    entry.build()
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd._lib import get_lib
    from deeplocalproteindocking_amd.engine import _ptr, _stream
    lib, dev = get_lib(), torch.device("cuda:0")
    for K in args.sizes:
        x, R, t = seeded(K)
        E, M = ops.pose_embedding(x, R, t, device=dev)
        nbytes = lib.call("dlpd_pose_cluster_ws", K)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        cen, siz, lab = (torch.empty(K, dtype=torch.int32, device=dev) for _ in range(3))
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        st = _stream(dev)

        def within():
            lib.call("dlpd_pose_within", _ptr(E), K, RADIUS, _ptr(ws), st)

        def cluster():
            lib.call("dlpd_pose_cluster", _ptr(E), K, RADIUS, 0, _ptr(cen), _ptr(siz), _ptr(lab), _ptr(cnt), _ptr(ws), nbytes, st)
        row = {"part": "pose clustering, K = %d, radius %.1f A (device %s)" % (K, RADIUS, torch.cuda.get_device_name(0)),
               "K": K, "max_abs_embedding": M, "bitmap_bytes": nbytes}
        row["hip_within_ms"] = _events(within, args.repeats)
        row["hip_cluster_ms"] = _events(cluster, args.repeats)
        row["hip_scan_ms"] = row["hip_cluster_ms"]["median"] - row["hip_within_ms"]["median"]
        n = int(cnt.item())
        hip = (cen[:n].cpu().numpy(), siz[:n].cpu().numpy(), lab.cpu().numpy())
        row["clusters"], row["largest"] = n, int(hip[1].max())
        row["pairs_per_s_bitmap"] = K * K / (row["hip_within_ms"]["median"] * 1e-3)
        row["torch_ms"], tc = _wall(lambda: torch_cluster(E, RADIUS), max(1, min(args.repeats, 3)))
        row["torch_labels_differing"] = int((tc[2] != hip[2]).sum())
        row["torch_over_hip"] = row["torch_ms"]["median"] / row["hip_cluster_ms"]["median"]
        if K <= args.cpu_max_k:
            Eh = E.cpu().numpy()
            t0 = time.perf_counter()
            nc = numpy_cluster(Eh, RADIUS)
            row["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            row["numpy_labels_differing"] = int((nc[2] != hip[2]).sum())
            row["numpy_over_hip"] = row["numpy_ms"] / row["hip_cluster_ms"]["median"]
        print(json.dumps(row), flush=True)
        del ws, E
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
