"""Time the pose evaluation (csrc/dlpd_evaluate.h) at K = 1,000 / 16,384 / 65,536 poses on a synthetic target (no files, no
search): two facing layers of 49 residues 3.6 Angstrom apart on a 3.8 Angstrom grid, every fourth residue 14 atoms and the others
5, the native contacts the residue pairs within 5 Angstrom (302 contacts and 353 atoms a side with the defaults), one
interface pair of the residues' first atoms, the ligand RMSD over 150 points; poses are the native one times rotations
N(0, 5 degrees) about the interface and shifts N(0, 2 Angstrom), every third one anywhere.

Per K one JSON line:
    hip_rmsd_ms / hip_contacts_ms / hip_capri_ms   the three launches, device events, median of --repeats after 2 warm-ups,
                                                   buffers allocated outside the timing
    hip_evaluate_ms                                ops.pose_evaluate as a caller sees it (wall clock, synchronised, poses already
                                                   on the device)
    host_ms                                        the existing host path on the same inputs: DockerParser.interface_rmsd per
                                                   pose (one torch.linalg.svdvals each) plus a cKDTree fnat per pose (pose the
                                                   ligand's interface atoms, query the receptor's tree, count the native
                                                   pairs).  Timed on the first --host-poses poses and SCALED to K:
                                                   host_ms = measured * K / host_poses; host_measured_ms is what was measured
    host_over_hip                                  host_ms / hip_evaluate_ms
and how many of the host subset's classes and counts differ from the device's (a pair distance within float32 rounding of the
cutoff may differ: printed, not asserted).  The variant DLPD_LIB_PATH names is the one measured (a block of 256 threads per
pose: scripts/build_variant.py block256 --topk=-DEVAL_CONTACT_NT=256).

    python scripts/bench_evaluate.py [--repeats 5] [--host-poses 200]

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

SIZES = (1000, 16384, 65536)
CUTOFF = 5.0


def _rotations(rv):
    """Rodrigues: rotation vectors (n, 3) -> matrices"""
    th = np.maximum(np.linalg.norm(rv, axis=1)[:, None, None], 1e-12)
    Kx = np.zeros((rv.shape[0], 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -rv[:, 2], rv[:, 1], rv[:, 2], -rv[:, 0], -rv[:, 1], rv[:, 0]
    return np.eye(3)[None] + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)


def target(seed=0, nres=49):
    """-> dict: rec / lig atoms (residue-contiguous, lig in its own frame), ranges (C, 4), the interface pair, the ligand RMSD
    points and the native pose"""
    rs = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(nres)))

    def layer(z):
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:nres] * 3.8
        cen = np.concatenate([g - g.mean(axis=0), np.full((nres, 1), z)], axis=1) + rs.normal(size=(nres, 3)) * 0.4
        return [cen[i] + np.concatenate([np.zeros((1, 3)), rs.normal(size=(13 if i % 4 == 1 else 4, 3)) * 0.9]) for i in range(nres)]
    rec_res, lig_res = [r + [4.0, 3.0, -6.0] for r in layer(0.0)], [r + [4.0, 3.0, -6.0] for r in layer(3.6)]
    pairs = [(i, j) for j, l in enumerate(lig_res) for i, r in enumerate(rec_res)
             if np.sqrt(((r[:, None] - l[None]) ** 2).sum(axis=2)).min() <= CUTOFF]
    Rn, tn = _rotations(rs.normal(size=(1, 3)))[0], np.array([7.0, 2.0, -4.0])
    rstart, lstart = np.cumsum([0] + [len(r) for r in rec_res]), np.cumsum([0] + [len(r) for r in lig_res])
    rec, lig_native = np.concatenate(rec_res), np.concatenate(lig_res)
    lig = (lig_native - tn) @ Rn
    ranges = np.array([(rstart[i], rstart[i + 1], lstart[j], lstart[j + 1]) for i, j in pairs], dtype=np.int32)
    a, y = rec[rstart[:-1]], lig[lstart[:-1]]
    ca = rs.normal(size=(150, 3)) * 9.0
    return dict(rec=rec, lig=lig, ranges=ranges, pair=(a, y, np.concatenate([a, y @ Rn.T + tn])), ligand_ca=ca,
                target_ca=ca @ Rn.T + tn, Rn=Rn, tn=tn, centre=lig_native.mean(axis=0), residue_pairs=pairs,
                rec_residue=np.repeat(np.arange(nres), np.diff(rstart)), lig_residue=np.repeat(np.arange(nres), np.diff(lstart)))


def poses(tg, K, seed=1):
    rs = np.random.RandomState(seed)
    Q = _rotations(rs.normal(size=(K, 3)) * np.radians(5.0))
    R = Q @ tg["Rn"]
    t = (tg["tn"] - tg["centre"]) @ np.transpose(Q, (0, 2, 1)) + tg["centre"] + rs.normal(size=(K, 3)) * 2.0
    far = np.arange(K) % 3 == 2
    R[far] = _rotations(rs.normal(size=(int(far.sum()), 3)) * 2.0)
    t[far] = tg["tn"] + rs.normal(size=(int(far.sum()), 3)) * 10.0
    R[0], t[0] = tg["Rn"], tg["tn"]
    return np.concatenate([R.reshape(K, 9), t], axis=1)


def host_evaluate(tg, P):
    """The existing host path, pose by pose -> (irmsd, count)"""
    from scipy.spatial import cKDTree
    from deeplocalproteindocking_amd.Results import DockerParser
    dp = DockerParser(".", coords_backend=object())
    dp.target_dict = {"conformations": [(torch.from_numpy(p[:9].reshape(1, 3, 3).copy()), torch.from_numpy(p[9:].reshape(1, 3).copy()), 0.0)
                                        for p in P]}
    a, y, q = (torch.from_numpy(v) for v in tg["pair"])
    tree = cKDTree(tg["rec"])
    native = set(tg["residue_pairs"])
    irmsd, count = [], []
    for k, p in enumerate(P):
        irmsd.append(dp.interface_rmsd([(a, y)], [q], k))
        posed = tg["lig"] @ p[:9].reshape(3, 3).T + p[9:]
        found = set()
        for j, hits in enumerate(tree.query_ball_point(posed, CUTOFF)):
            for i in hits:
                found.add((int(tg["rec_residue"][i]), int(tg["lig_residue"][j])))
        count.append(len(found & native))
    return np.array(irmsd), np.array(count)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-poses", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_evaluate.py needs a GPU"
    entry.build()
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd._lib import get_lib
    from deeplocalproteindocking_amd.engine import _ptr, _stream
    from deeplocalproteindocking_amd.Results.InterfaceSelection import native_reference_from_points
    lib, dev = get_lib(), torch.device("cuda:0")
    tg = target()
    native = native_reference_from_points([tg["pair"]], tg["ligand_ca"], tg["target_ca"], tg["rec"], tg["lig"], tg["ranges"], CUTOFF).to(dev)
    for K in args.sizes:
        Ph = poses(tg, K)
        P = torch.from_numpy(Ph).to(dev)
        ir, lr, fn = (torch.empty(K, dtype=torch.float64, device=dev) for _ in range(3))
        cnt, cl = (torch.empty(K, dtype=torch.int32, device=dev) for _ in range(2))
        st, nI = _stream(dev), native.counts.shape[0] - 1
        NRa, NLa, C = native.rec_atoms.shape[0], native.lig_atoms.shape[0], native.C

        def rmsd():
            lib.call("dlpd_pose_native_rmsd", _ptr(P), K, _ptr(native.moments), native.counts.ctypes.data, nI, _ptr(ir), _ptr(lr), st)

        def contacts():
            lib.call("dlpd_pose_native_contacts", _ptr(P), K, _ptr(native.rec_atoms), NRa, _ptr(native.lig_atoms), NLa, _ptr(native.ranges),
                     native.ranges_host.ctypes.data, C, CUTOFF, _ptr(cnt), st)

        def capri():
            lib.call("dlpd_pose_capri", _ptr(cnt), _ptr(ir), _ptr(lr), C, K, _ptr(fn), _ptr(cl), st)
        row = {"part": "pose evaluation, K = %d (device %s)" % (K, torch.cuda.get_device_name(0)), "K": K, "contacts": C,
               "rec_atoms": NRa, "lig_atoms": NLa, "library": os.path.basename(lib.path)}
        row["hip_rmsd_ms"], row["hip_contacts_ms"], row["hip_capri_ms"] = (_events(f, args.repeats) for f in (rmsd, contacts, capri))
        wall = []
        for _ in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ops.pose_evaluate(P, native)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        row["hip_evaluate_ms"] = float(np.median(wall[1:]))
        n = min(args.host_poses, K)
        t0 = time.perf_counter()
        h_ir, h_cnt = host_evaluate(tg, Ph[:n])
        row["host_poses"], row["host_measured_ms"] = n, (time.perf_counter() - t0) * 1e3
        row["host_ms"] = row["host_measured_ms"] * K / n                    # SCALED from the subset
        row["host_over_hip"] = row["host_ms"] / row["hip_evaluate_ms"]
        d_ir, d_cnt = got[0][:n].cpu().numpy(), (got[2][:n].cpu().numpy() * (C + 0.001)).round().astype(np.int64)
        row["irmsd_max_abs_diff"] = float(np.abs(d_ir - h_ir).max())
        row["counts_differing"] = int((d_cnt != h_cnt).sum())
        row["classes"] = np.bincount(got[3].cpu().numpy(), minlength=4).tolist()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
