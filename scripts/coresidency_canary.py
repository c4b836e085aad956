"""Co-residency canary, run in a FRESH process by tests/test_gpu_parity.py (and by hand): one batch of the reference's real
shapes is scored again and again while two more streams of the process are kept busy -- a representation plugin's bf16 x 3
convolutions and the engine's own full radix select -- and every stage's output is compared with the undisturbed run's bits.
    coresidency_canary.py se3_dense_convolution | e3_tile_occupancy_convolution   ->  one JSON line {"changed": {stage: count}, "scorings": 80}
Why a process of its own: HIP deals a process's streams over a handful of hardware queues; late in a long test session two
new streams often land on the queue the default stream uses and their kernels then run one after the other -- the pair is
never co-resident and the known-bad case passes for the wrong reason (seen in round 6: XFAIL in isolation 3 of 3, passed
inside the full suite)."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch
import __graft_entry__ as entry

entry.build()


def _rots(n, seed):
    from oracle import docking_oracle as orc
    ang = np.random.RandomState(seed).uniform(-np.pi, np.pi, size=(n, 3))
    return orc.euler_to_matrix(ang[:, 0], np.abs(ang[:, 1]), ang[:, 2])


def main(co_runner):
    dev = torch.device("cuda:0")
    import pathlib
    tmp_path = pathlib.Path(tempfile.mkdtemp(prefix="dlpd_canary_"))
    import threading
    import time
    from deeplocalproteindocking_amd.engine import DockingEngine
    from deeplocalproteindocking_amd.Models import E3MultiResRepr4x4, SE3MultiResReprScalar
    known_bad = co_runner == "e3_tile_occupancy_convolution"
    L, C, C1 = 80, 16, 32
    if known_bad:
        # the victim as scripts/stage_race_probe.py builds it (the configuration the 298 / 300 were measured in): the engine of
        # a Docker.dockSE3 on a synthetic protein-sized pair (protein-shaped volumes, clash channel from re-projected atoms)
        from synth_pdb import write_protein_like_pdb
        from deeplocalproteindocking_amd.Docker import Docker
        from deeplocalproteindocking_amd.Models import GlobalDockingModel, SimpleFilter
        from deeplocalproteindocking_amd.Utils.Rotations import Rotations
        pdb = {}
        for name, n, seed in (("r1", 150, 21), ("l1", 90, 22)):
            pdb[name] = str(tmp_path / (name + ".pdb"))
            write_protein_like_pdb(pdb[name], n, seed)
        torch.manual_seed(7)
        repr_ = SE3MultiResReprScalar(multiplier=8)
        model = GlobalDockingModel(repr_, SimpleFilter(repr_.get_num_outputs()), threshold_clash=40.0).to(dev).eval()
        Rall = Rotations(20, allow_generated=True, verbose=False).R.numpy()
        dk = Docker(model, box_size=L, resolution=1.25, max_conf=2000, rotations=Rall[:64], device=dev, randomize_rot=True, rotation_seed=7)
        with torch.no_grad():
            dk.dockSE3(pdb["r1"], pdb["l1"], batch_size=2)
        torch.cuda.synchronize()
        eng = dk.engine
        # the kernels the 298 / 300 were measured with: the dense K1 / K2 (round 6's occupancy-map kernels, which this
        # protein-shaped ligand would take by default, have another footprint and rarely show it within 80 scorings)
        for g in eng.grids:
            g.sparse = g.pencil_map = False
        R = torch.from_numpy(Rall[16:32]).to(device=dev, dtype=torch.float32).contiguous()
    else:
        torch.manual_seed(5)
        g = torch.Generator().manual_seed(5)
        rec, lig = torch.randn(C, L, L, L, generator=g) * 0.1, torch.randn(C, L, L, L, generator=g) * 0.1
        rec1, lig1 = torch.randn(C1, 40, 40, 40, generator=g) * 0.1, torch.randn(C1, 40, 40, 40, generator=g) * 0.1
        recf, ligf = torch.rand(L, L, L, generator=g), torch.rand(L, L, L, generator=g)
        W1, b1 = torch.randn(24, C + C1, generator=g) * 0.3, torch.randn(24, generator=g) * 0.1
        W2, b2 = torch.randn(1, 24, generator=g), torch.randn(1, generator=g)
        eng = DockingEngine(L, C, W1, b1, W2, b2, clip=5.0, threshold_clash=0.12 * L ** 3, max_conf=2000, batch=16, device=dev, coarse_channels=C1)
        eng.set_receptor(rec, recf, rec1)
        eng.set_ligand(lig, ligf, lig1)
        R = torch.from_numpy(_rots(16, seed=8)).float().to(dev).contiguous()
    buffers = {"coarse_k1": lambda: eng.coarse.wsA, "coarse_k2": lambda: eng.coarse.wsB, "coarse": lambda: eng.pre,
               "k1_rotate_zfft": lambda: eng.fine.wsA, "k2_xy_corr": lambda: eng.fine.wsB, "k3_zifft_filter": lambda: eng.V}
    ref = {}

    def record(name):
        if name in buffers:
            ref[name] = buffers[name]().clone()
    record.sub_stages = True
    eng.score_batch(R, mark=record)
    torch.cuda.synchronize()
    assert set(ref) == set(buffers)
    if known_bad:
        plugin = E3MultiResRepr4x4(multiplier=8).to(dev).eval()
        x11 = torch.zeros(4, 11, L, L, L, device=dev)             # zero away from a blob, as a protein's density is
        x11[:, :, 24:52, 20:48, 28:60] = torch.rand(4, 11, 28, 28, 32, device=dev)
    else:
        plugin = SE3MultiResReprScalar(multiplier=8).to(dev).eval()
        x11 = torch.rand(1, 11, L, L, L, device=dev)
    Vsel = eng.V.clone()
    stop = threading.Event()
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]

    def convolve():
        torch.cuda.set_device(dev)
        with torch.cuda.stream(streams[0]), torch.no_grad():
            while not stop.is_set():
                plugin(x11)
                streams[0].synchronize()

    def select():
        torch.cuda.set_device(dev)
        with torch.cuda.stream(streams[1]):
            while not stop.is_set():
                for _ in range(4):
                    eng.top.select(Vsel.reshape(16, -1), 16, None)
                streams[1].synchronize()
    threads = [threading.Thread(target=convolve, daemon=True), threading.Thread(target=select, daemon=True)]
    for t in threads:
        t.start()
    time.sleep(0.1)
    changed = {}
    try:
        for it in range(80):
            def check(name):
                if name in buffers and not torch.equal(buffers[name](), ref[name]):
                    changed.setdefault(name, []).append(it)
            check.sub_stages = True
            eng.score_batch(R, mark=check)
            torch.cuda.synchronize()
    finally:
        stop.set()
        for t in threads:
            t.join()
    print(json.dumps({"co_runner": co_runner, "scorings": 80, "changed": {k: len(v) for k, v in changed.items()}}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "e3_tile_occupancy_convolution")
