"""Check bodies of the training-set path: ``Docker.evaluate(fnonnat=True)``, Dataset.DecoySet (``native_pose``,
``near_native_poses``, ``write_decoy_set``), the stream reading what was written, ``local_train.main`` and the --decoys step of
scripts/dock_pair.py -- shared by tests/test_dataset_stream.py (emulated kernels, no GPU) and tests/test_fnonnat_gpu.py."""
import os
import sys

import numpy as np
import torch

import evaluate_checks as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def files(tmp_path, tag, nrec=14, nlig=11, seed=5):
    """a synthetic pair in contact, small enough for a 32 A box"""
    from synth_pdb import write_protein_like_pdb
    frec, flig = str(tmp_path / ("%s_r.pdb" % tag)), str(tmp_path / ("%s_l.pdb" % tag))
    write_protein_like_pdb(frec, nrec, seed=seed, extras=False)
    write_protein_like_pdb(flig, nlig, seed=seed + 1, offset=(7.0, 3.0, -2.0), extras=False)
    return frec, flig


def native_of(frec, flig, device, all_contacts=True):
    from deeplocalproteindocking_amd.Results import InterfaceSelection as isel
    return isel.native_reference(frec, flig, frec, flig, all_contacts=all_contacts).to(device)      # unbound = bound


def write_target(lib, device, tmp_path, dataset_dir, target, n, seed, subset="training_set.dat", randomize=True):
    """``n`` poses round the native one of a synthetic pair, evaluated and written -> (docker, native, poses, evaluation, files)"""
    from deeplocalproteindocking_amd.Dataset import near_native_poses, pose_entries, write_decoy_set
    frec, flig = files(tmp_path, target, seed=seed)
    native = native_of(frec, flig, device)
    dk = ec._docker(lib, device, randomize)
    P = near_native_poses(native, n, angle=8.0, shift=3.0, seed=seed)
    entries = pose_entries(P, dk)
    assert np.abs(dk.dat_frame_poses(entries) - P).max() <= 1e-12
    ev = dk.evaluate(native, poses=entries, fnonnat=True)
    table = write_decoy_set(dataset_dir, target, frec, flig, P, ev, subset=subset)
    return dk, native, P, ev, (frec, flig, table)


def check_docker_fnonnat(lib, device, tmp_path):
    """the flag adds three keys and a fifth column; without it the dict and the file are what they were"""
    import pytest
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.Dataset import near_native_poses, pose_entries
    frec, flig = files(tmp_path, "T")
    native, plain = native_of(frec, flig, device), native_of(frec, flig, device, all_contacts=False)
    assert plain.all is None and native.all is not None and native.all["n_native"] == len(set(native.contacts))
    dk = ec._docker(lib, device, False)
    entries = pose_entries(near_native_poses(native, 9, angle=8.0, shift=3.0, seed=2), dk)
    entries[1] = (entries[1][0], tuple(v + 40.0 for v in entries[1][1]), 0.0, 1)        # far away
    base = {k: v.copy() for k, v in dk.evaluate(plain, poses=entries).items()}
    assert sorted(base) == ["capri", "fnat", "irmsd", "lrmsd"]
    dk.new_log(str(tmp_path / "four.txt"))
    dk.write_evaluation()
    dk.cleanup()
    ev = dk.evaluate(native, poses=entries, fnonnat=True)
    assert ev is dk.evaluation and sorted(ev) == ["capri", "fnat", "fnonnat", "irmsd", "lrmsd", "n_corr", "n_dec"]
    for k in base:
        assert ev[k].tobytes() == base[k].tobytes(), k
    assert ev["n_dec"].dtype == np.int32 and ev["n_corr"].dtype == np.int32 and ev["fnonnat"].dtype == np.float64
    assert ev["fnonnat"].tobytes() == ((ev["n_dec"] - ev["n_corr"]) / (ev["n_dec"] + 0.001)).tobytes()
    if len(set(native.contacts)) == native.C:                                           # fnat and n_corr count the same set
        assert np.round(ev["fnat"] * (native.C + 0.001)).astype(np.int32).tolist() == ev["n_corr"].tolist()
    assert ev["n_corr"][0] == native.C and ev["n_dec"][0] >= native.C and ev["n_dec"][1] == 0 and ev["fnonnat"][1] == 0.0
    assert (ev["n_corr"] <= ev["n_dec"]).all() and len(set(ev["n_dec"].tolist())) >= 3
    # against the host's own route: every residue pair within the cutoff, by cKDTree on the posed float64 atoms
    from deeplocalproteindocking_amd.Results import InterfaceSelection as isel
    ur, ul = isel.read_structure(frec), isel.read_structure(flig)
    P = dk.dat_frame_poses(entries)
    nat = set(native.contacts)
    for k in (0, 2, 5):
        posed = dict(ul)
        posed["xyz"] = (ul["xyz"] - isel.bbox_centre(ul)) @ P[k, :9].reshape(3, 3).T + P[k, 9:]
        shifted = dict(ur)
        shifted["xyz"] = ur["xyz"] - isel.bbox_centre(ur)
        near = isel.native_contact_pairs(shifted, posed, 5.0 + 1e-3)
        far = isel.native_contact_pairs(shifted, posed, 5.0 - 1e-3)
        assert len(far) <= ev["n_dec"][k] <= len(near) and len(set(far) & nat) <= ev["n_corr"][k] <= len(set(near) & nat)
    dk.new_log(str(tmp_path / "five.txt"))
    dk.write_evaluation()
    dk.cleanup()
    four = [ln.split("\t") for ln in open(str(tmp_path / "four.txt")).read().strip().split("\n")]
    five = [ln.split("\t") for ln in open(str(tmp_path / "five.txt")).read().strip().split("\n")]
    assert len(four) == len(five) == 9 and all(len(r) == 4 for r in four) and all(len(r) == 5 for r in five)
    assert [r[:4] for r in five] == four and [r[4] for r in five] == ["%f" % v for v in ev["fnonnat"]]
    with pytest.raises(RuntimeError, match="all_contacts"):
        dk.evaluate(plain, poses=entries, fnonnat=True)
    empty = dk.evaluate(native, poses=[], fnonnat=True)
    assert empty["fnonnat"].shape == (0,) and empty["n_dec"].dtype == np.int32
    assert len(ops.pose_evaluate(P, native, lib=lib)) == 4                              # pose_evaluate keeps its four-tuple


def check_round_trip(lib, device, tmp_path):
    from deeplocalproteindocking_amd.Dataset import get_dataset_stream, native_pose
    from deeplocalproteindocking_amd.Dataset.DecoySet import HEADER, ROW
    from deeplocalproteindocking_amd.Results import InterfaceSelection as isel
    root = str(tmp_path / "set")
    dk, native, P, ev, (frec, flig, table) = write_target(lib, device, tmp_path, root, "1SYN", 7, seed=5)
    Rn, tn = native_pose(native)
    assert np.abs(P[0] - np.concatenate([Rn.reshape(-1), tn])).max() == 0.0
    assert ev["lrmsd"][0] < 1e-6 and ev["capri"][0] == 3                                # bound = unbound: the native pose is exact
    assert np.abs(Rn - np.eye(3)).max() < 1e-9 and np.abs(tn - (isel.bbox_centre(isel.read_structure(flig)) - isel.bbox_centre(isel.read_structure(frec)))).max() < 1e-9
    # the files
    ur, ul = isel.read_structure(frec), isel.read_structure(flig)
    c_rec, c_lig = isel.bbox_centre(ur), isel.bbox_centre(ul)
    rec_copy = isel.read_structure(os.path.join(root, "Decoys", "1SYN_r.pdb"))
    assert np.array_equal(rec_copy["xyz"], ur["xyz"]) and (rec_copy["resname"] == ur["resname"]).all()
    for k in range(7):
        got = isel.read_structure(os.path.join(root, "Decoys", "1SYN_l_%d.pdb" % k))
        want = (ul["xyz"] - c_lig) @ P[k, :9].reshape(3, 3).T + P[k, 9:] + c_rec
        assert got["xyz"].shape == want.shape and np.abs(got["xyz"] - want).max() <= 0.0005
        assert (got["atomname"] == ul["atomname"]).all() and (got["resnum"] == ul["resnum"]).all() and (got["chain"] == ul["chain"]).all()
    assert np.abs(isel.read_structure(os.path.join(root, "Decoys", "1SYN_l_0.pdb"))["xyz"] - ul["xyz"]).max() <= 0.0005
    # the table
    lines = open(table).read().split("\n")
    assert lines[0] + "\n" == HEADER and lines[-1] == "" and len(lines) == 1 + 7 + 1
    for k in range(7):
        want = ROW % (os.path.join(root, "Decoys", "1SYN_r.pdb"), os.path.join(root, "Decoys", "1SYN_l_%d.pdb" % k), ev["lrmsd"][k],
                      ev["irmsd"][k], ev["fnat"][k], ev["fnonnat"][k], ev["capri"][k])
        assert lines[1 + k] + "\n" == want
    assert open(os.path.join(root, "Description", "training_set.dat")).read() == "1SYN\n"
    # the stream on a MOVED copy of the set: the rows written, the paths re-rooted
    import shutil
    moved = str(tmp_path / "moved")
    shutil.copytree(root, moved)
    shutil.rmtree(root)
    stream = get_dataset_stream(moved, "training_set.dat", batch_size=10, device="cpu")
    assert len(stream) == 1
    ds = stream.dataset
    rows = ds.decoys["1SYN"]
    assert len(rows) == 7 and all(os.path.exists(r["receptor"]) and os.path.exists(r["ligand"]) for r in rows)
    for k, r in enumerate(rows):
        assert r["ligand"] == os.path.join(moved, "Decoys", "1SYN_l_%d.pdb" % k) and r["quality"] == float(ev["capri"][k])
        for key in ("lrmsd", "irmsd", "fnat", "fnonnat"):
            assert r[key] == float("%f" % ev[key][k]), (k, key)
    batches = list(stream)
    assert len(batches) == 1
    rec, lig, labels = batches[0]
    picked = [int(os.path.basename(f)[len("1SYN_l_"):-4]) for f in lig]
    pos = [k for k in range(7) if ev["capri"][k] >= 1][:5]
    want = pos + [k for k in range(7) if ev["capri"][k] < 1][:10 - len(pos)]
    assert picked == want and 0 in pos and labels.reshape(-1).tolist() == [float(ev["capri"][k]) for k in picked]
    assert tuple(labels.shape) == (len(want), 1) and labels.dtype == torch.float32 and len(rec) == len(want)
    assert all(f == os.path.join(moved, "Decoys", "1SYN_r.pdb") for f in rec)


def _stub_model(lib, device):
    import local_grad_checks as lg
    from deeplocalproteindocking_amd.Models import LocalDockingModel, SimpleFilter
    torch.manual_seed(11)
    stub = lg.TwoResolutionStub()
    model = LocalDockingModel(representation=stub, filter=SimpleFilter(stub.get_num_outputs()), lib=lib).to(device)
    with torch.no_grad():
        model.filter.fc[0].bias.fill_(0.5)
        model.filter.fc[0].weight.abs_()
    return model


def _local_train():
    pkg = os.path.join(ROOT, "deeplocalproteindocking_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import local_train
    return local_train


def check_epoch_loop(lib, device, tmp_path):
    """two epochs of local_train.main on a two-target set (box 16, resolution 2.0): four logs, the checkpoints, finite losses;
    a set with a one-decoy target reports the skipped batch"""
    local_train = _local_train()
    data = tmp_path / "data"
    root = str(data / "Syn")
    write_target(lib, device, tmp_path, root, "1SYN", 5, seed=5, subset="train.dat")
    write_target(lib, device, tmp_path, root, "2SYN", 4, seed=9, subset="train.dat")
    write_target(lib, device, tmp_path, root, "2SYN", 4, seed=9, subset="valid.dat")
    write_target(lib, device, tmp_path, root, "3ONE", 1, seed=13, subset="valid.dat")
    assert open(os.path.join(root, "Description", "train.dat")).read() == "1SYN\n2SYN\n"
    common = ["-experiment", "E", "-group", "SE3", "-model", "stub", "-lr", "0.01", "-max_epoch", "2", "-data_dir", str(data), "-log_dir",
              str(tmp_path / "logs"), "-models_dir", str(tmp_path / "models"), "-box_size", "16", "-resolution", "2.0", "-batch_size", "4", "-seed", "3"]
    model = _stub_model(lib, device)
    before = [p.detach().clone() for p in model.parameters()]
    out = local_train.main(common + ["-dataset", "Syn:train.dat:train.dat"], docking_model=model, lib=lib)
    assert out["skipped"] == 0 and len(out["train"]) == 2 == len(out["valid"]) and np.isfinite(out["train"] + out["valid"]).all()
    assert any(not torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))
    for epoch in (0, 1):
        for kind in ("training", "validation"):
            text = open(str(tmp_path / "logs" / "E" / ("%s_epoch%d.dat" % (kind, epoch)))).read().split("\n")
            heads = [ln for ln in text if ln.startswith("Loss\t")]
            assert len(heads) == 2 and text[-1] == "" and 2 + 2 + 2 <= len(text) - 1 <= 2 + 4 + 4      # two batches of two to four decoys
            assert all(np.isfinite(float(v)) for ln in heads for v in ln.split("\t")[1:])
        for part in ("repr", "filter"):
            assert os.path.exists(str(tmp_path / "models" / "E" / ("DPD_Model_%s_epoch%d.th" % (part, epoch))))
    out = local_train.main(common + ["-dataset", "Syn:train.dat:valid.dat", "-experiment", "F", "-max_epoch", "1"], docking_model=model, lib=lib)
    assert out["skipped"] == 1 and np.isfinite(out["valid"]).all() and np.isfinite(out["train"]).all()
    assert len([ln for ln in open(str(tmp_path / "logs" / "F" / "validation_epoch0.dat")) if ln.startswith("Loss\t")]) == 1


def check_dock_pair_decoys(lib, device, tmp_path, L=32):
    """the --decoys step of scripts/dock_pair.py on a searched list, then one ``optimize`` step on a batch of the stream"""
    import cluster_checks as cc
    from deeplocalproteindocking_amd.Dataset import get_dataset_stream
    from deeplocalproteindocking_amd.Models import BatchRankingLoss
    from deeplocalproteindocking_amd.Training import LocalTrainer
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import dock_pair
    assert dock_pair.parse_decoys("d") == ("d", 10, 10) and dock_pair.parse_decoys("d:3") == ("d", 3, 10) and dock_pair.parse_decoys("d:3:0") == ("d", 3, 0)
    frec, flig = files(tmp_path, "P")
    native = native_of(frec, flig, device)
    dk = cc._searched(lib, device, L, K=40)
    top = list(dk.top_list)
    root = str(tmp_path / "set")
    table = dock_pair.decoys_and_write(dk, native, root, str(tmp_path / "1PAIR.dat"), frec, flig, near=4, far=4, seed=1)
    assert table == os.path.join(root, "Description", "1PAIR.dat") and dk.top_list == top
    ev = dk.evaluation
    assert len(ev["capri"]) == 8 and ev["capri"][0] == 3 and "fnonnat" in ev
    far = dk.evaluate(native, poses=top[:4], fnonnat=True)
    for k in ("irmsd", "fnonnat", "n_dec"):
        assert far[k].tobytes() == ev[k][4:].tobytes(), k                               # FAR: the first poses of the searched list
    stream = get_dataset_stream(root, "training_set.dat", batch_size=6, device=device)
    rec, lig, labels = next(iter(stream))
    assert 2 <= len(rec) <= 6 and labels.device.type == torch.device(device).type and float(labels[0]) == 3.0     # the native pose first
    model = _stub_model(lib, device)
    trainer = LocalTrainer(model, BatchRankingLoss(), lr=0.01, box_size=L, resolution=2.0, randomize_rot=True, rotation_seed=3, lib=lib)
    before = [p.detach().clone() for p in (model.filter.fc[0].weight, model.filter.fc[2].weight)]
    loss = trainer.optimize((rec, lig, labels))
    assert np.isfinite(loss) and loss > 0
    assert not torch.equal(model.filter.fc[0].weight.detach(), before[0]) and not torch.equal(model.filter.fc[2].weight.detach(), before[1])
