"""The training-data path without a GPU: the stream (Dataset.SplitComplexDataset) against the reference's parsed tables and
sampler batches recorded in tests/golden/g9_training_data.json (made by tests/golden/make_golden_stream.py), its seeded
shuffle, ``Docker.evaluate(fnonnat=True)``, the round trip of Dataset.DecoySet on a synthetic pair, two epochs of
``local_train.main`` and the --decoys step of scripts/dock_pair.py on the emulated kernels.  Check bodies of the last four:
tests/decoy_checks.py.  Nothing here reads the reference tree."""
import os

import pytest
import torch

import decoy_checks as dc
import fnonnat_checks as fc


@pytest.fixture()
def tiny(tmp_path):
    """the fixture's dataset written out -> (root, fixture)"""
    fx = fc.fixture()
    root = tmp_path / "tiny"
    (root / "Description").mkdir(parents=True)
    (root / "Description" / fx["dataset"]["subset_name"]).write_text(fx["dataset"]["subset"])
    for t, text in fx["dataset"]["tables"].items():
        (root / "Description" / (t + ".dat")).write_text(text)
    return str(root), fx


def test_tables_parse_as_the_reference_parses_them(tiny):
    from deeplocalproteindocking_amd.Dataset import SplitComplexDataset
    root, fx = tiny
    ds = SplitComplexDataset("quality", 1, root, description_set=fx["dataset"]["subset_name"], device="cpu")
    assert ds.targets == fx["targets"] and len(ds) == fx["size"] == 3
    for t in ds.targets:
        want = [{k: (os.path.join(root, v) if isinstance(v, str) else v) for k, v in row.items()} for row in fx["parsed"][t]]
        assert ds.decoys[t] == want
        assert all(isinstance(r["quality"], float) and r["receptor"].startswith(root) for r in ds.decoys[t])
    assert ds.indexed == [r for t in ds.targets for r in ds.decoys[t]]
    rec, lig, label = ds[(1, 3)]
    assert rec == os.path.join(root, "Decoys", "2XYZ_r.pdb") and lig == os.path.join(root, "Decoys", "2XYZ_l_3.pdb")
    assert tuple(label.shape) == (1,) and label.dtype == torch.float32 and float(label) == 3.0 and label.device.type == "cpu"
    assert float(SplitComplexDataset("lrmsd", 1, root, description_set=fx["dataset"]["subset_name"], device="cpu", verbose=False)[(2, 0)][2]) == 0.5


@pytest.mark.parametrize("threshold", [1, 2])
@pytest.mark.parametrize("batch_size", [4, 10])
def test_batches_are_the_reference_samplers(tiny, batch_size, threshold):
    from deeplocalproteindocking_amd.Dataset import get_dataset_stream
    root, fx = tiny
    stream = get_dataset_stream(root, fx["dataset"]["subset_name"], batch_size=batch_size, threshold=threshold, device="cpu")
    want = fx["batches"]["%d:%d" % (batch_size, threshold)]
    assert len(stream) == 3 == len(want)
    assert [[list(p) for p in b] for b in stream.batch_sampler] == want
    for (rec, lig, labels), idx in zip(stream, want):                                   # one batch per target, in the sampler's order
        assert len(rec) == len(lig) == len(idx) and tuple(labels.shape) == (len(idx), 1)
        for f, l, (t, d) in zip(lig, labels, idx):
            row = stream.dataset.decoys[fx["targets"][t]][d]
            assert f == row["ligand"] and float(l) == row["quality"]


def test_seeded_shuffle_obeys_the_selection_rule(tiny):
    from deeplocalproteindocking_amd.Dataset import BatchSamplerQuality, SplitComplexDataset
    root, fx = tiny
    ds = SplitComplexDataset("quality", 1, root, description_set=fx["dataset"]["subset_name"], device="cpu", verbose=False)
    before = {t: list(rows) for t, rows in ds.decoys.items()}

    def batches(seed, bs=4):
        return [b for b in BatchSamplerQuality(ds.targets, ds.decoys, "quality", 1, bs, shuffle=True, seed=seed)]
    a, b, c = batches(7), batches(7), batches(8)
    assert a == b and a != c
    assert a != [[tuple(p) for p in bt] for bt in fx["batches"]["4:1"]]
    assert ds.decoys == before                                                           # the tables keep their file order
    for bs in (4, 10):
        for seed in range(5):
            sampler = BatchSamplerQuality(ds.targets, ds.decoys, "quality", 1, bs, shuffle=True, seed=seed)
            for ti, batch in enumerate(sampler):
                rows = ds.decoys[ds.targets[ti]]
                picked = [d for t, d in batch]
                assert all(t == ti for t, _ in batch) and len(set(picked)) == len(picked)
                q = [rows[d]["quality"] >= 1 for d in picked]
                npos, nneg = sum(1 for r in rows if r["quality"] >= 1), sum(1 for r in rows if r["quality"] < 1)
                assert q == sorted(q, reverse=True)                                      # positives first
                assert sum(q) == min(npos, (bs + 1) // 2) and len(picked) == sum(q) + min(nneg, bs - sum(q))
    two = BatchSamplerQuality(ds.targets, ds.decoys, "quality", 1, 4, shuffle=True, seed=1)
    assert list(two) != list(two)                                                       # every pass draws a new order


def test_docker_evaluate_with_fnonnat(emu, tmp_path):
    dc.check_docker_fnonnat(emu, "cpu", tmp_path)


def test_decoy_set_round_trip(emu, tmp_path):
    dc.check_round_trip(emu, "cpu", tmp_path)


def test_two_epochs_of_local_train(emu, tmp_path):
    dc.check_epoch_loop(emu, "cpu", tmp_path)


def test_dock_pair_decoys_step(emu, tmp_path):
    dc.check_dock_pair_decoys(emu, "cpu", tmp_path, L=16)
