"""Pose evaluation on the real gfx950 build: the interface and ligand RMSD kernel (csrc/dlpd_evaluate.h) against float64 within
the derived band, degenerate point sets, the contact kernel (under guarded allocations) exactly against the float64 predicate,
the class cascade, 65,536 poses with the truth on 512 of them, errors, ``Docker.evaluate`` and
``Results.evaluate_target_device`` on synthetic PDB files.  Check bodies and the derivation of the bands:
tests/evaluate_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import evaluate_checks as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    import __graft_entry__ as entry
    entry.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from deeplocalproteindocking_amd._lib import get_lib
    return get_lib()


@pytest.mark.parametrize("nr,nl", [(0, 3), (5, 1), (40, 35), (200, 180)])
@pytest.mark.parametrize("nI", [1, 3])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 257])
def test_rmsd_matches_float64(dev, lib, K, nI, nr, nl):
    ec.check_rmsd(lib, dev, K, nI, nr, nl)


@pytest.mark.parametrize("kind", ["collinear", "coplanar", "mirror", "exact", "tiny", "constant"])
def test_rmsd_of_degenerate_sets(dev, lib, kind):
    ec.check_rmsd_degenerate(lib, dev, kind)


@pytest.mark.parametrize("C,K", [(1, 1), (63, 5), (64, 65), (65, 65), (257, 5), (300, 5), (300, 1)])
def test_contacts_are_the_float64_predicate(dev, lib, C, K):
    ec.check_contacts(lib, dev, C, K, guard=True)


def test_contacts_at_the_ligand_limit(dev, lib):
    ec.check_contacts_limit(lib, dev)


def test_capri_table(dev, lib):
    ec.check_capri_table(lib, dev)


def test_evaluate_is_the_cascade_of_its_own_outputs(dev, lib):
    ec.check_evaluate(lib, dev)


def test_planted_ladder(dev, lib):
    ec.check_ladder(lib, dev)


def test_65536_poses(dev, lib):
    ec.check_large(lib, dev)


def test_evaluate_errors(dev, lib):
    ec.check_errors(lib, dev)


def test_docker_evaluate_on_synthetic_files(dev, tmp_path):
    ec.check_docker_evaluate(None, dev, tmp_path)


def test_evaluate_target_device_matches_the_host_loop(dev, tmp_path):
    ec.check_evaluate_target_device(None, dev, tmp_path)
