"""Pose evaluation on the CPU-emulated kernel library: the interface and ligand RMSD kernel (csrc/dlpd_evaluate.h) against
numpy's SVD Kabsch and direct differences in float64 within the derived band, degenerate point sets, the contact kernel exactly
against the float64 predicate at cutoffs placed in verified gaps, the class cascade, errors, ``Docker.evaluate`` and
``Results.evaluate_target_device`` on synthetic PDB files and the --native step of scripts/dock_pair.py.  Check bodies and the
derivation of the bands: tests/evaluate_checks.py."""
import pytest

import evaluate_checks as ec


@pytest.mark.parametrize("nr,nl", [(0, 3), (5, 1), (40, 35), (200, 180)])
@pytest.mark.parametrize("nI", [1, 3])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 257])
def test_rmsd_matches_float64(emu, K, nI, nr, nl):
    ec.check_rmsd(emu, "cpu", K, nI, nr, nl)


@pytest.mark.parametrize("kind", ["collinear", "coplanar", "mirror", "exact", "tiny", "constant"])
def test_rmsd_of_degenerate_sets(emu, kind):
    ec.check_rmsd_degenerate(emu, "cpu", kind)


@pytest.mark.parametrize("C,K", [(1, 1), (63, 5), (64, 65), (65, 65), (257, 5), (300, 5)])
def test_contacts_are_the_float64_predicate(emu, C, K):
    ec.check_contacts(emu, "cpu", C, K)


def test_contacts_at_the_ligand_limit(emu):
    ec.check_contacts_limit(emu, "cpu")


def test_capri_table(emu):
    ec.check_capri_table(emu, "cpu")


def test_evaluate_is_the_cascade_of_its_own_outputs(emu):
    ec.check_evaluate(emu, "cpu")


def test_planted_ladder(emu):
    ec.check_ladder(emu, "cpu")


def test_evaluate_errors(emu):
    ec.check_errors(emu, "cpu")


def test_docker_evaluate_on_synthetic_files(emu, tmp_path):
    ec.check_docker_evaluate(emu, "cpu", tmp_path)


def test_evaluate_target_device_matches_the_host_loop(emu, tmp_path):
    ec.check_evaluate_target_device(emu, "cpu", tmp_path)


def test_dock_pair_native_step(emu, tmp_path):
    ec.check_dock_pair(emu, "cpu", tmp_path)
