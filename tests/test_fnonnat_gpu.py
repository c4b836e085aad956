"""The all-contacts kernel (csrc/dlpd_contacts.h) on the real gfx950 build, under guarded allocations: n_dec and n_corr exactly
against integer arithmetic on lattice inputs, the two instances' capacities, the sphere filter at its bound, generic poses
between the float64 counts at r -+ band, n_corr against the existing native-contact kernel, 65,536 poses with the truth on 512
of them, errors; ``Docker.evaluate(fnonnat=True)``, the decoy set of scripts/dock_pair.py --decoys and one training step on a
batch of its stream.  Check bodies: tests/fnonnat_checks.py, tests/decoy_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import fnonnat_checks as fc

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


@pytest.mark.parametrize("K", [1, 24, 65])
@pytest.mark.parametrize("NRres,NLres", [(1, 1), (3, 65), (65, 3), (130, 67)])
def test_counts_are_integer_arithmetic(dev, lib, NRres, NLres, K):
    fc.check_exact(lib, dev, NRres, NLres, K)


@pytest.mark.parametrize("lig_atoms", [2048, 2049, 8192])
def test_counts_at_the_ligand_capacities(dev, lib, lig_atoms):
    fc.check_exact_capacity(lib, dev, lig_atoms)


def test_one_atom_over_the_capacity_is_refused(dev, lib):
    fc.check_over_capacity(lib, dev)


def test_sphere_filter_at_its_edge(dev, lib):
    fc.check_sphere_edge(lib, dev)


def test_generic_poses_between_the_float64_counts(dev, lib):
    fc.check_generic(lib, dev)


def test_n_corr_is_the_native_contact_kernels_count(dev, lib):
    fc.check_agreement(lib, dev)


def test_65536_poses(dev, lib):
    fc.check_large(lib, dev)


def test_contact_errors(dev, lib):
    fc.check_errors(lib, dev)


def test_docker_evaluate_with_fnonnat(dev, tmp_path):
    import decoy_checks as dc
    dc.check_docker_fnonnat(None, dev, tmp_path)


def test_decoy_set_round_trip(dev, tmp_path):
    import decoy_checks as dc
    dc.check_round_trip(None, dev, tmp_path)


def test_dock_pair_decoys_then_one_training_step(dev, tmp_path):
    import decoy_checks as dc
    dc.check_dock_pair_decoys(None, dev, tmp_path, L=32)
