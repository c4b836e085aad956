"""The interface kernels (csrc/dlpd_interface.h) on the real gfx950 build, under guarded allocations whose fresh buffers hold 0xFF
bytes: the residue bitmaps exactly against integer arithmetic on lattice inputs, the two instances' capacities, agreement with the
all-contacts counts, generic poses between the float64 sets at r -+ band, the sphere filter at its bound, the profile's sum bit for
bit in its documented order, the similarity bitmap against the integer test and the clustering on it, 65,536 poses through all
three kernels, errors, ``Docker.interface`` / ``cluster_interface`` and the two steps of scripts/dock_pair.py.  Check bodies:
tests/interface_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import interface_checks as ic

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
@pytest.mark.parametrize("NRres,NLres", ic.EXACT_SHAPES)
def test_bits_are_integer_arithmetic(dev, lib, NRres, NLres, K):
    ic.check_exact(lib, dev, NRres, NLres, K)


@pytest.mark.parametrize("lig_atoms", [2048, 2049, 8192])
def test_bits_at_the_ligand_capacities(dev, lib, lig_atoms):
    ic.check_exact(lib, dev, 5, 0, 3, lig_atoms=lig_atoms)


def test_unpack_bits(dev, lib):
    ic.check_unpack(lib, dev)


def test_bits_agree_with_the_contact_counts(dev, lib):
    ic.check_counts_agree(lib, dev)


def test_generic_poses_between_the_float64_sets(dev, lib):
    ic.check_generic(lib, dev)


def test_sphere_filter_at_its_edge(dev, lib):
    ic.check_sphere_edge(lib, dev)


@pytest.mark.parametrize("K", [1, 1023, 1024, 1025, 2049])
def test_profile_is_the_ordered_sum(dev, lib, K):
    ic.check_profile(lib, dev, K)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130, 513])
def test_similarity_bitmap_and_clusters(dev, lib, K):
    ic.check_within(lib, dev, K)


def test_65536_poses(dev, lib):
    ic.check_large(lib, dev)


def test_interface_errors(dev, lib):
    ic.check_errors(lib, dev)


def test_docker_interface(dev, tmp_path):
    ic.check_docker_interface(None, dev, tmp_path)


def test_docker_interface_under_a_random_rotation(dev, tmp_path):
    ic.check_random_rotation(None, dev, tmp_path)


def test_dock_pair_interface_flags(dev, tmp_path):
    ic.check_dock_pair(None, dev, tmp_path)
