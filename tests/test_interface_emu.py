"""The interface kernels (csrc/dlpd_interface.h) on the CPU-emulated kernel library: the residue bitmaps exactly against integer
arithmetic on lattice inputs (shapes on both sides of the 32-bit word, the 64-lane stride, 128 residues and the two instances'
capacities), agreement with the all-contacts counts, generic poses between the float64 sets at r -+ band, the sphere filter at
its bound, the profile's sum bit for bit in its documented order, the similarity bitmap against the integer test and the
clustering on it, errors, and the Docker level (65,536 poses: the device suite).  Check bodies: tests/interface_checks.py."""
import pytest

import interface_checks as ic


@pytest.mark.parametrize("K", [1, 24, 65])
@pytest.mark.parametrize("NRres,NLres", ic.EXACT_SHAPES)
def test_bits_are_integer_arithmetic(emu, NRres, NLres, K):
    ic.check_exact(emu, "cpu", NRres, NLres, K)


@pytest.mark.parametrize("lig_atoms", [2048, 2049, 8192])
def test_bits_at_the_ligand_capacities(emu, lig_atoms):
    ic.check_exact(emu, "cpu", 5, 0, 3, lig_atoms=lig_atoms)


def test_unpack_bits(emu):
    ic.check_unpack(emu, "cpu")


def test_bits_agree_with_the_contact_counts(emu):
    ic.check_counts_agree(emu, "cpu")


def test_generic_poses_between_the_float64_sets(emu):
    ic.check_generic(emu, "cpu")


def test_sphere_filter_at_its_edge(emu):
    ic.check_sphere_edge(emu, "cpu")


@pytest.mark.parametrize("K", [1, 1023, 1024, 1025, 2049])
def test_profile_is_the_ordered_sum(emu, K):
    ic.check_profile(emu, "cpu", K)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130, 513])
def test_similarity_bitmap_and_clusters(emu, K):
    ic.check_within(emu, "cpu", K)


def test_interface_errors(emu):
    ic.check_errors(emu, "cpu")


def test_docker_interface(emu, tmp_path):
    ic.check_docker_interface(emu, "cpu", tmp_path)


def test_docker_interface_under_a_random_rotation(emu, tmp_path):
    ic.check_random_rotation(emu, "cpu", tmp_path)


def test_dock_pair_interface_flags(emu, tmp_path):
    ic.check_dock_pair(emu, "cpu", tmp_path)
