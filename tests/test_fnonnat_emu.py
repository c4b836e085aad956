"""The all-contacts kernel (csrc/dlpd_contacts.h) on the CPU-emulated kernel library: n_dec and n_corr exactly against integer
arithmetic on lattice inputs (shapes on both sides of every index boundary and of the two instances' capacities), the sphere
filter at its bound, generic poses between the float64 counts at r -+ band, n_corr against the existing native-contact kernel,
the fnonnat formula against the fixture, errors (65,536 poses: the device suite; the emulator takes minutes for them).  Check bodies: tests/fnonnat_checks.py."""
import pytest

import fnonnat_checks as fc


@pytest.mark.parametrize("K", [1, 24, 65])
@pytest.mark.parametrize("NRres,NLres", [(1, 1), (3, 65), (65, 3), (130, 67)])
def test_counts_are_integer_arithmetic(emu, NRres, NLres, K):
    fc.check_exact(emu, "cpu", NRres, NLres, K)


@pytest.mark.parametrize("lig_atoms", [2048, 2049, 8192])
def test_counts_at_the_ligand_capacities(emu, lig_atoms):
    fc.check_exact_capacity(emu, "cpu", lig_atoms)


def test_one_atom_over_the_capacity_is_refused(emu):
    fc.check_over_capacity(emu, "cpu")


def test_sphere_filter_at_its_edge(emu):
    fc.check_sphere_edge(emu, "cpu")


def test_generic_poses_between_the_float64_counts(emu):
    fc.check_generic(emu, "cpu")


def test_n_corr_is_the_native_contact_kernels_count(emu):
    fc.check_agreement(emu, "cpu")


def test_fnonnat_formula_matches_the_fixture():
    fc.check_formula()


def test_contact_errors(emu):
    fc.check_errors(emu, "cpu")
