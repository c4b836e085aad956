"""The receptor in consumption order at boxes 64 / 32 (csrc/dlpd_k2.hip; dlpd_receptor_order, dlpd_xy_correlate_ordered) on
the emulated kernels.  The ordered call is compared bit for bit with the natural call where an emulated launch is short (nine
rotations at box 64 take 15 - 20 s each)."""
import pytest

import k2_operands_checks as op


@pytest.mark.parametrize("L", [32, 64])
def test_ordered_copy_is_the_permutation_the_header_names(emu, L):
    op.check_ordered_copy(emu, "cpu", L)


def test_size_queries_and_refusals(emu):
    op.check_size_queries(emu)


@pytest.mark.parametrize("nb", [1, 2, 3, 9])
@pytest.mark.parametrize("L", [32, 64])
def test_shared_receptor_ordered(emu, L, nb):
    """nb = 1, 2: one part, without and with a second rotation; 3: the last rotation on the flipped order; 9: two parts of
    4 and 5 rotations, both parities start and end a part."""
    op.check_ordered_against_float64(emu, "cpu", L, nb, natural_bits=not (L == 64 and nb == 9))


@pytest.mark.parametrize("L", [32, 64])
def test_receptor_per_rotation_stays_on_the_natural_layout(emu, L):
    op.check_receptor_per_rotation(emu, "cpu", L, 3)


def test_engine_lists_with_and_without_the_ordered_receptor(emu):
    """The short form of the search of test_k2_operands_gpu.py (40 rotations there): 6 rotations in batches of 3."""
    op.check_engine_lists(emu, "cpu", nrot=6, batch=3)
