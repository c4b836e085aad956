"""The atom projection (csrc/dlpd_atoms.hip) on the CPU-emulated kernel library: dense and cell-wise against float64 by the
yardstick with the fixed-point term, at windows that cross the box, boxes that are no multiple of 4 and non-default splats;
the exact bin-boundary positions; the type sum bit for bit; batches of different proteins; the refusals.  Check bodies and
bounds: tests/atoms_checks.py."""
import pytest

import atoms_checks as ac


@pytest.mark.parametrize("cells", [False, True], ids=["dense", "cells"])
@pytest.mark.parametrize("index", range(len(ac.CASES)), ids=ac.CASE_IDS)
def test_projection_follows_float64(emu, index, cells):
    ac.check_yardstick(emu, "cpu", index, cells)


@pytest.mark.parametrize("edge", ac.EDGE_CASES, ids=lambda e: "L%d-w%d-res%g-voff%g" % e[:4])
def test_projection_at_exact_bin_boundaries(emu, edge):
    ac.check_exact_edges(emu, "cpu", *edge)


@pytest.mark.parametrize("index", [0, 1], ids=ac.CASE_IDS[:2])
def test_type_sum_equals_the_integer_sum_of_the_types(emu, index):
    ac.check_type_sum(emu, "cpu", index)


def test_batch_of_distinct_proteins(emu):
    ac.check_distinct_proteins(emu, "cpu")


def test_repeated_rotation_gives_identical_rows(emu):
    ac.check_repeated_rotation(emu, "cpu")


def test_project_refuses_mismatched_rows_and_shifts(emu):
    ac.check_project_refusals(emu, "cpu")


def test_c_abi_refuses_bad_arguments_and_leaves_the_output(emu):
    ac.check_abi_refusals(emu, "cpu")
