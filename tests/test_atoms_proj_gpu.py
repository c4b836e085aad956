"""The atom projection (csrc/dlpd_atoms.hip) on the real gfx950 build -- expf, the integer atomics and the capped launches of
the device: dense and cell-wise against float64 by the yardstick with the fixed-point term, at windows that cross the box,
boxes that are no multiple of 4 and non-default splats; the exact bin-boundary positions; the type sum bit for bit; batches
of different proteins; the second trip of k_marked_cells' grid-stride loop; the refusals.  Check bodies and bounds:
tests/atoms_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import atoms_checks as ac

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


@pytest.mark.parametrize("cells", [False, True], ids=["dense", "cells"])
@pytest.mark.parametrize("index", range(len(ac.CASES)), ids=ac.CASE_IDS)
def test_projection_follows_float64(dev, lib, index, cells):
    ac.check_yardstick(lib, dev, index, cells)


@pytest.mark.parametrize("edge", ac.EDGE_CASES, ids=lambda e: "L%d-w%d-res%g-voff%g" % e[:4])
def test_projection_at_exact_bin_boundaries(dev, lib, edge):
    ac.check_exact_edges(lib, dev, *edge)


@pytest.mark.parametrize("index", [0, 1], ids=ac.CASE_IDS[:2])
def test_type_sum_equals_the_integer_sum_of_the_types(dev, lib, index):
    ac.check_type_sum(lib, dev, index)


def test_batch_of_distinct_proteins(dev, lib):
    ac.check_distinct_proteins(lib, dev)


def test_repeated_rotation_gives_identical_rows(dev, lib):
    ac.check_repeated_rotation(lib, dev)


def test_second_trip_of_the_capped_cell_loop(dev, lib):
    ac.check_second_trip(lib, dev)


def test_project_refuses_mismatched_rows_and_shifts(dev, lib):
    ac.check_project_refusals(lib, dev)


def test_c_abi_refuses_bad_arguments_and_leaves_the_output(dev, lib):
    ac.check_abi_refusals(lib, dev)
