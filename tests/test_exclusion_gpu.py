"""Search with an exclusion radius on the real gfx950 build: the local-minimum kernel (under guarded allocations, into NaN-filled
outputs, at the sizes of the real grids) and the candidate-list kernel (csrc/dlpd_suppress.h) against the definition written
out in numpy, their error codes, the engine driven by hand on both selection paths, the unfused loop, ``Docker.update_top``, a
live engine across radii, two ranks and the search step of scripts/dock_pair.py.  Check bodies and the oracle:
tests/exclusion_checks.py.  Every comparison is bit for bit.  Nothing here reads the reference tree."""
import pytest
import torch

import exclusion_checks as xc

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


@pytest.mark.parametrize("n", xc.SIZES)
def test_suppressed_volume_is_the_definition(dev, lib, n):
    xc.check_suppress_volumes(lib, dev, n)


@pytest.mark.parametrize("n", [3, 7, 9, 12, 33])
def test_equal_negatives_keep_the_lowest_flat_index(dev, lib, n):
    xc.check_planted(lib, dev, n)


@pytest.mark.parametrize("n", [3, 9, 12, 33])
def test_volume_without_a_negative_keeps_its_bits(dev, lib, n):
    xc.check_nonnegative_is_returned_as_is(lib, dev, n)


@pytest.mark.parametrize("n,r", [(128, 1), (160, 2), (40, 4)])
def test_suppressed_volume_under_guarded_allocations(dev, lib, n, r):
    xc.check_suppress_on_the_device(lib, dev, n, r)


def test_zero_fill_with_fewer_negatives_than_K(dev, lib):
    xc.check_zero_fill(lib, dev)


def test_rows_of_complete_candidate_lists_are_not_written(dev, lib):
    xc.check_rows_of_complete_lists_are_not_written(lib, dev)


def test_candidate_lists_keep_the_survivors_in_order(dev, lib):
    xc.check_suppress_cand(lib, dev)


def test_exclusion_errors(dev, lib):
    xc.check_errors(lib, dev)


# (radii 3 and 4 are the kernel tests' above: at 64^3 the oracle's 342 / 728 offsets per rotation would make these cases slow)
@pytest.mark.parametrize("K,r,C", [(16, 1, 2), (64, 2, 3), (16, 2, 4)])
def test_engine_list_with_complete_candidate_lists(dev, lib, K, r, C):
    xc.check_engine(lib, dev, K, r, C=C)


@pytest.mark.parametrize("K,r", [(16, 2), (64, 1)])
def test_engine_list_with_overflowing_candidate_lists(dev, lib, K, r):
    xc.check_engine(lib, dev, K, r, cap=64)


def test_engine_list_without_prefilter_and_at_other_launch_batches(dev, lib):
    xc.check_engine_variants(lib, dev)


def test_engine_list_on_an_embedded_box(dev, lib):
    xc.check_engine_embedded(lib, dev)


def test_user_defined_model_reaches_the_unfused_loop(dev):
    xc.check_docker_unfused(None, dev)


def test_update_top_on_a_small_volume(dev, lib):
    xc.check_update_top(lib, dev)


def test_live_engine_across_radii_and_the_default(dev):
    xc.check_reuse_and_defaults(None, dev)


def test_two_ranks_give_the_one_rank_list(dev):
    xc.check_two_ranks(None, dev)


def test_dock_pair_exclusion_step(dev, tmp_path):
    xc.check_dock_pair(None, dev, tmp_path)
