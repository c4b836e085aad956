"""Search with an exclusion radius on the CPU-emulated kernel library: the local-minimum kernel and the candidate-list kernel
(csrc/dlpd_suppress.h) against the definition written out in numpy, their error codes, the engine driven by hand on both
selection paths, the unfused loop, ``Docker.update_top``, a live engine across radii, two ranks and the search step of
scripts/dock_pair.py.  Check bodies and the oracle: tests/exclusion_checks.py.  Every comparison is bit for bit."""
import pytest

import exclusion_checks as xc


@pytest.mark.parametrize("n", xc.SIZES)
def test_suppressed_volume_is_the_definition(emu, n):
    # (the emulator runs a 33^3 grid's 50 blocks thread by thread, every wave shuffle a round of context switches: the two
    #  largest sizes take one radius each there, the largest and the smallest; the device tests take all four at both)
    xc.check_suppress_volumes(emu, "cpu", n, rs={31: (4,), 33: (1,)}.get(n))


@pytest.mark.parametrize("n", [3, 7, 9, 12, 33])
def test_equal_negatives_keep_the_lowest_flat_index(emu, n):
    xc.check_planted(emu, "cpu", n, rs=(2,) if n > 30 else None)


@pytest.mark.parametrize("n", [3, 9, 12, 33])
def test_volume_without_a_negative_keeps_its_bits(emu, n):
    xc.check_nonnegative_is_returned_as_is(emu, "cpu", n)


def test_zero_fill_with_fewer_negatives_than_K(emu):
    xc.check_zero_fill(emu, "cpu")


def test_rows_of_complete_candidate_lists_are_not_written(emu):
    xc.check_rows_of_complete_lists_are_not_written(emu, "cpu")


def test_candidate_lists_keep_the_survivors_in_order(emu):
    xc.check_suppress_cand(emu, "cpu")


def test_exclusion_errors(emu):
    xc.check_errors(emu, "cpu")


# (an emulated box-32 rotation costs about two seconds: the emulator takes two of the device's cases per path)
@pytest.mark.parametrize("K,r,C", [(16, 1, 2), (64, 2, 3)])
def test_engine_list_with_complete_candidate_lists(emu, K, r, C):
    xc.check_engine(emu, "cpu", K, r, C=C)


@pytest.mark.parametrize("K,r", [(16, 2), (64, 1)])
def test_engine_list_with_overflowing_candidate_lists(emu, K, r):
    xc.check_engine(emu, "cpu", K, r, C=2, cap=64)


def test_engine_list_without_prefilter_and_at_other_launch_batches(emu):
    xc.check_engine_variants(emu, "cpu")


def test_engine_list_on_an_embedded_box(emu):
    xc.check_engine_embedded(emu, "cpu")


def test_user_defined_model_reaches_the_unfused_loop(emu):
    xc.check_docker_unfused(emu, "cpu")


def test_update_top_on_a_small_volume(emu):
    xc.check_update_top(emu, "cpu")


def test_live_engine_across_radii_and_the_default(emu):
    xc.check_reuse_and_defaults(emu, "cpu")


def test_two_ranks_give_the_one_rank_list(emu):
    xc.check_two_ranks(emu, "cpu")


def test_dock_pair_exclusion_step(emu, tmp_path):
    xc.check_dock_pair(emu, "cpu", tmp_path)
