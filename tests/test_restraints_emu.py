"""Search under distance restraints on the CPU-emulated kernel library: the volume kernel and the candidate-list kernel
(csrc/dlpd_restrain.h) against ``Utils.Restraints.allowed``, planted geometry, their error codes, the host-side table and
selections, the engine driven by hand on every selection path, the unfused loop, ``Docker.update_top``, a live engine across
restraint sets, two ranks and the search step of scripts/dock_pair.py.  Check bodies and the oracle: tests/restraints_checks.py.
Every comparison is bit for bit."""
import itertools

import pytest

import restraints_checks as rc


@pytest.mark.parametrize("n", rc.SIZES)
def test_restrained_volume_is_the_definition(emu, n):
    # (the emulator runs a 64^3 grid's 128 blocks per rotation thread by thread: the two largest sizes take a cut of the
    #  combinations there -- both kinds, both batch sizes, every J, need 1, J and in between; the device tests take all)
    combos = None
    if n >= 34:
        combos = [(3, (5, 3), "normal"), (1, (32, 7), "integers"), (1, (32, 32), "normal"), (1, (1, 1), "integers"), (3, (5, 1), "integers")]
    rc.check_restrain_volumes(emu, "cpu", n, combos)


@pytest.mark.parametrize("n", [12, 34])
def test_planted_geometry(emu, n):
    rc.check_planted(emu, "cpu", n)


@pytest.mark.parametrize("n", [6, 12, 34])
def test_volume_without_a_negative_keeps_its_bits(emu, n):
    rc.check_nonnegative_is_returned_as_is(emu, "cpu", n)


def test_candidate_lists_are_thinned_and_rebuilt(emu):
    rc.check_restrain_cand(emu, "cpu")


def test_zero_fill_with_fewer_allowed_negatives_than_K(emu):
    rc.check_zero_fill(emu, "cpu")


def test_restraint_errors(emu):
    rc.check_errors(emu, "cpu")


def test_restraint_table_by_hand():
    rc.check_table_by_hand()


def test_select_point_and_its_errors(tmp_path):
    rc.check_select_point(tmp_path)


def test_engine_list_on_every_selection_path(emu):
    rc.check_engine_paths(emu, "cpu")


def test_engine_search_at_other_launch_batches_and_without_rebuild(emu):
    rc.check_engine_search(emu, "cpu")


def test_engine_list_on_an_embedded_box(emu):
    rc.check_engine_embedded(emu, "cpu")


def test_user_defined_model_reaches_the_unfused_loop(emu):
    rc.check_docker_unfused(emu, "cpu")


def test_update_top_and_the_report(emu):
    rc.check_update_top(emu, "cpu")


def test_live_engine_across_restraint_sets_and_the_default(emu):
    rc.check_reuse_and_defaults(emu, "cpu")


def test_two_ranks_give_the_one_rank_list(emu):
    rc.check_two_ranks(emu, "cpu")


def test_dock_pair_restraint_step(emu, tmp_path):
    rc.check_dock_pair(emu, "cpu", tmp_path)
