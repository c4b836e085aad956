"""Search under distance restraints on the real gfx950 build: the volume kernel (under guarded allocations, into NaN-filled
outputs, at the sizes of the real grids) and the candidate-list kernel (csrc/dlpd_restrain.h) against
``Utils.Restraints.allowed``, planted geometry, their error codes, the engine driven by hand on every selection path, the unfused
loop, ``Docker.update_top``, a live engine across restraint sets, two ranks and the search step of scripts/dock_pair.py.  Check
bodies and the oracle: tests/restraints_checks.py.  Every comparison is bit for bit.  Nothing here reads the reference tree."""
import pytest
import torch

import restraints_checks as rc

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


@pytest.mark.parametrize("n", rc.SIZES)
def test_restrained_volume_is_the_definition(dev, lib, n):
    rc.check_restrain_volumes(lib, dev, n)


@pytest.mark.parametrize("n", [12, 34])
def test_planted_geometry(dev, lib, n):
    rc.check_planted(lib, dev, n)


@pytest.mark.parametrize("n", [6, 12, 34])
def test_volume_without_a_negative_keeps_its_bits(dev, lib, n):
    rc.check_nonnegative_is_returned_as_is(lib, dev, n)


@pytest.mark.parametrize("n", [128, 160])
def test_restrained_volume_under_guarded_allocations(dev, lib, n):
    rc.check_restrain_on_the_device(lib, dev, n)


def test_candidate_lists_are_thinned_and_rebuilt(dev, lib):
    rc.check_restrain_cand(lib, dev)


def test_zero_fill_with_fewer_allowed_negatives_than_K(dev, lib):
    rc.check_zero_fill(lib, dev)


def test_restraint_errors(dev, lib):
    rc.check_errors(lib, dev)


def test_engine_list_on_every_selection_path(dev, lib):
    rc.check_engine_paths(lib, dev)


def test_engine_search_at_other_launch_batches_and_without_rebuild(dev, lib):
    rc.check_engine_search(lib, dev)


def test_engine_list_on_an_embedded_box(dev, lib):
    rc.check_engine_embedded(lib, dev)


def test_user_defined_model_reaches_the_unfused_loop(dev):
    rc.check_docker_unfused(None, dev)


def test_update_top_and_the_report(dev, lib):
    rc.check_update_top(lib, dev)


def test_live_engine_across_restraint_sets_and_the_default(dev):
    rc.check_reuse_and_defaults(None, dev)


def test_two_ranks_give_the_one_rank_list(dev):
    rc.check_two_ranks(None, dev)


def test_dock_pair_restraint_step(dev, tmp_path):
    rc.check_dock_pair(None, dev, tmp_path)
