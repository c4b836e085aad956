"""The tile-occupancy path of the representation stage at lopsided per-entry maps, on the real gfx950 build: every check with
the whole support family.  Check bodies, the supports and what each case asserts on its own inputs:
tests/repr_sparse_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import repr_sparse_checks as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    import __graft_entry__ as entry
    entry.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    rs.release_cases()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def lib(dev):
    from deeplocalproteindocking_amd._lib import get_lib
    return get_lib()


@pytest.mark.parametrize("D", [21, 13, 37, 80])
def test_tile_occupancy_equals_the_host_map(dev, lib, D):
    rs.check_map(lib, dev, D)


@pytest.mark.parametrize("D", [21, 13, 37, 80])
def test_skipping_changes_no_bit(dev, lib, D):
    rs.check_skipping_changes_no_bit(lib, dev, D)


@pytest.mark.parametrize("D", [21, 13, 37, 80])
def test_unwritten_activations_at_per_entry_maps(dev, lib, D):
    rs.check_unwritten(lib, dev, D)


@pytest.mark.parametrize("D", [21, 13, 37])
def test_covering_maps_give_the_same_bits(dev, lib, D):
    rs.check_covering_maps(lib, dev, D)


@pytest.mark.parametrize("D", [21, 13, 37])                      # (box 80: torch's float64 conv3d takes the host a minute)
def test_sparse_convolutions_and_pooling_against_torch(dev, lib, D):
    rs.check_truth(lib, dev, D)


@pytest.mark.parametrize("D", [21, 13, 37, 80])
def test_pooling_with_maps_meets_all_three_kinds_of_window(dev, lib, D):
    rs.check_pool_windows(lib, dev, D)


@pytest.mark.parametrize("L,C", [(32, 16), (40, 32)])
def test_volumes_k1_goes_by_per_entry_maps(dev, lib, L, C):
    rs.check_consumer(lib, dev, L, C)


@pytest.mark.parametrize("D", [21, 80])
def test_plugin_outputs_with_maps(dev, lib, D):
    rs.check_plugin(lib, dev, D)


def test_plugin_on_a_cell_wise_projected_protein(dev, lib):
    rs.check_plugin_on_projected_protein(lib, dev, 40, 1.25)


def test_pooling_of_more_volumes_than_one_launch_holds(dev, lib):
    rs.check_pool_many_volumes(lib, dev)


def test_pooling_with_maps_over_two_launches(dev, lib):
    rs.check_pool_chunked_maps(lib, dev)
