"""A live DockingEngine scores the next pair as a fresh engine does, on the real gfx950 build: the side stream, the two V
buffers and candidate sets, the packed receptor and the pencil map exist only here.  Every sequence runs poisoned and plain,
on the default stream arrangement of ``search()``.  Check bodies, the poison and what each case asserts on its own inputs:
tests/engine_reuse_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import engine_reuse_checks as rc

pytestmark = pytest.mark.gpu

BOTH = (True, False)


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


def test_box_40_sparse_dense_sparse_pairs_on_a_live_engine(dev, lib):
    rc.check_case1(lib, dev, BOTH)


@pytest.mark.parametrize("L", [64, 80])
def test_two_resolutions_on_a_live_engine(dev, lib, L):
    rc.check_two_resolutions(lib, dev, L, BOTH)


def test_per_channel_k1_on_a_live_engine(dev, lib):
    rc.check_per_channel(lib, dev, BOTH)


def test_embedded_extent_on_a_live_engine(dev, lib):
    rc.check_embedded_extent(lib, dev, BOTH)


def test_given_volumes_between_two_searches(dev, lib):
    rc.check_given_volumes(lib, dev, BOTH)


def test_live_filter_change_on_a_pooled_engine(dev, lib):
    rc.check_live_filter_change(lib, dev, BOTH)


def test_docker_keeps_its_engine_from_pair_to_pair(dev, lib):
    rc.check_docker(lib, dev)
