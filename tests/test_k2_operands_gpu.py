"""The receptor in consumption order at boxes 64 / 32 (csrc/dlpd_k2.hip; dlpd_receptor_order, dlpd_xy_correlate_ordered) on
the gfx950 build: the copy itself, K2 called directly on random spectra against float64 with 1, 2, 3 and 9 rotations and the
same bits as the natural call, a receptor per rotation, and a search with and without the copy."""
import pytest
import torch

import k2_operands_checks as op

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs a GPU"
    import __graft_entry__ as entry
    entry.build()
    from deeplocalproteindocking_amd._lib import get_lib
    return get_lib()


@pytest.mark.parametrize("L", [32, 64])
def test_ordered_copy_is_the_permutation_the_header_names_on_device(lib, L):
    op.check_ordered_copy(lib, "cuda:0", L)


def test_size_queries_and_refusals_on_device(lib):
    op.check_size_queries(lib)


@pytest.mark.parametrize("nb", [1, 2, 3, 9])
@pytest.mark.parametrize("L", [32, 64])
def test_shared_receptor_ordered_on_device(lib, L, nb):
    """nb = 1, 2: one part, without and with a second rotation; 3: the last rotation on the flipped order; 9: two parts of
    4 and 5 rotations, both parities start and end a part."""
    op.check_ordered_against_float64(lib, "cuda:0", L, nb)


@pytest.mark.parametrize("L", [32, 64])
def test_receptor_per_rotation_stays_on_the_natural_layout_on_device(lib, L):
    op.check_receptor_per_rotation(lib, "cuda:0", L, 3)


def test_engine_lists_with_and_without_the_ordered_receptor_on_device(lib):
    op.check_engine_lists(lib, "cuda:0")
