"""K2's set ping-pong (csrc/dlpd_k2.hip) on the gfx950 build, called directly on random spectra against float64: boxes 32
and 64 (N = 64, 128) with 1, 2, 3 and 9 rotations in both slab orientations, box 40 transposed (N = 80 through this kernel),
a receptor per rotation (fixed order, nothing kept), the forward-only mode, and the same bits as the kernel without the
ping-pong (tests/variants/libdlpd_k2_loop.so: dlpd_k2.hip compiled -DDLPD_K2_SET_PINGPONG=0, built with the test variants)."""
import pytest
import torch

import k2_set_order_checks as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs a GPU"
    import __graft_entry__ as entry
    entry.build()
    from deeplocalproteindocking_amd._lib import get_lib
    return get_lib()


@pytest.fixture(scope="module")
def loop_lib(lib):
    """K2 as it was before the ping-pong: fixed set order, two receptor fetches per rotation.  A build failure is an error."""
    import __graft_entry__ as entry
    from deeplocalproteindocking_amd._lib import DlpdLib
    return DlpdLib(entry.build_k2_loop_reference())


@pytest.mark.parametrize("transposed", [0, 1])
@pytest.mark.parametrize("nb", [1, 2, 3, 9])
@pytest.mark.parametrize("L", [32, 64])
def test_shared_receptor_on_device(lib, L, nb, transposed):
    """nb = 1, 2: one part, without and with a second rotation; 3: the last rotation on the flipped order; 9: two parts of
    4 and 5 rotations, both parities start and end a part."""
    so.check_against_float64(lib, "cuda:0", L, 3, nb, transposed)
    if nb > 1:
        so.check_position_in_the_batch_changes_no_bit(lib, "cuda:0", L, 3, nb, transposed)


@pytest.mark.parametrize("nb", [2, 9])
def test_shared_receptor_box_40_transposed_on_device(lib, nb):
    """N = 80 through this kernel: no register hand-over, blocked intermediates in the 8 spare rows."""
    so.check_against_float64(lib, "cuda:0", 40, 2, nb, 1)
    so.check_position_in_the_batch_changes_no_bit(lib, "cuda:0", 40, 2, nb, 1)


@pytest.mark.parametrize("nb", [3, 9])
@pytest.mark.parametrize("L", [32, 64])
def test_receptor_per_rotation_on_device(lib, L, nb):
    """Every rotation has its own receptor: nothing may be kept from one rotation to the next."""
    so.check_against_float64(lib, "cuda:0", L, 3, nb, 0, per_rotation=True)


def test_forward_only_on_device(lib):
    so.check_forward_only(lib, "cuda:0")


@pytest.mark.parametrize("L,nb,transposed", [(64, 9, 0), (32, 3, 1)])
def test_same_bits_as_the_build_without_the_ping_pong(lib, loop_lib, L, nb, transposed):
    """The arithmetic per element is untouched, so the library whose K2 visits the sets in a fixed order and fetches both
    sets' receptor values for every rotation gives the same bits."""
    so.check_same_bits_as(lib, loop_lib, "cuda:0", L, 3, nb, transposed)
