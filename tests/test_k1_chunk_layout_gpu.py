"""K1 gathering from the chunk-major ligand copy on the gfx950 build, against the channels-last source bit for bit: box 64
(8-channel chunks: three of them at 20 channels, the last half full), box 40 (the coarse grid of the reference model's shapes),
and the engine's ranked list with the layout on and off."""
import pytest
import torch

import k1_chunk_layout_checks as chk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs a GPU"
    import __graft_entry__ as entry
    entry.build()
    from deeplocalproteindocking_amd._lib import get_lib
    return get_lib()


@pytest.mark.parametrize("L,C", [(64, 20), (40, 16)])
def test_chunk_major_copy_layout_on_device(lib, L, C):
    chk.check_layout(lib, "cuda:0", L, C)


@pytest.mark.parametrize("L,C", [(64, 20), (40, 16)])
@pytest.mark.parametrize("case", ["dense", "extent", "occupancy", "c_base"])
def test_k1_from_chunks_equals_channels_last_on_device(lib, L, C, case):
    kw = {"dense": {}, "extent": {"extent": (3 * L) // 4}, "occupancy": {"occupancy": True}, "c_base": {"c_base": 3, "extra": 2}}[case]
    chk.check_k1_equality(lib, "cuda:0", L, C, chk.rotations("z+oblique", 2), **kw)


def test_engine_lists_do_not_depend_on_the_k1_source_layout_on_device(lib):
    chk.check_engine_lists(lib, "cuda:0")
