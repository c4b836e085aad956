"""K1's four-lane gather at box 64 (csrc/dlpd_k1.h, ZPAIR) on the gfx950 build, against the channels-last entry bit for bit:
integer sample positions, oblique rotations that straddle both z faces, whole planes outside on either z side, strictly
negative and mixed-sign volumes, one / a zero-padded second / three channel chunks, an embedded extent, occupancy maps, and
the engine's ranked list with the layout on and off.  Every case is at L = 64 with at most four rotations."""
import pytest
import torch

import k1_chunk_layout_checks as chk
import k1_zpair_checks as zp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs a GPU"
    import __graft_entry__ as entry
    entry.build()
    from deeplocalproteindocking_amd._lib import get_lib
    return get_lib()


@pytest.mark.parametrize("kind", ["negative", "mixed"])
@pytest.mark.parametrize("C", [8, 12])
def test_identity_and_quarter_turns_on_device(lib, C, kind):
    zp.check_lattice(lib, "cuda:0", C, kind)


@pytest.mark.parametrize("kind", ["negative", "mixed"])
@pytest.mark.parametrize("C", [8, 12])
def test_oblique_rotations_across_both_z_faces_on_device(lib, C, kind):
    zp.check_oblique_faces(lib, "cuda:0", C, kind, nb=3)


@pytest.mark.parametrize("kind", ["negative", "mixed"])
def test_twenty_channels_into_a_wider_workspace_on_device(lib, kind):
    zp.check_oblique_faces(lib, "cuda:0", 20, kind, c_base=3, extra=2, nb=3)


@pytest.mark.parametrize("kind", ["negative", "mixed"])
@pytest.mark.parametrize("side", ["low", "high"])
def test_whole_planes_outside_the_box_on_device(lib, side, kind):
    zp.check_planes_outside(lib, "cuda:0", 8, kind, side)


@pytest.mark.parametrize("C,c_base", [(8, 0), (12, 0), (20, 3)])
@pytest.mark.parametrize("case", ["extent", "occupancy"])
def test_embedded_extent_and_occupancy_maps_on_device(lib, case, C, c_base):
    kw = {"extent": {"extent": 48}, "occupancy": {"occupancy": True}}[case]
    chk.check_k1_equality(lib, "cuda:0", zp.L, C, chk.rotations("z+oblique", 2), c_base=c_base, extra=2, **kw)


def test_ranked_list_of_a_search_at_box_64_on_device(lib):
    chk.check_engine_lists(lib, "cuda:0", L=zp.L, C=8, nrot=32, batch=8)
