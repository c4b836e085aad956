"""K1's four-lane gather at box 64 (csrc/dlpd_k1.h, ZPAIR) on the emulated kernels, where the quad exchange is a wave shuffle
between fibers: the cases of test_k1_zpair_gpu.py with one or two rotations each -- a K1 launch at L = 64 is 256 emulated
blocks per rotation and chunk, about 8 s for the pair of launches a comparison makes.  The engine's ranked list at box 64 is
checked on the device only: the emulator would spend most of an hour in K2 and K3 there, which this gather does not touch."""
import pytest

import k1_chunk_layout_checks as chk
import k1_zpair_checks as zp


def test_identity_and_a_quarter_turn(emu):
    """One chunk, strictly negative: integer positions, one plane beyond the high z face (-0.0 samples)."""
    zp.check_lattice(emu, "cpu", 8, "negative", nb=2)


def test_oblique_rotation_across_both_z_faces_twenty_channels_into_a_wider_workspace(emu):
    """Three chunks, the last one half zero padding, c_base = 3."""
    zp.check_oblique_faces(emu, "cpu", 20, "mixed", c_base=3, extra=2, nb=1)


@pytest.mark.parametrize("side,kind", [("low", "negative"), ("high", "mixed")])
def test_whole_planes_outside_the_box(emu, side, kind):
    zp.check_planes_outside(emu, "cpu", 8, kind, side, nb=1)


@pytest.mark.parametrize("case", ["extent", "occupancy"])
def test_embedded_extent_and_occupancy_maps(emu, case):
    kw = {"extent": {"extent": 48}, "occupancy": {"occupancy": True}}[case]
    chk.check_k1_equality(emu, "cpu", zp.L, 8, chk.rotations("oblique", 1), **kw)
