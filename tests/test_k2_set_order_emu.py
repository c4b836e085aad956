"""K2's set ping-pong (csrc/dlpd_k2.hip) on the emulated kernels: the case matrix of test_k2_set_order_gpu.py (the comparison
with the build without the ping-pong is on the device only).  An emulated launch of nine rotations at box 64 takes 15 - 20 s;
the cases are independent and the CPU suite runs them on its parallel workers."""
import pytest

import k2_set_order_checks as so


@pytest.mark.parametrize("transposed", [0, 1])
@pytest.mark.parametrize("nb", [1, 2, 3, 9])
@pytest.mark.parametrize("L", [32, 64])
def test_shared_receptor(emu, L, nb, transposed):
    """nb = 1, 2: one part, without and with a second rotation; 3: the last rotation on the flipped order; 9: two parts of
    4 and 5 rotations, both parities start and end a part."""
    so.check_against_float64(emu, "cpu", L, 3, nb, transposed)


@pytest.mark.parametrize("transposed", [0, 1])
@pytest.mark.parametrize("nb", [2, 3, 9])
@pytest.mark.parametrize("L", [32, 64])
def test_position_in_the_batch_changes_no_bit(emu, L, nb, transposed):
    so.check_position_in_the_batch_changes_no_bit(emu, "cpu", L, 3, nb, transposed)


@pytest.mark.parametrize("nb", [2, 9])
def test_shared_receptor_box_40_transposed(emu, nb):
    """N = 80 through this kernel: no register hand-over, blocked intermediates in the 8 spare rows."""
    so.check_against_float64(emu, "cpu", 40, 2, nb, 1)
    so.check_position_in_the_batch_changes_no_bit(emu, "cpu", 40, 2, nb, 1)


@pytest.mark.parametrize("nb", [3, 9])
@pytest.mark.parametrize("L", [32, 64])
def test_receptor_per_rotation(emu, L, nb):
    """Every rotation has its own receptor: nothing may be kept from one rotation to the next."""
    so.check_against_float64(emu, "cpu", L, 3, nb, 0, per_rotation=True)


def test_forward_only(emu):
    so.check_forward_only(emu, "cpu")
