"""The rotation's gradient with respect to its matrices on the CPU-emulated kernel library: the kernel of
csrc/dlpd_rotate_rgrad.h against float64 autograd, its exact cases, determinism and chunking, errors, ``rotation_grad=True`` of
ops.VolumeRotation and ops.local_correlate_rotated, Docker.minimize on a planted pose.
Check bodies and the derivation of the bound: tests/pose_grad_checks.py."""
import pytest

import pose_grad_checks as pg

# (L, C, B): one block; an odd box; two blocks with the last partly filled and one channel more than 16; the emulator's largest
SHAPES = [(6, 3, 2), (9, 2, 3), (11, 17, 2), (12, 1, 2)]


def test_the_float64_expectation_follows_a_central_difference():
    pg.check_expectation()


@pytest.mark.parametrize("L,C,B", SHAPES)
def test_rotate_rgrad_matches_float64_autograd(emu, L, C, B):
    pg.check_kernel(emu, "cpu", L, C, B)


@pytest.mark.parametrize("L", [9, 12])
def test_rotate_rgrad_of_a_ramp_is_its_slope(emu, L):
    pg.check_ramp(emu, "cpu", L)


def test_rotate_rgrad_of_signed_permutations_is_the_forward_difference(emu):
    pg.check_signed_permutations(emu, "cpu", L=9)


def test_rotate_rgrad_zero_and_scaling(emu):
    pg.check_zero_and_scaling(emu, "cpu")


def test_rotation_grad_chunks_give_the_bytes_of_one_call(emu, monkeypatch):
    pg.check_chunking(emu, "cpu", monkeypatch)


def test_rotate_rgrad_errors(emu):
    pg.check_errors(emu, "cpu")


def test_volume_rotation_rotation_grad(emu):
    pg.check_volume_rotation_autograd(emu, "cpu", L=9)


def test_volume_rotation_rotation_grad_with_every_convention(emu):
    pg.check_volume_rotation_autograd(emu, "cpu", L=9, scale="(L-1)/L", axis_order="zyx", transpose=True)


@pytest.mark.parametrize("L,r,scale,mode,shared", [(7, 2, 2, "floor", True), (9, 1, 1, "trunc", False)])
def test_local_correlate_rotated_rotation_grad(emu, L, r, scale, mode, shared):
    pg.check_local_correlate_rotated(emu, "cpu", L, 2, 4, r, scale, mode, shared)


def test_minimize_descends_to_the_planted_pose(emu, tmp_path):
    """Box 16 (float64 pure torch: 6.00 degrees -> 0.32)."""
    pg.check_minimize(emu, "cpu", [16], tmp_path)
