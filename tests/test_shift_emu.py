"""Sub-voxel translations on the CPU-emulated kernel library: the trilinear rotation with a per-pose offset
(csrc/dlpd_rotate_shift.h) -- forward, adjoint, pose gradient, local correlation -- against float64, its exact cases,
determinism and chunking, errors, ``shift=`` of the ops, ``Docker.score_poses(shift=)`` and ``Docker.minimize(translation=True)``
on a planted pose with a planted fraction.  Check bodies and the derivation of the bounds: tests/shift_checks.py."""
import pytest

import shift_checks as sc

# (L, C, B): odd boxes (pivot 2.5 / 4.5) and an even one
SHAPES = [(5, 3, 3), (9, 2, 3), (8, 3, 3)]
GPU_SHAPES = [(33, 3, 3), (40, 17, 2), (128, 1, 1)]                      # tests/test_shift_gpu.py


def test_the_float64_expectation_follows_a_central_difference():
    sc.check_expectation()


def test_the_seeds_keep_the_samples_off_the_cell_faces_at_every_shape():
    sc.check_face_fractions(SHAPES + GPU_SHAPES)


@pytest.mark.parametrize("L,C,B", SHAPES)
def test_zero_offset_is_the_plain_call_bit_for_bit(emu, L, C, B):
    sc.check_zero_offset(emu, "cpu", L, C, B)


@pytest.mark.parametrize("L", [5, 8])
def test_signed_permutations_with_integer_offsets_are_exact(emu, L):
    sc.check_signed_permutations(emu, "cpu", L)


def test_an_offset_of_a_whole_box_leaves_nothing(emu):
    sc.check_offset_of_a_whole_box(emu, "cpu", 5)


@pytest.mark.parametrize("L,C,B", SHAPES)
def test_rotate_shift_matches_float64(emu, L, C, B):
    sc.check_forward(emu, "cpu", L, C, B)


@pytest.mark.parametrize("summed", [False, True])
@pytest.mark.parametrize("L,C,B", SHAPES)
def test_rotate_shift_grad_matches_float64_scatter_and_the_forward_kernel(emu, L, C, B, summed):
    sc.check_adjoint(emu, "cpu", L, C, B, summed)
    sc.check_transpose(emu, "cpu", L, C, B, summed)


def test_rotate_shift_grad_accumulates_across_calls(emu):
    sc.check_accumulate(emu, "cpu")


@pytest.mark.parametrize("L,C,B", SHAPES)
def test_pose_gradient_matches_float64_autograd(emu, L, C, B):
    sc.check_pose_gradient(emu, "cpu", L, C, B)


@pytest.mark.parametrize("L", [9, 8])
def test_offset_gradient_of_a_ramp_is_its_slope(emu, L):
    sc.check_ramp(emu, "cpu", L)


def test_shifted_chunks_give_the_bytes_of_one_call(emu, monkeypatch):
    sc.check_chunking(emu, "cpu", monkeypatch)


def test_shift_errors(emu):
    sc.check_errors(emu, "cpu")


def test_volume_rotation_shift(emu):
    sc.check_volume_rotation_autograd(emu, "cpu", L=9)


def test_volume_rotation_shift_with_every_convention(emu):
    sc.check_volume_rotation_autograd(emu, "cpu", L=9, scale="(L-1)/L", axis_order="zyx", transpose=True)


@pytest.mark.parametrize("L,r,scale,mode,shared", [(7, 2, 2, "floor", True), (9, 1, 1, "trunc", False)])
def test_local_correlate_rotated_shift(emu, L, r, scale, mode, shared):
    sc.check_local_correlate_rotated(emu, "cpu", L, 2, 4, r, scale, mode, shared)


def test_score_poses_shift(emu):
    sc.check_score_poses(emu, "cpu", [16])


def test_minimize_without_translation_is_unchanged(emu, tmp_path):
    sc.check_minimize_unchanged(emu, "cpu", [16], tmp_path)


def test_minimize_translation_finds_the_planted_fraction(emu, tmp_path):
    sc.check_minimize_translation(emu, "cpu", [16], tmp_path)
