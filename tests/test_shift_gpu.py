"""Sub-voxel translations on the real gfx950 build: the trilinear rotation with a per-pose offset (csrc/dlpd_rotate_shift.h)
-- forward, adjoint, pose gradient, local correlation -- against float64, its exact cases, determinism and chunking, errors,
``shift=`` of the ops, ``Docker.score_poses(shift=)`` and ``Docker.minimize(translation=True)`` on a planted pose with a planted
fraction.  Check bodies and the derivation of the bounds: tests/shift_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import shift_checks as sc

pytestmark = pytest.mark.gpu


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


# (L, C, B): odd, blocks straddle rows; one channel more than 16; the largest box (8192 partials per pose)
SHAPES = [(33, 3, 3), (40, 17, 2), (128, 1, 1)]


@pytest.mark.parametrize("L,C,B", SHAPES)
def test_zero_offset_is_the_plain_call_bit_for_bit(dev, lib, L, C, B):
    sc.check_zero_offset(lib, dev, L, C, B)


def test_signed_permutations_with_integer_offsets_are_exact(dev, lib):
    sc.check_signed_permutations(lib, dev, 33)


def test_an_offset_of_a_whole_box_leaves_nothing(dev, lib):
    sc.check_offset_of_a_whole_box(lib, dev, 33)


@pytest.mark.parametrize("L,C,B", SHAPES)
def test_rotate_shift_matches_float64(dev, lib, L, C, B):
    sc.check_forward(lib, dev, L, C, B)


@pytest.mark.parametrize("summed", [False, True])
@pytest.mark.parametrize("L,C,B", SHAPES)
def test_rotate_shift_grad_matches_float64_scatter_and_the_forward_kernel(dev, lib, L, C, B, summed):
    sc.check_adjoint(lib, dev, L, C, B, summed)
    sc.check_transpose(lib, dev, L, C, B, summed)


def test_rotate_shift_grad_accumulates_across_calls(dev, lib):
    sc.check_accumulate(lib, dev, L=33)


@pytest.mark.parametrize("L,C,B", SHAPES)
def test_pose_gradient_matches_float64_autograd(dev, lib, L, C, B):
    sc.check_pose_gradient(lib, dev, L, C, B)


def test_offset_gradient_of_a_ramp_is_its_slope(dev, lib):
    sc.check_ramp(lib, dev, 33)


def test_shifted_chunks_give_the_bytes_of_one_call(dev, lib, monkeypatch):
    sc.check_chunking(lib, dev, monkeypatch)


def test_shift_errors(dev, lib):
    sc.check_errors(lib, dev)


def test_volume_rotation_shift(dev, lib):
    sc.check_volume_rotation_autograd(lib, dev, L=33)


def test_volume_rotation_shift_with_every_convention(dev, lib):
    sc.check_volume_rotation_autograd(lib, dev, L=33, scale="(L-1)/L", axis_order="zyx", transpose=True)


def test_local_correlate_rotated_shift(dev, lib):
    sc.check_local_correlate_rotated(lib, dev, 40, 4, 3, 2, 2, "floor", True)
    sc.check_local_correlate_rotated(lib, dev, 40, 4, 3, 1, 1, "trunc", False)


@pytest.mark.parametrize("Ls", [[32], [32, 16]])
def test_score_poses_shift(dev, Ls):
    sc.check_score_poses(None, dev, Ls)


@pytest.mark.parametrize("Ls", [[32], [32, 16]])
def test_minimize_without_translation_is_unchanged(dev, Ls, tmp_path):
    sc.check_minimize_unchanged(None, dev, Ls, tmp_path)


@pytest.mark.parametrize("Ls", [[32], [32, 16]])
def test_minimize_translation_finds_the_planted_fraction(dev, Ls, tmp_path):
    sc.check_minimize_translation(None, dev, Ls, tmp_path)
