"""The rotation's gradient with respect to its matrices on the real gfx950 build: the kernel of csrc/dlpd_rotate_rgrad.h
against float64 autograd, its exact cases, determinism and chunking, errors, ``rotation_grad=True`` of ops.VolumeRotation and
ops.local_correlate_rotated, Docker.minimize on a planted pose.  Check bodies and the derivation of the bound:
tests/pose_grad_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import pose_grad_checks as pg

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


# (L, C, B): a box that is no multiple of anything; one channel more than 16; the reference's fine grid; the largest box
SHAPES = [(33, 3, 4), (40, 17, 3), (80, 2, 2), (128, 1, 1)]


@pytest.mark.parametrize("L,C,B", SHAPES)
def test_rotate_rgrad_matches_float64_autograd(dev, lib, L, C, B):
    pg.check_kernel(lib, dev, L, C, B)


def test_rotate_rgrad_of_a_ramp_is_its_slope(dev, lib):
    pg.check_ramp(lib, dev, 33)


def test_rotate_rgrad_of_signed_permutations_is_the_forward_difference(dev, lib):
    pg.check_signed_permutations(lib, dev, L=33)


def test_rotate_rgrad_zero_and_scaling(dev, lib):
    pg.check_zero_and_scaling(lib, dev, L=33)


def test_rotation_grad_chunks_give_the_bytes_of_one_call(dev, lib, monkeypatch):
    pg.check_chunking(lib, dev, monkeypatch)


def test_rotate_rgrad_errors(dev, lib):
    pg.check_errors(lib, dev)


def test_volume_rotation_rotation_grad(dev, lib):
    pg.check_volume_rotation_autograd(lib, dev, L=33)


def test_volume_rotation_rotation_grad_with_every_convention(dev, lib):
    pg.check_volume_rotation_autograd(lib, dev, L=33, scale="(L-1)/L", axis_order="zyx", transpose=True)


def test_local_correlate_rotated_rotation_grad(dev, lib):
    pg.check_local_correlate_rotated(lib, dev, 40, 4, 3, 2, 2, "floor", True)
    pg.check_local_correlate_rotated(lib, dev, 40, 4, 3, 1, 1, "trunc", False)


@pytest.mark.parametrize("Ls", [[32], [32, 16]])
def test_minimize_descends_to_the_planted_pose(dev, Ls, tmp_path):
    pg.check_minimize(None, dev, Ls, tmp_path)
