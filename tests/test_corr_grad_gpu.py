"""The differentiable VolumeConvolution on the real gfx950 build: the adjoint FFT kernels at every compiled box, the plan-free
adjoint, exact cases, the transpose identity with the forward kernel, the clamp, the autograd surface and
GlobalDockingModel(differentiable=True) trained on a loss over the whole translation grid.  Check bodies and tolerances:
tests/corr_grad_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import corr_grad_checks as cg

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


# batch and channel strides; three channels at the coarse box of the reference; the two large plans
@pytest.mark.parametrize("L,B,C", [(32, 2, 2), (40, 1, 3), (64, 1, 2), (80, 1, 1)])
def test_corr_grad_matches_float64(dev, lib, L, B, C):
    cg.check_dense(lib, dev, L, B, C)


# all four kinds at every compiled box; the two single-number kinds pooled over 16 volumes (check_special_gradients), 8 at
# box 80, where the float32 oracle of 18 volumes of 160^3 on the host is what the test costs.  Their truth is the closed form:
# boxes 64 and 80 leave the float64 transform out
@pytest.mark.parametrize("L,reps,float64_check", [(32, 16, True), (40, 16, True), (64, 16, False), (80, 8, False)])
def test_corr_grad_special_gradients(dev, lib, L, reps, float64_check):
    cg.check_special_gradients(lib, dev, L, reps=reps, float64_check=float64_check)


@pytest.mark.parametrize("L,C", [(32, 6), (80, 4)])
def test_corr_grad_is_the_transpose_of_the_forward_kernel(dev, lib, L, C):
    cg.check_transpose(lib, dev, L, 1, C)


def test_corr_grad_clip_masks_the_clamped_translations(dev, lib):
    cg.check_clip(lib, dev, 32)


def test_volume_convolution_autograd_surface(dev, lib):
    cg.check_autograd_surface(lib, dev, 32, C=5)


def test_corr_grad_chunks_of_volumes_give_the_bits_of_one(dev, lib):
    cg.check_chunks(lib, dev, 32)


def test_corr_grad_embedded_box(dev, lib):
    cg.check_dense(lib, dev, 33, 1, 2, embed=True)


def test_corr_grad_plan_free_box(dev, lib):
    cg.check_dense(lib, dev, 33, 1, 2, embed=False)


def test_corr_grad_errors(dev, lib):
    cg.check_errors(lib, dev)


def test_global_model_parameter_gradients_follow_float64(dev, lib):
    cg.check_model_gradients(lib, dev, 32)


def test_global_model_is_governed_by_the_differentiable_flag(dev, lib):
    cg.check_model_flag(lib, dev, 32)


def test_global_model_trains(dev, lib):
    cg.check_model_trains(lib, dev, 32)
