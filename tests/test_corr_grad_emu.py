"""The differentiable VolumeConvolution on the CPU-emulated kernel library: the adjoint FFT kernels (csrc/dlpd_corr_grad.h) and
the plan-free adjoint (dlpd_correlate_generic_grad) against the float64 formulas, their exact cases, the transpose identity
with the forward kernel, the clamp, the autograd surface of ops.VolumeConvolution and GlobalDockingModel(differentiable=True).
Boxes 32 and 40 only (the emulator runs every thread as a fibre).  Check bodies and tolerances: tests/corr_grad_checks.py."""
import pytest

import corr_grad_checks as cg


@pytest.mark.parametrize("L,B,C", [(32, 2, 2), (40, 1, 3)])
def test_corr_grad_matches_float64(emu, L, B, C):
    cg.check_dense(emu, "cpu", L, B, C)


def test_corr_grad_special_gradients(emu):
    cg.check_special_gradients(emu, "cpu", 32)


def test_corr_grad_is_the_transpose_of_the_forward_kernel(emu):
    cg.check_transpose(emu, "cpu", 32, 1, 6)


def test_corr_grad_clip_masks_the_clamped_translations(emu):
    cg.check_clip(emu, "cpu", 32)


def test_volume_convolution_autograd_surface(emu):
    cg.check_autograd_surface(emu, "cpu", 32, C=1)


def test_corr_grad_chunks_of_volumes_give_the_bits_of_one(emu):
    cg.check_chunks(emu, "cpu", 32)


def test_corr_grad_embedded_box(emu):
    cg.check_dense(emu, "cpu", 33, 1, 1, embed=True)


@pytest.mark.parametrize("L", [9, 33])
def test_corr_grad_plan_free_box(emu, L):
    cg.check_dense(emu, "cpu", L, 1, 2 if L == 9 else 1, embed=False)


def test_corr_grad_errors(emu):
    cg.check_errors(emu, "cpu")


def test_global_model_parameter_gradients_follow_float64(emu):
    cg.check_model_gradients(emu, "cpu", 32, channels=1)


def test_global_model_is_governed_by_the_differentiable_flag(emu):
    cg.check_model_flag(emu, "cpu", 32, channels=1)


def test_global_model_trains_on_plan_free_boxes(emu):
    """Boxes 8 and 4 by the plan-free kernels (embed=False): five Adam steps in a second; box 32 is the device test's."""
    cg.check_model_trains(emu, "cpu", 8, embed=False)
