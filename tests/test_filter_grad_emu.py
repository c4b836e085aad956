"""The differentiable grid filter on the CPU-emulated kernel library: the fused backward kernel (csrc/dlpd_filter_grad.h) against
the plain-torch restatement of the module path -- bit for bit on dyadic inputs, through the yardstick on random ones --, the
autograd surface of ops.filter_volumes_autograd and GlobalDockingModel(fused_filter_grad=True).  Check bodies and tolerances:
tests/filter_grad_checks.py."""
import pytest

import filter_grad_checks as fg


@pytest.mark.parametrize("shape", fg.EXACT_SHAPES)
def test_filter_grad_equals_float64_on_dyadic_inputs(emu, shape):
    fg.check_exact(emu, "cpu", shape)


@pytest.mark.parametrize("shape", fg.RANDOM_SHAPES)
def test_filter_grad_follows_float64(emu, shape):
    fg.check_random(emu, "cpu", shape)


def test_filter_volumes_autograd_surface(emu):
    fg.check_surface(emu, "cpu")


def test_filter_grad_unsupported_shapes(emu):
    fg.check_unsupported(emu, "cpu")


def test_global_model_with_the_fused_filter_backward(emu):
    """Boxes 8 and 4 by the plan-free correlations (embed=False): the emulator runs every thread as a fibre; box 32 is the
    device test's."""
    fg.check_model(emu, "cpu", 8, embed=False)
