"""The differentiable grid filter on the real gfx950 build: the fused backward kernel (csrc/dlpd_filter_grad.h) against the
plain-torch restatement of the module path -- bit for bit on dyadic inputs, through the yardstick on random ones, one of them
large enough for the cross-block reduction and the grid-stride loop --, the autograd surface of ops.filter_volumes_autograd and
GlobalDockingModel(fused_filter_grad=True).  Check bodies and tolerances: tests/filter_grad_checks.py.  Nothing here reads the
reference tree."""
import pytest
import torch

import filter_grad_checks as fg

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


@pytest.mark.parametrize("shape", fg.EXACT_SHAPES)
def test_filter_grad_equals_float64_on_dyadic_inputs(dev, lib, shape):
    fg.check_exact(lib, dev, shape)


@pytest.mark.parametrize("shape", fg.RANDOM_SHAPES + [fg.RANDOM_SHAPE_GPU])
def test_filter_grad_follows_float64(dev, lib, shape):
    fg.check_random(lib, dev, shape)


def test_filter_volumes_autograd_surface(dev, lib):
    fg.check_surface(lib, dev)


def test_filter_grad_unsupported_shapes(dev, lib):
    fg.check_unsupported(lib, dev)


def test_global_model_with_the_fused_filter_backward(dev, lib):
    fg.check_model(lib, dev, 32)
