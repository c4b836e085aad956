"""The convolution's backward on the real gfx950 build: the weight-gradient kernel at the emulator's small shapes and at the
reference's boxes (default nparts) against float64, its index arithmetic and determinism, the input gradient, the autograd
Function, both plugins with ``hip_autograd`` at box 16 and one LocalTrainer step with hip_conv.  Check bodies and
tolerances: tests/conv_grad_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import conv_grad_checks as cg

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


@pytest.mark.parametrize("B,cin,cout,ks,D,nparts", cg.SMALL_CASES + cg.LARGE_CASES)
def test_weight_grad_matches_float64(dev, lib, B, cin, cout, ks, D, nparts):
    cg.check_weight_grad(None, dev, B, cin, cout, ks, D, nparts, " (MI355X)")


@pytest.mark.parametrize("ks", [3, 5])
@pytest.mark.parametrize("far", [False, True])
def test_weight_grad_index_exactness(dev, lib, ks, far):
    cg.check_index_exactness(None, dev, ks, far)


def test_weight_grad_is_deterministic(dev, lib):
    cg.check_determinism(None, dev, 1, 32, 32, 3, 6, 7, 3)
    cg.check_determinism(None, dev, 2, 16, 32, 5, 40, 256, 64)


@pytest.mark.parametrize("precision", ["f32", "split_bf16"])
@pytest.mark.parametrize("B,cin,cout,ks,D", [(2, 16, 16, 3, 9), (1, 32, 16, 5, 7)])
def test_input_grad_matches_float64(dev, lib, B, cin, cout, ks, D, precision):
    cg.check_input_grad(None, dev, B, cin, cout, ks, D, precision)


def test_input_grad_refuses_a_layer_of_11_channels(dev, lib, monkeypatch):
    cg.check_input_grad_refuses(None, dev, monkeypatch)


@pytest.mark.parametrize("relu", [False, True])
def test_conv3d_autograd_follows_float64(dev, lib, relu):
    cg.check_function(None, dev, relu)


@pytest.mark.parametrize("plugin", ["E3MultiResRepr4x4", "SE3MultiResReprScalar"])
def test_plugin_trains_on_the_kernels(dev, lib, monkeypatch, plugin):
    from deeplocalproteindocking_amd import Models
    cg.check_plugin(None, dev, getattr(Models, plugin), 16, monkeypatch, " (MI355X)")


def test_local_trainer_takes_one_step_with_hip_conv(dev, lib, tmp_path, monkeypatch):
    cg.check_trainer(None, dev, tmp_path, monkeypatch)
