"""The convolution's backward on the CPU-emulated kernel library: the weight-gradient kernel (csrc/dlpd_conv_grad.h) against
float64, its index arithmetic, its determinism and its errors; the input gradient by the forward kernel; the autograd
Function; both plugins with ``hip_autograd``; the trainer's switch.  Check bodies: tests/conv_grad_checks.py."""
import inspect

import pytest
import torch

import conv_grad_checks as cg


@pytest.mark.parametrize("B,cin,cout,ks,D,nparts", cg.SMALL_CASES)
def test_weight_grad_matches_float64(emu, B, cin, cout, ks, D, nparts):
    cg.check_weight_grad(emu, "cpu", B, cin, cout, ks, D, nparts, " (emulated)")


@pytest.mark.parametrize("ks", [3, 5])
@pytest.mark.parametrize("far", [False, True])
def test_weight_grad_index_exactness(emu, ks, far):
    cg.check_index_exactness(emu, "cpu", ks, far)


def test_weight_grad_is_deterministic(emu):
    cg.check_determinism(emu, "cpu", 1, 32, 32, 3, 6, 7, 3)


def test_weight_grad_errors(emu):
    from deeplocalproteindocking_amd import ops
    x = torch.zeros(2 * 16 * 6 ** 3)
    p = x.data_ptr()

    def call(gw=p, B=1, cin=16, cout=16, D=6, ks=3, nparts=2):
        return emu.call("dlpd_conv3d_wgrad", p, p, gw, p, B, cin, cout, D, ks, nparts, 0)
    assert emu.call("dlpd_conv3d_wgrad_ws_floats", 11, 16, 5, 7) == 7 * 16 * 11 * 125
    with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
        call(gw=None)
    with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
        call(nparts=0)
    with pytest.raises(RuntimeError, match="DLPD_ERR_ARG"):
        call(B=0)
    for bad in (dict(ks=4), dict(cout=8), dict(D=81)):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            call(**bad)
    with pytest.raises(RuntimeError, match="has no HIP kernel"):
        ops.conv3d_weight_grad(torch.zeros(1, 4, 6, 6, 6), torch.zeros(1, 8, 6, 6, 6), 3, lib=emu)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.conv3d_weight_grad(torch.zeros(1, 4, 6, 6, 6), torch.zeros(2, 16, 6, 6, 6), 3, lib=emu)
    with pytest.raises(RuntimeError, match="has no HIP kernel"):
        ops.conv3d_autograd(torch.zeros(1, 4, 6, 6, 6, requires_grad=True), torch.zeros(8, 4, 3, 3, 3), lib=emu)


@pytest.mark.parametrize("precision", ["f32", "split_bf16"])
@pytest.mark.parametrize("B,cin,cout,ks,D", [(2, 16, 16, 3, 9), (1, 32, 16, 5, 7)])
def test_input_grad_matches_float64(emu, B, cin, cout, ks, D, precision):
    cg.check_input_grad(emu, "cpu", B, cin, cout, ks, D, precision)


def test_input_grad_refuses_a_layer_of_11_channels(emu, monkeypatch):
    cg.check_input_grad_refuses(emu, "cpu", monkeypatch)


@pytest.mark.parametrize("relu", [False, True])
def test_conv3d_autograd_follows_float64(emu, relu):
    cg.check_function(emu, "cpu", relu)


@pytest.mark.parametrize("plugin,precision", [("E3MultiResRepr4x4", None), ("SE3MultiResReprScalar", "split_bf16")])
def test_plugin_trains_on_the_kernels(emu, monkeypatch, plugin, precision):
    """E3 at the default arithmetic of the training path (``ops.CONV_GRAD_PRECISION``: exact f32).  SE3 -- eight 5^3 layers,
    whose emulated time is their number of matrix instructions -- with the forward and the input gradient at split_bf16, a
    third of them; its default is what the device test runs."""
    from deeplocalproteindocking_amd import Models, ops
    assert ops.CONV_GRAD_PRECISION == "f32"
    if precision is not None:
        monkeypatch.setattr(ops, "CONV_GRAD_PRECISION", precision)
    cg.check_plugin(emu, "cpu", getattr(Models, plugin), 8, monkeypatch, " (emulated)")


def test_trainer_switch_sets_the_plugins_and_defaults_stay(emu):
    """LocalTrainer(hip_conv=True) sets ``hip_autograd`` on a representation that has it; every default is off.  (The step
    itself runs on the device: tests/test_conv_grad_gpu.py.)"""
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd.Models import (BatchRankingLoss, E3MultiResRepr4x4, LocalDockingModel, SE3MultiResReprScalar,
                                                    SimpleFilter)
    from deeplocalproteindocking_amd.Models.ProteinRepresentationModels import IsotropicConv3d
    from deeplocalproteindocking_amd.Training import LocalTrainer
    assert inspect.signature(LocalTrainer.__init__).parameters["hip_conv"].default is False
    assert E3MultiResRepr4x4.hip_autograd is False and SE3MultiResReprScalar.hip_autograd is False and IsotropicConv3d.hip_autograd is False
    assert ops.CONV_WGRAD_PARTS == 256
    for cls in (E3MultiResRepr4x4, SE3MultiResReprScalar):
        for hip in (False, True):
            net = cls(multiplier=1)
            model = LocalDockingModel(representation=net, filter=SimpleFilter(net.get_num_outputs()), lib=emu)
            LocalTrainer(model, BatchRankingLoss(), box_size=16, lib=emu, hip_conv=hip)
            assert net.hip_autograd is hip and cls.hip_autograd is False

    class NoSwitch(torch.nn.Module):
        def get_num_outputs(self):
            return [2]
    stub = NoSwitch()
    LocalTrainer(LocalDockingModel(representation=stub, filter=SimpleFilter([2]), lib=emu), BatchRankingLoss(), lib=emu, hip_conv=True)
    assert not hasattr(stub, "hip_autograd")
