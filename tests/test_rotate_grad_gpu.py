"""The differentiable VolumeRotation on the real gfx950 build: the adjoint kernel of the trilinear rotation against the
float64 scatter and the forward kernel, its exact cases, chunking, errors, the autograd surface, ops.local_correlate_rotated
and LocalDockingModel.forward_poses against pure torch on the device.  Check bodies and tolerances:
tests/rotate_grad_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import local_grad_checks as lg
import rotate_grad_checks as rg

pytestmark = pytest.mark.gpu

CC = 16                  # DLPD_ROT_GRAD_CC: the channels a thread carries


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


# (L, C, B, summed): a box that is no multiple of anything, summed over the rotations; one channel more than a chunk; the
# reference's fine grid with a gradient per batch entry; the largest box
SHAPES = [(33, 3, 4, True), (40, CC + 1, 3, True), (80, 2, 2, False), (128, 1, 1, False)]


@pytest.mark.parametrize("L,C,B,summed", SHAPES)
def test_rotate_grad_matches_the_float64_scatter(dev, lib, L, C, B, summed):
    rg.check_kernel(lib, dev, L, C, B, summed)


@pytest.mark.parametrize("L,C,B,summed", SHAPES)
def test_rotate_grad_is_the_transpose_of_the_forward_kernel(dev, lib, L, C, B, summed):
    rg.check_transpose(lib, dev, L, C, B, summed)


def test_rotate_grad_exact_cases(dev, lib):
    rg.check_exact(lib, dev, 33)


def test_rotate_grad_of_a_singular_map_walks_the_whole_box(dev, lib):
    rg.check_singular(lib, dev)


def test_rotate_grad_accumulate_continues_the_sum(dev, lib):
    rg.check_accumulate(lib, dev, L=33)


def test_local_correlate_rotated_backward_splits_at_the_limit_the_library_states(dev, lib):
    rg.check_backward_split(lib, dev)


def test_rotate_grad_errors(dev, lib):
    rg.check_errors(lib, dev)


def test_volume_rotation_autograd(dev, lib):
    rg.check_volume_rotation_autograd(lib, dev, L=33)


def test_local_correlate_rotated(dev, lib):
    rg.check_local_correlate_rotated(lib, dev, 40, 4, 3, 2, 2, "floor", True)
    rg.check_local_correlate_rotated(lib, dev, 40, 4, 3, 2, 1, "trunc", False)


def test_forward_poses_gradients_follow_float64_on_the_device(dev, monkeypatch):
    """multiplier=1: layers of 2 and 4 channels, for which there is no HIP convolution kernel (output channels a multiple of
    16).  Under autograd the representation is plain torch anyway; for the no_grad comparison at the end of the check it is
    told to run on torch too (DLPD_ALLOW_TORCH_CONV=1, the documented switch; without it that call raises) -- what is compared
    is forward_poses, the correlation through the rotations and the filter, not the convolutions."""
    from deeplocalproteindocking_amd.Models import E3MultiResRepr4x4, LocalDockingModel, SimpleFilter
    monkeypatch.setenv("DLPD_ALLOW_TORCH_CONV", "1")
    torch.manual_seed(17)
    net = E3MultiResRepr4x4(multiplier=1)
    filt = SimpleFilter(net.get_num_outputs())
    with torch.no_grad():
        filt.fc[0].bias.normal_(0.0, 0.3)
    P, L = 4, 32
    g_ = torch.Generator().manual_seed(18)
    rec, lig = torch.rand(1, 11, L, L, L, generator=g_), torch.rand(1, 11, L, L, L, generator=g_)
    R = torch.from_numpy(lg.rots(P, seed=6)).float().contiguous()
    T = torch.tensor([[0.0, 0.0, 0.0], [-3.0, 5.0, -1.0], [2.5, -4.75, 1.25], [-7.0, -5.0, 3.0]])
    model = LocalDockingModel(net, filt, differentiable=True)
    out, out64 = rg.check_model_pose_gradients("forward_poses 11 @ 32, P = 4 (MI355X)", model, rec, lig, R, T, device=dev)
    assert out.shape == (P, 1) and float((out.double() - out64).abs().max()) <= 1e-4 * float(out64.abs().max())
