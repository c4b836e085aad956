"""Differentiable local docking on the real gfx950 build: the adjoint kernel of the local correlation at the reference's
shapes against float64, the batching of a long pose list, the differentiable LocalDockingModel's parameter gradients against
pure torch on the device, and one LocalTrainer step.  Check bodies and tolerances: tests/local_grad_checks.py.  Nothing here
reads the reference tree."""
import numpy as np
import pytest
import torch

import local_grad_checks as lg

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


# (L, C, r, P, shared, want, rotate): the reference's two resolutions, a box that is no multiple of anything (33: XT = 7,
# three chunks of rows, the last of one row) with one volume set for all poses at the widest window, the largest box, and
# the rotated ligand
@pytest.mark.parametrize("L,C,r,P,shared,want,rotate", [
    (80, 16, 0, 4, False, ("rec", "lig"), False),
    (40, 32, 1, 4, False, ("rec", "lig"), False),
    (33, 3, 3, 3, True, ("rec", "lig"), False),
    (128, 1, 0, 2, False, ("rec", "lig"), False),
    (40, 4, 2, 3, False, ("rec",), True),
])
def test_local_correlate_grad_matches_float64(dev, lib, L, C, r, P, shared, want, rotate):
    lg.check_kernel(lib, dev, L, C, r, P, scale=2 if L == 40 else 1, mode="trunc", shared=shared, want=want, rotate=rotate)


def _grads(ops, rec, lig, T, gout, lib=None):
    a, b = rec.clone().requires_grad_(), lig.clone().requires_grad_()
    ops.local_correlate(a, b, T, radius=0, lib=lib).backward(gout)
    return a.grad, b.grad


def test_local_correlate_backward_batches_a_list_beyond_the_launch_grid_limit(dev, lib):
    """More poses than one launch can hold (2^24 - 1 blocks), per-pose volumes: the backward splits the list as the forward
    does; the poses behind the split get the bits of a call of their own."""
    from deeplocalproteindocking_amd import ops
    L, C = 8, 1
    most = lib.call("dlpd_local_max_poses", C, L)
    P = most + 5
    need = 4 * P * C * L ** 3 * 4                       # receptor, ligand and their two gradients
    if need > 4 << 30:
        reason = "%d poses of %d @ %d^3 with their gradients take %.1f GB (> 4 GB)" % (P, C, L, need / 2.0 ** 30)
        print(reason)
        pytest.skip(reason)
    g_ = torch.Generator().manual_seed(1)
    rec, lig = torch.randn(P, C, L, L, L, generator=g_).to(dev), torch.randn(P, C, L, L, L, generator=g_).to(dev)
    T = torch.randint(-2, 3, (P, 3), generator=g_).int().to(dev)
    gout = torch.randn(P, C, 1, 1, 1, generator=g_).to(dev)
    ga, gb = _grads(ops, rec, lig, T, gout)
    ta, tb = _grads(ops, rec[-16:].contiguous(), lig[-16:].contiguous(), T[-16:].contiguous(), gout[-16:].contiguous())
    assert ga[-16:].cpu().numpy().tobytes() == ta.cpu().numpy().tobytes()
    assert gb[-16:].cpu().numpy().tobytes() == tb.cpu().numpy().tobytes()


def test_local_correlate_backward_splits_at_the_limit_the_library_states(dev, lib):
    """The same property at a size that always fits (the check's docstring)."""
    lg.check_backward_split(lib, dev)


def test_differentiable_model_gradients_follow_float64_on_the_device(dev):
    from deeplocalproteindocking_amd.Models import E3MultiResRepr4x4, LocalDockingModel, SimpleFilter
    torch.manual_seed(17)
    net = E3MultiResRepr4x4(multiplier=1)
    filt = SimpleFilter(net.get_num_outputs())
    with torch.no_grad():
        filt.fc[0].bias.normal_(0.0, 0.3)
    B, L = 4, 32
    g_ = torch.Generator().manual_seed(18)
    rec, lig = torch.rand(B, 11, L, L, L, generator=g_), torch.rand(B, 11, L, L, L, generator=g_)
    T = torch.tensor([[0.0, 0.0, 0.0], [-3.0, 5.0, -1.0], [2.5, -4.75, 1.25], [-7.0, -5.0, 3.0]])
    model = LocalDockingModel(net, filt, differentiable=True)
    out, out64 = lg.check_model_gradients("LocalDockingModel 11 @ 32, B = 4 (MI355X)", model, rec, lig, T, device=dev)
    assert out.shape == (B, 1) and float((out.double() - out64).abs().max()) <= 1e-4 * float(out64.abs().max())


def test_local_trainer_takes_one_step_on_the_device(dev, tmp_path):
    from test_atoms import write_fake_pdb
    from deeplocalproteindocking_amd.Models import BatchRankingLoss, LocalDockingModel, SimpleFilter
    from deeplocalproteindocking_amd.Training import LocalTrainer
    torch.manual_seed(11)
    stub = lg.TwoResolutionStub()
    model = LocalDockingModel(representation=stub, filter=SimpleFilter(stub.get_num_outputs())).to(dev)
    with torch.no_grad():
        model.filter.fc[0].bias.fill_(0.5)
        model.filter.fc[0].weight.abs_()
    recs, ligs = [], []
    for i in range(4):
        recs.append(str(tmp_path / ("r%d.pdb" % i)))
        ligs.append(str(tmp_path / ("l%d.pdb" % i)))
        write_fake_pdb(recs[-1], 10 + i, 20 + i)
        write_fake_pdb(ligs[-1], 7 + i, 30 + i)
    trainer = LocalTrainer(model, BatchRankingLoss(), lr=0.01, box_size=16, resolution=2.0, randomize_rot=True, rotation_seed=3)
    before = [p.detach().clone() for p in (model.filter.fc[0].weight, model.filter.fc[2].weight)]
    loss = trainer.optimize((recs, ligs, torch.tensor([0.1, 0.9, 0.5, 0.3])))
    assert np.isfinite(loss) and loss > 0 and model.differentiable is True
    assert not torch.equal(model.filter.fc[0].weight.detach(), before[0]) and not torch.equal(model.filter.fc[2].weight.detach(), before[1])
    assert bool(torch.isfinite(model.filter.fc[0].weight).all()) and bool(torch.isfinite(stub.conv.weight).all())
