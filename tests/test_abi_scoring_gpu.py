"""The scoring entry points of include/dlpd.h that DockingEngine and ops bypass, on the real gfx950 build: K3 with raw coarse
channels (aux_is_preact = 0) at boxes 32 and 40 -- and at box 64 in the variants library, where that form exists --,
dlpd_filter_preact and its two consumers, the one-call driver dlpd_score_rotations / dlpd_score_rotations_oriented at boxes 32,
40 and 64, and the two-resolution layout [C @ 64, C1 @ 32] through the engine (the product's only MODE 2 instantiation of the
channel-owning K3, and the role-split K3 at box 64 taking pre-activation planes).  Check bodies and tolerances:
tests/abi_scoring_checks.py, tests/accuracy_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import abi_scoring_checks as ab
import accuracy_checks as acc

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


@pytest.fixture(scope="module")
def variants(dev):
    """tests/variants/libdlpd_variants.so: the channel-owning K3 (and with it the raw-aux branch) at boxes 64 and 80."""
    import __graft_entry__ as entry
    from deeplocalproteindocking_amd._lib import DlpdLib
    return DlpdLib(entry.build_test_variants())


# 1. K3 with raw coarse channels ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Caux", ab.AUX_CHANNELS)
@pytest.mark.parametrize("L", [32, 40])
def test_k3_raw_aux_reads_the_coarse_parent_of_every_voxel(dev, lib, L, Caux):
    ab.check_raw_aux_index_exact(lib, dev, L, Caux)


@pytest.mark.parametrize("has_clash", [0, 1])
@pytest.mark.parametrize("Caux", ab.AUX_CHANNELS)
@pytest.mark.parametrize("L", [32, 40])
def test_k3_raw_aux_follows_float64(dev, lib, L, Caux, has_clash):
    ab.check_raw_aux_yardstick(lib, dev, L, Caux, has_clash)


def test_k3_raw_aux_three_spellings_give_equal_bits(dev, lib):
    ab.check_raw_aux_spellings(lib, dev)


def test_k3_raw_aux_refusals(dev, lib, variants):
    ab.check_raw_aux_refusals(variants, lib, dev)


def test_k3_raw_aux_at_box_64_reads_the_coarse_parent_of_every_voxel(dev, variants):
    ab.check_raw_aux_index_exact(variants, dev, 64, 5)


def test_k3_raw_aux_at_box_64_follows_float64(dev, variants):
    ab.check_raw_aux_yardstick(variants, dev, 64, 5, 1)


# 2. dlpd_filter_preact and its consumers ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ab.PREACT_SHAPES)
def test_filter_preact_equals_float64_on_dyadic_inputs(dev, lib, shape):
    ab.check_preact_exact(lib, dev, shape)


@pytest.mark.parametrize("shape", ab.PREACT_SHAPES)
def test_filter_preact_follows_float64(dev, lib, shape):
    ab.check_preact_random(lib, dev, shape)


def test_filter_preact_every_compiled_hidden_width(dev, lib):
    for HP in ab.hidden_table(lib):
        ab.check_preact_exact(lib, dev, (2, 5, 8, HP))
        ab.check_preact_random(lib, dev, (2, 5, 8, HP))


def test_filter_preact_refusals(dev, lib):
    ab.check_preact_refusals(lib, dev)


@pytest.mark.parametrize("N0,N1", [(16, 8), (12, 12)])
def test_filter_volumes_takes_the_planes_of_filter_preact(dev, lib, N0, N1):
    ab.check_filter_volumes_preact(lib, dev, N0, N1)


def test_filter_volumes_refuses_planes_at_a_quarter_of_the_grid(dev, lib):
    ab.check_filter_volumes_preact_refusal(lib, dev)


@pytest.mark.parametrize("Caux", ab.AUX_CHANNELS)
@pytest.mark.parametrize("L", [32, 40])
def test_k3_takes_the_planes_of_filter_preact(dev, lib, L, Caux):
    ab.check_k3_preact_from_filter_preact(lib, dev, L, Caux, 1)


# 3. the one-call driver --------------------------------------------------------------------------------------------------

def test_score_rotations_equals_its_stages_and_follows_float64(dev, lib):
    ab.check_driver_box32(lib, dev)


def test_score_rotations_box_40_follows_float64(dev, lib):
    ab.check_driver_yardstick(lib, dev, 40, 3, False, 1)


def test_score_rotations_box_64_follows_float64(dev, lib):
    ab.check_driver_yardstick(lib, dev, 64, 2, True, 1)


def test_score_rotations_propagates_errors(dev, lib):
    ab.check_driver_errors(lib, dev)


# 5. [C @ 64, C1 @ 32] ----------------------------------------------------------------------------------------------------

def test_two_resolutions_64_and_32_dense_probe(dev, lib):
    sw = acc.check_dense(None, dev, 64, 4, 6, nrot=1, seed=81).switches()
    assert sw["k1"] and not sw["k3_unfused"], sw


def test_two_resolutions_64_and_32_filter_and_clip(dev, lib):
    acc.check_filter_and_clip(None, dev, 64, 4, 6, nrot=1, seed=82)
