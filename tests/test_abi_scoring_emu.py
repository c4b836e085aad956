"""The scoring entry points of include/dlpd.h that DockingEngine and ops bypass, on the CPU-emulated kernel library: K3 with raw
coarse channels (aux_is_preact = 0) at boxes 32 and 40, dlpd_filter_preact and its two consumers, and the one-call driver
dlpd_score_rotations / dlpd_score_rotations_oriented.  Check bodies and tolerances: tests/abi_scoring_checks.py."""
import os
import sys

import pytest

import abi_scoring_checks as ab


@pytest.fixture(scope="module")
def emu_product():
    """The emulated library as libdlpd.so compiles it (no -DDLPD_TEST_VARIANTS): the dispatch tables of the product."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import build_emu
    from deeplocalproteindocking_amd._lib import DlpdLib
    return DlpdLib(build_emu.build(variants=False))


# 1. K3 with raw coarse channels ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Caux", ab.AUX_CHANNELS)
@pytest.mark.parametrize("L", [32, 40])
def test_k3_raw_aux_reads_the_coarse_parent_of_every_voxel(emu, L, Caux):
    ab.check_raw_aux_index_exact(emu, "cpu", L, Caux)


@pytest.mark.parametrize("has_clash", [0, 1])
@pytest.mark.parametrize("Caux", ab.AUX_CHANNELS)
@pytest.mark.parametrize("L", [32, 40])
def test_k3_raw_aux_follows_float64(emu, L, Caux, has_clash):
    ab.check_raw_aux_yardstick(emu, "cpu", L, Caux, has_clash)


def test_k3_raw_aux_three_spellings_give_equal_bits(emu):
    ab.check_raw_aux_spellings(emu, "cpu")


def test_k3_raw_aux_refusals(emu, emu_product):
    ab.check_raw_aux_refusals(emu, emu_product, "cpu")


# 2. dlpd_filter_preact and its consumers ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ab.PREACT_SHAPES)
def test_filter_preact_equals_float64_on_dyadic_inputs(emu, shape):
    ab.check_preact_exact(emu, "cpu", shape)


@pytest.mark.parametrize("shape", ab.PREACT_SHAPES)
def test_filter_preact_follows_float64(emu, shape):
    ab.check_preact_random(emu, "cpu", shape)


def test_filter_preact_every_compiled_hidden_width(emu):
    for HP in ab.hidden_table(emu):
        ab.check_preact_exact(emu, "cpu", (2, 5, 8, HP))
        ab.check_preact_random(emu, "cpu", (2, 5, 8, HP))


def test_filter_preact_refusals(emu):
    ab.check_preact_refusals(emu, "cpu")


@pytest.mark.parametrize("N0,N1", [(16, 8), (12, 12)])
def test_filter_volumes_takes_the_planes_of_filter_preact(emu, N0, N1):
    ab.check_filter_volumes_preact(emu, "cpu", N0, N1)


def test_filter_volumes_refuses_planes_at_a_quarter_of_the_grid(emu):
    ab.check_filter_volumes_preact_refusal(emu, "cpu")


@pytest.mark.parametrize("Caux", ab.AUX_CHANNELS)
@pytest.mark.parametrize("L", [32, 40])
def test_k3_takes_the_planes_of_filter_preact(emu, L, Caux):
    ab.check_k3_preact_from_filter_preact(emu, "cpu", L, Caux, 1)


# 3. the one-call driver --------------------------------------------------------------------------------------------------

def test_score_rotations_equals_its_stages_and_follows_float64(emu):
    ab.check_driver_box32(emu, "cpu")


def test_score_rotations_box_40_follows_float64(emu):
    ab.check_driver_yardstick(emu, "cpu", 40, 3, False, 1)


def test_score_rotations_propagates_errors(emu):
    ab.check_driver_errors(emu, "cpu")
