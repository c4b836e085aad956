"""The gfx950 build held to float64, not to the 1e-4 band: the regression gate of the search kernels (K1 rotation +
z-FFT, K2 slab correlation, K3 z-inverse + clip + MLP + mask), the stand-alone operators, the local path and the
convolution kernel.  tests/accuracy_checks.py states the yardstick and holds the check bodies; tests/test_accuracy_emu.py
runs them on the emulator.  The 1e-4 contract with the reference stays where it is (tests/test_gpu_parity.py).

Every kernel output X is compared with the oracle in float64 (X64) and must be no further from it than twice (RMS) /
three times (max) the oracle's own float32 evaluation (X32) is -- measured per case, inside the test.  Each check prints
its two ratios; EXPERIMENTS.md, section ACCURACY, holds the values of an MI355X.

Which case runs at which shape (two rotations per case unless stated -- the random filter / biting clip rows take one at
boxes 64 and 80 --; the float64 oracle on the host is what costs: the module takes about four minutes):

    case                               4 @ 32            48 @ 64   32 @ 40   16 @ 80   [16 @ 80, 32 @ 40]   48 @ 80
    a  dense, oblique                  3 launch forms    x         x         x         x, protein-shaped    x (one rotation)
       random filter / biting clip     x                 x         x         x         x
    b  impulses, volumes path          x                 x         x
    c  spectrally extreme ligands      x                 x                   x
    d  24 signed permutations          all, 4 launches   3         3         2         2
       ... through search()            all
    e  64 SOI rotations                search()                                        8
    f  mass on the faces               3 launch forms              x         x
    g  channels of unequal scale                         6 probes  8 probes

Nothing here reads the reference tree."""
import numpy as np
import pytest
import torch

import accuracy_checks as acc

pytestmark = pytest.mark.gpu

LAUNCHES = ({}, {"transposed": True}, {"quads": True}, {"transposed": True, "quads": True})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    import __graft_entry__ as entry
    entry.build()
    return torch.device("cuda:0")


# ---- section 3a: dense random volumes, oblique rotations --------------------------------------------------------------

@pytest.mark.parametrize("launch", ["default", "transposed", "quads"])
def test_dense_oblique_per_channel_k1(dev, launch):
    """4 @ 32 runs the per-channel K1, where slab orientation and the quad layout are reachable."""
    kw = {} if launch == "default" else {launch: True}
    sw = acc.check_dense(None, dev, 32, 4, seed=11, label=", " + launch, **kw).switches()
    assert sw["k1"] == "per_channel" and sw["k1_slab_orientation"] and sw["k1_quad_layout"]


@pytest.mark.parametrize("L,C,C1,nrot", [(64, 48, 0, 2), (40, 32, 0, 2), (80, 16, 0, 2), (80, 16, 32, 2), (80, 48, 0, 1)])
def test_dense_oblique_with_the_engines_own_switches(dev, L, C, C1, nrot):
    sw = acc.check_dense(None, dev, L, C, C1, nrot=nrot, seed=L + C).switches()
    assert sw["k1"] == "channels_last" and not sw["k3_unfused"]


def test_protein_shaped_ligand_picks_occupancy_and_pencil_maps(dev):
    """sparse_k1=None: the engine decides per ligand and grid -- on a mostly empty ligand it must go by occupancy maps on
    both grids and hand K2 the pencil map."""
    def expect(sw):
        occ = sw["k1_occupancy_maps"]
        assert sw["k1"] == "channels_last" and occ["fine"] and occ["coarse"], sw
        assert occ["k2_pencil_map"]["fine"] and occ["k2_pencil_map"]["coarse"], sw
    acc.check_dense(None, dev, 80, 16, 32, seed=13, protein=True, expect_switches=expect, engine_kw={"sparse_k1": None})


@pytest.mark.parametrize("L,C,C1,nrot", [(32, 4, 0, 2), (64, 48, 0, 1), (40, 32, 0, 2), (80, 16, 0, 1), (80, 16, 32, 1)])
def test_random_filter_and_biting_clip(dev, L, C, C1, nrot):
    acc.check_filter_and_clip(None, dev, L, C, C1, nrot=nrot, seed=14 + L)


# ---- 3b, 3c: structured inputs through the volumes path -----------------------------------------------------------------

@pytest.mark.parametrize("L,C", [(32, 4), (40, 32), (64, 48)])
def test_impulses_through_the_volumes_path(dev, L, C):
    acc.check_impulses(None, dev, L, C, seed=15 + L)


@pytest.mark.parametrize("L,C", [(32, 4), (64, 48), (80, 16)])
def test_spectrally_extreme_ligands(dev, L, C):
    acc.check_extreme_spectra(None, dev, L, C, seed=16 + L)


# ---- 3d: exact rotations through the fused K1 ---------------------------------------------------------------------------

def test_all_signed_permutations_through_the_per_channel_k1(dev):
    """Quads and both slab orientations, whatever search() would have picked for each matrix."""
    acc.check_exact_rotations(None, dev, 32, 4, which=range(24), seed=17, launches=LAUNCHES)


@pytest.mark.parametrize("L,C,C1,which", [(64, 48, 0, (2, 9, 20)), (40, 32, 0, (5, 12, 23)), (80, 16, 0, (7, 16)), (80, 16, 32, (3, 18))])
def test_signed_permutations_through_the_channels_last_k1(dev, L, C, C1, which):
    acc.check_exact_rotations(None, dev, L, C, which=which, seed=18 + L, C1=C1)


def test_signed_permutations_through_search(dev):
    """The 24 matrices sit on the ties of prefers_quads / prefers_transposed (|R02| = |R12| = 0 for a third of them): the
    grouping code of search() meets them, and the ranked list is the oracle's."""
    acc.check_rotation_list(None, dev, "4 @ 32, search(), 24 signed permutations", acc.signed_permutations(), seed=19)


# ---- 3e: the reference's own rotations ----------------------------------------------------------------------------------

def test_soi_rotations_through_search(dev, golden):
    """The 64 committed matrices of the reference's rotation sets (head and tail of the 20 / 15 / 12 / 10 degree files, which
    src/Utils/Rotations.py:47-66 of the reference reads): the heads hold the theta = 0 rows, nearly axis-aligned matrices with
    entries 1 - eps."""
    R = acc.soi_rotations(golden("g2_rotations.npz"))
    assert R.shape == (64, 3, 3) and float(np.abs(R[0]).max()) > 0.7
    acc.check_rotation_list(None, dev, "4 @ 32, search(), 64 SOI rotations", R, seed=20)


def test_soi_rotations_under_the_yardstick_at_the_reference_layout(dev, golden):
    """Eight of them (the first and the last of each set) at [16 @ 80, 32 @ 40] (src/Utils/Rotations.py:47-66)."""
    R = acc.soi_rotations(golden("g2_rotations.npz"))
    acc.check_rotations(None, dev, 80, 16, R[[0, 15, 16, 31, 32, 47, 48, 63]], "8 SOI rotations", C1=32, seed=21)


# ---- 3f, 3g -------------------------------------------------------------------------------------------------------------

def test_mass_on_the_faces_per_channel_k1(dev):
    acc.check_rotations(None, dev, 32, 4, acc.face_rotations(), "mass on the faces, 1e-4 / 1e-2 rad / quarter turn + 1e-4", seed=22,
                        ligand=acc.face_mass, launches=({}, {"quads": True}, {"transposed": True}))


@pytest.mark.parametrize("L,C", [(40, 32), (80, 16)])
def test_mass_on_the_faces_channels_last_k1(dev, L, C):
    acc.check_rotations(None, dev, L, C, acc.face_rotations(), "mass on the faces, 1e-4 / 1e-2 rad / quarter turn + 1e-4", seed=23 + L,
                        ligand=acc.face_mass)


@pytest.mark.parametrize("L,C,probed", [(40, 32, (0, 4, 9, 13, 18, 22, 27, 31)), (64, 48, (0, 9, 19, 28, 38, 47))])
def test_channels_of_unequal_scale(dev, L, C, probed):
    """Asserted: the yardstick on the errors pooled over the launch.  Reported only: the error of each probed channel
    relative to ITS largest correlation, beside the oracle's (parity section, says what the figures are)."""
    acc.check_unequal_scales(None, dev, L, C, probed, seed=24 + L)


# ---- section 4: stand-alone operators and the local path --------------------------------------------------------------

@pytest.mark.parametrize("L,C,embed", [(32, 3, True), (40, 3, True), (64, 2, True), (80, 2, True), (37, 2, True), (37, 2, False)])
def test_volume_convolution(dev, L, C, embed):
    """The compiled boxes, an embedded box (37 inside 40) and the plan-free transforms at the same box."""
    acc.check_volume_convolution(None, dev, L, C=C, embed=embed, seed=30 + L)


@pytest.mark.parametrize("L,C,inputs", [(65, 2, None), (84, 2, None), (127, 1, ("dense", "impulse ligand", "impulse x impulse")),
                                        (128, 1, ("dense", "impulse ligand", "impulse x impulse"))])
def test_volume_convolution_plan_free_above_64_kb_of_lds(dev, L, C, inputs):
    """The boxes that reach the plan-free route in normal use (81 .. 128; 65 .. 80 are embedded by default), where the tile of
    its middle-axis transform, (n_in * 64 + N) * 8 bytes, exceeds the 64 KB a kernel gets unasked: box 65 (N = 130, 67,600 B:
    the smallest, and N % 4 != 0 runs the k0 + u < N tail), 84 (N = 168), 127 (odd, N = 254), 128 (the largest box of the
    route, 133,120 B).  The yardstick and its formulation factor sqrt(N / log2 N) as check_volume_convolution derives them."""
    acc.check_volume_convolution(None, dev, L, C=C, embed=False, seed=30 + L, inputs=inputs)


def test_volume_convolution_plan_free_chunks_at_box_128(dev):
    acc.check_plan_free_chunks(None, dev, 128, 12, seed=31)


def test_volume_convolution_plan_free_clamp_bites(dev):
    acc.check_plan_free_clamp(None, dev, 84, 2, seed=32)


@pytest.mark.parametrize("L,C", [(32, 3), (80, 2), (127, 1)])
def test_volume_rotation(dev, L, C):
    acc.check_volume_rotation(None, dev, L, C=C, seed=40 + L)


@pytest.mark.parametrize("L,C", [(40, 4), (80, 2)])
def test_local_window_of_an_impulse_is_the_receptor(dev, L, C):
    acc.check_local_window_is_the_receptor(None, dev, L, C, seed=50 + L)


# ---- section 5: the convolution kernel --------------------------------------------------------------------------------

PLUGIN_SHAPES = [(11, 16, 5, 80), (16, 16, 3, 80), (16, 32, 5, 40), (32, 32, 3, 40), (11, 32, 3, 37), (32, 64, 5, 40), (11, 48, 3, 21)]


@pytest.mark.parametrize("precision", ["f32", "split_bf16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout,ks,D", PLUGIN_SHAPES)
def test_conv3d_impulse_response(dev, cin, cout, ks, D, stride, precision):
    acc.check_conv3d_impulse_response(None, dev, cin, cout, ks, D, stride, precision, seed=cin + D)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout,ks,D", PLUGIN_SHAPES)
def test_conv3d_under_the_yardstick(dev, cin, cout, ks, D, stride):
    acc.check_conv3d_yardstick(None, dev, cin, cout, ks, D, stride, seed=cin + D)
