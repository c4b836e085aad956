"""CPU twin of tests/test_gpu_accuracy.py: the check bodies of tests/accuracy_checks.py (float64 yardstick, probe filter,
structured inputs) on the fibre emulator, at boxes 32 / 40 with up to 8 channels.  The emulator runs the kernel sources'
index logic and arithmetic, not the packed-FMA assembly, LDS-DMA loads or wave scheduling of the gfx950 build: this file
is what a change can be checked against without a GPU, and what the mutation checks of the kernels were made on."""
import numpy as np
import pytest
import torch

import accuracy_checks as acc
from oracle import docking_oracle as orc

CPU = "cpu"


def test_oracle_features_are_the_rows_score_volumes_filters():
    """accuracy_checks.oracle_features + filter_mlp == oracle.score_volumes, bit for bit, in both precisions and on the
    two-resolution layout: the helper only lets several filters share one set of correlations."""
    g = torch.Generator().manual_seed(3)
    rec, lig = [torch.randn(3, 8, 8, 8, generator=g), torch.randn(2, 4, 4, 4, generator=g)], \
        [torch.randn(3, 8, 8, 8, generator=g), torch.randn(2, 4, 4, 4, generator=g)]
    filt = acc.random_filter(5, 3, 1, dead=1)
    for dtype in (torch.float32, torch.float64):
        want = orc.score_volumes([r[None] for r in rec], [l[None] for l in lig], *filt, clip=0.7, dtype=dtype)[0].reshape(-1)
        assert torch.equal(acc.oracle_scores(acc.oracle_features(rec, lig, 0.7, dtype), filt, dtype), want)


def test_probe_filter_reads_the_clamped_correlations_exactly():
    """relu(x) - relu(-x) = x: through the oracle's own MLP the probe returns sum_c w_c clamp(corr_c) to the last bit of a
    float32 sum, and every probed channel at full weight."""
    g = torch.Generator().manual_seed(4)
    feat = torch.randn(1000, 6, generator=g)
    for W1, b1, W2, b2 in acc.probe_filters(6, width=4, signs=2, seed=1):
        w = W2[0, :4]
        S = [int(torch.nonzero(W1[j])[0]) for j in range(4)]
        assert torch.equal(W2[0, 4:], -w) and set(w.tolist()) <= {1.0, -1.0}
        want = (feat[:, S].double() * w.double()).sum(dim=1)
        assert float((orc.filter_mlp(feat, W1, b1, W2, b2)[:, 0].double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(feat.abs().max()) * 4
    W1, b1, W2, b2 = acc.single_channel_probe(6, 2)
    assert torch.equal(orc.filter_mlp(feat, W1, b1, W2, b2)[:, 0], feat[:, 2])


def test_signed_permutations_and_their_index_arithmetic():
    P = acc.signed_permutations()
    assert len({tuple(p.reshape(-1)) for p in P}) == 24 and all(abs(np.linalg.det(p) - 1) < 1e-12 for p in P)
    v = torch.randn(2, 6, 6, 6, generator=torch.Generator().manual_seed(1))
    for p in P:
        Rb = torch.from_numpy(p[None])
        assert torch.equal(orc.rotate_volume(v[None], Rb, dtype=torch.float64)[0].float(), acc.permuted(v, p))
    assert torch.equal(acc.permuted(v, np.eye(3)), v)


# ---- section 3: the fused engine --------------------------------------------------------------------------------------

@pytest.mark.parametrize("launch", ["default", "transposed", "quads"])
def test_dense_oblique_per_channel_k1(emu, launch):
    kw = {} if launch == "default" else {launch: True}
    eng = acc.check_dense(emu, CPU, 32, 4, seed=11, label=", " + launch, engine_kw={"channels_last": False}, **kw)
    sw = eng.switches()
    assert sw["k1"] == "per_channel" and sw["k1_slab_orientation"] and sw["k1_quad_layout"]


def test_dense_oblique_channels_last_box_40(emu):
    eng = acc.check_dense(emu, CPU, 40, 8, nrot=1, seed=12)
    assert eng.switches()["k1"] == "channels_last"


def test_protein_shaped_ligand_picks_occupancy_and_pencil_maps(emu):
    def expect(sw):
        assert sw["k1"] == "channels_last" and sw["k1_occupancy_maps"]["fine"] and sw["k1_occupancy_maps"]["k2_pencil_map"]["fine"]
    acc.check_dense(emu, CPU, 40, 8, nrot=1, seed=13, protein=True, expect_switches=expect, engine_kw={"sparse_k1": None})


def test_random_filter_and_biting_clip(emu):
    acc.check_filter_and_clip(emu, CPU, 32, 4, nrot=1, seed=14)


def test_impulses_through_the_volumes_path(emu):
    acc.check_impulses(emu, CPU, 32, 4, seed=15)


def test_spectrally_extreme_ligands(emu):
    acc.check_extreme_spectra(emu, CPU, 32, 4, seed=16)


def test_exact_rotations_through_the_per_channel_k1(emu):
    acc.check_exact_rotations(emu, CPU, 32, 4, which=(8, 21), seed=17, engine_kw={"channels_last": False},
                              launches=({}, {"transposed": True}, {"quads": True}))


def test_exact_rotations_through_the_channels_last_k1(emu):
    acc.check_exact_rotations(emu, CPU, 40, 8, which=(19,), seed=18)


def test_signed_permutations_through_search(emu):
    """Ties of prefers_quads / prefers_transposed (|R02| = |R12| = 0 for a third of them): the grouping code meets them."""
    acc.check_rotation_list(emu, CPU, "4 @ 32, search(), 6 signed permutations", acc.signed_permutations()[::4], seed=19)


def test_soi_rotations_through_search(emu, golden):
    """The theta = 0 rows at the head of the reference's rotation sets (src/Utils/Rotations.py:47-66 reads them from the
    .eul files): nearly axis-aligned matrices with entries 1 - eps.  The emulator takes four of the head of the 20-degree set."""
    R = acc.soi_rotations(golden("g2_rotations.npz"))
    assert R.shape == (64, 3, 3)
    acc.check_rotation_list(emu, CPU, "4 @ 32, search(), head of the 20-degree SOI set", R[[0, 1, 2, 7]], seed=20)


def test_soi_rotations_under_the_yardstick(emu, golden):
    R = acc.soi_rotations(golden("g2_rotations.npz"))
    acc.check_rotations(emu, CPU, 32, 4, R[[0, 63]], "SOI rotations (first, last)", seed=21)


def test_mass_on_the_faces_of_the_box(emu):
    acc.check_rotations(emu, CPU, 32, 4, acc.face_rotations(), "mass on the faces, 1e-4 / 1e-2 rad / quarter turn + 1e-4",
                        seed=22, ligand=acc.face_mass, engine_kw={"channels_last": False}, launches=({}, {"quads": True}))


def test_mass_on_the_faces_channels_last(emu):
    acc.check_rotations(emu, CPU, 32, 8, acc.face_rotations()[[0, 2]], "mass on the faces, 1e-4 rad / quarter turn + 1e-4", seed=23,
                        ligand=acc.face_mass)


def test_channels_of_unequal_scale(emu):
    acc.check_unequal_scales(emu, CPU, 32, 8, probed=(0, 3, 5, 7), seed=24)


# ---- section 4: stand-alone operators and the local path --------------------------------------------------------------

@pytest.mark.parametrize("L,embed", [(32, True), (40, True), (37, True), (10, False)])
def test_volume_convolution(emu, L, embed):
    acc.check_volume_convolution(emu, CPU, L, C=2 if L > 10 else 3, embed=embed, seed=30 + L)


def test_volume_convolution_plan_free_clamp_bites(emu):
    """The body of the device's check at box 84, on the emulator at box 10."""
    acc.check_plan_free_clamp(emu, CPU, 10, 2, seed=32)


@pytest.mark.parametrize("L", [10, 32])
def test_volume_rotation(emu, L):
    acc.check_volume_rotation(emu, CPU, L, C=2, seed=40 + L)


def test_local_window_of_an_impulse_is_the_receptor(emu):
    acc.check_local_window_is_the_receptor(emu, CPU, 12, 3, seed=50)


# ---- section 5: the convolution kernel --------------------------------------------------------------------------------

# (cin, cout, k, D, which of accuracy_checks.conv_positions): the emulated matrix cores cost about ten seconds per item
CONV_SHAPES = [(11, 16, 5, 6, (0, 1, 4, 8)), (16, 32, 3, 9, (0, 1, 5, 9)), (8, 16, 3, 21, (8, 9)), (8, 16, 5, 7, (1, 3, 6))]


@pytest.mark.parametrize("precision", ["f32", "split_bf16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout,ks,D,positions", CONV_SHAPES)
def test_conv3d_impulse_response(emu, cin, cout, ks, D, positions, stride, precision):
    acc.check_conv3d_impulse_response(emu, CPU, cin, cout, ks, D, stride, precision, seed=cin + D, positions=positions)


@pytest.mark.parametrize("cin,cout,ks,D,stride", [(11, 16, 5, 6, 1), (16, 32, 3, 9, 1), (8, 16, 5, 7, 2)])
def test_conv3d_under_the_yardstick(emu, cin, cout, ks, D, stride):
    acc.check_conv3d_yardstick(emu, CPU, cin, cout, ks, D, stride, seed=cin + D)
