"""K1 gathering from the chunk-major ligand copy, on the emulated kernels: the layout itself, the spectra against the
channels-last source bit for bit (dense with an embedded extent, by occupancy maps, into a wider workspace), the engine."""
import pytest

import k1_chunk_layout_checks as chk


@pytest.mark.parametrize("C", [8, 12, 20])
def test_chunk_major_copy_layout(emu, C):
    """L = 32 (16-channel chunks): less than one chunk, a partly filled chunk, two chunks."""
    chk.check_layout(emu, "cpu", 32, C)


@pytest.mark.parametrize("C", [8, 20])
def test_k1_from_chunks_equals_channels_last_with_extent(emu, C):
    chk.check_k1_equality(emu, "cpu", 32, C, chk.rotations("oblique", 3), extent=24)


@pytest.mark.parametrize("C", [8, 20])
def test_k1_from_chunks_equals_channels_last_by_occupancy_maps(emu, C):
    chk.check_k1_equality(emu, "cpu", 32, C, chk.rotations("oblique", 3), occupancy=True)


@pytest.mark.parametrize("C", [8, 20])
def test_k1_from_chunks_equals_channels_last_into_a_wider_workspace(emu, C):
    chk.check_k1_equality(emu, "cpu", 32, C, chk.rotations("oblique", 3), c_base=3, extra=2)


def test_engine_lists_do_not_depend_on_the_k1_source_layout(emu):
    """Box 32, 8 channels, 32 rotations, both layouts.  The emulator spends about 3.5 s per rotation in K2 and K3, which both
    searches run in full: minutes here, 0.03 s on the device (test_k1_chunk_layout_gpu.py)."""
    chk.check_engine_lists(emu, "cpu")
