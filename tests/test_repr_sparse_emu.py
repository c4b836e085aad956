"""The tile-occupancy path of the representation stage at lopsided per-entry maps -- the emulator leg.  Check bodies, the
support family and what each case asserts on its own inputs: tests/repr_sparse_checks.py.  A dense k = 5 layer costs the emulator
half a second per 4 x 4 x 16 block, so the legs here take few entries: the map and the pooling at D = 21 and 13 with the whole
family; the first layer at D = 21 (two z tiles, six cells an axis) on two cuboids; the whole chain at D = 13; the plugin at
D = 21 on one cuboid and at D = 13 on a cuboid and the empty entry.  The device leg (tests/test_repr_sparse_gpu.py) runs every
check with the whole family at D = 21, 13, 37 and 80, the projected protein and the pooling's chunk loop."""
import pytest

import repr_sparse_checks as rs


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    rs.release_cases()


@pytest.mark.parametrize("D", [21, 13])
def test_tile_occupancy_equals_the_host_map_emulated(emu, D):
    rs.check_map(emu, "cpu", D)


@pytest.mark.parametrize("D", [21, 13])
def test_pooling_with_maps_meets_all_three_kinds_of_window_emulated(emu, D):
    rs.check_pool_windows(emu, "cpu", D)


def test_first_layer_over_two_z_tiles_emulated(emu):
    which = ("cuboid_xyz", "cuboid_zxy")
    rs.check_skipping_changes_no_bit(emu, "cpu", 21, which, depth=1)
    rs.check_unwritten(emu, "cpu", 21, which, depth=1)
    rs.check_truth(emu, "cpu", 21, which, depth=1)


def test_chain_with_maps_at_four_cells_an_axis_emulated(emu):
    which = ("cuboid_yzx", "empty", "full")
    rs.check_skipping_changes_no_bit(emu, "cpu", 13, which)
    rs.check_unwritten(emu, "cpu", 13, which)
    rs.check_truth(emu, "cpu", 13, which)


def test_covering_maps_give_the_same_bits_emulated(emu):
    rs.check_covering_maps(emu, "cpu", 13, ("cuboid_zxy", "empty"))


def test_volumes_k1_goes_by_per_entry_maps_emulated(emu):
    rs.check_consumer(emu, "cpu", 32, 16, ("cuboid_zxy", "empty"))


def test_plugin_outputs_with_maps_emulated(emu):
    rs.check_plugin(emu, "cpu", 13, ("cuboid_zxy", "empty"))


def test_plugin_outputs_with_maps_over_two_z_tiles_emulated(emu):
    rs.check_plugin(emu, "cpu", 21, ("cuboid_xyz",))


def test_outputs_with_maps_holds_for_the_entering_thread_only_emulated(emu):
    rs.check_outputs_with_maps_is_per_thread(emu, "cpu", 13)
