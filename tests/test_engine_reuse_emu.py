"""A live DockingEngine scores the next pair as a fresh engine does -- the emulator leg (one stream, one V, one candidate
set): case 1 shortened to A, C, A with two rotations each, the per-channel K1 and the live filter change, every sequence
poisoned.  Check bodies, the poison and what each case asserts on its own inputs: tests/engine_reuse_checks.py; the device
leg (tests/test_engine_reuse_gpu.py) runs every case, poisoned and plain."""
import engine_reuse_checks as rc


def test_box_40_sparse_pairs_on_a_live_engine_emulated(emu):
    rc.check_case1(emu, "cpu", (True,), short=True)


def test_per_channel_k1_on_a_live_engine_emulated(emu):
    rc.check_per_channel(emu, "cpu", (True,))


def test_live_filter_change_on_a_pooled_engine_emulated(emu):
    rc.check_live_filter_change(emu, "cpu", (True,))
