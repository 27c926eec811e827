"""The inputs of tests/test_gpu_topdb_mask_skip.py exercise the paths they are meant for: a numpy
replay of the mask rule (scripts/scout_sim.py on the oracle's log-mel, the window X read from
csrc/ewk_topdb_shift.h), no GPU."""
import pytest

import topdb_mask_inputs as inp


def test_window_is_read_from_the_header():
    assert 3.0 <= inp.window_db() <= 20.0


def test_loud_tile_first_skips_every_mask_and_nothing_rises():
    inp.check_loud_one()


@pytest.mark.parametrize("a3,rise", inp.FOOLED)
def test_fooled_scout_recomputes_the_unmasked_tiles(a3, rise):
    inp.check_fooled(a3, rise)


def test_masked_and_unmasked_tiles_meet_one_rise():
    inp.check_mixed()


def test_first_tile_self_clamped_and_unmasked():
    inp.check_first_unmasked()


def test_equal_tiles_mask_all_but_the_last():
    inp.check_tie()
