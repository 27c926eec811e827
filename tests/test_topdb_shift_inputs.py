"""The inputs of tests/test_gpu_topdb_shift.py exercise the paths they are meant for: a numpy
replay of the scorer's top_db rule (scripts/scout_sim.py on the oracle's log-mel), no GPU."""
import pytest

import topdb_shift_inputs as inp


@pytest.mark.parametrize("n", [9600, 25600])
def test_tie_case_is_flagged_by_the_old_rule_only(n):
    inp.check_tie(n)


def test_self_clamp_raises_the_max_late():
    inp.check_self_clamp()


@pytest.mark.parametrize("f2,a3,rise", inp.KEPT)
def test_kept_tiles_rise_by_a_decibel_or_more(f2, a3, rise):
    inp.check_kept_rise(f2, a3, rise)


def test_fallback_is_still_flagged():
    inp.check_fallback()


@pytest.mark.parametrize("n,frames,tiles", inp.EDGES)
def test_edges(n, frames, tiles):
    inp.check_edge(n, frames, tiles)


def test_long_segment_passes_the_tile_record():
    inp.check_long()
