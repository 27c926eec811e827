"""The gate matrix's test-side pieces, held to the plain oracle (CPU): the block-RMS cache of
gate_matrix.CachedRmsBuffer against oracle/gate_ref.SoundBufferRef, the conditions the recipe's
inputs must meet before an engine is looked at, the push schedule, and the engine's launch-info
call on an engine that cannot exist here."""
import numpy as np
import pytest

import gate_matrix as gm
from oracle.gate_ref import MIN_THRESHOLD

NAMES = list(gm.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_cached_oracle_equals_the_plain_oracle(name):
    """Both buffers side by side over the ticks that fill the ring and 50 more: threshold,
    is_silent() and block_rms() equal at every tick, and the detectors in step.  Two streams a case
    (the plain oracle costs n_blocks block sums a tick)."""
    case = gm.CASES[name]
    _, data = gm.signals(name)
    fs = case["block"]
    ticks = -(-gm.ring_len(case) // fs) + 50
    assert ticks < data.shape[1] // fs
    for s in (0, 5):
        plain = gm.detector(gm.gate_config(case), cached=False, keep_audio=False)
        cached = gm.detector(gm.gate_config(case), cached=True, keep_audio=False)
        for t in range(ticks):
            blk = data[s, t * fs:(t + 1) * fs]
            plain.push_tick(blk)
            cached.push_tick(blk)
            assert cached.buf.silence_threshold == plain.buf.silence_threshold, (s, t)
            assert cached.buf.is_silent() == plain.buf.is_silent(), (s, t)
            assert cached.state == plain.state and cached.started == plain.started, (s, t)
            if plain.buf.is_buffer_full():
                assert np.array_equal(cached.buf.block_rms(), plain.buf.block_rms()), (s, t)
        assert plain.started and plain.tick - ticks == 0
        assert [(e.tick, e.length, e.skipped) for e in cached.events] == \
            [(e.tick, e.length, e.skipped) for e in plain.events]


@pytest.mark.parametrize("name", NAMES)
def test_recipe_conditions(name):
    """Conditions on the inputs, from the oracle alone: without them a case could pass with the
    threshold frozen, ties never met or no event cut."""
    f = gm.recipe_facts(name)
    assert min(f["events"]) >= 3, f["events"]
    assert f["skipped"] >= 1
    assert min(f["thresholds"]) >= 20, f["thresholds"]
    assert min(f["clamped"]) >= 1, f["clamped"]
    assert sum(f["ties"]) >= 1 and min(f["ties"]) >= 1, f["ties"]
    if name != "e_8192":   # (0.512 s ticks: every event has one length -- gate_matrix's docstring)
        assert f["scored"] >= 3


@pytest.mark.parametrize("name", NAMES)
def test_push_schedule(name):
    case = gm.CASES[name]
    n_ticks = gm.signals(name)[0].shape[1] // case["block"]
    sched = gm.push_schedule(case, n_ticks)
    assert sum(sched) == n_ticks
    assert max(sched) < gm.n_blocks(case)                  # every block RMS ever computed is exported
    assert max(sched) > gm.ticks_per_launch(case)          # one push is several gate launches
    if gm.n_blocks(case) > 13:
        assert set(gm.PUSH_CYCLE) <= set(sched)


def test_case_table_covers_every_reachable_family():
    assert sorted(set((c["rb"], c["dma"]) for c in gm.CASES.values())) == gm.REACHABLE
    assert sorted(set(c["tree"] for c in gm.CASES.values())) == [0, 1, 2, 3]
    for name in gm.PROFILE_CASES + gm.LISTENER_CASES:
        assert name in gm.CASES


def test_pcm16_signals_are_whole_steps():
    src, data = gm.signals("p_500_i16")
    assert src.dtype == np.int16 and data.dtype == np.float32
    assert np.array_equal(data.astype(np.float64) * 32768.0, src.astype(np.float64))
    assert MIN_THRESHOLD == 0.005


def test_launch_info_is_bound():
    from easywakeword_amd import StreamEngine, _lib
    lib = _lib.load()
    assert "ewk_gate_launch_info" in _lib.EXPORTS and hasattr(lib, "ewk_gate_launch_info")
    assert hasattr(StreamEngine, "gate_launch_info")
    assert lib.ewk_gate_launch_info(None, None, None, None, None, None, None) == _lib.EWK_EINVAL
