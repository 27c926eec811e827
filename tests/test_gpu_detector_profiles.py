"""Detector profiles: per-stream gate timings (ewk_detector_profiles_set / ewk_stream_profile_assign).

Recipe (tests/profile_cases.py): 12 streams of lifecycle_util.streams(12, 1600, 8600), 231 ticks
of 1,600 samples (the ring fills at tick 100), a table of four profiles, stream i on the engine's
configuration when i % 5 == 0 and on profile i % 5 - 1 otherwise.  With the CPU oracle
(oracle/gate_ref.py, each stream with its own GateConfig) that gives 27 events, 4 of them skipped
(the streams of profile 1), every profiled stream's list different from the default
configuration's.  Those properties of the ORACLE's lists are asserted before an engine is looked
at (profile_cases.assert_recipe_tells), so no test here passes with the table ignored.

Bars: event lists equal to the oracle's; scores within 1e-4 of oracle/mfcc_ref (the project's
bar) with equal decisions; between two engine runs every field and the score's bits equal.
"""
import ctypes as C

import numpy as np
import pytest

import bank_cases as bc
import lifecycle_util as lu
import profile_cases as pc
from golden_io import matcher_fixture, score_close, template_arrays
from oracle import mfcc_ref

pytestmark = pytest.mark.gpu

N, BLOCK = pc.N, pc.BLOCK
FILL = 100   # ticks until the 10 s ring is full


@pytest.fixture(scope="module")
def template():
    fx, _ = matcher_fixture()
    return template_arrays(fx)


def _engine(template, n=N, table=True, assign=None, **cfg):
    from easywakeword_amd import StreamEngine
    eng = StreamEngine(n, **cfg)
    eng.set_template(*template)
    if table:
        eng.set_detector_profiles(pc.PROFILES)
        a = pc.assignment(n) if assign is None else np.asarray(assign, np.int32)
        eng.assign_stream_profiles(np.arange(n, dtype=np.int32), a)
    return eng


def _lockstep(eng, data, t0=0, t1=None, step=7, block=BLOCK, pcm16=False):
    t1 = data.shape[1] // block if t1 is None else t1
    got = [eng.poll()]
    for c in range(t0, t1, step):
        (eng.push_pcm16 if pcm16 else eng.push_many)(data[:, c * block:min(c + step, t1) * block])
        got.append(eng.poll())
    return np.concatenate(got)


def _final(eng, n=N):
    return dict(thr=[eng.state(i)["silence_threshold"] for i in range(n)],
                last=[eng.read_last(i, 6400) for i in range(n)])


_runs = {}


@pytest.fixture(scope="module")
def case(template):
    """The oracle's lists (held to the recipe's properties) and the lockstep run of the mixed engine."""
    c = pc.main_case()
    pc.assert_recipe_tells(c)
    if "mixed" not in _runs:
        eng = _engine(template)
        ev = _lockstep(eng, c["data"])
        _runs["mixed"] = dict(ev=ev, profiles=eng.stream_profiles(), table=eng.detector_profiles(), **_final(eng))
        eng.close()
    return dict(c, **_runs["mixed"])


def _check_oracle(ev, ref, template, n, max_scores=12):
    """Per stream (tick, length, skipped) and time equal the oracle's; the first `max_scores`
    scored events within 1e-4 of the oracle's score, decisions equal.  Returns (events, scores)."""
    tm, ts = template
    n_ev = n_sc = 0
    for i, mine in enumerate(lu.by_stream(ev, n)):
        assert pc.engine_key(mine) == pc.key(ref[i]), i
        np.testing.assert_array_equal(mine["time"], np.array([e.time for e in ref[i]], np.float64), err_msg=f"stream {i}")
        for m, e in zip(mine, ref[i]):
            n_ev += 1
            if e.skipped or e.audio is None or n_sc >= max_scores:
                continue
            cm, cs = mfcc_ref.extract_mfcc(e.audio)
            s = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
            assert score_close(float(m["score"]), s, 1e-4), (i, e.tick, float(m["score"]), s)
            assert bool(m["match"]) == (s >= 75.0), (i, e.tick)
            n_sc += 1
    return n_ev, n_sc


def _solo(template, data, stream, profile):
    """Stream `stream` alone in a one-stream engine whose ewk_config holds the profile's numbers."""
    k = ("solo", stream, profile)
    if k not in _runs:
        eng = _engine(template, n=1, table=False, **pc.engine_config(profile))
        _runs[k] = _lockstep(eng, data[stream:stream + 1])
        eng.close()
    return _runs[k]


def _as_stream0(ev, stream):
    out = ev[ev["stream"] == stream].copy()
    out["stream"] = 0
    return out


# ---- 1
def test_mixed_profiles_equal_the_oracle(case, template):
    n_ev, n_sc = _check_oracle(case["ev"], case["ref"], template, N)
    assert n_ev >= 20 and n_sc == 12
    np.testing.assert_array_equal(case["profiles"], case["assign"])
    assert len(case["table"]) == 4 and case["table"][1].max_segment_seconds == 0.8
    assert case["table"][0].padding == 0.05 and case["table"][2].reentry_timeout == 3.0   # missing fields: the config's
    # the timings do not leak into ingest: thresholds and rings of an engine without a table
    eng = _engine(template, table=False)
    _lockstep(eng, case["data"], step=33)
    plain = _final(eng)
    eng.close()
    assert plain["thr"] == case["thr"]
    for i in range(N):
        np.testing.assert_array_equal(plain["last"][i], case["last"][i], err_msg=f"stream {i}")


# ---- 2
@pytest.mark.parametrize("stream", [1, 2, 3, 4, 5])
def test_one_stream_equals_one_engine(case, template, stream):
    profile = int(case["assign"][stream])
    solo = _solo(template, case["data"], stream, profile)
    assert len(solo) == len(case["ref"][stream])
    lu.assert_events_equal(_as_stream0(case["ev"], stream), solo, 1)


# ---- 3
def test_wave_stream_loop_with_a_capped_grid(case, template, monkeypatch):
    """EWK_GATE_GRID_MAX=1: one workgroup, four waves of three streams each, every wave's streams
    on different profiles -- the profile is re-read for every stream of the loop."""
    monkeypatch.setenv("EWK_GATE_GRID_MAX", "1")
    eng = _engine(template)
    ev = _lockstep(eng, case["data"])
    eng.close()
    assert lu.assert_events_equal(case["ev"], ev, N) >= 20
    # the cap alone changes nothing: table-less engines with and without it
    capped = _engine(template, table=False)
    ev_capped = _lockstep(capped, case["data"], step=33)
    capped.close()
    monkeypatch.delenv("EWK_GATE_GRID_MAX")
    plain = _engine(template, table=False)
    ev_plain = _lockstep(plain, case["data"], step=33)
    plain.close()
    assert lu.assert_events_equal(ev_plain, ev_capped, N) >= 10
    assert [pc.engine_key(x) for x in lu.by_stream(ev_plain, N)] == [pc.key(r) for r in case["ref_default"]]


# ---- 4
GEOMETRIES = {
    # name: (block, seed, PCM16 pushes, engine config, oracle scores compared)
    "b1600_i16_compact": (1600, 8900, True,
                          dict(ring_format=1, ring_samples=lu.min_ring(1600, max_speech=2.4, post=0.5, pad=0.1)), 6),
    "b400_regs8": (400, 8700, False, {}, 4),
    "b250_memory": (250, 8802, False, {}, 4),
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_launch_geometries(template, name):
    block, seed, pcm16, cfg, n_scores = GEOMETRIES[name]
    assign = [0, 1, 3, -1]
    data = lu.streams(4, block, seed)
    src = data
    if pcm16:
        src, data = lu.to_pcm16(data)
    ref = [pc.run(data[i], pc.gate_config(p, block)) for i, p in enumerate(assign)]
    dflt = [pc.run(data[i], pc.gate_config(-1, block), keep_audio=False) for i in range(4)]
    assert sum(len(r) for r in ref) >= 6
    assert all(pc.key(ref[i]) != pc.key(dflt[i]) for i in range(3))   # the oracle tells the profiles apart
    eng = _engine(template, n=4, assign=assign, block=block, tick_seconds=block / 16000, **cfg)
    ev = _lockstep(eng, src, step=29, block=block, pcm16=pcm16)
    np.testing.assert_array_equal(eng.stream_profiles(), assign)
    eng.close()
    n_ev, n_sc = _check_oracle(ev, ref, template, 4, max_scores=n_scores)
    assert n_ev >= 6 and n_sc >= 1


# ---- 5
def test_reassignment_mid_stream(case, template):
    data, n_ticks = case["data"], case["n_ticks"]
    D, P0 = pc.gate_config(-1), pc.gate_config(0)
    half = np.arange(0, N, 2, dtype=np.int32)
    tail = data[:, 150 * BLOCK:]
    twice = np.concatenate([data, tail], axis=1)
    ref1 = [pc.run(data[i], [(0, D), (150, P0)], keep_audio=False) for i in range(N)]
    pure = [pc.key(pc.run(data[i], P0, keep_audio=False)) for i in range(N)]
    both = [i for i in range(N) if pc.key(ref1[i]) not in (pure[i], pc.key(case["ref_default"][i]))]
    assert len(both) >= 4, both   # the switch is visible in the oracle's lists
    ref2 = [pc.run(twice[i], [(0, D), (150, P0)] + ([(n_ticks, D)] if i in half else []), keep_audio=False)
            for i in range(N)]

    eng = _engine(template, table=False)
    eng.set_detector_profiles(pc.PROFILES)
    ev = [_lockstep(eng, data, 0, 150)]
    before = eng.state(2)
    eng.assign_stream_profiles(np.arange(N, dtype=np.int32), np.zeros(N, np.int32))
    after = eng.state(2)
    assert before == after                                   # FSM state and clock untouched
    assert (eng.stream_ticks() == 150).all()                 # still in lockstep
    ev.append(_lockstep(eng, data, 150))
    got1 = np.concatenate(ev)
    for i, mine in enumerate(lu.by_stream(got1, N)):
        assert pc.engine_key(mine) == pc.key(ref1[i]), i
    eng.assign_stream_profiles(half, np.full(half.size, -1, np.int32))
    ev.append(_lockstep(eng, tail))
    got2 = np.concatenate(ev)
    eng.close()
    for i, mine in enumerate(lu.by_stream(got2, N)):
        assert pc.engine_key(mine) == pc.key(ref2[i]), i
        np.testing.assert_array_equal(mine["time"], np.array([e.time for e in ref2[i]]), err_msg=f"stream {i}")


# ---- 6
def test_subset_pushes_and_resets(case, template):
    data, n_ticks = case["data"], case["n_ticks"]
    eng = _engine(template)
    got = []
    for sub, nt, first in lu.schedule(N, n_ticks, 77):
        eng.push_streams(sub, lu.rows_of(data, sub, first, nt, BLOCK))
        got.append(eng.poll())
    assert lu.assert_events_equal(case["ev"], np.concatenate(got), N) >= 20
    # a reset keeps the profile: the streams replay as fresh one-stream engines of their profile
    eng.reset_streams([3, 7])
    np.testing.assert_array_equal(eng.stream_profiles(), case["assign"])
    sub = np.array([7, 3], np.int32)
    again = []
    for c in range(0, n_ticks, 9):
        eng.push_streams(sub, lu.rows_of(data, sub, [c, c], min(9, n_ticks - c), BLOCK))
        again.append(eng.poll())
    again = np.concatenate(again)
    eng.close()
    assert set(again["stream"].tolist()) <= {3, 7}
    for s in (3, 7):
        solo = _solo(template, data, s, int(case["assign"][s]))
        assert len(solo) == len(case["ref"][s])
        lu.assert_events_equal(_as_stream0(again, s), solo, 1)
    assert len(case["ref"][7]) >= 1


# ---- 7
def test_stream_bank_with_profiles(case, template):
    from easywakeword_amd import _lib
    eng = _engine(template)
    eng.bank_from_pcm(bc.bank_audio()[:2], thresholds=bc.THRESHOLDS[:2])
    eng.set_stream_bank(np.arange(N, dtype=np.int32) % 2)
    ev = _lockstep(eng, case["data"])
    eng.close()
    for mine, want in zip(lu.by_stream(ev, N), lu.by_stream(case["ev"], N)):
        assert pc.engine_key(mine) == pc.engine_key(want)
    scored = ev[(ev["flags"] & _lib.EWK_EV_SKIPPED) == 0]
    assert len(scored) >= 15 and ((scored["flags"] & _lib.EWK_EV_BANK) != 0).all()
    assert (ev["flags"] & _lib.EWK_EV_SKIPPED != 0).sum() >= 1


# ---- 8
def _bad(i, **kw):
    t = [dict(p) for p in pc.PROFILES]
    t[i].update(kw)
    return t


def test_validation_changes_nothing(case, template):
    from easywakeword_amd import Engine, _lib
    eng = _engine(template)

    def unchanged():
        np.testing.assert_array_equal(eng.stream_profiles(), case["assign"])
        assert eng.detector_profiles() == case["table"]

    with pytest.raises(ValueError, match=r"profiles\[2\]\.speech_duration_min must be <= speech_duration_max"):
        eng.set_detector_profiles(_bad(2, speech_duration_min=2.5))
    unchanged()
    with pytest.raises(ValueError, match=r"profiles\[1\]\.post_speech_silence"):
        eng.set_detector_profiles(_bad(1, post_speech_silence=float("nan")))
    unchanged()
    with pytest.raises(ValueError, match=r"profiles\[3\]\.reentry_timeout is NaN"):
        eng.set_detector_profiles(_bad(3, reentry_timeout=float("nan")))
    unchanged()
    with pytest.raises(ValueError, match=r"profiles\[0\]\.padding"):
        eng.set_detector_profiles(_bad(0, padding=-0.01))
    unchanged()
    with pytest.raises(ValueError, match=str(_lib.EWK_PROFILE_MAX + 1)):
        eng.set_detector_profiles([pc.PROFILES[0]] * (_lib.EWK_PROFILE_MAX + 1))
    unchanged()
    with pytest.raises(ValueError, match=r"profile index 4 of stream 6"):
        eng.assign_stream_profiles([5, 6], [0, 4])
    unchanged()
    with pytest.raises(ValueError, match=r"profile index -2 of stream 5"):
        eng.assign_stream_profiles([5, 6], [-2, 0])
    unchanged()
    with pytest.raises(ValueError, match="listed twice"):
        eng.assign_stream_profiles([5, 6, 5], [0, 0, 0])
    unchanged()
    with pytest.raises(ValueError, match=r"stream 3 points at profile 2 of a table of 2"):
        eng.set_detector_profiles(pc.PROFILES[:2])
    unchanged()
    # ... and the engine still runs test 1's events (the first 20 ticks past the fill)
    upto = FILL + 20
    ev = _lockstep(eng, case["data"], 0, upto)
    want = case["ev"][case["ev"]["tick"] <= upto]
    lu.assert_events_equal(want, ev, N)
    eng.close()

    # a profile whose longest request does not fit a compact ring
    small = _engine(template, n=2, table=False, ring_samples=lu.min_ring(1600))
    with pytest.raises(ValueError, match=r"profiles\[1\]: ring_samples must hold .*\(\d+ samples for this profile"):
        small.set_detector_profiles(pc.PROFILES)
    assert small.detector_profiles() == [] and (small.stream_profiles() == -1).all()
    with pytest.raises(ValueError, match="no profile table"):
        small.assign_stream_profiles([0], [0])
    small.close()

    # an engine without streams
    scorer = Engine()
    p = _lib.EwkDetectorProfile()
    scorer._lib.ewk_default_detector_profile(scorer.handle, C.byref(p))
    assert (p.speech_duration_max, p.padding) == (2.0, 0.05)
    with pytest.raises(ValueError, match="no streams"):
        _lib.check(scorer._lib.ewk_detector_profiles_set(scorer.handle, C.byref(p), 1))
    scorer.close()


def test_clearing_the_table_returns_to_the_configuration(case, template):
    eng = _engine(template)
    eng.set_detector_profiles(pc.PROFILES[:1] * 5)     # a longer table replaces a shorter one
    assert len(eng.detector_profiles()) == 5
    eng.set_detector_profiles(None)
    assert eng.detector_profiles() == [] and (eng.stream_profiles() == -1).all()
    ev = _lockstep(eng, case["data"], step=33)
    eng.close()
    assert [pc.engine_key(x) for x in lu.by_stream(ev, N)] == [pc.key(r) for r in case["ref_default"]]


# ---- 9
def test_ticks_per_launch_follows_the_longest_profile(template):
    """A 4 s ring and a profile with a 3.0 s maximum and 0.5 s of post silence: the longest
    request leaves room for 3 ticks per gate launch where the configuration's own leaves 14
    (test_short_buffer_push_many_scores_intact_segments, now caused by a profile)."""
    data = lu.streams(6, BLOCK, 9304, n_words=5)
    n_ticks = data.shape[1] // BLOCK
    long = [dict(speech_duration_max=3.0, post_speech_silence=0.5)]
    ref = [pc.run(data[i], pc.gate_config(-1, buffer_seconds=4, **long[0]), keep_audio=False) for i in range(6)]
    assert sum(len(r) for r in ref) >= 10

    def run(step):
        eng = _engine(template, n=6, table=False, buffer_seconds=4)
        eng.set_detector_profiles(long)
        eng.assign_stream_profiles(np.arange(6, dtype=np.int32), np.zeros(6, np.int32))
        eng.profile(True)
        ev = _lockstep(eng, data, step=step)
        launches = eng.profile_read(2)[1]
        eng.close()
        return ev, launches

    ev40, l40 = run(40)
    ev1, l1 = run(1)
    assert l1 == n_ticks
    assert l40 == sum(-(-min(40, n_ticks - c) // 3) for c in range(0, n_ticks, 40))
    assert lu.assert_events_equal(ev1, ev40, 6) >= 10
    assert [pc.engine_key(x) for x in lu.by_stream(ev40, 6)] == [pc.key(r) for r in ref]
    # cleared: the configuration's own 14 ticks per launch again
    eng = _engine(template, n=6, table=False, buffer_seconds=4)
    eng.set_detector_profiles(long)
    eng.set_detector_profiles([])
    eng.profile(True)
    eng.push_many(data[:, :40 * BLOCK])
    assert eng.profile_read(2)[1] == 3
    eng.close()
