"""Stream listeners: several (detector profile, word) pairs on one stream, one ring and one gate
pass (ewk_stream_listeners_set).

Main recipe (tests/listener_cases.py): streams 0..3 of lifecycle_util.streams(12, 1600, 8600), 231
ticks, every stream with the five listeners (-1, 0, 1, 2, 3) of profile_cases.PROFILES.  The CPU
oracle (oracle/gate_ref.py, one run per (stream, profile)) gives 49 events, 7 of them skipped, at
least four pairwise different lists per stream and three ticks at which several listeners of one
stream cut together.  Those properties of the ORACLE's lists are asserted before an engine is
looked at (listener_cases.assert_main_recipe), so no test here passes with listeners ignored.

Bars: per listener the event list equals the oracle's; scores within 1e-4 of oracle/mfcc_ref (the
project's bar) with equal decisions; between two engine runs every field and the score's bits are
equal, flags apart from the listener bits where one side has a stream per listener.
"""
import ctypes as C

import numpy as np
import pytest

import bank_cases as bc
import lifecycle_util as lu
import listener_cases as lc
import profile_cases as pc
from golden_io import matcher_fixture, template_arrays

pytestmark = pytest.mark.gpu

BLOCK = lc.BLOCK
L5 = lc.LISTENERS
ROWS5 = lc.rows(L5)


@pytest.fixture(scope="module")
def template():
    fx, _ = matcher_fixture()
    return template_arrays(fx)


def _engine(template, n, table=True, listeners=None, **cfg):
    from easywakeword_amd import StreamEngine
    eng = StreamEngine(n, **cfg)
    eng.set_template(*template)
    if table:
        eng.set_detector_profiles(pc.PROFILES)
    if listeners is not None:
        eng.set_stream_listeners(np.arange(n, dtype=np.int32), listeners)
    return eng


def _lockstep(eng, data, t0=0, t1=None, step=7, block=BLOCK, pcm16=False):
    t1 = data.shape[1] // block if t1 is None else t1
    got = [eng.poll()]
    for c in range(t0, t1, step):
        (eng.push_pcm16 if pcm16 else eng.push_many)(data[:, c * block:min(c + step, t1) * block])
        got.append(eng.poll())
    return np.concatenate(got)


def _final(eng, n):
    return dict(thr=[eng.state(i)["silence_threshold"] for i in range(n)],
                last=[eng.read_last(i, 6400) for i in range(n)])


def _per_stream_engine(template, data4, words=None):
    """The path that exists without listeners: 20 streams, row 5 s + j holds stream s's audio and
    is gated with profile L5[j] (and listens for word j % 2)."""
    eng = _engine(template, 20)
    eng.assign_stream_profiles(np.arange(20, dtype=np.int32), np.array([L5[i % 5] for i in range(20)], np.int32))
    if words is not None:
        eng.bank_from_pcm(bc.bank_audio()[:2], thresholds=bc.THRESHOLDS[:2])
        eng.set_stream_bank(np.array([words[i % 5] for i in range(20)], np.int32))
    return eng, np.repeat(data4, 5, axis=0)


_runs = {}


@pytest.fixture(scope="module")
def case(template):
    """The oracle's lists (held to the recipe's properties) and the lockstep run of the 4-stream
    engine with five listeners per stream."""
    c = lc.main_case()
    lc.assert_main_recipe(c)
    if "main" not in _runs:
        data4 = np.ascontiguousarray(c["data"][:4])
        eng = _engine(template, 4, listeners=[ROWS5] * 4)
        ev = _lockstep(eng, data4)
        _runs["main"] = dict(ev=ev, data4=data4, listeners=[eng.stream_listeners(s) for s in range(4)], **_final(eng, 4))
        eng.close()
    return dict(c, **_runs["main"])


def _assert_listeners_equal(a, b, width=5, n=4):
    """Two runs with listeners: per (stream, listener) every field and the score's bits."""
    return lu.assert_events_equal(lc.as_streams(a, width), lc.as_streams(b, width), n * width)


# ---- 1
def test_listeners_equal_the_oracle(case, template):
    by = lc.by_listener(case["ev"], range(4), 5)
    budget, n_ev, n_sc = [12], 0, 0
    for s in range(4):
        for j, p in enumerate(L5):
            e, sc = lc.check_oracle(by[(s, j)], case["ref"][(s, p)], template, budget)
            n_ev, n_sc = n_ev + e, n_sc + sc
    assert n_ev == len(case["ev"]) == 49 and n_sc == 12
    assert case["listeners"] == [ROWS5] * 4
    # the poll's order: (tick, stream, listener)
    order = list(zip(case["ev"]["tick"].tolist(), case["ev"]["stream"].tolist(), lc.listener_of(case["ev"]).tolist()))
    assert order == sorted(order)
    # listeners do not leak into ingest: thresholds and rings of an engine without them
    eng = _engine(template, 4, table=False)
    _lockstep(eng, case["data4"], step=33)
    plain = _final(eng, 4)
    assert eng.stream_listeners(2) == [(-1, 0)]
    eng.close()
    assert plain["thr"] == case["thr"]
    for i in range(4):
        np.testing.assert_array_equal(plain["last"][i], case["last"][i], err_msg=f"stream {i}")


# ---- 2
def test_listeners_equal_separate_streams(case, template):
    eng, data20 = _per_stream_engine(template, case["data4"])
    ev20 = _lockstep(eng, data20)
    eng.close()
    assert lu.assert_events_equal(lc.as_streams(case["ev"], 5), ev20, 20) == 49


def test_listeners_equal_separate_streams_with_the_stream_bank(case, template):
    from easywakeword_amd import _lib
    words = [j % 2 for j in range(5)]
    eng, data20 = _per_stream_engine(template, case["data4"], words)
    ev20 = _lockstep(eng, data20)
    eng.close()
    eng = _engine(template, 4)
    eng.bank_from_pcm(bc.bank_audio()[:2], thresholds=bc.THRESHOLDS[:2])
    eng.set_stream_bank()
    eng.set_stream_listeners(np.arange(4, dtype=np.int32), [lc.rows(L5, words)] * 4)
    assert eng.stream_listeners(3) == lc.rows(L5, words)
    ev = _lockstep(eng, case["data4"])
    eng.close()
    assert lu.assert_events_equal(lc.as_streams(ev, 5), ev20, 20) == 49     # flags: EWK_EV_BANK and EWK_EV_BEST too
    scored = ev[(ev["flags"] & _lib.EWK_EV_SKIPPED) == 0]
    assert len(scored) >= 15 and ((scored["flags"] & _lib.EWK_EV_BANK) != 0).all()
    # the two words give different scores to one segment: listeners 0 and 2 (profiles -1, 1) of stream 0 at tick 161
    a = ev[(ev["stream"] == 0) & (ev["tick"] == 161)]
    assert len(a) >= 2 and len(set(a["score"].tolist())) >= 2


# ---- 3
def test_wave_loop_and_lane_edges(case, template, monkeypatch):
    """EWK_GATE_GRID_MAX=1: one workgroup, four waves of three streams each, 1..16 listeners per
    stream -- count, profile indices and lane states are re-read for every stream of the loop."""
    data = case["data"]
    counts = [1 + (5 * i) % 16 for i in range(12)]
    assert 1 in counts and 16 in counts
    listeners = [lc.rows([L5[j % 5] for j in range(c)]) for c in counts]

    def run():
        eng = _engine(template, 12, listeners=listeners)
        ev = _lockstep(eng, data)
        assert [len(eng.stream_listeners(i)) for i in range(12)] == counts
        eng.close()
        return ev

    monkeypatch.setenv("EWK_GATE_GRID_MAX", "1")
    capped = run()
    monkeypatch.delenv("EWK_GATE_GRID_MAX")
    plain = run()
    assert lu.assert_events_equal(lc.as_streams(plain, 16), lc.as_streams(capped, 16), 12 * 16) >= 49
    by = lc.by_listener(capped, range(12), 16)
    for s in range(4):
        for j in range(counts[s]):
            assert pc.engine_key(by[(s, j)]) == pc.key(case["ref"][(s, L5[j % 5])]), (s, j)
        for j in range(counts[s], 16):
            assert len(by[(s, j)]) == 0
    s16 = counts.index(16)
    assert len(by[(s16, 15)]) >= 1
    for f in lu.EVENT_FIELDS:      # listener 15 has listener 0's profile
        want = by[(s16, 0)][f] if f != "flags" else by[(s16, 0)][f] | (15 << 16)
        np.testing.assert_array_equal(by[(s16, 15)][f], want, err_msg=f)
    np.testing.assert_array_equal(by[(s16, 15)]["score"].view(np.int64), by[(s16, 0)]["score"].view(np.int64))


# ---- 4
@pytest.mark.parametrize("name", list(lc.GEOMETRIES))
def test_launch_geometries(template, name):
    g = lc.geometry_case(name)
    block = g["block"]
    eng = _engine(template, 2, listeners=[lc.rows(lc.GEOMETRY_LISTENERS)] * 2, block=block,
                  tick_seconds=block / 16000, **g["cfg"])
    ev = _lockstep(eng, g["src"], step=29, block=block, pcm16=g["pcm16"])
    eng.close()
    by = lc.by_listener(ev, range(2), 4)
    budget, n_ev, n_sc = [4], 0, 0
    for s in range(2):
        for j, p in enumerate(lc.GEOMETRY_LISTENERS):
            e, sc = lc.check_oracle(by[(s, j)], g["ref"][(s, p)], template, budget)
            n_ev, n_sc = n_ev + e, n_sc + sc
    assert n_ev == len(ev) >= 6 and n_sc >= 1


# ---- 5
def test_subset_pushes_and_resets(case, template):
    data4, n_ticks = case["data4"], case["n_ticks"]
    eng = _engine(template, 4, listeners=[ROWS5] * 4)
    got = []
    for sub, nt, first in lu.schedule(4, n_ticks, 77):
        eng.push_streams(sub, lu.rows_of(data4, sub, first, nt, BLOCK))
        got.append(eng.poll())
    assert _assert_listeners_equal(case["ev"], np.concatenate(got)) == 49
    for s in range(4):                                   # (f) listener 0 is the stream's own state
        assert eng.listener_state(s, 0) == eng.state(s)
        other = eng.listener_state(s, 3)
        assert (other["tick"], other["silence_threshold"]) == (eng.state(s)["tick"], eng.state(s)["silence_threshold"])
    with pytest.raises(ValueError, match="has 5 listener"):
        eng.listener_state(0, 5)
    # (b) a reset keeps the table; both streams replay as fresh one-stream engines of each profile
    eng.reset_streams([1, 3])
    assert [eng.stream_listeners(s) for s in range(4)] == [ROWS5] * 4
    assert eng.listener_state(1, 2)["state"] == 0 and eng.listener_state(1, 2)["start_time"] == 0.0
    sub = np.array([3, 1], np.int32)
    again = []
    for c in range(0, n_ticks, 9):
        eng.push_streams(sub, lu.rows_of(data4, sub, [c, c], min(9, n_ticks - c), BLOCK))
        again.append(eng.poll())
    again = np.concatenate(again)
    eng.close()
    assert set(again["stream"].tolist()) <= {1, 3}
    by = lc.by_listener(again, (1, 3), 5)
    n = 0
    for s in (1, 3):
        for j, p in enumerate(L5):
            solo = _engine(template, 1, table=False, **pc.engine_config(p))
            want = _lockstep(solo, data4[s:s + 1], step=33)
            solo.close()
            mine = by[(s, j)].copy()
            mine["stream"] = 0
            mine["flags"] &= ~lc.LISTENER_MASK
            assert len(want) == len(case["ref"][(s, p)])
            n += lu.assert_events_equal(mine, want, 1)
    assert n == sum(len(case["ref"][(s, p)]) for s in (1, 3) for p in L5) >= 20


def test_adding_and_dropping_listeners_mid_stream(case, template):
    data4, ref = case["data4"], case["ref"]
    P0 = pc.gate_config(0)
    late = [lc.run_entered(data4[s], P0, 150) for s in range(4)]
    differs = [s for s in range(4) if pc.key(late[s]) != pc.key([e for e in ref[(s, 0)] if e.tick > 150])]
    assert differs, "profile 0 entered at tick 150 must differ from profile 0 all along"
    # (c) streams running listeners (-1, 2) get a third listener, profile 0, at tick 150
    eng = _engine(template, 4, listeners=[lc.rows((-1, 2))] * 4)
    ev = [_lockstep(eng, data4, 0, 150)]
    before = [eng.listener_state(s, 1) for s in range(4)]
    eng.set_stream_listeners(np.arange(4, dtype=np.int32), [lc.rows((-1, 2, 0))] * 4)
    assert [eng.listener_state(s, 1) for s in range(4)] == before      # an existing listener keeps its state
    assert (eng.stream_ticks() == 150).all()                           # still in lockstep
    for s in range(4):
        st, new = eng.state(s), eng.listener_state(s, 2)
        assert new["start_time"] == 150 * 0.1 and new["state"] == (1 if st["last_silent"] else 0)
    ev.append(_lockstep(eng, data4, 150))
    ev = np.concatenate(ev)
    eng.close()
    # ... which equals a separate stream on profile 0 re-entered at tick 150
    sep = _engine(template, 4)
    sep.assign_stream_profiles(np.arange(4, dtype=np.int32), np.zeros(4, np.int32))
    _lockstep(sep, data4, 0, 150)
    sep.reenter(-1)
    want = _lockstep(sep, data4, 150)
    sep.close()
    by = lc.by_listener(ev, range(4), 3)
    for s in range(4):
        mine = by[(s, 2)].copy()
        mine["flags"] &= ~lc.LISTENER_MASK
        assert pc.engine_key(mine) == pc.key(late[s]), s
        lu.assert_events_equal(mine[mine["stream"] == s], want[want["stream"] == s], 4)
        assert pc.engine_key(by[(s, 0)]) == pc.key(ref[(s, -1)]) and pc.engine_key(by[(s, 1)]) == pc.key(ref[(s, 2)])
    # (d) five listeners shrink to two at tick 150: the dropped ones stop, the others go on
    eng = _engine(template, 4, listeners=[ROWS5] * 4)
    ev = [_lockstep(eng, data4, 0, 150)]
    eng.set_stream_listeners(np.arange(4, dtype=np.int32), [ROWS5[:2]] * 4)
    assert eng.stream_listeners(0) == ROWS5[:2]
    ev.append(_lockstep(eng, data4, 150))
    eng.close()
    ev = np.concatenate(ev)
    want = case["ev"][(lc.listener_of(case["ev"]) < 2) | (case["ev"]["tick"] <= 150)]
    assert len(want) < len(case["ev"])
    assert _assert_listeners_equal(want, ev) == len(want)


def test_reenter_reenters_every_listener(case, template):
    data4 = case["data4"]
    eng = _engine(template, 4, listeners=[ROWS5] * 4)
    ev = [_lockstep(eng, data4, 0, 150)]
    eng.reenter(2)
    ev.append(_lockstep(eng, data4, 150))
    eng.close()
    ev = np.concatenate(ev)
    sep, data20 = _per_stream_engine(template, data4)
    want = [_lockstep(sep, data20, 0, 150)]
    for i in range(10, 15):
        sep.reenter(i)
    want.append(_lockstep(sep, data20, 150))
    sep.close()
    assert lu.assert_events_equal(lc.as_streams(ev, 5), np.concatenate(want), 20) == len(ev)
    assert len(ev) < 49      # the re-entry costs stream 2 events (the oracle: profile 0 and 2 lose theirs)


# ---- 6
def test_validation_changes_nothing(case, template):
    from easywakeword_amd import Engine, _lib
    eng = _engine(template, 4, listeners=[ROWS5] * 4)
    expect = [ROWS5] * 4

    def unchanged():
        assert [eng.stream_listeners(s) for s in range(4)] == expect

    with pytest.raises(ValueError, match=r"stream 1: a stream has 1\.\.16 listeners, got count 0"):
        eng.set_stream_listeners([0, 1], [[-1], []])
    unchanged()
    with pytest.raises(ValueError, match=r"stream 2: .* got count 17"):
        eng.set_stream_listeners([2], [[-1] * 17])
    unchanged()
    with pytest.raises(ValueError, match=r"stride 2 is below the count 3 of stream 1"):
        eng.set_stream_listeners([0, 1], [[-1, 0], [-1, 0, 1]], stride=2)
    unchanged()
    with pytest.raises(ValueError, match=r"listener 1 of stream 3: profile 4 is outside \[-1, 4\)"):
        eng.set_stream_listeners([3], [[-1, 4]])
    unchanged()
    with pytest.raises(ValueError, match=r"listener 0 of stream 3: profile -2 is outside"):
        eng.set_stream_listeners([3], [[-2, 0]])
    unchanged()
    with pytest.raises(ValueError, match=r"listener 2 of stream 0: word 1 while the stream bank is off"):
        eng.set_stream_listeners([0], [[(-1, 0), (0, 0), (1, 1)]])
    unchanged()
    with pytest.raises(ValueError, match="listed twice"):
        eng.set_stream_listeners([1, 2, 1], [[-1]] * 3)
    unchanged()
    with pytest.raises(ValueError, match=r"listener 3 of stream 0 points at profile 2 of a table of 2"):
        eng.set_detector_profiles(pc.PROFILES[:2])
    with pytest.raises(ValueError, match=r"listener 1 of stream 0 points at profile 0 of a table of 0"):
        eng.set_detector_profiles(None)
    unchanged()
    assert len(eng.detector_profiles()) == 4
    # words: past the bank, and a bank that is too small for a listener's word
    audio = bc.bank_audio()
    eng.bank_from_pcm(audio[:2], thresholds=bc.THRESHOLDS[:2])
    eng.set_stream_bank()
    with pytest.raises(ValueError, match=r"listener 1 of stream 2: word 2 is outside \[0, 2\)"):
        eng.set_stream_listeners([2], [[(-1, 0), (0, 2)]])
    unchanged()
    expect = [lc.rows(L5, [0, 1, 0, 1, 1])] * 4
    eng.set_stream_listeners(np.arange(4, dtype=np.int32), expect)
    unchanged()
    eng.clear_stream_bank()
    eng.bank_from_pcm(audio[:1], thresholds=bc.THRESHOLDS[:1])
    with pytest.raises(ValueError, match=r"listener 1 of stream 0: word 1 is outside \[0, 1\)"):
        eng.set_stream_bank()
    unchanged()
    # ... and the engine (stream bank still off) runs test 1's events for 20 ticks past the fill
    upto = lc.FILL + 20
    ev = _lockstep(eng, case["data4"], 0, upto)
    want = case["ev"][case["ev"]["tick"] <= upto]
    _assert_listeners_equal(want, ev)
    eng.close()

    bare = _engine(template, 2, table=False)
    with pytest.raises(ValueError, match=r"listener 1 of stream 0: profile 0 is outside \[-1, 0\) \(no profile table"):
        bare.set_stream_listeners([0], [[-1, 0]])
    assert bare.stream_listeners(0) == [(-1, 0)]
    bare.set_stream_listeners([0], [[-1, -1, -1]])          # without a table: the configuration, three times
    assert bare.stream_listeners(0) == [(-1, 0)] * 3 and bare.stream_listeners(1) == [(-1, 0)]
    bare.close()

    scorer = Engine()
    one, row = np.ones(1, np.int32), _lib.EwkListener(-1, 0)
    with pytest.raises(ValueError, match="no streams"):
        _lib.check(scorer._lib.ewk_stream_listeners_set(scorer.handle, _lib.i32ptr(np.zeros(1, np.int32)), 1,
                                                        _lib.i32ptr(one), C.byref(row), 1))
    scorer.close()


# ---- 7
def test_ticks_per_launch_follows_a_listeners_profile(template):
    """test_ticks_per_launch_follows_the_longest_profile with the 3.0 s profile reached only through
    listener 2 of each stream: 3 ticks per gate launch in a 4 s ring, and intact segments."""
    data = lu.streams(6, BLOCK, 9304, n_words=5)
    n_ticks = data.shape[1] // BLOCK
    long = [dict(speech_duration_max=3.0, post_speech_silence=0.5)]
    ref = [pc.run(data[i], pc.gate_config(-1, buffer_seconds=4, **long[0]), keep_audio=False) for i in range(6)]
    dflt = [pc.run(data[i], pc.gate_config(-1, buffer_seconds=4), keep_audio=False) for i in range(6)]
    assert sum(len(r) for r in ref) >= 10

    def run(step):
        eng = _engine(template, 6, table=False, buffer_seconds=4)
        eng.set_detector_profiles(long)
        eng.set_stream_listeners(np.arange(6, dtype=np.int32), [[-1, -1, 0]] * 6)
        assert (eng.stream_profiles() == -1).all()
        eng.profile(True)
        ev = _lockstep(eng, data, step=step)
        launches = eng.profile_read(2)[1]
        eng.close()
        return ev, launches

    ev40, l40 = run(40)
    ev1, l1 = run(1)
    assert l1 == n_ticks
    assert l40 == sum(-(-min(40, n_ticks - c) // 3) for c in range(0, n_ticks, 40))
    assert lu.assert_events_equal(lc.as_streams(ev1, 3), lc.as_streams(ev40, 3), 18) >= 10
    by = lc.by_listener(ev40, range(6), 3)
    for i in range(6):
        assert pc.engine_key(by[(i, 2)]) == pc.key(ref[i]), i
        assert pc.engine_key(by[(i, 0)]) == pc.engine_key(by[(i, 1)]) == pc.key(dflt[i]), i
