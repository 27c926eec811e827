"""k_gate_ticks over every launch family and summation-tree shape, tick by tick (GPU).

Every case of tests/gate_matrix.py: nine streams on one workgroup (EWK_GATE_GRID_MAX=1: four
waves, each walking two or three streams, so the register-resident arrays are reloaded between
streams), pushes of 1, 2, 3, 5, 7 and 13 ticks and one longer than the ticks-per-launch cap.

After every push, for every stream, against that stream's oracle at the same tick, with ==:
the threshold, last_silent and the FSM state (state()), the exported block-RMS array and its
sorted copy (the snapshot sections "block_rms" and "sorted": RMS values, the oracle's
block_rms()).  At the end: the event list, the ring's samples of the events still in it, and
the scores within the project's 1e-4 with equal decisions.  The family the engine reports
(ewk_gate_launch_info) must be the case's, so a change of the dispatch conditions fails here
instead of moving a case onto another kernel.
"""
import numpy as np
import pytest

import gate_matrix as gm
from golden_io import matcher_fixture, score_close, template_arrays
from oracle import mfcc_ref

pytestmark = pytest.mark.gpu

_seen = {}      # case -> the (rb, dma) its launches reported
MAX_BAD = 200


@pytest.fixture(scope="module")
def template():
    fx, _ = matcher_fixture()
    return template_arrays(fx)


def _block_rms(frame):
    frame = frame.astype(np.float64)
    return np.sqrt(np.mean(frame ** 2))


def _check_events(eng, case, data, got, listener, streams, traces, template, bad):
    """One listener's events of `streams` against the oracle's lists: identity, the ring's samples
    where it still holds them, scores and decisions.  Returns (events, scored, read back)."""
    tm, ts = template
    fs = case["block"]
    total = data.shape[1]
    n_ev = n_sc = n_rd = 0
    lj = (got["flags"] >> 16) & 15
    for s in streams:
        ref = traces[s].events
        mine = got[(got["stream"] == s) & (lj == listener)]
        mine = mine[np.argsort(mine["tick"], kind="stable")]
        key = [(int(m["tick"]), int(m["length"]), bool(m["flags"] & 1)) for m in mine]
        want = [(e.tick, e.length, e.skipped) for e in ref]
        if key != want:
            bad.append(dict(why="events", stream=s, listener=listener, got=key, want=want))
            continue
        for m, e in zip(mine, ref):
            n_ev += 1
            if m["time"] != e.time:
                bad.append(dict(why="time", stream=s, listener=listener, tick=e.tick, got=m["time"], want=e.time))
            if e.tick * fs - e.n_request >= total - gm.sample_ring(case) and e.length > 0:   # still in the ring
                back = eng.read_segment(s, int(m["ring_start"]), int(m["length"]))
                diff = np.flatnonzero(back != np.asarray(e.audio, np.float32))
                n_rd += 1
                if len(diff):
                    bad.append(dict(why="ring", stream=s, listener=listener, tick=e.tick, n_diff=len(diff),
                                    first=int(diff[0]), got=back[diff[:16]], want=e.audio[diff[:16]]))
            if e.skipped:
                continue
            cm, cs = mfcc_ref.extract_mfcc(e.audio)
            sc = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
            n_sc += 1
            if not score_close(float(m["score"]), sc, 1e-4) or bool(m["match"]) != (sc >= 75.0):
                bad.append(dict(why="score", stream=s, listener=listener, tick=e.tick, length=e.length,
                                got=float(m["score"]), match=int(m["match"]), want=sc))
    return n_ev, n_sc, n_rd


def run_case(name, template, monkeypatch, profiles=False, listeners=False):
    from easywakeword_amd import StreamEngine
    from evidence import dump
    case = gm.CASES[name]
    n, fs, nb = gm.N_STREAMS, case["block"], gm.n_blocks(case)
    src, data = gm.signals(name)
    n_ticks = src.shape[1] // fs
    assign = [i % len(gm.PROFILES) for i in range(n)] if profiles else None
    tr = gm.traces(name, assign)
    lsn_streams = list(range(0, n, 2)) if listeners else []
    tr1 = gm.traces(name, [gm.LISTENER_PROFILES[1]] * n) if listeners else None

    monkeypatch.setenv("EWK_GATE_GRID_MAX", "1")
    eng = StreamEngine(n, **gm.engine_config(case))
    eng.set_template(*template)
    if profiles or listeners:
        eng.set_detector_profiles(gm.PROFILES)
    if profiles:
        eng.assign_stream_profiles(np.arange(n, dtype=np.int32), np.array(assign, np.int32))
    if listeners:
        eng.set_stream_listeners(lsn_streams, [[(p, 0) for p in gm.LISTENER_PROFILES]] * len(lsn_streams))
    want_info = dict(rb=case["rb"], dma=case["dma"], prof=int(profiles or listeners), lsn=int(listeners),
                     block_tree_kind=case["tree"], last_tree_kind=2)
    assert eng.snapshot_layout()["n_blocks"] == nb
    push = eng.push_pcm16 if case["input"] == "pcm16" else eng.push_many
    all_streams = list(range(n))
    exp = np.zeros((n, nb))
    # a compact ring keeps each block's RMS from its first write (block b is tick b's samples: the
    # oracle's expression on them); every other ring exports zeros until it is full
    pre = np.zeros((n, nb))
    bad, got, t = [], [], 0
    full_at = tr[0].full_at
    try:
        for nt in gm.push_schedule(case, n_ticks):
            push(src[:, t * fs:(t + nt) * fs])
            info = eng.gate_launch_info()
            assert info == want_info, (name, t, info, want_info)
            got.append(eng.poll())
            snap = eng.export_streams(all_streams)
            rms = np.ascontiguousarray(snap.section("block_rms")).view(np.float64)
            srt = np.ascontiguousarray(snap.section("sorted")).view(np.float64)
            for s in all_streams:
                for tt in range(t, t + nt):
                    for b, v in tr[s].updates[tt]:
                        exp[s, b] = v
                    if case["compact"] and tt < nb:
                        pre[s, tt] = _block_rms(data[s, tt * fs:(tt + 1) * fs])
            t += nt
            full = t >= full_at
            want_rms = exp if full else pre
            want_srt = np.sort(exp, axis=1) if full else np.zeros_like(exp)
            for s in all_streams:
                o, st = tr[s], eng.state(s)
                rec = dict(stream=s, tick=t)
                if st["tick"] != t or bool(st["started"]) != bool(o.started[t - 1]):
                    bad.append(dict(rec, why="clock", got=(st["tick"], st["started"]), want=(t, bool(o.started[t - 1]))))
                if st["silence_threshold"] != o.threshold[t - 1]:
                    bad.append(dict(rec, why="threshold", got=st["silence_threshold"], want=o.threshold[t - 1]))
                if o.started[t - 1] and (bool(st["last_silent"]) != bool(o.silent[t - 1]) or st["state"] != o.state[t - 1]):
                    bad.append(dict(rec, why="fsm", got=(st["last_silent"], st["state"]),
                                    want=(bool(o.silent[t - 1]), int(o.state[t - 1]))))
                if s in lsn_streams and tr1[s].started[t - 1]:
                    l1 = eng.listener_state(s, 1)
                    if l1["state"] != tr1[s].state[t - 1]:
                        bad.append(dict(rec, why="listener fsm", got=l1["state"], want=int(tr1[s].state[t - 1])))
                if not np.array_equal(rms[s], want_rms[s]):
                    d = np.flatnonzero(rms[s] != want_rms[s])
                    bad.append(dict(rec, why="block_rms", n_diff=len(d), blocks=d[:8], got=rms[s][d[:8]],
                                    want=want_rms[s][d[:8]]))
                if not np.array_equal(srt[s], want_srt[s]):
                    d = np.flatnonzero(srt[s] != want_srt[s])
                    bad.append(dict(rec, why="sorted", n_diff=len(d), ranks=d[:8], got=srt[s][d[:8]],
                                    want=want_srt[s][d[:8]]))
            if len(bad) >= MAX_BAD:
                break
        got = np.concatenate(got)
        counts = (0, 0, 0)
        if len(bad) < MAX_BAD:
            counts = _check_events(eng, case, data, got, 0, all_streams, tr, template, bad)
            if listeners:
                c1 = _check_events(eng, case, data, got, 1, lsn_streams, tr1, template, bad)
                counts = tuple(a + b for a, b in zip(counts, c1))
                lj = (got["flags"] >> 16) & 15
                assert not ((lj > 1) | ((lj == 1) & ~np.isin(got["stream"], lsn_streams))).any()
    finally:
        eng.close()
    if bad:
        path = dump("gate_matrix_" + name, dict(case=name, profiles=profiles, listeners=listeners, bad=bad))
        pytest.fail(f"{name}: {len(bad)} mismatches (evidence {path}): {bad[:3]}")
    assert t == n_ticks
    n_ev, n_sc, n_rd = counts
    assert n_ev >= 3 * n
    if case["buffer_seconds"] > 1:     # (the 1 s ring may have dropped every stream's last event by the end)
        assert n_rd >= 1
    if name != "e_8192":     # (every event of the 0.512 s tick is skipped: gate_matrix's docstring)
        assert n_sc >= 3
    return (want_info["rb"], want_info["dma"])


@pytest.mark.parametrize("name", list(gm.CASES))
def test_case(name, template, monkeypatch):
    _seen[name] = run_case(name, template, monkeypatch)


@pytest.mark.parametrize("name", gm.PROFILE_CASES)
def test_case_with_detector_profiles(name, template, monkeypatch):
    """Three profiles round-robin: each stream's oracle runs with its profile's timings (PROF families)."""
    run_case(name, template, monkeypatch, profiles=True)


@pytest.mark.parametrize("name", gm.LISTENER_CASES)
def test_case_with_listeners(name, template, monkeypatch):
    """Two listeners -- the engine's timings and profile 1 -- on every second stream (LSN families)."""
    run_case(name, template, monkeypatch, listeners=True)


def test_every_reachable_family_ran():
    """The union of the families the cases reported: both register families with each of the four
    sample paths, and the global-memory family."""
    missing = [n for n in gm.CASES if n not in _seen]
    assert not missing, f"cases that did not pass before this check (run the whole module): {missing}"
    assert sorted(set(_seen.values())) == [(0, 0), (2, 0), (2, 1), (2, 2), (2, 3), (8, 0), (8, 1), (8, 2), (8, 3)]
