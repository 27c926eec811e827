"""Subset pushes (ewk_push_streams): every stream on its own clock.

Engine A gets 12 streams in lockstep (push_many, 7 ticks a call).  Engine B gets the same audio
by a seeded random schedule (lifecycle_util.schedule): subsets of 1, 6, 11 or 12 streams in
shuffled order, 1..7 ticks a push, every stream's blocks in order.  Bar: per stream, every event
field and the score's bits equal between A and B, every final threshold and ring equal, the event
list equal to the oracle's (oracle/gate_ref.run_stream on that stream alone), scores within 1e-4
of the oracle (the project's bar), and stream_ticks() equal to the delivered counts after every
push.  Streams and seeds are those of test_gpu_compact_ring.py (more than 20 events each).
"""
import numpy as np
import pytest

import lifecycle_util as lu
from golden_io import matcher_fixture, score_close, template_arrays
from oracle import mfcc_ref
from oracle.gate_ref import GateConfig, normalize_level3, run_stream

pytestmark = pytest.mark.gpu

N = 12
CONFIGS = {
    # name: (block, pcm16 pushes, engine config)
    "b1600_f32": (1600, False, {}),
    "b1600_i16_compact": (1600, True, dict(ring_format=1, ring_samples=lu.min_ring(1600))),
    "b400_f32": (400, False, {}),
}


@pytest.fixture(scope="module")
def template():
    fx, _ = matcher_fixture()
    return template_arrays(fx)


_cache = {}


def _case(name, template):
    """Per configuration, computed once: the streams (float32 values, and int16 when pushed as
    PCM16), the oracle's events with the scores of the first 12 scored ones, and engine A's run."""
    if name in _cache:
        return _cache[name]
    from easywakeword_amd import StreamEngine
    block, pcm16, cfg = CONFIGS[name]
    data = lu.streams(N, block, 7000 + block)
    q = None
    if pcm16:
        q, data = lu.to_pcm16(data)
    tm, ts = template
    ref, want = [], {}
    for i in range(N):
        evs = run_stream(data[i], GateConfig(block=block, tick_seconds=block / 16000)).events
        ref.append(evs)
        for e in evs:
            if not e.skipped and len(want) < 12:
                cm, cs = mfcc_ref.extract_mfcc(e.audio)
                want[(i, e.tick)] = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
    eng = StreamEngine(N, block=block, tick_seconds=block / 16000, **cfg)
    eng.set_template(tm, ts)
    src = q if pcm16 else data
    got = []
    for c in range(0, src.shape[1], 7 * block):
        (eng.push_pcm16 if pcm16 else eng.push_many)(src[:, c:c + 7 * block])
        got.append(eng.poll())
    a = dict(ev=np.concatenate(got), thr=[eng.state(i)["silence_threshold"] for i in range(N)],
             last=[eng.read_last(i, 4 * block) for i in range(N)])
    eng.close()
    _cache[name] = dict(block=block, pcm16=pcm16, cfg=cfg, data=data, src=src, ref=ref, want=want, a=a)
    return _cache[name]


def _check_oracle(ev, case, upto=None):
    """The event list of every stream equals the oracle's (those up to tick upto[i]); scores of
    the events the case holds an oracle score for are within 1e-4.  Returns (events, scores)."""
    n_ev = n_sc = 0
    for i, mine in enumerate(lu.by_stream(ev, N)):
        ref = [e for e in case["ref"][i] if upto is None or e.tick <= upto[i]]
        assert [(int(m["tick"]), int(m["length"]), bool(m["flags"] & 1)) for m in mine] == \
               [(e.tick, e.length, e.skipped) for e in ref], i
        for m, e in zip(mine, ref):
            assert float(m["time"]) == e.time
            s = case["want"].get((i, e.tick))
            if s is not None:
                print(f"stream {i} tick {e.tick}: score {float(m['score'])!r} oracle {s!r}")
                assert score_close(float(m["score"]), s, 1e-4), (i, e.tick, float(m["score"]), s)
                assert bool(m["match"]) == (s >= 75.0)
                n_sc += 1
        n_ev += len(mine)
    return n_ev, n_sc


def _device_buffer(rows, nt, block, stride, dtype):
    """The rows of one push in device memory with `stride` samples between them (gaps hold a value
    no tick holds, so a read from a gap shows in the ring and the events)."""
    import torch
    buf = np.full(len(rows) * stride, 9, dtype)
    for i, r in enumerate(rows):
        buf[i * stride:i * stride + nt * block] = r
    return torch.from_numpy(buf).to(torch.device("cuda", 0))


def _run_schedule(case, template, seed, where, stride_pad=0, stop_after=None):
    """Engine B: the schedule's pushes through push_streams / push_streams_pcm16 (where="host") or
    push_streams_device; stream_ticks() checked after every push.  Returns the engine, its events
    and the ticks delivered per stream."""
    from easywakeword_amd import StreamEngine
    block, pcm16 = case["block"], case["pcm16"]
    src = case["src"]
    eng = StreamEngine(N, block=block, tick_seconds=block / 16000, **case["cfg"])
    eng.set_template(*template)
    done = np.zeros(N, np.int64)
    got = []
    sched = lu.schedule(N, src.shape[1] // block, seed)
    for k, (sub, nt, first) in enumerate(sched[:stop_after]):
        rows = lu.rows_of(src, sub, first, nt, block)
        if where == "host":
            (eng.push_streams_pcm16 if pcm16 else eng.push_streams)(sub, rows)
        else:
            stride = nt * block + stride_pad
            buf = _device_buffer(rows, nt, block, stride, src.dtype)
            eng.push_streams_device(sub, buf.data_ptr(), stride, block, nt, pcm16=pcm16)
        done[sub] += nt
        np.testing.assert_array_equal(eng.stream_ticks(), done)
        np.testing.assert_array_equal(eng.stream_ticks(sub[:2]), done[sub[:2]])
        got.append(eng.poll())     # (also keeps the device buffer alive until the push has run)
    return eng, np.concatenate(got), done


def _compare_with_lockstep(case, eng, ev):
    a = case["a"]
    n = lu.assert_events_equal(a["ev"], ev, N)
    assert n > 20
    assert [eng.state(i)["silence_threshold"] for i in range(N)] == a["thr"]
    for i in range(N):
        np.testing.assert_array_equal(eng.read_last(i, 4 * case["block"]), a["last"][i], err_msg=f"ring {i}")
    n_ev, n_sc = _check_oracle(ev, case)
    assert n_ev > 20 and n_sc >= 10


def test_b1600_f32_host(template):
    """launch_gate branch <2, 2>: 100 blocks, float32 rows 16-B aligned (the host staging), LDS-DMA
    in 16-B pieces."""
    case = _case("b1600_f32", template)
    eng, ev, _ = _run_schedule(case, template, 11, "host")
    _compare_with_lockstep(case, eng, ev)
    eng.close()


def test_b1600_f32_device_aligned(template):
    """launch_gate branch <2, 2> with pcm in device memory (stride = n_ticks * block)."""
    case = _case("b1600_f32", template)
    eng, ev, _ = _run_schedule(case, template, 12, "device")
    _compare_with_lockstep(case, eng, ev)
    eng.close()


def test_b1600_f32_device_unaligned_rows(template):
    """launch_gate branch <2, 1>: stride = n_ticks * block + 1 through push_streams_device (block
    + 1 for one tick), rows not 16-B aligned, LDS-DMA in 4-B pieces."""
    case = _case("b1600_f32", template)
    eng, ev, _ = _run_schedule(case, template, 13, "device", stride_pad=1)
    _compare_with_lockstep(case, eng, ev)
    eng.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_b1600_pcm16_into_compact_i16_ring(where, template):
    """launch_gate branch <2, 3>: PCM16 pushes, 16-B pieces, into an EWK_RING_I16 compact ring."""
    case = _case("b1600_i16_compact", template)
    eng, ev, _ = _run_schedule(case, template, 14, where)
    _compare_with_lockstep(case, eng, ev)
    eng.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_b400_f32(where, template):
    """launch_gate branch <8, 2>: block 400, 400 blocks (block RMSs in 8 registers per lane)."""
    case = _case("b400_f32", template)
    eng, ev, _ = _run_schedule(case, template, 15, where)
    _compare_with_lockstep(case, eng, ev)
    eng.close()


def test_full_push_on_a_desynchronised_engine(template):
    """After a few subset pushes, push_many to all streams continues every stream's own clock
    (branch <2, 2>, own clock, no index list): the oracle's events up to each stream's tick."""
    case = _case("b1600_f32", template)
    block, data = case["block"], case["data"]
    eng, ev0, done = _run_schedule(case, template, 16, "host", stop_after=9)
    assert len(set(done.tolist())) > 1, done
    got = [ev0]
    n_ticks = data.shape[1] // block
    while done.max() + 7 <= n_ticks:
        eng.push_many(lu.rows_of(data, np.arange(N), done, 7, block))
        done += 7
        np.testing.assert_array_equal(eng.stream_ticks(), done)
        got.append(eng.poll())
    assert [eng.state(i)["tick"] for i in range(N)] == done.tolist()
    n_ev, n_sc = _check_oracle(np.concatenate(got), case, upto=done)
    assert n_ev > 20 and n_sc >= 10
    eng.close()


def test_validation_changes_nothing(template):
    """A bad list or row count raises ValueError before anything is enqueued or changed: ticks,
    and the events of the next poll, are those of the valid pushes alone."""
    from easywakeword_amd import StreamEngine
    case = _case("b1600_f32", template)
    block, data = case["block"], case["data"]
    eng = StreamEngine(N, block=block, tick_seconds=block / 16000)
    eng.set_template(*template)
    sub = np.array([3, 0, 7], np.int32)
    done = np.zeros(N, np.int64)

    def good(nt):
        eng.push_streams(sub, lu.rows_of(data, sub, done[sub], nt, block))
        done[sub] += nt

    good(5)
    rows = lu.rows_of(data, sub, done[sub], 2, block)
    bad = [([3, 0, 3], rows, "twice"), ([3, -1, 7], rows, "outside"), ([3, N, 7], rows, "outside"),
           ([], rows[:0], "1.."), ([3, 0], rows, "len"), ([3, 0, 7, 1], rows, "len")]
    for lst, r, word in bad:
        with pytest.raises(ValueError, match=word):
            eng.push_streams(lst, r)
        np.testing.assert_array_equal(eng.stream_ticks(), done)
    for lst in ([3, 3], [-1], [N], []):
        with pytest.raises(ValueError):
            eng.reset_streams(lst)
        with pytest.raises(ValueError):
            eng.push_streams_device(lst, 0, block)      # (refused before the pointer is looked at)
        np.testing.assert_array_equal(eng.stream_ticks(), done)
    with pytest.raises(ValueError):
        eng.stream_ticks([N])
    for nt in (7,) * 20:
        good(nt)
    ev = eng.poll()
    assert [eng.state(int(s))["tick"] for s in sub] == done[sub].tolist()
    assert set(ev["stream"].tolist()) <= set(sub.tolist())
    for i in sub:
        mine = ev[ev["stream"] == i]
        ref = [e for e in case["ref"][i] if e.tick <= done[i]]
        assert [(int(m["tick"]), int(m["length"])) for m in mine] == [(e.tick, e.length) for e in ref], i
    assert len(ev) >= 1
    eng.close()


def test_normalize_events_uses_the_streams_own_tick(template):
    """An event polled from a lagging stream while the others are hundreds of ticks ahead gives the
    oracle's normalised segment; once that stream alone has passed its ring it is refused."""
    from easywakeword_amd import StreamEngine
    from easywakeword_amd._lib import RingOverwrittenError
    case = _case("b1600_f32", template)
    block, data = case["block"], case["data"]
    n_ticks = data.shape[1] // block
    lag = next(i for i in range(3) if any(not e.skipped and e.tick + 101 <= n_ticks for e in case["ref"][i]))
    ref = next(e for e in case["ref"][lag] if not e.skipped and e.tick + 101 <= n_ticks)
    others = np.array([i for i in range(3) if i != lag], np.int32)
    eng = StreamEngine(3, block=block, tick_seconds=block / 16000)
    eng.set_template(*template)
    for _ in range(2):        # the other two: the whole audio twice, > 200 ticks ahead of the cut
        eng.push_streams(others, data[others])
    assert 2 * n_ticks >= 200
    eng.poll()
    eng.push_streams([lag], data[lag:lag + 1, :ref.tick * block])
    ev = eng.poll()
    mine = ev[(ev["stream"] == lag) & (ev["tick"] == ref.tick)]
    assert len(mine) == 1
    np.testing.assert_array_equal(eng.stream_ticks(), [ref.tick if i == lag else 2 * n_ticks for i in range(3)])
    out = eng.normalize_events(mine)
    np.testing.assert_array_equal(out[0], normalize_level3(ref.audio))
    eng.push_streams(others, data[others, :50 * block])      # the others moving on changes nothing
    np.testing.assert_array_equal(eng.normalize_events(mine)[0], out[0])
    eng.push_streams([lag], data[lag:lag + 1, ref.tick * block:(ref.tick + 101) * block])
    with pytest.raises(RingOverwrittenError):
        eng.normalize_events(mine)
    eng.close()
