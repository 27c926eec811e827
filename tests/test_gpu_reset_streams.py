"""List reset (ewk_reset_stream_list): the listed streams become streams of a new engine, the
others never notice.

Twelve streams (the recipe of test_gpu_compact_ring.py).  After about half the audio: poll, then
reset_streams([2, 5]).  Right after it streams 2 and 5 show the state of a new engine and a zero
ring.  They are then fed other audio from its start through subset pushes while the other ten
continue theirs.  Bar: streams 2 and 5 equal a fresh engine on the new audio -- events with ticks
from 1, the score's bits, threshold, ring -- and the oracle; the other ten equal the lockstep run
bit for bit.
"""
import numpy as np
import pytest

import lifecycle_util as lu
from golden_io import matcher_fixture, score_close, template_arrays
from oracle import mfcc_ref
from oracle.gate_ref import GateConfig, run_stream

pytestmark = pytest.mark.gpu

N, BLOCK = 12, 1600
RESET = [2, 5]


@pytest.fixture(scope="module")
def template():
    fx, _ = matcher_fixture()
    return template_arrays(fx)


def _lockstep(n, src, pcm16, template, cfg):
    from easywakeword_amd import StreamEngine
    eng = StreamEngine(n, **cfg)
    eng.set_template(*template)
    got = []
    for c in range(0, src.shape[1], 7 * BLOCK):
        (eng.push_pcm16 if pcm16 else eng.push_many)(src[:, c:c + 7 * BLOCK])
        got.append(eng.poll())
    out = dict(ev=np.concatenate(got), thr=[eng.state(i)["silence_threshold"] for i in range(n)],
               last=[eng.read_last(i, 4 * BLOCK) for i in range(n)])
    eng.close()
    return out


@pytest.mark.parametrize("ring", ["f32_full", "i16_compact"])
def test_reset_two_streams_mid_run(ring, template):
    """float32 full ring (640,000-byte rows, 20 zeroing workgroups each) / int16 compact ring."""
    from easywakeword_amd import StreamEngine
    pcm16 = ring == "i16_compact"
    cfg = dict(ring_format=1, ring_samples=lu.min_ring(BLOCK)) if pcm16 else {}
    data = lu.streams(N, BLOCK, 7000 + BLOCK)
    fresh = lu.streams(2, BLOCK, 8100, n_words=2)         # what streams 2 and 5 hear after the reset
    src, new = data, fresh
    if pcm16:
        src, data = lu.to_pcm16(data)
        new, fresh = lu.to_pcm16(fresh)
    n_ticks, half = data.shape[1] // BLOCK, data.shape[1] // BLOCK // 2
    n_new = new.shape[1] // BLOCK      # (longer than what is left of the ten: the two finish alone)
    assert n_new >= 150 and n_new > n_ticks - half
    a = _lockstep(N, src, pcm16, template, cfg)
    f = _lockstep(2, new[:, :n_new * BLOCK], pcm16, template, cfg)
    push, push_sub = ("push_pcm16", "push_streams_pcm16") if pcm16 else ("push_many", "push_streams")

    eng = StreamEngine(N, **cfg)
    eng.set_template(*template)
    got = []
    for c in range(0, half, 7):
        getattr(eng, push)(src[:, c * BLOCK:min(c + 7, half) * BLOCK])
        got.append(eng.poll())
    before = np.concatenate(got)
    assert eng.state(2)["samples_collected"] == 160000 and eng.state(5)["started"] == 1
    eng.reset_streams(RESET)
    for s in RESET:
        st = eng.state(s)
        assert (st["samples_collected"], st["started"], st["tick"], st["pointer"]) == (0, 0, 0, 0), st
        assert st["silence_threshold"] == eng.config.initial_threshold
        assert not eng.read_last(s, 4 * BLOCK).any()
        assert not eng.read_segment(s, 0, eng.sample_ring).any()
    want_ticks = np.full(N, half)
    want_ticks[RESET] = 0
    np.testing.assert_array_equal(eng.stream_ticks(), want_ticks)
    assert eng.state(3)["tick"] == half

    # the ten go on in subset pushes of their own, the two start the new audio
    rest = np.array([i for i in range(N) if i not in RESET], np.int32)
    got = []
    for c in range(0, n_new, 5):
        if c < n_ticks - half:
            nt = min(5, n_ticks - half - c)
            getattr(eng, push_sub)(rest, src[rest, (half + c) * BLOCK:(half + c + nt) * BLOCK])
        k = min(5, n_new - c)
        getattr(eng, push_sub)(RESET[::-1], new[::-1, c * BLOCK:(c + k) * BLOCK])
        got.append(eng.poll())
    after = np.concatenate(got)
    want_ticks[:] = n_ticks
    want_ticks[RESET] = n_new
    np.testing.assert_array_equal(eng.stream_ticks(), want_ticks)

    # the other ten: the lockstep run, bit for bit
    mask = lambda ev, keep: ev[np.isin(ev["stream"], keep)]
    mine = np.concatenate([mask(before, rest), mask(after, rest)])
    n_rest = lu.assert_events_equal(mask(a["ev"], rest), mine, N)
    for i in rest:
        assert eng.state(int(i))["silence_threshold"] == a["thr"][i]
        np.testing.assert_array_equal(eng.read_last(int(i), 4 * BLOCK), a["last"][i])
    # streams 2 and 5: a fresh engine on the new audio (its streams 0 and 1), and the oracle
    re_ev = mask(after, RESET).copy()
    re_ev["stream"] = np.where(re_ev["stream"] == RESET[0], 0, 1)
    n_new_ev = lu.assert_events_equal(f["ev"], re_ev, 2)
    tm, ts = template
    n_sc = 0
    for j, s in enumerate(RESET):
        assert eng.state(s)["silence_threshold"] == f["thr"][j]
        np.testing.assert_array_equal(eng.read_last(s, 4 * BLOCK), f["last"][j])
        ref = run_stream(fresh[j, :n_new * BLOCK], GateConfig()).events
        got_s = lu.by_stream(re_ev, 2)[j]
        assert [(int(m["tick"]), int(m["length"]), bool(m["flags"] & 1)) for m in got_s] == \
               [(e.tick, e.length, e.skipped) for e in ref], s
        for m, e in zip(got_s, ref):
            if e.skipped:
                continue
            cm, cs = mfcc_ref.extract_mfcc(e.audio)
            sc = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
            print(f"stream {s} tick {e.tick}: score {float(m['score'])!r} oracle {sc!r}")
            assert score_close(float(m["score"]), sc, 1e-4), (s, e.tick, float(m["score"]), sc)
            n_sc += 1
    print(n_rest, n_new_ev, n_sc)
    assert n_rest > 10 and n_new_ev >= 2 and n_sc >= 2
    eng.close()
