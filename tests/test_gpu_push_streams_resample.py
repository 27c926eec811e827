"""Subset pushes and list resets with an input rate set (ewk_set_input_rate): the resampler's
history row and its "fresh" state (the first input_delay outputs are zero) belong to the stream.

Four streams at 48 kHz float32 / 44.1 kHz PCM16 / 12 kHz float32.  Engine A is pushed in
lockstep, engine B by a seeded subset schedule: events and rings are bit-identical.  Then streams 1 and 3 of B are reset
and fed what streams 0 and 2 heard from the start: they equal those streams of A, a fresh engine
-- the first input_delay zeros included -- while streams 0 and 2 of B keep their state.
"""
import numpy as np
import pytest

import lifecycle_util as lu
import synth
from golden_io import matcher_fixture, template_arrays

pytestmark = pytest.mark.gpu

BLOCK, OUT, N = 1600, 16000, 4
GATE = dict(buffer_seconds=2, pre_speech_silence=0.4, speech_duration_min=0.3, speech_duration_max=1.6,
            post_speech_silence=0.3, similarity_threshold=95.0)


def _input(rate, pcm16):
    from easywakeword_amd.audio import resample
    kinds = (["word", "white"], ["hp", "word"], ["word", "word"], ["tone880", "word"])
    pcms = [synth.make_stream(seed=5200 + i, n_words=2, prefill=2.5, kinds=k)[0] for i, k in enumerate(kinds)]
    L = min(len(p) for p in pcms) // BLOCK * BLOCK
    hi = np.stack([resample(p[:L], OUT, rate) for p in pcms]).astype(np.float32)
    ib = BLOCK * rate // OUT
    hi = hi[:, :hi.shape[1] // ib * ib]
    if pcm16:
        hi = lu.to_pcm16(hi)[0]
    return hi, ib


# (12 kHz upsamples 4/3 with a negative phase offset c0 = -2: the floor-division branch of k_resample;
# its band-limited streams give the oracle gate the same 8 events as the 48 kHz ones)
@pytest.mark.parametrize("rate,pcm16", [(48000, False), (44100, True), (12000, False)],
                         ids=["48k_f32", "44k1_pcm16", "12k_f32"])
def test_subset_schedule_and_list_reset_at_input_rate(rate, pcm16):
    from easywakeword_amd import StreamEngine
    tm, ts = template_arrays(matcher_fixture()[0])
    hi, ib = _input(rate, pcm16)
    n_ticks = hi.shape[1] // ib
    push, push_sub = ("push_pcm16", "push_streams_pcm16") if pcm16 else ("push_many", "push_streams")

    a = StreamEngine(N, **GATE)
    a.set_template(tm, ts)
    a.set_input_rate(rate)
    delay = a.input_delay
    assert delay > 0
    getattr(a, push)(hi[:, :ib])
    first_tick = [a.read_last(s, BLOCK) for s in range(N)]
    assert all(not f[:delay].any() and f[delay:].any() for f in first_tick)
    got = [a.poll()]
    for c in range(1, n_ticks, 3):
        getattr(a, push)(hi[:, c * ib:min(c + 3, n_ticks) * ib])
        got.append(a.poll())
    ev_a = np.concatenate(got)
    last_a = [a.read_last(s, 2 * BLOCK) for s in range(N)]
    thr_a = [a.state(s)["silence_threshold"] for s in range(N)]
    a.close()

    b = StreamEngine(N, **GATE)
    b.set_template(tm, ts)
    b.set_input_rate(rate)
    done = np.zeros(N, np.int64)
    got = []
    for sub, nt, first in lu.schedule(N, n_ticks, 21 + rate, max_ticks=3):
        getattr(b, push_sub)(sub, lu.rows_of(hi, sub, first, nt, ib))
        done[sub] += nt
        np.testing.assert_array_equal(b.stream_ticks(), done)
        got.append(b.poll())
    ev_b = np.concatenate(got)
    print(ev_a)
    assert lu.assert_events_equal(ev_a, ev_b, N) >= 4
    for s in range(N):
        np.testing.assert_array_equal(b.read_last(s, 2 * BLOCK), last_a[s], err_msg=f"ring {s}")
        assert b.state(s)["silence_threshold"] == thr_a[s]

    # streams 1 and 3 start again, on what streams 0 and 2 heard
    b.reset_streams([3, 1])
    for s in (1, 3):
        assert not b.read_last(s, 2 * BLOCK).any()
        assert b.state(s)["tick"] == 0
    b.push_streams_pcm16([3, 1], hi[[2, 0], :ib]) if pcm16 else b.push_streams([3, 1], hi[[2, 0], :ib])
    np.testing.assert_array_equal(b.read_last(1, BLOCK), first_tick[0])     # input_delay zeros, then the signal
    np.testing.assert_array_equal(b.read_last(3, BLOCK), first_tick[2])
    got = [b.poll()]
    for c in range(1, n_ticks, 3):
        getattr(b, push_sub)([3, 1], hi[[2, 0], c * ib:min(c + 3, n_ticks) * ib])
        got.append(b.poll())
    again = np.concatenate(got)
    want = ev_a[np.isin(ev_a["stream"], (0, 2))].copy()
    want["stream"] += 1
    assert lu.assert_events_equal(want, again, N) >= 2
    np.testing.assert_array_equal(b.stream_ticks(), [n_ticks] * N)
    for s, src in ((1, 0), (3, 2), (0, 0), (2, 2)):       # the reset two as a fresh engine, the others untouched
        np.testing.assert_array_equal(b.read_last(s, 2 * BLOCK), last_a[src], err_msg=f"ring {s}")
        assert b.state(s)["silence_threshold"] == thr_a[src]
    b.close()
