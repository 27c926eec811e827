"""The staging that tick pushes and chunk pushes share (pinned host samples -> device staging):
both regrow between pushes with no synchronisation in between, the two kinds of push alternating on
the same buffers.

Engine B gets 60 ticks of four streams as: push of 1 tick, push_many of 5, chunk pushes whose
packets grow from 160 to 11,200 samples per stream (18 blocks in all; streams start at different
phases of a block), push_many of 33 ticks (several gate launches; the 3 s ring allows 4 ticks a
launch) and one chunk of 3 blocks per stream -- every push but the last chunk larger than any
before it, nothing polled or read until the end.  A tick push to a stream with pending samples is
refused, so each chunk phase ends on whole blocks.  Engine A gets the same audio one tick at a time.
Bar: events (every field, the score's bits), thresholds, stream ticks and the whole ring content of
every stream equal A's.  Once with a float ring, once with an int16 ring (PCM16 pushes).
"""
import numpy as np
import pytest

import lifecycle_util as lu
import synth
from golden_io import matcher_fixture, template_arrays

pytestmark = pytest.mark.gpu

N, BLOCK, TICKS = 4, 1600, 60
# (seed, prefill seconds): the oracle gates one event per stream, at ticks 51, 56, 58 and 59 -- two
# inside the 33-tick push, two inside the last chunk push
STREAMS = [(901, 2.2), (905, 2.7), (902, 2.7), (906, 2.9)]
PACKETS = [160, 1440, 3200, 4800, 8000, 11200]          # 18 blocks; stream s moves 40 s samples from the 2nd to the 1st


def _audio():
    return np.stack([synth.make_stream(seed=seed, n_words=2, prefill=pre)[0][:TICKS * BLOCK] for seed, pre in STREAMS])


def _engine(template, pcm16):
    from easywakeword_amd import StreamEngine
    eng = StreamEngine(N, buffer_seconds=3, **(dict(ring_format=1) if pcm16 else {}))
    eng.set_template(*template)
    return eng


def _result(eng):
    ev = eng.poll()
    out = dict(ev=ev, thr=[eng.state(s)["silence_threshold"] for s in range(N)], ticks=eng.stream_ticks(),
               last=[eng.read_last(s, eng.ring_len) for s in range(N)])
    eng.close()
    return out


@pytest.mark.parametrize("pcm16", [False, True], ids=["f32_ring", "i16_ring"])
def test_staging_regrows_between_alternating_pushes(pcm16):
    fx, _ = matcher_fixture()
    template = template_arrays(fx)
    src = _audio()
    assert src.shape == (N, TICKS * BLOCK)
    if pcm16:
        src = lu.to_pcm16(src)[0]

    a = _engine(template, pcm16)
    for t in range(TICKS):
        (a.push_pcm16 if pcm16 else a.push)(src[:, t * BLOCK:(t + 1) * BLOCK])
    want = _result(a)

    b = _engine(template, pcm16)
    ticks, chunks = (b.push_pcm16, b.push_chunks_pcm16) if pcm16 else (b.push_many, b.push_chunks)
    at = np.zeros(N, np.int64)

    def tick_push(n_ticks, fn=ticks):
        assert (at == at[0]).all() and at[0] % BLOCK == 0
        fn(src[:, at[0]:at[0] + n_ticks * BLOCK])
        at[:] += n_ticks * BLOCK

    def chunk_push(counts):
        chunks(list(range(N)), [src[s, at[s]:at[s] + c] for s, c in enumerate(counts)])
        at[:] += counts

    tick_push(1, b.push_pcm16 if pcm16 else b.push)
    tick_push(5)
    for k, c in enumerate(PACKETS):
        shift = 40 * np.arange(N) * ((k == 0) - (k == 1))
        chunk_push(c + shift)
    assert not b.stream_pending().any()
    tick_push(33)
    chunk_push([3 * BLOCK] * N)
    assert (at == TICKS * BLOCK).all() and not b.stream_pending().any()
    got = _result(b)

    n = lu.assert_events_equal(want["ev"], got["ev"], N)
    assert n == len(want["ev"]) == len(got["ev"]) and n >= 3
    assert got["thr"] == want["thr"]
    np.testing.assert_array_equal(got["ticks"], want["ticks"])
    np.testing.assert_array_equal(got["ticks"], np.full(N, TICKS))
    for s in range(N):
        np.testing.assert_array_equal(got["last"][s], want["last"][s])
        assert len(got["last"][s]) == 3 * 16000
