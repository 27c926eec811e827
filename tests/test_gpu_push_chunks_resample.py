"""Chunk pushes with an input rate set (ewk_set_input_rate): chunks are counted in input samples,
the carry holds input samples (float32: PCM16 is decoded on append), and every group of the push
goes through the resampler with its streams' history rows.

The four streams, gate settings and rates of test_gpu_push_streams_resample.py: 48 kHz float32,
44.1 kHz PCM16, 12 kHz float32.  Engine A is pushed in lockstep, engine B by a seeded chunk
schedule whose sizes include in_block - 1, in_block and in_block + 1: events and rings are
bit-identical.
"""
import numpy as np
import pytest

import chunk_util as cu
import lifecycle_util as lu
import test_gpu_push_streams_resample as psr
from golden_io import matcher_fixture, template_arrays

pytestmark = pytest.mark.gpu

BLOCK, N, GATE = psr.BLOCK, psr.N, psr.GATE


@pytest.mark.parametrize("rate,pcm16", [(48000, False), (44100, True), (12000, False)],
                         ids=["48k_f32", "44k1_pcm16", "12k_f32"])
def test_chunk_schedule_at_input_rate(rate, pcm16):
    from easywakeword_amd import StreamEngine
    tm, ts = template_arrays(matcher_fixture()[0])
    hi, ib = psr._input(rate, pcm16)
    n_ticks = hi.shape[1] // ib

    a = StreamEngine(N, **GATE)
    a.set_template(tm, ts)
    a.set_input_rate(rate)
    got = []
    for c in range(0, n_ticks, 3):
        (a.push_pcm16 if pcm16 else a.push_many)(hi[:, c * ib:min(c + 3, n_ticks) * ib])
        got.append(a.poll())
    ev_a = np.concatenate(got)
    last_a = [a.read_last(s, 2 * BLOCK) for s in range(N)]
    thr_a = [a.state(s)["silence_threshold"] for s in range(N)]
    a.close()

    b = StreamEngine(N, **GATE)
    b.set_template(tm, ts)
    b.set_input_rate(rate)
    assert b.input_block == ib
    size_set = [0, 1, ib // 5, ib // 2 + 1, ib - 1, ib, ib + 1, 2 * ib + 7, 4 * ib]
    sched = cu.schedule(N, hi.shape[1], ib, 41 + rate, size_set=size_set)
    ev_b, delivered = cu.run(b, hi, ib, sched, "host", pcm16)
    assert (delivered == hi.shape[1]).all()
    print(ev_a)
    assert lu.assert_events_equal(ev_a, ev_b, N) >= 4
    for s in range(N):
        np.testing.assert_array_equal(b.read_last(s, 2 * BLOCK), last_a[s], err_msg=f"ring {s}")
        assert b.state(s)["silence_threshold"] == thr_a[s]
    b.close()
