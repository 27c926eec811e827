"""Chunk pushes beside everything else a stream can carry -- the stream bank, a detector-profile
table, listeners -- and the rules around them: validation that changes nothing, tick pushes
refused while samples are pending, resets and a new input rate dropping them."""
import numpy as np
import pytest

import bank_cases as bc
import chunk_util as cu
import lifecycle_util as lu
import listener_cases as lc
import profile_cases as pc
import test_gpu_push_streams as ps
from golden_io import matcher_fixture, template_arrays

pytestmark = pytest.mark.gpu

N, BLOCK = pc.N, pc.BLOCK


@pytest.fixture(scope="module")
def template():
    fx, _ = matcher_fixture()
    return template_arrays(fx)


def _mixed_engine(template):
    """12 streams: a profile per stream, the stream bank with two words, five listeners on stream
    0 and two on streams 1 and 3."""
    from easywakeword_amd import StreamEngine
    eng = StreamEngine(N)
    eng.set_template(*template)
    eng.set_detector_profiles(pc.PROFILES)
    eng.assign_stream_profiles(np.arange(N, dtype=np.int32), pc.assignment())
    eng.bank_from_pcm(bc.bank_audio()[:2], thresholds=bc.THRESHOLDS[:2])
    eng.set_stream_bank(np.arange(N, dtype=np.int32) % 2)
    eng.set_stream_listeners([0, 1, 3], [lc.rows(lc.LISTENERS, [0, 1, 0, 1, 0]), lc.rows((-1, 3), (0, 1)),
                                         lc.rows((2, 0), (1, 1))])
    return eng


def test_chunks_with_bank_profiles_and_listeners(template):
    from easywakeword_amd import _lib
    data = pc.main_case()["data"]
    a = _mixed_engine(template)
    got = []
    for c in range(0, data.shape[1], 7 * BLOCK):
        a.push_many(data[:, c:c + 7 * BLOCK])
        got.append(a.poll())
    ev_a = np.concatenate(got)
    a.close()
    b = _mixed_engine(template)
    ev_b, delivered = cu.run(b, data, BLOCK, cu.schedule(N, data.shape[1], BLOCK, 51))
    assert (delivered == data.shape[1]).all()
    b.close()
    n = lu.assert_events_equal(lc.as_streams(ev_a, 16), lc.as_streams(ev_b, 16), 16 * N)     # flags: bank and best template too
    assert n == len(ev_a) == len(ev_b) and n > 20
    np.testing.assert_array_equal(np.sort(ev_a["flags"]), np.sort(ev_b["flags"]))
    scored = ev_b[(ev_b["flags"] & _lib.EWK_EV_SKIPPED) == 0]
    assert len(scored) >= 10 and ((scored["flags"] & _lib.EWK_EV_BANK) != 0).all()
    assert (lc.listener_of(ev_b) > 0).sum() >= 4


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def test_validation_changes_nothing(template):
    """Each bad call raises ValueError before anything is enqueued or changed: ticks, pending and
    the events of the next poll are those of the valid pushes alone."""
    from easywakeword_amd import StreamEngine
    case = ps._case("b1600_f32", template)
    data = case["data"]
    eng = StreamEngine(ps.N, block=BLOCK, tick_seconds=0.1)
    eng.set_template(*template)
    sub = [3, 0, 7]
    done = np.zeros(ps.N, np.int64)

    def good(counts):
        eng.push_chunks(sub, [data[s, done[s]:done[s] + c] for s, c in zip(sub, counts)])
        done[sub] += counts

    def unchanged():
        np.testing.assert_array_equal(eng.stream_ticks(), done // BLOCK)
        np.testing.assert_array_equal(eng.stream_pending(), done % BLOCK)

    good([5 * BLOCK + 100, 700, 3 * BLOCK])
    unchanged()
    chunk = data[0, :2000]
    buf = _device(data[0, :8000])
    M = 64 * BLOCK
    bad_host = [([3, 0, 3], [chunk] * 3, "twice"), ([3, -1, 7], [chunk] * 3, "outside"),
                ([3, ps.N, 7], [chunk] * 3, "outside"), ([], [], "1.."), ([3, 0], [chunk] * 3, "chunks given"),
                ([5], [np.zeros(M + 1, np.float32)], r"counts\[0\] = %d is outside" % (M + 1))]
    for lst, chunks, word in bad_host:
        with pytest.raises(ValueError, match=word):
            eng.push_chunks(lst, chunks)
        unchanged()
    bad_dev = [([3, 0], [0, 100], [100, -1], r"counts\[1\] = -1 is outside"),          # a negative count
               ([3, 0], [0, 100], [100, M + 1], r"counts\[1\] = %d is outside" % (M + 1)),   # over the maximum
               ([3, 0], [0, 7000], [100, 1001], "chunk 1 .*is outside pcm"),           # past n_pcm
               ([3, 0], [-1, 0], [100, 100], "chunk 0 .*is outside pcm"),
               ([3, 3], [0, 0], [1, 1], "twice"), ([ps.N], [0], [1], "outside"), ([], [], [], "1..")]
    for lst, offs, counts, word in bad_dev:
        with pytest.raises(ValueError, match=word):
            eng.push_chunks_device(lst, buf.data_ptr(), 8000, offs, counts)
        unchanged()
    with pytest.raises(ValueError):
        eng.stream_pending([ps.N])
    for _ in range(24):       # stream 3 to tick 173, past its first event
        good([7 * BLOCK - 1, 2 * BLOCK + 1, 3 * BLOCK])
    assert done.max() <= data.shape[1]
    unchanged()
    ev = eng.poll()
    assert [eng.state(s)["tick"] for s in sub] == (done[sub] // BLOCK).tolist()
    assert set(ev["stream"].tolist()) <= set(sub)
    for i in sub:
        mine = ev[ev["stream"] == i]
        ref = [e for e in case["ref"][i] if e.tick <= done[i] // BLOCK]
        assert [(int(m["tick"]), int(m["length"])) for m in mine] == [(e.tick, e.length) for e in ref], i
    assert len(ev) >= 1
    eng.close()


def test_pending_samples_refuse_tick_pushes_and_resets_drop_them(template):
    from easywakeword_amd import StreamEngine
    case = ps._case("b1600_f32", template)
    data, a = case["data"], case["a"]
    n_ticks = data.shape[1] // BLOCK
    eng = StreamEngine(ps.N, block=BLOCK, tick_seconds=0.1)
    eng.set_template(*template)
    assert not eng.stream_pending().any()                     # before any chunk push: nothing allocated, nothing pending
    eng.push_chunks([3, 5], [data[3, :2 * BLOCK + 100], data[5, :BLOCK]])
    np.testing.assert_array_equal(eng.stream_pending([3, 5]), [100, 0])
    rows = data[[3, 5], :BLOCK]
    with pytest.raises(ValueError, match="stream 3 holds 100 pending"):
        eng.push_streams([5, 3], rows)
    with pytest.raises(ValueError, match="stream 3 holds 100 pending"):
        eng.push(data[:, :BLOCK])
    with pytest.raises(ValueError, match="stream 3 holds 100 pending"):
        eng.push_many(data[:, :2 * BLOCK])
    np.testing.assert_array_equal(eng.stream_ticks([3, 5]), [2, 1])
    eng.push_streams([5], data[5:6, BLOCK:2 * BLOCK])          # a stream without pending samples takes ticks
    np.testing.assert_array_equal(eng.stream_ticks([3, 5]), [2, 2])

    # a list reset drops the stream's pending samples; fed from the start it equals a fresh engine's stream
    eng.reset_streams([3])
    assert eng.stream_pending([3])[0] == 0 and eng.stream_ticks([3])[0] == 0
    eng.poll()
    sched = [[(s, a0, c) for s, a0, c in push if s == 3] for push in cu.schedule(ps.N, data.shape[1], BLOCK, 61)]
    ev, _ = cu_run_one(eng, data, [p for p in sched if p], 3)
    want = a["ev"][a["ev"]["stream"] == 3]
    assert lu.assert_events_equal(want, ev[ev["stream"] == 3], ps.N) == len(want) >= 1
    assert eng.state(3)["silence_threshold"] == a["thr"][3]
    np.testing.assert_array_equal(eng.read_last(3, 4 * BLOCK), a["last"][3])
    assert eng.stream_ticks([3])[0] == n_ticks

    # reset() and set_input_rate drop every stream's
    eng.push_chunks([1, 2], [data[1, :7], data[2, :BLOCK + 9]])
    np.testing.assert_array_equal(eng.stream_pending([1, 2]), [7, 9])
    eng.reset()
    assert not eng.stream_pending().any() and not eng.stream_ticks().any()
    eng.push(data[:, :BLOCK])                                  # lockstep again
    eng.push_chunks([1, 2], [data[1, :7], data[2, :BLOCK + 9]])
    np.testing.assert_array_equal(eng.stream_pending([1, 2]), [7, 9])
    eng.set_input_rate(48000)
    assert not eng.stream_pending().any()
    eng.push_chunks([1], [np.zeros(4799, np.float32)])         # pending counts input samples now
    assert eng.stream_pending([1])[0] == 4799 and eng.stream_ticks([1])[0] == 1
    eng.set_input_rate(0)
    assert not eng.stream_pending().any()
    eng.close()


def cu_run_one(eng, data, sched, stream):
    """chunk_util.run for a schedule of one stream on an engine whose other streams stand still."""
    got = []
    delivered = 0
    for k, push in enumerate(sched):
        (s, a0, c), = push
        eng.push_chunks([s], [data[s, a0:a0 + c]])
        delivered += c
        assert eng.stream_ticks([stream])[0] == delivered // BLOCK
        assert eng.stream_pending([stream])[0] == delivered % BLOCK
        if k % 16 == 15:
            got.append(eng.poll())
    got.append(eng.poll())
    return np.concatenate(got), delivered
