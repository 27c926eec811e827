"""Packet ingest (ewk_push_chunks): any number of samples per stream and push, re-blocked on the
device.

Engine A gets 12 streams in lockstep (the run of test_gpu_push_streams.py, same streams and seeds).
Engine B gets the same samples by a seeded chunk schedule (chunk_util.schedule): per push a random
subset of the streams, per stream 0, 1, 160, 320, 480, block - 1, block, block + 1, 2 block + 7 or
5 block samples, after the prologue [block - 1, block, block, 1] (the carry-overlap case), polled
every 16 pushes.  Bar: per stream every event field and the score's bits equal A's, final
thresholds and rings equal, after every push stream_ticks == delivered // block and stream_pending
== delivered % block, and the oracle comparison of test_gpu_push_streams._check_oracle (scores
within the project's 1e-4).  Event content does not depend on delivery, so that file's floors hold:
more than 20 events, at least 10 oracle scores.
"""
import numpy as np
import pytest

import chunk_util as cu
import lifecycle_util as lu
import test_gpu_push_streams as ps
from golden_io import matcher_fixture, template_arrays

pytestmark = pytest.mark.gpu

N = ps.N


@pytest.fixture(scope="module")
def template():
    fx, _ = matcher_fixture()
    return template_arrays(fx)


def _engine(case, template, **cfg):
    from easywakeword_amd import StreamEngine
    block = case["block"]
    eng = StreamEngine(N, block=block, tick_seconds=block / 16000, **dict(case["cfg"], **cfg))
    eng.set_template(*template)
    return eng


def _run(case, template, seed, where="host", phases=(0,), **kw):
    eng = _engine(case, template)
    sched = cu.schedule(N, case["src"].shape[1], case["block"], seed, **kw)
    ev, delivered = cu.run(eng, case["src"], case["block"], sched, where, case["pcm16"], phases)
    assert (delivered == case["src"].shape[1]).all()
    return eng, ev


def test_b1600_f32_host(template):
    case = ps._case("b1600_f32", template)
    eng, ev = _run(case, template, 31)
    ps._compare_with_lockstep(case, eng, ev)
    eng.close()


def test_b1600_f32_device_every_16_byte_phase(template):
    """Chunks in device memory at sample offsets 0, 1, 2 and 3 modulo 4: all four 16-byte phases of
    a float source, against whatever phase the stream's pending count gives the destination."""
    case = ps._case("b1600_f32", template)
    eng, ev = _run(case, template, 32, "device", phases=(0, 1, 2, 3))
    ps._compare_with_lockstep(case, eng, ev)
    eng.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_b1600_pcm16_into_compact_i16_ring(where, template):
    """PCM16 chunks into an EWK_RING_I16 compact ring (int16 carry and tick rows), from the host and
    from device memory at odd sample offsets; the 5-block chunks cross the ticks_per_launch cut of
    the smallest compact ring."""
    case = ps._case("b1600_i16_compact", template)
    eng, ev = _run(case, template, 33, where, phases=(1, 3, 4, 7, 0, 5))
    ps._compare_with_lockstep(case, eng, ev)
    eng.close()


def test_b1600_pcm16_into_a_float_ring(template):
    """PCM16 chunks into a float ring are decoded on append (x / 32768): the stream equals one
    pushed with push_pcm16."""
    base = ps._case("b1600_i16_compact", template)      # the same int16 streams, the same oracle
    case = dict(base, cfg={})
    a = _engine(case, template)
    got = []
    for c in range(0, case["src"].shape[1], 7 * 1600):
        a.push_pcm16(case["src"][:, c:c + 7 * 1600])
        got.append(a.poll())
    case["a"] = dict(ev=np.concatenate(got), thr=[a.state(i)["silence_threshold"] for i in range(N)],
                     last=[a.read_last(i, 4 * 1600) for i in range(N)])
    a.close()
    eng, ev = _run(case, template, 34)
    ps._compare_with_lockstep(case, eng, ev)
    eng.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_b400_f32(where, template):
    case = ps._case("b400_f32", template)
    eng, ev = _run(case, template, 35, where, phases=(3, 0, 2, 1))
    ps._compare_with_lockstep(case, eng, ev)
    eng.close()


def test_one_push_makes_0_1_2_and_3_ticks(template):
    """One push whose listed streams make 0, 1, 2 and 3 ticks (three gate groups and an append)."""
    case = ps._case("b1600_f32", template)
    block = case["block"]
    first = {5: block - 1, 0: block, 9: 2 * block + 5, 2: 3 * block, 7: 0, 3: 2 * block, 11: block + 1599}
    eng = _engine(case, template)
    sched = cu.schedule(N, case["src"].shape[1], block, 36, first_push=first, prologue=False)
    assert sched[0] == [(s, 0, c) for s, c in first.items()]
    cu.run(eng, case["src"], block, sched[:1])
    np.testing.assert_array_equal(eng.stream_ticks([5, 0, 9, 2, 7, 3, 11]), [0, 1, 2, 3, 0, 2, 1])
    np.testing.assert_array_equal(eng.stream_pending([5, 0, 9, 2, 7, 3, 11]), [block - 1, 0, 5, 0, 0, 0, 1599])
    assert [eng.state(s)["tick"] for s in (5, 0, 9, 2)] == [0, 1, 2, 3]
    for s, t in ((0, 1), (9, 2), (2, 3)):        # the ring holds exactly the ticks made
        np.testing.assert_array_equal(eng.read_last(s, t * block), case["data"][s, :t * block])
    eng.close()
    eng = _engine(case, template)
    ev, _ = cu.run(eng, case["src"], block, sched)
    ps._compare_with_lockstep(case, eng, ev)
    eng.close()


def test_score_overlap(template, monkeypatch):
    """An engine created with EWK_SCORE_OVERLAP=1: scoring passes beside the next gate launch."""
    case = ps._case("b1600_f32", template)
    monkeypatch.setenv("EWK_SCORE_OVERLAP", "1")
    eng, ev = _run(case, template, 37)
    monkeypatch.delenv("EWK_SCORE_OVERLAP")
    ps._compare_with_lockstep(case, eng, ev)
    eng.close()
