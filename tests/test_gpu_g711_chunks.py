"""G.711 packet ingest (ewk_push_chunks_g711): code bytes in chunks of any size, decoded by the
assembly launch into the float32 carry and tick rows.  Every case equals the lockstep push_pcm16
engine fed the decoded audio -- events, rings' bits, thresholds -- and stream_pending follows the
delivered bytes after every push."""
import numpy as np
import pytest

import chunk_util as cu
import g711_util as gu

pytestmark = pytest.mark.gpu

IB, N = gu.IB, gu.N
# around the 16-code unit and the 64-byte destination alignment, an RTP packet, around a tick, two ticks and four
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 160, 799, 800, 801, 1607, 3200]


@pytest.mark.parametrize("laws,where", [("ulaw", "host"), ("alaw", "device"), ("mixed", "host"), ("mixed", "device")])
def test_chunks_of_every_size(laws, where):
    d, n_ticks = gu.data()
    codes, _ = d[laws]
    sched = cu.schedule(N, n_ticks * IB, IB, 4100 + len(laws), size_set=SIZES)
    e = gu.engine()
    ev = gu.run_chunks(e, codes, sched, gu.MIXED if laws == "mixed" else laws, where=where)
    np.testing.assert_array_equal(e.stream_ticks(), [n_ticks] * N)
    assert not e.stream_pending().any()
    gu.assert_same(e, ev, gu.reference(laws), f"{laws} {where}")
    e.close()


def test_rtp_packets():
    """Five 160-byte packets per tick and stream, through the Python call."""
    d, n_ticks = gu.data()
    codes, _ = d["ulaw"]
    e = gu.engine()
    e.profile(True)
    got = []
    streams = list(range(N))
    for k in range(n_ticks * 5):
        e.push_chunks_g711(streams, [codes[s, k * 160:(k + 1) * 160] for s in streams], "ulaw")
        assert e.stream_pending().tolist() == [(k + 1) % 5 * 160] * N
        if k % 40 == 39:
            got.append(e.poll())
    got.append(e.poll())
    ms, launches = e.profile_read(4)
    assert launches == n_ticks * 5 and ms > 0          # kind 4 counts the assembly launch of a G.711 chunk push
    assert e.profile_read(3)[1] == n_ticks             # ... and kind 3 the resample stage of every tick made
    gu.assert_same(e, np.concatenate(got), gu.reference("ulaw"), "rtp")
    e.close()


def test_per_chunk_laws_through_the_python_call():
    d, n_ticks = gu.data()
    codes, _ = d["mixed"]
    e = gu.engine()
    got = []
    order = [2, 0, 3, 1]
    at = 0
    sizes = [160, 37, 800, 1, 1607, 63]
    k = 0
    while at < n_ticks * IB:
        c = min(sizes[k % len(sizes)], n_ticks * IB - at)
        e.push_chunks_g711(order, [codes[s, at:at + c] for s in order], [gu.MIXED[s] for s in order])
        at += c
        k += 1
        got.append(e.poll())
    with pytest.raises(ValueError, match="laws"):
        e.push_chunks_g711(order, [codes[s, :16] for s in order], ["ulaw", "alaw"])
    with pytest.raises(ValueError, match="alaw"):
        e.push_chunks_g711(order, [codes[s, :16] for s in order], ["ulaw", "alaw", "g722", "ulaw"])
    gu.assert_same(e, np.concatenate(got), gu.reference("mixed"), "per-chunk laws")
    e.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_g711_pushes_straddle_pcm16_pushes(where):
    """Every third push of the schedule delivers the decoded PCM16 through push_chunks_pcm16: a
    stream's block is assembled from G.711 and PCM16 chunks, in the same float32 carry."""
    d, n_ticks = gu.data()
    codes, dec16 = d["alaw"]
    sched = cu.schedule(N, n_ticks * IB, IB, 4200, size_set=SIZES)
    e = gu.engine()
    ev = gu.run_chunks(e, codes, sched, "alaw", where=where, pcm16_every=3, dec16=dec16)
    gu.assert_same(e, ev, gu.reference("alaw"), f"straddle {where}")
    e.close()
