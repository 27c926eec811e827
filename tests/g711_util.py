"""Shared by the G.711 GPU tests: the input (four 8 kHz PCM16 streams of
test_gpu_push_streams_resample, encoded and decoded back), the lockstep push_pcm16 engine every
test compares with -- run once per law and left unchanged -- and the chunk runner of chunk_util
for code bytes.

The oracle (oracle.gate_ref.run_stream on resample_ref.delayed_resample of the decoded audio) cuts
two events per stream on this input, 8 in all, for mu-law, A-law and the plain PCM16: every
equality test asserts that the PCM16 engine produced at least MIN_EVENTS, so that an empty
comparison cannot pass."""
import ctypes as C
import functools

import numpy as np

import lifecycle_util as lu

RATE, IB, N, MIN_EVENTS = 8000, 800, 4, 8
LAWS = ("ulaw", "alaw")
MIXED = ("ulaw", "alaw", "ulaw", "alaw")   # per stream: streams 0 and 2 mu-law, 1 and 3 A-law
# a code no test input may be read from: the law's most negative value (a read from a gap shows in the ring)
GAP = {"ulaw": 0x00, "alaw": 0x2A}


@functools.lru_cache(maxsize=None)
def data():
    """{law: (codes uint8 [N][n_ticks * IB], dec16 int16 of the same shape)}, n_ticks."""
    import test_gpu_push_streams_resample as psr
    from easywakeword_amd import audio
    pcm16, ib = psr._input(RATE, True)
    assert ib == IB and pcm16.shape[0] == N and pcm16.dtype == np.int16
    out = {}
    for law in LAWS:
        codes = audio.g711_encode(pcm16, law)
        out[law] = (codes, audio.g711_decode(codes, law))
    codes = np.stack([out[MIXED[s]][0][s] for s in range(N)])
    out["mixed"] = (codes, np.stack([out[MIXED[s]][1][s] for s in range(N)]))
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out, pcm16.shape[1] // IB


def engine(rate=RATE, **cfg):
    import test_gpu_push_streams_resample as psr
    from easywakeword_amd import StreamEngine
    from golden_io import matcher_fixture, template_arrays
    tm, ts = template_arrays(matcher_fixture()[0])
    e = StreamEngine(N, **{**psr.GATE, **cfg})
    e.set_template(tm, ts)
    if rate:
        e.set_input_rate(rate)
    return e


def results(e):
    """(rings, thresholds) of an engine: read_last(s, 2 * BLOCK) and silence_threshold per stream."""
    return ([e.read_last(s, 2 * 1600) for s in range(N)], [e.state(s)["silence_threshold"] for s in range(N)])


@functools.lru_cache(maxsize=None)
def reference(law):
    """The lockstep engine pushed dec16 with push_pcm16, 3 ticks per call: (events, rings,
    thresholds).  `law` may be "mixed"."""
    d, n_ticks = data()
    dec16 = d[law][1]
    a = engine()
    got = []
    for c in range(0, n_ticks, 3):
        a.push_pcm16(dec16[:, c * IB:min(c + 3, n_ticks) * IB])
        got.append(a.poll())
    ev = np.concatenate(got)
    rings, thr = results(a)
    a.close()
    assert len(ev) >= MIN_EVENTS, len(ev)
    ev.setflags(write=False)
    return ev, rings, thr


def assert_same(e, ev, ref, what=""):
    """Engine e, with its polled events ev, against a reference(): every event field and the
    score's bits, the rings' bits, the thresholds.  Returns the events compared."""
    ev_a, rings, thr = ref
    n = lu.assert_events_equal(ev_a, ev, N)
    assert n >= MIN_EVENTS, (what, n)
    got_rings, got_thr = results(e)
    for s in range(N):
        np.testing.assert_array_equal(got_rings[s].view(np.int32), rings[s].view(np.int32), err_msg=f"{what} ring {s}")
        assert got_thr[s] == thr[s], (what, s)
    return n


def strided(codes, c0, nt, gap, lead=3):
    """Ticks c0 .. c0 + nt of every row laid out as resample_gpu_util.push_sequence lays them out:
    tick_stride = IB + 5, stride = nt * tick_stride + 11 (both odd or not multiples of 4), the
    first row `lead` bytes into the buffer, the gaps filled with `gap`.  Returns (buffer, view
    from the first sample, stride, tick_stride)."""
    n = codes.shape[0]
    tick_stride = IB + 5
    stride = nt * tick_stride + 11
    buf = np.full(lead + n * stride, gap, np.uint8)
    for s in range(n):
        for t in range(nt):
            at = lead + s * stride + t * tick_stride
            buf[at:at + IB] = codes[s, (c0 + t) * IB:(c0 + t + 1) * IB]
    return buf, buf[lead:], stride, tick_stride


def push_strided(e, codes, c0, nt, law, streams=None):
    """One ewk_push_g711 / ewk_push_streams_g711 call on the layout of strided()."""
    from easywakeword_amd import _lib
    buf, view, stride, tick_stride = strided(codes, c0, nt, GAP[law])
    ptr = C.c_void_p(view.ctypes.data)
    if streams is None:
        _lib.check(e._lib.ewk_push_g711(e.handle, ptr, stride, tick_stride, nt, _lib.G711_LAWS[law], 0))
    else:
        s = np.ascontiguousarray(streams, np.int32)
        _lib.check(e._lib.ewk_push_streams_g711(e.handle, _lib.i32ptr(s), s.size, ptr, stride, tick_stride, nt,
                                                _lib.G711_LAWS[law], 0))


def packed(push, src, gaps=(1, 3, 16, 7), fill=0):
    """The chunks of one push in one uint8 buffer, every chunk at an odd byte offset, the gaps
    holding `fill`.  Returns (buffer, offsets, counts)."""
    offs, at = [], 0
    for k, (_, _, c) in enumerate(push):
        at = (at + gaps[k % len(gaps)]) | 1
        offs.append(at)
        at += c
    buf = np.full(at + 16, fill, np.uint8)
    for (s, a, c), o in zip(push, offs):
        buf[o:o + c] = src[s, a:a + c]
    return buf, offs, [c for _, _, c in push]


def run_chunks(e, codes, sched, laws, where="host", pcm16_every=0, dec16=None, poll_every=16):
    """chunk_util.run for code bytes.  laws: one name, or one name per stream (then every push
    carries a law per chunk).  The chunks of a push lie at odd byte offsets in one buffer, in host
    or device memory.  pcm16_every = k > 0: every k-th push is delivered as the PCM16 the codes
    decode to (dec16) through push_chunks_pcm16 instead -- the G.711 pushes around it straddle it.
    After every push stream_ticks() and stream_pending() follow the delivered samples.  Returns the
    polled events."""
    from easywakeword_amd import _lib
    delivered = np.zeros(N, np.int64)
    got, keep = [], []
    for k, push in enumerate(sched):
        streams = [s for s, _, _ in push]
        if pcm16_every and k % pcm16_every == pcm16_every - 1:
            e.push_chunks_pcm16(streams, [dec16[s, a:a + c] for s, a, c in push])
        else:
            one = laws if isinstance(laws, str) else None
            per = None if one else [laws[s] for s in streams]
            buf, offs, counts = packed(push, codes, fill=GAP[one or "ulaw"])
            if where == "host":
                s32 = np.ascontiguousarray(streams, np.int32)
                o64, c32 = np.ascontiguousarray(offs, np.int64), np.ascontiguousarray(counts, np.int32)
                l8 = None if one else np.array([_lib.G711_LAWS[l] for l in per], np.uint8)
                _lib.check(e._lib.ewk_push_chunks_g711(
                    e.handle, _lib.i32ptr(s32), s32.size, C.c_void_p(buf.ctypes.data), buf.size, _lib.i64ptr(o64),
                    _lib.i32ptr(c32), _lib.G711_LAWS[one] if one else 0,
                    l8.ctypes.data_as(C.c_void_p) if l8 is not None else None, 0))
            else:
                import torch
                dev = torch.from_numpy(buf).to(torch.device("cuda", 0))
                e.push_chunks_device(streams, dev.data_ptr(), dev.numel(), offs, counts, g711=one or per)
                keep.append(dev)
        for s, _, c in push:
            delivered[s] += c
        np.testing.assert_array_equal(e.stream_ticks(), delivered // IB, err_msg=f"push {k}")
        np.testing.assert_array_equal(e.stream_pending(), delivered % IB, err_msg=f"push {k}")
        if k % poll_every == poll_every - 1:
            got.append(e.poll())
            e.sync()          # the device buffers of the pushes so far have been read
            keep.clear()
    got.append(e.poll())
    e.sync()
    return np.concatenate(got)
