"""G.711 ingest on the device: the one-shot decode, tick pushes and the refusals.

The decode is exact and memoryless, so the bar is equality: an engine pushed G.711 bytes
(ewk_push_g711, decoded inside the resampler launch) produces what an engine pushed the decoded
PCM16 produces -- every event field, the score's bits, the ring samples and the thresholds.  One
check is independent of the PCM16 path: the ring against the host resample of the host decode,
within the resampler tests' tolerance."""
import ctypes as C

import numpy as np
import pytest

import g711_util as gu
import lifecycle_util as lu
import resample_gpu_util as rgu
from resample_ref import delayed_resample

pytestmark = pytest.mark.gpu

BLOCK = 1600


def _table(law):
    from easywakeword_amd import _lib
    t = np.zeros(256, np.int16)
    _lib.check(_lib.load().ewk_g711_table(_lib.G711_LAWS[law], t.ctypes.data_as(C.c_void_p)))
    return t.astype(np.float32) / np.float32(32768.0)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("law", gu.LAWS)
def test_one_shot_decode(law, where):
    """All 256 codes, source offsets 0..17 and lengths around the 16-byte unit, from host and
    device memory; the output too starts at every phase of a 16-byte vector.  Bit-equal to
    table / 32768; the guards either side of the output stay."""
    import torch
    from easywakeword_amd import Engine, _lib
    eng = Engine()
    lib, table, law_id = eng._lib, _table(law), _lib.G711_LAWS[law]
    dev = torch.device("cuda", 0)
    G, SENT = 8, np.float32(7.5)
    for off in range(18):
        for n in (0, 1, 15, 16, 17, 4099):
            codes = ((np.arange(off + n + 3) * 37 + off) % 256).astype(np.uint8)   # (4099 of them: every code)
            want = table[codes[off:off + n]]
            o_off = off % 4
            if where == "host":
                out = np.full(G + o_off + n + G, SENT, np.float32)
                _lib.check(lib.ewk_decode_g711(eng.handle, C.c_void_p(codes.ctypes.data + off), n,
                                               C.c_void_p(out.ctypes.data + 4 * (G + o_off)), law_id, 0))
            else:
                d_in = torch.from_numpy(codes).to(dev)
                d_out = torch.full((G + o_off + n + G,), float(SENT), dtype=torch.float32, device=dev)
                _lib.check(lib.ewk_decode_g711(eng.handle, C.c_void_p(d_in.data_ptr() + off), n,
                                               C.c_void_p(d_out.data_ptr() + 4 * (G + o_off)), law_id,
                                               _lib.EWK_PCM_DEVICE))
                eng.sync()
                out = d_out.cpu().numpy()
            got = out[G + o_off:G + o_off + n]
            np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32), err_msg=f"offset {off} n {n}")
            assert (out[:G + o_off] == SENT).all() and (out[G + o_off + n:] == SENT).all(), (off, n)
    codes = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(eng.decode_g711(codes, law), table)
    assert lib.ewk_decode_g711(eng.handle, C.c_void_p(codes.ctypes.data), 256, None, law_id, 0) == _lib.EWK_EINVAL
    assert lib.ewk_decode_g711(eng.handle, C.c_void_p(codes.ctypes.data), 256, C.c_void_p(codes.ctypes.data), 2,
                               0) == _lib.EWK_EINVAL
    eng.close()


@pytest.mark.parametrize("law", gu.LAWS)
def test_tick_pushes_equal_pcm16_pushes(law):
    from easywakeword_amd import audio
    d, n_ticks = gu.data()
    codes, dec16 = d[law]
    ref = gu.reference(law)
    b = gu.engine()
    got = []
    for c in range(0, n_ticks, 3):   # the split of the reference engine, on odd strides with gaps
        gu.push_strided(b, codes, c, min(3, n_ticks - c), law)
        got.append(b.poll())
    ev = np.concatenate(got)
    print(ev)
    gu.assert_same(b, ev, ref, law)
    np.testing.assert_array_equal(b.stream_ticks(), [n_ticks] * gu.N)
    assert b.gate_launch_info() == _gate_info_of_a_float_push()
    # independent of the PCM16 path: the host resample of the host decode
    x = audio.g711_decode(codes, law).astype(np.float32) / np.float32(32768.0)
    for s in range(gu.N):
        want = delayed_resample(x[s], gu.RATE, n_ticks * BLOCK)[-2 * BLOCK:]
        rgu.assert_close(b.read_last(s, 2 * BLOCK), want, float(np.max(np.abs(x))), f"{law} stream {s}")
    b.close()


def _gate_info_of_a_float_push():
    """The gate instantiation a float32 push with a rate set runs: a G.711 push runs the same."""
    d, _ = gu.data()
    e = gu.engine()
    e.push_many((d["ulaw"][1][:, :gu.IB].astype(np.float32) / np.float32(32768.0)))
    info = e.gate_launch_info()
    e.close()
    return info


def test_python_pushes_and_the_device_pointer():
    """push_g711 (host) and push_device_g711 on an odd device address with odd strides."""
    import torch
    d, n_ticks = gu.data()
    codes, _ = d["alaw"]
    ref = gu.reference("alaw")
    b = gu.engine()
    b.profile(True)
    got, keep = [], []
    for k, c in enumerate(range(0, n_ticks, 3)):
        nt = min(3, n_ticks - c)
        if k % 2 == 0:
            b.push_g711(codes[:, c * gu.IB:(c + nt) * gu.IB], "alaw")
        else:
            buf, _, stride, tick_stride = gu.strided(codes, c, nt, gu.GAP["alaw"], lead=3)
            dev = torch.from_numpy(buf).to(torch.device("cuda", 0))
            b.push_device_g711(dev.data_ptr() + 3, stride, tick_stride, nt, "alaw")
            keep.append(dev)
        got.append(b.poll())
    b.sync()
    ms, launches = b.profile_read(3)
    assert launches == len(got) and ms > 0      # kind 3 counts the resampler launch of a G.711 tick push
    assert b.profile_read(4)[1] == 0
    gu.assert_same(b, np.concatenate(got), ref, "alaw")
    with pytest.raises(ValueError, match="ulaw"):
        b.push_g711(codes[:, :gu.IB], "g722")
    with pytest.raises(ValueError):
        b.push_g711(codes[:3, :gu.IB], "alaw")
    b.close()


def test_refusals_leave_the_engine_unchanged():
    """Each refusal is EWK_EINVAL with its reason and changes nothing: the pushes that follow give
    the reference's events, rings and thresholds."""
    from easywakeword_amd import _lib
    law = "ulaw"
    d, n_ticks = gu.data()
    codes, dec16 = d[law]
    ref = gu.reference(law)
    IB = gu.IB

    # no input rate: the message says so; with the rate set the same engine runs the whole input
    b = gu.engine(rate=0)
    with pytest.raises(ValueError, match="input rate"):
        b.push_g711(codes[:, :2 * IB], law)     # (a tick of this engine is 1600 samples still)
    with pytest.raises(ValueError, match="input rate"):
        b.push_chunks_g711([0], [codes[0, :160]], law)
    assert not b.stream_ticks().any() and not b.stream_pending().any() and len(b.poll()) == 0
    b.set_input_rate(gu.RATE)
    got = []

    def refused(match, fn, *args):
        ticks, pending = b.stream_ticks(), b.stream_pending()
        with pytest.raises(ValueError, match=match):
            fn(*args)
        np.testing.assert_array_equal(b.stream_ticks(), ticks)
        np.testing.assert_array_equal(b.stream_pending(), pending)

    lib, h = b._lib, b.handle
    s32 = np.arange(gu.N, dtype=np.int32)
    offs, cnts = np.arange(gu.N, dtype=np.int64) * 160, np.full(gu.N, 160, np.int32)
    ptr = C.c_void_p(codes.ctypes.data)

    def bad_law():
        _lib.check(lib.ewk_push_g711(h, ptr, codes.shape[1], IB, 1, 2, 0))

    def bad_law_streams():
        _lib.check(lib.ewk_push_streams_g711(h, _lib.i32ptr(s32), gu.N, ptr, codes.shape[1], IB, 1, -1, 0))

    def bad_law_chunks():
        _lib.check(lib.ewk_push_chunks_g711(h, _lib.i32ptr(s32), gu.N, ptr, codes.size, _lib.i64ptr(offs),
                                            _lib.i32ptr(cnts), 7, None, 0))

    def bad_laws_entry():
        laws = np.array([0, 1, 2, 1], np.uint8)
        _lib.check(lib.ewk_push_chunks_g711(h, _lib.i32ptr(s32), gu.N, ptr, codes.size, _lib.i64ptr(offs),
                                            _lib.i32ptr(cnts), 0, laws.ctypes.data_as(C.c_void_p), 0))

    HALF = 30
    for c in range(0, HALF, 3):
        if c == 6:
            refused("law = 2", bad_law)
            refused("law = -1", bad_law_streams)
        if c == 12:
            refused("law = 7", bad_law_chunks)
            refused(r"laws\[2\] = 2", bad_laws_entry)
        gu.push_strided(b, codes, c, 3, law)
        got.append(b.poll())
    # tick HALF: stream 1 gets five bytes first -- a tick push onto them is refused
    t0 = HALF * IB
    b.push_chunks_g711([1], [codes[1, t0:t0 + 5]], law)
    assert b.stream_pending().tolist() == [0, 5, 0, 0]
    refused("pending", b.push_g711, codes[:, t0:t0 + IB], law)
    refused("pending", b.push_streams_g711, [1], codes[1:2, t0:t0 + IB], law)
    b.push_chunks_g711([1], [codes[1, t0 + 5:t0 + IB]], law)
    gu.push_strided(b, codes[[0, 2, 3]], HALF, 1, law, streams=[0, 2, 3])
    got.append(b.poll())
    for c in range(HALF + 1, n_ticks, 3):
        gu.push_strided(b, codes, c, min(3, n_ticks - c), law)
        got.append(b.poll())
    gu.assert_same(b, np.concatenate(got), ref, "after the refusals")
    b.close()

    # an int16 ring refuses an input rate, and G.711 the same way; the PCM16 push that follows is
    # that of an engine never asked
    from easywakeword_amd import StreamEngine
    import test_gpu_push_streams_resample as psr
    x16 = np.repeat(dec16[:, :25 * IB], 2, axis=1)   # (any 16 kHz PCM16)
    res = []
    for ask in (True, False):
        e = StreamEngine(gu.N, ring_format=_lib.EWK_RING_I16, **psr.GATE)
        if ask:
            with pytest.raises(ValueError, match="int16 ring"):
                e.set_input_rate(gu.RATE)
            with pytest.raises(ValueError, match="int16 ring"):
                e.push_g711(codes[:, :1600], law)
            with pytest.raises(ValueError, match="int16 ring"):
                e.push_chunks_g711([0], [codes[0, :160]], law)
            assert not e.stream_ticks().any() and not e.stream_pending().any()
        e.push_pcm16(x16)
        res.append((e.poll(), gu.results(e)))
        e.close()
    lu.assert_events_equal(res[0][0], res[1][0], gu.N)
    for s in range(gu.N):
        np.testing.assert_array_equal(res[0][1][0][s], res[1][1][0][s])
        assert res[0][1][1][s] == res[1][1][1][s]

