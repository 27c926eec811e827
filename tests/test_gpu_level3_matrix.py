"""k_normalize over every launch geometry, bit for bit (GPU).

Every case of tests/level3_matrix.py against the reference's numpy expression (normalize_ref),
compared with bits_equal -- NaN in the same places, every other bit equal, so the sign of a zero
counts: every chunk length 1..8192 (every shape of the pairwise tree), tails of every tree class
after one and two full chunks (the LDS state a chunk leaves behind), empty segments inside a batch,
the values numpy treats specially, the device-pointer forms of ewk_normalize_segments, and events
crafted so that the ring's wrap falls at every place inside a segment, in float32 and int16 rings.
test_level3_matrix.py holds the cases and the reference to their conditions on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

import level3_matrix as lm
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from easywakeword_amd import Engine
    e = Engine()
    yield e
    e.close()


def _check(segs, out, names=None):
    """Each output against the reference of its segment; the failure names the first that differs."""
    assert len(out) == len(segs)
    want = [lm.normalize_ref(x) if len(x) else np.zeros(0) for x in segs]   # (the reference refuses an empty segment)
    if all(y.shape == w.shape for y, w in zip(out, want)) and lm.bits_equal(np.concatenate(out), np.concatenate(want)):
        return
    for i, (y, w) in enumerate(zip(out, want)):
        if y.shape != w.shape or not lm.bits_equal(y, w):
            what = names[i] if names else ""
            pytest.fail(f"segment {i} {what} of {len(w)} samples: " +
                        (str(lm.first_diff(y, w)) if y.shape == w.shape else f"shape {y.shape}"))


@pytest.mark.parametrize("recipe", list(lm.RECIPES))
@pytest.mark.parametrize("call", range(lm.N_CALLS))
def test_every_chunk_length(eng, call, recipe):
    """Every segment length 1..8192 over the five calls: every tree the split rule can build."""
    segs = lm.chunk_length_segments(call, recipe)
    _check(segs, eng.normalize(segs))


@pytest.mark.parametrize("recipe", list(lm.RECIPES))
def test_tails_after_full_chunks(eng, recipe):
    """8192 * k + r: a chunk of every tree class evaluated on the LDS state of a full chunk."""
    segs = lm.tail_segments(recipe)
    _check(segs, eng.normalize(segs), [f"(8192 * {len(s) // lm.CHUNK} + {len(s) % lm.CHUNK})" for s in segs])


def test_empty_segments_inside_a_batch(eng):
    rng = np.random.default_rng(30)
    lengths = [0, 1, 0, 8193, 129, 0]
    segs = [lm.gauss(rng, n) for n in lengths]
    out = eng.normalize(segs)
    assert [len(y) for y in out] == lengths and all(y.dtype == np.float64 for y in out)
    _check(segs, out)


def test_special_values(eng):
    """NaN, either infinity and both, +-3e38, denormals with zeros of either sign, constants,
    negative zeros and one-ulp steps; a clean neighbour either side of each stays exact."""
    names, segs = lm.value_batch()
    _check(segs, eng.normalize(segs), names)


def test_device_forms_of_normalize_segments(eng):
    """ewk_normalize_segments with the samples, the output or both in device memory: the host
    form's bits, from a pcm pointer off the 16-byte grid, and nothing written outside the output."""
    import torch
    from easywakeword_amd import _lib
    segs = lm.device_form_segments()
    host = eng.normalize(segs)
    _check(segs, host)
    want = np.concatenate(host)
    lengths = np.array([len(s) for s in segs], np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64)
    pcm = np.concatenate(segs).astype(np.float32)
    total, G, SENT = int(lengths.sum()), 8, -123.25
    dev = torch.device("cuda", eng.gpu)
    d_pcm = torch.zeros(len(pcm) + 1, dtype=torch.float32, device=dev)
    d_pcm[1:] = torch.from_numpy(pcm).to(dev)
    pcm_dev_ptr = d_pcm.data_ptr() + 4
    assert pcm_dev_ptr % 16 == 4
    lib = eng._lib
    for flags in (_lib.EWK_PCM_DEVICE | _lib.EWK_OUT_DEVICE, _lib.EWK_PCM_DEVICE, _lib.EWK_OUT_DEVICE):
        p_in = C.c_void_p(pcm_dev_ptr) if flags & _lib.EWK_PCM_DEVICE else pcm.ctypes.data_as(C.c_void_p)
        if flags & _lib.EWK_OUT_DEVICE:
            d_out = torch.full((G + total + G,), SENT, dtype=torch.float64, device=dev)
            p_out = C.c_void_p(d_out.data_ptr() + 8 * G)
        else:
            h_out = np.full(G + total + G, SENT, np.float64)
            p_out = C.c_void_p(h_out.ctypes.data + 8 * G)
        torch.cuda.synchronize()     # (the kernel runs on the engine's stream, torch filled these on its own)
        _lib.check(lib.ewk_normalize_segments(eng.handle, p_in, len(pcm), _lib.i64ptr(offsets), _lib.i32ptr(lengths),
                                              len(segs), p_out, flags))
        eng.sync()
        out = d_out.cpu().numpy() if flags & _lib.EWK_OUT_DEVICE else h_out
        assert lm.bits_equal(out[G:G + total], want), (flags, lm.first_diff(out[G:G + total], want))
        assert (out[:G] == SENT).all() and (out[G + total:] == SENT).all(), flags


@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "i16"])
@pytest.mark.parametrize("ring", [lm.RING_COMPACT, lm.RING_DEFAULT])
def test_crafted_ring_events(ring, fmt):
    """Events of tick = now whose segments wrap nowhere, inside the first chunk, exactly at its
    end, inside the second, one sample before the end, and the whole ring; the reference segment
    comes from the pushed samples (global sample j lives at j mod ring)."""
    from easywakeword_amd import StreamEngine
    cfg = dict(ring_format=fmt)
    if ring != lm.RING_DEFAULT:
        cfg["ring_samples"] = ring
    se = StreamEngine(lm.N_STREAMS, **cfg)
    try:
        assert se.sample_ring == ring
        se.template_from_pcm(synth.load_word())
        src, data = lm.ring_signal(fmt, ring)
        now = lm.RING_TICKS[ring]
        push = se.push_pcm16 if fmt else se.push_many
        for t in range(0, now, 10):
            push(src[:, t * lm.BLOCK:(t + 10) * lm.BLOCK])
            assert len(se.poll()) == 0          # (noise below the gate's floor: the rings only fill)
        assert [se.state(s)["tick"] for s in range(lm.N_STREAMS)] == [now] * lm.N_STREAMS
        events = lm.ring_events(ring)
        ev = lm.event_array(events, now)
        segs = [lm.ring_segment(data[e["stream"]], ring, e["ring_start"], e["length"]) for e in events]
        for e, seg in zip(events, segs):        # a second reading of the same samples
            back = se.read_segment(e["stream"], e["ring_start"], e["length"])
            np.testing.assert_array_equal(back.view(np.int32), seg.view(np.int32), err_msg=str(e))
        out = se.normalize_events(ev)
        out_dev = se.normalize_events_device(ev)
        _check(segs, out, [str(e) for e in events])
        for e, y, yd in zip(events, out, out_dev):
            yd = yd.cpu().numpy()
            assert lm.bits_equal(yd, y), (e, lm.first_diff(yd, y))
    finally:
        se.close()
