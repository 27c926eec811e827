"""The level-3 front end on the GPU (csrc/ewk_whisper.hip behind ewk_whisper_features_*).

Every float32 element must lie within the bar, min(4 E, 2^-10), of the yardstick: E is the worst
error of the parent's own float32 torch front end over the same matrix (tests/whisper_frontend.py,
computed there on the CPU; about 6.7e-5, so the bar is about 2.7e-4), 2^-10 a quarter of a bf16 ulp
at 0.5..1.  The 3000-frame cases and every ring event are held to transformers' float64
``_np_extract_fbank_features`` directly, the 8-frame cases to the numpy restatement that
tests/test_whisper_frontend.py pins to it within 2e-7.  bf16 output, batching and the two input
paths are bit-for-bit properties.
"""
import ctypes as C

import numpy as np
import pytest

import synth
import whisper_frontend as wf

pytestmark = pytest.mark.gpu

CASES = wf.matrix()
SHORT = [i for i, c in enumerate(CASES) if c.n_frames == 8]
LONG = [i for i, c in enumerate(CASES) if c.n_frames == 3000]


@pytest.fixture(scope="module")
def engine():
    from easywakeword_amd import Engine
    eng = Engine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def outputs(engine):
    """float32 features of the whole matrix, one call per frame count (host input): {case index: [80, n_frames]}."""
    out = {}
    for idx, nf in ((SHORT, 8), (LONG, 3000)):
        f = engine.whisper_features([CASES[i].raw for i in idx], n_frames=nf).cpu().numpy()
        assert f.shape == (len(idx), 80, nf) and f.dtype == np.float32
        out.update({i: f[j] for j, i in enumerate(idx)})
    return out


def _bits(t):
    import torch
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def test_matrix_float32_within_the_bar(outputs):
    bar, refs = wf.bar(), wf.references()
    worst = {}
    for i, c in enumerate(CASES):
        want = wf.yardstick(c.y) if c.n_frames == 3000 else refs[i]
        worst[c.family] = max(worst.get(c.family, 0.0), wf.max_err(outputs[i], want))
    print(f"E = {wf.parent_error()}, bar = {bar:.4g}, kernel worst per family = {worst}")
    assert all(v <= bar for v in worst.values()), (worst, bar)
    by_name = {c.name: outputs[i] for i, c in enumerate(CASES)}
    assert np.all(by_name["zeros"] == np.float32(-1.5))
    assert np.isnan(by_name["nan"]).all()


def test_device_input_equals_host_input(engine, outputs):
    import torch
    for idx, nf in ((SHORT, 8), (LONG, 3000)):
        segs = [CASES[i].raw for i in idx]
        lengths = np.array([len(s) for s in segs], np.int32)
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        pcm = torch.from_numpy(np.concatenate(segs)).cuda()
        f = engine.whisper_features((pcm, offsets, lengths), n_frames=nf)
        np.testing.assert_array_equal(_bits(f), np.stack([outputs[i] for i in idx]).view(np.int32))


def test_bf16_is_the_rounded_float32(engine, outputs):
    import torch
    for idx, nf in ((SHORT, 8), (LONG, 3000)):
        f32 = np.stack([outputs[i] for i in idx])
        b = engine.whisper_features([CASES[i].raw for i in idx], n_frames=nf, dtype="bfloat16")
        assert b.dtype == torch.bfloat16 and tuple(b.shape) == f32.shape
        got = _bits(b).view(np.uint16)
        np.testing.assert_array_equal(got, wf.bf16_round(f32))            # NaN: 0x7FC0
        finite = ~np.isnan(f32)
        want = torch.from_numpy(f32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        np.testing.assert_array_equal(got[finite], want[finite])          # torch's own rounding


def test_each_case_alone_equals_the_batch(engine, outputs):
    for i, c in enumerate(CASES):
        f = engine.whisper_features([c.raw], n_frames=c.n_frames).cpu().numpy()
        np.testing.assert_array_equal(f[0].view(np.int32), outputs[i].view(np.int32), err_msg=repr(c))


@pytest.mark.parametrize("n_frames", [1, 2, 3, 9, 65])
def test_other_frame_counts_and_empty_segments(engine, n_frames):
    """Frame counts where the start reflection folds past the window (1), the workgroup's eight
    frames and the finish tile's 64 end mid-way (9, 65), with an empty segment inside the batch."""
    rng = np.random.default_rng(40 + n_frames)
    segs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (500, 0, 161, 12000)]
    f = engine.whisper_features(segs, n_frames=n_frames).cpu().numpy()
    bar = wf.bar()
    for s, g in zip(segs, f):
        assert wf.max_err(g, wf.features_ref(wf.normalize_level3(s), n_frames)) <= bar
    assert np.all(f[1] == np.float32(-1.5))


def test_bad_arguments_are_refused(engine):
    x = [np.zeros(100, np.float32)]
    for nf in (0, -1, 3001):
        with pytest.raises(ValueError, match="n_frames"):
            engine.whisper_features(x, n_frames=nf)
    with pytest.raises(ValueError, match="dtype"):
        engine.whisper_features(x, dtype="float16")
    from easywakeword_amd import _lib
    lib, buf = engine._lib, np.full(80 * 8, 7.0, np.float32)
    pcm, off, ln = np.zeros(100, np.float32), np.zeros(1, np.int64), np.full(1, 100, np.int32)
    out = buf.ctypes.data_as(C.c_void_p)
    args = (pcm.ctypes.data_as(C.c_void_p), 100, _lib.i64ptr(off), _lib.i32ptr(ln), 1)
    assert lib.ewk_whisper_features_segments(engine._h, *args, out, 0, 0) == _lib.EWK_EINVAL
    assert b"n_frames" in lib.ewk_last_error()
    assert lib.ewk_whisper_features_segments(engine._h, *args, out, 3001, 0) == _lib.EWK_EINVAL
    assert lib.ewk_whisper_features_segments(engine._h, *args, None, 8, 0) == _lib.EWK_EINVAL
    assert lib.ewk_whisper_features_segments(engine._h, None, 100, _lib.i64ptr(off), _lib.i32ptr(ln), 1, out, 8, 0) == \
        _lib.EWK_EINVAL
    assert lib.ewk_whisper_features_segments(engine._h, *args, out, 8, 64) == _lib.EWK_EINVAL   # unknown flag
    ln[0] = 101
    assert lib.ewk_whisper_features_segments(engine._h, *args, out, 8, 0) == _lib.EWK_EINVAL    # outside pcm
    assert np.all(buf == 7.0)
    ln[0] = 100
    assert lib.ewk_whisper_features_segments(engine._h, *args, out, 8, 0) == _lib.EWK_OK        # host output
    assert np.all(buf.reshape(80, 8) == np.float32(-1.5))


# ---------------------------------------------------------------- events from the rings
def _event_streams():
    # 1.4 s of room noise ahead of each stream puts its third word across sample 320000, the
    # physical end of the 10 s ring, and a word of each across the end of the compact ring
    parts = [np.concatenate([np.random.default_rng(100 + seed).normal(0.0, 1e-3, 14 * 1600).astype(np.float32),
                             synth.make_stream(seed, n_words=4)[0]]) for seed in (1, 2, 3)]
    n = min(len(p) for p in parts) // 1600 * 1600
    pcm16 = np.stack([np.clip(np.round(p[:n] * 32768.0), -32768, 32767).astype(np.int16) for p in parts])
    return pcm16


RINGS = {
    "float32": dict(),
    "int16": dict(ring_format=1),
    "compact_int16": dict(ring_format=1, ring_samples=43200),   # 2.7 s: the least the default timings allow is 2.65 s
}


@pytest.mark.parametrize("ring", list(RINGS))
def test_events_from_the_rings(ring):
    from easywakeword_amd import StreamEngine, _lib
    from easywakeword_amd._lib import RingOverwrittenError
    import torch
    pcm16 = _event_streams()
    n_ticks = pcm16.shape[1] // 1600
    eng = StreamEngine(3, **RINGS[ring])
    eng.template_from_pcm(synth.load_word())
    ring_len = RINGS[ring].get("ring_samples", 160000)
    bar, n_ev, wrapped, worst, first = wf.bar(), 0, 0, 0.0, None
    for t0 in range(0, n_ticks, 4):   # (the compact ring holds 27 ticks: an event is read within 4 of its cut)
        chunk = pcm16[:, t0 * 1600:(t0 + 4) * 1600]
        if ring == "float32":
            eng.push_many(chunk.astype(np.float32) / np.float32(32768.0))
        else:
            eng.push_pcm16(chunk)
        ev = eng.poll()
        ev = ev[(ev["flags"] & 1) == 0]
        if not len(ev):
            continue
        first = ev[:1].copy() if first is None else first
        f = eng.whisper_features_events(ev)               # before the rings move on
        b = eng.whisper_features_events(ev, dtype="bfloat16")
        assert tuple(f.shape) == (len(ev), 80, 3000) and f.dtype == torch.float32 and f.device.index == eng.gpu
        f = f.cpu().numpy()
        np.testing.assert_array_equal(_bits(b).view(np.uint16), wf.bf16_round(f))
        for e, g in zip(ev, f):
            audio = eng.read_segment(int(e["stream"]), int(e["ring_start"]), int(e["length"]))
            worst = max(worst, wf.max_err(g, wf.yardstick(wf.normalize_level3(audio))))
            wrapped += int(e["ring_start"]) + int(e["length"]) > ring_len
        n_ev += len(ev)
    print(f"{ring}: {n_ev} events, {wrapped} across the ring's end, worst error {worst:.3g} (bar {bar:.3g})")
    assert n_ev >= 6 and wrapped >= 1
    assert worst <= bar
    # ten more seconds of room noise: the first event's samples are overwritten in any of the
    # rings.  It is refused, and nothing is written
    quiet = np.random.default_rng(5).integers(-30, 31, (3, 100 * 1600)).astype(np.int16)
    if ring == "float32":
        eng.push_many(quiet.astype(np.float32) / np.float32(32768.0))
    else:
        eng.push_pcm16(quiet)
    with pytest.raises(RingOverwrittenError):
        eng.whisper_features_events(first)
    out = torch.full((80, 8), 7.0, device="cuda")
    rc = eng._lib.ewk_whisper_features_events(eng._h, first.ctypes.data_as(C.POINTER(_lib.EwkEvent)), 1,
                                              C.c_void_p(out.data_ptr()), 8, _lib.EWK_OUT_DEVICE)
    assert rc == _lib.EWK_EOVERWRITTEN
    eng.sync()
    assert bool((out == 7.0).all())
    eng.close()


def test_confirm_features_from_events():
    """WhisperConfirm.features_from_events: the model's bf16 input straight from the rings equals
    the torch front end on the same normalised events within the bar plus bf16 rounding (half an
    ulp below 2: 2^-8)."""
    from easywakeword_amd import StreamEngine
    from easywakeword_amd.confirm import WhisperConfirm
    import torch
    pcm16 = _event_streams()
    eng = StreamEngine(3)
    eng.template_from_pcm(synth.load_word())
    ev = []
    for c in range(0, pcm16.shape[1], 16 * 1600):   # up to the first chunk that gates a segment
        eng.push_many(pcm16[:, c:c + 16 * 1600].astype(np.float32) / np.float32(32768.0))
        ev = eng.poll()
        ev = ev[(ev["flags"] & 1) == 0]
        if len(ev):
            break
    assert len(ev) >= 1
    wc = WhisperConfirm(device="cuda", max_new_tokens=2)
    got = wc.features_from_events(eng, ev)
    assert tuple(got.shape) == (len(ev), 80, 3000) and got.dtype == torch.bfloat16 and got.is_cuda
    want = wc.log_mel(eng.normalize_events_device(ev))
    err = float((got.float() - want).abs().max())
    print(f"features_from_events vs log_mel: {err:.3g}")
    assert err <= wf.bar() + 2.0 ** -8
    assert wc.transcribe_events(eng, ev) == ["" for _ in ev]
    eng.close()
