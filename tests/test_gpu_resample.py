"""Input-rate resampler on the GPU: ewk_resample and the streaming push path at 48, 44.1 and
8 kHz against easywakeword_amd.audio.resample (scipy's resample_poly, float64).

The tolerance (one float32 ulp) and its argument are in resample_gpu_util.py; the other rates
and launch geometries are in test_gpu_resample_rates.py."""
import numpy as np
import pytest

import synth
from golden_io import matcher_fixture, template_arrays
from resample_gpu_util import BLOCK, assert_close, in_block_of, push_sequence, signal, stream_data
from resample_ref import OUT, design_params

pytestmark = pytest.mark.gpu

RATES = (48000, 44100, 8000)


@pytest.fixture(scope="module")
def scorer():
    from easywakeword_amd import Engine
    eng = Engine()
    yield eng
    eng.close()


@pytest.mark.parametrize("kind", ["noise", "square"])
@pytest.mark.parametrize("rate", RATES)
def test_one_shot_equals_host_resample(scorer, rate, kind):
    import torch
    from easywakeword_amd.audio import resample
    p = design_params(rate)
    lengths = [1, p["H"] - 1, p["down"] - 1, p["down"], p["down"] + 1, 3 * in_block_of(rate) + 7]
    for n in lengths:
        x = signal(kind, n, seed=rate + n)
        if n == 0:                                           # (one period - 1 at 8 kHz: down = 1)
            assert scorer.resample(x, rate).size == 0
            continue
        want = resample(x, rate, OUT)
        got = scorer.resample(x, rate)                       # host pointers
        assert_close(got, want, np.max(np.abs(x)), f"{rate} Hz {kind} n={n} host")
        d_x = torch.from_numpy(x).cuda()                     # device pointers
        d_y = torch.full((len(want) + 3,), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m = scorer.resample_device(d_x.data_ptr(), n, rate, d_y.data_ptr(), len(want) + 3)
        scorer.sync()
        y = d_y.cpu().numpy()
        assert m == len(want)
        assert np.all(y[m:] == 7.0)                          # nothing written past n_out
        assert_close(y[:m], want, np.max(np.abs(x)), f"{rate} Hz {kind} n={n} device")
    with pytest.raises(ValueError):
        scorer.resample(np.zeros(8, np.float32), 0)


@pytest.mark.parametrize("pcm16", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("rate", RATES)
def test_streaming_equals_delayed_host_resample(rate, pcm16):
    from easywakeword_amd import StreamEngine
    ib = in_block_of(rate)
    p = design_params(rate)
    data = stream_data(rate, 6, pcm16)
    eng = StreamEngine(3)
    assert (eng.input_rate, eng.input_block, eng.input_delay) == (OUT, BLOCK, 0)
    eng.set_input_rate(rate)
    assert (eng.input_rate, eng.input_block, eng.input_delay) == (rate, ib, p["delay"])
    first = push_sequence(eng, data, rate, pcm16)
    eng.reset()                                # the history is cleared: the same output again
    again = push_sequence(eng, data, rate, pcm16)
    assert np.array_equal(first, again)
    eng.set_input_rate(0)                      # back to 16 kHz pushes
    assert (eng.input_rate, eng.input_block, eng.input_delay) == (OUT, BLOCK, 0)
    blk = (0.1 * np.random.default_rng(rate).standard_normal((3, BLOCK))).astype(np.float32)
    eng.push(blk)
    for s in range(3):
        assert np.array_equal(eng.read_last(s, BLOCK), blk[s])
    eng.close()


def test_refusals():
    from easywakeword_amd import StreamEngine, _lib
    e16 = StreamEngine(1, ring_format=_lib.EWK_RING_I16)
    with pytest.raises(ValueError, match="int16"):
        e16.set_input_rate(48000)
    e16.close()
    eng = StreamEngine(2)
    with pytest.raises(ValueError, match="whole number"):
        eng.set_input_rate(11025)              # 1600 * 441 / 640 is not an integer
    assert eng.input_block == BLOCK            # the refused rate changed nothing
    eng.push(np.zeros((2, BLOCK), np.float32))
    for hz in (8000, 22050, 24000, 32000, 44100, 48000, 96000):
        eng.set_input_rate(hz)
        assert eng.input_block == BLOCK * hz // OUT
    eng.set_input_rate(48000)
    with pytest.raises(ValueError):
        eng.push(np.zeros((2, BLOCK), np.float32))          # a 16 kHz block while 48 kHz is set
    with pytest.raises(ValueError):
        eng.push_many(np.zeros((2, 4800 + 1), np.float32))
    with pytest.raises(ValueError):
        eng.push_pcm16(np.zeros((2, BLOCK), np.int16))
    eng.push(np.zeros((2, 4800), np.float32))
    eng.close()


GATE = dict(buffer_seconds=2, pre_speech_silence=0.4, speech_duration_min=0.3, speech_duration_max=1.6,
            post_speech_silence=0.3)


def test_resampled_stream_through_the_gate():
    """Engine A takes 48 kHz blocks; engine B is fed A's 16 kHz ring content tick by tick: the
    gate and scorer behind the resampler see exactly the blocks a 16 kHz push delivers."""
    from easywakeword_amd import StreamEngine
    from easywakeword_amd.audio import resample
    tm, ts = template_arrays(matcher_fixture()[0])
    pcms = [synth.make_stream(seed=4800 + i, n_words=2, prefill=2.5, kinds=k)[0]
            for i, k in enumerate((["word", "white"], ["hp", "word"]))]   # white: NaN score, hp: ~68 < 75
    L = min(len(p) for p in pcms) // BLOCK * BLOCK
    hi = np.stack([resample(p[:L], OUT, 48000) for p in pcms])      # [2][3 L]
    # (with these short gate settings the distractors score 81..90 against the word's template
    # and the word 99: a threshold of 95 for both engines gives both decisions)
    a, b = StreamEngine(2, similarity_threshold=95.0, **GATE), StreamEngine(2, similarity_threshold=95.0, **GATE)
    a.set_template(tm, ts)
    b.set_template(tm, ts)
    a.set_input_rate(48000)
    for t in range(L // BLOCK):
        a.push(hi[:, t * 4800:(t + 1) * 4800])
        b.push(np.stack([a.read_last(s, BLOCK) for s in range(2)]))
    ev_a, ev_b = a.poll(), b.poll()
    a.close()
    b.close()
    print(ev_a)
    assert len(ev_a) == len(ev_b) and len(ev_a) >= 2
    for f in ("stream", "tick", "length", "ring_start", "match", "flags"):
        assert np.array_equal(ev_a[f], ev_b[f]), f
    for x, y in zip(ev_a["score"], ev_b["score"]):
        assert (np.isnan(x) and np.isnan(y)) or abs(x - y) <= 1e-4
    assert ev_a["match"].any() and not ev_a["match"].all()


def test_wakeword_on_a_48k_wav_source(tmp_path):
    """WakeWord on a 48 kHz file left at its own rate (resampled on the device) against WakeWord
    on the host-resampled, delayed signal: the same result at the same ticks."""
    from easywakeword_amd import ArraySource, WakeWord, WavSource, write_wav
    from easywakeword_amd.audio import load_wav, resample
    pcm, _ = synth.make_stream(seed=4811, n_words=2, prefill=2.5, kinds=["tone880", "word"])
    path = str(tmp_path / "stream48k.wav")
    write_wav(path, resample(pcm, OUT, 48000), sr=48000)
    x48 = load_wav(path, sr=48000)
    delay = design_params(48000)["delay"]
    host = np.concatenate([np.zeros(delay, np.float32), resample(x48, 48000, OUT)])
    src = WavSource(path, native_rate=True)
    assert (src.rate, src.block, len(src.read())) == (48000, BLOCK, 4800)
    src.pos = 0
    res, ticks = [], []
    for source in (src, ArraySource(host)):
        ww = WakeWord("hello", synth.WAV, timeout=60, source=source, **GATE)
        seen = []
        handle = ww._handle_events
        ww._handle_events = lambda events, seen=seen, handle=handle: (seen.extend(events.copy()), handle(events))[1]
        res.append(ww.waitforit())
        eng = ww._sound_buffer.engine
        assert eng.input_rate == source.rate
        ticks.append([(int(e["tick"]), int(e["length"]), int(e["match"])) for e in seen] + [eng.state(0)["tick"]])
        ww.stop()
    print(res, ticks)
    assert res[0] == res[1] == "hello"
    assert ticks[0] == ticks[1] and len(ticks[0]) >= 2
