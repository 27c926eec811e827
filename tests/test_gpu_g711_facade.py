"""The facade on a G.711 source: a WakeWord on ArraySource(codes, rate=8000, codec="ulaw") returns
at the tick a WakeWord on the decoded float32 audio at 8 kHz returns, with whole ticks and with
160-byte packets; and a SoundBuffer snapshot taken across a half-delivered G.711 packet continues
identically in another buffer."""
import os

import numpy as np
import pytest

import g711_util as gu
import lifecycle_util as lu
import synth
from golden_io import GOLD

pytestmark = pytest.mark.gpu

WAV = os.path.join(GOLD, "reference_word.wav")
THRESHOLD = 75.0
GATE = dict(pre_speech_silence=0.8, speech_duration_min=0.3, speech_duration_max=2.0, post_speech_silence=0.4)


def _wait(tone, source):
    from easywakeword_amd import WakeWord
    ww = WakeWord("hello", [WAV, tone], timeout=60, similarity_threshold=THRESHOLD, source=source, **GATE)
    seen = []
    handle = ww._handle_events
    ww._handle_events = lambda events: (seen.extend(events.copy()), handle(events))[1]
    word = ww.waitforit()
    eng = ww._sound_buffer.engine
    out = dict(word=word, match=next(ev for ev in seen if ev["match"]), ticks=int(eng.stream_ticks()[0]),
               pending=int(eng.stream_pending()[0]), pos=ww._sound_buffer.source.pos)
    ww.stop()
    return out


def test_wakeword_on_a_g711_source(tmp_path):
    from easywakeword_amd import ArraySource, audio, write_wav
    tone = str(tmp_path / "tone.wav")
    write_wav(tone, synth.tone(880))
    pcm, _ = synth.make_stream(seed=7105, n_words=3, kinds=["tone880", "noise", "word"])
    pcm16 = lu.to_pcm16(audio.resample(pcm, 16000, 8000))[0]
    codes = audio.g711_encode(pcm16, "ulaw")
    dec = audio.g711_decode(codes, "ulaw").astype(np.float32) / np.float32(32768.0)
    a = _wait(tone, ArraySource(dec, rate=8000))
    b = _wait(tone, ArraySource(codes, rate=8000, codec="ulaw"))
    c = _wait(tone, ArraySource(codes, rate=8000, codec="ulaw", read_sizes=160))
    assert a["word"] == b["word"] == c["word"] == "hello"
    for x in (b, c):
        for f in ("tick", "length", "ring_start", "time", "flags", "match"):
            assert a["match"][f] == x["match"][f], f
        assert a["match"]["score"].tobytes() == x["match"]["score"].tobytes()
    assert int(a["match"]["tick"]) > 100            # past the buffer fill: cut by the detection loop
    assert a["pending"] == b["pending"] == 0 and a["ticks"] == b["ticks"]
    assert c["ticks"] == c["pos"] // 800 and c["pending"] == c["pos"] % 800


def test_snapshot_across_a_half_delivered_packet():
    import test_gpu_push_streams_resample as psr
    from easywakeword_amd import ArraySource, SoundBuffer
    d, n_ticks = gu.data()
    codes = d["alaw"][0][0]
    sizes = [160, 37, 160, 800]
    cut = 203          # reads before the snapshot

    def buffer(skip_reads=0):
        src = ArraySource(codes, rate=8000, codec="alaw", read_sizes=sizes)
        for _ in range(skip_reads):
            src.read()
        return SoundBuffer(seconds=psr.GATE["buffer_seconds"], source=src,
                           **{k: v for k, v in psr.GATE.items() if k != "buffer_seconds"})

    def finish(sb, got):
        while not sb.source.exhausted:
            sb.pump()
        got.append(sb.engine.poll())
        eng = sb.engine
        return (np.concatenate(got), eng.read_last(0, 3200), eng.state(0)["silence_threshold"],
                (int(eng.stream_ticks()[0]), int(eng.stream_pending()[0])))

    one = buffer()
    for _ in range(cut):
        one.pump()
    pending = int(one.engine.stream_pending()[0])
    assert 0 < pending < 800 and pending % 160 != 0        # mid-tick and mid-packet grid
    snap = one.snapshot()
    before = [one.engine.poll()]
    two = buffer(skip_reads=cut)
    two.restore(snap)
    assert int(two.engine.stream_pending()[0]) == pending
    ev1, ring1, thr1, ticks1 = finish(one, before)
    ev2, ring2, thr2, ticks2 = finish(two, [before[0]])
    assert ticks1 == ticks2 and ticks1[0] >= n_ticks - 1
    assert lu.assert_events_equal(ev1, ev2, 1) >= 2
    np.testing.assert_array_equal(ring1.view(np.int32), ring2.view(np.int32))
    assert thr1 == thr2
    one.engine.close()
    two.engine.close()
