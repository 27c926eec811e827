"""A WakeWord on a source whose reads are packets, not ticks: SoundBuffer.pump() sends a read of
another length than the engine's input block through push_chunks, and waitforit() returns the same
word at the same event tick as on the block-sized source (the stream of
test_gpu_stream_bank_facade.py)."""
import os

import pytest

import synth
from golden_io import GOLD

pytestmark = pytest.mark.gpu

WAV = os.path.join(GOLD, "reference_word.wav")
THRESHOLD = 90.0
GATE = dict(pre_speech_silence=0.8, speech_duration_min=0.3, speech_duration_max=2.0, post_speech_silence=0.4)


def _wait(pcm, tone, **source):
    from easywakeword_amd import ArraySource, WakeWord
    ww = WakeWord("hello", [WAV, tone], timeout=60, similarity_threshold=THRESHOLD, source=ArraySource(pcm, **source),
                  **GATE)
    seen = []
    handle = ww._handle_events
    ww._handle_events = lambda events: (seen.extend(events.copy()), handle(events))[1]
    word = ww.waitforit()
    eng = ww._sound_buffer.engine
    out = dict(word=word, match=next(ev for ev in seen if ev["match"]), seen=seen, pending=int(eng.stream_pending()[0]),
               ticks=int(eng.stream_ticks()[0]), reads=ww._sound_buffer.source.reads, pos=ww._sound_buffer.source.pos)
    ww.stop()
    return out


def test_pump_routes_ticks_and_packets():
    """A tick-sized read goes through push, also between packets when nothing is pending; behind
    pending samples it goes through push_chunks (push would refuse it).  The ring holds the audio
    in order either way."""
    import numpy as np
    from easywakeword_amd import ArraySource, SoundBuffer
    pcm, _ = synth.make_stream(seed=7105, n_words=1)
    sizes = [800, 800, 1600, 100, 1600, 1500, 1600]
    sb = SoundBuffer(source=ArraySource(pcm, read_sizes=sizes))
    eng, calls = sb.engine, []
    push, push_chunks = eng.push, eng.push_chunks
    eng.push = lambda a: (calls.append("push"), push(a))[1]
    eng.push_chunks = lambda s, c: (calls.append("chunks"), push_chunks(s, c))[1]
    for _ in sizes:
        sb.pump()
    assert calls == ["chunks", "chunks", "push", "chunks", "chunks", "chunks", "push"]
    assert eng.stream_ticks()[0] == 5 and eng.stream_pending()[0] == 0
    np.testing.assert_array_equal(eng.read_last(0, 8000), pcm[:8000].astype(np.float32))
    eng.close()


def test_waitforit_on_packets_equals_waitforit_on_ticks(tmp_path):
    from easywakeword_amd import write_wav
    tone = str(tmp_path / "tone.wav")
    write_wav(tone, synth.tone(880))
    pcm, _ = synth.make_stream(seed=7105, n_words=3, kinds=["tone880", "noise", "word"])
    a = _wait(pcm, tone)
    b = _wait(pcm, tone, read_sizes=[320, 1000, 37, 4800])
    assert a["word"] == b["word"] == "hello"
    for f in ("tick", "length", "ring_start", "time", "flags", "match"):
        assert a["match"][f] == b["match"][f], f
    assert a["match"]["score"].tobytes() == b["match"]["score"].tobytes()
    assert int(a["match"]["tick"]) > 100            # past the buffer fill: cut by the detection loop
    # the block-sized source went through push (nothing pending, a tick a read); the packets through push_chunks
    assert a["pending"] == 0 and a["ticks"] == a["reads"]
    assert b["ticks"] == b["pos"] // 1600 and b["pending"] == b["pos"] % 1600
    assert b["reads"] > b["ticks"]
