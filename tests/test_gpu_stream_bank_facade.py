"""WakeWord with several reference recordings on the stream bank: the stream engine holds every
reference (one word of its bank) and decides each gated event on the device, in the same push.

The stream: a 880 Hz tone burst (both references score below the threshold), a noise burst
(only the second reference, a tone, reaches it) and the word.  waitforit() returns at the tick
of the oracle's first event whose best-of-two score passes."""
import os

import numpy as np
import pytest

import synth
from golden_io import GOLD
from oracle import mfcc_ref
from oracle.gate_ref import GateConfig, run_stream

pytestmark = pytest.mark.gpu

WAV = os.path.join(GOLD, "reference_word.wav")
THRESHOLD = 90.0
GATE = dict(pre_speech_silence=0.8, speech_duration_min=0.3, speech_duration_max=2.0, post_speech_silence=0.4)


def test_waitforit_decides_on_the_stream_bank(tmp_path):
    from easywakeword_amd import ArraySource, WakeWord, _lib, write_wav
    tone = str(tmp_path / "tone.wav")
    write_wav(tone, synth.tone(880))
    pcm, _ = synth.make_stream(seed=7105, n_words=3, kinds=["tone880", "noise", "word"])
    ww = WakeWord("hello", [WAV, tone], timeout=60, similarity_threshold=THRESHOLD, source=ArraySource(pcm), **GATE)
    seen = []
    handle = ww._handle_events
    ww._handle_events = lambda events: (seen.extend(events.copy()), handle(events))[1]
    assert ww.waitforit() == "hello"
    eng = ww._sound_buffer.engine
    assert eng.bank_info() == (1, 2)
    tpl = [eng.bank_template(k) for k in range(2)]

    first, per_ref = None, None
    for e in run_stream(pcm, GateConfig(**GATE)).events:
        if e.skipped:
            continue
        cm, cs = mfcc_ref.extract_mfcc(e.audio)
        sc = [float(mfcc_ref.similarity_from_stats(m, s, cm, cs)) for m, s in tpl]
        print(e.tick, sc)
        if np.nanmax(sc) >= THRESHOLD:
            first, per_ref = e, sc
            break
    assert first is not None
    assert per_ref[0] < THRESHOLD <= per_ref[1]          # only the second reference passes: the bank decided
    assert eng.state(0)["tick"] == first.tick
    last = seen[-1]
    assert int(last["tick"]) == first.tick and last["match"]
    assert int(last["flags"]) & _lib.EWK_EV_BANK
    assert _lib.event_best_template(int(last["flags"])) == 1
    assert abs(float(last["score"]) - max(per_ref)) <= 1e-4
    assert all(int(ev["flags"]) & _lib.EWK_EV_BANK for ev in seen if not int(ev["flags"]) & 1)
    ww.stop()
