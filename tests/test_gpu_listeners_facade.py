"""WakeWordSet: several wake words on one microphone, one listener per word on one stream.

The source: 11.5 s of noise, the reference word, 1.6 s of noise, a 880 Hz tone ("the second
word": bank_cases.bank_audio()[1][1]), 2.5 s of noise.  With the CPU oracle the word's gate
(the reference defaults) cuts at ticks 128 and 153 and scores 99.97 / 92.35 against the word's
recording; the tone's gate (shorter timings) cuts at 127 and 152 and scores 88.50 / 95.82 against
the tone's.  Thresholds 96 and 94 give each word exactly its own segment, with more than 1.8
points of margin against the 1e-4 score bar."""
import numpy as np
import pytest

import bank_cases as bc
from oracle import mfcc_ref
from oracle.gate_ref import GateConfig, run_stream

pytestmark = pytest.mark.gpu

GATES = [dict(pre_speech_silence=0.8, speech_duration_min=0.3, speech_duration_max=2.0, post_speech_silence=0.4),
         dict(pre_speech_silence=0.5, speech_duration_min=0.2, speech_duration_max=1.5, post_speech_silence=0.3)]
THRESHOLDS = [96.0, 94.0]
NAMES = ["computer", "lights on"]


def _noise(rng, seconds):
    return rng.normal(0.0, 1e-3, int(seconds * 16000)).astype(np.float32)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from easywakeword_amd import write_wav
    audio = bc.bank_audio()
    clips = [audio[0][0], audio[1][1]]
    rng = np.random.default_rng(4242)
    pcm = np.concatenate([_noise(rng, 11.5), clips[0], _noise(rng, 1.6), clips[1], _noise(rng, 2.5)])
    pcm = pcm[:len(pcm) - len(pcm) % 1600]
    d = tmp_path_factory.mktemp("words")
    wavs = []
    for name, clip in zip(("word.wav", "tone.wav"), clips):
        wavs.append(str(d / name))
        write_wav(wavs[-1], clip)
    # the oracle: each word's first matching tick, and that the other segment does not match
    first = []
    for clip, gate, thr in zip(clips, GATES, THRESHOLDS):
        tm, ts = mfcc_ref.extract_mfcc(clip)
        scores = [(e.tick, float(mfcc_ref.similarity_from_stats(tm, ts, *mfcc_ref.extract_mfcc(e.audio))))
                  for e in run_stream(pcm, GateConfig(**gate)).events if not e.skipped]
        hits = [t for t, s in scores if s >= thr]
        assert len(scores) == 2 and len(hits) == 1 and all(abs(s - thr) > 1.0 for _, s in scores), scores
        first.append(hits[0])
    assert first[0] < first[1]
    words = [dict(textword=n, wavword=w, similarity_threshold=t, **g) for n, w, t, g in zip(NAMES, wavs, THRESHOLDS, GATES)]
    return dict(pcm=pcm, words=words, first=first)


def test_two_words_on_one_stream(scene):
    from easywakeword_amd import ArraySource, WakeWord, WakeWordSet
    plain = []
    for w in scene["words"]:
        ww = WakeWord(w["textword"], w["wavword"], timeout=60, similarity_threshold=w["similarity_threshold"],
                      source=ArraySource(scene["pcm"]), **{k: w[k] for k in GATES[0]})
        assert ww.waitforit() == w["textword"]
        plain.append(int(ww._sound_buffer.engine.state(0)["tick"]))
        ww.stop()
    assert plain == scene["first"]

    both = WakeWordSet(scene["words"], source=ArraySource(scene["pcm"]), timeout=60)
    got = []
    for _ in range(2):
        got.append((both.waitforit(), both.last_index, int(both._sound_buffer.engine.state(0)["tick"])))
    eng = both._sound_buffer.engine
    assert got == [(NAMES[0], 0, plain[0]), (NAMES[1], 1, plain[1])]
    assert eng.n_streams == 1 and eng.stream_listeners(0) == [(0, 0), (1, 1)]
    assert eng.bank_info() == (2, 2) and len(eng.detector_profiles()) == 2
    assert not both.is_listening()
    both.stop()


def test_timeout_without_either_word(scene):
    from easywakeword_amd import ArraySource, WakeWordSet
    rng = np.random.default_rng(7)
    both = WakeWordSet(scene["words"], source=ArraySource(_noise(rng, 12.0)), timeout=3)
    with pytest.raises(TimeoutError, match="timed out after 3 seconds"):
        both.waitforit()
    both.stop()


def test_words_are_validated():
    from easywakeword_amd import WakeWordSet
    with pytest.raises(ValueError, match="1..16 words"):
        WakeWordSet([])
    with pytest.raises(ValueError, match=r"words\[0\] needs textword and wavword"):
        WakeWordSet([dict(textword="x")])
    with pytest.raises(TypeError, match="unknown key"):
        WakeWordSet([dict(textword="x", wavword="x.wav", loudness=3)])
