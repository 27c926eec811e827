"""easywakeword_amd.detector_profile: the gate timings a WakeWord built with the same arguments
ends up with (CPU: WakeWord's constructor opens no device)."""
import os

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WAV = os.path.join(GOLD, "reference_word.wav")
TIMINGS = ("pre_speech_silence", "speech_duration_min", "speech_duration_max", "post_speech_silence")


def _pair(**kw):
    from easywakeword_amd import WakeWord, detector_profile
    ww = WakeWord("hello", WAV, **kw)
    return ww, detector_profile(WAV, "hello", **kw)


@pytest.mark.parametrize("kw", [
    {},
    dict(speech_duration_min=0.5),
    dict(speech_duration_min=0.4, speech_duration_max=1.5),
    dict(speech_duration_max=0.5),                       # below the analysed 0.69 s: max follows min
    dict(pre_speech_silence=0.6, post_speech_silence=0.25),
    dict(speech_duration_min=None, speech_duration_max=None),
])
def test_profile_equals_the_wakeword_attributes(kw):
    ww, p = _pair(**kw)
    for f in TIMINGS:
        assert getattr(p, f) == getattr(ww, f), f
    assert p.padding is None and p.max_segment_seconds is None and p.reentry_timeout is None


def test_analysed_duration_and_overrides():
    from easywakeword_amd import DetectorProfile, detector_profile
    p = detector_profile(WAV)
    assert isinstance(p, DetectorProfile)
    assert p.speech_duration_min == pytest.approx(0.69, abs=1e-9) and p.speech_duration_max == 2 * p.speech_duration_min
    assert detector_profile([WAV, "missing.wav"]).speech_duration_min == p.speech_duration_min   # the first recording
    q = detector_profile(WAV, padding=0.1, max_segment_seconds=2.0, reentry_timeout=30.0)
    assert (q.padding, q.max_segment_seconds, q.reentry_timeout) == (0.1, 2.0, 30.0)
    d = detector_profile()                                # no recording: the reference defaults
    assert (d.pre_speech_silence, d.speech_duration_min, d.speech_duration_max, d.post_speech_silence) == \
        (0.8, 0.3, 2.0, 0.4)


def test_unreadable_recording_falls_back_like_wakeword(tmp_path):
    from easywakeword_amd import WakeWord, detector_profile
    missing = str(tmp_path / "none.wav")
    ww = WakeWord("hello", missing)
    p = detector_profile(missing)
    assert (p.speech_duration_min, p.speech_duration_max) == (ww.speech_duration_min, ww.speech_duration_max) == (0.3, 2.0)


@pytest.mark.parametrize("kw, msg", [
    (dict(pre_speech_silence=0), "pre_speech_silence must be positive"),
    (dict(speech_duration_min=2.0, speech_duration_max=1.0), "speech_duration_min must be <= speech_duration_max"),
    (dict(post_speech_silence=-0.1), "post_speech_silence must be positive"),
])
def test_validation_as_wakeword(kw, msg):
    from easywakeword_amd import detector_profile
    with pytest.raises(ValueError, match=msg):
        detector_profile(WAV, **kw)
