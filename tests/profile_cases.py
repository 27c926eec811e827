"""Shared by the detector-profile tests: the table of four profiles, the stream -> profile
assignment, and the CPU oracle's event lists per stream (oracle/gate_ref.py with that stream's
GateConfig), computed once per recipe.

The oracle's SoundBufferRef recomputes every block RMS at every push.  MemoBuffer keeps the
RMS of the blocks a push did not touch (same samples, same value, bit for bit), which makes the
400- and 640-block recipes affordable; tests/test_detector_profile_oracle.py holds it to the
plain oracle.
"""
import numpy as np

import lifecycle_util as lu
from oracle.gate_ref import DetectorRef, GateConfig, SoundBufferRef

N = 12
BLOCK = 1600
SEED0 = 8600
# (fields not named take the engine's configuration = the reference defaults)
PROFILES = [
    dict(pre_speech_silence=0.5, speech_duration_min=0.2, speech_duration_max=1.0, post_speech_silence=0.3),
    dict(pre_speech_silence=1.0, speech_duration_min=0.6, speech_duration_max=2.4, post_speech_silence=0.5,
         max_segment_seconds=0.8),
    dict(reentry_timeout=3.0),
    dict(pre_speech_silence=0.3, speech_duration_min=0.1, speech_duration_max=2.4, post_speech_silence=0.2,
         padding=0.1),
]


def assignment(n=N):
    """Stream i: the engine's configuration (-1) when i % 5 == 0, else profile i % 5 - 1."""
    return np.array([i % 5 - 1 for i in range(n)], np.int32)


def gate_config(profile, block=BLOCK, **kw):
    """The oracle's GateConfig of a profile index (-1: the defaults) at `block` samples a tick."""
    d = dict(PROFILES[profile]) if profile >= 0 else {}
    d.update(kw)
    if d.get("reentry_timeout") is not None and d["reentry_timeout"] <= 0:
        d["reentry_timeout"] = None
    return GateConfig(block=block, tick_seconds=block / 16000, **d)


def engine_config(profile):
    """The same numbers as keyword arguments of a StreamEngine's configuration."""
    return dict(PROFILES[profile]) if profile >= 0 else {}


class MemoBuffer(SoundBufferRef):
    def push(self, block):
        n = len(np.asarray(block).ravel())
        self._dirty = (self.pointer, n)
        super().push(block)

    def _adjust_silence_threshold(self):
        fs = self.frame_size
        if fs == 0:
            return
        nf = len(self.data) // fs
        memo = getattr(self, "_memo", None)
        p0, n = self._dirty
        if memo is None or n >= self.buffer_length:
            memo = [np.sqrt(np.mean(self.data[i * fs:(i + 1) * fs] ** 2)) for i in range(nf)]
        else:
            L = self.buffer_length
            spans = [(p0, min(p0 + n, L))] + ([(0, p0 + n - L)] if p0 + n > L else [])
            for a, b in spans:
                for i in range(a // fs, min((b - 1) // fs, nf - 1) + 1):
                    memo[i] = np.sqrt(np.mean(self.data[i * fs:(i + 1) * fs] ** 2))
        self._memo = memo
        if memo:
            self.silence_threshold = max(np.percentile(memo, 25) * 1.5, self.MIN_THRESHOLD)


def run(pcm, cfgs, keep_audio=True, memo=True):
    """The oracle over `pcm` in cfg.block callbacks.  `cfgs`: a GateConfig, or a list of (first
    tick index, GateConfig) -- the detector's cfg is replaced before that tick is pushed, its
    state kept (what ewk_stream_profile_assign does to a stream)."""
    if isinstance(cfgs, GateConfig):
        cfgs = [(0, cfgs)]
    det = DetectorRef(cfgs[0][1], keep_audio=keep_audio)
    if memo:
        buf = MemoBuffer(det.cfg.buffer_seconds)
        det.buf = buf
    block = det.cfg.block
    switch = dict(cfgs)
    for k in range(len(pcm) // block):
        if k in switch:
            det.cfg = switch[k]
        det.push_tick(pcm[k * block:(k + 1) * block])
    return det.events


def key(events):
    """(tick, length, skipped) of oracle events."""
    return [(e.tick, e.length, e.skipped) for e in events]


def engine_key(ev):
    return [(int(m["tick"]), int(m["length"]), bool(m["flags"] & 1)) for m in ev]


_cache = {}


def main_case():
    """The 12-stream recipe: data, assignment, the oracle's lists with each stream's profile
    (`ref`) and with the default configuration (`ref_default`)."""
    if "main" not in _cache:
        data = lu.streams(N, BLOCK, SEED0)
        assign = assignment()
        ref = [run(data[i], gate_config(int(assign[i]))) for i in range(N)]
        ref_default = [ref[i] if assign[i] < 0 else run(data[i], gate_config(-1), keep_audio=False) for i in range(N)]
        _cache["main"] = dict(data=data, assign=assign, ref=ref, ref_default=ref_default,
                              n_ticks=data.shape[1] // BLOCK)
    return _cache["main"]


def assert_recipe_tells(case):
    """The oracle's own lists must tell profiles from the default configuration, or a test on
    them could pass with the table ignored."""
    ref, dflt, assign = case["ref"], case["ref_default"], case["assign"]
    assert sum(len(r) for r in ref) >= 20
    assert sum(e.skipped for r in ref for e in r) >= 1
    for i in range(len(ref)):
        if assign[i] >= 0:
            assert key(ref[i]) != key(dflt[i]), i
        else:
            assert key(ref[i]) == key(dflt[i]), i
