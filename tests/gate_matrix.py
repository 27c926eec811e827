"""Shared by the gate-matrix tests (tests/test_gate_matrix.py on the CPU, tests/test_gpu_gate_matrix.py
on the GPU): the case table, the signal recipe, the push schedule and an oracle that can afford
small blocks.

The matrix drives k_gate_ticks through every launch family (register slots x sample path, with
and without detector profiles and listeners) and every shape of numpy's pairwise-summation tree,
and compares the engine with oracle/gate_ref.py tick by tick.

The oracle's SoundBufferRef recomputes every block RMS at every push; at 2,285 blocks that costs
minutes.  CachedRmsBuffer keeps the array and recomputes only the physical blocks a push wrote
into, with the oracle's own expression on the same slices; test_gate_matrix.py holds it to the
plain oracle on every case.

Detector timings.  One set for every case (DETECTOR): the engine's ring is 4 s (1 s for the
7-sample block), so speech may last 1.0 s at the most.  A segment is then never longer than
1.0 + 2 * padding seconds and the reference's 3 s limit for level 2 can never bite; so that the
skipped flag is still exercised, max_segment_seconds is 0.7 (an event is skipped when its speech
lasted more than 0.6 s).  With 8,192-sample blocks a tick is 0.512 s and speech can only ever
last one tick: every event of that case is 0.612 s long, and the case uses 0.6, which skips all
of them.
"""
import numpy as np

import lifecycle_util as lu
import synth
from oracle.gate_ref import MIN_THRESHOLD, DetectorRef, GateConfig, SoundBufferRef

SR = 16000
N_STREAMS = 9
DETECTOR = dict(pre_speech_silence=0.3, speech_duration_min=0.2, speech_duration_max=1.0, post_speech_silence=0.2)
PADDING = 0.05
PUSH_CYCLE = (1, 2, 3, 5, 7, 13)
TREE_KINDS = {0: "leaf under 8", 1: "single leaf", 2: "balanced", 3: "general"}

# name: block, input ("f32" / "pcm16"), ring ("f32" / "i16"), buffer_seconds, compact, expected
# (rb, dma), expected (block tree kind, last-window tree kind), burst seconds (lo, hi),
# max_segment_seconds, seconds at the high noise level after the ring has filled.
# The last window is 1,600 samples everywhere: a balanced tree of 16 leaves (kind 2).


def _case(block, rb, dma, tree, inp="f32", ring="f32", seconds=4, compact=False, burst=(0.25, 0.75), max_seg=0.7,
          high=None, decade=(0.8, 1.1)):
    high = max(2.5, 55 * block / SR) if high is None else high   # the threshold changes at about every second tick
    return dict(decade=decade, block=block, rb=rb, dma=dma, tree=tree, input=inp, ring=ring, buffer_seconds=seconds,
                compact=compact, burst=burst, max_segment_seconds=max_seg, high=high)


CASES = {
    "a_1600": _case(1600, 2, 2, 2),
    "b_2000": _case(2000, 2, 2, 2),
    "c_3200": _case(3200, 2, 1, 3, burst=(0.25, 0.7)),
    "d_4100": _case(4100, 2, 0, 3, burst=(0.25, 0.6)),
    "e_8192": _case(8192, 2, 0, 3, burst=(0.3, 0.41), max_seg=0.6),
    "f_1000": _case(1000, 2, 2, 2),
    "g_500": _case(500, 2, 2, 3),
    "h_498": _case(498, 2, 1, 3),
    "i_496": _case(496, 8, 2, 2),     # (four leaves 120, 128, 120, 128: balanced)
    "j_260": _case(260, 8, 2, 3),
    "k_125": _case(125, 8, 1, 1),
    "l_124": _case(124, 0, 0, 1),
    "m_7": _case(7, 0, 0, 0, seconds=1, burst=(0.3, 0.62), high=1.2, decade=(1.4, 1.6)),
    "n_1600_i16": _case(1600, 2, 3, 2, inp="pcm16", ring="i16"),
    "o_496_i16": _case(496, 8, 3, 2, inp="pcm16", ring="i16"),
    "p_500_i16": _case(500, 2, 0, 3, inp="pcm16", ring="i16"),
    "q_4104_i16": _case(4104, 2, 0, 3, inp="pcm16", ring="i16", burst=(0.25, 0.6)),
    "r_120_i16": _case(120, 0, 0, 1, inp="pcm16", ring="i16"),
    "s_1600_pcm16_f32": _case(1600, 2, 3, 2, inp="pcm16"),
    # (not in the issue's table: the pair (8, 0) -- int16 input whose block is no multiple of 8, on
    # 256 blocks -- which the table's cases leave out)
    "u_250_i16": _case(250, 8, 0, 3, inp="pcm16", ring="i16"),
    "t_125_compact": _case(125, 8, 1, 1, compact=True),
    "t_1600_compact": _case(1600, 2, 2, 2, compact=True),
}
# every (rb, dma) pair launch_gate can reach: both register families with each sample path, and
# the global-memory family, which has one
REACHABLE = sorted([(rb, dma) for rb in (2, 8) for dma in (0, 1, 2, 3)] + [(0, 0)])

# Part 4: three detector profiles assigned round-robin (stream i: profile i % 3), and two
# listeners -- the engine's configuration and profile 1 -- on every second stream.
PROFILES = [
    dict(DETECTOR),
    dict(pre_speech_silence=0.2, speech_duration_min=0.1, speech_duration_max=0.6, post_speech_silence=0.15,
         max_segment_seconds=0.5),
    dict(pre_speech_silence=0.4, speech_duration_min=0.3, speech_duration_max=1.0, post_speech_silence=0.3,
         padding=0.1),
]
PROFILE_CASES = ("g_500", "j_260", "l_124")
LISTENER_CASES = ("a_1600", "i_496", "l_124")
LISTENER_PROFILES = (-1, 1)


def ring_len(case):
    return case["buffer_seconds"] * SR


def n_blocks(case):
    return ring_len(case) // case["block"]


def segment_need(case, max_speech=None, post=None, padding=None):
    """The longest segment request of a configuration, as the engine computes it."""
    max_speech = DETECTOR["speech_duration_max"] if max_speech is None else max_speech
    post = DETECTOR["post_speech_silence"] if post is None else post
    padding = PADDING if padding is None else padding
    return min(ring_len(case), int((max_speech + post + case["block"] / SR + padding) * SR) + 2)


def sample_ring(case):
    """Samples kept per stream: the reference ring, or the smallest compact ring the engine accepts."""
    if not case["compact"]:
        return ring_len(case)
    block = case["block"]
    assert ring_len(case) % block == 0
    ring = -(-(segment_need(case) + block) // block) * block
    # (the engine initialises the rings in 8-byte words: nine float32 rows of an odd length are no
    # whole number of them, and ewk_create refuses the ring)
    while (ring * N_STREAMS * 4) % 8:
        ring += block
    return ring


def ticks_per_launch(case, need=None):
    """The engine's cap on the ticks of one gate launch (segments are scored before the ring
    overwrites them)."""
    ring = sample_ring(case)
    need = segment_need(case) if need is None else need
    return max(1, min(32, (ring - min(need, ring)) // case["block"]))


def engine_config(case):
    cfg = dict(DETECTOR, block=case["block"], tick_seconds=case["block"] / SR, buffer_seconds=case["buffer_seconds"],
               padding=PADDING, max_segment_seconds=case["max_segment_seconds"])
    if case["ring"] == "i16":
        cfg["ring_format"] = 1
    if case["compact"]:
        cfg["ring_samples"] = sample_ring(case)
    return cfg


def gate_config(case, profile=-1):
    """The oracle's GateConfig of a case, with the engine's timings (-1) or a profile's."""
    d = dict(DETECTOR, padding=PADDING, max_segment_seconds=case["max_segment_seconds"])
    if profile >= 0:
        d.update(PROFILES[profile])
    return GateConfig(block=case["block"], tick_seconds=case["block"] / SR, buffer_seconds=case["buffer_seconds"], **d)


# ---- the signal -----------------------------------------------------------------------------
def _burst(rng, word, kind, n, level):
    """One loud event of n samples from the ingredients of synth.make_stream."""
    t = np.arange(n) / SR
    env = np.sin(np.pi * (np.arange(n) + 0.5) / n) ** 0.25
    if kind == 0:     # the reference word (quiet as recorded: x 10), looped past its end
        ev = np.clip(np.resize(word[1600:], n) * 10.0, -1.0, 1.0) + 0.02 * rng.standard_normal(n)
    elif kind == 1:
        ev = 0.3 * env * np.sin(2 * np.pi * 880 * t)
    elif kind == 2:
        ev = 0.15 * env * rng.standard_normal(n)
    else:
        ev = np.clip(np.resize(word[::-1][1600:], n) * 10.0, -1.0, 1.0) + 0.02 * rng.standard_normal(n)
    return ev + rng.normal(0.0, level, n)


def make_signal(case, seed):
    """One stream of a case, float32, a whole number of blocks; deterministic in (case, seed).

    The noise floor starts near 8e-3 (the threshold then follows the 25th percentile: above
    MIN_THRESHOLD, a new value at almost every tick), stays there while the ring fills and for
    case["high"] seconds more, then falls by about a decade per burst to 1e-5 (the threshold
    clamps at MIN_THRESHOLD): inserts into the sorted array land next to the removed value and
    far from it.  Bursts (word, reversed word, tone, noise burst) stand between quiet gaps long
    enough for the detector's pre- and post-speech silence at the case's tick.  One stretch of
    exact zeros covers more than a quarter of the ring (ties at 0).  In quiet gaps a physical
    block's samples are copied over the next physical block (ties at a non-zero RMS).
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    word = synth.load_word().astype(np.float64)
    fs, R = case["block"], ring_len(case)
    tick = fs / SR
    gap_s = 0.3 + 0.2 + 3 * tick + 0.12
    parts, gaps, pos = [], [], 0

    def quiet(seconds, level):
        nonlocal pos
        n = int(seconds * SR)
        # a slow wander of the level inside the gap: no two blocks alike
        w = level * (1.0 + 0.12 * np.sin(2 * np.pi * (pos + np.arange(n)) / (1.7 * SR) + seed))
        parts.append(rng.standard_normal(n) * w)
        gaps.append((pos, pos + n, level))
        pos += n

    def loud(level, k):
        nonlocal pos
        n = int(rng.uniform(*case["burst"]) * SR)
        parts.append(_burst(rng, word, k % 4, n, level))
        pos += n

    level = 8e-3 * 10 ** rng.uniform(-0.1, 0.1)
    k = int(rng.integers(0, 4))
    # the ring fills, with a burst in it; then the high level
    quiet(0.45 * case["buffer_seconds"], level)
    loud(level, k)
    while pos < R + int(case["high"] * SR):
        k += 1
        level *= 10 ** rng.uniform(-0.04, 0.04)
        quiet(gap_s + rng.uniform(0.0, 0.2), level)
        loud(level, k)
    # down three decades, a burst at each level; the zeros after the first step
    step = 0
    while level > 1e-5:
        level = max(1e-5, level * 10 ** -rng.uniform(*case["decade"]))
        k += 1
        quiet(gap_s + rng.uniform(0.0, 0.2), level)
        if step == 0:
            n = int(0.3 * R) + 2 * fs
            parts.append(np.zeros(n))
            pos += n
            quiet(gap_s, level)
        loud(level, k)
        step += 1
    quiet(gap_s, level)
    x = np.concatenate(parts)
    x = x[:len(x) - len(x) % fs]
    # ties: physical block b + 1 := physical block b, both inside one quiet gap after the ring filled
    nb, done = R // fs, 0
    for a, b, lv in gaps:
        a = max(a, R)
        if lv < 2e-4 or done >= 3:
            continue
        p0 = a + ((-(a % R)) % fs)      # the next physical block boundary
        if (p0 % R) % fs or p0 // R != (p0 + 2 * fs - 1) // R or (p0 % R) // fs + 1 >= nb or p0 + 2 * fs > min(b, len(x)):
            continue
        x[p0 + fs:p0 + 2 * fs] = x[p0:p0 + fs]
        done += 1
    return np.clip(x, -1.0, 1.0).astype(np.float32)


_signals = {}


def signals(name):
    """The nine streams of a case cut to a common whole number of ticks: (src, data) -- what is
    pushed (int16 for PCM16 input) and the float32 values it decodes to."""
    if name not in _signals:
        case = CASES[name]
        xs = [make_signal(case, 7100 + 97 * i + sum(map(ord, name))) for i in range(N_STREAMS)]
        L = min(len(x) for x in xs)
        data = np.stack([x[:L] for x in xs])
        src = data
        if case["input"] == "pcm16":
            src, data = lu.to_pcm16(data)
        _signals[name] = (np.ascontiguousarray(src), np.ascontiguousarray(data))
    return _signals[name]


def push_schedule(case, n_ticks):
    """Ticks per push: the cycle 1, 2, 3, 5, 7, 13 (each capped below n_blocks, so every block RMS
    ever computed is exported at least once), with one push longer than the engine's
    ticks-per-launch cap right after the ring has filled."""
    nb = n_blocks(case)
    long_push = min(nb - 1, 33)
    assert long_push > ticks_per_launch(case)
    out, t, i, did_long = [], 0, 0, False
    while t < n_ticks:
        if not did_long and t > nb + 2:
            nt, did_long = long_push, True
        else:
            nt = min(PUSH_CYCLE[i % len(PUSH_CYCLE)], nb - 1)
            i += 1
        nt = min(nt, n_ticks - t)
        out.append(nt)
        t += nt
    assert did_long
    return out


# ---- the oracle ------------------------------------------------------------------------------
class CachedRmsBuffer(SoundBufferRef):
    """SoundBufferRef that keeps all_rms from push to push and recomputes only the physical blocks
    the push wrote into: np.sqrt(np.mean(frame ** 2)) on the slices the oracle takes, fed to
    np.percentile(all_rms, 25) * 1.5 as the oracle feeds it.  `updates` collects (block, value) of
    every recomputed block until the caller clears it; `silent` is the last is_silent()."""

    def __init__(self, seconds):
        super().__init__(seconds)
        self.all_rms = None
        self.updates = []
        self.silent = None
        self._wrote = (0, 0)

    def push(self, block):
        self._wrote = (self.pointer, len(np.asarray(block).ravel()))
        super().push(block)

    def _frame_rms(self, i):
        frame = self.data[i * self.frame_size:(i + 1) * self.frame_size]
        return np.sqrt(np.mean(frame ** 2))

    def _adjust_silence_threshold(self):
        fs = self.frame_size
        if fs == 0:
            return
        num_frames = len(self.data) // fs
        p0, n = self._wrote
        L = self.buffer_length
        if self.all_rms is None or n >= L:
            blocks = range(num_frames)
            self.all_rms = np.zeros(num_frames)
        else:
            spans = [(p0, min(p0 + n, L))] + ([(0, p0 + n - L)] if p0 + n > L else [])
            blocks = [i for a, b in spans for i in range(a // fs, min((b - 1) // fs, num_frames - 1) + 1)]
        for i in blocks:
            v = self._frame_rms(i)
            self.all_rms[i] = v
            self.updates.append((i, v))
        if num_frames:
            new_threshold = np.percentile(self.all_rms, 25) * 1.5
            self.silence_threshold = max(new_threshold, self.MIN_THRESHOLD)

    def block_rms(self):
        if self.all_rms is None:
            return super().block_rms()
        return self.all_rms.copy()

    def is_silent(self):
        self.silent = super().is_silent()
        return self.silent


def detector(cfg, cached=True, keep_audio=True):
    det = DetectorRef(cfg, keep_audio=keep_audio)
    if cached:
        det.buf = CachedRmsBuffer(cfg.buffer_seconds)
    return det


class Trace:
    """One stream through the cached oracle: per tick (index t = tick - 1) the threshold, the
    detector's last is_silent() and FSM state and whether it has started; `updates[t]`, the
    (block, value) pairs tick t + 1 wrote into the block-RMS array; the events."""

    def __init__(self, pcm, cfg, keep_audio=True):
        det = detector(cfg, keep_audio=keep_audio)
        fs = cfg.block
        T = len(pcm) // fs
        self.threshold = np.zeros(T)
        self.silent = np.zeros(T, bool)
        self.state = np.zeros(T, np.int8)
        self.started = np.zeros(T, bool)
        self.updates = []
        self.ties = 0          # ticks with two equal non-zero block RMS values
        for t in range(T):
            det.push_tick(pcm[t * fs:(t + 1) * fs])
            buf = det.buf
            self.threshold[t] = buf.silence_threshold
            self.started[t] = det.started
            self.state[t] = det.state
            self.silent[t] = bool(buf.silent) if det.started else True
            self.updates.append(buf.updates)
            self.ties += any(v > 0 and (buf.all_rms == v).sum() > 1 for _, v in buf.updates[-2:])
            buf.updates = []
        self.events = det.events
        self.n_ticks = T
        self.full_at = int(np.argmax(self.started)) + 1 if self.started.any() else None   # the tick the ring filled


_traces = {}


def traces(name, profiles=None):
    """The traces of a case's nine streams with the engine's timings, or with stream i gated by
    profile profiles[i] (-1: the engine's).  Computed once."""
    key = (name, tuple(profiles) if profiles is not None else None)
    if key not in _traces:
        case = CASES[name]
        _, data = signals(name)
        _traces[key] = [Trace(data[i], gate_config(case, -1 if profiles is None else profiles[i]))
                        for i in range(N_STREAMS)]
    return _traces[key]


def recipe_facts(name):
    """What the oracle alone shows of a case's inputs (the conditions test_gate_matrix.py asserts)."""
    tr = traces(name)
    after = [t.threshold[t.full_at - 1:] for t in tr]
    return dict(events=[len(t.events) for t in tr],
                skipped=sum(e.skipped for t in tr for e in t.events),
                scored=sum(not e.skipped for t in tr for e in t.events),
                thresholds=[len(np.unique(a)) for a in after],
                clamped=[int((a == MIN_THRESHOLD).sum()) for a in after],
                ties=[int(t.ties) for t in tr],
                n_ticks=tr[0].n_ticks)
