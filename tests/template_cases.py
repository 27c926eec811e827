"""Reference recordings for the template-parity tests (tests/test_gpu_template_parity.py): the
audio a template is derived from, a candidate batch, and a yardstick that expresses an error in
template statistics in the unit of the project's bar -- how far it moves a score.

Everything here is the CPU oracle's (oracle.mfcc_ref) and synth's; tests/test_template_cases.py
checks, without a GPU, that the oracle alone pins every recording's template tightly enough
(reference_spread <= SPREAD_CAP) for a 1e-4 comparison to mean something.

The fuzz picks are selected by rule, not by index: the loud (x 1000) fuzz clips of seed 31 with
the smallest |mean| and the fuzz clips of seeds 3 and 5 with |std| nearest 20, skipping any clip the
oracle itself does not pin (a clip with |std| = 0.05 has a spread of 6e-3: its float32 template
is rounding noise, and no engine can be held to it).
"""
import functools

import numpy as np

import synth
from oracle import mfcc_ref

BAR = 1e-4            # the project's score bar
SPREAD_CAP = 1e-5     # a tenth of it: what the reference's own arithmetic may leave open
THRESHOLD = 75.0
N_MEAN_PICKS = 3      # vanishing-mean recordings (|mean| < kTinyMean-like norms)
N_STD_PICKS = 4       # stationary recordings (|std| around 20, on both sides of it)
STD_SEEDS = (3, 5)    # fuzz seeds they come from (seed 3 alone has one pinned clip under 22)
MIN_PICK_LEN = 2000   # the fuzz picks are longer than this

# The recordings by name (the audio is made on first use: recordings()); the fuzz picks are
# numbered in the order their rule finds them.
NAMES = (["word", "word_0.2s", "word_0.4s", "word_1600", "word_2559", "word_reversed",
          "word_x0.01", "word_x30", "word_x200", "word_x1000", "tone440", "tone880_0.7s", "speech_like",
          "noise", "noise_x1000"] + [f"vanishing_mean_{k}" for k in range(N_MEAN_PICKS)] +
         [f"stationary_{k}" for k in range(N_STD_PICKS)] + ["burst_at_end", "long_200000"])


def stats(audio, dtype=np.float32):
    """(mean[20], std[20]) of the oracle for `audio` in `dtype` arithmetic."""
    return mfcc_ref.extract_mfcc(np.asarray(audio).astype(dtype))


def f32_template(audio):
    """The reference's template: WordMatcher.set_reference on float32 audio."""
    return stats(audio, np.float32)


def f64_template_rounded(audio):
    """The float64 statistics of the same float32 samples, rounded once to float32."""
    m, s = stats(np.asarray(audio, np.float32), np.float64)
    return m.astype(np.float32), s.astype(np.float32)


def template_drift(stats_a, stats_b, cand_stats) -> float:
    """max over candidates of |score(a, c) - score(b, c)|, pairs with a NaN ignored: how far
    the difference between two (mean, std) pairs moves a score when they serve as templates."""
    worst = 0.0
    for cm, cs in cand_stats:
        a = float(mfcc_ref.similarity_from_stats(stats_a[0], stats_a[1], cm, cs))
        b = float(mfcc_ref.similarity_from_stats(stats_b[0], stats_b[1], cm, cs))
        if np.isnan(a) or np.isnan(b):
            continue
        worst = max(worst, abs(a - b))
    return worst


@functools.lru_cache(maxsize=None)
def candidates():
    """The candidate batch: 40 ragged segments, ten fuzz segments and ten loud (x 1000) fuzz
    segments, without the constant ones (every log-mel value at the floor: parity unpinned)."""
    word = synth.load_word()
    segs = list(synth.ragged_segments(4321, 40, 160, 48000))
    segs += synth.fuzz_segments(3, 60, word)[:10]
    segs += [(x * np.float32(1000.0)).astype(np.float32) for x in synth.fuzz_segments(31, 60, word)[:10]]
    return tuple(x for x in segs if np.ptp(mfcc_ref.log_mel(x.astype(np.float64))) != 0.0)


@functools.lru_cache(maxsize=None)
def candidate_stats(dtype="float64"):
    """Oracle (mean, std) of every candidate in `dtype` arithmetic (computed once)."""
    return tuple(stats(x, np.dtype(dtype)) for x in candidates())


def reference_spread(audio) -> float:
    """template_drift between the oracle's float32 template and its float64 template rounded
    to float32: what the reference's own arithmetic leaves open for this recording."""
    return template_drift(f32_template(audio), f64_template_rounded(audio), candidate_stats())


def _norm(v) -> float:
    return float(np.linalg.norm(np.asarray(v, np.float64)))


def _pick(clips, key, n):
    """The first n clips in ascending `key` order that are longer than MIN_PICK_LEN and that
    the oracle pins (reference_spread <= SPREAD_CAP): (index, clip) pairs."""
    ranked = sorted((key(x), i) for i, x in enumerate(clips) if len(x) > MIN_PICK_LEN)
    out = []
    for _, i in ranked:
        if reference_spread(clips[i]) <= SPREAD_CAP:
            out.append((i, clips[i]))
            if len(out) == n:
                break
    return out


def _burst_at_end():
    """Quiet noise with a loud word burst in its last 0.3 s: top_db bites most tiles."""
    rng = np.random.Generator(np.random.PCG64(4101))
    word = synth.load_word()
    x = rng.normal(0, 1e-5, 24000).astype(np.float32)
    w = word[:4800] * np.float32(3.0)
    x[-len(w):] += w
    return x


def _long_recording():
    """Longer than the scorer's 1024-frame tile record, the word mid-way."""
    rng = np.random.Generator(np.random.PCG64(4102))
    word = synth.load_word()
    x = rng.normal(0, 1e-5, 200000).astype(np.float32)
    w = word * np.float32(2.5)
    s0 = (len(x) - len(w)) // 2
    x[s0:s0 + len(w)] += w
    return x


@functools.lru_cache(maxsize=None)
def recordings():
    """((name, float32 audio), ...): every reference recording of the parity tests."""
    word = synth.load_word()
    rng = np.random.Generator(np.random.PCG64(4100))
    noise = rng.normal(0, 0.01, 32000).astype(np.float32)
    recs = [("word", word),
            ("word_0.2s", word[2000:5200].copy()),
            ("word_0.4s", word[1000:7400].copy()),
            ("word_1600", word[2000:3600].copy()),
            ("word_2559", word[2000:4559].copy()),
            ("word_reversed", word[::-1].copy())]
    for g in (0.01, 30.0, 200.0, 1000.0):
        recs.append((f"word_x{g:g}", (word * np.float32(g)).astype(np.float32)))
    recs += [("tone440", synth.tone(440)), ("tone880_0.7s", synth.tone(880, 0.7)),
             ("speech_like", synth.speech_like()),
             ("noise", noise), ("noise_x1000", (noise * np.float32(1000.0)).astype(np.float32))]
    loud = [(x * np.float32(1000.0)).astype(np.float32) for x in synth.fuzz_segments(31, 60, word)]
    picks = _pick(loud, lambda x: _norm(f32_template(x)[0]), N_MEAN_PICKS)
    recs += [(f"vanishing_mean_{k}", x) for k, (_, x) in enumerate(picks)]
    steady = [x for seed in STD_SEEDS for x in synth.fuzz_segments(seed, 60, word)]
    picks = _pick(steady, lambda x: abs(_norm(f32_template(x)[1]) - 20.0), N_STD_PICKS)
    recs += [(f"stationary_{k}", x) for k, (_, x) in enumerate(picks)]
    recs += [("burst_at_end", _burst_at_end()), ("long_200000", _long_recording())]
    assert [n for n, _ in recs] == NAMES, "the selection rules found fewer clips than NAMES lists"
    return tuple((n, np.ascontiguousarray(x, dtype=np.float32)) for n, x in recs)


EDGE_LENGTHS = (2560, 2561, 48000, 48161, 60000, 100003)   # test_edge_lengths' lengths above 16 frames


@functools.lru_cache(maxsize=None)
def edge_recordings():
    """The tone of tests/test_gpu_scorer.py::test_edge_lengths at EDGE_LENGTHS (statistics only:
    these are scored, never set as templates)."""
    return tuple(np.full(n, 0.1, np.float32) * np.sin(np.arange(n, dtype=np.float32)) for n in EDGE_LENGTHS)


@functools.lru_cache(maxsize=None)
def oracle_template(name):
    """The reference's float32 template of a recording (computed once)."""
    return f32_template(recording(name))


def recording(name) -> np.ndarray:
    return dict(recordings())[name]


@functools.lru_cache(maxsize=None)
def describe(name):
    """{"mean_norm", "std_norm", "frames", "spread"} of a recording, by the oracle alone."""
    x = recording(name)
    m, s = f32_template(x)
    return {"mean_norm": _norm(m), "std_norm": _norm(s), "frames": mfcc_ref.n_frames(len(x)),
            "spread": reference_spread(x)}


@functools.lru_cache(maxsize=None)
def oracle_scores(name, dtype="float64"):
    """float64[n_candidates]: WordMatcherRef(recording).calculate_similarity(candidate.astype(dtype))."""
    tm, ts = oracle_template(name)
    return np.array([float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs)) for cm, cs in candidate_stats(dtype)])
