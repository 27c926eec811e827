"""The template-bank test batch (tests/test_gpu_bank.py): a bank of three words with 1, 3 and
64 templates (K = 68, word_first = [0, 1, 4, 68]: unaligned) made from distinct audio, 96
ragged segments with the word index cycling 0, 1, 2, and the CPU oracle's scores for them.

SEED was chosen with the oracle alone (templates from oracle.mfcc_ref on the CPU): no segment's
two best scores within its word are closer than 1e-3, so the argmax over a word's templates is
unambiguous at the 1e-4 score bar (check_margin() recomputes it; test_bank_layout.py runs it).
"""
import numpy as np

import synth
from oracle import mfcc_ref

SEED = 20240
N_SEG = 96
SIZES = (1, 3, 64)
THRESHOLDS = (96.0, 92.0, 86.0)   # each splits its word's scores (a few within 1e-3: re-scored)
TIE = 2e-4          # two oracle scores closer than this may swap rank within the 1e-4 bar


def bank_audio():
    """[[word], [3 clips], [64 clips]]: the word, tones, speech-like clips, fuzzed word bursts."""
    word = synth.load_word()
    w1 = [synth.tone(440), synth.tone(880, 0.7), synth.speech_like(0.8)]
    w2 = [synth.tone(f, 0.5 + 0.05 * i) for i, f in enumerate(range(200, 4200, 250))]              # 16
    w2 += [synth.speech_like(0.4 + 0.15 * i) for i in range(12)]                                    # 12
    w2 += [word[::-1].copy(), (word * np.float32(0.5)).astype(np.float32), word[2000:9000].copy()]  # 3
    fz = [x for x in synth.fuzz_segments(77, 60, word) if len(x) >= 3200]
    w2 += fz[:64 - len(w2)]
    assert len(w2) == 64
    return [[word], w1, w2]


def segments(seed: int = SEED, n: int = N_SEG):
    """n ragged segments of 160..48,000 samples (several of at most 16 frames) and their words."""
    segs = synth.ragged_segments(seed, n, 160, 48000)
    short = synth.ragged_segments(seed + 1, 8, 160, 2559)      # <= 16 frames: always fp64
    for k, s in enumerate(short):
        segs[11 * k + 3] = s
    return segs, np.arange(n, dtype=np.int32) % len(SIZES)


def oracle_templates(dtype=np.float32):
    """(mean[K, 20], std[K, 20]) of the bank's audio by the CPU oracle, as float32 templates."""
    st = [mfcc_ref.extract_mfcc(a.astype(dtype)) for w in bank_audio() for a in w]
    return (np.array([m for m, _ in st], np.float32), np.array([s for _, s in st], np.float32))


def oracle_scores(segs, word, tmean, tstd, dtype=np.float64, sizes=SIZES):
    """scores[n, 64] of segment i against template j of its word (NaN past the word's size),
    candidates in `dtype` (float64: the streaming arithmetic; float32: WordMatcher's)."""
    first = np.concatenate([[0], np.cumsum(sizes)])
    out = np.full((len(segs), 64), np.nan)
    for i, x in enumerate(segs):
        cm, cs = mfcc_ref.extract_mfcc(np.asarray(x).astype(dtype))
        w = int(word[i])
        for j in range(sizes[w]):
            k = first[w] + j
            out[i, j] = float(mfcc_ref.similarity_from_stats(tmean[k], tstd[k], cm, cs))
    return out


def top2_gap(scores):
    """Per row: best - second best over the finite scores (inf with fewer than two)."""
    gap = np.full(len(scores), np.inf)
    for i, r in enumerate(scores):
        f = np.sort(r[np.isfinite(r)])
        if f.size >= 2:
            gap[i] = f[-1] - f[-2]
    return gap


def check_margin():
    segs, word = segments()
    tm, ts = oracle_templates()
    return top2_gap(oracle_scores(segs, word, tm, ts))
