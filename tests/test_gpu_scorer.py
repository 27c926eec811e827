"""Level-2 parity on the GPU: HIP scorer vs the golden fixtures made from the
reference code (tests/golden/make_golden.py) and vs the CPU oracle.

Bar (BASELINE.json north star): similarity scores within 1e-4 (NaN == NaN)
and identical match decisions.  MFCC mean/std within rtol 1e-4 / atol 2e-3.
"""
import math

import numpy as np
import pytest

import synth
import template_cases
from golden_io import matcher_fixture, score_close, template_arrays
from oracle import mfcc_ref

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4


@pytest.fixture(scope="module")
def engine():
    from easywakeword_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def fixture():
    return matcher_fixture()


def test_template_from_wav_matches_reference(engine, fixture):
    fx, _ = fixture
    engine.template_from_pcm(synth.load_word())
    m, s = engine.get_template()
    tm, ts = template_arrays(fx)
    np.testing.assert_allclose(m, tm, rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(s, ts, rtol=1e-4, atol=2e-3)
    # the tolerances above let through errors that move scores by several 1e-4 (a 1e-3 error per
    # coefficient: 2.5e-4, tests/test_template_cases.py); the bar itself, in score units:
    drift = template_cases.template_drift((m, s), (tm, ts), template_cases.candidate_stats())
    print("template drift vs the reference's template =", drift)
    assert drift <= SCORE_TOL


@pytest.mark.parametrize("ref_dtype", ["float64", "float32"])
def test_golden_scores_and_decisions(engine, fixture, ref_dtype):
    fx, audio = fixture
    engine.set_template(*template_arrays(fx))
    engine.set_threshold(75.0)
    names = [c["name"] for c in fx["cases"]]
    mean, std, score, match = engine.score([audio[n] for n in names], candidate_dtype=ref_dtype)
    bad = []
    for i, c in enumerate(fx["cases"]):
        ref = c[ref_dtype]
        if ref_dtype == "float32" and c["name"].startswith("silence"):
            continue   # reference float32 silence is a rounding artefact
        if not score_close(score[i], ref["score"], SCORE_TOL):
            bad.append((c["name"], float(score[i]), ref["score"]))
        if bool(match[i]) != ref["match"]:
            bad.append((c["name"], "decision", bool(match[i]), ref["match"]))
        if ref["score"] is not None:
            np.testing.assert_allclose(mean[i], ref["mean"], rtol=1e-4, atol=2e-3, err_msg=c["name"])
            np.testing.assert_allclose(std[i], ref["std"], rtol=1e-4, atol=2e-3, err_msg=c["name"])
    assert not bad, bad


def test_fp64_path_matches_float64_reference_tightly(engine, fixture):
    fx, audio = fixture
    engine.set_template(*template_arrays(fx))
    names = [c["name"] for c in fx["cases"]]
    mean, std, score = engine.score_f64([audio[n] for n in names])
    for i, c in enumerate(fx["cases"]):
        ref = c["float64"]
        assert score_close(score[i], ref["score"], 1e-9), (c["name"], score[i], ref["score"])
        np.testing.assert_allclose(mean[i], ref["mean"], rtol=1e-9, atol=1e-9, err_msg=c["name"])
        np.testing.assert_allclose(std[i], ref["std"], rtol=1e-9, atol=1e-9, err_msg=c["name"])


def test_random_ragged_batch_vs_oracle(engine):
    word = synth.load_word()
    engine.template_from_pcm(word)
    tm, ts = engine.get_template()
    segs = synth.ragged_segments(4321, 200, 160, 48000)
    _, _, score, match = engine.score(segs, candidate_dtype="float64")
    worst = 0.0
    for i, x in enumerate(segs):
        cm, cs = mfcc_ref.extract_mfcc(x.astype(np.float64))
        ref = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
        assert score_close(score[i], ref, SCORE_TOL), (i, len(x), score[i], ref)
        assert bool(match[i]) == (ref >= 75.0)
        if not math.isnan(ref):
            worst = max(worst, abs(score[i] - ref))
    print("max |score - oracle| =", worst)


def test_reference_unit_expectations():
    """tests/test_wakeword_simulated.py:104-205, 330-360 and test_cross_platform.py:69-109."""
    from easywakeword_amd import WordMatcher
    m = WordMatcher(sample_rate=16000)
    a440 = synth.tone(440)
    m.set_reference(a440, "test")
    ok, s = m.matches(a440)
    assert ok and s == 100.0
    ok, s = m.matches(synth.tone(440))
    assert ok and s == 100.0
    _, s880 = m.matches(synth.tone(880))
    assert s880 < 100.0
    rs = np.random.RandomState(42)
    _, sn = m.matches(rs.randn(16000).astype(np.float32) * np.float32(0.1))
    assert sn < 100.0
    assert m.matches(a440 * np.float32(0.5), threshold=75.0)[1] > 50.0
    sp = synth.speech_like()
    m.set_reference(sp, "speech")
    ok, s = m.matches(sp)
    assert ok and s == 100.0
    mean, std = m.extract_mfcc(sp)
    assert mean.shape == (20,) and std.shape == (20,) and np.all(np.isfinite(mean))
    # LEARNINGS.md:92-94 observations: 880 Hz ~89 %, noise ~77 %+, silence NaN
    m.set_reference(a440, "ref")
    assert 89.0 < m.calculate_similarity(synth.tone(880)) < 90.5
    assert m.calculate_similarity(rs.randn(16000).astype(np.float32) * np.float32(0.1)) > 77.0
    assert math.isnan(m.calculate_similarity(np.zeros(16000, np.float32)))
    with pytest.raises(ValueError, match="No reference word set"):
        WordMatcher().calculate_similarity(np.zeros(16000, np.float32))


def test_near_threshold_decisions_are_exact(engine):
    """A threshold placed exactly on the float64 score must decide like the
    reference (score >= threshold) -> the fp32 score falls inside the rescore
    margin and the fp64 path decides."""
    engine.template_from_pcm(synth.load_word())
    segs = synth.ragged_segments(99, 12, 8000, 30000)
    _, _, s64 = engine.score_f64(segs)
    for i, x in enumerate(segs):
        if math.isnan(s64[i]):
            continue
        engine.set_threshold(float(s64[i]))
        _, _, sc, mt = engine.score([x], candidate_dtype="float64")
        assert bool(mt[0]), (i, sc[0], s64[i])
        engine.set_threshold(float(np.nextafter(s64[i], np.inf)))
        _, _, sc, mt = engine.score([x], candidate_dtype="float64")
        assert not bool(mt[0]), (i, sc[0], s64[i])
    engine.set_threshold(75.0)


def test_edge_lengths(engine):
    engine.template_from_pcm(synth.load_word())
    tm, ts = engine.get_template()
    segs = [np.full(n, 0.1, np.float32) * np.sin(np.arange(n, dtype=np.float32)) for n in
            (1, 2, 159, 160, 161, 255, 256, 257, 511, 512, 513, 2559, 2560, 2561, 48000, 48161, 60000, 100003)]
    _, _, score, _ = engine.score(segs, candidate_dtype="float64")
    for i, x in enumerate(segs):
        cm, cs = mfcc_ref.extract_mfcc(x.astype(np.float64))
        ref = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
        assert score_close(score[i], ref, SCORE_TOL), (len(x), score[i], ref)


def test_longest_first_order_is_bit_identical(engine):
    """Batches with more segments than 2 x the resident waves are handed out longest
    first (k_lpt_order); every output must equal the index-order result of small
    batches, bit for bit (each segment is scored by one wave, independently)."""
    engine.template_from_pcm(synth.load_word())
    rng = np.random.Generator(np.random.PCG64(77))
    segs = [rng.normal(0, 0.01, int(n)).astype(np.float32) for n in rng.integers(200, 40000, 4500)]
    segs += [np.zeros(0, np.float32), np.zeros(100, np.float32)] + [synth.load_word()] * 10
    m1, s1, sc1, mt1 = engine.score(segs, candidate_dtype="float64")     # > 4096 segments: LPT order
    parts = [engine.score(segs[i:i + 1500], candidate_dtype="float64") for i in range(0, len(segs), 1500)]
    m2 = np.concatenate([p[0] for p in parts]); s2 = np.concatenate([p[1] for p in parts])
    sc2 = np.concatenate([p[2] for p in parts]); mt2 = np.concatenate([p[3] for p in parts])
    np.testing.assert_array_equal(m1, m2)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_array_equal(sc1, sc2)     # NaN == NaN in assert_array_equal
    np.testing.assert_array_equal(mt1, mt2)


def test_speculative_top_db_clamp(engine):
    """Pass 1 clamps each 16-frame tile at the running segment max - 80 dB
    (top_db), the tiles taken loudest first by a sample scout.  A
    loud burst placed in the last tile, the first tile or mid-way, and a tone in the last
    0.2 s (a single loud tile the scout must find) -- every quiet tile the threshold bites
    is either exact in pass 1 or recomputed.  All must equal the oracle, and a quiet tail
    after the burst must not be clamped at a stale threshold."""
    engine.template_from_pcm(synth.load_word())
    tm, ts = engine.get_template()
    rng = np.random.Generator(np.random.PCG64(5))
    word = synth.load_word()
    segs = []
    for L in (16000, 30000, 47000):
        for where in (0.0, 0.5, 1.0):
            x = rng.normal(0, 1e-5, L).astype(np.float32)   # ~ -100 dB floor, far below max - 80
            w = word[: min(len(word), L // 3)] * np.float32(3.0)
            s0 = int(where * (L - len(w)))
            x[s0:s0 + len(w)] += w
            segs.append(x)
        # loud 880 Hz tone in the last 0.2 s only: every earlier tile is fixed up
        t = np.arange(3200) / 16000
        y = rng.normal(0, 1e-4, L).astype(np.float32)
        y[-3200:] += (0.9 * np.sin(2 * np.pi * 880 * t)).astype(np.float32)
        segs.append(y)
    _, _, score, match = engine.score(segs, candidate_dtype="float64")
    for i, x in enumerate(segs):
        cm, cs = mfcc_ref.extract_mfcc(x.astype(np.float64))
        ref = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
        assert score_close(score[i], ref, SCORE_TOL), (i, len(x), score[i], ref)
        assert bool(match[i]) == (ref >= 75.0)


def test_extract_mfcc_keeps_the_input_dtype():
    """float64 input returns float64 stats like the reference (the device's
    fp64 path, within 1e-9 of the float64 oracle); float32 input returns float32."""
    from easywakeword_amd import WordMatcher
    m = WordMatcher()
    for x in (synth.load_word(), synth.speech_like(), synth.ragged_segments(77, 1, 20000, 20000)[0]):
        m64, s64 = m.extract_mfcc(x.astype(np.float64))
        assert m64.dtype == np.float64 and s64.dtype == np.float64
        rm, rs = mfcc_ref.extract_mfcc(x.astype(np.float64))
        np.testing.assert_allclose(m64, rm, rtol=0, atol=1e-9 * max(1.0, float(np.abs(rm).max())))
        np.testing.assert_allclose(s64, rs, rtol=0, atol=1e-9 * max(1.0, float(np.abs(rs).max())))
        m32, s32 = m.extract_mfcc(x.astype(np.float32))
        assert m32.dtype == np.float32 and s32.dtype == np.float32


def test_top_db_past_the_tile_record(engine):
    """Segments longer than the per-wave tile record (kSpecTiles = 48 tiles, 768 frames):
    taken in time order, the tiles past the record are stored unclamped and always
    recomputed when top_db bites -- a loud burst early, mid-way or at the end of 12-20 s
    of quiet noise must still equal the oracle."""
    engine.template_from_pcm(synth.load_word())
    tm, ts = engine.get_template()
    rng = np.random.Generator(np.random.PCG64(8))
    word = synth.load_word()
    segs = []
    for L, where in ((192000, 0.1), (200000, 0.55), (320000, 1.0)):
        x = rng.normal(0, 1e-5, L).astype(np.float32)
        w = word * np.float32(2.5)
        s0 = int(where * (L - len(w)))
        x[s0:s0 + len(w)] += w
        segs.append(x)
    _, _, score, match = engine.score(segs, candidate_dtype="float64")
    for i, x in enumerate(segs):
        cm, cs = mfcc_ref.extract_mfcc(x.astype(np.float64))
        ref = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
        assert score_close(score[i], ref, SCORE_TOL), (i, len(x), score[i], ref)
        assert bool(match[i]) == (ref >= 75.0)


def _fuzz_vs_oracle(engine, seed, n, gain=1.0):
    engine.template_from_pcm(synth.load_word())
    tm, ts = engine.get_template()
    segs = [(x * np.float32(gain)).astype(np.float32) for x in synth.fuzz_segments(seed, n, synth.load_word())]
    _, _, score, match = engine.score(segs, candidate_dtype="float64")
    n_const = 0
    for i, x in enumerate(segs):
        if np.ptp(mfcc_ref.log_mel(x.astype(np.float64))) == 0.0:
            # every log-mel value at the -100 dB floor: all frames identical, zero std; the
            # reference's float64 score is then a rounding artefact of numpy's pairwise mean
            # over pocketfft's DCT noise (NaN or some finite value depending on T) -- parity
            # unpinned; the engine returns NaN (numerics)
            assert math.isnan(score[i]) and not match[i], (i, score[i])
            n_const += 1
            continue
        cm, cs = mfcc_ref.extract_mfcc(x.astype(np.float64))
        ref = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
        assert score_close(score[i], ref, SCORE_TOL), (seed, i, len(x), score[i], ref)
        assert bool(match[i]) == (ref >= 75.0), (seed, i, score[i], ref)
    return n_const


def test_top_db_order_fuzz(engine):
    """Randomised segments for the loudest-first order, the self-clamp and the recompute of
    tiles the final top_db threshold bites: 0-4 bursts of random level (0-100 dB above a
    random noise floor) at random places, stretches of digital silence (the -100 dB amin
    floor), equal-energy tiles (ties in the scout ranking), lengths 1-60000 samples.  Every
    score must equal the oracle's within 1e-4 with the same decision."""
    n_const = _fuzz_vs_oracle(engine, 2024, 120)
    assert 0 < n_const < 10


@pytest.mark.parametrize("seed", [31, 33])
def test_fuzz_loud_segments_vanishing_mean(engine, seed):
    """The recipe 60 dB louder (samples up to ~1e3, un-normalised float audio): log-mel values
    average near 0 dB, c0 cancels and the MFCC mean vector nearly vanishes (|mean| 5-30), so
    float32 rounding moved the score by up to 7e-4 before such segments (|mean| < 64; the bench's
    batch has >= 154) went to the fp64 re-score in linear batches (DESIGN.md numerics)."""
    _fuzz_vs_oracle(engine, seed, 200, gain=1000.0)


@pytest.mark.parametrize("seed", [3, 5, 7, 12])
def test_fuzz_stationary_segments(engine, seed):
    """More seeds of the same recipe, the ones whose steady-noise segments (MFCC std vectors
    of norm 2-8, no speech contrast) missed 1e-4 by up to 2.9e-4 in float32 before such
    segments (|std| < 20; the bench's ragged batch has >= 24.8, the streaming recipe's
    events >= 32.5) went to the fp64 re-score (scripts/fuzz_err.py, scripts/std_norm_dist.py)."""
    _fuzz_vs_oracle(engine, seed, 200)


def test_non_finite_samples_do_not_disturb_the_batch(engine):
    """NaN / Inf samples (corrupt input) give the reference's NaN score -- librosa propagates
    them -- without disturbing the other segments of the batch (the scout's ranking and the
    per-tile record must stay well formed)."""
    engine.template_from_pcm(synth.load_word())
    tm, ts = engine.get_template()
    word = synth.load_word()
    rng = np.random.Generator(np.random.PCG64(12))
    good = [rng.normal(0, 1e-3, 24000).astype(np.float32) for _ in range(6)]
    for g in good:
        g[5000:5000 + len(word)] += word
    bad = []
    for k, val in enumerate((np.nan, np.inf, -np.inf)):
        x = rng.normal(0, 1e-3, 20000 + 3000 * k).astype(np.float32)
        x[[100, 7000, 15000]] = val
        bad.append(x)
    segs = [good[0], bad[0], good[1], good[2], bad[1], good[3], bad[2], good[4], good[5]]
    _, _, score, match = engine.score(segs, candidate_dtype="float64")
    for i, x in enumerate(segs):
        if not np.all(np.isfinite(x)):
            assert math.isnan(score[i]) and not match[i], (i, score[i])
            continue
        cm, cs = mfcc_ref.extract_mfcc(x.astype(np.float64))
        ref = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
        assert score_close(score[i], ref, SCORE_TOL), (i, score[i], ref)


def test_every_segment_rescored_part_pool_overflow():
    """rescore_margin = 1e9 lists every segment of a 1,500-segment batch for the fp64 re-score:
    ~24,000 8-frame chunks against the engine's 16,384 part records, so the slots listed after
    the pool runs out go serial (one wave each, claimed from their own list after every chunk
    is taken).  Every score must equal the fp64 API's (ewk_score_segments_f64, every slot
    serial) within 1e-9, and every decision must follow it; a sample spread over the batch
    (pooled and serial slots alike) must equal the oracle's float64 path within 1e-9."""
    from easywakeword_amd import Engine
    segs = synth.ragged_segments(2024, 1500, 6400, 40000)
    e = Engine(rescore_margin=1e9)
    f = Engine()
    try:
        e.template_from_pcm(synth.load_word())
        f.template_from_pcm(synth.load_word())
        _, _, s64 = f.score_f64(segs)
        _, _, sc, mt = e.score(segs, candidate_dtype="float64")
        ok = np.isfinite(s64)
        assert np.array_equal(np.isnan(sc), np.isnan(s64))
        assert float(np.max(np.abs(sc[ok] - s64[ok]))) <= 1e-9
        assert np.array_equal(mt.astype(bool)[ok], s64[ok] >= 75.0)
        tm, ts = e.get_template()
        for i in range(0, len(segs), 94):   # 16 segments over the listing order's whole range
            cm, cs = mfcc_ref.extract_mfcc(np.asarray(segs[i], dtype=np.float64))
            ref = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
            assert score_close(sc[i], ref, 1e-9), (i, sc[i], ref)
    finally:
        e.close()
        f.close()
