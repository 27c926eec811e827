"""The fp64 re-score (csrc/ewk_rescore.h) on every chunk shape and drain path of
tests/rescore_matrix.py, against oracle/mfcc_ref.py's float64 path at DESIGN.md's bar: mean and
std within 1e-9 x max(1, max|ref|), the score within 1e-9, the decision the oracle's.

Serial slots (`score_f64`: one wave a segment, every chunk in rs_finish), pooled slots
(rescore_margin = 1e9: every chunk through the part pool, the finishing wave reads maxima and
flags 64 chunks a round and merges the records), the float32 pass on the same inputs, and ring
sources (float32, int16 and compact int16 rings) with every event re-scored.  No case is skipped;
the only comparisons that are not with the oracle are the all-zero inputs (exact 0 std, NaN
score: DESIGN.md leaves parity unpinned for a constant log-mel) and the non-finite inputs (NaN).
tests/test_rescore_matrix.py shows on the CPU that every input reaches its path.  Each test
prints its figures per case before it asserts.
"""
import math

import numpy as np
import pytest

import rescore_matrix as rm
import synth
from golden_io import score_close
from oracle import mfcc_ref

pytestmark = pytest.mark.gpu

BAR = 1e-9
F32_BAR = 1e-4


@pytest.fixture(scope="module")
def serial():
    """score_f64 of every case: (mean, std, score), float64."""
    from easywakeword_amd import Engine
    e = Engine()
    e.set_template(*rm.template())
    out = e.score_f64([c.x for c in rm.cases()])
    e.close()
    return out


@pytest.fixture(scope="module")
def pooled():
    """Every case listed for the re-score and chunked through the part pool: (score, match)."""
    from easywakeword_amd import Engine
    e = Engine(rescore_margin=1e9)
    e.set_template(*rm.template())
    _, _, score, match = e.score([c.x for c in rm.cases()], candidate_dtype="float64")
    e.close()
    return score, match


def _worst(rows):
    """Per family: the worst |dmean| / scale, |dstd| / scale and |dscore| of (family, dm, dsd, ds) rows."""
    out = {}
    for fam, dm, dsd, ds in rows:
        w = out.setdefault(fam, [0.0, 0.0, 0.0])
        for k, v in enumerate((dm, dsd, ds)):
            if v is not None and not math.isnan(v):
                w[k] = max(w[k], v)
    return out


def test_serial_slots_vs_oracle(serial):
    mean, std, score = serial
    bad, rows = [], []
    for i, c in enumerate(rm.cases()):
        if c.expect == "nan":           # f: the reference propagates a non-finite sample
            ok = np.isnan(mean[i]).all() and np.isnan(std[i]).all() and math.isnan(score[i])
            print(f"{c.name}: NaN statistics {bool(ok)}")
            if not ok:
                bad.append((c.name, "not NaN", mean[i], std[i], score[i]))
            continue
        if c.expect == "zero_std":      # d-v
            ok = not std[i].any() and math.isnan(score[i]) and np.isfinite(mean[i]).all()
            print(f"{c.name}: std == 0 {not std[i].any()} score {score[i]}")
            if not ok:
                bad.append((c.name, "constant log-mel", std[i], score[i]))
            continue
        cm, cs, ref = rm.oracle(c)
        scale = max(1.0, float(np.abs(cm).max()))
        dm, dsd = float(np.abs(mean[i] - cm).max()) / scale, float(np.abs(std[i] - cs).max()) / scale
        ds = 0.0 if math.isnan(ref) and math.isnan(score[i]) else abs(score[i] - ref)
        rows.append((c.family, dm, dsd, ds))
        print(f"{c.name}: T={c.T} |dmean|/scale={dm:.3e} |dstd|/scale={dsd:.3e} |dscore|={ds:.3e} "
              f"score={score[i]!r} oracle={ref!r}")
        try:
            np.testing.assert_allclose(mean[i], cm, rtol=0, atol=BAR * scale)
            np.testing.assert_allclose(std[i], cs, rtol=0, atol=BAR * max(1.0, float(np.abs(cs).max())))
        except AssertionError as err:
            bad.append((c.name, str(err).strip().splitlines()[:6]))
        if not score_close(score[i], ref, BAR):
            bad.append((c.name, "score", float(score[i]), ref))
        if bool(score[i] >= 75.0) != bool(ref >= 75.0):
            bad.append((c.name, "decision", float(score[i]), ref))
    print("serial, worst per family (|dmean|/scale, |dstd|/scale, |dscore|):", _worst(rows))
    assert not bad, bad


def test_pooled_slots_vs_oracle(pooled, serial):
    score, match = pooled
    s_serial = serial[2]
    bad, rows = [], []
    for i, c in enumerate(rm.cases()):
        if not c.oracle:                 # d-v and f: NaN, no match
            print(f"{c.name}: score {score[i]} match {bool(match[i])}")
            if not (math.isnan(score[i]) and not match[i]):
                bad.append((c.name, float(score[i]), bool(match[i])))
            continue
        ref = rm.oracle(c)[2]
        ds = 0.0 if math.isnan(ref) and math.isnan(score[i]) else abs(score[i] - ref)
        dser = 0.0 if math.isnan(s_serial[i]) and math.isnan(score[i]) else abs(score[i] - s_serial[i])
        rows.append((c.family, None, None, ds))
        print(f"{c.name}: chunks={c.n_chunks} |dscore|={ds:.3e} |pooled - serial|={dser:.3e} score={score[i]!r}")
        if not score_close(score[i], ref, BAR):
            bad.append((c.name, "score", float(score[i]), ref))
        if bool(match[i]) != bool(ref >= 75.0):
            bad.append((c.name, "decision", float(score[i]), ref))
        if not score_close(score[i], s_serial[i], BAR):
            bad.append((c.name, "pooled vs serial", float(score[i]), float(s_serial[i])))
    print("pooled, worst |dscore| per family:", {f: w[2] for f, w in _worst(rows).items()})
    assert not bad, bad


def test_pooled_results_do_not_depend_on_the_batch():
    """The shaped cases alone and spread over a batch of 64: which waves ran which chunks, and
    which wave finished a slot, must not matter -- the same bits."""
    from easywakeword_amd import Engine
    shaped = rm.shaped()
    fill = synth.ragged_segments(2610, 64 - len(shaped))
    batch, where = list(fill), []
    for k, c in enumerate(shaped):
        where.append(3 + 4 * k + k)           # 3, 8, 13, ...: between the fillers
        batch.insert(where[-1], c.x)
    assert len(batch) == 64 and all(batch[w] is c.x for w, c in zip(where, shaped))
    e = Engine(rescore_margin=1e9)
    try:
        e.set_template(*rm.template())
        _, _, s_alone, m_alone = e.score([c.x for c in shaped], candidate_dtype="float64")
        _, _, s_batch, m_batch = e.score(batch, candidate_dtype="float64")
    finally:
        e.close()
    for k, c in enumerate(shaped):
        print(f"{c.name}: alone {s_alone[k]!r} in the batch {s_batch[where[k]]!r}")
    np.testing.assert_array_equal(s_batch[where].view(np.int64), s_alone.view(np.int64))
    np.testing.assert_array_equal(m_batch[where], m_alone)
    assert np.isfinite(s_alone).sum() >= len(shaped) - 2      # (b with k = 0 and e: the oracle's NaN)


def test_float32_pass_on_the_same_inputs():
    """The default engine (float32 pass, re-score by its own criteria) on cases a-d at the suite's
    float32 bar: the dummy-frame and late-max inputs are as pointed for k_score_f32's partial last
    pass as for the re-score."""
    from easywakeword_amd import Engine
    cases = rm.by_family("a", "b", "c", "d")
    e = Engine()
    try:
        e.set_template(*rm.template())
        _, _, score, match = e.score([c.x for c in cases], candidate_dtype="float64")
    finally:
        e.close()
    bad = []
    for i, c in enumerate(cases):
        if not c.oracle:                 # d-v: the engine's NaN
            print(f"{c.name}: score {score[i]} match {bool(match[i])}")
            if not (math.isnan(score[i]) and not match[i]):
                bad.append((c.name, float(score[i])))
            continue
        ref = rm.oracle(c)[2]
        ds = 0.0 if math.isnan(ref) and math.isnan(score[i]) else abs(score[i] - ref)
        print(f"{c.name}: |dscore|={ds:.3e} score={score[i]!r}")
        if not score_close(score[i], ref, F32_BAR) or bool(match[i]) != bool(ref >= 75.0):
            bad.append((c.name, float(score[i]), ref, bool(match[i])))
    assert not bad, bad


def test_ring_every_event_rescored_int16_and_compact():
    """The ten PCM16 streams of test_gpu_int16_ring.py with every event listed for the re-score,
    on float32 rings (RsSrc<1>), int16 rings (RsSrc<2>) and compact int16 rings, where segments
    straddle the physical end (the wrap in rs_sample): the same events bit for bit, each
    re-scored, each score -- all of them -- within 1e-9 of the oracle's float64 score."""
    from easywakeword_amd import StreamEngine, _lib
    q = rm.pcm16_streams()
    runs = []
    for cfg in (dict(), dict(ring_format=1), dict(ring_format=1, ring_samples=rm.COMPACT_RING)):
        eng = StreamEngine(q.shape[0], rescore_margin=1e9, **cfg)
        try:
            eng.set_template(*rm.template())
            got = []
            for c in range(0, q.shape[1], 9 * 1600):
                eng.push_pcm16(q[:, c:c + 9 * 1600])
                got.append(eng.poll())
        finally:
            eng.close()
        runs.append(np.concatenate(got))
    ev_f = runs[0]
    for ev in runs[1:]:
        for f in ("stream", "tick", "length", "flags", "match"):
            np.testing.assert_array_equal(ev[f], ev_f[f], err_msg=f)
        np.testing.assert_array_equal(ev["score"].view(np.int64), ev_f["score"].view(np.int64))
    tm, ts = rm.template()
    ref_events = rm.ring_oracle_events()
    n_scored, n_straddle, worst, bad = 0, 0, 0.0, []
    for i in range(q.shape[0]):
        mine = ev_f[ev_f["stream"] == i]
        compact = runs[2][runs[2]["stream"] == i]
        assert [(int(m["tick"]), int(m["length"]), bool(m["flags"] & _lib.EWK_EV_SKIPPED)) for m in mine] == \
               [(e.tick, e.length, e.skipped) for e in ref_events[i]], i
        for m, mc, e in zip(mine, compact, ref_events[i]):
            if e.skipped:
                continue
            score = float(m["score"])
            assert m["flags"] & _lib.EWK_EV_RESCORED or math.isnan(score), (i, m)
            cm, cs = mfcc_ref.extract_mfcc(e.audio)
            s = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
            ds = 0.0 if math.isnan(s) and math.isnan(score) else abs(score - s)
            across = int(mc["ring_start"]) + int(mc["length"]) > rm.COMPACT_RING
            assert across == rm.straddles(e.tick, e.n_request, e.length)
            print(f"stream {i} tick {e.tick}: length {e.length} across the compact ring's end {across} "
                  f"|dscore|={ds:.3e} score={score!r}")
            if not score_close(score, s, BAR) or bool(m["match"]) != (s >= 75.0):
                bad.append((i, e.tick, score, s))
            n_scored += 1
            n_straddle += across
            worst = max(worst, ds) if not math.isnan(ds) else worst
    print(f"ring: {n_scored} events, {n_straddle} across the compact ring's end, worst |dscore| = {worst:.3e}")
    assert not bad, bad
    assert n_scored >= 15 and n_straddle >= 3


def test_redo_all_and_nan_flag_with_a_finite_score():
    """With the word's template a huge segment's score is NaN, and a segment whose float32
    statistics are not finite is listed only when T <= 16.  Against the statistics of another huge
    segment the score is finite: the serial slot of e, and pooled slots of two chunks (T = 15, 16)
    whose finishing wave meets redo_all -- or a part record's NaN flag -- must give the oracle's."""
    from easywakeword_amd import Engine
    short = rm.short_cases()
    e_huge = next(c for c in rm.cases() if c.name == "e_huge")
    f = Engine()
    p = Engine(rescore_margin=1e9)
    try:
        f.set_template(*rm.huge_template())
        p.set_template(*rm.huge_template())
        mean, std, s_serial = f.score_f64([c.x for c in [e_huge] + short])
        _, _, s_pool, m_pool = p.score([c.x for c in short], candidate_dtype="float64")
    finally:
        f.close()
        p.close()
    bad = []
    for i, c in enumerate([e_huge] + short):
        got = [("serial", s_serial[i])] + ([("pooled", s_pool[i - 1])] if i else [])
        if c.oracle:
            cm, cs, _ = rm.oracle(c)
            np.testing.assert_allclose(mean[i], cm, rtol=0, atol=BAR * max(1.0, float(np.abs(cm).max())), err_msg=c.name)
            np.testing.assert_allclose(std[i], cs, rtol=0, atol=BAR * max(1.0, float(np.abs(cs).max())), err_msg=c.name)
        for how, s in got:
            if c.expect == "nan":
                print(f"{c.name} {how}: score {s}")
                if not math.isnan(s):
                    bad.append((c.name, how, float(s)))
                continue
            ref = rm.huge_score(c)
            print(f"{c.name} {how}: |dscore|={abs(s - ref):.3e} score={s!r} oracle={ref!r}")
            if not score_close(s, ref, BAR):
                bad.append((c.name, how, float(s), ref))
        if i and bool(m_pool[i - 1]) != (c.oracle and rm.huge_score(c) >= 75.0):
            bad.append((c.name, "decision", bool(m_pool[i - 1])))
    assert not bad, bad
