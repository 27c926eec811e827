"""Template parity on the GPU: templates the engine derives itself (template_from_pcm,
bank_from_pcm, WordMatcher.set_reference / set_references, the mean / std Engine.score hands out)
against the reference's, end to end.

The reference side is always the CPU oracle's WordMatcherRef: its template is
extract_mfcc(audio.astype(float32)), as WordMatcher.set_reference computes it in the reference;
the oracle never sees an engine-derived template here, so an error in the template statistics
cannot cancel.  Bar: scores within 1e-4 (NaN == NaN), identical decisions outside 1e-4 of the
threshold, and -- for statistics on their own -- tests/template_cases.py's template_drift <= 1e-4:
the error may not move any candidate's score by more than the bar when the statistics serve as a
template.  The recordings, the candidate batch and the oracle's numbers are built once
(template_cases, checked without a GPU by tests/test_template_cases.py)."""
import numpy as np
import pytest

import bank_cases as bc
import template_cases as tc
from golden_io import gate_fixture, score_close, sha, stream_pcm
from oracle import mfcc_ref

pytestmark = pytest.mark.gpu

BAR = tc.BAR
BANK_SIZES = (1, 3, len(tc.NAMES) - 4)     # the recordings as three words, in NAMES order


@pytest.fixture(scope="module")
def engine():
    from easywakeword_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def bare_engine():
    """An engine that never gets a template (statistics-only scoring)."""
    from easywakeword_amd import Engine
    e = Engine()
    yield e
    e.close()


def _drift(stats, name):
    return tc.template_drift(stats, tc.oracle_template(name), tc.candidate_stats())


@pytest.mark.parametrize("name", tc.NAMES)
def test_scores_end_to_end(engine, name):
    """template_from_pcm(recording), then the candidate batch: every score and decision against
    WordMatcherRef with the same recording as its reference, float64 and float32 candidates."""
    engine.set_threshold(tc.THRESHOLD)
    engine.template_from_pcm(tc.recording(name))
    cands = list(tc.candidates())
    bad = []
    for dt in ("float64", "float32"):
        _, _, score, match = engine.score(cands, candidate_dtype=dt)
        ref = tc.oracle_scores(name, dt)
        ok = np.isfinite(ref) & np.isfinite(score)
        worst = float(np.max(np.abs(score[ok] - ref[ok]))) if ok.any() else 0.0
        print(f"{name} {dt}: max |score - reference| = {worst:.3g} over {int(ok.sum())} finite scores")
        for i in range(len(cands)):
            if not score_close(score[i], ref[i], BAR):
                bad.append((dt, i, len(cands[i]), float(score[i]), float(ref[i])))
            if abs(ref[i] - tc.THRESHOLD) > BAR and bool(match[i]) != bool(ref[i] >= tc.THRESHOLD):
                bad.append((dt, i, "decision", bool(match[i]), float(ref[i])))
    assert not bad, bad[:10]


@pytest.mark.parametrize("name", tc.NAMES)
def test_template_statistics(engine, name):
    """The derived template on its own: places a failure of the end-to-end test on the template
    side or on the candidate side."""
    engine.template_from_pcm(tc.recording(name))
    d = _drift(engine.get_template(), name)
    print(f"{name}: template drift = {d:.3g}")
    assert d <= BAR


def _check_returned(mean, std, names, what):
    bad = []
    for i, n in enumerate(names):
        d = _drift((mean[i], std[i]), n)
        print(f"{what} {n}: drift = {d:.3g}")
        if not d <= BAR:
            bad.append((n, d))
    assert not bad, (what, bad)


@pytest.mark.parametrize("candidate_dtype", ["float64", "float32"])
def test_returned_statistics_as_templates(engine, bare_engine, candidate_dtype):
    """The mean / std that Engine.score returns are handed out as statistics and are what
    bank_from_pcm stores: held to the same drift bound, with a template set (the vanishing-mean,
    stationary and short recordings are then on the fp64 re-score list) and with none."""
    recs = [x for _, x in tc.recordings()]
    engine.template_from_pcm(tc.recording("word"))
    m, s, _, _ = engine.score(recs, candidate_dtype=candidate_dtype)
    _check_returned(m, s, tc.NAMES, "template set,")
    m, s, _, _ = bare_engine.score(recs, require_template=False, candidate_dtype=candidate_dtype)
    _check_returned(m, s, tc.NAMES, "no template,")


def test_returned_statistics_of_edge_lengths(engine, bare_engine):
    """The same bound at test_edge_lengths' lengths above 16 frames (tile and record edges)."""
    segs = list(tc.edge_recordings())
    engine.template_from_pcm(tc.recording("word"))
    for what, (m, s, _, _) in (("template set", engine.score(segs, candidate_dtype="float32")),
                              ("no template", bare_engine.score(segs, require_template=False))):
        for i, x in enumerate(segs):
            d = tc.template_drift((m[i], s[i]), tc.f32_template(x), tc.candidate_stats())
            print(f"{what}, length {len(x)}: drift = {d:.3g}")
            assert d <= BAR, (what, len(x), d)


def test_extract_mfcc_as_templates(bare_engine):
    """WordMatcher.extract_mfcc on float32 audio returns the statistics a caller may assign as
    reference_mfcc_mean / reference_mfcc_std: the same bound."""
    from easywakeword_amd import WordMatcher
    wm = WordMatcher(engine=bare_engine)
    bad = []
    for name, x in tc.recordings():
        d = _drift(wm.extract_mfcc(x.astype(np.float32)), name)
        print(f"extract_mfcc {name}: drift = {d:.3g}")
        if not d <= BAR:
            bad.append((name, d))
    assert not bad, bad


def _words(audios, sizes):
    out, k = [], 0
    for s in sizes:
        out.append(audios[k:k + s])
        k += s
    assert k == len(audios)
    return out


def test_every_derivation_agrees_bitwise(engine):
    """The template of a recording must not depend on the entry point or on its neighbours in the
    batch: template_from_pcm, bank_from_pcm in two orders and word layouts, and
    WordMatcher.set_reference / set_references give the same bits."""
    from easywakeword_amd import WordMatcher
    recs = [x for _, x in tc.recordings()]
    n = len(recs)
    single = []
    for x in recs:
        engine.template_from_pcm(x)
        single.append(engine.get_template())
    try:
        engine.bank_from_pcm(_words(recs, BANK_SIZES))
        bank_a = [engine.bank_template(k) for k in range(n)]
        engine.bank_from_pcm(_words(recs[::-1], (n - 7, 2, 5)))
        bank_b = [engine.bank_template(n - 1 - k) for k in range(n)]
    finally:
        engine.clear_bank()
    wm = WordMatcher(engine=engine)
    for k, name in enumerate(tc.NAMES):
        for what, got in (("bank order A", bank_a[k]), ("bank order B", bank_b[k])):
            assert np.array_equal(got[0], single[k][0]) and np.array_equal(got[1], single[k][1]), (name, what)
        wm.set_reference(recs[k])
        got = (wm.reference_mfcc_mean, wm.reference_mfcc_std)
        assert np.array_equal(got[0], single[k][0]) and np.array_equal(got[1], single[k][1]), (name, "set_reference")
        wm.set_references([recs[k], recs[(k + 1) % n]])
        got = (wm.reference_mfcc_mean, wm.reference_mfcc_std)
        assert np.array_equal(got[0], single[k][0]) and np.array_equal(got[1], single[k][1]), (name, "set_references")
    wm.set_reference(recs[0])      # (clears the matcher's bank)


@pytest.mark.parametrize("candidate_dtype", ["float64", "float32"])
def test_bank_from_pcm_scores_end_to_end(engine, candidate_dtype):
    """One bank of every recording (words of 1, 3 and the rest) from audio: each per-template
    score against WordMatcherRef, and the best template wherever the reference's two best are
    further apart than a tie."""
    recs = [x for _, x in tc.recordings()]
    cands = list(tc.candidates())
    first = np.concatenate([[0], np.cumsum(BANK_SIZES)])
    ref_all = np.array([tc.oracle_scores(n, candidate_dtype) for n in tc.NAMES])     # [template, candidate]
    bad, worst = [], 0.0
    try:
        engine.bank_from_pcm(_words(recs, BANK_SIZES))
        for w, size in enumerate(BANK_SIZES):
            res, scores = engine.score_bank(cands, word=np.full(len(cands), w, np.int32),
                                            candidate_dtype=candidate_dtype, all_scores=True)
            ref = ref_all[first[w]:first[w] + size].T                                 # [candidate, template of w]
            gap = bc.top2_gap(ref)
            for i in range(len(cands)):
                for j in range(size):
                    if not score_close(scores[i, j], ref[i, j], BAR):
                        bad.append((w, i, tc.NAMES[first[w] + j], float(scores[i, j]), float(ref[i, j])))
                    elif np.isfinite(ref[i, j]):
                        worst = max(worst, abs(scores[i, j] - ref[i, j]))
                if np.all(np.isnan(ref[i])):
                    if res["best_tmpl"][i] != -1:
                        bad.append((w, i, "best_tmpl", int(res["best_tmpl"][i]), -1))
                elif gap[i] > bc.TIE:
                    want = int(first[w] + np.nanargmax(ref[i]))
                    if int(res["best_tmpl"][i]) != want:
                        bad.append((w, i, "best_tmpl", int(res["best_tmpl"][i]), want))
    finally:
        engine.clear_bank()
    print(f"bank {candidate_dtype}: max |score - reference| = {worst:.3g}")
    assert not bad, bad[:10]


@pytest.mark.parametrize("name", ["word_x200", "noise"])
def test_stream_events_read_the_derived_template(name):
    """The ring scorer reads the same template: a reference gate run (distractors_a, one stream)
    with the template derived from a loud word and from steady noise; every event's score
    against WordMatcherRef on the event's own segment."""
    from easywakeword_amd import StreamEngine
    rec = next(r for r in gate_fixture() if r["name"] == "distractors_a")
    gate = rec["gate"]
    pcm = stream_pcm(rec)
    tm, ts = tc.oracle_template(name)
    eng = StreamEngine(1, pre_speech_silence=gate["pre_speech_silence"], speech_duration_min=gate["speech_duration_min"],
                       speech_duration_max=gate["speech_duration_max"], post_speech_silence=gate["post_speech_silence"],
                       buffer_seconds=gate["buffer_seconds"], block=gate["block"])
    try:
        eng.template_from_pcm(tc.recording(name))
        block = gate["block"]
        got = []
        for k in range(0, len(pcm) // block, 16):
            eng.push_many(pcm[k * block:(k + 16) * block].reshape(1, -1))
            for ev in eng.poll():
                if ev["flags"] & 1:
                    continue
                audio = eng.read_segment(0, int(ev["ring_start"]), int(ev["length"]))
                got.append((int(ev["tick"]), sha(audio.astype(np.float64)), float(ev["score"]), bool(ev["match"]), audio))
    finally:
        eng.close()
    assert [(g[0], g[1]) for g in got] == [(e["tick"], e["sha256"]) for e in rec["events"]]
    assert len(got) >= 5
    worst = 0.0
    for tick, _, score, match, audio in got:
        cm, cs = mfcc_ref.extract_mfcc(audio.astype(np.float64))
        ref = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
        assert score_close(score, ref, BAR), (tick, score, ref)
        if abs(ref - tc.THRESHOLD) > BAR:
            assert match == (ref >= tc.THRESHOLD), (tick, score, ref)
        if np.isfinite(ref):
            worst = max(worst, abs(score - ref))
    print(f"stream, template {name}: max |score - reference| = {worst:.3g} over {len(got)} events")
