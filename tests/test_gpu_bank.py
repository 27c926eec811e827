"""Template bank on the GPU (ewk_score_segments_bank*, csrc/ewk_bank.hip): every segment scored
against all the templates of one word, vs the CPU oracle and vs the single-template scorer.

Bar: scores within 1e-4 of the oracle (NaN == NaN), identical decisions.  The batch and its
oracle scores are built once (tests/bank_cases.py) and shared."""
import os

import numpy as np
import pytest

import bank_cases as bc
import synth
from golden_io import GOLD, gate_fixture, score_close, stream_pcm

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4
WAV = os.path.join(GOLD, "reference_word.wav")


@pytest.fixture(scope="module")
def engine():
    from easywakeword_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def case(engine):
    """The three-word bank on `engine`, the 96-segment batch, its bank results (float64
    candidates, all scores) and the oracle's scores against the engine's own templates."""
    engine.bank_from_pcm(bc.bank_audio(), thresholds=bc.THRESHOLDS)
    assert engine.bank_info() == (3, 68)
    segs, word = bc.segments()
    tpl = [engine.bank_template(k) for k in range(68)]
    tm, ts = np.array([m for m, _ in tpl]), np.array([s for _, s in tpl])
    res, scores = engine.score_bank(segs, word=word, candidate_dtype="float64", all_scores=True)
    ref = bc.oracle_scores(segs, word, tm, ts)
    return dict(segs=segs, word=word, tm=tm, ts=ts, res=res.copy(), scores=scores.copy(), ref=ref)


def _restore(engine):
    engine.bank_from_pcm(bc.bank_audio(), thresholds=bc.THRESHOLDS)


def _check_against(res, scores, ref, word, thresholds, sizes=bc.SIZES):
    """Every (segment, template) score and hit bit, and every segment's summary, vs `ref`."""
    first = np.concatenate([[0], np.cumsum(sizes)])
    bad, excused, worst = [], 0, 0.0
    for i in range(len(ref)):
        w = int(word[i])
        size, thr = sizes[w], thresholds[w]
        assert np.all(np.isnan(scores[i, size:])), i            # past the word's size
        for j in range(size):
            if not score_close(scores[i, j], ref[i, j], SCORE_TOL):
                bad.append((i, j, float(scores[i, j]), float(ref[i, j])))
            elif np.isfinite(ref[i, j]):
                worst = max(worst, abs(scores[i, j] - ref[i, j]))
            if bool((int(res["hit_mask"][i]) >> j) & 1) != bool(ref[i, j] >= thr):
                bad.append((i, j, "hit", float(scores[i, j]), float(ref[i, j]), thr))
        assert int(res["hit_mask"][i]) >> size == 0, i
        assert bool(res["match"][i]) == bool(np.any(ref[i, :size] >= thr)), i
        if np.all(np.isnan(ref[i, :size])):
            assert np.isnan(res["best_score"][i]) and res["best_tmpl"][i] == -1, i
            continue
        assert score_close(res["best_score"][i], np.nanmax(ref[i, :size]), SCORE_TOL), i
        want = int(first[w] + np.nanargmax(ref[i, :size]))
        if int(res["best_tmpl"][i]) != want:
            top = np.sort(ref[i, :size][np.isfinite(ref[i, :size])])
            near_tie = top.size >= 2 and top[-1] - top[-2] <= bc.TIE
            got = int(res["best_tmpl"][i]) - int(first[w])
            if near_tie and 0 <= got < size and top[-1] - ref[i, got] <= bc.TIE:
                excused += 1
            else:
                bad.append((i, "best_tmpl", int(res["best_tmpl"][i]), want))
    print(f"max |score - oracle| = {worst:.3g}, {excused} near-tie argmax excused, "
          f"{int(res['rescored'].sum())} of {len(ref)} segments re-scored in fp64")
    assert not bad, bad[:10]
    return excused


def test_one_word_one_template_equals_the_single_template_scorer(engine):
    """1 word x 1 template against Engine.score with that template and threshold: identical
    decisions; scores within 1e-9 (the two paths order their dot products differently) and NaN
    in the same places; a segment that went through fp64 gets the identical score."""
    word = synth.load_word()
    segs = synth.ragged_segments(515, 64, 160, 48000)
    segs[5::10] = synth.ragged_segments(516, 6, 160, 2559)     # <= 16 frames: fp64 on both paths
    engine.template_from_pcm(word)
    engine.set_threshold(90.0)
    try:
        engine.set_bank([[engine.get_template()]])            # thresholds None: the engine's
        _, _, score, match = engine.score(segs, candidate_dtype="float64")
        res = engine.score_bank(segs, candidate_dtype="float64")
    finally:
        engine.set_threshold(75.0)
        _restore(engine)
    assert np.array_equal(res["match"].astype(bool), match)
    assert np.array_equal(res["hit_mask"], match.astype(np.uint64))
    assert np.array_equal(np.isnan(res["best_score"]), np.isnan(score))
    ok = ~np.isnan(score)
    print("max |bank - single| =", float(np.max(np.abs(res["best_score"][ok] - score[ok]))),
          "re-scored", int(res["rescored"].sum()))
    assert float(np.max(np.abs(res["best_score"][ok] - score[ok]))) <= 1e-9
    assert np.array_equal(res["best_tmpl"][ok], np.zeros(int(ok.sum()), np.int32))
    rs = ok & (res["rescored"] == 1)
    assert rs.sum() >= 6                                       # (the <= 16-frame segments at least)
    assert np.array_equal(res["best_score"][rs], score[rs])   # both listed: the same fp64 score


def test_lane_patterns_vs_oracle(case):
    """Words of 1, 3 and 64 templates (word_first = [0, 1, 4, 68]), float64 candidates."""
    excused = _check_against(case["res"], case["scores"], case["ref"], case["word"], bc.THRESHOLDS)
    assert excused < 0.01 * len(case["ref"])
    short = np.array([1 + len(s) // 160 <= 16 for s in case["segs"]])
    assert short.sum() >= 8 and np.all(case["res"]["rescored"][short] == 1)
    assert 0 < case["res"]["rescored"].sum() < len(short)     # both passes decide segments


@pytest.mark.parametrize("sizes", [(2, 1, 4, 3), (5, 8, 1)])
def test_small_words_share_a_wave_vs_oracle(engine, case, sizes):
    """A bank whose largest word has 4 (8) templates: a segment takes 4 (8) lanes and a wave
    scores 16 (8) segments per step.  40 segments (a partial last step, three waves), the word
    index cycling, against the oracle like the 64-lane case."""
    audio = [a for a in bc.bank_audio()[2][10:40:2]]           # 15 distinct clips: tones, speech-like
    words, k = [], 0
    for sz in sizes:
        words.append(audio[k:k + sz])
        k += sz
    thr = [84.0 + w for w in range(len(sizes))]
    segs = case["segs"][:40]
    word = (np.arange(40) % len(sizes)).astype(np.int32)
    try:
        engine.bank_from_pcm(words, thresholds=thr)
        K = sum(sizes)
        tpl = [engine.bank_template(i) for i in range(K)]
        res, scores = engine.score_bank(segs, word=word, candidate_dtype="float64", all_scores=True)
    finally:
        _restore(engine)
    assert scores.shape == (40, max(sizes))
    tm, ts = np.array([m for m, _ in tpl]), np.array([s for _, s in tpl])
    ref = bc.oracle_scores(segs, word, tm, ts, sizes=sizes)[:, :max(sizes)]
    assert _check_against(res, scores, ref, word, thr, sizes=sizes) == 0
    assert res["rescored"].sum() >= 3                           # (segments 3, 14, 25, 36: <= 16 frames)


def test_float32_candidates_vs_oracle(engine, case):
    idx = np.arange(16) * 5                                    # 16 segments over all three words
    segs = [case["segs"][i] for i in idx if np.any(case["segs"][i])]   # (float32 silence: an artefact)
    word = np.array([case["word"][i] for i in idx if np.any(case["segs"][i])], np.int32)
    assert len(segs) == 16 and set(word.tolist()) == {0, 1, 2}
    res, scores = engine.score_bank(segs, word=word, candidate_dtype="float32", all_scores=True)
    ref = bc.oracle_scores(segs, word, case["tm"], case["ts"], dtype=np.float32)
    _check_against(res, scores, ref, word, bc.THRESHOLDS)


def test_threshold_on_the_fp64_score_decides_exactly(engine):
    """A word threshold placed exactly on the fp64 score of (segment, template 1): bit 1 is set
    and the segment was re-scored; one ulp above, bit 1 is clear."""
    audio = [synth.load_word(), synth.speech_like(0.9), synth.tone(660)]
    segs = synth.ragged_segments(99, 8, 8000, 30000)
    try:
        engine.bank_from_pcm([audio])
        tpl = [engine.bank_template(k) for k in range(3)]
        engine.set_template(*tpl[1])
        _, _, s64 = engine.score_f64(segs)
        assert np.isfinite(s64).sum() >= 6
        for i, x in enumerate(segs):
            if np.isnan(s64[i]):
                continue
            engine.set_bank([tpl], thresholds=[float(s64[i])])
            r = engine.score_bank([x], candidate_dtype="float64")
            assert (int(r["hit_mask"][0]) >> 1) & 1 == 1 and r["rescored"][0] == 1, (i, s64[i])
            engine.set_bank([tpl], thresholds=[float(np.nextafter(s64[i], np.inf))])
            r = engine.score_bank([x], candidate_dtype="float64")
            assert (int(r["hit_mask"][0]) >> 1) & 1 == 0 and r["rescored"][0] == 1, (i, s64[i])
    finally:
        _restore(engine)


def test_nan_rules(engine, case):
    zero = np.zeros(16000, np.float32)
    res, scores = engine.score_bank([zero] * 3, word=[0, 1, 2], candidate_dtype="float64", all_scores=True)
    assert np.all(np.isnan(scores))
    assert np.all(np.isnan(res["best_score"])) and np.all(res["best_tmpl"] == -1)
    assert not res["match"].any() and not res["hit_mask"].any()
    word = synth.load_word()
    seg = case["segs"][0]
    try:
        # word 1 mixes a template made from silence (NaN against anything) with a real one
        engine.bank_from_pcm([[synth.tone(440)], [zero, word]], thresholds=[50.0, 50.0])
        res, scores = engine.score_bank([seg], word=[1], candidate_dtype="float64", all_scores=True)
    finally:
        _restore(engine)
    assert np.isnan(scores[0, 0]) and np.isfinite(scores[0, 1])
    assert res["best_tmpl"][0] == 2 and res["best_score"][0] == scores[0, 1]
    assert res["hit_mask"][0] == (2 if scores[0, 1] >= 50.0 else 0)


def test_listing_order_does_not_matter(engine, case):
    """The fp64 list is appended to in whatever order the waves finish: the same batch twice,
    and once reversed, must give bit-identical results per segment (rescored flags included)."""
    segs, word = case["segs"], case["word"]
    r1, s1 = engine.score_bank(segs, word=word, candidate_dtype="float64", all_scores=True)
    r2, s2 = engine.score_bank(segs[::-1], word=word[::-1].copy(), candidate_dtype="float64", all_scores=True)
    for r, s in ((r1, s1), (r2[::-1], s2[::-1])):
        assert np.ascontiguousarray(r).tobytes() == case["res"].tobytes()
        np.testing.assert_array_equal(s, case["scores"])       # (NaN == NaN)


def test_device_variant_is_bit_identical(engine, case):
    import torch
    dev = torch.device("cuda", engine.gpu)
    segs, word = case["segs"], case["word"]
    n = len(segs)
    lengths = np.array([len(s) for s in segs], np.int32)
    offsets = np.zeros(n, np.int64)
    offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
    stride = 64
    ext = torch.cuda.ExternalStream(engine.stream_handle(), device=dev)
    with torch.cuda.stream(ext):
        pcm = torch.from_numpy(np.concatenate(segs).astype(np.float32)).to(dev)
        off, ln = torch.from_numpy(offsets).to(dev), torch.from_numpy(lengths).to(dev)
        wd = torch.from_numpy(word.copy()).to(dev)
        out = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
        sc = torch.zeros((n, stride), dtype=torch.float64, device=dev)
        engine.score_bank_device(pcm.data_ptr(), off.data_ptr(), ln.data_ptr(), n, wd.data_ptr(), out.data_ptr(),
                                 sc.data_ptr(), stride)
        out_h, sc_h = out.cpu().numpy(), sc.cpu().numpy()
    ext.synchronize()
    from easywakeword_amd import _lib
    assert out_h.tobytes() == case["res"].tobytes()
    assert out_h.view(_lib.BANK_RESULT_DTYPE).shape == (n,)
    np.testing.assert_array_equal(sc_h, case["scores"])
    # an index outside the bank cannot be checked from the host: an empty result, no fault
    with torch.cuda.stream(ext):
        wd2 = torch.from_numpy(np.array([3, -1, 1 << 30, 0], np.int32)).to(dev)
        out2 = torch.zeros(4 * 24, dtype=torch.uint8, device=dev)
        sc2 = torch.zeros((4, stride), dtype=torch.float64, device=dev)
        engine.score_bank_device(pcm.data_ptr(), off.data_ptr(), ln.data_ptr(), 4, wd2.data_ptr(), out2.data_ptr(),
                                 sc2.data_ptr(), stride)
        r2 = out2.cpu().numpy().view(_lib.BANK_RESULT_DTYPE)
        s2 = sc2.cpu().numpy()
    ext.synchronize()
    assert np.all(r2["best_tmpl"][:3] == -1) and np.all(np.isnan(r2["best_score"][:3]))
    assert not r2["match"][:3].any() and not r2["hit_mask"][:3].any() and np.all(np.isnan(s2[:3]))
    assert r2[3:].tobytes() == case["res"][3:4].tobytes()


def test_errors(engine, case):
    from easywakeword_amd import Engine
    segs = case["segs"][:2]
    with pytest.raises(ValueError, match=r"word index 3 of segment 1 is outside \[0, 3\)"):
        engine.score_bank(segs, word=[0, 3])
    with pytest.raises(ValueError, match="outside"):
        engine.score_bank(segs, word=[-1, 0])
    e = Engine()
    try:
        assert e.bank_info() == (0, 0)
        with pytest.raises(ValueError, match="No reference word set"):
            e.score_bank(segs)
        # the C ABI checks its own arguments before anything is launched
        import ctypes as C
        from easywakeword_amd import _lib
        lib, tpl = _lib.load(), np.ones((4, 20), np.float32)
        for first in ([0, 2, 2, 4], [0, 3, 2, 4], [1, 2, 3, 4]):      # empty word, not monotonic, first != 0
            wf = np.array(first, np.int32)
            assert lib.ewk_bank_set(e.handle, 3, _lib.i32ptr(wf), _lib.fptr(tpl), _lib.fptr(tpl), None) == \
                _lib.EWK_EINVAL
        big = np.ones((65, 20), np.float32)
        assert lib.ewk_bank_set(e.handle, 1, _lib.i32ptr(np.array([0, 65], np.int32)), _lib.fptr(big),
                                _lib.fptr(big), None) == _lib.EWK_EINVAL
        assert e.bank_info() == (0, 0)
        e.bank_from_pcm([[synth.load_word(), synth.tone(440), synth.tone(880)]])
        m0, s0 = e.bank_template(1)
        assert m0.shape == (20,) and np.all(np.isfinite(m0)) and np.all(s0 >= 0)
        with pytest.raises(ValueError, match="template index out of range"):
            e.bank_template(3)
        pcm, off, ln = np.zeros(3200, np.float32), np.zeros(1, np.int64), np.array([3200], np.int32)
        out, sc = np.zeros(1, _lib.BANK_RESULT_DTYPE), np.zeros(2)
        assert lib.ewk_score_segments_bank(e.handle, _lib.fptr(pcm), 3200, _lib.i64ptr(off), _lib.i32ptr(ln), 1, None,
                                           out.ctypes.data_as(C.POINTER(_lib.EwkBankResult)), _lib.dptr(sc), 2,
                                           0) == _lib.EWK_EINVAL     # stride 2 < the 3-template word
        e.clear_bank()
        with pytest.raises(ValueError, match="No reference word set"):
            e.score_bank(segs)
    finally:
        e.close()


def test_word_matcher_references():
    from easywakeword_amd import WordMatcher
    a440, a880 = synth.tone(440), synth.tone(880)
    m = WordMatcher()
    probe = synth.speech_like()
    singles = []
    for a in (a880, a440):
        m.set_reference(a)
        singles.append(m.calculate_similarity(probe))
    single_880_vs_440 = m.matches(a880)                        # (reference: a440)
    m.set_references([a880, a440])
    assert m.matches(synth.tone(440)) == (True, 100.0)
    assert abs(m.calculate_similarity(probe) - max(singles)) <= 1e-9
    mt, sc = m.matches_batch([a440, a880, probe], threshold=99.0)
    assert sc[0] == 100.0 and sc[1] == 100.0 and sc[2] == m.calculate_similarity(probe)
    assert mt.tolist() == [True, True, bool(sc[2] >= 99.0)]
    m.set_reference(a440)                                      # back to one template
    assert m.engine.bank_info() == (0, 0)
    assert m.matches(a880) == single_880_vs_440
    assert m.matches(a880)[1] < 100.0


def _gate_kw(rec):
    g = rec["gate"]
    return dict(pre_speech_silence=g["pre_speech_silence"], speech_duration_min=g["speech_duration_min"],
                speech_duration_max=g["speech_duration_max"], post_speech_silence=g["post_speech_silence"],
                buffer_seconds=g["buffer_seconds"])


def test_wakeword_with_several_reference_files(tmp_path):
    """WakeWord(textword, [unrelated.wav, reference_word.wav]) returns at the tick of the
    single-reference detector; with the unrelated reference alone it times out."""
    from easywakeword_amd import WakeWord, WavSource, write_wav
    rec = next(r for r in gate_fixture() if r["name"] == "config1_word_x8")
    capture = tmp_path / "capture.wav"
    write_wav(str(capture), stream_pcm(rec))
    rng = np.random.Generator(np.random.PCG64(6))
    unrelated = tmp_path / "unrelated.wav"                     # loud high-passed noise: the oracle scores
    write_wav(str(unrelated), (np.diff(rng.standard_normal(12001)) * 0.5).astype(np.float32))   # the gated word ~42
    kw = _gate_kw(rec)
    one = WakeWord("hello", WAV, timeout=60, source=WavSource(str(capture)), **kw)
    assert one.waitforit() == "hello"
    tick = one._sound_buffer.engine.state(0)["tick"]
    one.stop()
    many = WakeWord("hello", [str(unrelated), WAV], timeout=60, source=WavSource(str(capture)), **kw)
    assert many.waitforit() == "hello"
    assert many._sound_buffer.engine.state(0)["tick"] == tick
    assert many._matcher.engine.bank_info() == (1, 2)
    many.stop()
    none = WakeWord("hello", str(unrelated), timeout=5, source=WavSource(str(capture)), **kw)
    with pytest.raises(TimeoutError):
        none.waitforit()
    assert none._sound_buffer.engine.state(0)["tick"] > tick  # the word went by unmatched
    none.stop()
