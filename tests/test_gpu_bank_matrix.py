"""The template bank (csrc/ewk_bank.hip) on every launch geometry, against the numpy reference
of tests/bank_matrix.py: every group size G in {1, 2, 4, 8, 16, 32, 64}, batch sizes on every
step, run and workgroup edge, four word patterns, ties, NaN templates, hit bit 63, both passes
(k_bank<float> on Engine(rescore_margin=0), k_bank<double> on Engine(rescore_margin=1e9)), both
candidate dtypes, the device variant and the event path (k_bank_events).

The reference is given the engine's own statistics (Engine.score without a template for the
float32 mean / std, Engine.score_f64 for the fp64 ones), so the comparison measures the bank
pass alone.  Asserted for every batch:

  scores        within the bar of bank_ref on the float32 statistics where rescored == 0 and on
                the fp64 statistics where rescored == 1; NaN exactly where the reference has it;
                NaN past the word's size
  exact         hit_mask, match, best_score and best_tmpl equal summarise() of the kernel's own
                score row bit for bit; hit_mask, match and best_tmpl also equal summarise() of
                the reference (test_bank_matrix.py: no two best scores within 1e-3, no score
                within 1e-3 of a threshold, so nothing is excused)
  rescored      the listing rule evaluated on the reference (bank_matrix.listed)
  prefixes      the results of the first n segments are the first n results of the whole batch

The score bar is measured, not chosen (fixture `bars`): everything before the pow is IEEE-exact
and restated in the same order, so the bar is 4 x the worst distance between the device's power
and the reference's as seen through code this file does not test -- Engine.score_f64 and
Engine.score(candidate_dtype="float32") with a single pool template against bank_ref on the
statistics the same call returned -- in ulps of the score, at least 4 ulp, at most 1e-9 (the
project's bank-vs-single bound).  Measured on an MI355X (profiles/bank_matrix.json):

  float64 candidates  pow distance 1 ulp, bar 4 ulp of the score (5.7e-14 at 90); the kernel's
                      worst error 1 ulp at every G, in both passes
  float32 candidates  distance 0: the power is pow15f (ewk_score.h), p * sqrt(p) in double
                      rounded to float32, IEEE operations that bank_ref restates bit for bit,
                      and the single-template float32 finish takes the same.  4 float32 ulp is
                      3.1e-5 at 90, so the bar is the cap, 1e-9 -- less than one float32 ulp of
                      any score above 0.01: the reference's bits.  The kernel's worst error 0
                      at every G.  (With the device's powf in that place the matrix found one
                      float32 ulp against libm's powf for 2,342 of 11,518 scores, at every G
                      and in the single-template scorer alike: DESIGN.md.)
"""
import json

import numpy as np
import pytest

import bank_matrix as bm

pytestmark = pytest.mark.gpu

CAP = 1e-9


@pytest.fixture(scope="module")
def M():
    return bm.matrix()


@pytest.fixture(scope="module")
def engines():
    from easywakeword_amd import Engine
    e = {"f32": Engine(rescore_margin=0.0), "f64": Engine(rescore_margin=1e9)}
    yield e
    for x in e.values():
        x.close()


@pytest.fixture(scope="module")
def crit():
    from easywakeword_amd._lib import NAN_MARGIN_A, NAN_MARGIN_B, RESCORE_TINY_MEAN
    return dict(tiny_mean=RESCORE_TINY_MEAN, nan_a=NAN_MARGIN_A, nan_b=NAN_MARGIN_B)


@pytest.fixture(scope="module")
def ref(M, engines):
    """{cand: {"f32" | "f64": (score, percent, mean2, std2)}}: bank_ref of the engine's own float32
    and fp64 statistics of the N_SEG segments against the whole pool, computed once."""
    m32, s32, _, _ = engines["f32"].score(M.segs, require_template=False, candidate_dtype="float64")
    m64, s64, _ = engines["f32"].score_f64(M.segs)
    assert m32.dtype == np.float32 and m64.dtype == np.float64
    tm, ts = bm.pool()
    return {c: {"f32": bm.bank_ref(tm, ts, m32, s32, c), "f64": bm.bank_ref(tm, ts, m64, s64, c)}
            for c in ("float64", "float32")}


@pytest.fixture(scope="module")
def bars(M, crit):
    """The measured pow distance and the bars: {cand: (worst ulps, bar in ulps)}."""
    from easywakeword_amd import Engine
    tm, ts = bm.pool()
    lens = np.array([len(s) for s in M.segs])
    worst = {"float64": 0.0, "float32": 0.0}
    e = Engine(rescore_margin=0.0)
    try:
        for k in (0, 9, 21, 34, 47, 60):
            e.set_template(tm[k], ts[k])
            m, s, sc = e.score_f64(M.segs)
            want = bm.bank_ref(tm[k:k + 1], ts[k:k + 1], m, s, "float64")[0][:, 0]
            assert np.array_equal(np.isnan(sc), np.isnan(want)), k
            worst["float64"] = max(worst["float64"], float(bm.ulps(sc, want).max()))
            m, s, sc, _ = e.score(M.segs, candidate_dtype="float32")
            want, _, mean2, std2 = bm.bank_ref(tm[k:k + 1], ts[k:k + 1], m, s, "float32")
            # (margin 0: the float32 pass decided every segment its listing rule leaves alone)
            own = ~((1 + lens // 160 <= bm.RESCORE_FRAMES) | ((std2 > 0) & (std2 < bm.KTINY_STD ** 2)) |
                    (mean2 < crit["tiny_mean"] ** 2))
            assert own.sum() > bm.N_SEG // 2
            assert np.array_equal(np.isnan(sc[own]), np.isnan(want[own, 0])), k
            worst["float32"] = max(worst["float32"], float(bm.ulps(sc[own], want[own, 0], np.float32).max()))
    finally:
        e.close()
    out = {c: (w, max(4.0, 4.0 * w)) for c, w in worst.items()}
    print("measured pow distance and bars (ulps):", out)
    return out


def _tol(want, cand, bars, cap=CAP):
    """The score bar per element: bars[cand] ulps of the reference score (float32 ulps for
    float32 candidates), at most `cap`."""
    t = np.float32 if cand == "float32" else np.float64
    with np.errstate(invalid="ignore"):
        return np.minimum(bars[cand][1] * np.spacing(np.abs(want).astype(t)).astype(np.float64), cap)


def _check(b, word, lengths, res, scores, ref, cand, margin, crit, bars, cap=CAP):
    """Every assertion on one batch (the module's docstring)."""
    n = len(word)
    assert scores.shape == (n, b.max_word) and res.shape == (n,)
    tabs = ref[cand]
    rows32, thr = b.rows(tabs["f32"][0][:n], word)
    rows64, _ = b.rows(tabs["f64"][0][:n], word)
    rescored = res["rescored"].astype(bool)
    want = np.where(rescored[:, None], rows64, rows32)
    # scores: NaN placement (past the word's size included) and the bar
    assert np.array_equal(np.isnan(scores), np.isnan(want)), (b.name, n, np.argwhere(np.isnan(scores) != np.isnan(want))[:5])
    with np.errstate(invalid="ignore"):
        err = np.abs(scores - want)
        over = err > _tol(want, cand, bars, cap)
    assert not over.any(), (b.name, n, cand, [(i, j, scores[i, j], want[i, j]) for i, j in np.argwhere(over)[:5]])
    # the summary against the kernel's own row, bit for bit
    first = b.first[np.asarray(word, np.int64)]
    own = bm.summarise(scores, thr)
    own_tmpl = np.where(own["best_tmpl"] >= 0, own["best_tmpl"] + first, -1)
    assert np.array_equal(res["hit_mask"], own["hit_mask"]), (b.name, n)
    assert np.array_equal(res["match"].astype(bool), own["match"]), (b.name, n)
    assert np.array_equal(res["best_score"], own["best_score"], equal_nan=True), (b.name, n)
    assert np.array_equal(res["best_tmpl"], own_tmpl), (b.name, n, np.nonzero(res["best_tmpl"] != own_tmpl)[0][:5])
    assert not res["pad"].any()
    # ... and against the reference: decisions and argmax exact, the best score within the bar
    exp = bm.summarise(want, thr)
    exp_tmpl = np.where(exp["best_tmpl"] >= 0, exp["best_tmpl"] + first, -1)
    assert np.array_equal(res["hit_mask"], exp["hit_mask"]), (b.name, n, np.nonzero(res["hit_mask"] != exp["hit_mask"])[0][:5])
    assert np.array_equal(res["match"].astype(bool), exp["match"]), (b.name, n)
    assert np.array_equal(res["best_tmpl"], exp_tmpl), (b.name, n, np.nonzero(res["best_tmpl"] != exp_tmpl)[0][:5])
    assert np.array_equal(np.isnan(res["best_score"]), np.isnan(exp["best_score"]))
    with np.errstate(invalid="ignore"):
        assert not (np.abs(res["best_score"] - exp["best_score"]) > _tol(exp["best_score"], cand, bars, cap)).any()
    # rescored: the listing rule on the float32 statistics
    prc, _ = b.rows(tabs["f32"][1][:n], word)
    lst = bm.listed(b, word, lengths, rows32, prc, tabs["f32"][2][:n], tabs["f32"][3][:n], margin, cand, **crit)
    assert np.array_equal(rescored, lst), (b.name, n, np.nonzero(rescored != lst)[0][:5])
    return rescored


def _run(engine, b, M, kind, n, cand):
    word = b.pattern(kind, n)
    res, scores = engine.score_bank(M.segs[:n], word=word, candidate_dtype=cand, all_scores=True)
    return word, res, scores


MARGINS = {"f32": 0.0, "f64": 1e9}


@pytest.mark.parametrize("which", ["f32", "f64"])
@pytest.mark.parametrize("L", bm.SIZES)
def test_batch_matrix(M, engines, ref, bars, crit, L, which):
    """Every batch size and word pattern of the bank with largest word L, float64 candidates:
    all of _check, and every n-prefix equal to the first n results of the whole batch."""
    b, e = M.banks[L], engines[which]
    e.set_bank(b.templates(), thresholds=b.thr)
    lens = np.array([len(s) for s in M.segs])
    sizes = bm.batch_sizes(L)
    for kind in bm.PATTERNS:
        _, full_res, full_scores = _run(e, b, M, kind, sizes[-1], "float64")
        for n in sizes:
            word, res, scores = _run(e, b, M, kind, n, "float64")
            assert res.tobytes() == full_res[:n].tobytes(), (L, kind, n)
            assert np.array_equal(scores, full_scores[:n], equal_nan=True), (L, kind, n)
            rescored = _check(b, word, lens[:n], res, scores, ref, "float64", MARGINS[which], crit, bars)
            short = [i for i in bm.SHORT_AT if i < n]
            assert rescored[short].all()
            if which == "f64":
                assert rescored.all()                                  # (every word has a finite score)


@pytest.mark.parametrize("which", ["f32", "f64"])
@pytest.mark.parametrize("L", bm.SIZES)
def test_float32_candidates(M, engines, ref, bars, crit, L, which):
    """Float32 candidates at 4 run + 1 segments, the word cycling: the same assertions, the
    reference in float32 arithmetic (the fp64 statistics rounded to float32 where re-scored).
    The bar is the cap, 1e-9: less than one float32 ulp, so the scores are the reference's bits."""
    b, e = M.banks[L], engines[which]
    e.set_bank(b.templates(), thresholds=b.thr)
    n = 4 * b.run + 1
    lens = np.array([len(s) for s in M.segs[:n]])
    word, res, scores = _run(e, b, M, "cycle", n, "float32")
    _check(b, word, lens, res, scores, ref, "float32", MARGINS[which], crit, bars)



@pytest.mark.parametrize("which", ["f32", "f64"])
@pytest.mark.parametrize("G", [1, 2, 4, 8, 16, 32, 64])
def test_ties_and_nan_templates(M, engines, ref, bars, crit, G, which):
    """The special bank of a G: one template at two lanes that differ in each shuffle distance
    and at three lanes (best_tmpl: the lowest of them, exactly), the zero-std template at lane 0,
    at the last lane, at the lane that would have been best and at every lane of a word."""
    b, e = M.special[G], engines[which]
    e.set_bank(b.templates(), thresholds=b.thr)
    lens = np.array([len(s) for s in M.segs])
    for kind, n in M.cases(b):
        word, res, scores = _run(e, b, M, kind, n, "float64")
        _check(b, word, lens[:n], res, scores, ref, "float64", MARGINS[which], crit, bars)
        if kind != "cycle" or n != b.n_max():
            continue
        for w, t in enumerate(b.ties):
            mine = word == w
            local = res["best_tmpl"][mine] - b.first[w]
            if t:
                assert (local == t[0]).any() and not np.isin(local, t[1:]).any(), (G, w, t)
            if set(b.words[w]) == {bm.NAN_TMPL}:
                assert mine.any() and (res["best_tmpl"][mine] == -1).all() and not res["hit_mask"][mine].any()
                assert np.isnan(res["best_score"][mine]).all() and np.isnan(scores[mine]).all()


@pytest.mark.parametrize("which", ["f32", "f64"])
def test_hit_bit_63(M, engines, ref, bars, crit, which):
    """A 64-template word whose threshold leaves template 63 alone above it: hit_mask is bit 63;
    and alone below it: every bit but 63."""
    b, e = M.bit63, engines[which]
    e.set_bank(b.templates(), thresholds=b.thr)
    lens = np.array([len(s) for s in M.segs])
    for (w, n), want in zip(M.cases(b), (1 << 63, (1 << 63) - 1)):
        word, res, scores = _run(e, b, M, w, n, "float64")
        _check(b, word, lens[:n], res, scores, ref, "float64", MARGINS[which], crit, bars)
        assert int(res["hit_mask"][M.bit63_seg]) == want, (w, hex(int(res["hit_mask"][M.bit63_seg])))


# ---------------------------------------------------------------- the device variant
SENTINEL = -777.0


def _device_run(engine, segs, word, stride):
    """score_bank_device on a sentinel-filled score buffer one row longer than the batch:
    (results[n], scores[n + 1, stride])."""
    import torch
    from easywakeword_amd import _lib
    dev = torch.device("cuda", engine.gpu)
    n = len(segs)
    lengths = np.array([len(s) for s in segs], np.int32)
    offsets = np.zeros(n, np.int64)
    offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
    ext = torch.cuda.ExternalStream(engine.stream_handle(), device=dev)
    with torch.cuda.stream(ext):
        pcm = torch.from_numpy(np.concatenate(segs).astype(np.float32)).to(dev)
        off, ln = torch.from_numpy(offsets).to(dev), torch.from_numpy(lengths).to(dev)
        wd = torch.from_numpy(np.ascontiguousarray(word, np.int32)).to(dev)
        out = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
        sc = torch.full((n + 1, stride), SENTINEL, dtype=torch.float64, device=dev)
        engine.score_bank_device(pcm.data_ptr(), off.data_ptr(), ln.data_ptr(), n, wd.data_ptr(), out.data_ptr(),
                                 sc.data_ptr(), stride)
        engine.sync()
        out_h, sc_h = out.cpu().numpy(), sc.cpu().numpy()
    ext.synchronize()
    return out_h.view(_lib.BANK_RESULT_DTYPE), sc_h


@pytest.mark.parametrize("which", ["f32", "f64"])
@pytest.mark.parametrize("L", bm.SIZES)
def test_device_variant_dead_groups(M, engines, L, which):
    """Word indices -1, n_words and 1 << 30 over every 5th item of the largest batch: those rows
    come back empty, every other row bit-identical to the run without them (a dead group must
    not disturb its neighbours' cached words), and both equal the host call."""
    b, e = M.banks[L], engines[which]
    e.set_bank(b.templates(), thresholds=b.thr)
    n = b.n_max()
    word = b.pattern("random", n)
    segs = M.segs[:n]
    host_res, host_scores = e.score_bank(segs, word=word, candidate_dtype="float64", all_scores=True)
    res, sc = _device_run(e, segs, word, L)
    assert res.tobytes() == host_res.tobytes() and np.array_equal(sc[:n], host_scores, equal_nan=True)
    assert (sc[n] == SENTINEL).all()
    dead = word.copy()
    at = np.arange(0, n, 5)
    dead[at] = np.resize(np.array([-1, b.n_words, 1 << 30], np.int32), len(at))
    res2, sc2 = _device_run(e, segs, dead, L)
    live = np.ones(n, bool)
    live[at] = False
    assert res2[live].tobytes() == res[live].tobytes()
    assert np.array_equal(sc2[:n][live], sc[:n][live], equal_nan=True) and (sc2[n] == SENTINEL).all()
    d = res2[at]
    assert np.isnan(d["best_score"]).all() and (d["best_tmpl"] == -1).all() and not d["hit_mask"].any()
    assert not d["match"].any() and not d["rescored"].any() and np.isnan(sc2[at]).all()


@pytest.mark.parametrize("L", [5, 17])
def test_device_variant_strides(M, engines, L):
    """out_scores strides {largest word, G, G + 1, 64}: the same scores at every stride, NaN at
    and past the word's size up to the stride, nothing written past the last row."""
    b, e = M.banks[L], engines["f64"]
    e.set_bank(b.templates(), thresholds=b.thr)
    n = 4 * b.run + 1
    word = b.pattern("cycle", n)
    segs = M.segs[:n]
    host_res, host_scores = e.score_bank(segs, word=word, candidate_dtype="float64", all_scores=True)
    size = np.array(b.sizes)[word]
    for stride in (L, b.G, b.G + 1, 64):
        res, sc = _device_run(e, segs, word, stride)
        assert res.tobytes() == host_res.tobytes(), stride
        assert np.array_equal(sc[:n, :L], host_scores, equal_nan=True), stride
        past = np.arange(stride)[None] >= size[:, None]
        assert np.isnan(sc[:n][past]).all() and not np.isnan(sc[:n][~past]).any(), stride
        assert (sc[n] == SENTINEL).all(), stride


# ---------------------------------------------------------------- the event path
@pytest.mark.parametrize("L", bm.EVENT_SIZES)
def test_event_path(M, L):
    """k_bank_events on 2 per + 1 streams that gate in lockstep (one stream's audio in every
    stream, stream_word cycling): a tick's pass holds two full steps and a partial one.  Every
    event goes through fp64 (rescore_margin = 1e9); its score against bank_ref on the oracle's
    statistics of the samples read back from the ring at 1e-9 (test_stream_bank_rescore_all's
    bar), match and the best template exact."""
    from easywakeword_amd import StreamEngine, _lib
    from oracle import mfcc_ref
    b = M.banks[L]
    ns = 2 * b.per + 1
    pcm, _ = bm.event_stream()
    assert len(pcm) % 1600 == 0
    data = np.ascontiguousarray(np.tile(pcm, (ns, 1)))
    sw = (np.arange(ns) % b.n_words).astype(np.int32)
    tm, ts = bm.pool()
    eng = StreamEngine(ns, rescore_margin=1e9, **bm.GATE)
    events, audio = [], []
    try:
        eng.set_bank(b.templates(), thresholds=b.thr)
        eng.set_stream_bank(sw)
        for c in range(0, data.shape[1], 8 * 1600):
            eng.push_many(data[:, c:c + 8 * 1600])
            ev = eng.poll()
            events.append(ev)
            audio.extend(eng.read_segment(int(x["stream"]), int(x["ring_start"]), int(x["length"])) for x in ev)
    finally:
        eng.close()
    ev = np.concatenate(events)
    assert np.bincount(ev["stream"], minlength=ns).min() >= 3
    assert np.unique(ev["tick"], return_counts=True)[1].max() > b.per
    known = {a.astype(np.float32).tobytes(): k for k, a in enumerate(M.events)}
    rows_of = {}
    for x, a in zip(ev, audio):
        flags = int(x["flags"])
        assert not flags & _lib.EWK_EV_SKIPPED and flags & _lib.EWK_EV_BANK and flags & _lib.EWK_EV_RESCORED, x
        key = np.asarray(a, np.float32).tobytes()
        assert key in known                                    # the gate oracle's events (conditions: CPU test)
        if key not in rows_of:
            cm, cs = mfcc_ref.extract_mfcc(np.asarray(a).astype(np.float64))
            rows_of[key] = bm.bank_ref(tm, ts, cm[None], cs[None], "float64")[0]
        w = int(sw[int(x["stream"])])
        rows, s = b.expect(rows_of[key], np.array([w]))
        assert abs(float(x["score"]) - float(s["best_score"][0])) <= 1e-9, (x, s)
        assert bool(x["match"]) == bool(s["match"][0]), (x, s)
        assert int(_lib.event_best_template(flags)) == int(s["best_tmpl"][0]) - int(b.first[w]), (x, s)
    assert len(rows_of) == len(M.events)


def test_worst_error_per_group_size(M, engines, ref, bars):
    """The bank pass's worst score error per G, over the largest cycling batch of every plain
    bank on both engines and in both candidate dtypes, computed here (no other test's state):
    float32 candidates exactly 0, float64 candidates within the bar.  Prints the line that
    profiles/bank_matrix.json records."""
    worst = {c: {} for c in ("float64", "float32")}
    for e in engines.values():
        for L in bm.SIZES:
            b = M.banks[L]
            e.set_bank(b.templates(), thresholds=b.thr)
            for cand in worst:
                word, res, scores = _run(e, b, M, "cycle", b.n_max(), cand)
                rows32, _ = b.rows(ref[cand]["f32"][0][:len(word)], word)
                rows64, _ = b.rows(ref[cand]["f64"][0][:len(word)], word)
                want = np.where(res["rescored"].astype(bool)[:, None], rows64, rows32)
                u = float(bm.ulps(scores, want, np.float32 if cand == "float32" else np.float64).max())
                worst[cand][str(b.G)] = max(worst[cand].get(str(b.G), 0.0), u)
    out = dict(pow_distance_ulps={c: v[0] for c, v in bars.items()}, bar_ulps={c: v[1] for c, v in bars.items()},
               cap=CAP, kernel_worst_ulps_per_G=worst)
    print("BANK_MATRIX_REPORT " + json.dumps(out))
    assert sorted(worst["float64"], key=int) == ["1", "2", "4", "8", "16", "32", "64"] == sorted(worst["float32"], key=int)
    assert max(worst["float32"].values()) == 0.0, worst
    assert max(worst["float64"].values()) <= bars["float64"][1], worst
