"""The template-bank matrix on the CPU (tests/bank_matrix.py): the numpy reference against the
oracle, the conditions that make the GPU comparison (tests/test_gpu_bank_matrix.py) unambiguous,
and the proof that the matrix sees every named defect.  No device is touched."""
import os
import re

import numpy as np
import pytest

import bank_matrix as bm
from oracle import mfcc_ref

PARITY_ULPS_F64 = 9


@pytest.fixture(scope="module")
def M():
    return bm.matrix()


def test_geometry_and_batch_sizes():
    assert [bm.geometry(L)[0] for L in bm.SIZES] == [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert bm.batch_sizes(64) == [1, 2, 15, 16, 17, 63, 64, 65, 131]                     # per = 1, run = 16
    assert bm.batch_sizes(5) == [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 131]                # per = 8, run = 16
    assert bm.batch_sizes(1) == [1, 63, 64, 65, 255, 256, 257, 515]                      # per = run = 64
    assert max(bm.batch_sizes(1)) == bm.N_SEG


def test_listing_constants_match_the_source():
    """bank_matrix.listed restates the listing rule with kTinyStd and kRescoreFrames of
    csrc/ewk_score.h (the tiny-mean and NaN-margin constants come from _lib, which
    test_rescore_criteria.py holds to csrc/ewk_mfcc.hip): read the way that test reads its own."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "easywakeword_amd", "csrc", "ewk_score.h")).read()
    std = re.search(r"constexpr double kTinyStd = ([0-9.]+);", src)
    frames = re.search(r"constexpr int kRescoreFrames = ([0-9]+);", src)
    assert std is not None and frames is not None
    assert float(std.group(1)) == bm.KTINY_STD and int(frames.group(1)) == bm.RESCORE_FRAMES


def test_banks_are_what_the_matrix_needs(M):
    assert sorted(M.banks) == sorted(bm.SIZES) and sorted(M.special) == [1, 2, 4, 8, 16, 32, 64]
    for L, b in M.banks.items():
        assert b.max_word == L and 3 <= b.n_words <= 4 and 1 in b.sizes
        assert len(set(b.thr.tolist())) == b.n_words
        if L > 1:
            assert any(f % b.G for f in b.first[1:-1])                   # word_first unaligned
        for w in b.words:
            assert len(set(w)) == len(w)                                 # distinct templates: no tie
    for G, b in M.special.items():
        assert b.G == G and b.max_word == G
        tied = [t for t in b.ties if t]
        assert [t for t in tied if len(t) == 2] == [p for p in bm.TIE_PAIRS if p[1] < G]
        assert (len([t for t in tied if len(t) == 3]) == 1) == (G >= 4)
        for w, t in enumerate(b.ties):
            if t:
                assert len({b.words[w][lane] for lane in t}) == 1 and len(set(b.words[w])) == G - len(t) + 1
        nan_words = [w for w in b.words if bm.NAN_TMPL in w]
        assert any(w[0] == bm.NAN_TMPL for w in nan_words) and any(w[-1] == bm.NAN_TMPL for w in nan_words)
        assert any(set(w) == {bm.NAN_TMPL} for w in nan_words)
    assert M.bit63.sizes == [64, 1, 64]
    lens = np.array([len(s) for s in M.segs])
    short = 1 + lens // 160 <= bm.RESCORE_FRAMES
    assert np.nonzero(short)[0].tolist() == list(bm.SHORT_AT) and lens[~short].min() >= 3200 and lens.max() <= 8000


@pytest.mark.parametrize("cand", ["float64", "float32"])
def test_reference_restates_the_oracle(M, cand):
    """bank_ref against oracle.mfcc_ref.similarity_from_stats over the pool x 200 oracle statistics.

    float32 candidates: bit for bit (0 ulp).  float64 candidates: 9 ulp of the score at the
    worst, 55 % of the scores not equal.  The difference is the order of the 20-term float64
    dots and nothing else: the oracle takes uv and vv from numpy's BLAS ddot, whose vector
    kernel keeps several partial sums, while ewk_score.h (ddot20, ddot20s) and bank_ref add the
    terms in order; 1745 of 4000 such dots differ in the last bits between the two orders, and
    the cosine's cancellation near 1 carries that to a few ulp of the score.  The float32
    self-dots (sdot20 against np.dot of two float32 vectors) are identical, as ewk_score.h says,
    and so is every float32-candidate score."""
    tm, ts = bm.pool()
    tm, ts = tm[:68], ts[:68]
    cm, cs = M.stats[cand][0][:200], M.stats[cand][1][:200]
    got = bm.bank_ref(tm, ts, cm, cs, cand)[0]
    ref = np.array([[float(mfcc_ref.similarity_from_stats(tm[k], ts[k], cm[i], cs[i])) for k in range(68)]
                    for i in range(200)])
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    u = bm.ulps(got, ref, np.dtype(cand).type)
    print(f"{cand}: worst {u.max():.0f} ulp, {np.mean(u > 0):.1%} of the scores differ")
    assert u.max() <= (PARITY_ULPS_F64 if cand == "float64" else 0)
    # every defect in the reference's arithmetic moves the scores far beyond that
    for mutant in ("std_mean_swapped", "vv_neighbour"):
        bad = bm.bank_ref(tm, ts, cm, cs, cand, mutant=mutant)[0]
        with np.errstate(invalid="ignore"):
            moved = (np.isnan(bad) != np.isnan(got)) | (np.abs(bad - got) > 1e-3)
        assert moved.mean() > 0.5, mutant


def test_summarise():
    nan = np.nan
    rows = np.array([[1.0, 3.0, 3.0, nan], [nan, nan, nan, nan], [nan, 2.0, 1.0, 2.0], [5.0, 5.0, 5.0, 5.0]])
    s = bm.summarise(rows, [3.0, 0.0, 2.5, 5.0])
    assert s["hit_mask"].dtype == np.uint64 and s["hit_mask"].tolist() == [6, 0, 0, 15]
    assert s["match"].tolist() == [True, False, False, True]
    assert s["best_tmpl"].tolist() == [1, -1, 1, 0]
    assert np.array_equal(s["best_score"], [3.0, nan, 2.0, 5.0], equal_nan=True)
    assert bm.summarise(rows, [3.0, 0.0, 2.5, 5.0], "tie_high")["best_tmpl"].tolist() == [2, -1, 3, 3]
    wide = np.full((1, 64), nan)
    wide[0, 63] = 1.0
    assert bm.summarise(wide, [1.0])["hit_mask"].tolist() == [1 << 63]


def test_conditions_on_the_inputs(M):
    """With the oracle's statistics, over every batch of the matrix and both candidate dtypes:
    no segment's two best scores within its word are closer than 1e-3 (the lanes of a tie word
    that hold one template count once) and no score lies within 1e-3 of its word's threshold.
    Zero cases are excused; the event path's three segments are held to the same."""
    worst_gap, worst_thr = np.inf, np.inf
    for b in M.all_banks():
        for kind, n in M.cases(b):
            word = b.pattern(kind, n)
            for cand, sc in M.scores.items():
                gap, dist = M.conditions(b, sc[:n], word)
                assert gap >= bm.MARGIN and dist >= bm.MARGIN, (b.name, kind, n, cand, gap, dist)
                worst_gap, worst_thr = min(worst_gap, gap), min(worst_thr, dist)
    for L in bm.EVENT_SIZES:
        b = M.banks[L]
        for w in range(b.n_words):
            gap, dist = M.conditions(b, M.event_scores["float64"], np.full(len(M.events), w))
            assert gap >= bm.MARGIN and dist >= bm.MARGIN, (L, w, gap, dist)
    print(f"smallest top-2 gap {worst_gap:.3g}, smallest threshold distance {worst_thr:.3g}, "
          f"{M.n_candidates_dropped} candidate segments passed over")
    assert len(M.events) == 3


def test_special_cases_occur(M):
    """Every tie word has a segment whose best template is the tied one (best_tmpl: the lowest
    of its lanes), every NaN word gives NaN at its lane and the all-NaN word an empty result;
    the hit-bit-63 words give bit 63 alone and every bit but 63; both hit values occur in
    every plain word."""
    sc = M.scores["float64"]
    for G, b in M.special.items():
        word = b.pattern("cycle", b.n_max())
        rows, s = b.expect(sc[:len(word)], word)
        for w, t in enumerate(b.ties):
            mine = np.nonzero(word == w)[0]
            if t:
                local = s["best_tmpl"][mine] - b.first[w]
                assert (local == t[0]).any(), (G, w, t)
                assert not np.isin(local, t[1:]).any()
                assert np.array_equal(rows[mine][:, t[0]], rows[mine][:, t[-1]])
            lanes = [j for j, k in enumerate(b.words[w]) if k == bm.NAN_TMPL]
            assert np.isnan(rows[mine][:, lanes]).all()
            if len(lanes) == b.sizes[w] and lanes:
                assert (s["best_tmpl"][mine] == -1).all() and not s["match"][mine].any()
    b = M.bit63
    for w, want in ((0, 1 << 63), (2, (1 << 63) - 1)):
        _, s = b.expect(sc[:bm.BIT63_N], b.pattern(w, bm.BIT63_N))
        assert int(s["hit_mask"][M.bit63_seg]) == want
    for b in M.banks.values():
        word = b.pattern("cycle", b.n_max())
        _, s = b.expect(sc[:len(word)], word)
        for w in range(b.n_words):
            hits = s["hit_mask"][word == w]
            assert (hits != 0).any() and (hits != (1 << b.sizes[w]) - 1).any(), (b.name, w)


def _differs(a, b, bar=1e-9):
    (ra, sa), (rb, sb) = a, b
    with np.errstate(invalid="ignore"):
        if (np.isnan(ra) != np.isnan(rb)).any() or np.nanmax(np.abs(ra - rb), initial=0.0) > bar:
            return True
    return any(not np.array_equal(sa[k], sb[k], equal_nan=True) for k in ("hit_mask", "match", "best_tmpl", "best_score"))


@pytest.mark.parametrize("mutant", bm.MUTANTS)
def test_every_mutant_is_seen_in_every_family(M, mutant):
    """Each named defect changes a quantity the GPU test asserts (a score beyond its bar -- here
    the bar's cap, 1e-9 -- or NaN placement, hit_mask, match, best_score, best_tmpl) in some
    batch of every G family.  A word of one template cannot tie: tie_high has no G = 1 case."""
    arith = mutant in ("std_mean_swapped", "vv_neighbour")
    good = M.scores["float64"]
    bad = M.mutant_scores(mutant) if arith else good
    for G in (1, 2, 4, 8, 16, 32, 64):
        if mutant == "tie_high" and G == 1:
            continue
        seen = False
        for b in M.family(G):
            for kind, n in M.cases(b):
                word = b.pattern(kind, n)
                if _differs(b.expect(good[:n], word), b.expect(bad[:n], word, None if arith else mutant)):
                    seen = True
                    break
            if seen:
                break
        assert seen, (mutant, G)
