"""The float32 scorer matrix's inputs, held to the oracle alone (CPU): the conditions every case must
meet before a kernel is looked at, the staged replay of the oracle against oracle/mfcc_ref.py, and the
mutants -- one small wrong version of each stage -- that the inputs of tests/scorer_matrix.py must
throw out of the GPU test's own bars by a factor of 10.  Each test prints what it measured.

Figures of this recipe (drift = how far the error moves a score; the bar is 1e-4): smallest |std|
32.8 and |mean| 124.0 over the cases of more than 16 frames, worst float32-vs-float64 drift of the
oracle itself 6.6e-6, nearest score 2.6 from the threshold; bin 128 moved to 129: drift 1.6e-2; the
last frame dropped at T = 17: 3.4e-2 ... 1.5; a frame rotated by 32 samples: 6.2e-3 ... 1.1; a pad
read from the filler: 4.3 ... 12.
"""
import numpy as np
import pytest

import scorer_matrix as sm
import template_cases as tc
from oracle import mfcc_ref


def _excess(c, **mut):
    return sm.excess(sm.replay(c.x, **mut), sm.oracle(c), c.T)


def test_case_list():
    cs = sm.cases()
    A, B, C = sm.by_family("A"), sm.by_family("B"), sm.by_family("C")
    assert len(cs) == len(A) + len(B) + len(C) == 257 + 4 * 43 * 3 + 4 + 9
    assert [c.k for c in A] == list(range(257)) and {(c.T, c.rem) for c in A} == {(17, 37)}
    grid = {(c.kind, c.k, c.T, c.rem) for c in B if not c.name.startswith("B_long")}
    want_T = list(range(1, 41)) + [47, 48, 49]
    assert grid == {(kind, k, T, rem) for kind, k in (("tone", 5), ("tone", 128), ("tone", 250), ("click", None))
                    for T in want_T for rem in (0, 1, 159)}
    assert sorted(c.T for c in B if c.name.startswith("B_long")) == [767, 768, 769, 770]
    assert {(c.k, c.amp) for c in C} == {(k, a) for k in (5, 128, 250) for a in (5e-4, 0.5, 15.0)}
    for c in cs:
        assert c.x.dtype == np.float32 and mfcc_ref.n_frames(len(c.x)) == c.T, c.name
        assert len(c.x) == (c.T - 1) * 160 + c.rem
    assert sum(len(c.x) for c in cs) < 3_000_000
    assert all(c.T <= 49 for c in cs if not c.name.startswith("B_long"))


def test_seeded_inputs_are_reproducible():
    np.testing.assert_array_equal(sm.tone_probe(128, 17, 1), sm.case("B_tone128_T17_r1").x)
    np.testing.assert_array_equal(sm.click_probe(9, 159), sm.case("B_click_T9_r159").x)
    assert not np.array_equal(sm.case("A_k5").x, sm.case("C_k5_a0.5").x)      # seeded by the case


def test_tone_probe_puts_its_energy_into_its_bin():
    for c in sm.by_family("A")[::16] + [sm.case("A_k256")]:
        P = mfcc_ref.power_spectrogram(c.x.astype(np.float64))[:, 2:-2].sum(axis=1)   # frames clear of the pads
        assert int(np.argmax(P)) == c.k
        far = np.ones(257, bool)
        far[max(c.k - 2, 0):c.k + 3] = False
        assert P[far].sum() < 0.1 * P.sum(), c.name        # the rest: the gain steps' splatter and the noise


def test_conditions_on_the_inputs():
    """Above 16 frames every case lies where DESIGN.md claims float32 alone meets the bar, the oracle
    pins its statistics to a tenth of the bar, and its decision is not a coin toss."""
    tm, ts = sm.template()
    worst = dict(std=np.inf, mean=np.inf, spread=0.0, margin=np.inf)
    bad = []
    held = [(c.name, c.T, sm.oracle(c), sm.oracle(c, "float32")) for c in sm.cases()]
    # the windows of family D's overlapping layout are segments of their own: held like the cases
    held += [(f"D_window{i}", sm.n_frames(x), sm.stats_of(x), sm.stats_of(x, np.float32))
             for i, x in enumerate(sm.windows(sm.d_overlap_layout()))]
    assert sum(T > sm.SHORT_T for n, T, _, _ in held if n.startswith("D_window")) == 6
    for name, T, o, o32 in held:
        if T <= sm.SHORT_T:
            continue
        mn, sd = sm.norms(o)
        spread = sm.drift(o32, o)
        s = sm.score_of(o)
        worst = dict(std=min(worst["std"], sd), mean=min(worst["mean"], mn), spread=max(worst["spread"], spread),
                     margin=min(worst["margin"], abs(s - sm.THRESHOLD)))
        if not (sd >= sm.MIN_STD and mn >= sm.MIN_MEAN and spread <= sm.SPREAD_CAP and np.isfinite(s)
                and abs(s - sm.THRESHOLD) > 1e-3):
            bad.append((name, mn, sd, spread, s))
    print("over the cases and windows of more than 16 frames:", worst)
    assert not bad, bad
    spread = tc.template_drift(sm.oracle(sm.case("A_k128"), "float32"), sm.oracle(sm.case("A_k128")), tc.candidate_stats())
    assert spread <= sm.SPREAD_CAP


def test_short_cases_by_the_oracle():
    """T = 1: one frame, std exactly 0, a NaN score; 2 <= T <= 16: finite statistics."""
    for c in sm.cases():
        if c.T > sm.SHORT_T:
            continue
        m, s = sm.oracle(c)
        assert np.isfinite(m).all() and np.isfinite(s).all(), c.name
        if c.T == 1:
            assert not s.any() and np.isnan(sm.oracle_score(c)), c.name
        else:
            assert np.linalg.norm(s) > 1.0, c.name


def test_replay_reproduces_the_oracle():
    worst = 0.0
    for c in sm.cases()[::5]:
        for dt in ("float64", "float32"):
            r, o = sm.replay(c.x, np.dtype(dt)), sm.oracle(c, dt)
            np.testing.assert_allclose(r[0], o[0], rtol=0, atol=1e-9)
            np.testing.assert_allclose(r[1], o[1], rtol=0, atol=1e-9)
            if c.T > 1:
                worst = max(worst, sm.drift(r, o))
    print(f"replay vs extract_mfcc: worst drift {worst:.3e}")
    assert worst <= 1e-12


# ---- the mutants ---------------------------------------------------------------------------------
def test_mutant_bin_moved_to_the_next():
    """Every bin's probe catches its power landing one bin up, but for the bins the oracle's
    filterbank leaves without leverage -- and those are zero columns of it, nothing else."""
    A = sm.by_family("A")
    e = [_excess(A[k], **sm.mut_bin_to_next(k)) for k in range(257)]
    missed = [k for k in range(257) if e[k] < sm.CAUGHT]
    zero = sm.zero_weight_bins()
    print(f"bin k -> k + 1: smallest excess of a caught bin {min(x for x in e if x >= sm.CAUGHT):.1f} x the bar, "
          f"k = 128: drift {sm.drift(sm.replay(A[128].x, **sm.mut_bin_to_next(128)), sm.oracle(A[128])):.2e}; "
          f"not caught: {missed} (excess {[e[k] for k in missed]}); zero-weight bins {zero}; "
          f"without leverage {sm.bins_without_leverage()}")
    assert missed == sm.bins_without_leverage()
    # a bin without leverage is a zero column (256); the other zero column, bin 0, has leverage
    # because its power arrives in bin 1, which band 0 weighs
    assert zero == [0, 256] and set(missed) <= set(zero)
    assert missed == [k for k in zero if k == 256 or k + 1 in zero]
    assert all(e[k] == 0.0 or e[k] < 1e-6 for k in missed)


def test_mutant_band_row_shifted():
    """A band's weight row one bin up or down.  The probe at the band's peak bin catches every band
    in at least one direction.  Where the peak lies between two bins (bands 83, 101 and 124; band
    101: weights 0.00838 and 0.00841 at bins 133 and 134) a shift towards the twin changes that
    probe's band value by 0.4 % and moves it 2.0, 3.7 and 3.4 times the bar, not 10; the probe one
    bin over catches it: every band, both directions, by a probe in its support."""
    A = sm.by_family("A")
    pk = sm.band_peak_bins()
    weak, worst_peak, worst_any = [], np.inf, np.inf
    for m in range(128):
        at_peak = [_excess(A[pk[m]], **sm.mut_band_row_shifted(m, by)) for by in (1, -1)]
        best = []
        for i, by in enumerate((1, -1)):
            b = at_peak[i]
            for k in sm.band_support(m):
                if b >= sm.CAUGHT:
                    break
                b = max(b, _excess(A[k], **sm.mut_band_row_shifted(m, by)))
            best.append(b)
        if min(at_peak) < sm.CAUGHT:
            weak.append((m, pk[m], [round(x, 1) for x in at_peak]))
        worst_peak, worst_any = min(worst_peak, max(at_peak)), min(worst_any, min(best))
        assert max(at_peak) >= sm.CAUGHT, (m, at_peak)
        assert min(best) >= sm.CAUGHT, (m, best)
    assert [m for m, _, _ in weak] == [83, 101, 124]
    print(f"row shift: peak probe, better direction >= {worst_peak:.1f} x; any probe of the band, either direction "
          f">= {worst_any:.1f} x; peak probe under 10 x in one direction: {weak}")


def test_mutant_bands_swapped():
    A = sm.by_family("A")
    pk = sm.band_peak_bins()
    e = [_excess(A[pk[m]], **sm.mut_bands_swapped(m)) for m in range(128)]
    print(f"bands m, m ^ 1 swapped: smallest excess {min(e):.1f} x at band {int(np.argmin(e))}")
    assert min(e) >= sm.CAUGHT, [(m, x) for m, x in enumerate(e) if x < sm.CAUGHT]


@pytest.mark.parametrize("name,mut", [("dropped", sm.mut_last_frame_dropped), ("repeats", sm.mut_last_frame_repeats)])
def test_mutant_last_frame(name, mut):
    """At every T of the grid (from 2 on: one frame has no other), in every case of that T."""
    per = {}
    for c in sm.by_family("B"):
        if c.T >= 2:
            per.setdefault(c.T, []).append(_excess(c, **mut()))
    assert sorted(per) == [T for T in sm.B_T if T >= 2] + list(sm.LONG_T)
    t17 = [sm.drift(sm.replay(c.x, **mut()), sm.oracle(c)) for c in sm.by_family("B") if c.T == 17]
    print(f"last frame {name}: smallest excess per T {({T: round(min(v), 1) for T, v in per.items()})}; "
          f"drift at T = 17: {min(t17):.2e} ... {max(t17):.2e}")
    short = {T: min(v) for T, v in per.items() if min(v) < sm.CAUGHT}
    assert not short, short


@pytest.mark.parametrize("by", [32, 160])
def test_mutant_frame_rotated(by):
    """Every frame of the click probes at T = 17 and T = 33 (every slot of a tile, twice)."""
    for name in ("B_click_T17_r1", "B_click_T33_r1"):
        c = sm.case(name)
        e = [_excess(c, **sm.mut_frame_rotated(f, by)) for f in range(c.T)]
        d = [sm.drift(sm.replay(c.x, **sm.mut_frame_rotated(f, by)), sm.oracle(c)) for f in (0, 7, 16)]
        print(f"{name}, a frame rotated by {by}: excess {min(e):.1f} ... {max(e):.1f} x, drift at frames 0, 7, 16: {d}")
        assert min(e) >= sm.CAUGHT, (name, [f for f in range(c.T) if e[f] < sm.CAUGHT])


def test_mutant_frame_rotated_by_one_sample():
    """One sample moves a click by 1/512 of the window: a frame whose clicks sit where the window is
    flat or nearly zero barely changes.  Every slot of a tile is caught by one of the six click
    probes at T = 17 and T = 33."""
    probes = [sm.case(f"B_click_T{T}_r{rem}") for T in (17, 33) for rem in sm.B_REM]
    best = np.zeros(16)
    for c in probes:
        for f in range(c.T):
            best[f % 16] = max(best[f % 16], _excess(c, **sm.mut_frame_rotated(f, 1)))
    print("a frame rotated by 1: best excess per tile slot", np.round(best, 1).tolist())
    assert best.min() >= sm.CAUGHT, best


def test_mutant_first_tile_peak():
    per = {}
    for c in sm.by_family("B"):
        if c.T >= 33:
            per.setdefault(c.T, []).append(_excess(c, **sm.mut_first_tile_peak()))
    n = sum(x >= sm.CAUGHT for v in per.values() for x in v)
    print(f"top_db from the first tile's max: {n} of {sum(len(v) for v in per.values())} cases caught; best per T "
          f"{({T: round(max(v), 1) for T, v in per.items()})}")
    assert sorted(per) == list(range(33, 41)) + [47, 48, 49] + list(sm.LONG_T)
    assert all(max(v) >= sm.CAUGHT for v in per.values()), per


@pytest.mark.parametrize("side", ["left", "right"])
def test_mutant_pad_read_from_the_filler(side):
    buf, offs, lens = sm.d_spaced_layout()
    e = {}
    for c, o, n in zip(sm.d_cases(), offs.tolist(), lens.tolist()):
        st = sm.replay(c.x, **sm.mut_pad_from_buffer(buf, o, n, side))
        e[c.name] = sm.excess(st, sm.oracle(c), c.T)
        if c.T == 17:
            print(f"{c.name}: {side} pad from the filler, drift {sm.drift(st, sm.oracle(c)):.2f}")
    print(f"{side} pad from the filler: smallest excess {min(e.values()):.0f} x")
    assert min(e.values()) >= sm.CAUGHT, e


def test_placement_layouts():
    cs = sm.d_cases()
    assert len(cs) == 24 and {c.T for c in cs} == {1, 2, 9, 17} and {c.kind for c in cs} == {"tone", "click"}
    buf, offs, lens = sm.d_spaced_layout()
    assert {0, 1, 2, 3, 31, 63} <= set((offs % 64).tolist()) and sum(o % 2 for o in offs.tolist()) >= 8
    ends = offs + lens
    assert offs[0] >= sm.D_GAP and (offs[1:] - ends[:-1] >= sm.D_GAP).all() and len(buf) - ends[-1] >= sm.D_GAP
    for c, w in zip(cs, sm.windows((buf, offs, lens))):
        np.testing.assert_array_equal(w, c.x)
    inside = np.zeros(len(buf), bool)
    for o, n in zip(offs.tolist(), lens.tolist()):
        inside[o:o + n] = True
    assert np.abs(buf[~inside]).max() > 0.8 and np.sqrt(np.mean(buf[~inside].astype(np.float64) ** 2)) > 0.6   # loud all around
    buf2, offs2, lens2 = sm.d_overlap_layout()
    assert sorted(lens2.tolist()) == sorted(lens.tolist())
    for i in range(len(offs2) - 1):
        assert offs2[i + 1] == offs2[i] + max(int(lens2[i]) - sm.D_OVERLAP, sm.D_SHORT_STEP)
    wins = sm.windows((buf2, offs2, lens2))
    same = [(i, j) for i in range(24) for j in range(i) if len(wins[i]) == len(wins[j]) and np.array_equal(wins[i], wins[j])]
    assert [(len(wins[i]), len(wins[j])) for i, j in same] == [(0, 0)], same      # only the two empty windows are alike
    for c, w in zip(sorted(sm.d_cases(), key=lambda c: -c.T), wins):              # each keeps the head of its own case
        n = min(len(w), sm.D_SHORT_STEP)
        np.testing.assert_array_equal(w[:n], c.x[:n])
    assert (offs2 + lens2).max() <= len(buf2) and offs2.min() >= 0
    assert sum(int(lens2[i]) >= sm.D_OVERLAP for i in range(len(lens2))) >= 12


def test_batch_position_sample():
    idx = sm.e_sample()
    cs = sm.cases()
    assert len(idx) == len(set(idx)) == sm.E_SAMPLE == 32 and idx == sm.e_sample()
    assert {cs[i].family for i in idx} >= {"A", "B"} and sum(cs[i].T <= 16 for i in idx) >= 3
    assert len(sm.e_pad_segment()) == sm.E_PAD_LEN == 161
    # k_score_f32's grid stops at 256 workgroups of 8 waves: the sample lies past the grid's first claims
    assert sm.E_PAD_N >= 256 * 8 and sm.E_PAD_N + sm.E_SAMPLE <= 2 * 256 * 8      # (and under the longest-first order)
