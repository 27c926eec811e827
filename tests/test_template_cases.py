"""The inputs of the template-parity tests, checked with the CPU oracle alone (no GPU): the
reference itself must pin every recording's template to a tenth of the 1e-4 bar, the set must
hold the recordings templates go wrong on, and no template may put more than two candidates on
the decision threshold."""
import numpy as np
import pytest

import template_cases as tc
from oracle import mfcc_ref


def test_the_listed_recordings_exist():
    recs = tc.recordings()
    assert [n for n, _ in recs] == tc.NAMES and len(set(tc.NAMES)) == len(tc.NAMES)
    assert 16 <= len(recs) <= 26
    for _, x in recs:
        assert x.dtype == np.float32 and x.ndim == 1 and np.all(np.isfinite(x))
    assert max(len(x) for _, x in recs) == 200000        # one past the 1024-frame tile record
    assert len(tc.candidates()) <= 60 and max(len(c) for c in tc.candidates()) <= 60000


@pytest.mark.parametrize("name", tc.NAMES)
def test_the_reference_pins_the_template(name):
    d = tc.describe(name)
    print(f"{name}: |mean| {d['mean_norm']:.3f} |std| {d['std_norm']:.3f} frames {d['frames']} "
          f"reference_spread {d['spread']:.2e}")
    assert d["spread"] <= tc.SPREAD_CAP


def test_the_reference_pins_the_edge_length_statistics():
    for x in tc.edge_recordings():
        assert mfcc_ref.n_frames(len(x)) > 16
        assert tc.reference_spread(x) <= tc.SPREAD_CAP, len(x)


def test_degenerate_clips_are_refused_by_the_rule():
    """A nearly constant clip's float32 template is rounding noise (the spread is past the cap by
    orders of magnitude): the selection must skip it, however close its norms are."""
    import synth
    x = synth.fuzz_segments(3, 60, synth.load_word())[52]
    assert tc.reference_spread(x) > 10 * tc.SPREAD_CAP
    assert tc._pick([x], lambda c: 0.0, 1) == []


def test_the_set_holds_the_hard_recordings():
    d = [tc.describe(n) for n in tc.NAMES]
    assert sum(x["mean_norm"] < 32.0 for x in d) >= 2     # vanishing mean
    assert sum(x["std_norm"] < 22.0 for x in d) >= 2      # stationary
    assert sum(x["frames"] <= 16 for x in d) >= 2         # too short for the float32 statistics
    assert sum(x["frames"] > 1024 for x in d) >= 1


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_few_candidates_sit_on_the_threshold(dtype):
    for name in tc.NAMES:
        s = tc.oracle_scores(name, dtype)
        assert int(np.sum(np.abs(s - tc.THRESHOLD) <= tc.BAR)) <= 2, name
        assert np.isfinite(s).sum() >= 5, name


def test_no_candidate_is_constant():
    for c in tc.candidates():
        assert np.ptp(mfcc_ref.log_mel(c.astype(np.float64))) != 0.0


def test_template_drift_is_in_score_units():
    """The yardstick on a known error: 1e-3 per coefficient (half of what rtol 1e-4 / atol 2e-3
    lets through) moves the word's scores by more than the bar; no error moves nothing."""
    t = tc.f32_template(tc.recording("word"))
    rng = np.random.default_rng(2)
    p = (t[0] + rng.normal(0, 1e-3, 20).astype(np.float32), t[1] + rng.normal(0, 1e-3, 20).astype(np.float32))
    np.testing.assert_allclose(p[0], t[0], rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(p[1], t[1], rtol=1e-4, atol=2e-3)
    assert tc.template_drift(t, p, tc.candidate_stats()) > tc.BAR
    assert tc.template_drift(t, t, tc.candidate_stats()) == 0.0
