"""The re-score matrix's inputs, held to the oracle and the numpy replay (CPU): every input
reaches the path of ewk_rescore.h it is meant for, and the replay of the kernel's chunk algebra
(scripts/f64_chunk_model.py, theta_s = theta + 1e-5 dB, W = kRsWindow) is within 1e-11 of
oracle/mfcc_ref.py on every one of them -- the reference alone is 100x inside the 1e-9 bar the
GPU test (tests/test_gpu_rescore_matrix.py) holds the engine to."""
import numpy as np
import pytest

import rescore_matrix as rm

NAMES = [c.name for c in rm.cases()]
CASES = {c.name: c for c in rm.cases()}
GUARD = 1e-11


@pytest.mark.parametrize("name", NAMES)
def test_input_reaches_its_path(name):
    c = CASES[name]
    assert c.x.dtype == np.float32
    c.check(c)


@pytest.mark.parametrize("name", [c.name for c in rm.cases() if c.oracle])
def test_replay_is_within_the_guard_of_the_oracle(name):
    c = CASES[name]
    cm, cs, s = rm.oracle(c)
    assert np.isfinite(cm).all() and np.isfinite(cs).all()
    dm, dsd, ds = rm.replay_error(c)
    print(f"{name}: T={c.T} |dmean|/scale={dm:.2e} |dstd|/scale={dsd:.2e} |dscore|={ds:.2e}")
    assert dm <= GUARD and dsd <= GUARD and ds <= GUARD
    m, sd, _, _ = rm.replay(c)
    s2 = float(rm.mfcc_ref.similarity_from_stats(*rm.template(), m, sd))
    assert np.isnan(s2) == np.isnan(s)


@pytest.mark.parametrize("k", range(3))
def test_short_cases_reach_the_pool_past_a_nan_float32_score(k):
    c = rm.short_cases()[k]
    c.check(c)
    if c.oracle:
        dm, dsd, _ = rm.replay_error(c)
        assert dm <= GUARD and dsd <= GUARD
        m, sd, _, _ = rm.replay(c)
        s2 = float(rm.mfcc_ref.similarity_from_stats(*rm.huge_template(), m, sd))
        assert abs(s2 - rm.huge_score(c)) <= GUARD


def test_case_table():
    fam = {f: [c for c in rm.cases() if c.family == f] for f in "abcdef"}
    assert [len(c.x) for c in fam["a"]] == list(rm.GRID_L) and len(fam["a"]) == 20
    assert sorted({c.T for c in fam["a"]}) == [1, 2, 3, 7, 8, 9, 15, 16, 17, 18]
    assert {c.last_n for c in fam["a"]} == {1, 2, 3, 7, 8}
    assert [len(c.x) for c in fam["b"]] == [160 * k + 159 for k in rm.DUMMY_K]
    assert {c.last_n for c in fam["b"]} == {1, 3, 5, 7}
    assert sorted({c.n_chunks for c in fam["c"]}) == [64, 65, 129]
    assert len(fam["c"]) == 4 + len(rm.FLAG_DELTAS) and len(fam["d"]) == 6 and len(fam["e"]) == 1 and len(fam["f"]) == 2
    assert max(len(c.x) for c in rm.cases()) == rm.LONG and len(rm.cases()) <= 45
    # the only comparisons that are not with the oracle: all zeros and the non-finite inputs
    assert [c.name for c in rm.cases() if not c.oracle] == ["d_zeros_L1600", "d_zeros_L20000", "f_nan", "f_inf"]
    assert len(rm.shaped()) == 13


def test_nan_oracle_scores_are_exactly_the_listed_ones():
    assert tuple(c.name for c in rm.cases() if c.oracle and np.isnan(rm.oracle(c)[2])) == rm.NAN_SCORE
    for c in rm.cases():
        if c.name in rm.NAN_SCORE and c.family != "e":
            assert c.T == 1 and not rm.oracle(c)[1].any()      # one frame: an exact zero std


def test_no_oracle_score_sits_on_the_threshold():
    """A decision of the GPU test can differ from the oracle's only through a wrong score."""
    s = np.array([rm.oracle(c)[2] for c in rm.cases() if c.oracle and c.name not in rm.NAN_SCORE])
    assert np.isfinite(s).all() and (np.abs(s - 75.0) > 1e-3).all()


def test_ring_segments_straddle_the_compact_ring():
    ev = rm.ring_oracle_events()
    scored = [e for s in ev for e in s if not e.skipped]
    assert len(scored) >= 15
    assert sum(rm.straddles(e.tick, e.n_request, e.length) for e in scored) >= 3
    assert max(e.length for e in scored) < rm.COMPACT_RING
