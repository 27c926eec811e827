"""Subset pushes with the stream bank on, and ewk_stream_bank_assign.

The bank, thresholds and the 12 PCM16-exact streams of test_gpu_stream_bank.py (26 events against
three words of 1, 3 and 64 templates; that file holds them to the oracle).  Bar here: the events
of an engine pushed by the seeded subset schedule equal the lockstep engine's in every field --
score bits, match, EWK_EV_BANK and the best template (EWK_EV_BEST) included -- and a word
assigned through assign_stream_words scores exactly as the same word given to set_stream_bank.
"""
import numpy as np
import pytest

import bank_cases as bc
import lifecycle_util as lu
from test_gpu_stream_bank import GATE, N, THRESHOLDS, make_streams

pytestmark = pytest.mark.gpu

BLOCK = 1600


def _engine(word="none"):
    from easywakeword_amd import StreamEngine
    eng = StreamEngine(N, **GATE)
    eng.bank_from_pcm(bc.bank_audio(), thresholds=THRESHOLDS)
    if not isinstance(word, str):
        eng.set_stream_bank(word)
    return eng


def _lockstep(eng, data, t0=0, t1=None):
    t1 = data.shape[1] // BLOCK if t1 is None else t1
    got = []
    for c in range(t0, t1, 8):
        eng.push_many(data[:, c * BLOCK:min(c + 8, t1) * BLOCK])
        got.append(eng.poll())
    return np.concatenate(got)


@pytest.fixture(scope="module")
def case():
    data, _, word = make_streams()
    eng = _engine(word)
    ev = _lockstep(eng, data)
    eng.close()
    assert len(ev) > 20
    return dict(data=data, word=word, ev=ev)


def test_subset_schedule_equals_lockstep(case):
    from easywakeword_amd import _lib
    data, n_ticks = case["data"], case["data"].shape[1] // BLOCK
    eng = _engine(case["word"])
    got = []
    for sub, nt, first in lu.schedule(N, n_ticks, 31):
        eng.push_streams(sub, lu.rows_of(data, sub, first, nt, BLOCK))
        got.append(eng.poll())
    ev = np.concatenate(got)
    eng.close()
    assert lu.assert_events_equal(case["ev"], ev, N) > 20
    scored = ev[(ev["flags"] & _lib.EWK_EV_SKIPPED) == 0]
    assert len(scored) > 20 and ((scored["flags"] & _lib.EWK_EV_BANK) != 0).all()
    assert len(set(_lib.event_best_template(scored["flags"]).tolist())) > 1


def test_assign_before_the_first_push_equals_set_stream_bank(case):
    """Enabled with word 0 for every stream, then every stream assigned its word (in two calls,
    shuffled): the per-stream array is created, all zeros, and filled."""
    eng = _engine(None)
    order = np.random.default_rng(5).permutation(N).astype(np.int32)
    eng.assign_stream_words(order[:5], case["word"][order[:5]])
    eng.assign_stream_words(order[5:], case["word"][order[5:]])
    ev = _lockstep(eng, case["data"])
    eng.close()
    assert lu.assert_events_equal(case["ev"], ev, N) > 20


def test_mid_run_assignment(case):
    """One stream changes its word between two pushes (no poll, no wait in between): its events
    from the pushes before equal the lockstep run with the old word, those after the run with the
    new word; every other stream is the old run's."""
    data, word, old = case["data"], case["word"], case["ev"]
    counts = np.bincount(old["stream"], minlength=N)
    s = int(np.argmax(counts))
    ticks = np.sort(old["tick"][old["stream"] == s])
    assert len(ticks) >= 2
    cut = int(ticks[len(ticks) // 2 - 1]) // 8 * 8 + 8          # a push boundary behind its first events
    assert ticks[0] <= cut < ticks[-1]
    word2 = word.copy()
    word2[s] = (word[s] + 1) % 3
    ref = _engine(word2)
    new = _lockstep(ref, data)
    ref.close()
    o, n = old[old["stream"] == s], new[new["stream"] == s]
    assert not np.array_equal(o["score"].view(np.int64), n["score"].view(np.int64))    # the word matters

    eng = _engine(word)
    before = _lockstep(eng, data, 0, cut)
    eng.assign_stream_words([s], [word2[s]])
    after = _lockstep(eng, data, cut)
    eng.close()
    want = np.concatenate([old[(old["stream"] != s) | (old["tick"] <= cut)], new[(new["stream"] == s) & (new["tick"] > cut)]])
    assert (before["tick"] <= cut).all() and (after["tick"] > cut).all()
    assert lu.assert_events_equal(want, np.concatenate([before, after]), N) > 20


def test_assign_refusals(case):
    eng = _engine()                                   # a bank, but the stream bank is off
    with pytest.raises(ValueError, match="stream bank is off"):
        eng.assign_stream_words([0], [0])
    eng.set_stream_bank(case["word"])
    for streams, words in (([0, 0], [1, 1]), ([N], [0]), ([-1], [0]), ([1], [3]), ([1], [-1]), ([], []), ([1, 2], [0])):
        with pytest.raises(ValueError):
            eng.assign_stream_words(streams, words)
    ev = _lockstep(eng, case["data"])                 # the refused calls changed no word
    eng.close()
    assert lu.assert_events_equal(case["ev"], ev, N) > 20
