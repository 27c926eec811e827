"""Template bank, CPU part: the ewk_bank_result binding's layout, the pure layout / validation
function of Engine.set_bank (easywakeword_amd.engine.bank_layout) and the oracle margin of the
GPU test batch (tests/bank_cases.py).  No device is touched."""
import ctypes

import numpy as np
import pytest

import bank_cases
from easywakeword_amd import _lib
from easywakeword_amd.engine import bank_layout


def test_bank_result_layout():
    assert ctypes.sizeof(_lib.EwkBankResult) == 24
    dt = _lib.BANK_RESULT_DTYPE
    assert dt.itemsize == 24
    for name in ("best_score", "hit_mask", "best_tmpl", "match", "rescored", "pad"):
        assert dt.fields[name][1] == getattr(_lib.EwkBankResult, name).offset, name
        assert dt.fields[name][0].itemsize == getattr(_lib.EwkBankResult, name).size, name
    assert [dt.fields[n][1] for n in ("best_score", "hit_mask", "best_tmpl", "match", "rescored", "pad")] == \
        [0, 8, 16, 20, 21, 22]
    assert (_lib.EWK_BANK_MAX_PER_WORD, _lib.EWK_BANK_MAX_TEMPLATES) == (64, 65536)


def test_bank_symbols_are_exported():
    for name in ("ewk_bank_set", "ewk_bank_from_pcm", "ewk_bank_clear", "ewk_bank_info", "ewk_bank_get",
                 "ewk_score_segments_bank", "ewk_score_segments_bank_device"):
        assert name in _lib.EXPORTS


def test_layout_word_first():
    t = (np.zeros(20), np.ones(20))
    word_first, thr = bank_layout([[t], [t] * 3, [t] * 64])
    assert word_first.dtype == np.int32 and word_first.tolist() == [0, 1, 4, 68]
    assert thr is None
    word_first, thr = bank_layout([[t], [t] * 3], thresholds=[75, 80.5])
    assert word_first.tolist() == [0, 1, 4]
    assert thr.dtype == np.float64 and thr.tolist() == [75.0, 80.5]


def test_layout_errors():
    t = (np.zeros(20), np.ones(20))
    with pytest.raises(ValueError, match="a bank needs at least one word"):
        bank_layout([])
    with pytest.raises(ValueError, match="word 1 has no templates"):
        bank_layout([[t], []])
    with pytest.raises(ValueError, match="word 2 has 65 templates; at most 64 per word"):
        bank_layout([[t], [t], [t] * 65])
    bank_layout([[t] * 64] * 1024)                       # exactly 65,536 templates: allowed
    with pytest.raises(ValueError, match="bank has 65537 templates; at most 65536"):
        bank_layout([[t] * 64] * 1024 + [[t]])
    with pytest.raises(ValueError, match="3 thresholds for 2 words"):
        bank_layout([[t], [t]], thresholds=[75.0, 75.0, 75.0])
    with pytest.raises(ValueError, match="threshold is NaN"):
        bank_layout([[t]], thresholds=[float("nan")])


def test_gpu_batch_has_an_unambiguous_argmax():
    """The oracle alone: every segment's best template leads the second best by far more than
    the 2e-4 within which the GPU test (test_gpu_bank.py) would accept either index."""
    gap = bank_cases.check_margin()
    assert gap.shape == (bank_cases.N_SEG,)
    assert float(gap.min()) > 1e-3, float(gap.min())
