"""Input-rate resampler, host side (CPU): the filter design of ewk_resample_design against
scipy's firwin, its error paths, the ABI bookkeeping, and the streaming definition (block by
block, with history and delay) against the whole-signal audio.resample."""
import ctypes as C
from math import gcd

import numpy as np
import pytest

from resample_ref import design_params, stream_resample_ref

RATES = (48000, 44100, 8000, 32000, 22050, 96000)
OUT = 16000


def design(in_rate, out_rate=OUT, cap=None):
    from easywakeword_amd import _lib
    lib = _lib.load()
    n, up, down = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = lib.ewk_resample_design(in_rate, out_rate, None, 0, C.byref(n), C.byref(up), C.byref(down))
    if n.value < 0:
        return rc, None, n.value, up.value, down.value
    taps = np.full(n.value if cap is None else cap, np.nan, np.float64)
    rc = lib.ewk_resample_design(in_rate, out_rate, _lib.dptr(taps), len(taps), C.byref(n), C.byref(up),
                                 C.byref(down))
    return rc, taps, n.value, up.value, down.value


@pytest.mark.parametrize("rate", RATES)
def test_design_matches_scipy_firwin(rate):
    from scipy.signal import firwin
    rc, taps, n, up, down = design(rate)
    assert rc == 0
    g = gcd(rate, OUT)
    assert (up, down) == (OUT // g, rate // g)
    half = 10 * max(up, down)
    assert n == 2 * half + 1
    ref = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    err = float(np.max(np.abs(taps - ref)))
    print(f"{rate} Hz: up {up} down {down} taps {n}, max |taps - firwin| = {err:.3e}")
    assert np.max(np.abs(ref)) < 1.01   # taps of magnitude ~1: 1e-13 absolute is ~450 ulp of the largest
    assert err <= 1e-13


def test_design_error_paths():
    from easywakeword_amd import _lib
    lib = _lib.load()
    n = C.c_int32(-1)
    for bad in ((0, OUT), (-48000, OUT), (48000, 0), (48000, -1)):
        assert lib.ewk_resample_design(bad[0], bad[1], None, 0, C.byref(n), None, None) == _lib.EWK_EINVAL
    assert lib.ewk_last_error()
    # a buffer that is too small: EWK_EINVAL, the size still reported, nothing written
    rc, taps, n_taps, up, down = design(48000, cap=60)
    assert rc == _lib.EWK_EINVAL and n_taps == 61 and (up, down) == (1, 3)
    assert np.isnan(taps).all()
    rc, taps, n_taps, _, _ = design(48000, cap=61)
    assert rc == 0 and np.isfinite(taps).all()


def test_new_symbols_are_exported():
    from easywakeword_amd import _lib
    lib = _lib.load()
    for name in ("ewk_resample_design", "ewk_resample", "ewk_set_input_rate", "ewk_input_rate_info"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert lib.ewk_abi_version() == 4


@pytest.mark.parametrize("rate", RATES)
def test_streaming_definition_equals_delayed_whole_signal_resample(rate):
    """Block by block, each tick from its own in_block samples and the H = J + 1 samples before
    them (sequential float64 sums in ascending input order, one rounding to float32), the 16 kHz
    stream is concat(zeros(delay), audio.resample(x)) bit for bit: pins delay and look-ahead."""
    from easywakeword_amd.audio import resample
    _, taps, _, up, down = design(rate)
    p = design_params(rate)
    assert (p["up"], p["down"]) == (up, down)
    block, ticks = 1600, 2
    in_block = block * down // up
    rng = np.random.default_rng(rate)
    x = (0.5 * rng.standard_normal(ticks * in_block)).astype(np.float32)
    got = stream_resample_ref(x, rate, block, taps=taps)
    whole = resample(x, rate, OUT)
    want = np.concatenate([np.zeros(p["delay"], np.float32), whole])[: ticks * block]
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (rate, bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.all(got[: p["delay"]] == 0)
