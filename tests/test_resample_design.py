"""Input-rate resampler, host side (CPU): the filter design of ewk_resample_design against
scipy's firwin, its error paths, the ABI bookkeeping, and the streaming definition (block by
block, with history and delay) against the whole-signal audio.resample."""
import ctypes as C
from math import gcd

import numpy as np
import pytest

from resample_ref import design_params, launch_geometry, one_shot_lengths, stream_resample_ref

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


# the streaming definition also at the rates whose phase offset c0 = half - delay * down is
# negative (upsampling, `down` not dividing 10 * up), at 176.4 kHz (J = 221) and at rates whose
# tick is shorter than the history (1 kHz with block 320: 20 samples against H = 22)
STREAM_RATES = RATES + (24000, 12000, 12800, 9600, 176400, 1000, 2000)
NEGATIVE_C0 = {12000: -2, 12800: -2, 9600: -1}


def _check_streaming_definition(rate, block):
    from easywakeword_amd.audio import resample
    _, taps, _, up, down = design(rate)
    p = design_params(rate)
    assert (p["up"], p["down"]) == (up, down)
    c0 = p["half"] - p["delay"] * down
    assert -down < c0 <= 0
    if rate in NEGATIVE_C0:
        assert c0 == NEGATIVE_C0[rate] < 0
    ticks = 13 if rate in (1000, 2000) else 2
    in_block = block * down // up
    if (rate, block) == (1000, 320):
        assert in_block < p["H"]              # a tick's history reaches into the tick before the last
    rng = np.random.default_rng(rate)
    x = (0.5 * rng.standard_normal(ticks * in_block)).astype(np.float32)
    got = stream_resample_ref(x, rate, block, taps=taps)
    whole = resample(x, rate, OUT)
    want = np.concatenate([np.zeros(p["delay"], np.float32), whole])[: ticks * block]
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (rate, bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.all(got[: p["delay"]] == 0)


@pytest.mark.parametrize("rate", RATES)
def test_streaming_definition_equals_delayed_whole_signal_resample(rate):
    """Block by block, each tick from its own in_block samples and the H = J + 1 samples before
    them (sequential float64 sums in ascending input order, one rounding to float32), the 16 kHz
    stream is concat(zeros(delay), audio.resample(x)) bit for bit: pins delay and look-ahead."""
    _check_streaming_definition(rate, 1600)


@pytest.mark.parametrize("rate,block", [(r, b) for b in (1600, 320) for r in STREAM_RATES
                                        if not (b == 1600 and r in RATES)])
def test_streaming_definition_at_more_rates_and_blocks(rate, block):
    """The same at 320-sample ticks and at the further rates of STREAM_RATES (13 ticks at 1 and 2 kHz)."""
    _check_streaming_definition(rate, block)


def test_launch_geometry_table():
    """The workgroup size and staged span of each rate the GPU tests run (resample_threads,
    resample_span), and the rates on the far side of the limits."""
    table = {22050: (320, 1791), 12800: (255, 837), 176400: (240, 10794), 176000: (256, 11474),
             11025: (640, 1785), 16016: (1000, 4024), 96000: (256, 6259), 48000: (256, 3130), 8000: (256, 533)}
    for rate, (threads, span) in table.items():
        g = launch_geometry(rate)
        assert (g["threads"], g["span"], g["accepted"]) == (threads, span, True), (rate, g)
        assert g["tile"] == 4 * threads and threads % design_params(rate)["up"] == 0
        lengths = one_shot_lengths(rate)
        outs = [n_out for _, n_out in lengths]
        assert outs == sorted(set(outs)) and all(n_in >= 1 for n_in, _ in lengths)
        assert g["tile"] in outs and outs[0] <= 2 and outs[-1] >= 2 * g["tile"] + 3
        assert any(o < g["tile"] for o in outs[1:]) and any(g["tile"] < o < 2 * g["tile"] for o in outs)
        if design_params(rate)["down"] >= design_params(rate)["up"]:      # downsampling reaches every n_out
            assert outs == [1, g["tile"] - 1, g["tile"], g["tile"] + 1, 2 * g["tile"] + 3]
    g = launch_geometry(192000)
    assert (g["span"], g["accepted"]) == (12517, False)
    assert design_params(16001)["up"] == 16000 and not launch_geometry(16001)["accepted"]
    assert design_params(176400)["J"] == 221 and design_params(96000)["J"] == 121
