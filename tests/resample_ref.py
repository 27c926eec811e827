"""Host restatement of the input-rate resampler's streaming definition (include/ewk.h,
ewk_set_input_rate) and of the kernel's launch geometry, shared by tests/test_resample_design.py
and the resampler's GPU tests.

The 16 kHz stream is the whole-signal resample y (easywakeword_amd.audio.resample) delayed by
`delay` samples.  Output n uses c = (n - delay) * down + half, i = floor(c / up), p = c mod up:
sum over j = J - 1 .. 0 of h[p + j * up] * x[i - j] -- ascending input index, the order of
scipy's upfirdn -- in float64, rounded once to float32."""
from math import gcd

import numpy as np

OUT = 16000


def design_params(rate, out=OUT):
    g = gcd(int(rate), int(out))
    up, down = out // g, rate // g
    half = 10 * max(up, down)
    J = 2 * half // up + 1
    return dict(up=up, down=down, half=half, J=J, H=J + 1, delay=-(-half // down))


Q, MAX_THREADS, MAX_SPAN = 4, 1024, 12288      # kRsQ, kRsMaxThreads, kRsMaxSpan (ewk_internal.h)


def launch_geometry(rate, out=OUT):
    """The resample kernel's launch for `rate`, restated from resample_threads / resample_span /
    rs_prepare: threads per workgroup, outputs per workgroup (tile), input samples a workgroup
    stages (span), and whether the engine takes the rate at all (up and span within the limits)."""
    p = design_params(rate, out)
    up, down, J = p["up"], p["down"], p["J"]
    threads = up if up > 256 else up * (256 // up)
    tile = Q * threads
    span = ((tile - 1) * down + up - 1) // up + J
    return dict(threads=threads, tile=tile, span=span,
                accepted=up <= MAX_THREADS and J + 1 <= MAX_SPAN and span <= MAX_SPAN)


def one_shot_lengths(rate, out=OUT):
    """[(n_in, n_out)] for a whole-signal resample whose outputs end just short of, on and just
    past a workgroup's tile: n_out = ceil(n_in * up / down) of 1, tile - 1, tile, tile + 1 and
    2 * tile + 3.  When upsampling not every n_out exists (4/3: 2, 3, 4, 6, ..): the nearest one
    below and the nearest one above stand in for it."""
    p = design_params(rate, out)
    up, down = p["up"], p["down"]
    tile = launch_geometry(rate, out)["tile"]
    n_ins = set()
    for target in (1, tile - 1, tile, tile + 1, 2 * tile + 3):
        n_in = max(1, target * down // up)           # the longest input with n_out <= target
        n_ins.add(n_in)
        if -(-n_in * up // down) != target:
            n_ins.add(n_in + 1)                      # the shortest with n_out > target
    return [(n, -(-n * up // down)) for n in sorted(n_ins)]


def host_taps(rate, out=OUT):
    from scipy.signal import firwin
    p = design_params(rate, out)
    return firwin(2 * p["half"] + 1, 1.0 / max(p["up"], p["down"]), window=("kaiser", 5.0)) * p["up"]


def stream_resample_ref(x, rate, block, taps=None, hist=None):
    """x: whole ticks of input (n_ticks * in_block samples) -> (n_ticks * block) float32, computed
    tick by tick: a tick reads its own in_block samples and the H samples before them (`hist`,
    default zeros, before the first).  Nothing else is visible to a tick."""
    p = design_params(rate)
    up, down, half, J, H, delay = (p[k] for k in ("up", "down", "half", "J", "H", "delay"))
    h = np.asarray(host_taps(rate) if taps is None else taps, np.float64)
    hp = np.concatenate([h, np.zeros(J * up - len(h))])      # taps past the filter are zero
    in_block = block * down // up
    assert block * down % up == 0 and len(x) % in_block == 0
    x = np.asarray(x, np.float32)
    prev = np.zeros(H, np.float32) if hist is None else np.asarray(hist, np.float32)
    assert len(prev) == H
    out = []
    for t in range(len(x) // in_block):
        cur = x[t * in_block:(t + 1) * in_block]
        win = np.concatenate([prev, cur]).astype(np.float64)   # index H + i - t * in_block
        n = t * block + np.arange(block, dtype=np.int64)
        c = (n - delay) * down + half
        i = c // up - t * in_block + H                          # floor division (c may be negative)
        ph = c - (c // up) * up
        assert i.max() < len(win) and (i - (J - 1)).min() >= 0, "a tick read outside its block + history"
        acc = np.zeros(block, np.float64)
        for j in range(J - 1, -1, -1):
            acc = acc + hp[ph + j * up] * win[i - j]
        acc[n < delay] = 0.0                                     # the stream starts with `delay` zeros
        out.append(acc.astype(np.float32))
        prev = np.concatenate([prev, cur])[-H:]
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def delayed_resample(x, rate, n_out=None):
    """concat(zeros(delay), audio.resample(x, rate, 16000)), cut to n_out samples."""
    from easywakeword_amd.audio import resample
    d = design_params(rate)["delay"]
    y = np.concatenate([np.zeros(d, np.float32), resample(np.asarray(x, np.float32), rate, OUT)])
    return y if n_out is None else y[:n_out]
