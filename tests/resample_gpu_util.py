"""Shared by the resampler's GPU tests (test_gpu_resample.py, test_gpu_resample_rates.py): the
tolerance, the test signals and the streaming push sequence.

Tolerance, every sample: |device - host| <= max(one float32 ulp of the host value, 2^-40 max|x|).
Both sides accumulate at most 256 products in float64 (error < 2^-43 max|x|) and round once to
float32, so they can differ only where the float64 sums straddle a rounding boundary, and then
by one ulp; the absolute term covers outputs that cancel to near zero.  The count of samples that
are not bit-equal is printed (expected: about none)."""
import ctypes as C

import numpy as np

from resample_ref import delayed_resample, design_params

BLOCK = 1600
MAX_PRODUCTS = 256      # the tolerance's argument: J, the products of one output, is at most this


def in_block_of(rate, block=BLOCK):
    p = design_params(rate)
    assert block * p["down"] % p["up"] == 0
    return block * p["down"] // p["up"]


def assert_close(dev, host, x_max, what):
    dev, host = np.asarray(dev, np.float32), np.asarray(host, np.float32)
    assert dev.shape == host.shape, (what, dev.shape, host.shape)
    if dev.size == 0:
        return 0
    tol = np.maximum(np.spacing(np.abs(host)).astype(np.float64), 2.0 ** -40 * float(x_max))
    err = np.abs(dev.astype(np.float64) - host.astype(np.float64))
    unequal = int(np.count_nonzero(dev != host))
    print(f"{what}: {dev.size} samples, {unequal} not bit-equal, max err {float(err.max()):.3e}")
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, (what, bad[:8], dev[bad[:8]], host[bad[:8]])
    return unequal


def signal(kind, n, seed):
    if kind == "noise":
        return (0.3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    return np.where((np.arange(n) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)   # full-scale square wave


def stream_data(rate, n_ticks, pcm16, block=BLOCK, n_streams=3):
    """[n_streams][n_ticks * in_block] noise at `rate`, float32 or the int16 it rounds to."""
    ib = in_block_of(rate, block)
    rng = [np.random.default_rng(1000 * rate + s) for s in range(n_streams)]
    data = np.stack([(0.25 * r.standard_normal(n_ticks * ib)).astype(np.float32) for r in rng])
    if pcm16:
        data = np.clip(np.round(data * 32768.0), -32768, 32767).astype(np.int16)
    return data


def push_sequence(eng, data, rate, pcm16, block=BLOCK, pattern=(1, 3, 1, 1)):
    """The pushes of `pattern` (ticks per call: one tick is a push, more are a push_many with
    tick_stride != in_block); streams stride > n_ticks * tick_stride apart, the gaps filled with
    a value that must not be read.  data: [n_streams][sum(pattern) * in_block].  After each call
    read_last of the ticks just pushed is checked against the delayed host resample of everything
    pushed so far; returns every read_last, concatenated."""
    from easywakeword_amd import _lib
    lib = eng._lib
    ib = in_block_of(rate, block)
    n_s, total = data.shape[0], sum(pattern)
    assert data.shape[1] == total * ib
    dt = np.int16 if pcm16 else np.float32
    x = data if not pcm16 else data.astype(np.float32) / np.float32(32768.0)
    want = [delayed_resample(x[s], rate, total * block) for s in range(n_s)]
    x_max = float(np.max(np.abs(x)))
    out = []
    done = 0
    for nt in pattern:
        tick_stride = ib + 5
        stride = nt * tick_stride + 11
        buf = np.full(n_s * stride, 9 if pcm16 else 9.0, dt)       # the gaps must not be read
        for s in range(n_s):
            for t in range(nt):
                buf[s * stride + t * tick_stride: s * stride + t * tick_stride + ib] = \
                    data[s, (done + t) * ib:(done + t + 1) * ib]
        ptr = buf.ctypes.data_as(C.c_void_p)
        if nt == 1:
            fn = lib.ewk_push_pcm16 if pcm16 else lib.ewk_push
            _lib.check(fn(eng.handle, ptr, stride, 0))
        else:
            fn = lib.ewk_push_many_pcm16 if pcm16 else lib.ewk_push_many
            _lib.check(fn(eng.handle, ptr, stride, tick_stride, nt, 0))
        done += nt
        for s in range(n_s):
            got = eng.read_last(s, nt * block)
            assert_close(got, want[s][(done - nt) * block: done * block], x_max,
                         f"{rate} Hz block {block} {'pcm16' if pcm16 else 'f32'} stream {s} ticks {done - nt}..{done}")
            out.append(got)
    d = design_params(rate)["delay"]
    assert all(np.all(w[:d] == 0) for w in want)
    return np.concatenate(out)
