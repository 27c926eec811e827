"""Input-rate resampler on the GPU at every launch geometry: the rates whose workgroup is not
256 or 160 threads, whose staged span comes close to the LDS cap, whose streaming phase offset is
negative, and the tick sizes at which a workgroup's span crosses several ticks or a tick is
shorter than the history.  Reference and tolerance are those of test_gpu_resample.py
(resample_gpu_util): easywakeword_amd.audio.resample in float64, one float32 ulp.

Which case reaches which path of k_resample / k_resample_save / rs_prepare:
  rb < 0 (negative c0)        streaming at 12,000 (c0 = -2), 12,800 (-2), 9,600 Hz (-1)
  255 threads, partial wave   12,800 and 9,600 Hz (up = 5)
  320 / 240 / 640 / 1000      22,050 / 176,400 / 11,025 / 16,016 Hz
  span > 10,000 floats        176,400 (10,794) and 176,000 Hz (11,474)
  dt > 1 while staging        block 320 at 48,000 (in_block 960, span 3,130) and 8,000 Hz (160, 533)
  n_in < H in the save        block 320 at 1,000 Hz, single ticks (in_block 20, H 22)
  caller's strides            push_device / push_device_pcm16 / push_streams_device
  H changing                  48,000 -> 96,000 -> 12,000 -> 0 -> 22,050 Hz on one engine (62, 122, 22, 29)
"""
import numpy as np
import pytest

from resample_gpu_util import (BLOCK, MAX_PRODUCTS, assert_close, in_block_of, push_sequence, signal,
                               stream_data)
from resample_ref import OUT, delayed_resample, design_params, launch_geometry, one_shot_lengths

pytestmark = pytest.mark.gpu

ONE_SHOT_RATES = (32000, 24000, 22050, 96000, 12000, 12800, 11025, 16016, 176400, 176000)
STREAM_RATES = (12000, 12800, 9600, 22050, 24000, 32000, 96000)
SMALL_BLOCK = 320
SMALL_BLOCK_RATES = (48000, 8000, 12000, 1000, 2000)


@pytest.fixture(scope="module")
def scorer():
    from easywakeword_amd import Engine
    eng = Engine()
    yield eng
    eng.close()


@pytest.mark.parametrize("kind", ["noise", "square"])
@pytest.mark.parametrize("rate", ONE_SHOT_RATES)
def test_one_shot_at_tile_edges(scorer, rate, kind):
    import torch
    from easywakeword_amd.audio import resample
    p, g = design_params(rate), launch_geometry(rate)
    assert p["J"] <= MAX_PRODUCTS and g["accepted"]          # the tolerance's argument holds at this rate
    print(f"{rate} Hz: up {p['up']} down {p['down']} J {p['J']} threads {g['threads']} tile {g['tile']} span {g['span']}")
    for n, n_out in one_shot_lengths(rate):
        x = signal(kind, n, seed=rate + n)
        want = resample(x, rate, OUT)
        assert len(want) == n_out
        got = scorer.resample(x, rate)                       # host pointers
        assert_close(got, want, np.max(np.abs(x)), f"{rate} Hz {kind} n={n} -> {n_out} host")
        d_x = torch.from_numpy(x).cuda()                     # device pointers
        d_y = torch.full((n_out + 3,), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m = scorer.resample_device(d_x.data_ptr(), n, rate, d_y.data_ptr(), n_out + 3)
        scorer.sync()
        y = d_y.cpu().numpy()
        assert m == n_out
        assert np.all(y[m:] == 7.0)                          # nothing written past n_out
        assert_close(y[:m], want, np.max(np.abs(x)), f"{rate} Hz {kind} n={n} -> {n_out} device")


def _round_trip_16k(eng, seed):
    blk = (0.1 * np.random.default_rng(seed).standard_normal((eng.n_streams, eng.block))).astype(np.float32)
    eng.push(blk)
    for s in range(eng.n_streams):
        assert np.array_equal(eng.read_last(s, eng.block), blk[s])


def test_rates_over_the_limits_are_refused(scorer):
    from easywakeword_amd import StreamEngine
    from easywakeword_amd.audio import resample
    x = np.zeros(64, np.float32)
    assert not launch_geometry(192000)["accepted"] and not launch_geometry(16001)["accepted"]
    with pytest.raises(ValueError, match=r"up 1, down 12\).*up <= 1024, 12288 staged samples"):
        scorer.resample(x, 192000)                           # span 12,517 > 12,288
    with pytest.raises(ValueError, match=r"up 16000, down 16001\).*up <= 1024, 12288 staged samples"):
        scorer.resample(x, 16001)                            # up > 1024
    x = x + np.float32(0.5)                                  # a refusal leaves the engine usable
    assert_close(scorer.resample(x, 48000), resample(x, 48000, OUT), 0.5, "48000 Hz after the refusals")
    eng = StreamEngine(2)
    with pytest.raises(ValueError, match=r"up 1, down 12\)"):
        eng.set_input_rate(192000)
    assert (eng.input_rate, eng.input_block, eng.input_delay) == (OUT, BLOCK, 0)
    _round_trip_16k(eng, 192)
    eng.close()


@pytest.mark.parametrize("pcm16", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("rate", STREAM_RATES)
def test_streaming_block_1600(rate, pcm16):
    from easywakeword_amd import StreamEngine
    ib, p = in_block_of(rate), design_params(rate)
    if rate in (12000, 12800, 9600):
        assert p["half"] - p["delay"] * p["down"] < 0        # the floor-division fix-up of k_resample
    data = stream_data(rate, 6, pcm16)
    eng = StreamEngine(3)
    eng.set_input_rate(rate)
    assert (eng.input_rate, eng.input_block, eng.input_delay) == (rate, ib, p["delay"])
    first = push_sequence(eng, data, rate, pcm16)
    assert not first[:p["delay"]].any() and first[p["delay"]:BLOCK].any()
    eng.reset()                                              # the history is cleared: the same output again
    again = push_sequence(eng, data, rate, pcm16)
    assert np.array_equal(first, again)
    eng.close()


@pytest.mark.parametrize("rate", SMALL_BLOCK_RATES)
def test_streaming_block_320(rate):
    """20 ms ticks: at 48 and 8 kHz a workgroup's staged span covers several ticks (the dt > 1
    branch while staging, with tick_stride != in_block); at 1 kHz a tick (20 samples) is shorter
    than the history (22), which three single-tick pushes in a row build from two earlier pushes."""
    from easywakeword_amd import StreamEngine
    ib, p, g = in_block_of(rate, SMALL_BLOCK), design_params(rate), launch_geometry(rate)
    if rate in (48000, 8000):
        assert g["span"] > 2 * ib
    if rate == 1000:
        assert ib < p["H"]
    pattern = (1, 1, 1, 13, 1, 5) if rate in (1000, 2000) else (1, 13, 1, 5)
    data = stream_data(rate, sum(pattern), False, block=SMALL_BLOCK)
    eng = StreamEngine(3, block=SMALL_BLOCK, tick_seconds=SMALL_BLOCK / OUT)
    eng.set_input_rate(rate)
    assert (eng.input_rate, eng.input_block, eng.input_delay) == (rate, ib, p["delay"])
    first = push_sequence(eng, data, rate, False, block=SMALL_BLOCK, pattern=pattern)
    assert not first[:p["delay"]].any()
    eng.reset()
    again = push_sequence(eng, data, rate, False, block=SMALL_BLOCK, pattern=pattern)
    assert np.array_equal(first, again)
    eng.close()


def _device_rows(data, ib, first, nt, pad):
    """Ticks first .. first + nt of every row of `data` as a device tensor with
    stride > nt * tick_stride > in_block; the padding holds `pad`.  (tensor, stride, tick_stride)"""
    import torch
    tick_stride, stride = ib + 7, nt * (ib + 7) + 13
    buf = np.full((data.shape[0], stride), pad, data.dtype)
    for t in range(nt):
        buf[:, t * tick_stride: t * tick_stride + ib] = data[:, (first + t) * ib:(first + t + 1) * ib]
    return torch.from_numpy(buf).cuda(), stride, tick_stride


@pytest.mark.parametrize("rate,pcm16", [(48000, False), (12000, True)], ids=["48k_f32", "12k_pcm16"])
def test_device_pushes_equal_host_pushes(rate, pcm16):
    """The kernel reads the caller's stride and tick_stride directly (no host staging): the rings
    equal those of an engine fed the same values from host memory, bit for bit.  The padding
    between ticks and rows is full scale: one sample of it read would show."""
    import torch
    from easywakeword_amd import StreamEngine
    ib, p = in_block_of(rate), design_params(rate)
    data = stream_data(rate, 6, pcm16)
    x = data.astype(np.float32) / np.float32(32768.0) if pcm16 else data
    want = [delayed_resample(x[s], rate, 6 * BLOCK) for s in range(3)]
    pad = 32767 if pcm16 else 1.0e4
    host, dev, sub = StreamEngine(3), StreamEngine(3), StreamEngine(3)
    for e in (host, dev, sub):
        e.set_input_rate(rate)
    done = 0
    for nt in (1, 3, 2):
        cur = data[:, done * ib:(done + nt) * ib]
        (host.push_pcm16 if pcm16 else host.push_many)(cur)
        d, stride, tick_stride = _device_rows(data, ib, done, nt, pad)
        torch.cuda.synchronize()
        (dev.push_device_pcm16 if pcm16 else dev.push_device)(d.data_ptr(), stride, tick_stride, nt)
        dev.sync()
        done += nt
        for s in range(3):
            h = host.read_last(s, nt * BLOCK)
            assert_close(h, want[s][(done - nt) * BLOCK: done * BLOCK], float(np.max(np.abs(x))),
                         f"{rate} Hz host engine stream {s} ticks {done - nt}..{done}")
            np.testing.assert_array_equal(dev.read_last(s, nt * BLOCK), h, err_msg=f"stream {s} after {done} ticks")
    assert not host.read_last(0, 6 * BLOCK)[:p["delay"]].any()

    # one subset push from device memory: rows 0 and 1 go to streams 2 and 0, stream 1 is not touched
    (sub.push_pcm16 if pcm16 else sub.push_many)(data[:, :ib])               # (every stream has a tick)
    before = sub.read_last(1, BLOCK)
    np.testing.assert_array_equal(before, host.read_last(1, 6 * BLOCK)[:BLOCK])
    d, stride, tick_stride = _device_rows(data[[2, 0]], ib, 1, 3, pad)
    torch.cuda.synchronize()
    sub.push_streams_device([2, 0], d.data_ptr(), stride, tick_stride, 3, pcm16=pcm16)
    sub.sync()
    np.testing.assert_array_equal(sub.stream_ticks(), [4, 1, 4])
    for s in (2, 0):
        np.testing.assert_array_equal(sub.read_last(s, 4 * BLOCK), host.read_last(s, 6 * BLOCK)[:4 * BLOCK],
                                      err_msg=f"stream {s}")
    np.testing.assert_array_equal(sub.read_last(1, BLOCK), before)
    assert sub.state(1)["tick"] == 1
    for e in (host, dev, sub):
        e.close()


def test_rate_changes_on_a_live_engine():
    """set_input_rate clears the history and the history row changes its length (H = 62, 122, 22,
    29): after each change the stream is the delayed resample of that rate's input alone, its
    first `delay` samples zero again."""
    from easywakeword_amd import StreamEngine
    eng = StreamEngine(3)
    for rate in (48000, 96000, 12000, 0, 22050):
        eng.set_input_rate(rate)
        if rate == 0:
            assert (eng.input_rate, eng.input_block, eng.input_delay) == (OUT, BLOCK, 0)
            _round_trip_16k(eng, 5)
            continue
        ib, p = in_block_of(rate), design_params(rate)
        assert (eng.input_rate, eng.input_block, eng.input_delay) == (rate, ib, p["delay"])
        data = stream_data(rate, 3, False) + np.float32(0.5)     # (an offset: history left over would show)
        want = [delayed_resample(data[s], rate, 3 * BLOCK) for s in range(3)]
        x_max = float(np.max(np.abs(data)))
        eng.push(data[:, :ib])
        for s in range(3):
            got = eng.read_last(s, BLOCK)
            assert not got[:p["delay"]].any()
            assert_close(got, want[s][:BLOCK], x_max, f"after the change to {rate} Hz (H {p['H']}) stream {s} tick 0")
        eng.push_many(data[:, ib:])
        for s in range(3):
            assert_close(eng.read_last(s, 2 * BLOCK), want[s][BLOCK:], x_max,
                         f"after the change to {rate} Hz (H {p['H']}) stream {s} ticks 1..3")
    eng.close()
