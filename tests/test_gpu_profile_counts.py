"""Which launches the profiling brackets of ewk_profile_enable cover, as launch counts from
ewk_profile_read (kind 0 = fp32 scorer, 1 = fp64 re-scorer, 2 = gate, 3 = resampler): one
bracket per scorer launch and per re-score launch of a device batch and of a streaming pass,
one per gate launch, one around the resampler's launches of a push, one around a one-shot
resample.  A read drains its kind: the next one finds no launches."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

BLOCK = 1600


def counts(eng):
    return tuple(eng.profile_read(k)[1] for k in range(4))


def test_bracketed_launch_counts():
    import torch
    from easywakeword_amd import StreamEngine
    dev = torch.device("cuda", 0)
    eng = StreamEngine(2)
    eng.template_from_pcm(synth.load_word())
    eng.profile(True)
    assert counts(eng) == (0, 0, 0, 0)

    # one device batch of three short segments
    rng = np.random.default_rng(7)
    lengths = np.array([1600, 2401, 4000], np.int32)
    offsets = np.array([0, 1600, 4001], np.int64)
    pcm = torch.from_numpy((0.1 * rng.standard_normal(int(lengths.sum()))).astype(np.float32)).to(dev)
    off, ln = torch.from_numpy(offsets).to(dev), torch.from_numpy(lengths).to(dev)
    mean = torch.empty((3, 20), device=dev)
    std = torch.empty((3, 20), device=dev)
    score = torch.empty(3, device=dev, dtype=torch.float64)
    match = torch.empty(3, device=dev, dtype=torch.uint8)
    torch.cuda.synchronize()
    eng.score_device(pcm.data_ptr(), off.data_ptr(), ln.data_ptr(), 3, mean.data_ptr(), std.data_ptr(),
                     score.data_ptr(), match.data_ptr())
    eng.sync()
    assert counts(eng) == (1, 1, 0, 0)
    assert counts(eng) == (0, 0, 0, 0)

    # one push of three ticks: one gate launch, one scoring pass
    eng.push_many((0.1 * rng.standard_normal((2, 3 * BLOCK))).astype(np.float32))
    eng.sync()
    assert counts(eng) == (1, 1, 1, 0)
    assert counts(eng) == (0, 0, 0, 0)

    # the same push at 48 kHz: the resampler's launches of the push under one bracket
    eng.set_input_rate(48000)
    eng.push_many((0.1 * rng.standard_normal((2, 3 * eng.input_block))).astype(np.float32))
    eng.sync()
    assert counts(eng) == (1, 1, 1, 1)
    assert counts(eng) == (0, 0, 0, 0)

    # a one-shot resample
    y = eng.resample((0.1 * rng.standard_normal(4801)).astype(np.float32), 48000)
    assert y.size == 1601
    assert counts(eng) == (0, 0, 0, 1)
    assert counts(eng) == (0, 0, 0, 0)
    eng.close()
