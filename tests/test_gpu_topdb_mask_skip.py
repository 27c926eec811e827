"""Masks only where the clamp can still rise (mask_near / mask_wanted, csrc/ewk_topdb_shift.h) on
the GPU against the oracle.

A tile with clamped entries gets its mask DCT only if the scout ranks the next tile within X dB of
the loudest; a tile left without one that does meet a later rise is recomputed and swapped as
plain columns.  The inputs are built in tests/topdb_mask_inputs.py; a numpy replay of the rule
asserts that each exercises the path it is meant for, here before the GPU is touched and again in
test_topdb_mask_inputs.py, which needs no GPU.  The segments (2-6 tiles, or the 51-tile one in
time order) go through Engine.score_device and are compared with oracle/mfcc_ref.py at the bars of
test_gpu_fullsize.py (score within 1e-4, identical decisions) and test_gpu_scorer.py (mean / std
within rtol 1e-4, atol 2e-3).
"""
import numpy as np
import pytest

import synth
import topdb_mask_inputs as inp
import topdb_shift_inputs as shift_inp
from golden_io import score_close
from oracle import mfcc_ref

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4


@pytest.fixture(scope="module")
def env():
    import torch
    import easywakeword_amd as ewa
    dev = torch.device("cuda", 0)
    eng = ewa.Engine()
    eng.template_from_pcm(synth.load_word())
    yield torch, dev, eng
    eng.close()


def score_device(env, segs):
    torch, dev, eng = env
    n = len(segs)
    lengths = np.array([len(s) for s in segs], np.int32)
    offsets = np.zeros(n, np.int64)
    offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
    pcm = torch.from_numpy(np.concatenate(segs).astype(np.float32)).to(dev)
    off, ln = torch.from_numpy(offsets).to(dev), torch.from_numpy(lengths).to(dev)
    mean = torch.empty((n, 20), device=dev)
    std = torch.empty((n, 20), device=dev)
    score = torch.empty(n, device=dev, dtype=torch.float64)
    match = torch.empty(n, device=dev, dtype=torch.uint8)
    s = torch.cuda.current_stream(dev)
    eng.score_device(pcm.data_ptr(), off.data_ptr(), ln.data_ptr(), n, mean.data_ptr(), std.data_ptr(),
                     score.data_ptr(), match.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), std.cpu().numpy(), score.cpu().numpy(), match.cpu().numpy().astype(bool)


def check_vs_oracle(env, y, name):
    tm, ts = env[2].get_template()
    mean, std, score, match = score_device(env, [y])
    cm, cs = mfcc_ref.extract_mfcc(y.astype(np.float64))
    ref = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
    print(f"{name}: score {score[0]!r} oracle {ref!r} |d| {abs(score[0] - ref):.3e}  "
          f"max|dmean| {np.abs(mean[0] - cm).max():.3e}  max|dstd| {np.abs(std[0] - cs).max():.3e}")
    assert score_close(score[0], ref, SCORE_TOL), (name, score[0], ref)
    assert bool(match[0]) == (ref >= 75.0), name
    np.testing.assert_allclose(mean[0], cm, rtol=1e-4, atol=2e-3, err_msg=name)
    np.testing.assert_allclose(std[0], cs, rtol=1e-4, atol=2e-3, err_msg=name)


def test_loud_tile_first_no_mask_no_rise(env):
    inp.check_loud_one()
    check_vs_oracle(env, inp.loud_one_segment(), "loud tile first")


@pytest.mark.parametrize("a3,rise", inp.FOOLED)
def test_fooled_scout_unmasked_tiles_are_recomputed(env, a3, rise):
    """Tiles 0..2 hold clamped entries without a mask and the clamp rises under them by `rise` dB:
    left at their own clamp they would move c0 of 48 of the 61 frames by ~10 x rise."""
    inp.check_fooled(a3, rise)
    check_vs_oracle(env, inp.fooled_segment(a3), f"fooled a3={a3}")


def test_shift_and_replace_in_one_segment(env):
    inp.check_mixed()
    check_vs_oracle(env, inp.mixed_segment(), "masked and unmasked tiles under one rise")


def test_equal_tiles_mask_all_but_the_last(env):
    inp.check_tie()
    check_vs_oracle(env, inp.tie_segment(), "equal tiles")


def test_first_tile_self_clamped_and_unmasked(env):
    inp.check_first_unmasked()
    check_vs_oracle(env, inp.first_unmasked_segment(), "first tile unmasked")


def test_all_zero_pcm(env):
    """Silence: every tile sits at the -100 dB floor, the scout is all zero (every tile near).
    As before: the oracle's statistics, a standard deviation of exactly 0 and with it a NaN score
    and no match (the float64 oracle's own score for silence is a rounding artefact of a std of
    ~1e-13, test_gpu_scorer.py)."""
    y = np.zeros(9600, np.float32)
    mean, std, score, match = score_device(env, [y])
    cm, cs = mfcc_ref.extract_mfcc(y.astype(np.float64))
    np.testing.assert_allclose(mean[0], cm, rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(std[0], cs, rtol=1e-4, atol=2e-3)
    assert (std[0] == 0.0).all() and np.isnan(score[0]) and not match[0]


def test_nan_sample_gives_nan_statistics(env):
    y = inp.fooled_segment(0.3)
    y[5000] = np.nan
    mean, std, score, match = score_device(env, [y])
    # as before: NaN means, a NaN score, no match, the std output floored at 0
    assert np.isnan(mean[0]).all() and np.isnan(score[0]) and not match[0]
    assert (std[0] == 0.0).all()


def test_segment_in_time_order_keeps_every_mask(env):
    y = shift_inp.tie_segment(130000)
    assert 1 + len(y) // 160 > 16 * inp.SPEC_TILES   # 51 tiles: time order, the rule before
    check_vs_oracle(env, y, "long L=130000")


def test_batch_independence_bit_for_bit(env):
    ys = [inp.loud_one_segment(), inp.fooled_segment(0.18), inp.fooled_segment(0.3), inp.mixed_segment(),
          inp.tie_segment(), inp.first_unmasked_segment(), np.zeros(9600, np.float32)]
    others = list(synth.ragged_segments(97, 64 - len(ys), 2560, 15360))
    at = [3, 11, 19, 27, 35, 43, 51]
    batch, it = [], iter(others)
    for k in range(64):
        batch.append(ys[at.index(k)] if k in at else next(it))
    mb, sb, scb, _ = score_device(env, batch)
    for y, k in zip(ys, at):
        m1, s1, sc1, _ = score_device(env, [y])
        np.testing.assert_array_equal(m1[0], mb[k])
        np.testing.assert_array_equal(s1[0], sb[k])
        np.testing.assert_array_equal(sc1[0], scb[k])
