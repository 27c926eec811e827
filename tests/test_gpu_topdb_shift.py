"""The scorer's top_db shift (csrc/ewk_topdb_shift.h) on the GPU against the oracle.

A stored tile's clamped log-mel entries move up with the speculative clamp inside the
statistics (mask DCT, three running sums); only a tile holding an unclamped value below the
final threshold is recomputed.  The inputs are built in tests/topdb_shift_inputs.py; a numpy replay
of the rule (scripts/scout_sim.py, no GPU) asserts that each exercises the path it is meant for,
here before the GPU is touched and again in test_topdb_shift_inputs.py, which needs no GPU.  The
segments go through Engine.score_device and are compared with oracle/mfcc_ref.py at the bars of
test_gpu_fullsize.py (score within 1e-4, identical decisions) and test_gpu_scorer.py (mean / std
within rtol 1e-4, atol 2e-3).
"""
import numpy as np
import pytest

import synth
import topdb_shift_inputs as inp
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


@pytest.mark.parametrize("n", [9600, 25600])
def test_tie_case_is_shifted_only(env, n):
    inp.check_tie(n)
    check_vs_oracle(env, inp.tie_segment(n), f"tie L={n}")


def test_self_clamp_late_in_the_order(env):
    inp.check_self_clamp()
    check_vs_oracle(env, inp.self_clamp_segment(), "self-clamp")


@pytest.mark.parametrize("f2,a3,rise", inp.KEPT)
def test_kept_tiles_shift_by_a_large_rise(env, f2, a3, rise):
    """Tiles 1 and 2 are never recomputed and their clamp rises by `rise` dB: a wrong mask, sign
    or coefficient slot moves every coefficient of 32 of the 61 frames far past the bars (left at
    their own clamp they move c0 alone by ~10 x rise)."""
    inp.check_kept_rise(f2, a3, rise)
    check_vs_oracle(env, inp.kept_rise_segment(f2, a3), f"kept rise f2={f2} a3={a3}")


def test_fallback_still_recomputes(env):
    inp.check_fallback()
    check_vs_oracle(env, inp.fallback_segment(), "fallback")


@pytest.mark.parametrize("n,frames,tiles", inp.EDGES)
def test_edges_of_the_tile_grid(env, n, frames, tiles):
    inp.check_edge(n, frames, tiles)
    check_vs_oracle(env, inp.tie_segment(n, seed=1), f"edge L={n}")


def test_nan_sample_gives_nan_statistics(env):
    y = inp.tie_segment(9600)
    y[5000] = np.nan
    mean, std, score, match = score_device(env, [y])
    # as before the shift: NaN means, a NaN score, no match; the std output is 0 (finish_stats
    # floors a variance that is not > 0, NaN included, at 0), never a number computed from the NaN
    assert np.isnan(mean[0]).all() and np.isnan(score[0]) and not match[0]
    assert (std[0] == 0.0).all()


def test_segment_longer_than_the_tile_record(env):
    inp.check_long()
    check_vs_oracle(env, inp.tie_segment(130000), "long L=130000")


def test_batch_independence_bit_for_bit(env):
    ys = [inp.tie_segment(25600), inp.kept_rise_segment(*inp.KEPT[0][:2])]
    others = synth.ragged_segments(97, 62, 160, 40000)
    batch = list(others[:31]) + [ys[0]] + list(others[31:50]) + [ys[1]] + list(others[50:])
    assert len(batch) == 64
    mb, sb, scb, _ = score_device(env, batch)
    for y, k in zip(ys, (31, 51)):
        m1, s1, sc1, _ = score_device(env, [y])
        np.testing.assert_array_equal(m1[0], mb[k])
        np.testing.assert_array_equal(s1[0], sb[k])
        np.testing.assert_array_equal(sc1[0], scb[k])
