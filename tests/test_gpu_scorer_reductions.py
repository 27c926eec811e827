"""k_score_f32's per-segment reductions (csrc/ewk_mfcc_stats.h: the scout with sixteen lanes per
tile, the wave minima / maxima, the narrowing row sums of finish_stats) on linear batches, through
Engine.score_device: segments chosen for the places where those steps can go wrong, each scored
alone and inside one batch of all of them (51 segments, so several workgroups run).

  frames      T = 1, 2, 8, 9, 16, 17, 41: one pass, two passes, one tile and the first frame of
              the next, tone and click probes (tests/scorer_matrix.py)
  tiles       1, 2, 4, 5, 8, 9, 17, 48 and 49 tiles: the scout's groups of four and batches of
              eight tiles, a time-ordered single tile, the last recorded tile (48) and the first
              segment that is taken in time order without a scout (49)
  end         the segment's last sample 0 (the row starts past the end), 1, 2, 3, 5 and 63 samples
              into a 64-sample scout row of tile 1, 4 and 8, and between two rows: a 16-byte scout
              load that straddles the end must read what four dword loads read
  ties        a 2,560-sample block repeated over 4 and 9 tiles: equal scout energies, ranked by index
  silence     all zeros: every log-mel value at the floor, std exactly 0, NaN score
  NaN         one NaN sample: NaN statistics and score, the rest of the batch undisturbed

Bars: tests/test_gpu_scorer_matrix.py's (its record() and report(): drift 1e-4 above 16 frames,
every coefficient within rtol 1e-4 / atol 2e-3, the score within 1e-4, the oracle's decision),
against oracle/mfcc_ref.py's float64 statistics, and the same bits alone as inside the batch.
"""
import math

import numpy as np
import pytest

import scorer_matrix as sm
from test_gpu_scorer_matrix import _same_bits, env, record, report, score_packed   # noqa: F401 (env: fixture)

pytestmark = pytest.mark.gpu

HOP = sm.HOP
FRAMES = (1, 2, 8, 9, 16, 17, 41)
TILES = (1, 2, 4, 5, 8, 9, 17, 48, 49)
TILE_EDGE = (2, 5, 9)                     # a click probe whose last tile holds one frame
ROWS = ((1, 2), (4, 0), (8, 3))           # (tile, row): the scout row the segment ends in
INTO_ROW = (0, 1, 2, 3, 5, 63, 164)       # samples of that row inside the segment (164: between rows)
TIE_TILES = (4, 9)


def _probe(kind, L, seed):
    T = 1 + L // HOP
    rem = L - (T - 1) * HOP
    return sm.tone_probe(128, T, rem, seed=seed) if kind == "tone" else sm.click_probe(T, rem, seed=seed)


def scout_row_start(tile, row):
    """First sample of scout row `row` of tile `tile` (csrc/ewk_mfcc_stats.h: one 64-sample row every
    640 samples, from sample 64 of the tile's 2,560)."""
    return tile * 16 * HOP + 640 * row + 64


def _build():
    out = []
    for T in FRAMES:
        out.append((f"frames_tone_T{T}", _probe("tone", sm.seg_len(T, 37), (60,))))
        out.append((f"frames_click_T{T}", _probe("click", sm.seg_len(T, 37), (60,))))
    for n in TILES:
        out.append((f"tiles_{n}", _probe("tone", sm.seg_len(16 * n, 37), (61,))))
    for n in TILE_EDGE:
        out.append((f"tiles_{n}_edge", _probe("click", sm.seg_len(16 * (n - 1) + 1, 0), (61,))))
    for tile, row in ROWS:
        for d in INTO_ROW:
            out.append((f"end_t{tile}_r{row}_d{d}", _probe("tone", scout_row_start(tile, row) + d, (62, tile))))
    block = sm.tone_probe(128, 17, 0, seed=(63,))[:16 * HOP]
    for n in TIE_TILES:
        out.append((f"ties_{n}", np.tile(block, n)))
    out.append(("silence", np.zeros(sm.seg_len(41, 37), np.float32)))
    x = _probe("tone", sm.seg_len(41, 37), (64,)).copy()
    x[3000] = np.nan
    out.append(("nan_sample", x))
    assert len({n for n, _ in out}) == len(out) <= 80
    return out


@pytest.fixture(scope="module")
def segments():
    return _build()


@pytest.fixture(scope="module")
def batch(env, segments):
    return score_packed(env, [x for _, x in segments])


def test_inputs_sit_where_they_claim(segments):
    """The lengths reach the tile counts and the scout rows named above."""
    by = dict(segments)
    for n in TILES:
        assert (sm.n_frames(by[f"tiles_{n}"]) + 15) // 16 == n
    for n in TILE_EDGE:
        assert sm.n_frames(by[f"tiles_{n}_edge"]) == 16 * (n - 1) + 1
    for tile, row in ROWS:
        for d in INTO_ROW:
            x = by[f"end_t{tile}_r{row}_d{d}"]
            assert len(x) - scout_row_start(tile, row) == d
            assert (sm.n_frames(x) + 15) // 16 > tile          # the row's tile exists, and is scouted
            assert 1 < (sm.n_frames(x) + 15) // 16 <= 48
    for n in TIE_TILES:
        x = by[f"ties_{n}"].reshape(n, -1)
        assert (x == x[0]).all()


def test_against_the_oracle(env, segments, batch):
    recs = []
    for i, (name, x) in enumerate(segments):
        if name in ("silence", "nan_sample"):
            continue
        recs.append(record(env, name, sm.n_frames(x), sm.stats_of(x), sm.stats_of(x, np.float32),
                           [a[i] for a in batch]))
    report("scorer reductions", recs)


def test_silence_and_nan(segments, batch):
    names = [n for n, _ in segments]
    mean, std, score, match = batch
    i = names.index("silence")
    print(f"silence: mean[0] {mean[i][0]!r} std max {std[i].max()!r} score {score[i]!r}")
    assert np.isfinite(mean[i]).all() and not std[i].any()
    assert math.isnan(score[i]) and not match[i]
    i = names.index("nan_sample")
    print(f"nan_sample: mean {mean[i][:3]!r} score {score[i]!r}")
    assert np.isnan(mean[i]).all() and math.isnan(score[i]) and not match[i]
    others = [k for k, n in enumerate(names) if n != "nan_sample" and sm.n_frames(segments[k][1]) > 1]
    assert np.isfinite(mean[others]).all() and np.isfinite(std[others]).all()


def test_alone_as_in_the_batch(env, segments, batch):
    alone = [score_packed(env, [x]) for _, x in segments]
    alone = [np.concatenate([r[k] for r in alone]) for k in range(4)]
    diff = [n for i, (n, _) in enumerate(segments)
            if not all(np.array_equal(a[i:i + 1].view(np.uint8), b[i:i + 1].view(np.uint8)) for a, b in zip(alone, batch))]
    print(f"{len(segments)} segments alone and in one batch; differing: {diff}")
    _same_bits(alone, batch, "alone vs inside the batch")
