"""The float associations of k_score_f32's per-segment reductions (csrc/ewk_mfcc_stats.h), old
and new, modelled lane by lane in numpy: the new forms must give the old bits for any input.

  scout         old: lane = column of a 64-sample row, wave_sum_f (a row_shr 1, 2, 4, 8 scan over
                each 16-lane row, then (r0 + r1) + (r2 + r3) of the four lane-15 totals);
                new (scout_quads): lane l of a 16-lane row holds columns 4l .. 4l + 3, adds
                (c0 + c1) + (c2 + c3) and scans its row
  finish_stats  old: each of the ten doubles s1[0..4], s2[0..4] scanned over the 16 columns, lane 15
                holds the totals; new (row_sums_to_pd): the narrowing reduction with partners
                col ^ 1, col ^ 2, col ^ 7, col ^ 15, every lane storing the totals it ends up with

The models follow the kernels' data movement (which lane reads which, zeros where a DPP source is
missing), in the kernels' precision.  No GPU, no product code.
"""
import numpy as np
import pytest


def row_shr_scan(x):
    """x[..., 16] -> the DPP scan x += row_shr:d(x), d = 1, 2, 4, 8 (no source: 0), in x's dtype."""
    x = x.copy()
    for d in (1, 2, 4, 8):
        sh = np.zeros_like(x)
        sh[..., d:] = x[..., :-d]
        x = x + sh
    return x


def column_energy(x):
    """[4 rows, 64 columns] float32 -> the per-column chain a = x0 * x0, a = fma(xq, xq, a): the same
    statement in both scouts (a product of two float32 is exact in float64)."""
    x = x.astype(np.float32)
    a = x[0] * x[0]
    for q in range(1, 4):
        a = (x[q].astype(np.float64) * x[q].astype(np.float64) + a.astype(np.float64)).astype(np.float32)
    return a


def scout_old(a):
    """a[64] float32 per-lane values -> wave_sum_f."""
    r = row_shr_scan(a.reshape(4, 16))[:, 15]
    return np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3]))


def scout_new(a):
    """a[64] float32 per-column values, four columns per lane -> lane 15 of the row scan."""
    c = a.reshape(16, 4)
    s = (c[:, 0] + c[:, 1]) + (c[:, 2] + c[:, 3])
    return row_shr_scan(s.astype(np.float32))[15]


def finish_old(s1, s2):
    """s1, s2 [5 slots, 16 columns] float64 -> totals [2, 5] (lane 15 of each scan)."""
    return np.stack([row_shr_scan(s1)[:, 15], row_shr_scan(s2)[:, 15]])


def finish_new(s1, s2):
    """row_sums_to_pd on one 16-lane row: what every lane stores where.  Returns totals [2, 5] and
    checks that lanes storing to the same place store the same bits."""
    col = np.arange(16)
    k1 = ((col ^ (col >> 2)) & 1).astype(bool)
    k2 = (((col >> 1) ^ (col >> 2)) & 1).astype(bool)
    k3 = (((col >> 2) ^ (col >> 3)) & 1).astype(bool)

    def xchg(keep, send, x):        # lane l: keep[l] + send[l ^ x]
        return keep + send[..., col ^ x]

    v = xchg(np.where(k1, s2, s1), np.where(k1, s1, s2), 1)                  # [5, 16]
    w = np.stack([xchg(np.where(k2, v[2 * i + 1], v[2 * i]), np.where(k2, v[2 * i], v[2 * i + 1]), 2)
                  for i in range(2)])
    v4 = xchg(v[4], v[4], 2)
    z = xchg(np.where(k3, w[1], w[0]), np.where(k3, w[0], w[1]), 7)
    v4 = xchg(v4, v4, 7)
    z = xchg(z, z, 15)
    v4 = xchg(v4, v4, 15)
    pd = {}
    for l in range(16):
        for key, val in (((int(k1[l]), 2 * int(k3[l]) + int(k2[l])), z[l]), ((int(k1[l]), 4), v4[l])):
            bits = np.float64(val).view(np.int64)
            assert pd.setdefault(key, bits) == bits, (l, key)
    assert len(pd) == 10
    return np.array([[pd[(t, i)] for i in range(5)] for t in range(2)], np.int64).view(np.float64)


def _inputs(rng, shape, dtype):
    """Random values, denormals, zeros and values of very different magnitude, mixed by position."""
    tiny = np.finfo(dtype).tiny
    kinds = [
        rng.normal(0.0, 1.0, shape),
        rng.normal(0.0, 1.0, shape) * 10.0 ** rng.uniform(-30, 30, shape),
        rng.normal(0.0, 1.0, shape) * tiny * rng.uniform(0.0, 4.0, shape),        # around and below tiny
        np.zeros(shape),
        np.where(rng.random(shape) < 0.5, 0.0, rng.normal(0.0, 1e8, shape)),
    ]
    pick = rng.integers(0, len(kinds), shape)
    with np.errstate(all="ignore"):
        mixed = np.choose(pick, kinds).astype(dtype)
        return [k.astype(dtype) for k in kinds] + [mixed]


@pytest.mark.parametrize("seed", range(4))
def test_scout_association(seed):
    rng = np.random.Generator(np.random.PCG64([70, seed]))
    n = 0
    with np.errstate(all="ignore"):
        for _ in range(6):
            for x in _inputs(rng, (4, 64), np.float32):
                a = column_energy(x)
                old, new = scout_old(a), scout_new(a)
                assert np.float32(old).view(np.int32) == np.float32(new).view(np.int32), (old, new)
                n += 1
        # energies that overflow, and a NaN column: the same infinity, a NaN either way
        big = np.full((4, 64), 3e19, np.float32)
        assert scout_old(column_energy(big)) == scout_new(column_energy(big)) == np.inf
        big[2, 17] = np.nan
        assert np.isnan(scout_old(column_energy(big))) and np.isnan(scout_new(column_energy(big)))
    assert n == 36


@pytest.mark.parametrize("seed", range(4))
def test_finish_stats_tree(seed):
    rng = np.random.Generator(np.random.PCG64([71, seed]))
    with np.errstate(all="ignore"):
        for _ in range(6):
            for s1, s2 in zip(_inputs(rng, (5, 16), np.float64), _inputs(rng, (5, 16), np.float64)):
                s2 = np.abs(s2)
                old, new = finish_old(s1, s2), finish_new(s1, s2)
                np.testing.assert_array_equal(old.view(np.int64), new.view(np.int64))
    nan = np.full((5, 16), np.nan)                  # NaN input: every s1 is the same NaN
    s2 = np.abs(rng.normal(0.0, 1.0, (5, 16)))
    old, new = finish_old(nan, s2), finish_new(nan, s2)
    assert np.isnan(old[0]).all() and np.isnan(new[0]).all()
    np.testing.assert_array_equal(old[1].view(np.int64), new[1].view(np.int64))


def test_the_models_notice_another_pairing():
    """A sequential sum of the same values differs from the tree for some input: the equality above
    is not vacuous."""
    rng = np.random.Generator(np.random.PCG64([72]))
    a = column_energy(rng.normal(0.0, 1.0, (4, 64)).astype(np.float32))
    seq = np.float32(0.0)
    for v in a:
        seq = np.float32(seq + v)
    assert seq != scout_old(a)
    s = rng.normal(0.0, 1.0, (5, 16))
    assert (np.add.accumulate(s, axis=1)[:, 15] != row_shr_scan(s)[:, 15]).any()
