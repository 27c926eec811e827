"""Inputs of the top_db shift tests and their numpy replay (no GPU): shared by
test_topdb_shift_inputs.py, which checks on the CPU that each input exercises the path it is meant
for, and test_gpu_topdb_shift.py, which scores them on the GPU."""
import os
import sys

import numpy as np

import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import scout_sim  # noqa: E402

SPEC_TILES = 48          # tiles the kernel records and scout-orders (kSpecTiles, ewk_mfcc.hip)


def tone(n, amp=0.3):
    return amp * np.sin(2 * np.pi * 880 * np.arange(n) / 16000)


def tie_segment(n, seed=0):
    """Equally loud tiles: each later tile raises the running max by ~0.001 dB."""
    return (tone(n) + np.random.default_rng(seed).normal(0.0, 1e-4, n)).astype(np.float32)


def self_clamp_segment(seed=0):
    """A tone that steps up 6 dB in the middle of the last tile, where the scout's four sample
    rows do not look: the tile is processed last and raises the max over its own clamped values.
    The noise floor of every earlier tile reaches into the 6 dB the clamp rises by, so they are
    all recomputed: the shift and the fix-up that takes it out again run together."""
    s0 = 4 * 2560
    n = s0 + 1984
    amp = np.where(np.arange(n) < s0 + 1408, 0.15, 0.3)
    return (amp * np.sin(2 * np.pi * 880 * np.arange(n) / 16000) +
            np.random.default_rng(seed).normal(0.0, 1e-4, n)).astype(np.float32)


def kept_rise_segment(f2=2000.0, a3=0.3):
    """Tiles that are shifted by a large rise and never recomputed.  Tile 0 holds a 0.15 tone and
    is processed first; tiles 1 and 2 hold only a quiet bin-centred tone (three FFT bins, every
    other band far below the clamp: a mask that is neither empty nor full, and no value near
    the clamp); the last tile holds a louder 880 Hz burst (a3) between the scout's sample rows,
    so it is processed last and raises the clamp under tiles 1 and 2 by 20 log10(a3 / 0.15) dB."""
    n = 9664
    t = np.arange(n)
    y = np.zeros(n)
    y[:8380] += 0.05 * np.sin(2 * np.pi * f2 * t[:8380] / 16000)
    y[:2200] += 0.15 * np.sin(2 * np.pi * 880 * t[:2200] / 16000)
    y[9088:] += a3 * np.sin(2 * np.pi * 880 * t[9088:] / 16000)
    return y.astype(np.float32)


def fallback_segment(seed=10):
    """The golden word at gain 3 over sigma = 1e-4 noise, placed (seed searched on the CPU) so
    that the scout ranks a quieter tile first and a tile keeps an unclamped value below theta."""
    word = synth.load_word()
    rng = np.random.default_rng(seed)
    n = int(rng.integers(12000, 33600))
    st = int(rng.integers(0, n - len(word)))
    y = rng.normal(0.0, 1e-4, n)
    y[st:st + len(word)] += 3.0 * word
    return y.astype(np.float32)


def replay(y):
    L = scout_sim.log_mel_raw(y)
    ntile = (L.shape[1] + 15) // 16
    ordered = 1 < ntile <= SPEC_TILES
    return scout_sim.replay_rules(L, scout_sim.scout_order(y, ntile) if ordered else list(range(ntile)))


EDGES = [(2400, 16, 1), (4960, 32, 2), (5120, 33, 3)]      # samples, frames, tiles
KEPT = [(1000.0, 0.3, 6.0), (2000.0, 0.18, 1.5)]           # f2, a3, the rise in dB at least


def check_tie(n):
    r = replay(tie_segment(n))
    assert r["tiles"] == (4 if n == 9600 else 11)
    assert r["old_tiles"] >= 1 and r["new_tiles"] == 0 and r["masked"] >= 2, r


def check_self_clamp():
    r = replay(self_clamp_segment())
    assert r["late_self_clamps"] >= 1 and r["masked"] == r["tiles"] == 5 and r["new_tiles"] == 4, r


def check_kept_rise(f2, a3, rise):
    r = replay(kept_rise_segment(f2, a3))
    # tiles 1 and 2 (four passes): masked with a partial mask, not recomputed, risen by >= `rise`
    assert r["tiles"] == 4 and r["new_tiles"] == 1 and r["late_self_clamps"] >= 1, r
    assert r["kept_partial"] >= 4 and r["max_kept_rise"] >= rise >= 1.0, r


def check_fallback():
    r = replay(fallback_segment())
    assert r["new_tiles"] >= 1 and r["masked"] > r["new_tiles"], r


def check_edge(n, frames, tiles):
    r = replay(tie_segment(n, seed=1))
    assert 1 + n // 160 == frames and r["tiles"] == tiles and r["masked"] >= 1, r


def check_long():
    r = replay(tie_segment(130000))
    assert r["tiles"] > SPEC_TILES and r["masked"] >= SPEC_TILES, r   # the unrecorded tiles too
