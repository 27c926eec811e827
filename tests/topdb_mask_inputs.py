"""Inputs of the mask-rule tests ("top_db masks only where the clamp can still rise", mask_near /
mask_wanted in csrc/ewk_topdb_shift.h) and their numpy replay (no GPU): shared by
test_topdb_mask_inputs.py, which checks on the CPU that each input exercises the path it is meant
for, and test_gpu_topdb_mask_skip.py, which scores them on the GPU.

The tones are bin-centred (875 Hz = bin 28, 2,000 Hz = bin 64 of the 512-point FFT): a steady
frame holds three bins and every other band at the -100 dB floor, so a tile's mask is neither
empty nor full and no stored value lies near the clamp.  The scout reads four rows of 64 samples
at offsets 64 + 640 q of a tile (2,560 samples); a burst placed between the rows is invisible to it.
"""
import os
import re
import sys

import numpy as np

import topdb_shift_inputs as shift_inp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import scout_sim  # noqa: E402

SPEC_TILES = 48          # kSpecTiles (ewk_mfcc.hip)


def window_db():
    """X of the built rule: -10 log10 of EWK_MASK_NEAR_RATIO's default in the header."""
    text = open(os.path.join(ROOT, "easywakeword_amd", "csrc", "ewk_topdb_shift.h")).read()
    m = re.search(r"#define\s+EWK_MASK_NEAR_RATIO\s+([0-9.eE+-]+)f", text)
    return -10.0 * np.log10(float(m.group(1)))


def sine(n, f, amp):
    return amp * np.sin(2 * np.pi * f * np.arange(n) / 16000)


def loud_one_segment():
    """Tile 0 holds a loud tone, tiles 1..3 only a tone 40 dB down: the scout ranks them far below
    it, they hold the floor (more than 80 dB below the loud peak) and nothing after tile 0 raises
    the clamp.  No mask is built and nothing is recomputed."""
    n = 9600
    y = sine(n, 2000.0, 0.003)
    y[:2400] += sine(2400, 875.0, 0.3)
    return y.astype(np.float32)


def fooled_segment(a3):
    """The scout fooled: tile 0 holds a 0.15 tone, tiles 1 and 2 a tone 30 dB down (unmasked:
    nothing near tile 0 is left by the scout), and the last tile a louder burst (a3) between the
    scout's rows.  It is processed last and raises the clamp under tiles 0..2 by
    20 log10(a3 / 0.15) dB: all three hold clamped entries without a mask and are recomputed."""
    n = 9664
    y = np.zeros(n)
    y[:8380] += sine(8380, 2000.0, 0.005)
    y[:2200] += sine(2200, 875.0, 0.15)
    y[9088:] += sine(n, 875.0, a3)[9088:]
    return y.astype(np.float32)


def mixed_segment(a3=0.3):
    """Four tiles, three of them equally loud by the scout (K = 3: the first two processed get a
    mask, the third does not), then a burst between the scout's rows of the silent last tile.  The
    rise meets masked tiles (shifted, their steady passes never recomputed) and an unmasked one
    (recomputed, swapped as plain columns) in one segment."""
    n = 9664
    y = np.zeros(n)
    y[:7744] += sine(7744, 875.0, 0.15)
    y[9088:] += sine(n, 875.0, a3)[9088:]
    return y.astype(np.float32)


def first_unmasked_segment():
    """Two tiles: the first is self-clamped at its own max and gets no mask (the second is far
    down by the scout), the second holds a louder burst between the scout's rows."""
    n = 4600
    y = np.zeros(n)
    y[:3900] += sine(3900, 2000.0, 0.005)
    y[:2200] += sine(2200, 875.0, 0.15)
    y[3968:4544] += sine(n, 875.0, 0.3)[3968:4544]
    return y.astype(np.float32)


def tie_segment():
    """Equally loud tiles (880 Hz tone over noise): every tile but the last is masked and each
    later tile raises the clamp by ~0.001 dB."""
    return shift_inp.tie_segment(9600)


def replay(y):
    """The rule's replay on the oracle's log-mel, plus the clamp's rise at the last tile processed."""
    L = scout_sim.log_mel_raw(y)
    T = L.shape[1]
    ntile = (T + 15) // 16
    e = scout_sim.scout_energy(y, ntile)
    ordered = 1 < ntile <= SPEC_TILES
    order = sorted(range(ntile), key=lambda t: (-e[t], t)) if ordered else list(range(ntile))
    r = scout_sim.replay_mask_rule(L, order, e, window_db() if ordered else None)
    before = max(L[:, 16 * t:16 * t + 16].max() for t in order[:-1]) if ntile > 1 else L.max()
    r.update(tiles=ntile, order=order, last_rise=float(L.max() - before))
    return r


FOOLED = [(0.18, 1.5), (0.3, 6.0)]      # a3, the rise in dB at least


def check_loud_one():
    r = replay(loud_one_segment())
    assert r["tiles"] == 4 and r["order"][0] == 0 and r["near"] == 1, r
    assert r["masks"] == 0 and r["skipped"] == 4 and r["rises"] == 0 and r["passes"] == 0, r


def check_fooled(a3, rise):
    r = replay(fooled_segment(a3))
    assert r["tiles"] == 4 and r["order"] == [0, 1, 2, 3] and r["near"] == 1, r
    assert r["masks"] == 0 and r["last_rise"] >= rise, r
    # tiles 0, 1 and 2 hold clamped entries without a mask and meet the rise: all six passes
    assert r["skipped_fixed_tiles"] == 3 and r["skipped_fixed_passes"] == 6 and r["first_skipped_fixed"] == 1, r


def check_mixed():
    r = replay(mixed_segment())
    assert r["tiles"] == 4 and r["order"][3] == 3 and r["near"] == 3, r
    assert r["masks"] == 2 and r["skipped_fixed_tiles"] == 1 and r["last_rise"] >= 5.0, r
    assert r["kept_shifted_passes"] >= 1, r


def check_first_unmasked():
    r = replay(first_unmasked_segment())
    assert r["tiles"] == 2 and r["order"] == [0, 1] and r["near"] == 1, r
    assert r["masks"] == 0 and r["first_skipped_fixed"] == 1 and r["last_rise"] >= 5.0, r


def check_tie():
    r = replay(tie_segment())
    assert r["tiles"] == 4 and r["near"] == 4 and r["masks"] == 3 and r["skipped"] == 1 and r["rises"] >= 1, r
    assert r["last_rise"] < 0.01, r
