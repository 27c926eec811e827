"""Masks only where the clamp can still rise (mask_near / mask_wanted in
easywakeword_amd/csrc/ewk_topdb_shift.h) on the CPU.

tests/topdb_mask_model.cpp is compiled on the host against the header the kernel includes and run
once.  On random tiles in random processing orders, with every, no or a random subset of the tiles
that hold clamped entries left without a mask, the scorer's bookkeeping in float64 -- the shift for
masked tiles, the per-pass records, the recompute of flagged passes, the plain swap for an unmasked
tile that met a rise -- must reproduce the sums of the tiles clamped at the final threshold
directly within 1e-12 relative (s1 relative to sum |d|, s2 to itself: fp64 rounding of sums of a
few thousand terms), and no pass whose stored image is wrong may go unflagged.  The count of near
tiles is checked on ties, an all-zero scout, NaN, one tile and the last position.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "topdb_mask_model.cpp")


def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("topdb_mask") / "model")
    subprocess.run([cxx, "-O2", "-std=c++17", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return {k: float(v) for k, v in (line.split() for line in out.strip().splitlines())}


def test_any_subset_of_unmasked_tiles_reproduces_the_clamped_sums(model):
    print(model)
    # every path ran: all masked, none masked, mixed; kept and recomputed passes of both kinds
    assert model["trials_all"] >= 10 and model["trials_none"] >= 10 and model["trials_some"] >= 10
    assert model["rises"] >= 50
    assert model["masked_kept"] >= 20 and model["masked_fixed"] >= 10
    assert model["unmasked_kept"] >= 20 and model["unmasked_fixed"] >= 20
    assert model["rel_s1"] <= 1e-12
    assert model["rel_s2"] <= 1e-12


def test_no_wrong_pass_goes_unflagged(model):
    assert model["missed"] == 0


def test_count_of_near_tiles(model):
    assert 0.0 < model["ratio"] < 1.0
    assert model["k_ties"] == 5          # equal energies: every tile near, all but the last masked
    assert model["k_zero"] == 3          # an all-zero scout: the same
    assert model["k_all_nan"] == 2       # NaN is mapped to 0
    assert model["k_nan"] == 1
    assert model["k_one"] == 1 and model["k_one_zero"] == 1
    assert model["k_edge"] == 2          # e == ratio * e_max counts as near
    assert model["k_loud_one"] == 1


def test_last_position_and_single_tile_are_never_masked(model):
    assert model["last_masked"] == 0
    assert model["single_masked"] == 0


def test_count_agrees_with_the_next_tile_in_descending_order(model):
    """Position k is masked under the count exactly when tile k + 1 of the descending order is
    within the window of the loudest."""
    assert model["order_mismatch"] == 0
