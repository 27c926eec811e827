"""The top_db shift rule's formulas (easywakeword_amd/csrc/ewk_topdb_shift.h) on the CPU.

tests/topdb_shift_model.cpp is compiled on the host against the header the kernel includes and
run once: on random tiles, in float64, the incremental rule -- shift_add per column, shift_rise
(s1, s2 and B) over a sequence of clamp rises, shift_replace for the tiles the rule refuses --
must reproduce the directly clamped sums within 1e-12 relative (s1 relative to sum |d|, s2 to
itself), and the rule must refuse every tile that holds a value in (run_k, theta).
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "topdb_shift_model.cpp")


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
    exe = str(tmp_path_factory.mktemp("topdb_shift") / "model")
    subprocess.run([cxx, "-O2", "-std=c++17", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return {k: float(v) for k, v in (line.split() for line in out.strip().splitlines())}


def test_incremental_rule_reproduces_the_clamped_sums(model):
    print(model)
    assert model["rises"] >= 50 and model["flagged"] >= 10 and model["kept"] >= 50   # every path ran
    assert model["rel_s1"] <= 1e-12
    assert model["rel_s2"] <= 1e-12


def test_rule_refuses_every_tile_with_a_value_in_the_window(model):
    assert model["flag_mismatch"] == 0
