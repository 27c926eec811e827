"""build_pw_tree (csrc/ewk_gate_tree.h), the host-side flattening of numpy's pairwise summation
that k_gate_ticks evaluates level by level.  A stand-alone program built with g++
-fsanitize=address,undefined (the header is HIP-free; nothing of it is loaded into Python) builds
the tree of every length below, evaluates it in plain C++ the way the device's tree_sumsq does --
every leaf with numpy's eight accumulators, then the levels in order -- on the squares of a seeded
float32 vector, and prints the sum's bits and pw_tree_kind.  The bits must be those of
oracle.gate_ref.pairwise_sum_f64, the kinds those tests/gate_matrix.py expects of its blocks.
CPU only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import gate_matrix as gm
from oracle.gate_ref import pairwise_sum_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "easywakeword_amd", "csrc", "ewk_gate_tree.h")
LENGTHS = (1, 7, 8, 9, 120, 124, 125, 128, 129, 250, 260, 496, 498, 500, 1000, 1600, 2000, 3200, 4100, 4104, 8191, 8192)

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "%s"
using namespace ewk;

// tree_sumsq's additions: a leaf's eight accumulator chains, their combination and the tail, then
// every internal node from its two children, level after level
static double eval(const PwTree& t, const float* x) {
    const int L = t.n_leaves;
    std::vector<double> val(L + kPwMaxLeaves);
    for (int l = 0; l < L; ++l) {
        const int s0 = t.leaf_start[l], n = t.leaf_len[l];
        double res = 0.0;
        if (n < 8) {
            for (int i = 0; i < n; ++i) { const double v = x[s0 + i]; res += v * v; }
        } else {
            double r[8];
            for (int j = 0; j < 8; ++j) { const double v = x[s0 + j]; r[j] = v * v; }
            const int lim = n - n %% 8;
            for (int i = 8; i < lim; i += 8)
                for (int j = 0; j < 8; ++j) { const double v = x[s0 + i + j]; r[j] += v * v; }
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (int i = lim; i < n; ++i) { const double v = x[s0 + i]; res += v * v; }
        }
        val.at(l) = res;
    }
    int b = 0;
    for (int h = 0; h < t.n_levels; ++h) {
        const int e = t.level_end[h];
        for (int k = b; k < e; ++k) val.at(L + k) = val.at(t.left[k]) + val.at(t.right[k]);
        b = e;
    }
    return L == 1 ? val[0] : val.at(L + b - 1);
}

int main(int argc, char** argv) {
    std::vector<float> x(kPwChunk);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    fclose(f);
    for (int a = 2; a < argc; ++a) {
        const int n = atoi(argv[a]);
        PwTree t;
        build_pw_tree(n, &t);
        int covered = 0;   // the leaves tile [0, n) in order
        for (int l = 0; l < t.n_leaves; ++l) {
            if (t.leaf_start[l] != covered || t.leaf_len[l] < 1 || t.leaf_len[l] > 128) return 3;
            covered += t.leaf_len[l];
        }
        if (covered != n || t.n != n) return 3;
        const double s = eval(t, x.data());
        unsigned long long bits;
        memcpy(&bits, &s, 8);
        printf("%%d %%d %%llu\n", n, pw_tree_kind(t), bits);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("gate_tree")
    src, exe, vec = tmp / "tree_main.cpp", tmp / "tree_main", tmp / "x.f32"
    src.write_text(MAIN % HDR)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(src), "-o", str(exe)], check=True)
    x = (np.random.default_rng(20250311).standard_normal(8192) * 0.1).astype(np.float32)
    x[::97] = 0.0
    vec.write_bytes(x.tobytes())
    r = subprocess.run([str(exe), str(vec)] + [str(n) for n in LENGTHS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = {int(n): (int(kind), int(bits)) for n, kind, bits in (l.split() for l in r.stdout.splitlines())}
    assert sorted(out) == sorted(LENGTHS)
    return x, out


@pytest.mark.parametrize("n", LENGTHS)
def test_flattened_tree_sums_in_numpys_order(rows, n):
    x, out = rows
    sq = x[:n].astype(np.float64) ** 2
    want = pairwise_sum_f64(sq)
    assert want == np.add.reduce(sq)
    assert out[n][1] == struct.unpack("<Q", struct.pack("<d", want))[0]


def test_tree_kinds_are_the_gate_matrix_cases(rows):
    _, out = rows
    for name, case in gm.CASES.items():
        assert case["block"] in out, name
        assert out[case["block"]][0] == case["tree"], (name, gm.TREE_KINDS[out[case["block"]][0]])
    assert out[1600][0] == 2    # the last window everywhere
    assert {k for k, _ in out.values()} == set(gm.TREE_KINDS)
