"""ewk_chunk_plan (csrc/ewk_chunk_plan.h), the planning step of a chunk push: ticks and new pending
per chunk, the ticking chunks ordered by (ticks, position), the groups of equal ticks.  Checked
through the library against a numpy model on fixed and seeded random cases, and once more in a
stand-alone program built with g++ -fsanitize=address,undefined that replays the same cases (the
header is HIP-free; nothing of it is loaded into Python).  The same program runs the two layout
functions of a planned push (chunk_stage_layout, chunk_row_layout: internal, no export), checked
against numpy models and by their properties.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "easywakeword_amd", "csrc", "ewk_chunk_plan.h")
MAX_TICKS = 64


def model(in_block, pending, counts):
    total = np.asarray(pending, np.int64) + np.asarray(counts, np.int64)
    ticks, new = total // in_block, total % in_block
    idx = np.flatnonzero(ticks >= 1)
    order = idx[np.argsort(ticks[idx], kind="stable")]
    group_ticks = np.unique(ticks[order])
    first = np.r_[np.searchsorted(ticks[order], group_ticks), len(order)]
    return ticks, new, order, group_ticks, first


def stage_model(unit, pending, counts):
    """chunk_stage_layout: (src_at, total) -- every non-empty chunk at the next multiple of `unit`
    plus its pending % unit, an empty one at 0."""
    p, c = np.asarray(pending, np.int64), np.asarray(counts, np.int64)
    src_at, total = np.zeros(len(c), np.int64), 0
    for i in np.flatnonzero(c):
        src_at[i] = -(-total // unit) * unit + p[i] % unit
        total = int(src_at[i] + c[i])
    return src_at, total


def row_model(row_unit, in_block, group_ticks, first):
    """chunk_row_layout: (group_base, asm_total) -- group g holds one row of group_ticks[g] * in_block
    samples per member, from the next multiple of row_unit."""
    size = np.diff(np.asarray(first, np.int64)) * np.asarray(group_ticks, np.int64) * in_block
    base, total = np.zeros(len(size), np.int64), 0
    for g in range(len(size)):
        base[g] = -(-total // row_unit) * row_unit
        total = int(base[g] + size[g])
    return base, total


UNITS = (8, 16)     # samples in 32 bytes of float32 and of int16


def cases():
    """(in_block, pending, counts, group_cap): the fixed cases, then seeded random ones."""
    out = [
        (1600, [0, 5, 1599], [0, 0, 0], 64),                                # count 0
        (1600, [0, 0, 0, 0], [1599, 1600, 1601, 3200], 64),                 # pending 0
        (1600, [1, 800, 1599], [1599, 800, 1], 64),                         # pending + count == in_block exactly
        (1600, [1599], [1600], 64),                                         # in_block - 1 + in_block
        (1600, [0, 1599, 7], [64 * 1600, 64 * 1600, 64 * 1600 - 7], 64),    # 64 ticks
        (1, [0, 0, 0, 0], [0, 1, 5, 64], 64),                               # in_block 1
        (4410, [4409, 0, 17, 4409], [1, 4410, 13230, 4410 * 64], 64),       # in_block 4410
        (400, [0, 399, 1, 2], [400, 401, 1200, 2000], 64),                  # all ticking
        (400, [0, 100, 398], [399, 299, 1], 64),                            # none ticking
        (160, [], [], 0),                                                   # an empty call
        (1600, [0, 0, 0], [1600, 3200, 4800], 3),                           # group_cap exactly enough
    ]
    rng = np.random.default_rng(20240917)
    for _ in range(200):
        in_block = int(rng.choice([1, 2, 7, 160, 400, 1600, 4410, 4800]))
        n = int(rng.integers(0, 40))
        pending = rng.integers(0, in_block, n)
        kind = rng.integers(0, 3, n)
        counts = np.where(kind == 0, rng.integers(0, in_block + 1, n),
                          np.where(kind == 1, rng.integers(0, 4 * in_block + 1, n),
                                   rng.integers(0, MAX_TICKS * in_block + 1, n)))
        out.append((in_block, pending.tolist(), counts.tolist(), 64))
    return out


def plan(in_block, pending, counts, group_cap, fill=-7):
    """ewk_chunk_plan through the library: (rc, ticks, new_pending, order, n_ticking, group_ticks,
    group_first, n_groups); every output array starts filled with `fill`."""
    from easywakeword_amd import _lib
    lib = _lib.load()
    n = len(pending)
    p, c = np.array(pending, np.int32), np.array(counts, np.int32)
    ticks, new, order = (np.full(max(n, 1), fill, np.int32) for _ in range(3))
    gt, gf = np.full(max(group_cap, 1), fill, np.int32), np.full(group_cap + 1, fill, np.int32)
    nt, ng = C.c_int32(fill), C.c_int32(fill)
    rc = lib.ewk_chunk_plan(in_block, n, _lib.i32ptr(p), _lib.i32ptr(c), _lib.i32ptr(ticks), _lib.i32ptr(new),
                            _lib.i32ptr(order), C.byref(nt), _lib.i32ptr(gt), _lib.i32ptr(gf), group_cap, C.byref(ng))
    return rc, ticks[:n], new[:n], order[:n], nt.value, gt, gf, ng.value


def check_against_model(in_block, pending, counts, got):
    rc, ticks, new, order, nt, gt, gf, ng = got
    assert rc == 0
    m_ticks, m_new, m_order, m_gt, m_first = model(in_block, pending, counts)
    np.testing.assert_array_equal(ticks, m_ticks)
    np.testing.assert_array_equal(new, m_new)
    assert nt == len(m_order) and ng == len(m_gt)
    np.testing.assert_array_equal(order[:nt], m_order)
    np.testing.assert_array_equal(gt[:ng], m_gt)
    np.testing.assert_array_equal(gf[:ng + 1], m_first)
    # the invariants, on their own
    assert sorted(order[:nt].tolist()) == np.flatnonzero(ticks >= 1).tolist()       # a permutation of the ticking chunks
    assert (np.diff(gt[:ng]) > 0).all() and (gt[:ng] >= 1).all()                      # groups strictly increasing
    np.testing.assert_array_equal(ticks.astype(np.int64) * in_block + new,
                                  np.asarray(pending, np.int64) + np.asarray(counts, np.int64))
    assert ((new >= 0) & (new < in_block)).all()
    for g in range(ng):
        members = order[gf[g]:gf[g + 1]]
        assert (ticks[members] == gt[g]).all() and (np.diff(members) > 0).all()       # stable: in call order


def test_plan_equals_the_numpy_model():
    for in_block, pending, counts, cap in cases():
        check_against_model(in_block, pending, counts, plan(in_block, pending, counts, cap))


def test_failures_write_nothing():
    from easywakeword_amd import _lib
    bad = [
        (1600, [0, 0, 0], [1600, 3200, 4800], 2, b"groups"),            # group_cap too small
        (1600, [0, 0], [1600, 3200], 0, b"groups"),
        (1600, [0, 1600], [1, 1], 64, b"pending[1]"),                   # pending outside [0, in_block)
        (1600, [0, -1], [1, 1], 64, b"pending[1]"),
        (1600, [0, 0, 0], [1, -1, 1], 64, b"counts[1]"),                # a negative count
        (1600, [0, 0, 0], [1, 1, 64 * 1600 + 1], 64, b"counts[2]"),     # a count over the maximum
        (0, [0], [1], 64, b"in_block"),
    ]
    for in_block, pending, counts, cap, word in bad:
        rc, ticks, new, order, nt, gt, gf, ng = plan(in_block, pending, counts, cap)
        assert rc == _lib.EWK_EINVAL
        assert word in _lib.load().ewk_last_error(), _lib.load().ewk_last_error()
        for a in (ticks, new, order, gt, gf):
            assert (a == -7).all()
        assert nt == -7 and ng == -7


MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "%s"
// stdin: per case "in_block n group_cap", n pending values, n counts.  stdout: per case the
// return code and, when 0, n_ticking n_groups, ticks, new_pending, order, group_ticks, group_first.
int main() {
    int in_block, n, cap;
    while (scanf("%%d %%d %%d", &in_block, &n, &cap) == 3) {
        // exact sizes, so the sanitizer sees any access past what the call is entitled to
        std::vector<int32_t> pending(n), counts(n), ticks(n), np(n), order(n), gt(cap), gf(cap + 1);
        for (int i = 0; i < n; ++i) if (scanf("%%d", &pending[i]) != 1) return 2;
        for (int i = 0; i < n; ++i) if (scanf("%%d", &counts[i]) != 1) return 2;
        int32_t nt = -1, ng = -1, bad = -1;
        int rc = (int)ewk::chunk_plan(in_block, n, pending.data(), counts.data(), ticks.data(), np.data(), order.data(),
                                      &nt, gt.data(), gf.data(), cap, &ng, &bad);
        printf("%%d", rc);
        if (rc == 0) {
            printf(" %%d %%d", nt, ng);
            for (int i = 0; i < n; ++i) printf(" %%d", ticks[i]);
            for (int i = 0; i < n; ++i) printf(" %%d", np[i]);
            for (int i = 0; i < nt; ++i) printf(" %%d", order[i]);
            for (int i = 0; i < ng; ++i) printf(" %%d", gt[i]);
            for (int i = 0; i <= ng; ++i) printf(" %%d", gf[i]);
        }
        printf("\n");
        // the layout of the planned push, a line "L unit total src_at[n] asm_total group_base[ng]" per unit
        const int units[2] = {8, 16};
        for (int u = 0; rc == 0 && u < 2; ++u) {
            std::vector<int64_t> src_at(n), base(ng);
            long long total = ewk::chunk_stage_layout(units[u], n, pending.data(), counts.data(), src_at.data());
            long long rows = ewk::chunk_row_layout(units[u], in_block, ng, gt.data(), gf.data(), base.data());
            printf("L %%d %%lld", units[u], total);
            for (int i = 0; i < n; ++i) printf(" %%lld", (long long)src_at[i]);
            printf(" %%lld", rows);
            for (int i = 0; i < ng; ++i) printf(" %%lld", (long long)base[i]);
            printf("\n");
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def standalone(tmp_path_factory):
    """The header alone, in a program with its own main, built with the address and undefined-
    behaviour sanitizers, run once over the cases (group_cap cut to what each needs, so every array
    has its exact size): (todo, the plan line of each, the layout lines of those that fit)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp_path = tmp_path_factory.mktemp("plan")
    src = tmp_path / "plan_main.cpp"
    src.write_text(MAIN % HDR)
    exe = tmp_path / "plan_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(src), "-o", str(exe)], check=True)
    todo, lines = [], []
    for in_block, pending, counts, cap in cases():
        need = len(model(in_block, pending, counts)[3])
        for c in {need, max(need - 1, 0)}:          # exactly enough, and one too few
            todo.append((in_block, pending, counts, c, c >= need))
            lines.append(" ".join(map(str, [in_block, len(pending), c, *pending, *counts])))
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""
    out = r.stdout.strip().split("\n")
    return todo, [x for x in out if not x.startswith("L")], [x for x in out if x.startswith("L")]


def test_standalone_program_under_sanitizers(standalone):
    """The same cases, the same answers, no report."""
    todo, out, _ = standalone
    assert len(out) == len(todo)
    for (in_block, pending, counts, cap, fits), line in zip(todo, out):
        v = np.array(line.split(), np.int64)
        if not fits:
            assert v.tolist() == [4]                 # kChunkPlanGroups, nothing else
            continue
        n = len(pending)
        rc, nt, ng = v[:3]
        assert rc == 0
        rest = v[3:]
        ticks, new, order = rest[:n], rest[n:2 * n], rest[2 * n:2 * n + nt]
        gt, gf = rest[2 * n + nt:2 * n + nt + ng], rest[2 * n + nt + ng:]
        assert len(gf) == ng + 1
        m_ticks, m_new, m_order, m_gt, m_first = model(in_block, pending, counts)
        np.testing.assert_array_equal(ticks, m_ticks)
        np.testing.assert_array_equal(new, m_new)
        np.testing.assert_array_equal(order, m_order)
        np.testing.assert_array_equal(gt, m_gt)
        np.testing.assert_array_equal(gf, m_first)


def test_layouts_under_sanitizers(standalone):
    """chunk_stage_layout and chunk_row_layout for every planned case and both units: equal to the
    numpy models, and the properties the assembly kernel and the gate rely on, on their own."""
    todo, _, lines = standalone
    fitting = [t for t in todo if t[4]]
    assert len(lines) == len(UNITS) * len(fitting)
    for k, (in_block, pending, counts, cap, _) in enumerate(fitting):
        n = len(pending)
        p, c = np.asarray(pending, np.int64), np.asarray(counts, np.int64)
        _, _, _, m_gt, m_first = model(in_block, pending, counts)
        ng = len(m_gt)
        for u, unit in enumerate(UNITS):
            word = lines[len(UNITS) * k + u].split()
            v = np.array(word[1:], np.int64)
            assert word[0] == "L" and v[0] == unit and len(v) == 2 + n + 1 + ng
            total, src_at, asm_total, base = int(v[1]), v[2:2 + n], int(v[2 + n]), v[3 + n:]
            m_src, m_total = stage_model(unit, pending, counts)
            np.testing.assert_array_equal(src_at, m_src)
            assert total == m_total
            m_base, m_asm = row_model(unit, in_block, m_gt, m_first)
            np.testing.assert_array_equal(base, m_base)
            assert asm_total == m_asm
            # the staged chunks: in phase with the samples they follow, in call order, not overlapping
            full = np.flatnonzero(c)
            assert (src_at[c == 0] == 0).all()
            assert (src_at[full] % unit == p[full] % unit).all()
            assert (src_at[full][1:] >= (src_at[full] + c[full])[:-1]).all() and (src_at[full] >= 0).all()
            assert total == (src_at[full[-1]] + c[full[-1]] if len(full) else 0)
            assert total <= c.sum() + 2 * unit * n
            # the tick rows: every group aligned, the groups not overlapping, the total their end
            size = np.diff(m_first) * m_gt * in_block
            assert (base % unit == 0).all() and (base >= 0).all()
            assert (base[1:] >= (base + size)[:-1]).all()
            assert asm_total == (base[-1] + size[-1] if ng else 0)
