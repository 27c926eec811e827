// ewk_gate_tree.h -- numpy's pairwise summation order, flattened on the host (no HIP: a host
// compiler can include this file alone).
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace ewk {

// numpy's pairwise summation order (np.add.reduce on a contiguous float64 array,
// numpy/_core/src/umath/loops_utils.h.src pairwise_sum) for ONE chunk of n <= 8192
// elements, flattened on the host: leaves of <= 128 elements (8-accumulator loop),
// and the internal nodes grouped by height so a wave evaluates each level in parallel.
// Node ids: leaves 0..n_leaves-1, internal node k has id n_leaves + k.
constexpr int kPwChunk = 8192;
constexpr int kPwMaxLeaves = 256;
constexpr int kPwMaxLevels = 16;
struct PwTree {
    int32_t n;
    int32_t n_leaves;
    int32_t n_levels;
    int32_t balanced;   // 1: 2^d <= 16 leaves of one length >= 8, combined pairwise in leaf order (tree_sumsq's register path)
    int16_t leaf_start[kPwMaxLeaves];
    int16_t leaf_len[kPwMaxLeaves];
    int16_t left[kPwMaxLeaves];     // internal node k = val[left[k]] + val[right[k]]
    int16_t right[kPwMaxLeaves];
    int16_t level_end[kPwMaxLevels];   // internal nodes of height h+1: [level_end[h-1], level_end[h])
};
// The gate's summation lengths: the callback block (frame_size) and the last 0.1 s,
// each as a full-chunk tree (n = 8192, used when the length exceeds one chunk) and
// the tree of the final (or only) chunk.
enum { kTreeBlockFull = 0, kTreeBlockRem = 1, kTreeLastFull = 2, kTreeLastRem = 3, kNumTrees = 4 };

// ---- host: flatten numpy's pairwise recursion for one chunk --------------------
inline int split_point(int n) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    return n2;
}

inline void build_pw_tree(int n, PwTree* t) {
    memset(t, 0, sizeof(*t));
    t->n = n;
    if (n <= 0) return;
    struct Node { int a, b, h; };   // children as tagged ids: >= 0 leaf, < 0 internal (-1 - index)
    std::vector<Node> inner;
    int nleaf = 0;
    // returns tagged id and height
    struct R { int id, h; };
    auto rec = [&](auto&& self, int s, int m) -> R {
        if (m <= 128) {
            t->leaf_start[nleaf] = (int16_t)s;
            t->leaf_len[nleaf] = (int16_t)m;
            return R{nleaf++, 0};
        }
        const int n2 = split_point(m);
        const R a = self(self, s, n2);
        const R b = self(self, s + n2, m - n2);
        inner.push_back(Node{a.id, b.id, std::max(a.h, b.h) + 1});
        return R{-1 - (int)(inner.size() - 1), std::max(a.h, b.h) + 1};
    };
    rec(rec, 0, n);
    t->n_leaves = nleaf;
    // order internal nodes by height (children always lower), keep creation order within a level
    std::vector<int> order(inner.size());
    for (size_t i = 0; i < inner.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return inner[x].h < inner[y].h; });
    std::vector<int> pos(inner.size());
    for (size_t k = 0; k < order.size(); ++k) pos[order[k]] = (int)k;
    auto node_id = [&](int tag) { return tag >= 0 ? tag : nleaf + pos[-1 - tag]; };
    int levels = 0;
    for (size_t k = 0; k < order.size(); ++k) {
        const Node& nd = inner[order[k]];
        t->left[k] = (int16_t)node_id(nd.a);
        t->right[k] = (int16_t)node_id(nd.b);
        t->level_end[nd.h - 1] = (int16_t)(k + 1);
        levels = nd.h;
    }
    t->n_levels = levels;
    // balanced: every level pairs the previous level's nodes in order (node 2k with 2k + 1),
    // there are 2^d <= 16 leaves and each has >= 8 elements (1,600: 16 leaves of 96 / 104)
    bool bal = nleaf >= 1 && nleaf <= 16 && (nleaf & (nleaf - 1)) == 0;
    for (int l = 0; bal && l < nleaf; ++l) bal = t->leaf_len[l] >= 8;
    int first = 0, cnt = nleaf, k = 0;   // level h's nodes: ids [first, first + cnt)
    for (int h = 0; bal && h < levels; ++h) {
        for (int q = 0; bal && q < cnt / 2; ++q, ++k)
            bal = t->left[k] == first + 2 * q && t->right[k] == first + 2 * q + 1 && k < t->level_end[h];
        bal = bal && k == t->level_end[h];
        first = h == 0 ? nleaf : first + cnt;
        cnt /= 2;
    }
    t->balanced = bal && cnt == 1;
}

// How tree_sumsq evaluates a PwTree: 0 = one leaf of fewer than 8 elements (a plain loop), 1 = one
// leaf (8 accumulators), 2 = balanced (DPP, no LDS), 3 = the general LDS tree.
inline int pw_tree_kind(const PwTree& t) {
    if (t.n_leaves <= 1) return t.n < 8 ? 0 : 1;
    return t.balanced ? 2 : 3;
}

}  // namespace ewk
