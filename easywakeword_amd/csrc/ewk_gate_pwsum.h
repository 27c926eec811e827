// ewk_gate_pwsum.h -- device sums of squares in numpy's pairwise order (included by ewk_gate.hip
// under its `fp contract(off)`).
#pragma once

#include "ewk_gate.h"

namespace ewk {

// The lane index through an empty asm: values derived from it (per-lane offsets) are then
// computed where they are used instead of being hoisted out of the stream loop and kept live
// (or spilled) across everything in between.
__device__ __forceinline__ int lane_here(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}
__device__ __forceinline__ void wave_sync() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

struct LdsSrc {
    const float* p;
    __device__ __forceinline__ float operator()(int i) const { return p[i]; }
};

// the int16 stage of the vector int16 path (DMA 3): the PCM16 value / 32768, exactly the float
// the float stage held (half the LDS: five workgroups of four waves fit a CU)
struct LdsSrc16 {
    const int16_t* p;
    __device__ __forceinline__ float operator()(int i) const { return (float)p[i] * (1.0f / 32768.0f); }
};

struct RingSrc {
    const float* ring;
    const int16_t* ring16;   // int16 ring (EWK_RING_I16) when set: value = x / 32768, exact
    int32_t first;   // physical index of element 0
    int32_t R;
    __device__ __forceinline__ float operator()(int i) const {
        int k = first + i;
        if (k >= R) k -= R;
        return ring16 ? (float)ring16[k] * (1.0f / 32768.0f) : ring[k];
    }
};

// DPP / permlane helpers for doubles (wave-uniform control)
template <int CTRL, int BANKS>
__device__ __forceinline__ double dpp_mov_d(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, BANKS, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, BANKS, false);
    return __hiloint2double(hi, lo);
}
// the value of lane ^ 16 (rows 0 <-> 1, 2 <-> 3) / lane ^ 32 (rows 0, 1 <-> 2, 3)
template <int W>
__device__ __forceinline__ double swap_rows_d(double x, int lane) {
    const uint32_t lo = (uint32_t)__double2loint(x), hi = (uint32_t)__double2hiint(x);
    const auto rl = W == 16 ? __builtin_amdgcn_permlane16_swap(lo, lo, false, false)
                            : __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto rh = W == 16 ? __builtin_amdgcn_permlane16_swap(hi, hi, false, false)
                            : __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    // (vdst, vsrc) = (x, x): the upper half of each pair finds the partner in vdst, the lower in vsrc
    const bool upper = (lane & W) != 0;
    return __hiloint2double((int)(upper ? rh[0] : rh[1]), (int)(upper ? rl[0] : rl[1]));
}

// A balanced chunk (build_pw_tree: 2^d <= 16 leaves of >= 8 elements, paired in order) without LDS:
// lane = leaf % 8 * 8 + j runs accumulator j of leaf (leaf % 8) + 8 s for s = 0, 1 (numpy's
// r[j] += x[i + j]^2, i = 8, 16, ...); the eight accumulators combine as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) by DPP exchanges (lane ^ 1, ^ 2, 7 - lane
// within eight: every lane of the eight then holds the same bits, a + b == b + a), the tail
// elements are added in order, and the leaves pair in order across lane groups (row_ror:8,
// rows ^ 1, rows ^ 2, then set 0 + set 1) -- numpy's additions, operand for operand.
template <typename Src>
__device__ double tree_sumsq_bal(const Src& src, const PwTree* t, int lane) {
    const int L = t->n_leaves;
    const int j = lane & 7, li = lane >> 3;
    double tot[2] = {0.0, 0.0};
#pragma unroll
    for (int set = 0; set < 2; ++set) {
        if (8 * set >= L) break;   // (wave-uniform)
        const int l = li + 8 * set < L ? li + 8 * set : 0;   // (lanes past the last leaf: a copy of leaf 0, unused)
        const int s0 = t->leaf_start[l], m = t->leaf_len[l], m8 = m - m % 8;
        double r;
        { const double x = src(s0 + j); r = x * x; }
        for (int i = 8; i < m8; i += 8) { const double x = src(s0 + i + j); r += x * x; }
        r = r + dpp_mov_d<0xB1, 0xf>(r);   // quad_perm [1,0,3,2]: lane ^ 1
        r = r + dpp_mov_d<0x4E, 0xf>(r);   // quad_perm [2,3,0,1]: lane ^ 2
        r = r + dpp_mov_d<0x141, 0xf>(r);  // row_half_mirror: 7 - lane within eight
        for (int i = m8; i < m; ++i) { const double x = src(s0 + i); r += x * x; }
        // leaves of this set: pairs (row_ror:8), then rows ^ 1, rows ^ 2
        if (L > 1) r = r + dpp_mov_d<0x128, 0xf>(r);   // row_ror:8
        if (L > 2) r = r + swap_rows_d<16>(r, lane);
        if (L > 4) r = r + swap_rows_d<32>(r, lane);
        tot[set] = r;
    }
    // lane 0 holds its set's sum (for fewer than 8 leaves the rows past them hold copies of leaf
    // 0); for 16 leaves the root adds the two halves in order.  Broadcast: a uniform result.
    const double res = L > 8 ? tot[0] + tot[1] : tot[0];
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(res)),
                            __builtin_amdgcn_readfirstlane(__double2loint(res)));
}

// One chunk (n = t->n elements of src) in numpy's pairwise order, wave-parallel.
// val: per-wave LDS scratch of 10 * n_leaves doubles (node values, then the leaves'
// 8 accumulators).  Each accumulator chain of a leaf runs on its own lane (numpy's
// r[j] += x[i + j]^2, i = 8, 16, ...), a second step combines the eight in numpy's
// order and adds the < 8 tail elements -- the additions of numpy's loop over one leaf.
// Uniform result.
template <typename Src>
__device__ double tree_sumsq(const Src& src, const PwTree* t, int lane, double* val) {
    if (t->balanced) return tree_sumsq_bal(src, t, lane);   // (the default 1,600-sample block: 16 leaves)
    const int L = t->n_leaves;
    double* acc8 = val + 2 * L;
    for (int q = lane; q < 8 * L; q += 64) {
        const int l = q >> 3, j = q & 7;
        const int s0 = t->leaf_start[l], n = t->leaf_len[l];
        if (n >= 8) {
            double r;
            { const double x = src(s0 + j); r = x * x; }
            const int lim = n - (n % 8);
            for (int i = 8; i < lim; i += 8) { const double x = src(s0 + i + j); r += x * x; }
            acc8[q] = r;
        }
    }
    wave_sync();
    for (int l = lane; l < L; l += 64) {
        const int s0 = t->leaf_start[l], n = t->leaf_len[l];
        double res;
        if (n < 8) {
            res = 0.0;
            for (int i = 0; i < n; ++i) { const double x = src(s0 + i); res += x * x; }
        } else {
            const double* r = acc8 + 8 * l;
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (int i = n - (n % 8); i < n; ++i) { const double x = src(s0 + i); res += x * x; }
        }
        val[l] = res;
    }
    wave_sync();
    int b = 0;
    for (int h = 0; h < t->n_levels; ++h) {
        const int e = t->level_end[h];
        for (int k = b + lane; k < e; k += 64) val[L + k] = val[t->left[k]] + val[t->right[k]];
        b = e;
        wave_sync();
    }
    const double r = (L == 1) ? val[0] : val[L + b - 1];   // the root is the last internal node
    wave_sync();
    return r;
}

// np.add.reduce(x**2) over n samples: chunks of 8192 accumulated from 0.0.
template <typename MakeSrc>
__device__ double pw_sumsq(const MakeSrc& make, int n, const PwTree* full, const PwTree* rem, int lane,
                           double* val) {
    double acc = 0.0;
    for (int c0 = 0; c0 < n; c0 += kPwChunk) {
        // (unused, and kept: without this line all 27 k_gate_ticks come out with other instructions)
        [[maybe_unused]] const int cn = min(kPwChunk, n - c0);
        // the final (or only) chunk has its own tree, also when it is a whole chunk: n == kPwChunk
        // has no full-chunk tree at all (ewk_create builds that one for n > kPwChunk only)
        acc += tree_sumsq(make(c0), c0 + kPwChunk < n ? full : rem, lane, val);   // (full->n == kPwChunk)
    }
    return acc;
}

}  // namespace ewk
