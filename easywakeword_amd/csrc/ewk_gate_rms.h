// ewk_gate_rms.h -- the block RMS multiset of a stream and its sorted copy, in global memory or
// in registers, and the percentile read from it (included by ewk_gate.hip).
#pragma once

#include "ewk_gate_pwsum.h"

namespace ewk {

// First fill: rank-sort v (global, nb values) into dst (global).
__device__ void rank_sort(const double* v, double* dst, int nb, int lane) {
    for (int i = lane; i < nb; i += 64) {
        const double x = v[i];
        int r = 0;
        for (int k = 0; k < nb; ++k) {
            const double y = v[k];
            r += (y < x) || (y == x && k < i);
        }
        dst[r] = x;
    }
}

// src (sorted) with one occurrence of vo replaced by vn -> dst (sorted).
// Returns false when vo is absent (cache inconsistent: caller re-sorts).
__device__ bool sorted_replace(const double* src, double* dst, int nb, double vo, double vn, int lane) {
    int pos = nb;
    for (int i = lane; i < nb; i += 64)
        if (src[i] == vo) { pos = i; break; }
    for (int m = 1; m < 64; m <<= 1) pos = min(pos, __shfl_xor(pos, m, 64));
    if (pos >= nb) return false;
    int cnt = 0;
    for (int i = lane; i < nb; i += 64) cnt += (i != pos && src[i] < vn) ? 1 : 0;
    for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m, 64);
    for (int i = lane; i < nb; i += 64) {
        if (i == pos) continue;
        const int i1 = i < pos ? i : i - 1;
        dst[i1 < cnt ? i1 : i1 + 1] = src[i];
    }
    if (lane == 0) dst[cnt] = vn;
    return true;
}

// numpy.percentile(v, 25) ("linear") of nb values; get(i) reads element i of the sorted copy.
template <typename Get>
__device__ __forceinline__ double percentile25(const Get& get, int nb) {
    // virtual index = n*q + (alpha + q*(1-alpha-beta)) - 1, alpha = beta = 1, q = 0.25
    const double q = 0.25;
    const double vi = (double)nb * q + (1.0 + q * (1.0 - 1.0 - 1.0)) - 1.0;
    const double prevd = floor(vi);
    int prev = (int)prevd, next = prev + 1;
    if (vi >= (double)(nb - 1)) { prev = nb - 1; next = nb - 1; }
    if (vi < 0.0) { prev = 0; next = 0; }
    const double gamma = vi - prevd;
    const double a = get(prev), b = get(next);
    // numpy _lerp: a + (b-a)*t, replaced by b - (b-a)*(1-t) where t >= 0.5
    const double d = b - a;
    double r = a + d * gamma;
    if (gamma >= 0.5) r = b - d * (1.0 - gamma);
    return r;
}

// ---- register-resident block RMS multiset (n_blocks <= 64 * RB) ------------------
// Element i of a per-stream array lives in lane i % 64, slot i / 64.
template <int RB>
__device__ __forceinline__ double reg_get(const double (&v)[RB], int i) {
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < RB; ++j)
        if ((i >> 6) == j) r = __shfl(v[j], i & 63, 64);
    return r;
}

template <int RB>
__device__ __forceinline__ void reg_set(double (&v)[RB], int i, double x, int lane, uint32_t& dirty) {
#pragma unroll
    for (int j = 0; j < RB; ++j)
        if ((i >> 6) == j && lane == (i & 63)) { v[j] = x; dirty |= 1u << j; }
}

// so (sorted, nb values) with one occurrence of vo replaced by vn, kept sorted: the
// new element d comes from old element d - 1, d or d + 1 (or is vn), so the update is
// two neighbour shuffles.  Returns false when vo is absent (caller re-sorts).
template <int RB>
__device__ bool reg_replace(double (&so)[RB], int nb, double vo, double vn, int lane, uint32_t& dirty) {
    int pos = nb;
#pragma unroll
    for (int j = RB - 1; j >= 0; --j) {
        const unsigned long long m = __ballot(lane + 64 * j < nb && so[j] == vo);
        if (m) pos = 64 * j + __ffsll((long long)m) - 1;
    }
    if (pos >= nb) return false;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int i = lane + 64 * j;
        cnt += __popcll(__ballot(i < nb && i != pos && so[j] < vn));
    }
    double prev[RB], next[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const double up = __shfl(so[j], (lane + 63) & 63, 64);    // element d - 1 (lane 0: slot j-1's lane 63)
        const double dn = __shfl(so[j], (lane + 1) & 63, 64);     // element d + 1 (lane 63: slot j+1's lane 0)
        prev[j] = up;
        next[j] = dn;
    }
    // the cross-slot neighbours for lane 0 / lane 63 (wave-uniform shuffles)
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const double tail = j > 0 ? __shfl(so[j - 1], 63, 64) : 0.0;
        const double head = j + 1 < RB ? __shfl(so[j + 1], 0, 64) : 0.0;
        if (lane == 0) prev[j] = tail;
        if (lane == 63) next[j] = head;
    }
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int d = lane + 64 * j;
        const int i1 = d < cnt ? d : d - 1;
        const int i = i1 < pos ? i1 : i1 + 1;
        const double x = i == d ? so[j] : (i < d ? prev[j] : next[j]);
        so[j] = d == cnt ? vn : x;
        if (d >= min(pos, cnt) && d <= max(pos, cnt)) dirty |= 1u << (RB + j);   // elements that moved
    }
    return true;
}

// First fill / repair: so = sorted copy of gr (stable rank sort through LDS scratch tmp[nb]).
template <int RB>
__device__ void reg_rank_sort(const double (&gr)[RB], double (&so)[RB], int nb, double* tmp, int lane, uint32_t& dirty) {
    dirty |= ((1u << RB) - 1) << RB;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int i = lane + 64 * j;
        const double x = gr[j];
        int r = 0;
#pragma unroll
        for (int jj = 0; jj < RB; ++jj)
            for (int kk = 0; kk < 64; ++kk) {
                const int k = 64 * jj + kk;
                const double y = __shfl(gr[jj], kk, 64);
                r += k < nb && ((y < x) || (y == x && k < i));
            }
        if (i < nb) tmp[r] = x;
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int i = lane + 64 * j;
        so[j] = i < nb ? tmp[i] : 0.0;
    }
    wave_sync();
}

}  // namespace ewk
