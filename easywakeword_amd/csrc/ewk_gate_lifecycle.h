// ewk_gate_lifecycle.h -- the kernels around the gate that are not the gate: re-entry, listener
// tables, ring and stream resets, index scatter; with their launchers (ewk_gate.h declares them).
// Included by ewk_gate.hip alone, after k_gate_ticks.
#pragma once

#include <algorithm>

#include "ewk_gate.h"

namespace ewk {

// _detect_word entry (wakeword.py:1048-1057) for streams whose detection runs: state from
// the current is_silent(), start_time = now.  Streams still filling their ring are left
// alone (their entry happens in k_gate_ticks when the ring first fills).
__global__ void k_reenter(GateStream* st, int32_t first, int32_t n, double tick_seconds, const int32_t* lsn_count,
                          LsnState* lsn_st) {
    const int i = first + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= first + n) return;
    GateStream s = st[i];
    if (!s.started) return;
    const double now = (double)s.tick * tick_seconds;
    s.state = s.last_silent ? kInSilence : kWaiting;
    if (s.last_silent) s.silence_start = now;
    s.start_time = now;
    st[i] = s;
    if (!lsn_count) return;
    const int cnt = min(lsn_count[i], (int)EWK_LISTENERS_MAX);
    for (int j = 1; j < cnt; ++j) {   // every listener of the stream: the same entry
        LsnState* l = lsn_st + (int64_t)i * kLsnStates + j - 1;
        l->state = s.state;
        if (s.last_silent) l->silence_start = now;
        l->start_time = now;
    }
}

// ewk_stream_listeners_set: thread (i, j) handles listener j of stream ids[i] (16 threads per
// stream, 16 streams per workgroup).  A listener at or past the stream's old count is new and
// starts as k_reenter starts listener 0 (a stream still filling its ring: zeros, it enters when
// the ring fills); one at or past the new count is dropped and zeroed.
__global__ __launch_bounds__(256) void k_listeners_set(const ListenerSetArgs a) {
    const int i = (int)(blockIdx.x * 16 + (threadIdx.x >> 4)), j = (int)(threadIdx.x & 15);
    const bool in = i < a.n;
    const int64_t sid = in ? a.ids[i] : 0;
    const int newc = in ? a.counts[i] : 0;
    const int oldc = in ? a.lsn_count[sid] : 0;
    __syncthreads();   // every thread of the stream has read the old count
    if (!in) return;
    const ewk_listener row = j < newc ? a.rows[(int64_t)i * EWK_LISTENERS_MAX + j] : ewk_listener{-1, 0};
    a.lsn_tab[sid * EWK_LISTENERS_MAX + j] = row;
    if (j == 0) {
        a.lsn_count[sid] = newc;
        if (a.stream_profile) a.stream_profile[sid] = row.profile;
        if (a.stream_word) a.stream_word[sid] = row.word;
        return;
    }
    if (j < newc && j < oldc) return;   // an existing listener keeps its state
    LsnState z = {};
    if (j < newc) {
        const GateStream g = a.st[sid];
        if (g.started) {
            const double now = (double)g.tick * a.tick_seconds;
            z.state = g.last_silent ? kInSilence : kWaiting;
            if (g.last_silent) z.silence_start = now;
            z.start_time = now;
        }
    }
    a.lsn_st[sid * kLsnStates + j - 1] = z;
}

hipError_t launch_listeners_set(const ListenerSetArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (!a.ids || !a.counts || !a.rows || !a.lsn_count || !a.lsn_tab || !a.lsn_st || !a.st) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_listeners_set, dim3((a.n + 15) / 16), dim3(256), 0, s, a);
    return hipGetLastError();
}

// Ring initialisation (ewk_reset_streams).  Round 6's recording build caught the ring scorer
// reading four 128-B lines of ZEROS -- the ring's initial fill -- where the gate had written
// samples twice since ("The ring-path miss recurred"); the fill used
// hipMemsetAsync.  Here every line is written by an agent-scope store (global_store sc1:
// performed at memory, not kept in the XCD's L2), 8 B per lane.
__global__ void k_ring_zero(uint64_t* p, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x)
        __hip_atomic_store(p + i, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
hipError_t launch_ring_zero(void* p, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    if (bytes % 8 || ((uintptr_t)p & 7)) return hipErrorInvalidValue;
    const size_t n8 = bytes / 8;
    const unsigned grid = (unsigned)std::min<size_t>(4096, (n8 + 255) / 256);
    hipLaunchKernelGGL(k_ring_zero, dim3(grid), dim3(256), 0, s, static_cast<uint64_t*>(p), n8);
    return hipGetLastError();
}

// ewk_reset_stream_list: workgroup (i, c) zeroes piece c of stream ids[i]'s ring row with the
// stores of k_ring_zero (for its reason); piece 0 also clears the block RMS row, the state, the
// resampler history row and sets the fresh flag.  A row starts at a multiple of the sample size
// only, so the bytes before the first and after the last 8-byte boundary go in 2-byte stores.
constexpr int kResetPiece = 32768;   // ring bytes per workgroup
__global__ __launch_bounds__(256) void k_reset_list(const ResetListArgs a, const int32_t pieces) {
    const int i = (int)(blockIdx.x / (uint32_t)pieces), c = (int)(blockIdx.x % (uint32_t)pieces);
    const int64_t sid = a.ids[i];
    const uintptr_t b0 = (uintptr_t)(a.ring + sid * a.row_bytes), b1 = b0 + (uintptr_t)a.row_bytes;
    const uintptr_t up0 = (b0 + 7) & ~(uintptr_t)7, dn1 = b1 & ~(uintptr_t)7;
    const uintptr_t a0 = up0 < b1 ? up0 : b1, a1 = dn1 > a0 ? dn1 : a0;   // [a0, a1): the whole 8-byte words
    {
        const uintptr_t p0 = a0 + (uintptr_t)c * kResetPiece, p1 = p0 + kResetPiece < a1 ? p0 + kResetPiece : a1;
        for (uintptr_t p = p0 + 8 * (uintptr_t)threadIdx.x; p < p1; p += 8 * 256)
            __hip_atomic_store(reinterpret_cast<uint64_t*>(p), (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (c != 0) return;
    {   // (fewer than 4 + 4 two-byte pieces)
        const uintptr_t p = threadIdx.x < 4 ? b0 + 2 * (uintptr_t)threadIdx.x : a1 + 2 * ((uintptr_t)threadIdx.x - 4);
        const bool in = threadIdx.x < 4 ? p < a0 : (threadIdx.x < 8 && p < b1);
        if (in) __hip_atomic_store(reinterpret_cast<uint16_t*>(p), (uint16_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int k = threadIdx.x; k < a.n_blocks; k += blockDim.x) a.block_rms[sid * a.n_blocks + k] = 0.0;
    if (a.hist)
        for (int k = threadIdx.x; k < a.H; k += blockDim.x) a.hist[sid * a.H + k] = 0.0f;
    if (a.lsn_st && threadIdx.x < kLsnStates) a.lsn_st[sid * kLsnStates + threadIdx.x] = LsnState{};
    if (threadIdx.x == 0) {
        GateStream z = {};   // (ewk_reset_streams' initial state)
        z.threshold = a.init_threshold;
        z.last_silent = 1;
        a.st[sid] = z;
        if (a.fresh) a.fresh[sid] = 1;
    }
}

hipError_t launch_reset_list(const ResetListArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.row_bytes % 2 || ((uintptr_t)a.ring & 7)) return hipErrorInvalidValue;
    const int64_t pieces = std::max<int64_t>(1, (a.row_bytes + kResetPiece - 1) / kResetPiece);
    if (pieces * a.n > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_reset_list, dim3((unsigned)(pieces * a.n)), dim3(256), 0, s, a, (int32_t)pieces);
    return hipGetLastError();
}

__global__ void k_scatter_i32(int32_t* dst, const int32_t* ids, const int32_t* vals, int32_t n) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) dst[ids[i]] = vals[i];
}

hipError_t launch_scatter_i32(int32_t* dst, const int32_t* ids, const int32_t* vals, int32_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_i32, dim3((n + 255) / 256), dim3(256), 0, s, dst, ids, vals, n);
    return hipGetLastError();
}

hipError_t launch_reenter(GateStream* st, int32_t first, int32_t n, double tick_seconds, const int32_t* lsn_count,
                          LsnState* lsn_st, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if ((lsn_count == nullptr) != (lsn_st == nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_reenter, dim3((n + 255) / 256), dim3(256), 0, s, st, first, n, tick_seconds, lsn_count, lsn_st);
    return hipGetLastError();
}

}  // namespace ewk
