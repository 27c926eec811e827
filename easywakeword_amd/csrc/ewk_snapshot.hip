// ewk_snapshot.hip -- stream snapshots: gathering listed streams into records and scattering
// records back (ewk_export_streams / ewk_import_streams; the record format is in include/ewk.h
// and ewk_snapshot_plan.h).
//
// Both kernels are pure data movement, 99.5 % of it the ring row.  The geometry is k_reset_list's:
// workgroup (i, c) moves piece c (kSnapPiece bytes) of stream ids[i]'s ring row, and piece 0 also
// moves the small sections, as 8-, 4- or 2-byte words spread over its threads.
//
// The record side of the ring section is 16-byte aligned by construction; the ring side of a row
// starts at a multiple of the sample size only (an int16 ring of an odd number of samples per
// row).  A copy is cut at the DESTINATION's 16-byte boundaries: a head and a tail of fewer than
// eight 2-byte pieces each, and between them 16-byte stores whose 16 source bytes come from one
// 16-byte load where the source is aligned there too, else from 8-, 4- or 2-byte loads according
// to the phase between the two sides.
//
// Unpack writes the ring row with agent-scope stores (sc1: performed at memory, the line is not
// kept in the writing XCD's L2), as k_ring_zero and k_reset_list do and for k_ring_zero's reason:
// no cached copy of a ring line's first fill may outlive the gate's later plain writes to it.
// 16 bytes per lane as global_store_dwordx4 sc1 (clang has no 16-byte atomic store; with
// -DEWK_SNAPSHOT_STORE8 two 8-byte __hip_atomic_store instead, for the A/B of
// scripts/bench_stream_snapshot.py).  Nothing is handed over inside a launch: no fences, no LDS.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <algorithm>

#include "ewk_snapshot.h"

namespace ewk {

constexpr int kSnapThreads = 256;
constexpr int kSnapPiece = 32768;   // ring bytes per workgroup (a multiple of 16)
constexpr int kGateWords = (int)(sizeof(GateStream) / 8);
constexpr int kLsnWords = (int)(kLsnStates * sizeof(LsnState) / 8);
constexpr int kLsnRowWords = (int)(sizeof(LsnState) / 8);
static_assert(sizeof(GateStream) == 96 && offsetof(GateStream, sorted_sel) == 88, "record layout (ewk_snapshot_plan.h)");
static_assert(sizeof(LsnState) == 40, "record layout (ewk_snapshot_plan.h)");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 16 bytes at p, which is aligned to `u` bytes (16, 8, 4 or 2)
__device__ __forceinline__ u32x4 load16(const unsigned char* p, int u) {
    u32x4 r;
    if (u >= 16) {
        r = *reinterpret_cast<const u32x4*>(p);
    } else if (u == 8) {
        const uint64_t* q = reinterpret_cast<const uint64_t*>(p);
        const uint64_t a = q[0], b = q[1];
        r = u32x4{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
    } else if (u == 4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        r = u32x4{q[0], q[1], q[2], q[3]};
    } else {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
        r = u32x4{q[0] | ((uint32_t)q[1] << 16), q[2] | ((uint32_t)q[3] << 16), q[4] | ((uint32_t)q[5] << 16),
                  q[6] | ((uint32_t)q[7] << 16)};
    }
    return r;
}

template <bool AGENT>
__device__ __forceinline__ void store16(uintptr_t p, u32x4 v) {
    if constexpr (!AGENT) {
        *reinterpret_cast<u32x4*>(p) = v;
    } else {
#ifndef EWK_SNAPSHOT_STORE8
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(reinterpret_cast<void*>(p)), "v"(v) : "memory");
#else
        __hip_atomic_store(reinterpret_cast<uint64_t*>(p), v.x | ((uint64_t)v.y << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<uint64_t*>(p) + 1, v.z | ((uint64_t)v.w << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
#endif
    }
}

template <bool AGENT>
__device__ __forceinline__ void store2(uintptr_t p, uint16_t v) {
    if constexpr (AGENT) __hip_atomic_store(reinterpret_cast<uint16_t*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *reinterpret_cast<uint16_t*>(p) = v;
}

// Piece c of dst[0, nbytes) = src[0, nbytes) (both 2-byte aligned, nbytes even) by the whole
// workgroup; piece 0 also copies the head and the tail.  Reads stay inside the source, writes
// inside the destination.
template <bool AGENT>
__device__ __forceinline__ void copy_row(unsigned char* dst, const unsigned char* src, int64_t nbytes, int c) {
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)nbytes;
    const uintptr_t up0 = (d0 + 15) & ~(uintptr_t)15, dn1 = d1 & ~(uintptr_t)15;
    const uintptr_t a0 = up0 < d1 ? up0 : d1, a1 = dn1 > a0 ? dn1 : a0;   // [a0, a1): the whole 16-byte words
    const unsigned char* sb = src + (a0 - d0);
    const int phase = (int)((uintptr_t)sb & 15);
    const int u = phase ? (phase & -phase) : 16;
    {
        const uintptr_t p0 = a0 + (uintptr_t)c * kSnapPiece, p1 = p0 + kSnapPiece < a1 ? p0 + kSnapPiece : a1;
        constexpr uintptr_t kStep = 16 * kSnapThreads;   // four loads in flight per lane before their stores
        for (uintptr_t p = p0 + 16 * (uintptr_t)threadIdx.x; p < p1; p += 4 * kStep) {
            u32x4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p + j * kStep < p1) v[j] = load16(sb + (p + j * kStep - a0), u);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p + j * kStep < p1) store16<AGENT>(p + j * kStep, v[j]);
        }
    }
    if (c != 0 || threadIdx.x >= 16) return;
    {   // (fewer than 8 + 8 two-byte pieces)
        const uintptr_t p = threadIdx.x < 8 ? d0 + 2 * (uintptr_t)threadIdx.x : a1 + 2 * ((uintptr_t)threadIdx.x - 8);
        const bool in = threadIdx.x < 8 ? p < a0 : p < d1;
        if (in) store2<AGENT>(p, *reinterpret_cast<const uint16_t*>(src + (p - d0)));
    }
}

// dst[k] = live ? src[k] : 0, k < n, by the whole workgroup (src may be nullptr when !live)
template <typename W>
__device__ __forceinline__ void copy_words(W* dst, const W* src, int32_t n, bool live) {
    for (int32_t k = (int32_t)threadIdx.x; k < n; k += kSnapThreads) dst[k] = live ? src[k] : (W)0;
}

__global__ __launch_bounds__(kSnapThreads) void k_snapshot_pack(const SnapArgs a, const int32_t pieces) {
    const int i = (int)(blockIdx.x / (uint32_t)pieces), c = (int)(blockIdx.x % (uint32_t)pieces);
    const int64_t sid = a.ids[i];
    unsigned char* rec = a.rec + (int64_t)i * a.record_bytes;
    copy_row<false>(rec + a.off[EWK_SNAP_RING], a.ring + sid * a.row_bytes, a.row_bytes, c);
    if (c != 0) return;
    const int tid = (int)threadIdx.x;
    const int nb = a.n_blocks;
    const GateStream* st = a.st + sid;
    const bool filled = st->filled != 0;
    const int sel = st->sorted_sel & 1;
    if (tid < kGateWords) {   // sorted_sel = 0: the record holds the current half as half 0
        uint64_t w = reinterpret_cast<const uint64_t*>(st)[tid];
        if (tid == (int)(offsetof(GateStream, sorted_sel) / 8)) w &= 0xffffffff00000000ULL;
        reinterpret_cast<uint64_t*>(rec + a.off[EWK_SNAP_GATE])[tid] = w;
    }
    if (tid < kLsnWords) {   // rows of listeners the stream does not have: zero
        const int cnt = (a.lsn_st && a.lsn_count) ? a.lsn_count[sid] : 1;
        const bool live = tid / kLsnRowWords < cnt - 1;
        reinterpret_cast<uint64_t*>(rec + a.off[EWK_SNAP_LISTENERS])[tid] =
            live ? reinterpret_cast<const uint64_t*>(a.lsn_st + sid * kLsnStates)[tid] : 0;
    }
    // block RMSs are valid once the ring has filled (a compact ring keeps them from the first
    // write), the sorted copy once it has filled
    copy_words(reinterpret_cast<uint64_t*>(rec + a.off[EWK_SNAP_BLOCK_RMS]),
               reinterpret_cast<const uint64_t*>(a.block_rms + sid * nb), nb, filled || a.compact);
    copy_words(reinterpret_cast<uint64_t*>(rec + a.off[EWK_SNAP_SORTED]),
               reinterpret_cast<const uint64_t*>(a.sorted_rms + (sid * 2 + sel) * nb), nb, filled);
    if (a.sec_bytes[EWK_SNAP_HISTORY] > 0) {
        copy_words(reinterpret_cast<uint32_t*>(rec + a.off[EWK_SNAP_HISTORY]),
                   reinterpret_cast<const uint32_t*>(a.hist + sid * a.H), a.H, a.hist != nullptr);
        if (tid < 4)
            reinterpret_cast<uint32_t*>(rec + a.off[EWK_SNAP_FRESH])[tid] =
                tid == 0 ? (uint32_t)((a.fresh ? a.fresh[sid] : a.fresh_all) != 0) : 0u;
    }
    {   // the carry: `pending` samples, zeros after them
        const int32_t pend = (a.pending && a.carry) ? a.pending[i] : 0;
        unsigned char* d = rec + a.off[EWK_SNAP_CARRY];
        const unsigned char* s = a.carry + sid * (int64_t)a.in_block * a.es;
        for (int32_t k = tid; k < a.in_block; k += kSnapThreads) {
            if (a.es == 2) reinterpret_cast<uint16_t*>(d)[k] = k < pend ? reinterpret_cast<const uint16_t*>(s)[k] : (uint16_t)0;
            else reinterpret_cast<uint32_t*>(d)[k] = k < pend ? reinterpret_cast<const uint32_t*>(s)[k] : 0u;
        }
    }
    // padding: behind every section up to the next one, and up to the end of the record
    for (int k = 0; k < EWK_SNAP_SECTIONS; ++k) {
        const int64_t end = a.off[k] + a.sec_bytes[k];
        const int64_t next = k + 1 < EWK_SNAP_SECTIONS ? a.off[k + 1] : a.record_bytes;
        for (int64_t j = end + 2 * tid; j < next; j += 2 * kSnapThreads) *reinterpret_cast<uint16_t*>(rec + j) = 0;
    }
}

__global__ __launch_bounds__(kSnapThreads) void k_snapshot_unpack(const SnapArgs a, const int32_t pieces) {
    const int i = (int)(blockIdx.x / (uint32_t)pieces), c = (int)(blockIdx.x % (uint32_t)pieces);
    const int64_t sid = a.ids[i];
    const unsigned char* rec = a.rec + (int64_t)i * a.record_bytes;
    copy_row<true>(a.ring + sid * a.row_bytes, rec + a.off[EWK_SNAP_RING], a.row_bytes, c);
    if (c != 0) return;
    const int tid = (int)threadIdx.x;
    const int nb = a.n_blocks;
    if (tid < kGateWords)
        reinterpret_cast<uint64_t*>(a.st + sid)[tid] = reinterpret_cast<const uint64_t*>(rec + a.off[EWK_SNAP_GATE])[tid];
    if (a.lsn_st && tid < kLsnWords)
        reinterpret_cast<uint64_t*>(a.lsn_st + sid * kLsnStates)[tid] =
            reinterpret_cast<const uint64_t*>(rec + a.off[EWK_SNAP_LISTENERS])[tid];
    copy_words(reinterpret_cast<uint64_t*>(a.block_rms + sid * nb),
               reinterpret_cast<const uint64_t*>(rec + a.off[EWK_SNAP_BLOCK_RMS]), nb, true);
    copy_words(reinterpret_cast<uint64_t*>(a.sorted_rms + sid * 2 * nb),   // half 0 (the record's sorted_sel is 0)
               reinterpret_cast<const uint64_t*>(rec + a.off[EWK_SNAP_SORTED]), nb, true);
    if (a.hist && a.sec_bytes[EWK_SNAP_HISTORY] > 0) {
        copy_words(reinterpret_cast<uint32_t*>(a.hist + sid * a.H),
                   reinterpret_cast<const uint32_t*>(rec + a.off[EWK_SNAP_HISTORY]), a.H, true);
        if (a.fresh && tid == 0)
            a.fresh[sid] = (uint8_t)(*reinterpret_cast<const uint32_t*>(rec + a.off[EWK_SNAP_FRESH]) != 0);
    }
    if (a.carry) {
        unsigned char* d = a.carry + sid * (int64_t)a.in_block * a.es;
        const unsigned char* s = rec + a.off[EWK_SNAP_CARRY];
        if (a.es == 2) copy_words(reinterpret_cast<uint16_t*>(d), reinterpret_cast<const uint16_t*>(s), a.in_block, true);
        else copy_words(reinterpret_cast<uint32_t*>(d), reinterpret_cast<const uint32_t*>(s), a.in_block, true);
    }
}

static hipError_t check_args(const SnapArgs& a, int64_t* pieces) {
    if (!a.ids || !a.rec || !a.ring || !a.st || !a.block_rms || !a.sorted_rms) return hipErrorInvalidValue;
    if (((uintptr_t)a.rec & 15) || a.record_bytes % 16 || a.row_bytes % 2 || ((uintptr_t)a.ring & 15))
        return hipErrorInvalidValue;
    if (a.es != 2 && a.es != 4) return hipErrorInvalidValue;
    for (int k = 0; k < EWK_SNAP_SECTIONS; ++k)
        if (a.off[k] % 16 || a.off[k] < 0 || a.sec_bytes[k] < 0 || a.off[k] + a.sec_bytes[k] > a.record_bytes)
            return hipErrorInvalidValue;
    if (a.sec_bytes[EWK_SNAP_RING] != a.row_bytes || a.sec_bytes[EWK_SNAP_BLOCK_RMS] != (int64_t)a.n_blocks * 8 ||
        a.sec_bytes[EWK_SNAP_SORTED] != (int64_t)a.n_blocks * 8 || a.sec_bytes[EWK_SNAP_HISTORY] != (int64_t)a.H * 4 ||
        a.sec_bytes[EWK_SNAP_CARRY] != (int64_t)a.in_block * a.es || a.sec_bytes[EWK_SNAP_GATE] != (int64_t)sizeof(GateStream) ||
        a.sec_bytes[EWK_SNAP_LISTENERS] != (int64_t)(kLsnStates * sizeof(LsnState)))
        return hipErrorInvalidValue;
    *pieces = std::max<int64_t>(1, (a.row_bytes + kSnapPiece - 1) / kSnapPiece);
    if (*pieces * a.n > 0x7fffffffLL) return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t launch_snapshot_pack(const SnapArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    int64_t pieces = 0;
    const hipError_t err = check_args(a, &pieces);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_snapshot_pack, dim3((unsigned)(pieces * a.n)), dim3(kSnapThreads), 0, s, a, (int32_t)pieces);
    return hipGetLastError();
}

hipError_t launch_snapshot_unpack(const SnapArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    int64_t pieces = 0;
    const hipError_t err = check_args(a, &pieces);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_snapshot_unpack, dim3((unsigned)(pieces * a.n)), dim3(kSnapThreads), 0, s, a, (int32_t)pieces);
    return hipGetLastError();
}

}  // namespace ewk
