// ewk_chunks.hip -- packet ingest: re-blocking the chunks of ewk_push_chunks* on the device.
//
// A source delivers any number of samples per call (RTP packets, a decoder's output); the gate
// takes whole ticks.  Every stream keeps its unfinished block in a carry row in device memory,
// and one launch per push cuts carry ++ chunk into tick rows and the new carry (ChunkDesc,
// ewk_internal.h).  Work items, one 256-thread workgroup each (grid = chunks x max ticks):
//   item A (y = 0), one per chunk: without a tick, append the chunk to the carry.  Else write row 0
//     from carry ++ chunk, then -- behind a workgroup barrier, when every read of the old carry has
//     returned -- the new carry, which comes from the chunk's tail alone (pending < in_block, so
//     the chunk is longer than what it leaves behind): old and new carry overlap in the row;
//   item B (y = t, 1 <= t < ticks): row t, from the chunk alone.
// Every copy is a span of contiguous samples with any phase at either end (a float row need not
// be 16-byte aligned, an int16 offset may be odd): scalar up to the destination's alignment, then
// units of 16 source bytes -- one 16-byte load where the source is aligned there too, element
// loads where the phases differ -- stored as 16-byte vectors, then a scalar tail.  Four type
// pairs: f32 -> f32, i16 -> f32 (x / 32768, exact), i16 -> i16, and G.711 codes -> f32 (u8,
// decoded with the chunk's own law, ewk_g711.h: a unit is 16 codes and four 16-byte stores, the
// destination aligned to 64 bytes).  u8 -> i16 is not built: G.711 needs an input rate, which an
// int16 ring refuses.
#include <hip/hip_runtime.h>

#include "ewk_g711.h"
#include "ewk_internal.h"

namespace ewk {

constexpr int kChunkThreads = 256;

// law: the chunk's G.711 law, wave-uniform (read by the u8 pair alone)
template <typename S, typename D>
__device__ __forceinline__ D chunk_conv(S x, int32_t law) {
    return (D)x;
}
template <>
__device__ __forceinline__ float chunk_conv<int16_t, float>(int16_t x, int32_t law) {
    return (float)x * (1.0f / 32768.0f);   // (as the gate decodes PCM16)
}
template <>
__device__ __forceinline__ float chunk_conv<uint8_t, float>(uint8_t x, int32_t law) {
    return g711_sample(x, law);
}

// dst[0..n) = src[0..n) by the whole workgroup.  Reads stay inside [src, src + n), writes inside
// [dst, dst + n).
template <typename S, typename D>
__device__ __forceinline__ void copy_span(D* dst, const S* src, int32_t n, int32_t law = 0) {
    constexpr int V = 16 / (int)sizeof(S);           // samples per unit: 16 source bytes
    constexpr int kDstVecs = V * (int)sizeof(D) / 16;   // 16-byte stores per unit
    constexpr uintptr_t kAlign = (uintptr_t)V * sizeof(D);
    const int tid = (int)threadIdx.x;
    int32_t head = (int32_t)(((kAlign - ((uintptr_t)dst & (kAlign - 1))) & (kAlign - 1)) / sizeof(D));
    head = head < n ? head : n;
    const int32_t units = (n - head) / V;
    for (int32_t i = tid; i < head; i += kChunkThreads) dst[i] = chunk_conv<S, D>(src[i], law);
    const bool src_vec = ((uintptr_t)(src + head) & 15) == 0;
    for (int32_t u = tid; u < units; u += kChunkThreads) {
        const S* sp = src + head + (int64_t)u * V;
        S in[V];
        if (src_vec) {
            const uint4 raw = *reinterpret_cast<const uint4*>(sp);
            __builtin_memcpy(in, &raw, 16);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) in[j] = sp[j];
        }
        D v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = chunk_conv<S, D>(in[j], law);
        uint4 outv[kDstVecs];
        __builtin_memcpy(outv, v, sizeof(outv));
        uint4* dp = reinterpret_cast<uint4*>(dst + head + (int64_t)u * V);
#pragma unroll
        for (int c = 0; c < kDstVecs; ++c) dp[c] = outv[c];
    }
    for (int32_t i = head + units * V + tid; i < n; i += kChunkThreads) dst[i] = chunk_conv<S, D>(src[i], law);
}

template <typename S, typename D>
__global__ __launch_bounds__(kChunkThreads) void k_chunk_assemble(ChunkArgs a) {
    const ChunkDesc d = a.desc[blockIdx.x];
    const int32_t in_block = a.in_block;
    const int32_t total = d.pending + d.count;   // (< 65 * in_block; the host keeps that below 2^31)
    const int32_t ticks = total / in_block;
    const int32_t t = (int32_t)blockIdx.y;
    if (t > 0 && t >= ticks) return;
    const S* chunk = static_cast<const S*>(a.src) + d.src;
    D* out = static_cast<D*>(a.out) + d.row;
    D* carry = static_cast<D*>(a.carry) + (int64_t)d.stream * in_block;
    if (t > 0) {   // item B
        copy_span<S, D>(out + (int64_t)t * in_block, chunk + ((int64_t)t * in_block - d.pending), in_block, d.law);
        return;
    }
    if (ticks == 0) {
        copy_span<S, D>(carry + d.pending, chunk, d.count, d.law);
        return;
    }
    copy_span<D, D>(out, carry, d.pending);
    copy_span<S, D>(out + d.pending, chunk, in_block - d.pending, d.law);
    __syncthreads();   // the old carry has been read (every load's value went into a store above)
    const int32_t rem = total - ticks * in_block;
    copy_span<S, D>(carry, chunk + (d.count - rem), rem, d.law);
}

hipError_t launch_chunk_assemble(const ChunkArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.in_block < 1 || a.max_ticks < 1 || (a.out16 && !a.src16) || (a.src8 && (a.src16 || a.out16)))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n, (unsigned)a.max_ticks);
    if (a.src8) hipLaunchKernelGGL((k_chunk_assemble<uint8_t, float>), grid, dim3(kChunkThreads), 0, s, a);
    else if (!a.src16) hipLaunchKernelGGL((k_chunk_assemble<float, float>), grid, dim3(kChunkThreads), 0, s, a);
    else if (!a.out16) hipLaunchKernelGGL((k_chunk_assemble<int16_t, float>), grid, dim3(kChunkThreads), 0, s, a);
    else hipLaunchKernelGGL((k_chunk_assemble<int16_t, int16_t>), grid, dim3(kChunkThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace ewk
