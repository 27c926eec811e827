// ewk_resample.hip -- input-rate resampler: polyphase FIR from a source's own sample rate to
// the engine's 16 kHz, for whole signals (ewk_resample) and for the streaming push path
// (ewk_set_input_rate), float32, int16 PCM or G.711 input.  The arithmetic is ResampleArgs'
// (ewk_internal.h): only the taps of an output's phase are touched, J per output.
//
// One workgroup computes kRsQ * S consecutive outputs of one row, S = blockDim.x a multiple of
// `up`: thread t owns outputs t, t + S, .. of the tile, which share a phase, so each tap is
// loaded once for kRsQ outputs.  The tile's input span, history included, is staged in LDS
// once with coalesced loads (int16 and G.711 decoded on the way); outputs are stored coalesced.  The tap
// table is [J][up] (phase-minor) and read through L1/L2: with up = 1 (48, 32, 96 kHz) a tap
// load is one address for the whole wave.
//
// G.711 input (ResampleG711) runs instantiations of its own, k_resample<ResampleG711> and
// k_resample_save<ResampleG711>, which take it as a trailing argument: a tick's code bytes are read
// once and land in LDS as float, nothing is written in between.  k_resample<> and
// k_resample_save<> keep the arguments and the code they had before G.711.
#include "ewk_g711.h"
#include "ewk_internal.h"

namespace ewk {

// G.711 input sample `at`; G is empty (float32 / PCM16 input, never called) or ResampleG711
template <typename... G>
__device__ __forceinline__ float rs_g711(int64_t at, const G&... g) {
    if constexpr (sizeof...(G) > 0) return (g711_sample(g.p[at], g.law), ...);
    else return 0.0f;
}

// X(i) of a row (ResampleArgs), any i
template <typename... G>
__device__ __forceinline__ float rs_x(const ResampleArgs& a, int64_t row, int64_t hrow, int64_t i, const G&... g) {
    if (i < 0) return (a.hist && i >= -(int64_t)a.H) ? a.hist[hrow * a.H + a.H + i] : 0.0f;
    if (i >= a.n_in) return 0.0f;
    const int64_t t = i / a.in_block, r = i - t * a.in_block;
    const int64_t at = row * a.stride + t * a.tick_stride + r;
    if constexpr (sizeof...(G) > 0) return rs_g711(at, g...);
    else return a.in16 ? (float)a.in16[at] * (1.0f / 32768.0f) : a.in[at];
}

template <typename... G>
__global__ __launch_bounds__(kRsMaxThreads) void k_resample(const ResampleArgs a, const int32_t tiles, const G... g) {
    extern __shared__ float s_x[];   // [a.span]: X(i_lo ..)
    const int S = (int)blockDim.x, t = (int)threadIdx.x;
    const int64_t row = blockIdx.x / (uint32_t)tiles;
    const int64_t hrow = a.ids ? a.ids[row] : row;   // the stream of this row: its history and fresh flag
    const int64_t o0 = (int64_t)(blockIdx.x % (uint32_t)tiles) * kRsQ * S;
    // c of the tile's first output, floor-divided by up (c > -down can be negative)
    const int64_t cb = o0 * a.down + a.c0;
    int64_t ib = cb / a.up, rb = cb - ib * a.up;
    if (rb < 0) { rb += a.up; ib -= 1; }
    const int64_t i_lo = ib - (a.J - 1);
    {   // stage the span: the tick of the first sample once, then a compare per sample
        const int64_t i_pos = i_lo > 0 ? i_lo : 0;
        const int64_t t_lo = i_pos / a.in_block;
        const int64_t base = row * a.stride;
        for (int k = t; k < a.span; k += S) {
            const int64_t i = i_lo + k;
            float v = 0.0f;
            if (i < 0) {
                if (a.hist && i >= -(int64_t)a.H) v = a.hist[hrow * a.H + a.H + i];
            } else if (i < a.n_in) {
                int64_t tt = t_lo, r = i - t_lo * a.in_block;
                if (r >= a.in_block) {
                    const int64_t dt = r / a.in_block;
                    tt += dt;
                    r -= dt * a.in_block;
                }
                const int64_t at = base + tt * a.tick_stride + r;
                if constexpr (sizeof...(G) > 0) v = rs_g711(at, g...);
                else v = a.in16 ? (float)a.in16[at] * (1.0f / 32768.0f) : a.in[at];
            }
            s_x[k] = v;
        }
    }
    __syncthreads();
    const uint32_t d0 = (uint32_t)t * (uint32_t)a.down + (uint32_t)rb;
    const uint32_t idx0 = d0 / (uint32_t)a.up, p = d0 - idx0 * (uint32_t)a.up;
    const uint32_t step = (uint32_t)((int64_t)S * a.down / a.up);   // exact: S is a multiple of up
    const double* tp = a.taps + p;
    double acc[kRsQ];
#pragma unroll
    for (int q = 0; q < kRsQ; ++q) acc[q] = 0.0;
    uint32_t k = idx0;   // s_x[k] = X(i - j) for j = J - 1
    for (int j = a.J - 1; j >= 0; --j, ++k) {
        const double h = tp[(size_t)j * a.up];
#pragma unroll
        for (int q = 0; q < kRsQ; ++q) acc[q] = fma(h, (double)s_x[k + q * step], acc[q]);
    }
    float* o = a.out + row * a.out_stride;
    const int64_t n_zero = (a.fresh && !a.fresh[hrow]) ? 0 : a.n_zero;
#pragma unroll
    for (int q = 0; q < kRsQ; ++q) {
        const int64_t n = o0 + t + (int64_t)q * S;
        if (n < a.n_out) o[n] = n < n_zero ? 0.0f : (float)acc[q];
    }
}

// one workgroup per row: read the new tail (it may reach into the old history), then write it;
// the row's stream has had a push now (its fresh flag)
template <typename... G>
__global__ __launch_bounds__(256) void k_resample_save(const ResampleArgs a, float* hist, uint8_t* fresh,
                                                       const G... g) {   // (hist == a.hist, fresh == a.fresh)
    extern __shared__ float s_h[];   // [a.H]
    const int64_t row = blockIdx.x;
    const int64_t hrow = a.ids ? a.ids[row] : row;
    for (int k = threadIdx.x; k < a.H; k += blockDim.x) s_h[k] = rs_x(a, row, hrow, a.n_in - a.H + k, g...);
    __syncthreads();
    for (int k = threadIdx.x; k < a.H; k += blockDim.x) hist[hrow * a.H + k] = s_h[k];
    if (fresh && threadIdx.x == 0) fresh[hrow] = 0;
}

int resample_threads(int32_t up) {
    if (up <= 0 || up > kRsMaxThreads) return 0;
    return up > 256 ? up : up * (256 / up);
}

int64_t resample_span(int32_t up, int32_t down, int32_t J, int32_t threads) {
    const int64_t tile = (int64_t)kRsQ * threads;
    return ((tile - 1) * down + up - 1) / up + J;
}

hipError_t launch_resample(const ResampleArgs& a, hipStream_t s, ResampleG711 g) {
    if (a.rows <= 0 || a.n_out <= 0) return hipSuccess;
    if (a.threads <= 0 || a.threads % a.up || a.span > kRsMaxSpan ||
        a.span != resample_span(a.up, a.down, a.J, a.threads) || a.in_block <= 0 ||
        (g.p && (a.in || a.in16 || (g.law != kG711Ulaw && g.law != kG711Alaw))))
        return hipErrorInvalidValue;
    const int64_t tile = (int64_t)kRsQ * a.threads;
    const int64_t tiles = (a.n_out + tile - 1) / tile;
    if (tiles * a.rows > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(tiles * a.rows));
    const size_t lds = (size_t)a.span * sizeof(float);
    if (g.p) hipLaunchKernelGGL(k_resample<ResampleG711>, grid, dim3(a.threads), lds, s, a, (int32_t)tiles, g);
    else hipLaunchKernelGGL(k_resample<>, grid, dim3(a.threads), lds, s, a, (int32_t)tiles);
    return hipGetLastError();
}

hipError_t launch_resample_save(const ResampleArgs& a, float* hist, uint8_t* fresh, hipStream_t s, ResampleG711 g) {
    if (a.rows <= 0 || a.H <= 0) return hipSuccess;
    if (a.H > kRsMaxSpan || a.in_block <= 0) return hipErrorInvalidValue;
    const size_t lds = (size_t)a.H * sizeof(float);
    if (g.p) hipLaunchKernelGGL(k_resample_save<ResampleG711>, dim3(a.rows), dim3(256), lds, s, a, hist, fresh, g);
    else hipLaunchKernelGGL(k_resample_save<>, dim3(a.rows), dim3(256), lds, s, a, hist, fresh);
    return hipGetLastError();
}

}  // namespace ewk
