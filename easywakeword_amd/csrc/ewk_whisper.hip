// ewk_whisper.hip -- the level-3 front end: Whisper's 80-band log-mel input features
// (include/ewk.h, ewk_whisper_features_*) of segments k_normalize (ewk_level3.hip) has written
// as float64.  Two kernels (ewk_internal.h, WfArgs):
//
//   * k_whisper_frames: the live frames only.  A workgroup of four waves stages the samples of
//     eight consecutive frames (1520, reflected at both ends of the n_frames * 160 window, rounded
//     once to float32) in LDS; each wave then takes two of the frames, one after the other:
//     window, a 400-point real transform as 16 x 25 (below), power of bins 0..200, the 80 packed
//     Slaney bands, log10.  The raw log-mel goes to scratch frame-major, with the frame's maximum.
//   * k_whisper_finish: a workgroup per 64 frames of a segment reduces the segment's frame
//     maxima, transposes its tile of the scratch through LDS and stores [80][n_frames] rows with
//     the frame index along the lanes; frames past the live ones get the floor constant.
//
// The transform.  n = 16 a + b, k = k1 + 25 k2:
//     X[k] = sum_b W400^(b k) * Y[b][k1],   Y[b][k1] = sum_a x[16 a + b] W25^(a k1)
// 25-point DFTs of the 16 decimated rows first (real input: k1 = 0..12, the rest by conjugation),
// then one 16-term sum per bin, twiddle and radix-16 step in one table of W400.  The longest sum
// has 25 terms, so the float32 error stays that of an FFT.  Twiddles, window and mel weights are
// float64 values rounded once (ewk_tables.cpp).
//
// A non-finite sample (k_normalize leaves only NaN) is carried as a flag next to the maxima: a
// frame that read one reports NaN as its maximum, and the finish stage turns any NaN among a
// segment's frame maxima into an all-NaN output, as np.maximum / torch.maximum do.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ewk_internal.h"

namespace ewk {

constexpr int kWfSpan = kWfHop * (kWfFramesPerBlock - 1) + kWfFft;   // 1520 samples per workgroup
constexpr int kWfRows = 16, kWfCols = 25, kWfHalf = 13;              // 400 = 16 x 25; k1 = 0..12 stored

__global__ __launch_bounds__(256) void k_whisper_frames(WfArgs a) {
    __shared__ float s_x[kWfSpan];
    __shared__ float s_win[kWfFft], s_c400[kWfFft], s_s400[kWfFft], s_c25[25], s_s25[25];
    __shared__ float s_melw[kWfMelCap];
    __shared__ int32_t s_lo[kWfMels], s_n[kWfMels], s_off[kWfMels];
    __shared__ float s_yr[4][kWfRows * kWfHalf], s_yi[4][kWfRows * kWfHalf];
    __shared__ float s_p[4][kWfBins + 7];
    const WfSeg sg = a.seg[blockIdx.x];
    const int t0 = blockIdx.y * kWfFramesPerBlock;
    if (t0 >= sg.n_live) return;   // (the whole workgroup)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const WhisperTables* __restrict__ tab = a.tab;
    for (int i = tid; i < kWfFft; i += 256) {
        s_win[i] = tab->win[i];
        s_c400[i] = tab->c400[i];
        s_s400[i] = tab->s400[i];
    }
    for (int i = tid; i < kWfMelCap; i += 256) s_melw[i] = tab->mel_w[i];
    if (tid < 25) {
        s_c25[tid] = tab->c25[tid];
        s_s25[tid] = tab->s25[tid];
    }
    if (tid < kWfMels) {
        s_lo[tid] = tab->mel_lo[tid];
        s_n[tid] = tab->mel_n[tid];
        s_off[tid] = tab->mel_off[tid];
    }
    // the samples of frames t0 .. t0 + 7: x[i] for i = 160 t0 - 200 + j, reflected about 0 and
    // n - 1 (period 2 n - 2, as np.pad's reflect continues it), zero at and past the segment's end
    const int n = a.n_frames * kWfHop, period = 2 * n - 2;
    const double* __restrict__ y = a.y + sg.y_off;
    for (int j = tid; j < kWfSpan; j += 256) {
        int i = (kWfHop * t0 - kWfFft / 2 + j) % period;
        if (i < 0) i += period;
        if (i >= n) i = period - i;
        s_x[j] = i < sg.len ? (float)y[i] : 0.0f;
    }
    __syncthreads();
    const int b = lane & 15, g = lane >> 4;
    for (int it = 0; it < kWfFramesPerBlock / 4; ++it) {
        const int f = w + 4 * it, t = t0 + f;
        const bool live = t < sg.n_live;   // per wave
        bool bad = false;
        // ---- 25-point DFTs of row b, k1 = g, g + 4, g + 8 (and 12 for g = 0)
        if (live) {
            float xr[kWfCols];
#pragma unroll
            for (int q = 0; q < kWfCols; ++q) {
                const float v = s_x[kWfHop * f + kWfRows * q + b];
                bad |= v != v;
                xr[q] = v * s_win[kWfRows * q + b];
            }
#pragma unroll 1   // (unrolled, the four passes keep 246 VGPRs live: two waves per SIMD instead of five)
            for (int r = 0; r < 4; ++r) {
                const int k1 = g + 4 * r;
                if (k1 >= kWfHalf) break;
                float re = 0.0f, im = 0.0f;
                int idx = 0;
#pragma unroll
                for (int q = 0; q < kWfCols; ++q) {
                    re += xr[q] * s_c25[idx];
                    im -= xr[q] * s_s25[idx];
                    idx += k1;
                    if (idx >= kWfCols) idx -= kWfCols;
                }
                s_yr[w][b * kWfHalf + k1] = re;
                s_yi[w][b * kWfHalf + k1] = im;
            }
        }
        __syncthreads();
        // ---- X[k] = sum_b Y[b][k mod 25] W400^(b k), k = lane + 64 j; power
        if (live) {
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int k = lane + 64 * j;
                if (k >= kWfBins) break;
                const int k1 = k % kWfCols;
                const int kk = k1 < kWfHalf ? k1 : kWfCols - k1;
                const float sgn = k1 < kWfHalf ? 1.0f : -1.0f;   // Y[b][25 - k1] = conj(Y[b][k1])
                float re = 0.0f, im = 0.0f;
                int idx = 0;
#pragma unroll
                for (int q = 0; q < kWfRows; ++q) {
                    const float yr = s_yr[w][q * kWfHalf + kk], yi = sgn * s_yi[w][q * kWfHalf + kk];
                    const float c = s_c400[idx], s = s_s400[idx];
                    re += yr * c + yi * s;
                    im += yi * c - yr * s;
                    idx += k;
                    if (idx >= kWfFft) idx -= kWfFft;
                }
                s_p[w][k] = re * re + im * im;
            }
        }
        __syncthreads();
        // ---- mel bands lane and lane + 64, log10, the frame's maximum
        if (live) {
            float mx = -10.0f;
            for (int m = lane; m < kWfMels; m += 64) {
                const int lo = s_lo[m], cnt = s_n[m], off = s_off[m];
                float acc = 0.0f;
                for (int q = 0; q < cnt; ++q) acc += s_melw[off + q] * s_p[w][lo + q];
                const float L = acc <= 1e-10f ? -10.0f : log10f(acc);   // log10(max(acc, 1e-10)); NaN stays
                bad |= L != L;
                mx = fmaxf(mx, L);
                a.raw[(sg.raw_off + t) * kWfMels + m] = L;
            }
            for (int s = 1; s < 64; s <<= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
            const bool any_bad = __any(bad) != 0;
            if (lane == 0) a.fmax[sg.raw_off + t] = any_bad ? __builtin_nanf("") : mx;
        }
    }
}

__device__ __forceinline__ uint16_t wf_bf16(float v) {   // round to nearest even; NaN -> 0x7FC0
    if (v != v) return 0x7FC0;
    const uint32_t u = __float_as_uint(v);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

__global__ __launch_bounds__(256) void k_whisper_finish(WfArgs a) {
    __shared__ float s_tile[kWfTile][kWfMels + 1];
    __shared__ float s_mx[4];
    __shared__ int32_t s_bad[4];
    const WfSeg sg = a.seg[blockIdx.x];
    const int t0 = blockIdx.y * kWfTile;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // the segment's maximum (every raw value is >= -10, the value of a frame of pad zeros) and
    // its NaN flag
    float mx = -10.0f;
    int bad = 0;
    const float* __restrict__ fm = a.fmax + sg.raw_off;
    for (int i = tid; i < sg.n_live; i += 256) {
        const float p = fm[i];
        bad |= p != p;
        mx = fmaxf(mx, p);
    }
    for (int s = 1; s < 64; s <<= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
    bad = __any(bad) != 0;
    if (lane == 0) {
        s_mx[w] = mx;
        s_bad[w] = bad;
    }
    const int nl = min(max(sg.n_live - t0, 0), kWfTile);   // live frames of this tile
    const float* __restrict__ raw = a.raw + (sg.raw_off + t0) * kWfMels;
    for (int e = tid; e < nl * kWfMels; e += 256) s_tile[e / kWfMels][e % kWfMels] = raw[e];
    __syncthreads();
    mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
    const float floor_ = mx - 8.0f;
    const float dead = (fmaxf(-10.0f, floor_) + 4.0f) * 0.25f;
    const int t = t0 + lane;
    if (t >= a.n_frames) return;
    for (int m = w; m < kWfMels; m += 4) {
        float v = lane < nl ? (fmaxf(s_tile[lane][m], floor_) + 4.0f) * 0.25f : dead;
        if (bad) v = __builtin_nanf("");
        const int64_t o = ((int64_t)blockIdx.x * kWfMels + m) * a.n_frames + t;
        if (a.bf16)
            static_cast<uint16_t*>(a.out)[o] = wf_bf16(v);
        else
            static_cast<float*>(a.out)[o] = v;
    }
}

hipError_t launch_whisper_features(const WfArgs& a, hipStream_t s) {
    if (a.n_seg <= 0) return hipSuccess;
    if (a.max_live > 0) {
        const unsigned chunks = (unsigned)((a.max_live + kWfFramesPerBlock - 1) / kWfFramesPerBlock);
        hipLaunchKernelGGL(k_whisper_frames, dim3((unsigned)a.n_seg, chunks), dim3(256), 0, s, a);
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    const unsigned tiles = (unsigned)((a.n_frames + kWfTile - 1) / kWfTile);
    hipLaunchKernelGGL(k_whisper_finish, dim3((unsigned)a.n_seg, tiles), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ewk
