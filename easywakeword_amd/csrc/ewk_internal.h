// ewk_internal.h -- shared constants, table layout and launch prototypes.
// Internal to libewk.so; the public C ABI is include/ewk.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ewk.h"

namespace ewk {

// librosa.feature.mfcc(y, sr=16000, n_mfcc=20, n_fft=512, hop_length=160)
// as called by WordMatcher.extract_mfcc (wakeword.py:561-563).
constexpr int NFFT = 512;
constexpr int HOP = 160;
constexpr int NBIN = NFFT / 2 + 1;   // 257
constexpr int NMEL = 128;
constexpr int NMFCC = EWK_N_MFCC;    // 20
constexpr int MEL_ITERS = 40;        // unrolled mel FMAs per lane: sum of per-group band widths
constexpr int SCR_FRAME = 272;       // per-frame FFT scratch floats (16 rows x 17)
// fp32 scorer shape: two frames per 16-lane group per pass (kNF, two independent FFT
// instruction streams per lane; the untangle pairs conjugate bins inside a lane), eight
// waves per workgroup, one workgroup per CU (2 waves per SIMD at 256 VGPRs).
constexpr int kNF = 2;
#ifndef EWK_WAVES
#define EWK_WAVES 8
#endif
constexpr int WAVES = EWK_WAVES;   // waves per scorer workgroup (one workgroup per CU)
// start (floats) of frame fr's FFT scratch / power spectrum in a scorer wave's LDS scratch:
// the two frames a 16-lane group untangles side by side (fr, fr + 4) land 8 banks apart
__host__ __device__ constexpr int scr_frame_off(int fr) { return fr * SCR_FRAME + 8 * (fr >> 2); }

// Host-built constant tables (ewk_tables.cpp); copied to LDS by every workgroup.
struct Tables {
    float2 win2[256];        // (w[2n], w[2n+1]) periodic Hann, n = 0..255
    float2 tw1[256];         // [k1*16 + j] = exp(-2*pi*i*j*k1/256)
    float2 tw2[256];         // [k]  = (cos, sin)(2*pi*k/512) for the real-FFT untangle
    int32_t band_lo[NMEL];   // first non-zero bin of mel band m
    // 0.25 * librosa float32 weights (0.25 folds the untangle's 1/2 squared), laid
    // out [iteration][lane j] for band m = j + 16*i, zero-padded to the group width
    float wpad[MEL_ITERS * 16];
    float dct[NMFCC * NMEL]; // DCT-II ortho rows 0..19
    int32_t ok;              // every band fits its compile-time group width
};

// fp64 path tables (rescoring / reference precision).
struct Tables64 {
    double win[NFFT];        // periodic Hann (scipy.signal.get_window('hann', 512, fftbins=True))
    double cs[NFFT];         // cos(2*pi*n/512)
    double sn[NFFT];         // sin(2*pi*n/512)
    float melw_dense[NMEL * NBIN];  // librosa float32 mel basis [128][257]
    double dct[NMFCC * NMEL];
    // the basis's band support, packed: band m = weights mel_w[mel_off[m] .. mel_off[m+1])
    // on bins mel_lo[m], mel_lo[m] + 1, ... (every non-zero weight, in bin order)
    int32_t mel_lo[NMEL];
    int32_t mel_off[NMEL + 1];
    float mel_w[2 * NBIN + 2 * NMEL];
};

void build_tables(Tables* t);
// the builders build_tables uses (also linked by scripts/probes/fp4_probe.hip)
void table_window(double* w /* [512] */);
void table_mel(float* w /* [128][257] */);
void table_dct(double* d /* [20][128] */);
void build_tables64(Tables64* t);

// fp64 re-score (csrc/ewk_rescore.h).  A segment the float32 pass cannot decide alone is
// listed in a slot and its 8-frame chunks get consecutive part records; a launch after the
// scorer (k_rescore_linear / k_rescore_ring) claims the chunks with one atomic each (part
// record g -> its slot), each chunk's sums land in its part record, and the wave finishing a
// slot's last chunk combines them in chunk order.  A slot that finds the part pool full (or
// every slot of ewk_score_segments_f64) is serial: one wave runs its chunks in order.
constexpr int kRsFrames = 8;   // frames per re-score chunk
constexpr int kRsCtl = 8;      // ints of ScoreArgs::rs_ctl
constexpr int kRsMelW = 12;    // widest Slaney band of the basis in bins (fp64 mel window; checked at engine creation)
constexpr int kRsMelWLo = 3;   // widest of bands 0..63 (the fp64 path's window for a lane's low band; checked too)
struct RsSlot {
    int32_t seg;       // segment (linear) or event (ring) index
    int32_t T;         // frames
    int32_t nclaim;    // chunks (1 for a serial slot)
    int32_t base;      // first part record of the slot (pooled slots)
    int32_t pad;
    int32_t done;      // chunks finished (atomic; zeroed by the lister)
    float theta_s;     // speculative top_db clamp: the float32 pass's log-mel max - 80 dB
    int32_t serial;    // 1: one wave runs every chunk in order (no part records)
};
struct RsPart {                 // one chunk: per coefficient k, rA rB sA sB sAA sAB sBB ([7][20])
    double v[7 * 20];
    double mx;                  // log-mel max of the chunk's frames
    int32_t n;                  // frames
    int32_t flags;              // 1: a value within the ambiguity window of theta_s, 2: NaN
    int32_t slot;               // the slot this record belongs to (-1: a failed reservation)
    int32_t pad[3];
};
// Whole 128-B lines per record (1,152 B): the records of one slot are written at the same time
// by different waves into uncached memory, and records sharing a line lost bytes (round 4, a
// 1,184-B layout: a few wrong fp64 scores).
static_assert(sizeof(RsPart) % 128 == 0, "part records own their cache lines");

// Segment sources for the scorer.
//   linear: segment i = pcm[offsets[i] : offsets[i] + lengths[i]]
//   ring  : event i -> ring + stream*ring_len, first sample ring_start, wrap at ring_len
struct ScoreArgs {
    const float* pcm;
    const int16_t* pcm16;     // ring mode with an int16 ring (EWK_RING_I16): samples x 32768
    const int64_t* offsets;
    const int32_t* lengths;
    ewk_event* events;        // ring mode: read stream/ring_start/length, write score/match/flags
    const int32_t* n_events;  // ring mode: device-side event count
    const int32_t* ev_base;   // ring mode: first unscored event (watermark, count space)
    int32_t ev_base0;         // ring mode: the bank's epoch base (event slot = count - ev_base0, wrapping)
    int32_t* work;            // per-launch work counter (zeroed before the launch)
    int64_t ring_len;
    int32_t n_seg;            // linear mode count, ring mode capacity
    int32_t has_template;
    int32_t cand_f32;         // candidate dtype of the reference path: 1 float32, 0 float64
    const float* tmpl;        // [40] template mean[20], std[20]
    float uu_m32, uu_s32;     // template self-dots as numpy computes them (float32 sdot)
    float* out_mean;          // linear mode by segment; ring modes (nullptr: none) by event slot
    float* out_std;
    float* out_theta;         // ring modes (nullptr: none): the pass's theta_s by event slot
    double* out_score;
    uint8_t* out_match;
    double threshold;
    double rescore_margin;
    int32_t* order;           // linear mode: work order scratch [n_seg] (longest first), nullptr = index order
    // fp64 re-score (nullptr rs_slots: none).  rs_ctl (kRsCtl ints): [0] slots listed,
    // [1] part records reserved, [2] serial slots listed, [3] workgroups out, [4] chunk claim
    // cursor, [5] serial claim cursor; the last workgroup out of the re-score launch zeroes
    // them (and *work) and, in ring mode, sets *adv_ev_base = *n_events.  The part records
    // live in uncached memory (hipDeviceMallocUncached): written by one wave and read by
    // another, on any XCD, with no L2 write-back or invalidate in between.
    int32_t* rs_ctl;
    RsSlot* rs_slots;
    int32_t* rs_serial;       // [rs_cap] serial slots, in listing order
    int32_t rs_cap;
    int32_t rs_part_cap;
    RsPart* rs_parts;
    int32_t list_all;         // every segment goes to the fp64 path (ewk_score_segments_f64)
    double* out_mean64;       // list_all: fp64 statistics [n][20]
    double* out_std64;
    int32_t* adv_ev_base;
    const struct Tables64* tab64;   // fp64 tables
    // ring mode poll mirror (nullptr: none): the last workgroup copies the bank's counters
    // (evc) and its first min(queued, mirror_chunk) events into pinned host memory
    unsigned char* mirror;
    const int32_t* evc;
    int32_t mirror_chunk;
};

// ring_mode: 0 linear batch, 1 ring events one segment per workgroup, 2 ring events one
// segment per wave (many events per tick)
hipError_t launch_score_f32(const Tables* d_tab, const ScoreArgs& a, int ring_mode, hipStream_t s);
// fp64 re-score of what a linear launch listed (ring launches drain their list themselves)
hipError_t launch_rescore_linear(const ScoreArgs& a, hipStream_t s);
hipError_t launch_rescore_ring(const ScoreArgs& a, hipStream_t s);
// streams from which a tick's events are scored one segment per wave (ring_mode 2)
constexpr int kRingWaveStreams = 65536;
// ScoreArgs::order holds n_seg indices followed by kLptScratch ints of bucket counters
constexpr int kLptScratch = 128;
hipError_t launch_snapshot(const int32_t* src, int32_t* dst, hipStream_t s);   // *dst = *src, stream-ordered
// counters + first min(queued, chunk) events of an event bank -> pinned host memory (poll mirror)
hipError_t launch_bank_mirror(const int32_t* evc, const ewk_event* ev, uint32_t base0, int32_t cap, int32_t chunk,
                              unsigned char* host, hipStream_t s);

// Template bank (ewk_bank.hip): every segment's MFCC statistics against the templates of one
// word.  Pass 1 is launch_score_f32 without a template (statistics only), pass 2
// launch_bank_score, pass 3 the list_all fp64 path on the listed segments followed by
// launch_bank_rescore.
struct RescoreCriteria {           // the scorer's vanishing-mean listing constants (ewk_mfcc.hip)
    double tiny_mean, nan_a, nan_b;
};
RescoreCriteria rescore_criteria();
constexpr int kBankRow = 2 * NMFCC + 2;   // floats per template: mean[20], std[20], uu_m, uu_s
struct BankArgs {
    // word w (s = its size) starts at bank + kBankRow * word_first[w] and is value-major:
    // value c of its template j at [c * s + j] -- lane j's loads are contiguous across its group
    const float* bank;
    const int32_t* word_first;    // [n_words + 1]
    const double* thresholds;     // [n_words]
    int32_t n_words;
    int32_t max_word;             // the bank's largest word: a segment takes the next power of two lanes
    int32_t group_log2;           // (set by the launchers) log2 of that group width
    // statistics [.][20]: float32 by segment (launch_bank_score), float64 by list position
    // (launch_bank_rescore)
    const void* mean;
    const void* stdv;
    const int64_t* offsets;       // by segment (launch_bank_score only)
    const int32_t* lengths;
    const int32_t* word;          // by segment; nullptr: word 0
    int32_t n;                    // segments (launch_bank_score) / listed segments (launch_bank_rescore)
    ewk_bank_result* out;         // by segment
    double* out_scores;           // nullptr or [n][stride]
    int32_t stride;
    int32_t cand_f32;
    double rescore_margin;
    RescoreCriteria crit;
    // segments the float32 statistics cannot decide: count, then (segment, offset, length) per
    // entry in arrival order (any order gives the same results: pass 3 writes by segment)
    int32_t* list_cnt;
    int32_t* list_seg;
    int64_t* list_off;
    int32_t* list_len;
};
hipError_t launch_bank_score(const BankArgs& a, hipStream_t s);     // (zeroes *list_cnt first)
hipError_t launch_bank_rescore(const BankArgs& a, hipStream_t s);

// Stream bank (ewk_bank.hip, k_bank_events): the pending events of a ring-mode scoring pass
// against the templates of their streams' words, with k_bank's code.  Between the ring scorer
// without a template (statistics by event slot: ScoreArgs::out_mean / out_std / out_theta) and
// launch_rescore_ring, the float32 pass scores every event of the pending window -- read
// device-side as the ring scorer reads it -- and lists those it cannot decide: into the
// re-score slots (rs_list) and, as a count plus event slots, into ev_list.  After
// launch_rescore_ring (fp64 statistics by event slot: out_mean64 / out_std64) the fp64 pass
// scores the events of ev_list again and its last workgroup out zeroes the count.
// BankArgs: bank, word_first, thresholds, n_words, max_word, rescore_margin, crit, and mean /
// stdv = the statistics by event slot (float32 or float64); the rest is unused.
// ScoreArgs: events, n_events, ev_base, ev_base0, n_seg (capacity), out_theta and the re-score
// list (rs_ctl, rs_slots, rs_serial, rs_cap, rs_parts, rs_part_cap).
constexpr int kEvListHdr = 4;   // ints before ev_list's slots: [0] count, [1] workgroups out
struct BankEvArgs {
    const int32_t* stream_word;   // [n_streams]; nullptr: word 0
    int32_t* ev_list;             // [kEvListHdr + capacity]
    int32_t grid;                 // workgroups (fixed per engine: the waves stride over the events)
    // stream listeners: an event cut by listener j >= 1 (EWK_EV_LISTENER) is scored against word
    // lsn_tab[stream * EWK_LISTENERS_MAX + j].word; nullptr: no stream has had listeners
    const ewk_listener* lsn_tab;
};
hipError_t launch_bank_events(const BankArgs& b, const ScoreArgs& a, const BankEvArgs& x, hipStream_t s);
hipError_t launch_bank_events_rescore(const BankArgs& b, const ScoreArgs& a, const BankEvArgs& x, hipStream_t s);

constexpr int kScoreGridMax = 256;   // one resident workgroup wave of the grid
constexpr int kScoreGridRing = 256;                     // ring-mode grid (device-side event count)
int score_grid(int n_seg, int ring_mode);

// Level-3 pre-processing (ewk_level3.hip): segment i is pcm[offsets[i] ...][:lengths[i]]
// (linear) or the ring slice of events[i] (ring_len > 0); output at out[out_offsets[i]].
struct L3Args {
    const float* pcm;
    const int16_t* pcm16;        // ring mode with an int16 ring: samples x 32768
    const int64_t* offsets;
    const int32_t* lengths;
    const ewk_event* events;
    int64_t ring_len;            // 0 = linear
    const int64_t* out_offsets;
    double* out;
    int32_t n;
};
hipError_t launch_normalize(const L3Args& a, hipStream_t s);
hipError_t launch_decode_pcm16(const int16_t* in, float* out, int64_t n, hipStream_t s);
// G.711 codes (ewk_g711.h) -> float32, any alignment of `in` and `out`
hipError_t launch_decode_g711(const uint8_t* in, float* out, int64_t n, int32_t law, hipStream_t s);

// Input-rate resampler (ewk_resample.hip): polyphase FIR in_rate -> cfg.sample_rate with the
// filter of audio.resample (ewk_tables.cpp: up = out / gcd, down = in / gcd, half = 10 *
// max(up, down), 2 * half + 1 taps).  Output n of a row is
//   sum_j h[p + j * up] * X(i - j),  c = n * down + c0,  i = floor(c / up),  p = c - i * up,
// j = J - 1 .. 0 (ascending input index, scipy's order) in float64, rounded once to float32.
// X(i) is input sample i of the row: tick i / in_block, offset i % in_block of it; zero at and
// past n_in; for i < 0 the row's history hist[H + i] (the H samples before sample 0), zero
// without one.  c0 = half for the whole-signal resample, half - delay * down when streaming:
// the stream is the whole-signal resample delayed by `delay` samples, and its first `delay`
// samples (which would be the filter's ringing ahead of the signal) are zero.
void resample_ratio(int32_t in_rate, int32_t out_rate, int32_t* up, int32_t* down);
void resample_taps(int32_t up, int32_t down, double* h /* [20 * max(up, down) + 1] */);
constexpr int kRsQ = 4;              // outputs per thread (they share a phase, so a tap load)
constexpr int kRsMaxThreads = 1024;  // a workgroup covers whole periods of `up` outputs: up <= this
constexpr int kRsMaxSpan = 12288;    // floats of input a workgroup stages in LDS (48 KB)
struct ResampleArgs {
    const float* in;          // float32 input, or
    const int16_t* in16;      // int16 PCM (x / 32768), or ResampleG711 below
    int64_t stride;           // samples between rows (streams)
    int64_t tick_stride;      // samples between the ticks of a row
    int64_t in_block;         // samples per tick (one-shot: n_in)
    int64_t n_in;             // input samples per row
    const float* hist;        // nullptr or [rows][H]
    float* out;               // [rows][out_stride]
    int64_t out_stride;
    int64_t n_out;            // outputs per row
    int32_t rows;
    const double* taps;       // [J][up]: taps[j * up + p] = h[p + j * up], zero past the filter
    int32_t up, down, J, H;
    int64_t c0;
    int64_t n_zero;           // outputs n < n_zero are zero (a stream's first `delay` samples)
    int32_t threads;          // resample_threads(up)
    int32_t span;             // resample_span(up, down, J, threads) <= kRsMaxSpan
    // subset pushes (ewk_push_streams): row r is stream ids[r] -- its history row and fresh flag;
    // nullptr: row r is stream r
    const int32_t* ids;
    // nullptr: n_zero holds for every row; else [streams] and only for the streams flagged (no push
    // since their history was cleared); launch_resample_save clears the flags of its rows
    const uint8_t* fresh;
};
// G.711 input of a launch (ResampleArgs::in and in16 nullptr then): one code byte per sample at p,
// indexed as `in`, decoded with `law` (ewk_g711.h) on the way into LDS.  p == nullptr: none.  It
// travels beside ResampleArgs, not in it, and runs instantiations of its own: the float32 / PCM16
// launches keep the argument layout and the code they had.
struct ResampleG711 {
    const uint8_t* p;
    int32_t law;
};
int resample_threads(int32_t up);   // workgroup size: a multiple of up (0: up > kRsMaxThreads)
int64_t resample_span(int32_t up, int32_t down, int32_t J, int32_t threads);
hipError_t launch_resample(const ResampleArgs& a, hipStream_t s, ResampleG711 g = {nullptr, 0});
// hist[r][k] = X(n_in - H + k): the tail of a push, saved once every workgroup of launch_resample
// has read the old one (stream order); fresh: nullptr or a.fresh
hipError_t launch_resample_save(const ResampleArgs& a, float* hist, uint8_t* fresh, hipStream_t s,
                                ResampleG711 g = {nullptr, 0});

// Packet ingest (ewk_chunks.hip): one launch per ewk_push_chunks* call re-blocks the call's
// chunks.  Stream d.stream holds d.pending < in_block samples in its carry row
// carry[d.stream * in_block ..]; its chunk src[d.src .. d.src + d.count) follows them.  With
// T = (d.pending + d.count) / in_block >= 1 the first T * in_block samples of carry ++ chunk
// become the tick rows out[d.row + t * in_block ..], t < T, and the rest (from the chunk's tail
// alone) the new carry; with T = 0 the chunk is appended to the carry at d.pending.  Carry and
// rows have the ring's sample type, PCM16 into float is decoded as x / 32768, G.711 into float
// with the chunk's own law (ewk_g711.h): a call may mix PCMU and PCMA streams.
struct ChunkDesc {
    int64_t src;       // first sample of the chunk (elements of the source type)
    int64_t row;       // first sample of the chunk's tick row 0 in `out` (elements; unused without a tick)
    int32_t stream;
    int32_t count;
    int32_t pending;   // before the push
    int32_t law;       // G.711 sources: the chunk's law (kG711Ulaw / kG711Alaw); else 0
};
static_assert(sizeof(ChunkDesc) == 32, "chunk descriptors are staged as bytes");
struct ChunkArgs {
    const void* src;          // float32, int16 with src16, or G.711 bytes with src8
    void* out;                // tick rows: float32, or int16 with out16
    void* carry;              // [n_streams][in_block], the type of out
    const ChunkDesc* desc;    // [n]
    int32_t n;
    int32_t in_block;
    int32_t max_ticks;        // the largest T of the call (the launch's grid.y, at least 1)
    int32_t src16, out16;     // (float32 into int16 does not exist: an int16 ring takes PCM16)
    int32_t src8;             // (G.711 into int16 neither: it needs an input rate, which an int16 ring refuses)
};
hipError_t launch_chunk_assemble(const ChunkArgs& a, hipStream_t s);

// ewk_gather.hip: positives compaction (scratch: 2 * compact_blocks(n) int32)
int compact_blocks(int32_t n);
hipError_t launch_compact_positives(const double* score, const uint8_t* match, int32_t n, int64_t first_id,
                                    int64_t step, ewk_positive* out, int32_t* d_count, int32_t* scratch, int append,
                                    hipStream_t s);

// Level-3 front end (ewk_whisper.hip): Whisper's log-mel features (include/ewk.h,
// ewk_whisper_features_*) of segments k_normalize has written as float64.  Segment i is
// y[seg[i].y_off ..][:seg[i].len], len already cut to n_frames * 160.  Frame t of it reads samples
// 160 t - 200 .. 160 t + 199 (reflected at 0 and at n_frames * 160), so the first
// n_live = min(n_frames, (len + 199) / 160 + 1) frames (0 for len = 0) read a sample of the segment
// and every later one reads only pad zeros.  k_whisper_frames writes the raw log-mel of the live
// frames to raw[(seg[i].raw_off + t) * 80 + m] and the frame's maximum over m to
// fmax[seg[i].raw_off + t] (NaN for a frame that read a NaN); k_whisper_finish reduces a
// segment's maxima, clamps, scales and writes out[i][m][t] for every t < n_frames.
constexpr int kWfFft = 400;
constexpr int kWfHop = 160;
constexpr int kWfBins = kWfFft / 2 + 1;   // 201
constexpr int kWfMels = 80;
constexpr int kWfMaxFrames = 3000;
constexpr int kWfMelCap = 512;            // packed non-zero mel weights (about 2 per bin)
constexpr int kWfFramesPerBlock = 8;      // k_whisper_frames: two frames per wave
constexpr int kWfTile = 64;               // k_whisper_finish: frames per workgroup
struct WhisperTables {
    float win[kWfFft];                 // periodic Hann, 0.5 - 0.5 cos(2 pi i / 400)
    float c25[25], s25[25];            // cos, sin (2 pi j / 25)
    float c400[kWfFft], s400[kWfFft];  // cos, sin (2 pi j / 400)
    // float32 of confirm._slaney_mel(16000, 400, 80), packed: band m = weights
    // mel_w[mel_off[m] .. mel_off[m] + mel_n[m]) on bins mel_lo[m], mel_lo[m] + 1, ...
    float mel_w[kWfMelCap];
    int32_t mel_lo[kWfMels], mel_n[kWfMels], mel_off[kWfMels];
    int32_t ok;                        // the packed weights fit kWfMelCap
};
void build_whisper_tables(WhisperTables* t);
struct WfSeg {
    int64_t y_off;      // first sample of the segment in WfArgs::y
    int64_t raw_off;    // first live frame of the segment in raw / fmax (frames)
    int32_t len;        // min(length, n_frames * 160)
    int32_t n_live;
};
struct WfArgs {
    const double* y;
    const WfSeg* seg;
    const WhisperTables* tab;
    float* raw;          // [sum n_live][80]
    float* fmax;         // [sum n_live]
    void* out;           // [n_seg][80][n_frames] float32, or bf16 bits
    int32_t n_seg, n_frames, bf16;
    int32_t max_live;    // the largest n_live
};
hipError_t launch_whisper_features(const WfArgs& a, hipStream_t s);

}  // namespace ewk
