// ewk_engine.cpp -- the C ABI (include/ewk.h): engine lifetime and device memory, the single
// template, the threshold, profiling and the last error; with the helpers every engine source
// shares (ewk_engine.h).
#include <dlfcn.h>

#include "ewk_engine.h"

using namespace ewk;

static thread_local std::string g_err;

int ewk::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

hipEvent_t ewk::pool_event(ewk_engine* e) {
    if (!e->ev_pool.empty()) {
        hipEvent_t x = e->ev_pool.back();
        e->ev_pool.pop_back();
        return x;
    }
    hipEvent_t x = nullptr;
    if (hipEventCreate(&x) != hipSuccess) return nullptr;
    return x;
}

// Longest segment request the cut can make (wakeword.py:1100-1111): nreq =
// int(|sound_start - now - padding| * sr) with now - sound_start <= max speech +
// (post silence rounded up to a tick), capped at the ring (return_last_n_seconds).
int64_t ewk::segment_need(const ewk_config& c, int64_t ring_len, double speech_duration_max,
                          double post_speech_silence, double padding) {
    return std::min<int64_t>(ring_len, (int64_t)((speech_duration_max + post_speech_silence + c.tick_seconds + padding) *
                                                 (double)c.sample_rate) + 2);
}

// A segment is cut at the tick that ends it and scored after its gate launch,
// so the ticks of one launch after the cut must not reach its first sample:
// ticks_per_launch <= (ring - longest request) / block (>= 1: a one-tick launch is
// always safe, the cut never asks for more than the ring).  Overlapping the
// scoring with the next gate launch doubles the ticks that may pass.
void ewk::set_launch_ticks(ewk_engine* e, int64_t seg_need) {
    const int64_t room = (e->sring_len - std::min(seg_need, e->sring_len)) / (int64_t)e->cfg.block;
    const int64_t tpl = std::max<int64_t>(1, std::min<int64_t>(32, room));
    const int64_t tpl_ov = std::min<int64_t>(32, room / 2);
    e->overlap = tpl_ov >= 1 && e->overlap_want;
    e->ticks_per_launch = (int32_t)(e->overlap ? tpl_ov : tpl);
}

// Order stream s after every ring-mode scoring pass enqueued so far (they run on
// sstream): needed before touching what those passes read or share -- the template,
// the re-score list, the log-mel and fp64 scratch, the event banks.
hipError_t ewk::join_scoring(ewk_engine* e, hipStream_t s) {
    if (!e->overlap || !e->score_tail) return hipSuccess;
    return hipStreamWaitEvent(s, e->score_tail, 0);
}

// The re-score list holds at most one slot per segment of a launch (slots must start zeroed).
hipError_t ewk::reserve_rescore(ewk_engine* e, int32_t n_seg) {
    if (n_seg <= e->rs_cap) return hipSuccess;
    hipError_t err = hipSuccess;
    if (e->stream) err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess && e->sstream) err = hipStreamSynchronize(e->sstream);
    if (err != hipSuccess) return err;
    err = e->rs_slots.reserve((size_t)n_seg);
    if (err == hipSuccess) err = hipMemset(e->rs_slots.p, 0, (size_t)n_seg * sizeof(RsSlot));
    if (err == hipSuccess) err = e->rs_serial.reserve((size_t)n_seg);
    if (err != hipSuccess) return err;
    err = e->order.reserve((size_t)n_seg + kLptScratch);
    if (err != hipSuccess) return err;
    e->rs_cap = n_seg;
    return hipSuccess;
}

// Part records for the chunks of the slots listed in one launch (8 frames each).
static hipError_t reserve_parts(ewk_engine* e, int32_t n) {
    if (n <= e->rs_part_cap) return hipSuccess;
    hipError_t err = hipSuccess;
    if (e->stream) err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess && e->sstream) err = hipStreamSynchronize(e->sstream);
    e->rs_parts.flags = hipDeviceMallocUncached;
    if (err == hipSuccess) err = e->rs_parts.reserve((size_t)n);
    if (err == hipSuccess) e->rs_part_cap = n;
    return err;
}

extern "C" {

void ewk_default_config(ewk_config* c) {
    memset(c, 0, sizeof(*c));
    c->sample_rate = 16000;
    c->buffer_seconds = 10;
    c->block = 1600;
    c->tick_seconds = 0.1;
    c->pre_speech_silence = 0.8;
    c->speech_duration_min = 0.3;
    c->speech_duration_max = 2.0;
    c->post_speech_silence = 0.4;
    c->padding = 0.05;
    c->max_segment_seconds = 3.0;
    c->similarity_threshold = 75.0;
    c->reentry_timeout = 0.0;
    c->min_threshold = 0.005;
    c->initial_threshold = 0.01;
    c->rescore_margin = 1e-3;
}

const char* ewk_last_error(void) { return g_err.c_str(); }
int ewk_abi_version(void) { return EWK_ABI_VERSION; }

int ewk_runtime_info(char* path, int32_t cap, int32_t* hip_version) {
    // the definition hipLaunchKernel resolved to for this library: with RTLD_GLOBAL
    // interposition (e.g. torch's bundled runtime loaded first) it is not the
    // libamdhip64.so.7 libewk.so was linked against
    Dl_info info;
    memset(&info, 0, sizeof(info));
    const void* sym = reinterpret_cast<const void*>(&hipLaunchKernel);
    if (!dladdr(sym, &info) || !info.dli_fname) return fail(EWK_EHIP, "dladdr(hipLaunchKernel) failed");
    if (path && cap > 0) {
        strncpy(path, info.dli_fname, (size_t)cap - 1);
        path[cap - 1] = 0;
    }
    if (hip_version) {
        int v = -1;
        if (hipRuntimeGetVersion(&v) != hipSuccess) v = -1;
        *hip_version = v;
    }
    return EWK_OK;
}

int ewk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void ewk_destroy(ewk_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->sstream) (void)hipStreamSynchronize(e->sstream);
    // what no DevBuf or PinnedStage owns: those go with `delete e` below -- by then the device is
    // set and the streams are idle and destroyed, so nothing can still read what they free
    (void)hipFree(e->d_tab);
    (void)hipFree(e->d_tab64);
    (void)hipFree(e->d_tmpl);
    (void)hipFree(e->d_work);
    (void)hipFree(e->d_compact);
    (void)hipFree(e->d_ring);
    (void)hipFree(e->d_brms);
    (void)hipFree(e->d_sorted);
    (void)hipFree(e->d_trees);
    (void)hipFree(e->d_st);
    (void)hipFree(e->d_events);
    (void)hipFree(e->d_evc);
    if (e->h_poll) (void)hipHostFree(e->h_poll);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->cstream) (void)hipStreamDestroy(e->cstream);
    if (e->sstream) (void)hipStreamDestroy(e->sstream);
    for (int b = 0; b < 2; ++b) {
        if (e->bank_done[b]) (void)hipEventDestroy(e->bank_done[b]);
        if (e->gate_evt[b]) (void)hipEventDestroy(e->gate_evt[b]);
        if (e->score_evt[b]) (void)hipEventDestroy(e->score_evt[b]);
    }
    for (auto& pairs : e->ev)   // profiling brackets nobody read
        for (auto& p : pairs) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
    for (hipEvent_t x : e->ev_pool) (void)hipEventDestroy(x);
    delete e;
}

int ewk_create(ewk_engine** out, int device, int32_t n_streams, const ewk_config* cfg) {
    if (!out) return fail(EWK_EINVAL, "out is NULL");
    *out = nullptr;
    ewk_config c;
    if (cfg) c = *cfg;
    else ewk_default_config(&c);
    if (c.sample_rate != 16000) return fail(EWK_EINVAL, "sample_rate must be 16000 (SoundBuffer.FREQUENCY)");
    if (c.buffer_seconds <= 0) return fail(EWK_EINVAL, "buffer_seconds must be positive");
    if (c.block <= 0 || c.block > 8192) return fail(EWK_EINVAL, "block must be in [1, 8192]");
    if (c.tick_seconds <= 0) return fail(EWK_EINVAL, "tick_seconds must be positive");
    if (c.pre_speech_silence <= 0) return fail(EWK_EINVAL, "pre_speech_silence must be positive");
    if (c.speech_duration_min <= 0) return fail(EWK_EINVAL, "speech_duration_min must be positive");
    if (c.speech_duration_max <= 0) return fail(EWK_EINVAL, "speech_duration_max must be positive");
    if (c.speech_duration_min > c.speech_duration_max)
        return fail(EWK_EINVAL, "speech_duration_min must be <= speech_duration_max");
    if (c.post_speech_silence <= 0) return fail(EWK_EINVAL, "post_speech_silence must be positive");
    if (n_streams < 0) return fail(EWK_EINVAL, "n_streams must be >= 0");
    if (c.ring_format != EWK_RING_F32 && c.ring_format != EWK_RING_I16)
        return fail(EWK_EINVAL, "ring_format must be EWK_RING_F32 or EWK_RING_I16");
    const int64_t ring_len = (int64_t)c.buffer_seconds * c.sample_rate;
    if (ring_len > INT32_MAX / 2) return fail(EWK_EINVAL, "buffer_seconds too large");
    const int64_t seg_need = segment_need(c, ring_len, c.speech_duration_max, c.post_speech_silence, c.padding);
    if (c.ring_samples != 0) {
        if (c.ring_samples < 0 || c.ring_samples > ring_len)
            return fail(EWK_EINVAL, "ring_samples must be in [0, buffer_seconds * sample_rate]");
        if (c.ring_samples < ring_len) {
            if (ring_len % c.block != 0 || c.ring_samples % c.block != 0)
                return fail(EWK_EINVAL, "a compact ring (ring_samples) needs block to divide both rings");
            if (gate_stage_len(c.block, (int64_t)(0.1 * (double)c.sample_rate)) < c.block)
                return fail(EWK_EINVAL, "a compact ring (ring_samples) needs block <= 4096");
            if (c.ring_samples < seg_need + c.block || c.ring_samples < (int64_t)(0.1 * (double)c.sample_rate))
                return fail(EWK_EINVAL, "ring_samples must hold the longest segment request plus one tick (" +
                                            std::to_string(seg_need + c.block) + " samples for this config)");
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(EWK_ENODEV, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(EWK_ENODEV, "device index out of range");
    HIP_TRY(hipSetDevice(device));

    ewk_engine* e = new ewk_engine();
    e->device = device;
    e->cfg = c;
    e->n_streams = n_streams;
    e->ring_len = ring_len;
    e->sring_len = c.ring_samples > 0 ? (int64_t)c.ring_samples : ring_len;
    e->ring_es = c.ring_format == EWK_RING_I16 ? sizeof(int16_t) : sizeof(float);
    e->n_blocks = (int32_t)(e->ring_len / c.block);
    e->n_last = (int64_t)(0.1 * (double)c.sample_rate);   // int(0.1 * FREQUENCY)
    auto bail = [&](hipError_t err, const char* what) {
        std::string m = std::string(what) + ": " + hipGetErrorString(err);
        ewk_destroy(e);
        return fail(err == hipErrorOutOfMemory ? EWK_ENOMEM : EWK_EHIP, m);
    };
    hipError_t err;
    if ((err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return bail(err, "stream");
    if ((err = hipStreamCreateWithFlags(&e->cstream, hipStreamNonBlocking)) != hipSuccess) return bail(err, "stream");
    if ((err = hipStreamCreateWithFlags(&e->sstream, hipStreamNonBlocking)) != hipSuccess) return bail(err, "stream");
    for (int b = 0; b < 2; ++b) {
        if ((err = hipEventCreateWithFlags(&e->gate_evt[b], hipEventDisableTiming)) != hipSuccess) return bail(err, "event");
        if ((err = hipEventCreateWithFlags(&e->score_evt[b], hipEventDisableTiming)) != hipSuccess) return bail(err, "event");
    }
    for (int b = 0; b < 2; ++b)
        if ((err = hipEventCreateWithFlags(&e->bank_done[b], hipEventDisableTiming)) != hipSuccess)
            return bail(err, "event");
    {
        std::vector<unsigned char> buf(sizeof(Tables));
        Tables* t = reinterpret_cast<Tables*>(buf.data());
        build_tables(t);
        if (!t->ok) {
            ewk_destroy(e);
            return fail(EWK_EHIP, "mel filterbank does not fit the kernel's band layout");
        }
        if ((err = hipMalloc(&e->d_tab, sizeof(Tables))) != hipSuccess) return bail(err, "tables");
        if ((err = hipMemcpy(e->d_tab, t, sizeof(Tables), hipMemcpyHostToDevice)) != hipSuccess) return bail(err, "tables");
        std::vector<unsigned char> buf64(sizeof(Tables64));
        Tables64* t64 = reinterpret_cast<Tables64*>(buf64.data());
        build_tables64(t64);
        for (int m = 0; m < NMEL; ++m)
            if (t64->mel_off[m + 1] - t64->mel_off[m] > (m < NMEL / 2 ? kRsMelWLo : kRsMelW)) {
                ewk_destroy(e);
                return fail(EWK_EHIP, "mel filterbank band wider than the fp64 path's window (kRsMelWLo / kRsMelW)");
            }
        if ((err = hipMalloc(&e->d_tab64, sizeof(Tables64))) != hipSuccess) return bail(err, "tables64");
        if ((err = hipMemcpy(e->d_tab64, t64, sizeof(Tables64), hipMemcpyHostToDevice)) != hipSuccess)
            return bail(err, "tables64");
    }
    if ((err = hipMalloc(&e->d_tmpl, 2 * NMFCC * sizeof(float))) != hipSuccess) return bail(err, "template");
    if ((err = reserve_rescore(e, 4096)) != hipSuccess) return bail(err, "rescore slots");
    if ((err = reserve_parts(e, 16384)) != hipSuccess) return bail(err, "rescore parts");
    if ((err = hipMalloc(&e->d_work, kWorkInts * sizeof(int32_t))) != hipSuccess) return bail(err, "work counter");
    if ((err = hipMemset(e->d_work, 0, kWorkInts * sizeof(int32_t))) != hipSuccess) return bail(err, "work counter");
    if (n_streams > 0) {
        const size_t ring_bytes = (size_t)n_streams * e->sring_len * e->ring_es;
        if ((err = hipMalloc(&e->d_ring, ring_bytes)) != hipSuccess) return bail(err, "ring");
        if ((err = hipMalloc(&e->d_brms, (size_t)n_streams * std::max(1, e->n_blocks) * sizeof(double))) != hipSuccess)
            return bail(err, "block rms");
        if ((err = hipMalloc(&e->d_sorted, (size_t)n_streams * 2 * std::max(1, e->n_blocks) * sizeof(double))) !=
            hipSuccess)
            return bail(err, "sorted block rms");
        if ((err = hipMalloc(&e->d_st, (size_t)n_streams * sizeof(GateStream))) != hipSuccess) return bail(err, "state");
        {
            std::vector<PwTree> tr(kNumTrees);
            const int64_t lens[2] = {c.block, e->n_last};
            for (int k = 0; k < 2; ++k) {
                const int64_t n = std::min<int64_t>(lens[k], e->ring_len);
                build_pw_tree(n > kPwChunk ? kPwChunk : 0, &tr[2 * k]);
                const int64_t r = n % kPwChunk;
                build_pw_tree((int)(n > kPwChunk ? (r ? r : kPwChunk) : n), &tr[2 * k + 1]);
            }
            if ((err = hipMalloc(&e->d_trees, kNumTrees * sizeof(PwTree))) != hipSuccess) return bail(err, "trees");
            if ((err = hipMemcpy(e->d_trees, tr.data(), kNumTrees * sizeof(PwTree), hipMemcpyHostToDevice)) != hipSuccess)
                return bail(err, "trees");
            e->gate_val_len = gate_val_len(tr.data(), e->n_blocks);
            e->gate_tree_kind[0] = pw_tree_kind(tr[kTreeBlockRem]);
            e->gate_tree_kind[1] = pw_tree_kind(tr[kTreeLastRem]);
        }
        e->ev_cap = std::max(4096, 4 * n_streams);
        if ((err = reserve_rescore(e, e->ev_cap)) != hipSuccess) return bail(err, "rescore list");
        // a tick lists ~4 % of its events (the configs[2] recipe), ~20 chunks each
        if ((err = reserve_parts(e, std::min(262144, std::max(16384, e->ev_cap / 2)))) != hipSuccess)
            return bail(err, "rescore parts");
        if ((err = hipMalloc(&e->d_events, 2 * (size_t)e->ev_cap * sizeof(ewk_event))) != hipSuccess)
            return bail(err, "events");
        if ((err = hipMalloc(&e->d_evc, 8 * sizeof(int32_t))) != hipSuccess) return bail(err, "event counters");
        e->gate_stage = gate_stage_len(c.block, e->n_last);
        {
            // opt-in (EWK_SCORE_OVERLAP=1): measured on MI355X the extra stream/event calls
            // per tick cost more host time than the concurrency saves (scripts/mb_stream.py)
            const char* env = getenv("EWK_SCORE_OVERLAP");
            e->overlap_want = env && env[0] == '1';
            set_launch_ticks(e, seg_need);
            // EWK_GATE_GRID_MAX=<workgroups>: a smaller gate grid than the built-in maximum (a wave
            // then walks several streams at sizes a test can afford); unset or invalid: the maximum
            const char* cap = getenv("EWK_GATE_GRID_MAX");
            if (cap && cap[0]) {
                char* end = nullptr;
                const long v = strtol(cap, &end, 10);
                if (end && *end == 0 && v > 0 && v <= INT32_MAX) e->gate_grid_cap = (int32_t)v;
            }
        }
        int rc = ewk_reset_streams(e);
        if (rc != EWK_OK) {
            std::string m = g_err;
            ewk_destroy(e);
            return fail(rc, m);
        }
    }
    if ((err = hipStreamSynchronize(e->stream)) != hipSuccess) return bail(err, "sync");
    *out = e;
    return EWK_OK;
}

int ewk_sync(ewk_engine* e) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipStreamSynchronize(e->sstream));
    return EWK_OK;
}

void* ewk_stream_handle(ewk_engine* e) { return e ? (void*)e->stream : nullptr; }

int ewk_set_template(ewk_engine* e, const float* mean20, const float* std20) {
    if (!e || !mean20 || !std20) return fail(EWK_EINVAL, "NULL argument");
    memcpy(e->h_tmpl, mean20, NMFCC * sizeof(float));
    memcpy(e->h_tmpl + NMFCC, std20, NMFCC * sizeof(float));
    {   // cblas_sdot for n = 20: float products accumulated in double, rounded to float
        double am = 0.0, as = 0.0;
        for (int i = 0; i < NMFCC; ++i) {
            const float pm = mean20[i] * mean20[i], ps = std20[i] * std20[i];
            am += (double)pm;
            as += (double)ps;
        }
        e->uu_m32 = (float)am;
        e->uu_s32 = (float)as;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(join_scoring(e, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_tmpl, e->h_tmpl, sizeof(e->h_tmpl), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->has_tmpl = true;
    return EWK_OK;
}

int ewk_set_similarity_threshold(ewk_engine* e, double threshold) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (!(threshold == threshold)) return fail(EWK_EINVAL, "threshold is NaN");
    e->cfg.similarity_threshold = threshold;
    return EWK_OK;
}

int ewk_get_template(ewk_engine* e, float* mean20, float* std20) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (!e->has_tmpl) return fail(EWK_ENOTEMPLATE, "No reference word set. Call set_reference() first.");
    if (mean20) memcpy(mean20, e->h_tmpl, NMFCC * sizeof(float));
    if (std20) memcpy(std20, e->h_tmpl + NMFCC, NMFCC * sizeof(float));
    return EWK_OK;
}

int ewk_profile_enable(ewk_engine* e, int32_t on) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    e->prof = on != 0;
    return EWK_OK;
}

int ewk_profile_read(ewk_engine* e, int32_t kind, double* total_ms, int64_t* launches) {
    if (!e || !total_ms || !launches) return fail(EWK_EINVAL, "NULL argument");
    if (kind < 0 || kind > 5) return fail(EWK_EINVAL, "kind must be 0, 1, 2, 3, 4 or 5");
    HIP_TRY(hipSetDevice(e->device));
    double tot = 0.0;
    for (auto& p : e->ev[kind]) {
        HIP_TRY(hipEventSynchronize(p.second));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        tot += ms;
        e->ev_pool.push_back(p.first);
        e->ev_pool.push_back(p.second);
    }
    *total_ms = tot;
    *launches = (int64_t)e->ev[kind].size();
    e->ev[kind].clear();
    return EWK_OK;
}

int ewk_gate_launch_info(ewk_engine* e, int32_t* rb, int32_t* dma, int32_t* prof, int32_t* lsn,
                         int32_t* block_tree_kind, int32_t* last_tree_kind) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (rb) *rb = e->gate_last.rb;
    if (dma) *dma = e->gate_last.dma;
    if (prof) *prof = e->gate_last.prof;
    if (lsn) *lsn = e->gate_last.lsn;
    if (block_tree_kind) *block_tree_kind = e->gate_tree_kind[0];
    if (last_tree_kind) *last_tree_kind = e->gate_tree_kind[1];
    return EWK_OK;
}

}  // extern "C"
