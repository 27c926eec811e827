// ewk_engine_resample.cpp -- the C ABI's input-rate resampler (ewk_resample.hip): filter design,
// the one-shot ewk_resample, ewk_set_input_rate and the resample stage of a push.
#include "ewk_engine.h"

using namespace ewk;

int ewk_resample_design(int32_t in_rate, int32_t out_rate, double* taps, int32_t cap, int32_t* n_taps, int32_t* up,
                        int32_t* down) {
    if (in_rate <= 0 || out_rate <= 0) return fail(EWK_EINVAL, "sample rates must be positive");
    int32_t u = 1, d = 1;
    resample_ratio(in_rate, out_rate, &u, &d);
    const int64_t n = 20 * (int64_t)std::max(u, d) + 1;
    if (n > 0x7fffffffLL) return fail(EWK_EINVAL, "the filter of this rate pair has more than 2^31 taps");
    if (up) *up = u;
    if (down) *down = d;
    if (n_taps) *n_taps = (int32_t)n;
    if (!taps || cap < n) return fail(EWK_EINVAL, "taps holds fewer than " + std::to_string(n) + " values");
    resample_taps(u, d, taps);
    return EWK_OK;
}

// The filter in_rate -> cfg.sample_rate in the kernel's layout.  Waits for the engine's stream
// before the taps of another rate replace those it may still read.
static int rs_prepare(ewk_engine* e, ewk_engine::RsFilter& f, int32_t in_rate, bool streaming) {
    if (f.rate == in_rate && f.taps.p) return EWK_OK;
    int32_t up = 1, down = 1;
    resample_ratio(in_rate, e->cfg.sample_rate, &up, &down);
    const int64_t half = 10 * (int64_t)std::max(up, down), J = 2 * half / up + 1;
    const int threads = resample_threads(up);
    const int64_t span = threads ? resample_span(up, down, (int32_t)std::min<int64_t>(J, kRsMaxSpan), threads) : 0;
    if (!threads || J + 1 > kRsMaxSpan || span > kRsMaxSpan)
        return fail(EWK_EINVAL, "the filter " + std::to_string(in_rate) + " -> " + std::to_string(e->cfg.sample_rate) +
                                    " Hz (up " + std::to_string(up) + ", down " + std::to_string(down) +
                                    ") is over the size the resampler supports (up <= " + std::to_string(kRsMaxThreads) +
                                    ", " + std::to_string(kRsMaxSpan) + " staged samples per workgroup)");
    // streaming: the whole-signal resample delayed by ceil(half / down) samples
    const int64_t c0 = streaming ? half - (half + down - 1) / down * down : half;
    std::vector<double> h((size_t)(2 * half + 1)), tt((size_t)(J * up), 0.0);
    resample_taps(up, down, h.data());
    for (int64_t j = 0; j < J; ++j)
        for (int64_t p = 0; p < up; ++p)
            if (p + j * up <= 2 * half) tt[(size_t)(j * up + p)] = h[(size_t)(p + j * up)];
    HIP_TRY(hipStreamSynchronize(e->stream));
    f.rate = 0;
    HIP_TRY(f.taps.reserve(tt.size()));
    HIP_TRY(hipMemcpy(f.taps.p, tt.data(), tt.size() * sizeof(double), hipMemcpyHostToDevice));
    f.up = up;
    f.down = down;
    f.half = (int32_t)half;
    f.c0 = c0;
    f.J = (int32_t)J;
    f.H = (int32_t)J + 1;
    f.threads = threads;
    f.span = (int32_t)span;
    f.rate = in_rate;
    return EWK_OK;
}

// Launch arguments with the filter's fields set, the rest zero.
static ResampleArgs filter_args(const ewk_engine::RsFilter& f) {
    ResampleArgs r;
    memset(&r, 0, sizeof(r));
    r.taps = f.taps.p;
    r.up = f.up;
    r.down = f.down;
    r.J = f.J;
    r.H = f.H;
    r.c0 = f.c0;
    r.threads = f.threads;
    r.span = f.span;
    return r;
}

int ewk::resample_ticks(ewk_engine* e, TickSrc* src, int32_t rows, int32_t n_ticks, const int32_t* d_list,
                        hipStream_t s) {
    const size_t per_stream = (size_t)n_ticks * e->cfg.block;
    if (per_stream * rows > e->rs_out.cap) {
        HIP_TRY(hipStreamSynchronize(s));   // an earlier gate launch may still read the old buffer
        HIP_TRY(e->rs_out.reserve(per_stream * rows));
    }
    ResampleArgs r = filter_args(e->rs_in);
    ResampleG711 g{nullptr, 0};
    if (src->kind.type == kSampleG711) g = ResampleG711{static_cast<const uint8_t*>(src->p), src->kind.law};
    else if (src->kind.type == kSamplePcm16) r.in16 = static_cast<const int16_t*>(src->p);
    else r.in = static_cast<const float*>(src->p);
    r.stride = src->stride;
    r.tick_stride = src->tick_stride;
    r.in_block = e->rs_in_block;
    r.n_in = (int64_t)n_ticks * e->rs_in_block;
    r.hist = e->rs_hist.p;
    r.out = e->rs_out.p;
    r.out_stride = (int64_t)per_stream;
    r.n_out = (int64_t)per_stream;
    r.rows = rows;
    r.ids = d_list;
    r.fresh = e->rs_flags.p;   // per stream once there are flags, else rs_fresh for all
    r.n_zero = (e->rs_flags.p || e->rs_fresh) ? e->rs_delay : 0;
    {
        ProfScope ps(e, 3, s);
        HIP_TRY(launch_resample(r, s, g));
        HIP_TRY(launch_resample_save(r, e->rs_hist.p, e->rs_flags.p, s, g));
    }
    if (!d_list) e->rs_fresh = false;   // (a subset push made the flags: rs_fresh is not read again)
    *src = TickSrc{e->rs_out.p, kKindF32, (int64_t)per_stream, e->cfg.block};
    return EWK_OK;
}

int ewk_resample(ewk_engine* e, const float* in, int64_t n_in, int32_t in_rate, float* out, int64_t cap,
                 int64_t* n_out, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n_out) *n_out = 0;
    if (in_rate <= 0) return fail(EWK_EINVAL, "sample rates must be positive");
    if (n_in < 0 || n_in >= (1LL << 40)) return fail(EWK_EINVAL, "n_in must be in [0, 2^40)");
    int32_t up = 1, down = 1;
    resample_ratio(in_rate, e->cfg.sample_rate, &up, &down);
    const int64_t no = (n_in * up + down - 1) / down;   // ceil(n_in * out / in)
    if (n_out) *n_out = no;
    if (cap < no) return fail(EWK_EINVAL, "out holds fewer than " + std::to_string(no) + " samples");
    if (no == 0) return EWK_OK;
    if (!in || !out) return fail(EWK_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const bool in_dev = (flags & EWK_PCM_DEVICE) != 0, out_dev = (flags & EWK_OUT_DEVICE) != 0;
    if (up == 1 && down == 1) {   // the engine's own rate: a copy (as resample_poly returns it)
        HIP_TRY(hipMemcpyAsync(out, in, (size_t)n_in * sizeof(float), hipMemcpyDefault, s));
        if (!in_dev || !out_dev) HIP_TRY(hipStreamSynchronize(s));
        return EWK_OK;
    }
    int rc = rs_prepare(e, e->rs_one, in_rate, false);
    if (rc) return rc;
    DevBuf<float> d_in, d_out;
    if (!in_dev) {
        HIP_TRY(d_in.reserve((size_t)n_in));
        HIP_TRY(hipMemcpyAsync(d_in.p, in, (size_t)n_in * sizeof(float), hipMemcpyHostToDevice, s));
    }
    if (!out_dev) HIP_TRY(d_out.reserve((size_t)no));
    ResampleArgs r = filter_args(e->rs_one);
    r.in = in_dev ? in : d_in.p;
    r.in_block = n_in;
    r.n_in = n_in;
    r.out = out_dev ? out : d_out.p;
    r.out_stride = no;
    r.n_out = no;
    r.rows = 1;
    {
        ProfScope ps(e, 3, s);
        HIP_TRY(launch_resample(r, s));
    }
    if (!out_dev) HIP_TRY(hipMemcpyAsync(out, d_out.p, (size_t)no * sizeof(float), hipMemcpyDeviceToHost, s));
    if (!in_dev || !out_dev) HIP_TRY(hipStreamSynchronize(s));   // (the staging buffers die on return)
    return EWK_OK;
}

int ewk_set_input_rate(ewk_engine* e, int32_t in_rate) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (in_rate < 0) return fail(EWK_EINVAL, "in_rate must be >= 0");
    HIP_TRY(hipSetDevice(e->device));
    if (in_rate == 0 || in_rate == e->cfg.sample_rate) {
        if (!e->rs_on) return EWK_OK;
        HIP_TRY(hipStreamSynchronize(e->stream));
        e->rs_on = false;
        e->drop_all_pending();   // (pending chunk samples were counted at the old rate)
        return EWK_OK;
    }
    if (e->ring_es == sizeof(int16_t))
        return fail(EWK_EINVAL, "an int16 ring (EWK_RING_I16) stores PCM16 as delivered: resampled samples are not int16");
    int32_t up = 1, down = 1;
    resample_ratio(in_rate, e->cfg.sample_rate, &up, &down);
    if (((int64_t)e->cfg.block * down) % up)
        return fail(EWK_EINVAL, "a tick of " + std::to_string(e->cfg.block) + " samples at " +
                                    std::to_string(e->cfg.sample_rate) + " Hz is not a whole number of samples at " +
                                    std::to_string(in_rate) + " Hz");
    e->rs_on = false;   // (a failure below leaves the engine at its own rate)
    e->drop_all_pending();   // the unit of a pending chunk count changes with the rate, also on that failure
    int rc = rs_prepare(e, e->rs_in, in_rate, true);   // waits for the pushes so far when the rate changes
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const ewk_engine::RsFilter& f = e->rs_in;
    const size_t nh = (size_t)e->n_streams * f.H;
    if (nh > e->rs_hist.cap) HIP_TRY(e->rs_hist.reserve(nh));
    HIP_TRY(hipMemset(e->rs_hist.p, 0, e->rs_hist.cap * sizeof(float)));
    HIP_TRY(e->rs_out.reserve((size_t)e->n_streams * e->cfg.block));
    if (e->desync || e->rs_flags.p) {   // streams on their own clocks: every one starts fresh
        HIP_TRY(e->rs_flags.reserve((size_t)e->n_streams));
        HIP_TRY(hipMemset(e->rs_flags.p, 1, e->rs_flags.cap));
    }
    e->rs_in_block = (int32_t)((int64_t)e->cfg.block * down / up);
    e->rs_delay = (int32_t)((f.half + down - 1) / down);
    e->rs_fresh = true;
    e->rs_on = true;
    return EWK_OK;
}

int ewk_input_rate_info(ewk_engine* e, int32_t* in_rate, int32_t* in_block, int32_t* delay) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (in_rate) *in_rate = e->rs_on ? e->rs_in.rate : e->cfg.sample_rate;
    if (in_block) *in_block = e->rs_on ? e->rs_in_block : e->cfg.block;
    if (delay) *delay = e->rs_on ? e->rs_delay : 0;
    return EWK_OK;
}
