// demod_scope_host.hip -- the host side of the demod scope (jsdr_demod_scope_*): the batch call through demod_run
// (demod_call.hip), then demod.paintComponent's trace and spectrum (:509-558) for every frame of it, in passes of the scope's
// kernels (demod_scope.hip, through demod.h's launchers).  Host code only.
#include "demod_handle.h"

// ---- the demod scope: demod.paintComponent's trace and spectrum (:509-558) for every frame of a batch call
// the column schedules of (n, width) in the reference's float arithmetic; any of the four arrays may be null.  Refuses a pair
// at which the reference would index outside sam[] (getAbsMax, :569-578) or psd[] (getMax, :560-567).
static int demod_scope_layout(const char *who, int n, int width, int32_t *tf, int32_t *tc, int32_t *sf, int32_t *sc)
{
    const float scale = dscope_scale(n, width), pi = dscope_pi(n, width);
    const int tcnt = (int)scale, scnt = (int)pi;
    for (int x = 0; x < width; x++) {
        const bool col = x < width - 1;
        const int i = col ? dscope_trace_first(x, scale) : 0;
        // sam[2i] always; then sam[2i + 1], sam[2i + 3], .. below 2i + (int)scale: the Qs of samples i .. i + tcnt/2 - 1
        JSDR_REQUIRE(!col || (i >= 0 && i < n && i + tcnt / 2 <= n),
                     "%s: n=%d, width=%d: trace column %d would read sam[] from sample %d on, %d values", who, n, width, x, i, tcnt);
        if (tf) tf[x] = i;
        if (tc) tc[x] = col ? tcnt : 0;
        const int k = x ? dscope_spec_first(x, pi) : 0;
        JSDR_REQUIRE(k >= 0 && k < n && (!x || k + scnt <= n),
                     "%s: n=%d, width=%d: spectrum column %d would read psd[] from bin %d on, %d values", who, n, width, x, k, scnt);
        if (sf) sf[x] = k;
        if (sc) sc[x] = x ? scnt : 0;
    }
    return JSDR_OK;
}

static int demod_scope_run(const char *who, jsdr_demod *h, bool f32in, const int16_t *raw_dev, const float *rawf_dev,
                           int64_t stride_i16, int64_t L, int ic, int qc, int16_t *audio_dev, int64_t audio_stride_i16, int width, int height,
                           int32_t *trace_dev, int32_t *spec_dev, float *dbg_dev, hipStream_t st)
{
    const char *in_name = f32in ? "iq_dev" : "raw_dev", *stride_name = f32in ? "stream_stride_f32" : "stream_stride_i16";
    // every refusal before any device work, the handle and its state untouched
    JSDR_REQUIRE(h, "%s: null handle", who);
    JSDR_REQUIRE(raw_dev || rawf_dev, "%s: null %s", who, in_name);
    JSDR_REQUIRE(audio_dev, "%s: null audio_dev", who);
    JSDR_REQUIRE(width >= 1 && width <= DSCOPE_WIDTH_MAX, "%s: width=%d outside 1..%d", who, width, (int)DSCOPE_WIDTH_MAX);
    JSDR_REQUIRE(height >= 0, "%s: height=%d is negative", who, height);
    JSDR_REQUIRE(!h->chan, "%s: a channel handle (jsdr_demod_create_channels) has no scope", who);
    JSDR_REQUIRE(!spec_dev || (h->n >= 2 && h->n <= 20000),
                 "%s: spec_dev with a frame of %d samples: jsdr_fft_create takes 2 .. 20000", who, h->n);
    JSDR_REQUIRE((stride_i16 & 1) == 0 && (h->nstreams == 1 || (stride_i16 >= 0 && stride_i16 / 2 >= L)),
                 "%s: %s=%lld is odd or below a stream's nsamples=%lld", who, stride_name, (long long)stride_i16, (long long)L);
    JSDR_REQUIRE((audio_stride_i16 & 1) == 0 && (h->nstreams == 1 || (audio_stride_i16 >= 0 && audio_stride_i16 / 2 >= L)),
                 "%s: audio_stride_i16=%lld is odd or below a stream's nsamples=%lld", who, (long long)audio_stride_i16, (long long)L);
    JSDR_REQUIRE(h->n > 0 && L > 0 && L <= h->max_batch && L % h->n == 0,
                 "%s: nsamples=%lld must be a positive multiple of the frame (%d) and at most max_batch_samples=%lld", who,
                 (long long)L, h->n, h->max_batch);
    if (trace_dev || spec_dev)
        if (demod_scope_layout(who, h->n, width, nullptr, nullptr, nullptr, nullptr) != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE((reinterpret_cast<uintptr_t>(dbg_dev) & 15) == 0, "%s: dbg_dev is not aligned to 16 bytes", who);
    JSDR_REQUIRE((reinterpret_cast<uintptr_t>(trace_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(spec_dev) & 3) == 0,
                 "%s: trace_dev or spec_dev is not aligned to 4 bytes", who);
    if (!trace_dev && !spec_dev && !dbg_dev) {  // the batch call itself
        h->scope.kernel.clear();
        return demod_run(h, f32in, raw_dev, rawf_dev, stride_i16, L, ic, qc, audio_dev, audio_stride_i16, st);
    }
    jsdr_demod::Scope &sc = h->scope;
    const int n = h->n, nfr = (int)(L / n);
    const long long rows = (long long)h->nstreams * nfr;
    // frames of a pass: what DSCOPE_SCRATCH_BYTES holds of dbg (8n), final floats (4n) and PSD (4n + 8) rows -- one frame at least
    long long fpp = (long long)(DSCOPE_SCRATCH_BYTES / (16 * (size_t)n + 8));
    if (fpp < 1) fpp = 1;
    if (sc.chunk > 0 && sc.chunk < fpp) fpp = sc.chunk;
    if (fpp > rows) fpp = rows;
    // scratch, the schedule table and the FFT handle: before the call's own work, so that a failure leaves the state as it was
    const size_t want_dbg = dbg_dev ? 0 : (size_t)fpp * n, want_fin = trace_dev ? (size_t)fpp * n : 0,
                 want_psd = spec_dev ? (size_t)fpp * ((size_t)n + 2) : 0;
    if (want_dbg > sc.dbg.n || want_fin > sc.fin.n || want_psd > sc.psd.n || !sc.tab.p) {
        JSDR_HIP_TRY(hipDeviceSynchronize());  // earlier calls may still use the smaller rows
        if (want_dbg > sc.dbg.n && sc.dbg.alloc(want_dbg) != JSDR_OK) return JSDR_ERR;
        if (want_fin > sc.fin.n && sc.fin.alloc(want_fin) != JSDR_OK) return JSDR_ERR;
        if (want_psd > sc.psd.n && sc.psd.alloc(want_psd) != JSDR_OK) return JSDR_ERR;
        if (!sc.tab.p) {
            if (sc.tab.alloc(4 * (size_t)DSCOPE_WIDTH_MAX) != JSDR_OK) return JSDR_ERR;
            sc.tab_width = 0;
        }
    }
    if (spec_dev && !sc.fft.h) {
        jsdr_fft *f = nullptr;
        if (jsdr_fft_create(&f, n, h->rate) != JSDR_OK) return JSDR_ERR;
        sc.fft.adopt(f);
    }
    // what the passes read, as it is BEFORE the call: demod_run leaves the other halves of hist / lilq and this call's
    // carrier table alone until the next call (the call after next, for the table)
    const int set = carrier_set_next(h);
    DemodArgs a = demod_args_of(h, set, raw_dev, rawf_dev, stride_i16, L, ic, qc);
    a.d = nullptr;
    a.fmax_bits = nullptr;
    if (demod_run(h, f32in, raw_dev, rawf_dev, stride_i16, L, ic, qc, audio_dev, audio_stride_i16, st) != JSDR_OK) return JSDR_ERR;
    if ((trace_dev || spec_dev) && sc.tab_width != width) {  // on the caller's stream, behind the previous call's readers
        sc.tab_width = 0;
        if (launch_demod_scope_layout(n, width, sc.tab.p, st) != JSDR_OK) return JSDR_ERR;
        sc.tab_width = width;
    }
    for (long long r0 = 0; r0 < rows; r0 += fpp) {
        const int nr = (int)(rows - r0 < fpp ? rows - r0 : fpp);
        float2 *dbg_rows = dbg_dev ? reinterpret_cast<float2 *>(dbg_dev) + (size_t)r0 * n : sc.dbg.p;
        if (launch_demod_scope_front(a, f32in, h->stats.p, r0, nr, dbg_rows, trace_dev ? sc.fin.p : nullptr, st) != JSDR_OK)
            return JSDR_ERR;
        if (trace_dev &&
            launch_demod_trace(sc.fin.p, dbg_rows, n, a.c.mode == MODE_OFF, nr, width, height / 4, sc.tab.p,
                               trace_dev + (size_t)r0 * width, st) != JSDR_OK)
            return JSDR_ERR;
        if (spec_dev) {
            if (jsdr_fft_batch_f32(sc.fft.h, reinterpret_cast<const float *>(dbg_rows), nr, sc.psd.p, st) != JSDR_OK) return JSDR_ERR;
            if (launch_demod_spec(sc.psd.p, n, nr, width, height / 2, sc.tab.p, spec_dev + (size_t)r0 * width, st) != JSDR_OK)
                return JSDR_ERR;
        }
    }
    if (a.c.dodwn && carrier_end(h, set, st) != JSDR_OK) return JSDR_ERR;  // the passes read the carrier table too
    sc.kernel = "k_demod_scope_front";
    if (trace_dev) sc.kernel += "+k_demod_trace";
    if (spec_dev) sc.kernel += std::string("+") + jsdr_fft_kernel(sc.fft.h) + "+k_demod_spec";
    return JSDR_OK;
}

extern "C" {

int jsdr_demod_scope_layout(int n, int width, int32_t *trace_first, int32_t *trace_count, int32_t *spec_first, int32_t *spec_count,
                            int cap)
{
    JSDR_REQUIRE(n >= 1, "jsdr_demod_scope_layout: n=%d must be positive", n);
    JSDR_REQUIRE(width >= 1 && width <= DSCOPE_WIDTH_MAX, "jsdr_demod_scope_layout: width=%d outside 1..%d", width,
                 (int)DSCOPE_WIDTH_MAX);
    JSDR_REQUIRE(cap >= width || !(trace_first || trace_count || spec_first || spec_count),
                 "jsdr_demod_scope_layout: cap=%d is below width=%d", cap, width);
    // (checked first, so that a refused pair writes nothing)
    if (demod_scope_layout("jsdr_demod_scope_layout", n, width, nullptr, nullptr, nullptr, nullptr) != JSDR_OK) return JSDR_ERR;
    return demod_scope_layout("jsdr_demod_scope_layout", n, width, trace_first, trace_count, spec_first, spec_count);
}

int jsdr_demod_scope_i16(jsdr_demod *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc,
                         int16_t *audio_dev, int64_t audio_stride_i16, int width, int height, int32_t *trace_dev,
                         int32_t *spec_dev, float *dbg_dev, void *stream)
{
    return demod_scope_run("jsdr_demod_scope_i16", h, false, raw_dev, nullptr, stream_stride_i16, nsamples, ic, qc, audio_dev,
                           audio_stride_i16, width, height, trace_dev, spec_dev, dbg_dev, as_stream(stream));
}

int jsdr_demod_scope_f32(jsdr_demod *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples, int16_t *audio_dev,
                         int64_t audio_stride_i16, int width, int height, int32_t *trace_dev, int32_t *spec_dev, float *dbg_dev,
                         void *stream)
{
    return demod_scope_run("jsdr_demod_scope_f32", h, true, nullptr, iq_dev, stream_stride_f32, nsamples, 0, 0, audio_dev,
                           audio_stride_i16, width, height, trace_dev, spec_dev, dbg_dev, as_stream(stream));
}

int jsdr_demod_scope_chunk(jsdr_demod *h, int frames_per_pass)
{
    JSDR_REQUIRE(h, "jsdr_demod_scope_chunk: null handle");
    JSDR_REQUIRE(frames_per_pass >= 0, "jsdr_demod_scope_chunk: frames_per_pass=%d is negative", frames_per_pass);
    h->scope.chunk = frames_per_pass;
    return JSDR_OK;
}

const char *jsdr_demod_scope_kernel(jsdr_demod *h) { return h ? h->scope.kernel.c_str() : ""; }

}  // extern "C"
