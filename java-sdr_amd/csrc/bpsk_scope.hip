// bpsk_scope.hip -- what FUNcubeBPSKDemod.paintComponent's first panel (FUNcubeBPSKDemod.java:231-268) draws after receive() of
// a frame, and the five debug rings it draws from (:118-125), for every frame of a batch call: jsdr_bpsk_scope_i16 / _f32,
// jsdr_bpsk_scope_layout, jsdr_bpsk_scope_kernel.  Compiled with -ffp-contract=off like the pipeline's units: every product,
// sum and quotient is one IEEE double operation, in the reference's order.
//
// A scope call IS the batch call (jsdr_bpsk_batch_i16 / _f32, untouched) plus the passes below on the caller's stream:
//   k_bpsk_scope_front  one workgroup a tile of a frame: the input converted and mixed once with the call's own tuner schedule
//                       (:388-396) -- the `tuned` row, 16-byte stores -- then the 27-tap low-pass at the frame's decimated
//                       instants, newest first, products and sums separate (:479-483), x HOWARD (:486), stored straight into
//                       the slot of the `downSmpl` row where the sample is the last one of its frame to land there.  The 26
//                       samples before the call come from the handle's double-buffered input history.
//   k_bpsk_scope_walk   one lane a stream: RxDemodulate's bit clock (:533-593) again, sample by sample, over the (fi, fq) the
//                       batch call has just left in the handle's y buffer, from the clock state of BEFORE the call; it marks
//                       demodBits and demodRe (:549-551).  A second, plain statement of the tail -- k_tail / k_tail8 are not
//                       touched and not shared.
//   k_bpsk_scope_pts    one workgroup a row: the demodIQ ring image gathered from y, mi / mq under the strict compare of
//                       :232-238, then the painter's integers (:247-262).
// The clock state of before the call is copied on the handle's side stream ahead of the call's own tail kernel (the stream's
// order puts the copy behind the previous call's tail and in front of this one's), and the caller's stream waits for the
// copy's event: no host wait.  demodRe's marks are written in place, into the last two ints of the slot's pts entry, which
// k_bpsk_scope_pts reads before it writes the entry.
//
// A spectra call (jsdr_bpsk_scope_spectra_i16 / _f32) IS the scope call plus the painter's two spectra (:270-327): the kernels of
// bpsk_scope_spec.hip over the caller's `tuned` / `ds` rows where they are given, else over rows of the handle's own that
// k_bpsk_scope_front fills a pass of frames at a time -- the pass's geometry is the call's with its first frame moved on, and the
// 26 inputs in front of a pass that does not start the call are gathered by k_hist_in (launch_hist_in) as between two calls.
#include "bpsk_handle.h"
#include "bpsk_scope_spec.h"
#include <stdint.h>

namespace jsdr {
#pragma GCC visibility push(hidden)

enum { SCOPE_TILE = 1024, SCOPE_THREADS = 256 };

// where the frames of a call lie in the stream of decimated samples.  g counts RxDemodulate calls since the origin; the
// sample with absolute number a (since creation) is g = a - origin
struct ScopeGeom {
    long long n_in;    // samples taken before the call (a multiple of n)
    long long origin;  // decimated samples before the origin
    long long a0;      // decimated samples before the call, n_in / D
    long long nds;     // ... of the call
    int n, D, L, frames, nstreams;
};
// decimated samples before frame f of the call, since creation: output k (1-based) completes with sample D k - 1
__host__ __device__ inline long long scope_before(const ScopeGeom &g, long long f) { return (g.n_in + f * (long long)g.n) / g.D; }

struct ScopeFrontArgs {
    const int *raw;           // int16 pairs as dwords, [S][stride] (null: rawf)
    const float2 *rawf;
    long long stride_pairs;
    int ic, qc;
    const int2 *hist;         // [S][32] the 26 inputs before the call, in the call's input form
    const unsigned short *k9; // [26 + L] 9-bit tuner index of every sample (256: passed through, :395)
    const double *sc9;        // cos[0..256], sin[0..256], (1.0, 1.0) at 256
    double taps[DS_N];        // dsFilter
    double2 *tuned;           // [rows][n], or null
    double *ds;               // [rows][L][2], or null
};

template <bool F32IN>
__global__ __launch_bounds__(SCOPE_THREADS) void k_bpsk_scope_front(ScopeFrontArgs a, ScopeGeom g)
{
    __shared__ double sc[514];
    __shared__ double2 xm[SCOPE_TILE + 26];  // the tile's mixed samples behind their 26-sample halo
    const int tid = threadIdx.x;
    for (int i = tid; i < 514; i += SCOPE_THREADS) sc[i] = a.sc9[i];
    const int tiles = (g.n + SCOPE_TILE - 1) / SCOPE_TILE;
    const long long row = (long long)blockIdx.x / tiles;
    const int t = (int)((long long)blockIdx.x - row * tiles);
    const int s = (int)(row / g.frames);
    const int f = (int)(row - (long long)s * g.frames);
    const int t0 = t * SCOPE_TILE;
    const int len = (g.n - t0) < SCOPE_TILE ? (g.n - t0) : SCOPE_TILE;
    const long long base = (long long)f * g.n + t0;  // the call's index of the tile's sample 0
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const float2 *rawf = a.rawf + (long long)s * a.stride_pairs;
    const int2 *hist = a.hist + (long long)s * 32;
    __syncthreads();
    for (int i = tid; i < len + 26; i += SCOPE_THREADS) {
        const long long m = base - 26 + i;  // >= -26
        double di, dq;
        if constexpr (F32IN) {
            float2 v;
            if (m >= 0) {
                v = rawf[m];
            } else {
                const int2 h = hist[26 + m];
                v = make_float2(__int_as_float(h.x), __int_as_float(h.y));
            }
            di = (double)v.x;  // (double)buf[n*2]  :372
            dq = (double)v.y;
        } else {
            int w;
            if (m >= 0) {
                w = raw[m];
                const int si = java_short_add((int)(short)(w & 0xffff), a.ic);
                const int sq = java_short_add(w >> 16, a.qc);
                w = (si & 0xffff) | (sq << 16);
            } else {
                w = hist[26 + m].x;
            }
            di = (double)i16_to_float_java((int)(short)(w & 0xffff));
            dq = (double)i16_to_float_java(w >> 16);
        }
        const int k = a.k9[26 + m];
        const double2 v = make_double2(di * sc[k], dq * sc[257 + k]);  // :389-390, or :395 through the (1.0, 1.0) entry
        xm[i] = v;
        if (a.tuned && i >= 26) a.tuned[row * g.n + t0 + (i - 26)] = v;  // :471-472
    }
    if (!a.ds) return;
    __syncthreads();
    const double HOWARD = 0.9 * 32768.0;  // :469
    const long long A0 = g.n_in + base, A1 = A0 + len;        // the tile's samples, numbered since creation
    const long long klo = (A0 + g.D) / g.D, khi = A1 / g.D + 1;  // outputs k (1-based) with A0 <= D k - 1 < A1
    const long long gnext = scope_before(g, f + 1) - g.origin;   // G of the next frame
    for (long long k = klo + tid; k < khi; k += SCOPE_THREADS) {
        const long long gg = k - 1 - g.origin;
        if (gg + g.L < gnext) continue;  // a later sample of the frame takes the slot
        const int idx = (int)((long long)g.D * k - 1 - A0) + 26;
        double fi = 0.0, fq = 0.0;
#pragma unroll
        for (int age = 0; age < DS_N; age++) {  // :479-483, newest first
            const double2 x = xm[idx - age];
            const double tp = a.taps[age];
            fi += x.x * tp;
            fq += x.y * tp;
        }
        double *o = a.ds + 2 * (row * g.L + (gg % g.L));  // :507-509
        o[0] = fi * HOWARD;
        o[1] = fq * HOWARD;
    }
}

struct ScopeWalkArgs {
    const double2 *y;  // [S][y_stride] (fi, fq) of the call
    long long y_stride;
    const TailState *t0;  // [S] the clock state of before the call
    signed char *bits;    // [rows][L], zeroed; or null
    int *pts;             // [rows][L][4], zeroed; di goes into ints 2 (low word) and 3 (high word); or null
};

// :533-593 over the call's samples.  dmBitPos is g mod 8 and the new peak is measured behind every g = 7 mod 8, g counted
// since creation: the bit clock is input independent (checked at create, as for k_tail).  A lane walks bit periods: the eight
// samples of the next period are asked for before the eight of this one are stepped through, so the memory latency is paid
// once a period and not once a sample, and the bit position of a sample is a constant of the unrolled body.
__global__ __launch_bounds__(64) void k_bpsk_scope_walk(ScopeWalkArgs a, ScopeGeom g)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= g.nstreams) return;
    const TailState *sp = a.t0 + s;
    double e[8];
#pragma unroll
    for (int k = 0; k < 8; k++) e[k] = sp->dmEnergy[k];
    double lastI = sp->lastI, lastQ = sp->lastQ;
    int peakPos = sp->peakPos, newPeak = sp->newPeak;
    const double K1 = 1.0 - 1.0 / 200.0, S1 = 1.0 / 200.0;  // BIT_SMOOTH1 (:89)
    const double2 *y = a.y + (long long)s * a.y_stride;
    auto load = [&](long long j) { return (j >= 0 && j < g.nds) ? y[j] : make_double2(0.0, 0.0); };
    auto frame_end = [&](int f) {
        const long long je = scope_before(g, f + 1) - g.a0;
        return je < g.nds ? je : g.nds;
    };
    int f = 0;
    long long row = (long long)s * g.frames, jend = frame_end(0);
    int slot = (int)((g.a0 - g.origin + 1) % g.L);  // of the call's sample 0: demodIdx is advanced before the write (:529)
    long long jb = -(g.a0 & 7);                     // the call's index of the first sample of its first bit period
    double2 cur[8], nxt[8];
#pragma unroll
    for (int u = 0; u < 8; u++) cur[u] = load(jb + u);
    for (; jb < g.nds; jb += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) nxt[u] = load(jb + 8 + u);
#pragma unroll
        for (int u = 0; u < 8; u++) {  // u is dmBitPos
            const long long j = jb + u;
            if (j >= 0 && j < g.nds) {
                while (j >= jend && f + 1 < g.frames) {
                    f++;
                    row++;
                    jend = frame_end(f);
                }
                const double fi = cur[u].x, fq = cur[u].y;
                const double energy1 = fi * fi + fq * fq;  // :534
                e[u] = (e[u] * K1) + (energy1 * S1);       // :535
                if (u == peakPos) {                        // :537
                    const double di = -(lastI * fi + lastQ * fq);
                    const double dq = lastI * fq - lastQ * fi;
                    lastI = fi;
                    lastQ = fq;
                    // energy2 = Math.sqrt(di*di+dq*dq) > 100.0 (:543-544), decided on the square: sqrt is correctly rounded and
                    // monotone, sqrt(10000) is 100 exactly and the root of the next double above 10000 rounds above 100; a NaN
                    // fails both (the lanes of a wave sit on different bit positions, so a root here would be taken eight
                    // times a period)
                    if (di * di + dq * dq > 10000.0) {
                        const long long at = row * g.L + slot;
                        if (a.bits) a.bits[at] = di < 0.0 ? (signed char)1 : (signed char)-1;  // :550
                        if (a.pts) {                                                          // :549
                            a.pts[4 * at + 2] = __double2loint(di);
                            a.pts[4 * at + 3] = __double2hiint(di);
                        }
                    }
                }
                if (u == ((peakPos + 4) & 7)) peakPos = newPeak;  // dmHalfTable (:500, :577-578)
                if (u == 7) {                                     // :582-592
                    double eMax = (double)-1.0e10F;
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        if (e[k] > eMax) {
                            newPeak = k;
                            eMax = e[k];
                        }
                }
                slot = slot + 1 == g.L ? 0 : slot + 1;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) cur[u] = nxt[u];
    }
}

struct ScopePtsArgs {
    const double2 *y;
    long long y_stride;
    double *iq;   // [rows][L][2], or null
    double *mx;   // [rows][2], or null
    int *pts;     // [rows][L][4], or null
};

__global__ __launch_bounds__(SCOPE_THREADS) void k_bpsk_scope_pts(ScopePtsArgs a, ScopeGeom g)
{
    __shared__ double red[2][SCOPE_THREADS];
    const int tid = threadIdx.x;
    const long long row = blockIdx.x;
    const int s = (int)(row / g.frames);
    const int f = (int)(row - (long long)s * g.frames);
    const double2 *y = a.y + (long long)s * a.y_stride;
    // slot (g + 1) mod L holds (fi, fq) of sample g (:529-531), the largest g of the frame for each slot
    const long long glast = scope_before(g, f + 1) - g.origin - 1;
    const int slast = (int)((glast + 1) % g.L);
    auto sample = [&](int slot) {
        int back = slast - slot;
        if (back < 0) back += g.L;
        return y[glast - back + g.origin - g.a0];
    };
    double mi = 0.0, mq = 0.0;  // :232-238
    for (int slot = tid; slot < g.L; slot += SCOPE_THREADS) {
        const double2 v = sample(slot);
        if (a.iq) {
            a.iq[2 * (row * g.L + slot)] = v.x;
            a.iq[2 * (row * g.L + slot) + 1] = v.y;
        }
        if (mi < fabs(v.x)) mi = fabs(v.x);
        if (mq < fabs(v.y)) mq = fabs(v.y);
    }
    if (!a.mx && !a.pts) return;
    // (the strict compare takes the largest |x| that is not a NaN, in any order: a NaN never wins and never sits in mi)
    red[0][tid] = mi;
    red[1][tid] = mq;
    __syncthreads();
    for (int w = SCOPE_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            if (red[0][tid] < red[0][tid + w]) red[0][tid] = red[0][tid + w];
            if (red[1][tid] < red[1][tid + w]) red[1][tid] = red[1][tid + w];
        }
        __syncthreads();
    }
    mi = red[0][0];
    mq = red[1][0];
    if (a.mx && tid == 0) {
        a.mx[2 * row] = mi;
        a.mx[2 * row + 1] = mq;
    }
    if (!a.pts) return;
    const double xs = 100.0 / mi, ys = 100.0 / mq;  // :239
    const double rs = 50.0 / (mi * mq);             // :260
    for (int slot = tid; slot < g.L; slot += SCOPE_THREADS) {
        const double2 v = sample(slot);
        int *p = a.pts + 4 * (row * g.L + slot);
        const double re = __hiloint2double(p[3], p[2]);  // demodRe[slot], marked by the walk
        p[0] = java_d2i(v.x * xs);  // :247, :254
        p[1] = java_d2i(v.y * ys);  // :248
        p[2] = java_d2i(v.y * xs);  // :256 (xs, as written)
        p[3] = java_d2i(re * rs);   // :262
    }
}

#pragma GCC visibility pop
}  // namespace jsdr

// ------------------------------------------------------------------------------------------- the host side
// what a scope call and jsdr_bpsk_scope_layout both ask of the handle and the call's length, before anything else
static int scope_geom_check(const jsdr_bpsk *h, long long L, const char *who, ScopeGeom &g)
{
    JSDR_REQUIRE(h, "%s: null handle", who);
    JSDR_REQUIRE(h->nch == 0, "%s: a channel handle (jsdr_bpsk_create_channels and its kin) has no scope; the handle is unchanged", who);
    JSDR_REQUIRE(!h->pst, "%s: a tuned handle (jsdr_bpsk_create_tuned, jsdr_bpsk_create_tuned_channels) has no scope; the handle is "
                 "unchanged", who);
    JSDR_REQUIRE(h->variant == JSDR_VARIANT_EXACT, "%s: the fast variant (JSDR_VARIANT_FAST) has no scope: its (fi, fq) are not the "
                 "reference's; the handle is unchanged", who);
    JSDR_REQUIRE(!h->do_fft && h->seam == SEAM_NONE, "%s: do_fft is set or a mode switch is pending: in FFT-acquire the tuned ring is the "
                 "inverse transform's real part twice, which the scope does not build; the handle is unchanged", who);
    JSDR_REQUIRE(h->rate >= 9600, "%s: rate=%d below 9600 Hz: a frame does not refill the rings; the handle is unchanged", who, h->rate);
    JSDR_REQUIRE(L > 0 && L <= h->max_batch, "%s: nsamples=%lld outside (0, max_batch_samples=%lld]; the handle is unchanged", who, L,
                 h->max_batch);
    JSDR_REQUIRE(L % h->nsf == 0, "%s: nsamples=%lld is not whole frames of %d samples; the handle is unchanged", who, L, h->nsf);
    JSDR_REQUIRE(h->n_in % h->nsf == 0, "%s: n_in=%lld, the samples the handle has taken, is not whole frames of %d samples: the "
                 "reference never paints such a state; the handle is unchanged", who, h->n_in, h->nsf);
    const long long ring = (long long)h->nsf * 9600 / h->rate;  // samples*DOWN_SAMPLE_RATE/adsc.rate (:201)
    JSDR_REQUIRE(ring >= 1 && ring <= 0x7fffffffLL, "%s: ring length L=%lld (n * 9600 / rate) is below 1: the frame of %d samples is too "
                 "short for the rings; the handle is unchanged", who, ring, h->nsf);
    g.n_in = h->n_in;
    g.origin = h->scope_origin;
    g.n = h->nsf;
    g.D = h->decim;
    g.L = (int)ring;
    g.frames = (int)(L / h->nsf);
    g.nstreams = h->nstreams;
    g.a0 = h->n_in / h->decim;
    g.nds = scope_before(g, g.frames) - g.a0;
    JSDR_REQUIRE(h->decim == h->rate / 9600 && g.a0 == h->n_ds && h->dsCnt == (int)(h->n_in % h->decim) && g.origin <= g.a0,
                 "%s: internal: the handle's decimation counters (n_in=%lld, n_ds=%lld, dsCnt=%d) are not those of whole frames", who,
                 h->n_in, h->n_ds, h->dsCnt);
    // (every frame refills the rings: true of every rate >= 9600; the kernels place slots by it)
    for (int f = 0; f < g.frames; f++)
        JSDR_REQUIRE(scope_before(g, f + 1) - scope_before(g, f) >= g.L, "%s: internal: frame %d holds fewer than L=%d decimated samples",
                     who, f, g.L);
    return JSDR_OK;
}

int jsdr_bpsk_scope_layout(jsdr_bpsk *h, int64_t nsamples, int *ring_len, int64_t *origin, int64_t *g_first, int cap)
{
    ScopeGeom g;
    if (scope_geom_check(h, nsamples, "jsdr_bpsk_scope_layout", g) != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(!g_first || cap >= g.frames + 1, "jsdr_bpsk_scope_layout: cap=%d below frames + 1 = %d", cap, g.frames + 1);
    if (ring_len) *ring_len = g.L;
    if (origin) *origin = g.origin;
    if (g_first)
        for (int f = 0; f <= g.frames; f++) g_first[f] = scope_before(g, f) - g.origin;
    return JSDR_OK;
}

const char *jsdr_bpsk_scope_kernel(jsdr_bpsk *h) { return h ? h->scope_name.c_str() : ""; }

// ---- the spectra of a call (jsdr_bpsk_scope_spectra_*): k = 0 the green one over `tuned` (n points), k = 1 the cyan one over
// `ds` (L points)
struct ScopeSpecReq {
    int width = 0;
    int32_t *spec[2] = {nullptr, nullptr};
    double *peak[2] = {nullptr, nullptr};
    double *psd[2] = {nullptr, nullptr};
    bool want(int k) const { return spec[k] || peak[k] || psd[k]; }
};
constexpr size_t SCOPE_SPEC_ROWS_BYTES = (size_t)64 << 20;  // the handle's own rows of one pass

// i and l of every column, checked against psd[]: what jsdr_bpsk_scope_spec_layout states and a spectra call relies on
static int spec_layout_check(int len, int width, int32_t *first, int32_t *count, const char *who)
{
    JSDR_REQUIRE(len >= 2, "%s: len=%d below 2", who, len);
    JSDR_REQUIRE(width >= 1 && width <= SPEC_WIDTH_MAX, "%s: plot_width=%d outside 1 .. %d; the handle is unchanged", who, width,
                 SPEC_WIDTH_MAX);
    for (int m = 0; m < width; m++) {
        int i, l;
        scope_spec_column(len, width, m, i, l);
        JSDR_REQUIRE(i >= 0 && l >= 0 && (long long)i + (l > 1 ? l : 1) <= len, "%s: column %d of %d reads psd[%d .. %d) of %d bins", who, m,
                     width, i, i + l, len);
        if (first) first[m] = i;
        if (count) count[m] = l;
    }
    return JSDR_OK;
}

int jsdr_bpsk_scope_spec_layout(int len, int plot_width, int32_t *first, int32_t *count, int cap)
{
    JSDR_REQUIRE(cap >= plot_width, "jsdr_bpsk_scope_spec_layout: cap=%d below plot_width=%d", cap, plot_width);
    return spec_layout_check(len, plot_width, first, count, "jsdr_bpsk_scope_spec_layout");
}

int jsdr_bpsk_scope_chunk(jsdr_bpsk *h, int frames_per_pass)
{
    JSDR_REQUIRE(h, "jsdr_bpsk_scope_chunk: null handle");
    JSDR_REQUIRE(frames_per_pass >= 0, "jsdr_bpsk_scope_chunk: frames_per_pass=%d is negative; the handle is unchanged", frames_per_pass);
    h->scope_spec_chunk = frames_per_pass;
    return JSDR_OK;
}

// what a spectra call refuses on top of the scope call, before any device work
static int spec_check(const ScopeSpecReq &sq, const ScopeGeom &g, const double *ds_dev, const char *who)
{
    static const char *const row[2] = {"tuned", "ds"};
    for (int k = 0; k < 2; k++) {
        if (!sq.want(k)) continue;
        const int len = k ? g.L : g.n;
        JSDR_REQUIRE(scope_spec_form(len), "%s: no spectrum kernel serves the %s rows of %d points (served: powers of two %d .. %d, every "
                     "other length up to %d); the handle is unchanged", who, row[k], len, SPEC_POW2_MIN, SPEC_POW2_MAX, FM_NMAX);
        if (sq.spec[k] && spec_layout_check(len, sq.width, nullptr, nullptr, who) != JSDR_OK) return JSDR_ERR;
        JSDR_REQUIRE((reinterpret_cast<uintptr_t>(sq.spec[k]) & 3) == 0, "%s: %cspec_dev is not aligned to 4 bytes; the handle is unchanged",
                     who, row[k][0]);
        JSDR_REQUIRE((reinterpret_cast<uintptr_t>(sq.peak[k]) & 15) == 0 && (reinterpret_cast<uintptr_t>(sq.psd[k]) & 15) == 0,
                     "%s: %cpeak_dev or %cpsd_dev is not aligned to 16 bytes; the handle is unchanged", who, row[k][0], row[k][0]);
    }
    JSDR_REQUIRE(!sq.want(1) || (reinterpret_cast<uintptr_t>(ds_dev) & 15) == 0, "%s: ds_dev is not aligned to 16 bytes, which the cyan "
                 "spectrum's 16-byte loads need; the handle is unchanged", who);
    return JSDR_OK;
}

// the plan of spectrum k and its tables on the device, built once a handle (again where the row length has changed)
static int spec_plan_ensure(jsdr_bpsk *h, int k, int len, const char *who)
{
    if (h->scope_spec_plan[k].n == len && h->scope_spec_w[k].p) return JSDR_OK;
    std::vector<double2> w;
    FftPlan pl;
    JSDR_REQUIRE(fft_plan_build_row(pl, w, len) && !w.empty(), "%s: internal: no plan for a row of %d points", who, len);
    DevBuf<double2> d;
    if (d.alloc(w.size()) != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipMemcpy(d.p, w.data(), sizeof(double2) * w.size(), hipMemcpyHostToDevice));
    h->scope_spec_w[k] = std::move(d);
    h->scope_spec_plan[k] = pl;
    return JSDR_OK;
}

static ScopeSpecArgs spec_args(const jsdr_bpsk *h, const ScopeSpecReq &sq, int k, const ScopeGeom &g, const double2 *rows, int c, int f0)
{
    ScopeSpecArgs sa = {};
    sa.rows = rows;
    sa.len = k ? g.L : g.n;
    sa.c = c;
    sa.frames = g.frames;
    sa.f0 = f0;
    sa.width = sq.spec[k] ? sq.width : 1;
    sa.pi = (double)(sa.len / 2) / (double)sa.width;  // :285, :317
    sa.l = (int)sa.pi;
    sa.spec = sq.spec[k];
    sa.peak = sq.peak[k];
    sa.psd = sq.psd[k];
    sa.logn = h->scope_spec_plan[k].logn;
    sa.tw = h->scope_spec_w[k].p;
    sa.m = h->scope_spec_plan[k].args;
    sa.m.f.tw = sa.tw;
    sa.m.f.n = sa.len;
    return sa;
}

static int scope_run(jsdr_bpsk *h, const int16_t *raw_dev, const float *rawf_dev, int64_t stride, int64_t L, int ic, int qc,
                     double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev, void *stream,
                     const char *who, const ScopeSpecReq *sq = nullptr)
{
    ScopeGeom g;
    JSDR_REQUIRE(h, "%s: null handle", who);
    JSDR_REQUIRE(raw_dev || rawf_dev, "%s: null input; the handle is unchanged", who);
    if (scope_geom_check(h, L, who, g) != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE((stride & 1) == 0 && (h->nstreams == 1 || stride >= 2 * L), "%s: stream stride %lld is odd or too small for %lld "
                 "samples; the handle is unchanged", who, (long long)stride, (long long)L);
    JSDR_REQUIRE((reinterpret_cast<uintptr_t>(tuned_dev) & 15) == 0, "%s: tuned_dev is not aligned to 16 bytes; the handle is unchanged", who);
    JSDR_REQUIRE((reinterpret_cast<uintptr_t>(ds_dev) & 7) == 0, "%s: ds_dev is not aligned to 8 bytes; the handle is unchanged", who);
    JSDR_REQUIRE((reinterpret_cast<uintptr_t>(iq_dev) & 7) == 0, "%s: iq_dev is not aligned to 8 bytes; the handle is unchanged", who);
    JSDR_REQUIRE((reinterpret_cast<uintptr_t>(max_dev) & 7) == 0, "%s: max_dev is not aligned to 8 bytes; the handle is unchanged", who);
    JSDR_REQUIRE((reinterpret_cast<uintptr_t>(pts_dev) & 3) == 0, "%s: pts_dev is not aligned to 4 bytes; the handle is unchanged", who);
    const long long rows = (long long)g.nstreams * g.frames;
    const long long tiles = (g.n + SCOPE_TILE - 1) / SCOPE_TILE;
    JSDR_REQUIRE(rows * tiles < (1LL << 31), "%s: nsamples=%lld: %lld rows of %lld tiles exceed one launch; the handle is unchanged", who,
                 (long long)L, rows, tiles);
    if (sq && spec_check(*sq, g, ds_dev, who) != JSDR_OK) return JSDR_ERR;
    hipStream_t st = as_stream(stream);
    // a spectrum whose rows the caller did not ask for reads rows of the handle's own, a pass of own_c frames at a time
    const bool own_t = sq && sq->want(0) && !tuned_dev, own_d = sq && sq->want(1) && !ds_dev;
    int own_c = 0;
    if (own_t || own_d) {
        const size_t per = (size_t)g.nstreams * sizeof(double2) * ((own_t ? (size_t)g.n : 0) + (own_d ? (size_t)g.L : 0));
        size_t c = SCOPE_SPEC_ROWS_BYTES / per;
        if (h->scope_spec_chunk > 0 && c > (size_t)h->scope_spec_chunk) c = (size_t)h->scope_spec_chunk;
        own_c = (int)(c < 1 ? 1 : c > (size_t)g.frames ? (size_t)g.frames : c);
    }
    const bool want_front = tuned_dev || ds_dev, want_walk = pts_dev || bits_dev, want_pts = iq_dev || max_dev || pts_dev;
    // the scratch, before anything of the handle moves on: what can fail for want of memory leaves the handle as it was
    if (want_walk && !h->scope_tail0.p) {
        if (h->scope_tail0.alloc((size_t)h->nstreams) != JSDR_OK || h->scope_ev_copy.create(hipEventDisableTiming) != JSDR_OK ||
            h->scope_ev_walk.create(hipEventDisableTiming) != JSDR_OK)
            return JSDR_ERR;
    }
    if (sq) {
        for (int k = 0; k < 2; k++)
            if (sq->want(k) && spec_plan_ensure(h, k, k ? g.L : g.n, who) != JSDR_OK) return JSDR_ERR;
        const size_t own_rows = (size_t)g.nstreams * (size_t)own_c;
        if (own_t && h->scope_spec_tuned.n < own_rows * (size_t)g.n && h->scope_spec_tuned.alloc(own_rows * (size_t)g.n) != JSDR_OK)
            return JSDR_ERR;
        if (own_d && h->scope_spec_ds.n < own_rows * (size_t)g.L * 2 && h->scope_spec_ds.alloc(own_rows * (size_t)g.L * 2) != JSDR_OK)
            return JSDR_ERR;
        if (own_c && own_c < g.frames && !h->scope_spec_hist.p && h->scope_spec_hist.alloc((size_t)g.nstreams * 32) != JSDR_OK)
            return JSDR_ERR;
    }
    if (want_front || own_c) {
        if (!h->scope_k9.p && h->scope_k9.alloc((size_t)h->max_batch + SCHED_HIST) != JSDR_OK) return JSDR_ERR;
        if (sincos9_ensure(h) != JSDR_OK) return JSDR_ERR;
    }
    unsigned char mh0[SCHED_HIST];  // which of the 26 samples before the call were mixed (the call moves the flags on)
    memcpy(mh0, h->h_mhist, SCHED_HIST);
    const bool first = h->n_in == 0;
    if (want_walk) {
        // the clock state the call's own tail starts from, copied where that tail runs: behind the previous call's tail, in
        // front of this one's -- and behind the previous scope call's walk, which reads the copy
        hipStream_t ts = h->overlap ? (hipStream_t)h->tail_stream : st;
        if (h->overlap && h->scope_walk_pending) JSDR_HIP_TRY(hipStreamWaitEvent(ts, h->scope_ev_walk, 0));
        h->scope_walk_pending = false;
        JSDR_HIP_TRY(hipMemcpyAsync(h->scope_tail0.p, h->tail.p, sizeof(TailState) * (size_t)h->nstreams, hipMemcpyDeviceToDevice, ts));
        if (h->overlap) JSDR_HIP_TRY(hipEventRecord(h->scope_ev_copy, ts));
    }
    h->scope_name.clear();
    const int rc = rawf_dev ? jsdr_bpsk_batch_f32(h, rawf_dev, stride, L, stream) : jsdr_bpsk_batch_i16(h, raw_dev, stride, L, ic, qc, stream);
    if (rc != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(h->last_nds == g.nds, "%s: internal: the call demodulated %lld samples, the frames hold %lld", who, h->last_nds, g.nds);
    auto named = [&](const char *k) {
        if (!h->scope_name.empty()) h->scope_name += "+";
        h->scope_name += k;
    };
    ScopeFrontArgs fa;
    if (want_front || own_c) {
        // the call's tuner schedule as a 9-bit table: the schedule's index where the sample was mixed, 256 where it passed (:395)
        expand_k9(h->scope_h_k9, h->cur.ktu.data(), 0, (long long)L, first ? nullptr : mh0, h->cur.f0, h->cur.n0);
        JSDR_HIP_TRY(hipMemcpyAsync(h->scope_k9.p, h->scope_h_k9.data(), sizeof(unsigned short) * ((size_t)L + SCHED_HIST),
                                    hipMemcpyHostToDevice, st));
        fa.raw = reinterpret_cast<const int *>(raw_dev);
        fa.rawf = reinterpret_cast<const float2 *>(rawf_dev);
        fa.stride_pairs = stride / 2;
        fa.ic = ic;
        fa.qc = qc;
        fa.hist = h->hist_in[h->hist_cur ^ 1].p;  // (the call has written the other half for the next one)
        fa.k9 = h->scope_k9.p;
        fa.sc9 = h->sincos9.p;
        double taps[32];
        if (jsdr_bpsk_table(0, taps, 32) != JSDR_OK) return JSDR_ERR;
        memcpy(fa.taps, taps, sizeof(fa.taps));
        fa.tuned = reinterpret_cast<double2 *>(tuned_dev);
        fa.ds = ds_dev;
    }
    if (want_front) {
        const dim3 grid((unsigned)(rows * tiles));
        if (rawf_dev)
            hipLaunchKernelGGL(k_bpsk_scope_front<true>, grid, dim3(SCOPE_THREADS), 0, st, fa, g);
        else
            hipLaunchKernelGGL(k_bpsk_scope_front<false>, grid, dim3(SCOPE_THREADS), 0, st, fa, g);
        JSDR_LAUNCH_CHECK();
        named("k_bpsk_scope_front");
    }
    const double2 *y = h->y[h->last_y].p + Y_PAD;
    if (want_walk) {
        if (h->overlap) JSDR_HIP_TRY(hipStreamWaitEvent(st, h->scope_ev_copy, 0));
        if (bits_dev) JSDR_HIP_TRY(hipMemsetAsync(bits_dev, 0, (size_t)rows * (size_t)g.L, st));                 // :367-370
        if (pts_dev) JSDR_HIP_TRY(hipMemsetAsync(pts_dev, 0, (size_t)rows * (size_t)g.L * 4 * sizeof(int), st));
        ScopeWalkArgs wa;
        wa.y = y;
        wa.y_stride = h->y_stride;
        wa.t0 = h->scope_tail0.p;
        wa.bits = reinterpret_cast<signed char *>(bits_dev);
        wa.pts = pts_dev;
        hipLaunchKernelGGL(k_bpsk_scope_walk, dim3((unsigned)((g.nstreams + 63) / 64)), dim3(64), 0, st, wa, g);
        JSDR_LAUNCH_CHECK();
        if (h->overlap) {
            JSDR_HIP_TRY(hipEventRecord(h->scope_ev_walk, st));
            h->scope_walk_pending = true;
        }
        named("k_bpsk_scope_walk");
    }
    if (want_pts) {
        ScopePtsArgs pa;
        pa.y = y;
        pa.y_stride = h->y_stride;
        pa.iq = iq_dev;
        pa.mx = max_dev;
        pa.pts = pts_dev;
        hipLaunchKernelGGL(k_bpsk_scope_pts, dim3((unsigned)rows), dim3(SCOPE_THREADS), 0, st, pa, g);
        JSDR_LAUNCH_CHECK();
        named("k_bpsk_scope_pts");
    }
    if (!sq) return JSDR_OK;
    // the spectra over the caller's rows: one launch each over the whole call
    const double2 *caller[2] = {reinterpret_cast<const double2 *>(tuned_dev), reinterpret_cast<const double2 *>(ds_dev)};
    const bool own[2] = {own_t, own_d};
    const char *form[2] = {scope_spec_form(g.n), scope_spec_form(g.L)};
    for (int k = 0; k < 2; k++) {
        if (!sq->want(k) || own[k]) continue;
        if (launch_scope_spec(spec_args(h, *sq, k, g, caller[k], g.frames, 0), rows, st) != JSDR_OK) return JSDR_ERR;
    }
    // ... and over the handle's: a pass of own_c frames of every stream through k_bpsk_scope_front, then its spectra
    for (int f0 = 0; own_c && f0 < g.frames; f0 += own_c) {
        const int c = g.frames - f0 < own_c ? g.frames - f0 : own_c;
        const long long skip = (long long)f0 * g.n;  // samples of the call in front of the pass
        ScopeFrontArgs pa = fa;
        ScopeGeom pg = g;
        pg.n_in = g.n_in + skip;
        pg.frames = c;
        if (pa.raw) pa.raw += skip;
        if (pa.rawf) pa.rawf += skip;
        pa.k9 += skip;
        if (f0 > 0) {
            HistArgs ha = hist_args(h, fa.raw, fa.rawf, fa.stride_pairs, skip, ic, qc, g.nstreams);
            ha.hist_old = fa.hist;
            ha.hist_new = h->scope_spec_hist.p;
            if (launch_hist_in(ha, st) != JSDR_OK) return JSDR_ERR;
            pa.hist = h->scope_spec_hist.p;
        }
        pa.tuned = own_t ? h->scope_spec_tuned.p : nullptr;
        pa.ds = own_d ? h->scope_spec_ds.p : nullptr;
        const long long prows = (long long)g.nstreams * c;
        const dim3 grid((unsigned)(prows * tiles));
        if (rawf_dev)
            hipLaunchKernelGGL(k_bpsk_scope_front<true>, grid, dim3(SCOPE_THREADS), 0, st, pa, pg);
        else
            hipLaunchKernelGGL(k_bpsk_scope_front<false>, grid, dim3(SCOPE_THREADS), 0, st, pa, pg);
        JSDR_LAUNCH_CHECK();
        const double2 *mine[2] = {h->scope_spec_tuned.p, reinterpret_cast<const double2 *>(h->scope_spec_ds.p)};
        for (int k = 0; k < 2; k++)
            if (own[k] && launch_scope_spec(spec_args(h, *sq, k, g, mine[k], c, f0), prows, st) != JSDR_OK) return JSDR_ERR;
    }
    if (own_c && !want_front) named("k_bpsk_scope_front");
    for (int k = 0; k < 2; k++)
        if (sq->want(k)) named(form[k]);
    return JSDR_OK;
}

int jsdr_bpsk_scope_i16(jsdr_bpsk *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc,
                        double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev,
                        void *stream)
{
    JSDR_REQUIRE(h && raw_dev, "jsdr_bpsk_scope_i16: null %s; the handle is unchanged", h ? "input raw_dev" : "handle");
    return scope_run(h, raw_dev, nullptr, stream_stride_i16, nsamples, ic, qc, tuned_dev, ds_dev, iq_dev, max_dev, pts_dev, bits_dev, stream,
                     "jsdr_bpsk_scope_i16");
}

int jsdr_bpsk_scope_f32(jsdr_bpsk *h, const float *iq_in_dev, int64_t stream_stride_f32, int64_t nsamples, double *tuned_dev,
                        double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev, void *stream)
{
    JSDR_REQUIRE(h && iq_in_dev, "jsdr_bpsk_scope_f32: null %s; the handle is unchanged", h ? "input iq_in_dev" : "handle");
    return scope_run(h, nullptr, iq_in_dev, stream_stride_f32, nsamples, 0, 0, tuned_dev, ds_dev, iq_dev, max_dev, pts_dev, bits_dev, stream,
                     "jsdr_bpsk_scope_f32");
}

static ScopeSpecReq spec_req(int plot_width, int32_t *tspec_dev, double *tpeak_dev, double *tpsd_dev, int32_t *dspec_dev, double *dpeak_dev,
                             double *dpsd_dev)
{
    ScopeSpecReq sq;
    sq.width = plot_width;
    sq.spec[0] = tspec_dev, sq.peak[0] = tpeak_dev, sq.psd[0] = tpsd_dev;
    sq.spec[1] = dspec_dev, sq.peak[1] = dpeak_dev, sq.psd[1] = dpsd_dev;
    return sq;
}

int jsdr_bpsk_scope_spectra_i16(jsdr_bpsk *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc,
                                double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev,
                                int plot_width, int32_t *tspec_dev, double *tpeak_dev, double *tpsd_dev, int32_t *dspec_dev,
                                double *dpeak_dev, double *dpsd_dev, void *stream)
{
    JSDR_REQUIRE(h && raw_dev, "jsdr_bpsk_scope_spectra_i16: null %s; the handle is unchanged", h ? "input raw_dev" : "handle");
    const ScopeSpecReq sq = spec_req(plot_width, tspec_dev, tpeak_dev, tpsd_dev, dspec_dev, dpeak_dev, dpsd_dev);
    return scope_run(h, raw_dev, nullptr, stream_stride_i16, nsamples, ic, qc, tuned_dev, ds_dev, iq_dev, max_dev, pts_dev, bits_dev, stream,
                     "jsdr_bpsk_scope_spectra_i16", (sq.want(0) || sq.want(1)) ? &sq : nullptr);
}

int jsdr_bpsk_scope_spectra_f32(jsdr_bpsk *h, const float *iq_in_dev, int64_t stream_stride_f32, int64_t nsamples, double *tuned_dev,
                                double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev, int plot_width,
                                int32_t *tspec_dev, double *tpeak_dev, double *tpsd_dev, int32_t *dspec_dev, double *dpeak_dev,
                                double *dpsd_dev, void *stream)
{
    JSDR_REQUIRE(h && iq_in_dev, "jsdr_bpsk_scope_spectra_f32: null %s; the handle is unchanged", h ? "input iq_in_dev" : "handle");
    const ScopeSpecReq sq = spec_req(plot_width, tspec_dev, tpeak_dev, tpsd_dev, dspec_dev, dpeak_dev, dpsd_dev);
    return scope_run(h, nullptr, iq_in_dev, stream_stride_f32, nsamples, 0, 0, tuned_dev, ds_dev, iq_dev, max_dev, pts_dev, bits_dev, stream,
                     "jsdr_bpsk_scope_spectra_f32", (sq.want(0) || sq.want(1)) ? &sq : nullptr);
}
