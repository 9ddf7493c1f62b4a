// demod.hip -- the demod.java AM/FM chain, demod.java:341-483, batched over S streams:
//   21-tap complex float FIR band-pass (filter(), :378-396), down-conversion NCO (:423-434), AM envelope with its
//   running mean (:448-451) / FM quadrature-delay detector (:453-461), per-frame maximum, AGC and the float ->
//   int16 stereo output (:465-481).
// Compiled with -ffp-contract=off: every float multiply and add rounds separately, as Java's do.
//
// What is sequential in the reference and how it is laid out here:
//   * the FIR delay line and the FM detector's previous sample carry over frames and calls: 21 samples of halo
//     are re-read (from the stream buffer, or from a per-stream history of the previous call), the previous
//     mixed sample is recomputed from that halo -- nothing is serial;
//   * the NCO phase `car` is a float accumulator: input independent, so the host steps it in float exactly as
//     the reference does and a kernel turns the call's phases into (cos, sin) pairs once for all streams;
//   * the AM mean avg = (k*avg + a_k)/(k+1) is a data-dependent float recurrence over the frame: one LANE per
//     frame walks it (64 frames per wave, amplitudes transposed through LDS so that global reads stay coalesced);
//   * max / AGC need the whole frame: the output is a second pass over the demodulated floats.
// Kernels: k_demod_front (raw -> demodulated float per sample + per-frame max), k_demod_mean (AM only),
// k_demod_out (-> int16 L,R), k_demod_state (history for the next call), k_demod_nco.
// The demod scope (jsdr_demod_scope_*: the batch call, then demod.paintComponent's trace and spectrum per frame) has its host
// side here, behind demod_run, and its kernels in demod_scope.hip.
#include "common.h"
#include "demod.h"
#include "demod_dev.h"
#include <math.h>
#include <stdlib.h>
#include <thread>
#include <vector>

namespace jsdr {


// (DemodArgs, demod_in, demod_mixed_at, demod_mixed and demod_tile: demod_dev.h, shared with demod_scope.hip)

__device__ __forceinline__ unsigned demod_block_max(unsigned mbits, unsigned *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o = __shfl_xor(mbits, off, 64);
        mbits = o > mbits ? o : mbits;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mbits;
    __syncthreads();
    unsigned mx = red[0];
    for (int w = 1; w < 4; w++) mx = red[w] > mx ? red[w] : mx;
    return mx;
}

// AM (whose running mean needs the whole frame first) and frames longer than 5 tiles: one tile per workgroup, the
// detected samples go to HBM as floats and k_demod_mean / k_demod_out finish the frame
template <bool F32IN>
__global__ __launch_bounds__(256) void k_demod_front(DemodArgs a)
{
    constexpr int PER = DPER;
    __shared__ float2 xs[DXS];
    __shared__ float2 last[256];
    __shared__ unsigned red[4];
    const int tid = threadIdx.x;
    const int s = blockIdx.y;
    const int tiles_per_frame = (a.n + DTILE - 1) / DTILE;
    const int f = blockIdx.x / tiles_per_frame;
    const int j = blockIdx.x - f * tiles_per_frame;
    const long long g0 = (long long)f * a.n + (long long)j * DTILE;
    const int len = (a.n - j * DTILE) < DTILE ? (a.n - j * DTILE) : DTILE;
    const int t0 = tid * PER;
    float dv[PER];
    unsigned mbits = 0;
    demod_tile<F32IN, false>(a, s, f, j, xs, last, dv, mbits);
    float *d = a.d + (long long)s * a.L + g0 + t0;
    if (t0 + PER <= len && (((long long)s * a.L + g0) & 3) == 0) {
        reinterpret_cast<float4 *>(d)[0] = make_float4(dv[0], dv[1], dv[2], dv[3]);
        reinterpret_cast<float4 *>(d)[1] = make_float4(dv[4], dv[5], dv[6], dv[7]);
    } else {
#pragma unroll
        for (int u = 0; u < PER; u++)
            if (t0 + u < len) d[u] = dv[u];
    }
    const unsigned mx = demod_block_max(mbits, red);
    if (tid == 0) atomicMax(&a.fmax_bits[(long long)s * a.nfr + f], mx);
}

// Every mode but AM, frames of at most NT tiles: one workgroup per frame keeps the detected samples in registers,
// takes the frame maximum itself and writes the int16 audio (:465-481) -- no float round trip through HBM and no
// second pass (4 B in, 4 B out per sample).
template <bool F32IN, int NT>
__global__ __launch_bounds__(256) void k_demod_fused(DemodArgs a, int *__restrict__ out, long long out_stride_pairs,
                                                     float *__restrict__ stats)
{
    constexpr int PER = DPER;
    __shared__ float2 xs[DXS];
    __shared__ float2 last[256];
    __shared__ unsigned red[4];
    const int tid = threadIdx.x;
    const int s = blockIdx.y, f = blockIdx.x;
    const int t0 = tid * PER;
    float dv[NT][PER];
    unsigned mbits = 0;
#pragma unroll
    for (int j = 0; j < NT; j++) {
        if (j) {
            __syncthreads();  // the previous tile's LDS image is still being read
            demod_tile<F32IN, true>(a, s, f, j, xs, last, dv[j], mbits);
        } else {
            demod_tile<F32IN, false>(a, s, f, j, xs, last, dv[j], mbits);
        }
    }
    const float mx = __uint_as_float(demod_block_max(mbits, red));
    const float scale = a.c.doagc ? 1.0f / mx : 1.0f;
    const long long F = (long long)s * a.nfr + f;
    if (stats && tid == 0) {  // the reference's `max` / `avg` fields after the frame
        stats[2 * F] = mx;
        stats[2 * F + 1] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int len = (a.n - j * DTILE) < DTILE ? (a.n - j * DTILE) : DTILE;
        const long long g = (long long)f * a.n + (long long)j * DTILE + t0;
        int *dst = out + (long long)s * out_stride_pairs + g;
        int o[PER];
#pragma unroll
        for (int u = 0; u < PER; u++) {
            o[u] = demod_lr(dv[j][u] * scale);
        }
        if (t0 + PER <= len && ((((long long)s * out_stride_pairs + g) & 3) == 0)) {
            reinterpret_cast<int4 *>(dst)[0] = make_int4(o[0], o[1], o[2], o[3]);
            reinterpret_cast<int4 *>(dst)[1] = make_int4(o[4], o[5], o[6], o[7]);
        } else {
#pragma unroll
            for (int u = 0; u < PER; u++)
                if (t0 + u < len) dst[u] = o[u];
        }
    }
}

// history for the next call: the last 21 filter inputs (only while the filter runs: the reference's ring is not
// written otherwise) and the FM detector's last sample (only in the FM modes, :453-461)
template <bool F32IN>
__global__ __launch_bounds__(64) void k_demod_state(DemodArgs a, float2 *hist_new, float2 *lilq_new, int nstreams)
{
    __shared__ float2 xs[2 * DHALO];
    const int s = blockIdx.x;
    const int tid = threadIdx.x;
    if (s >= nstreams) return;
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const float2 *rawf = a.rawf + (long long)s * a.stride_pairs;
    const float2 *hist = a.hist + (long long)s * DHALO;
    // xs[i] = x(L - 42 + i): enough for the filter at the last sample even when L < 21
    if (tid < 2 * DHALO) {
        const long long g = a.L - 2 * DHALO + tid;
        xs[tid] = (g >= -DHALO) ? demod_in<F32IN>(a, raw, rawf, hist, g) : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    if (tid < DHALO) hist_new[(long long)s * DHALO + tid] = a.c.dofir ? xs[DHALO + tid] : hist[tid];
    if (tid == 0) {
        const bool fm = a.c.mode == MODE_NFM || a.c.mode == MODE_WFM;
        lilq_new[s] = (fm && a.L > 0) ? demod_mixed_at(a.c, xs, [](int i) { return i; }, 2 * DHALO - 1, a.nco, a.L - 1) : a.lilq[s];
    }
}

// (float)Math.cos(car), (float)Math.sin(car) (:425-426) for the call's phases, once for all streams
__global__ __launch_bounds__(256) void k_demod_nco(const float *__restrict__ car, long long n, float2 *__restrict__ nco)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const double c = (double)car[g];
    nco[g] = make_float2((float)cos(c), (float)sin(c));
}

// AM running mean (:450): avg = ((s/2)*avg + sam[s]) / (s/2 + 1), one lane per frame.  64 frames per wave; their
// amplitudes are read row by row (256 contiguous bytes per instruction) and transposed through LDS.
__global__ __launch_bounds__(64) void k_demod_mean(const float *__restrict__ d, long long L, int n, int nfr,
                                                   long long nframes_total, float *__restrict__ favg)
{
    __shared__ float tile[64][65];
    const int lane = threadIdx.x;
    const long long F0 = (long long)blockIdx.x * 64;
    const long long F = F0 + lane;
    const bool valid = F < nframes_total;
    // base of this lane's frame; rows are addressed through readlane below
    const long long base = valid ? (F / nfr) * L + (F % nfr) * (long long)n : 0;
    const int nrows = (int)((nframes_total - F0) < 64 ? (nframes_total - F0) : 64);
    float avg = 0.0f;
    for (int c0 = 0; c0 < n; c0 += 64) {
        // the whole 64 x 64 tile in flight at once: sixteen 16-byte loads per lane (four rows of 64 samples per
        // wave instruction), 16 KB per wave -- the kernel is a 4-byte-per-sample stream read whose only problem
        // is memory-level parallelism (64-thread blocks, 9 per CU)
        if ((n & 3) == 0 && (L & 3) == 0 && c0 + 64 <= n) {
            float4 v[16];
            const int sub = lane >> 4, col = 4 * (lane & 15);
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int r = (4 * u + sub) < nrows ? (4 * u + sub) : (nrows - 1);
                const long long rb = __shfl(base, r, 64);
                v[u] = *reinterpret_cast<const float4 *>(d + rb + c0 + col);
            }
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int r = 4 * u + sub;
                if (r < nrows) {
                    tile[r][col] = v[u].x;
                    tile[r][col + 1] = v[u].y;
                    tile[r][col + 2] = v[u].z;
                    tile[r][col + 3] = v[u].w;
                }
            }
        } else {
            for (int r0 = 0; r0 < nrows; r0 += 16) {
                float v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const int r = (r0 + u) < nrows ? (r0 + u) : (nrows - 1);
                    const long long rb = __shfl(base, r, 64);
                    v[u] = (c0 + lane < n) ? d[rb + c0 + lane] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < 16; u++)
                    if (r0 + u < nrows) tile[r0 + u][lane] = v[u];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int cn = (n - c0) < 64 ? (n - c0) : 64;
        if (valid) {
            for (int c = 0; c < cn; c++) {
                const int k = c0 + c;
                avg = ((float)k * avg + tile[lane][c]) / (float)(k + 1);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    if (valid) favg[F] = avg;
}

// :465-481: max -= avg (AM); sam = (AM ? sam - avg : sam) * (doagc ? 1.0f/max : 1); (short)(sam * 32767f) to L and R.
// grid (chunks of 1024 samples within a frame, frame, stream): the frame's statistics are uniform per workgroup
__global__ __launch_bounds__(256) void k_demod_out(const float *__restrict__ d, long long L, int n, int nfr, int mode,
                                                   int doagc, const unsigned *__restrict__ fmax_bits,
                                                   const float *__restrict__ favg, int *__restrict__ out,
                                                   long long out_stride_pairs, float *__restrict__ stats)
{
    const int f = blockIdx.y, s = blockIdx.z;
    const long long F = (long long)s * nfr + f;
    float mx = __uint_as_float(fmax_bits[F]);
    const float avg = (mode == MODE_AM) ? favg[F] : 0.0f;
    if (mode == MODE_AM) mx -= avg;
    const float scale = doagc ? 1.0f / mx : 1.0f;
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) {  // the reference's `max` / `avg` fields after the frame
        stats[2 * F] = mx;
        stats[2 * F + 1] = avg;
    }
    const int t = (blockIdx.x * 256 + threadIdx.x) * 4;  // within the frame
    if (t >= n) return;
    const long long g = (long long)f * n + t;
    const float *src = d + (long long)s * L + g;
    int *dst = out + (long long)s * out_stride_pairs + g;
    float v[4];
    const bool vec = (t + 4 <= n) && ((((long long)s * L + g) & 3) == 0) && ((((long long)s * out_stride_pairs + g) & 3) == 0);
    if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(src);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = (t + u < n) ? src[u] : 0.0f;
    }
    int o[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        float x = v[u];
        if (mode == MODE_AM) x = x - avg;
        o[u] = demod_lr(x * scale);
    }
    if (vec) {
        *reinterpret_cast<int4 *>(dst) = make_int4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (t + u < n) dst[u] = o[u];
    }
}

}  // namespace jsdr

using namespace jsdr;

// the scope's jsdr_fft, owned like a stream or an event (counted by jsdr_live_resources among them)
static hipError_t demod_scope_fft_release(jsdr_fft *f)
{
    (void)jsdr_fft_destroy(f);
    return hipSuccess;
}
using DemodScopeFft = Owned<jsdr_fft *, demod_scope_fft_release>;

struct jsdr_demod {
    int rate = 0, n = 0, nstreams = 0;
    long long max_batch = 0;
    int mode = MODE_OFF, dofir = 0, dodwn = 0, doagc = 0;
    int flo = (-2147483647 - 1), fhi = 2147483647;
    float wfir[21] = {0};
    float phi = 0.0f, car = 0.0f;
    DevBuf<float2> hist[2], lilq[2];
    PinnedStage pin;        // receive(): [frame in | audio out]
    bool pin_tried = false;
    int cur = 0;
    // carrier tables, double-buffered: call k fills set k&1 on the copy stream while call k-1's kernels still read
    // the other one (no bubble between calls for the host's phase recurrence and its upload)
    DevBuf<float2> nco[2];
    DevBuf<float> car_dev[2];
    Pinned<float> car_pinned[2];
    Stream copy_stream;
    Event ev_table[2], ev_used[2];
    bool used[2] = {false, false};
    unsigned calls = 0;
    DevBuf<float> d, favg, stats;
    DevBuf<unsigned> fmax;
    DevBuf<float> stage_in;  // one frame, receive_f32
    DevBuf<int> stage_out;
    int last_nfr = 0;
    // optional per-kernel HIP-event timing (bench.py's roofline leg), same contract as jsdr_bpsk_profile_*
    bool prof_on = false;
    struct Rec {
        int k;
        Event a, b;
    };
    std::vector<Rec> recs;
    std::vector<Event> pool;
    // channel handles (jsdr_demod_create_channels): nstreams = nin * nch, channel c of input i is stream i * nch + c; every
    // channel has its own controls and carrier phase (the handle-wide fields above are unused)
    bool chan = false;
    int nin = 0, nch = 1;
    struct Chan {
        int mode = MODE_OFF, dofir = 0, dodwn = 0, doagc = 0;
        int flo = (-2147483647 - 1), fhi = 2147483647;
        float w[21] = {0};
        float phi = 0.0f, car = 0.0f;
    };
    std::vector<Chan> ch;
    long long nco_pitch = 0;   // entries between two carrier tables of a set
    DevBuf<float> dch;         // [dslots * nin][L] float rows (AM channels; every channel of a frame above 5 tiles)
    Event ev_done, ev_clear;   // end of the last call; a channel ring cleared after it
    bool done_any = false, clear_pending = false;
    // the demod scope (jsdr_demod_scope_*): all of it empty until the first scope call
    struct Scope {
        DevBuf<float2> dbg;    // [frames of a pass][n] mixed IQ, when the caller takes no dbg rows
        DevBuf<float> fin;     // [frames of a pass][n] final floats (trace)
        DevBuf<float> psd;     // [frames of a pass][n + 2] (spectrum)
        DevBuf<int> tab;       // int[4][width]: the column schedules of tab_width
        int tab_width = 0;
        DemodScopeFft fft;     // jsdr_fft of n samples (spectrum)
        int chunk = 0;         // jsdr_demod_scope_chunk; 0: the default
        std::string kernel;
    } scope;
};

enum { DK_NCO = 0, DK_FRONT, DK_STATE, DK_MEAN, DK_OUT, DK_CHAN, DK_COUNT };
// (DK_CHAN: every launch of a channel handle but the shared k_demod_nco / k_demod_mean)
static const char *const kDemodKernels[DK_COUNT] = {"k_demod_nco", "k_demod_front", "k_demod_state", "k_demod_mean",
                                                    "k_demod_out", "k_demod_chan"};
struct DemodProf {
    jsdr_demod *h;
    hipStream_t st;
    Event a, b;
    int k;
    static Event get(jsdr_demod *h)
    {
        Event e;
        if (h->pool.empty()) {
            (void)e.create();  // (none: the scope records nothing)
        } else {
            e = std::move(h->pool.back());
            h->pool.pop_back();
        }
        return e;
    }
    DemodProf(jsdr_demod *h_, int k_, hipStream_t st_) : h(h_), st(st_), k(k_)
    {
        if (h->prof_on) {
            a = get(h);
            b = get(h);
            (void)hipEventRecord(a, st);
        }
    }
    ~DemodProf()
    {
        if (h->prof_on && a && b) {
            (void)hipEventRecord(b, st);
            h->recs.push_back({k, std::move(a), std::move(b)});
        }
    }
};

static double dsinl(double x) { return (double)sinl((long double)x); }
static double dcosl(double x) { return (double)cosl((long double)x); }

// demod.weights() (:341-375) for the band [flo, fhi] at `rate` into w; a band-pass (false for flo = INT_MIN, the all-pass
// impulse) also sets phi
static bool demod_weights_of(int rate, int flo, int fhi, float w[21], float *phi)
{
    const int len = 21;
    if ((-2147483647 - 1) == flo) {
        for (int i = 0; i < len; i++) w[i] = 0;
        w[(len - 1) / 2] = 1;
        return false;
    }
    const float frate = (float)rate;
    const float nlo = (float)flo / frate;
    const float nhi = (float)fhi / frate;
    const int ord = len - 1;
    const double PI = 3.14159265358979323846;
    for (int n = 0; n < len; n++) {
        if (n == ord / 2) {
            w[n] = 2.0f * (nhi - nlo);
        } else {
            w[n] = (float)((dsinl(2 * PI * nhi * (double)(n - ord / 2)) / (PI * (double)(n - ord / 2))) -
                           (dsinl(2 * PI * nlo * (double)(n - ord / 2)) / (PI * (double)(n - ord / 2))));
        }
        w[n] *= (float)(0.54 - 0.46 * dcosl(2 * PI * (double)n / (double)ord));
    }
    *phi = (float)(2 * PI * nlo);
    return true;
}

template <bool F32IN>
static int demod_run(jsdr_demod *h, const int16_t *raw_dev, const float *rawf_dev, int64_t stride_i16, int64_t L, int ic,
                     int qc, int16_t *audio_dev, int64_t audio_stride_i16, hipStream_t st)
{
    JSDR_REQUIRE(h, "demod: null handle");
    JSDR_REQUIRE((raw_dev || rawf_dev) && audio_dev, "demod: null buffer");
    JSDR_REQUIRE(L > 0 && L <= h->max_batch && L % h->n == 0,
                 "demod: nsamples=%lld must be a positive multiple of the frame (%d) and at most max_batch_samples=%lld",
                 (long long)L, h->n, h->max_batch);
    JSDR_REQUIRE((stride_i16 & 1) == 0 && (h->nstreams == 1 || stride_i16 >= 2 * L) && (audio_stride_i16 & 1) == 0 &&
                     (h->nstreams == 1 || audio_stride_i16 >= 2 * L),
                 "demod: stream stride too small for %lld samples", (long long)L);
    const int S = h->nstreams;
    const int nfr = (int)(L / h->n);
    DemodArgs a;
    a.raw = reinterpret_cast<const int *>(raw_dev);
    a.rawf = reinterpret_cast<const float2 *>(rawf_dev);
    a.stride_pairs = stride_i16 / 2;
    a.L = L;
    a.n = h->n;
    a.nfr = nfr;
    a.ic = ic;
    a.qc = qc;
    a.hist = h->hist[h->cur].p;
    a.lilq = h->lilq[h->cur].p;
    const int set = (int)(h->calls++ & 1);
    a.nco = h->nco[set].p;
    a.d = h->d.p;
    a.fmax_bits = h->fmax.p;
    memcpy(a.c.w, h->wfir, sizeof(a.c.w));
    a.c.fmgain = (float)h->rate / (MODE_NFM == h->mode ? 5000.0f : 75000.0f);  // :410
    a.c.mode = h->mode;
    a.c.dofir = h->dofir;
    a.c.dodwn = h->dodwn;
    a.c.doagc = h->doagc;
    if (h->dodwn) {
        // :427-429 in float, exactly as the reference steps it
        if (h->used[set]) JSDR_HIP_TRY(hipEventSynchronize(h->ev_used[set]));  // the call before last has let go of this set
        float *tab = h->car_pinned[set].p;
        float car = h->car;
        const float phi = h->phi, two_pi = (float)(2 * 3.14159265358979323846);
        // a serial float recurrence, on the host; kept as a (well predicted) branch so that the dependent chain per
        // sample is the one subtraction -- as a select it is subtract + add + blend, four times slower, and longer
        // than the GPU takes for the whole batch
        for (int64_t g = 0; g < L; g++) {
            tab[g] = car;
            car -= phi;
            if (__builtin_expect(car < 0.0f, 0)) {
                asm volatile("" : "+x"(car));
                car += two_pi;
            }
        }
        h->car = car;
        JSDR_HIP_TRY(hipMemcpyAsync(h->car_dev[set].p, tab, sizeof(float) * (size_t)L, hipMemcpyHostToDevice, h->copy_stream));
        {
            DemodProf ps(h, DK_NCO, h->copy_stream);
            hipLaunchKernelGGL(k_demod_nco, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, h->copy_stream, h->car_dev[set].p,
                               (long long)L, h->nco[set].p);
            JSDR_LAUNCH_CHECK();
        }
        JSDR_HIP_TRY(hipEventRecord(h->ev_table[set], h->copy_stream));
        JSDR_HIP_TRY(hipStreamWaitEvent(st, h->ev_table[set], 0));
    }
    const int tiles_per_frame = (h->n + DTILE - 1) / DTILE;
    // every mode but AM, frames of up to 5 tiles (the reference's 9600-sample default included): one kernel from
    // raw samples to int16 audio; JSDR_DEMOD_FUSED=0 keeps the three-kernel path for A/B runs
    static const bool fused_ok = [] {
        const char *e = knob("JSDR_DEMOD_FUSED");
        return !(e && e[0] == '0');
    }();
    const bool fused = fused_ok && h->mode != MODE_AM && tiles_per_frame <= 5;
    if (fused) {
        DemodProf ps(h, DK_FRONT, st);
        int *outp = reinterpret_cast<int *>(audio_dev);
        const long long osp = (long long)(audio_stride_i16 / 2);
        const dim3 grid((unsigned)nfr, (unsigned)S);  // (streams fastest instead, for carrier-table locality: measured, no gain)
        switch (tiles_per_frame) {
            case 1: hipLaunchKernelGGL((k_demod_fused<F32IN, 1>), grid, dim3(256), 0, st, a, outp, osp, h->stats.p); break;
            case 2: hipLaunchKernelGGL((k_demod_fused<F32IN, 2>), grid, dim3(256), 0, st, a, outp, osp, h->stats.p); break;
            case 3: hipLaunchKernelGGL((k_demod_fused<F32IN, 3>), grid, dim3(256), 0, st, a, outp, osp, h->stats.p); break;
            case 4: hipLaunchKernelGGL((k_demod_fused<F32IN, 4>), grid, dim3(256), 0, st, a, outp, osp, h->stats.p); break;
            default: hipLaunchKernelGGL((k_demod_fused<F32IN, 5>), grid, dim3(256), 0, st, a, outp, osp, h->stats.p); break;
        }
        JSDR_LAUNCH_CHECK();
    } else {
        JSDR_HIP_TRY(hipMemsetAsync(h->fmax.p, 0, sizeof(unsigned) * (size_t)S * nfr, st));
        DemodProf ps(h, DK_FRONT, st);
        hipLaunchKernelGGL(k_demod_front<F32IN>, dim3((unsigned)(tiles_per_frame * nfr), (unsigned)S), dim3(256), 0, st, a);
        JSDR_LAUNCH_CHECK();
    }
    {
        DemodProf ps(h, DK_STATE, st);
        hipLaunchKernelGGL(k_demod_state<F32IN>, dim3((unsigned)S), dim3(64), 0, st, a, h->hist[h->cur ^ 1].p,
                           h->lilq[h->cur ^ 1].p, S);
        JSDR_LAUNCH_CHECK();
    }
    h->cur ^= 1;
    const long long nft = (long long)S * nfr;
    if (h->mode == MODE_AM) {
        DemodProf ps(h, DK_MEAN, st);
        hipLaunchKernelGGL(k_demod_mean, dim3((unsigned)((nft + 63) / 64)), dim3(64), 0, st, h->d.p, (long long)L, h->n, nfr,
                           nft, h->favg.p);
        JSDR_LAUNCH_CHECK();
    }
    if (!fused) {
        DemodProf ps(h, DK_OUT, st);
        hipLaunchKernelGGL(k_demod_out, dim3((unsigned)((h->n + 1023) / 1024), (unsigned)nfr, (unsigned)S), dim3(256), 0, st, h->d.p, (long long)L,
                           h->n, nfr, h->mode, h->doagc, h->fmax.p, h->favg.p, reinterpret_cast<int *>(audio_dev),
                           (long long)(audio_stride_i16 / 2), h->stats.p);
        JSDR_LAUNCH_CHECK();
    }
    if (h->dodwn) {
        JSDR_HIP_TRY(hipEventRecord(h->ev_used[set], st));
        h->used[set] = true;
    }
    h->last_nfr = nfr;
    return JSDR_OK;
}

// one call of a channel handle: stride_i16 between INPUTS, audio_stride_i16 between the nin * nch output rows
template <bool F32IN>
static int demod_chan_run(jsdr_demod *h, const int16_t *raw_dev, const float *rawf_dev, int64_t stride_i16, int64_t L, int ic,
                          int qc, int16_t *audio_dev, int64_t audio_stride_i16, hipStream_t st)
{
    JSDR_REQUIRE((raw_dev || rawf_dev) && audio_dev, "demod: null buffer");
    JSDR_REQUIRE(L > 0 && L <= h->max_batch && L % h->n == 0,
                 "demod: nsamples=%lld must be a positive multiple of the frame (%d) and at most max_batch_samples=%lld",
                 (long long)L, h->n, h->max_batch);
    JSDR_REQUIRE((stride_i16 & 1) == 0 && (h->nin == 1 || stride_i16 >= 2 * L) && (audio_stride_i16 & 1) == 0 &&
                     (h->nstreams == 1 || audio_stride_i16 >= 2 * L),
                 "demod: input or output row stride too small for %lld samples", (long long)L);
    const int K = h->nch;
    const int nfr = (int)(L / h->n);
    const bool fused = (h->n + DTILE - 1) / DTILE <= 5;
    DemodChanArgs a = {};
    // float rows in d: the AM channels (their mean needs the whole frame), then, for frames above 5 tiles, every other one
    int nslots = 0;
    for (int c = 0; c < K; c++) {
        a.c[c].dslot = -1;
        if (h->ch[c].mode == MODE_AM) {
            a.c[c].dslot = nslots;
            a.slot_chan[nslots++] = c;
        }
    }
    const int nam = nslots;
    if (!fused)
        for (int c = 0; c < K; c++)
            if (h->ch[c].mode != MODE_AM) {
                a.c[c].dslot = nslots;
                a.slot_chan[nslots++] = c;
            }
    const int drows = nslots * h->nin;
    if ((size_t)drows * (size_t)L > h->dch.n) {
        JSDR_HIP_TRY(hipDeviceSynchronize());  // earlier calls may still use the smaller buffer
        if (h->dch.alloc((size_t)drows * (size_t)L) != JSDR_OK) return JSDR_ERR;
    }
    // distinct carrier tables: one per (car, phi) among the down-converting channels
    int rows = 0;
    uint32_t key[DCHAN_MAX][2];
    for (int c = 0; c < K; c++) {
        a.c[c].nco_row = 0;
        if (!h->ch[c].dodwn) continue;
        uint32_t k2[2];
        memcpy(&k2[0], &h->ch[c].car, 4);
        memcpy(&k2[1], &h->ch[c].phi, 4);
        int r = 0;
        while (r < rows && (key[r][0] != k2[0] || key[r][1] != k2[1])) r++;
        if (r == rows) {
            key[r][0] = k2[0];
            key[r][1] = k2[1];
            rows++;
        }
        a.c[c].nco_row = r;
    }
    const int set = (int)(h->calls++ & 1);
    if (rows) {
        if (h->used[set]) JSDR_HIP_TRY(hipEventSynchronize(h->ev_used[set]));  // the call before last has let go of this set
        float endcar[DCHAN_MAX];
        // :427-429 in float, exactly as demod_run steps it; one host thread per distinct table
        auto build = [&](int r) {
            float *tab = h->car_pinned[set].p + (size_t)r * h->nco_pitch;
            float car, phi;
            memcpy(&car, &key[r][0], 4);
            memcpy(&phi, &key[r][1], 4);
            const float two_pi = (float)(2 * 3.14159265358979323846);
            for (int64_t g = 0; g < L; g++) {
                tab[g] = car;
                car -= phi;
                if (__builtin_expect(car < 0.0f, 0)) {
                    asm volatile("" : "+x"(car));
                    car += two_pi;
                }
            }
            endcar[r] = car;
        };
        if (rows == 1 || L < 65536) {  // (a thread start costs more than a short table)
            for (int r = 0; r < rows; r++) build(r);
        } else {
            std::vector<std::thread> th;
            for (int r = 0; r < rows; r++) th.emplace_back(build, r);
            for (auto &t : th) t.join();
        }
        for (int c = 0; c < K; c++)
            if (h->ch[c].dodwn) h->ch[c].car = endcar[a.c[c].nco_row];
        const long long cnt = (long long)(rows - 1) * h->nco_pitch + L;
        JSDR_HIP_TRY(hipMemcpyAsync(h->car_dev[set].p, h->car_pinned[set].p, sizeof(float) * (size_t)cnt, hipMemcpyHostToDevice,
                                    h->copy_stream));
        {
            DemodProf ps(h, DK_NCO, h->copy_stream);
            hipLaunchKernelGGL(k_demod_nco, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->copy_stream, h->car_dev[set].p,
                               cnt, h->nco[set].p);
            JSDR_LAUNCH_CHECK();
        }
        JSDR_HIP_TRY(hipEventRecord(h->ev_table[set], h->copy_stream));
        JSDR_HIP_TRY(hipStreamWaitEvent(st, h->ev_table[set], 0));
    }
    if (h->clear_pending) {  // a channel's ring cleared since the last call
        JSDR_HIP_TRY(hipStreamWaitEvent(st, h->ev_clear, 0));
        h->clear_pending = false;
    }
    a.raw = reinterpret_cast<const int *>(raw_dev);
    a.rawf = reinterpret_cast<const float2 *>(rawf_dev);
    a.stride_pairs = stride_i16 / 2;
    a.L = L;
    a.n = h->n;
    a.nfr = nfr;
    a.ic = ic;
    a.qc = qc;
    a.ninputs = h->nin;
    a.K = K;
    a.hist = h->hist[h->cur].p;
    a.lilq = h->lilq[h->cur].p;
    a.nco = h->nco[set].p;
    a.nco_pitch = h->nco_pitch;
    a.d = h->dch.p;
    a.fmax_bits = h->fmax.p;
    a.out = reinterpret_cast<int *>(audio_dev);
    a.out_stride_pairs = audio_stride_i16 / 2;
    a.stats = h->stats.p;
    for (int c = 0; c < K; c++) {
        const jsdr_demod::Chan &ch = h->ch[c];
        memcpy(a.c[c].w, ch.w, sizeof(a.c[c].w));
        a.c[c].fmgain = (float)h->rate / (MODE_NFM == ch.mode ? 5000.0f : 75000.0f);  // :410
        a.c[c].mode = ch.mode;
        a.c[c].dofir = ch.dofir;
        a.c[c].dodwn = ch.dodwn;
        a.c[c].doagc = ch.doagc;
    }
    if (!fused) JSDR_HIP_TRY(hipMemsetAsync(h->fmax.p, 0, sizeof(unsigned) * (size_t)drows * nfr, st));
    {
        DemodProf ps(h, DK_CHAN, st);
        if (launch_demod_chan(a, F32IN, fused, st) != JSDR_OK) return JSDR_ERR;
    }
    {
        DemodProf ps(h, DK_CHAN, st);
        if (launch_demod_chan_state(a, F32IN, h->hist[h->cur ^ 1].p, h->lilq[h->cur ^ 1].p, st) != JSDR_OK) return JSDR_ERR;
    }
    h->cur ^= 1;
    if (nam) {
        const long long nft = (long long)nam * h->nin * nfr;  // the AM rows come first
        DemodProf ps(h, DK_MEAN, st);
        hipLaunchKernelGGL(k_demod_mean, dim3((unsigned)((nft + 63) / 64)), dim3(64), 0, st, h->dch.p, (long long)L, h->n, nfr,
                           nft, h->favg.p);
        JSDR_LAUNCH_CHECK();
    }
    if (drows) {
        DemodProf ps(h, DK_CHAN, st);
        if (launch_demod_chan_out(a, drows, h->favg.p, st) != JSDR_OK) return JSDR_ERR;
    }
    if (rows) {
        JSDR_HIP_TRY(hipEventRecord(h->ev_used[set], st));
        h->used[set] = true;
    }
    JSDR_HIP_TRY(hipEventRecord(h->ev_done, st));
    h->done_any = true;
    h->last_nfr = nfr;
    return JSDR_OK;
}

// receive(float[]) of a 1-input channel handle: one frame in, nch frames of audio out (channel c at c * 2n)
static int demod_chan_receive(jsdr_demod *h, const float *buf_host, int16_t *audio_host)
{
    JSDR_REQUIRE(h->nin == 1, "jsdr_demod_receive_f32: the frame-by-frame form needs a 1-input handle");
    const size_t in_bytes = sizeof(float) * 2 * (size_t)h->n, out_bytes = sizeof(int) * (size_t)h->n * h->nch;
    if (!h->pin_tried) {
        h->pin.alloc(in_bytes + out_bytes);
        h->pin_tried = true;
    }
    if (h->pin.p) {
        memcpy(h->pin.p, buf_host, in_bytes);
        SyncOnExit guard;
        JSDR_HIP_TRY(hipMemcpyAsync(h->stage_in.p, h->pin.p, in_bytes, hipMemcpyHostToDevice, 0));
        if (demod_chan_run<true>(h, nullptr, h->stage_in.p, 2 * (int64_t)h->n, h->n, 0, 0,
                                 reinterpret_cast<int16_t *>(h->stage_out.p), 2 * (int64_t)h->n, 0) != JSDR_OK)
            return JSDR_ERR;
        JSDR_HIP_TRY(hipMemcpyAsync(h->pin.p + in_bytes, h->stage_out.p, out_bytes, hipMemcpyDeviceToHost, 0));
        JSDR_HIP_TRY(hipStreamSynchronize(0));
        guard.armed = false;
        memcpy(audio_host, h->pin.p + in_bytes, out_bytes);
        return JSDR_OK;
    }
    JSDR_HIP_TRY(hipMemcpy(h->stage_in.p, buf_host, in_bytes, hipMemcpyHostToDevice));
    if (demod_chan_run<true>(h, nullptr, h->stage_in.p, 2 * (int64_t)h->n, h->n, 0, 0, reinterpret_cast<int16_t *>(h->stage_out.p),
                             2 * (int64_t)h->n, 0) != JSDR_OK)
        return JSDR_ERR;
    JSDR_HIP_TRY(hipMemcpy(audio_host, h->stage_out.p, out_bytes, hipMemcpyDeviceToHost));
    return JSDR_OK;
}

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

template <bool F32IN>
static int demod_scope_run(const char *who, jsdr_demod *h, const int16_t *raw_dev, const float *rawf_dev, int64_t stride_i16,
                           int64_t L, int ic, int qc, int16_t *audio_dev, int64_t audio_stride_i16, int width, int height,
                           int32_t *trace_dev, int32_t *spec_dev, float *dbg_dev, hipStream_t st)
{
    const char *in_name = F32IN ? "iq_dev" : "raw_dev", *stride_name = F32IN ? "stream_stride_f32" : "stream_stride_i16";
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
        return demod_run<F32IN>(h, raw_dev, rawf_dev, stride_i16, L, ic, qc, audio_dev, audio_stride_i16, st);
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
    DemodArgs a;
    a.raw = reinterpret_cast<const int *>(raw_dev);
    a.rawf = reinterpret_cast<const float2 *>(rawf_dev);
    a.stride_pairs = stride_i16 / 2;
    a.L = L;
    a.n = n;
    a.nfr = nfr;
    a.ic = ic;
    a.qc = qc;
    a.hist = h->hist[h->cur].p;
    a.lilq = h->lilq[h->cur].p;
    const int set = (int)(h->calls & 1);
    a.nco = h->nco[set].p;
    a.d = nullptr;
    a.fmax_bits = nullptr;
    memcpy(a.c.w, h->wfir, sizeof(a.c.w));
    a.c.fmgain = (float)h->rate / (MODE_NFM == h->mode ? 5000.0f : 75000.0f);  // :410
    a.c.mode = h->mode;
    a.c.dofir = h->dofir;
    a.c.dodwn = h->dodwn;
    a.c.doagc = h->doagc;
    if (demod_run<F32IN>(h, raw_dev, rawf_dev, stride_i16, L, ic, qc, audio_dev, audio_stride_i16, st) != JSDR_OK) return JSDR_ERR;
    if ((trace_dev || spec_dev) && sc.tab_width != width) {  // on the caller's stream, behind the previous call's readers
        sc.tab_width = 0;
        if (launch_demod_scope_layout(n, width, sc.tab.p, st) != JSDR_OK) return JSDR_ERR;
        sc.tab_width = width;
    }
    for (long long r0 = 0; r0 < rows; r0 += fpp) {
        const int nr = (int)(rows - r0 < fpp ? rows - r0 : fpp);
        float2 *dbg_rows = dbg_dev ? reinterpret_cast<float2 *>(dbg_dev) + (size_t)r0 * n : sc.dbg.p;
        if (launch_demod_scope_front(a, F32IN, h->stats.p, r0, nr, dbg_rows, trace_dev ? sc.fin.p : nullptr, st) != JSDR_OK)
            return JSDR_ERR;
        if (trace_dev &&
            launch_demod_trace(sc.fin.p, dbg_rows, n, h->mode == MODE_OFF, nr, width, height / 4, sc.tab.p,
                               trace_dev + (size_t)r0 * width, st) != JSDR_OK)
            return JSDR_ERR;
        if (spec_dev) {
            if (jsdr_fft_batch_f32(sc.fft.h, reinterpret_cast<const float *>(dbg_rows), nr, sc.psd.p, st) != JSDR_OK) return JSDR_ERR;
            if (launch_demod_spec(sc.psd.p, n, nr, width, height / 2, sc.tab.p, spec_dev + (size_t)r0 * width, st) != JSDR_OK)
                return JSDR_ERR;
        }
    }
    if (h->dodwn) JSDR_HIP_TRY(hipEventRecord(h->ev_used[set], st));  // the passes read the carrier table too
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
    return demod_scope_run<false>("jsdr_demod_scope_i16", h, raw_dev, nullptr, stream_stride_i16, nsamples, ic, qc, audio_dev,
                                  audio_stride_i16, width, height, trace_dev, spec_dev, dbg_dev, as_stream(stream));
}

int jsdr_demod_scope_f32(jsdr_demod *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples, int16_t *audio_dev,
                         int64_t audio_stride_i16, int width, int height, int32_t *trace_dev, int32_t *spec_dev, float *dbg_dev,
                         void *stream)
{
    return demod_scope_run<true>("jsdr_demod_scope_f32", h, nullptr, iq_dev, stream_stride_f32, nsamples, 0, 0, audio_dev,
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

int jsdr_demod_create(jsdr_demod **out, int rate, int nsamples_per_frame, int nstreams, int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_demod_create: null handle pointer");
    *out = nullptr;
    JSDR_REQUIRE(rate > 0 && nsamples_per_frame > 0 && nstreams > 0, "jsdr_demod_create: rate, frame and nstreams must be positive");
    if (max_batch_samples <= 0) max_batch_samples = nsamples_per_frame;
    JSDR_REQUIRE(max_batch_samples % nsamples_per_frame == 0, "jsdr_demod_create: max_batch_samples must be whole frames");
    JSDR_REQUIRE(nstreams <= 65535 && max_batch_samples / nsamples_per_frame <= 65535,
                 "jsdr_demod_create: at most 65535 streams and 65535 frames per call");
    JSDR_REQUIRE((long long)nstreams * (max_batch_samples / nsamples_per_frame) < (1LL << 31) &&
                     (max_batch_samples / nsamples_per_frame) * ((nsamples_per_frame + DTILE - 1) / DTILE) < (1LL << 31),
                 "jsdr_demod_create: batch too large");
    jsdr_demod *h = new jsdr_demod();
    h->rate = rate;
    h->n = nsamples_per_frame;
    h->nstreams = nstreams;
    h->max_batch = max_batch_samples;
    const size_t S = (size_t)nstreams, L = (size_t)max_batch_samples, nf = S * (L / (size_t)h->n);
    bool ok = true;
    for (int k = 0; k < 2; k++)
        ok = ok && h->hist[k].alloc(S * DHALO) == JSDR_OK && h->lilq[k].alloc(S) == JSDR_OK && h->hist[k].zero() == JSDR_OK &&
             h->lilq[k].zero() == JSDR_OK;
    for (int k = 0; k < 2; k++)
        ok = ok && h->nco[k].alloc(L + 8) == JSDR_OK && h->nco[k].zero() == JSDR_OK && h->car_dev[k].alloc(L) == JSDR_OK &&
             h->car_pinned[k].alloc(sizeof(float) * L) && h->ev_table[k].create(hipEventDisableTiming) == JSDR_OK &&
             h->ev_used[k].create(hipEventDisableTiming) == JSDR_OK;
    ok = ok && h->copy_stream.create(hipStreamNonBlocking) == JSDR_OK;
    ok = ok && h->d.alloc(S * L) == JSDR_OK &&
         h->favg.alloc(nf) == JSDR_OK && h->stats.alloc(2 * nf) == JSDR_OK && h->fmax.alloc(nf) == JSDR_OK &&
         h->stage_in.alloc(2 * (size_t)h->n) == JSDR_OK && h->stage_out.alloc((size_t)h->n) == JSDR_OK &&
         h->favg.zero() == JSDR_OK && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        jsdr_demod_destroy(h);
        return JSDR_ERR;
    }
    *out = h;
    return JSDR_OK;
}

int jsdr_demod_destroy(jsdr_demod *h)
{
    if (!h) return JSDR_OK;
    (void)hipDeviceSynchronize();
    delete h;
    return JSDR_OK;
}

int jsdr_demod_profile_enable(jsdr_demod *h, int on)
{
    JSDR_REQUIRE(h, "jsdr_demod_profile_enable: null handle");
    h->prof_on = on != 0;
    return JSDR_OK;
}
int jsdr_demod_profile_count(void) { return DK_COUNT; }
const char *jsdr_demod_profile_name(int k) { return (k >= 0 && k < DK_COUNT) ? kDemodKernels[k] : ""; }
int jsdr_demod_profile_read(jsdr_demod *h, double *ms_total, int *launches)
{
    JSDR_REQUIRE(h && ms_total && launches, "jsdr_demod_profile_read: null argument");
    for (int k = 0; k < DK_COUNT; k++) {
        ms_total[k] = 0.0;
        launches[k] = 0;
    }
    for (auto &r : h->recs) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            ms_total[r.k] += ms;
            launches[r.k]++;
        }
        h->pool.push_back(std::move(r.a));
        h->pool.push_back(std::move(r.b));
    }
    h->recs.clear();
    return JSDR_OK;
}

int jsdr_demod_configure(jsdr_demod *h, int mode, int dofir, int dodwn, int doagc)
{
    JSDR_REQUIRE(h, "jsdr_demod_configure: null handle");
    JSDR_REQUIRE(mode >= MODE_OFF && mode <= MODE_WFM, "jsdr_demod_configure: mode %d outside 0..4 (demod.java:39-43)", mode);
    for (auto &c : h->ch) {  // a channel handle: every channel
        c.mode = mode;
        c.dofir = dofir != 0;
        c.dodwn = dodwn != 0;
        c.doagc = doagc != 0;
    }
    h->mode = mode;
    h->dofir = dofir != 0;
    h->dodwn = dodwn != 0;
    h->doagc = doagc != 0;
    return JSDR_OK;
}

// demod.weights() (:341-375) for the given band; clears the delay lines of every stream
int jsdr_demod_weights(jsdr_demod *h, int flo, int fhi, float w_out[21], float *phi_out)
{
    JSDR_REQUIRE(h, "jsdr_demod_weights: null handle");
    if (h->chan) {  // every channel
        float w[21], phi = 0.0f;
        const bool bandpass = demod_weights_of(h->rate, flo, fhi, w, &phi);
        for (auto &c : h->ch) {
            c.flo = flo;
            c.fhi = fhi;
            memcpy(c.w, w, sizeof(w));
            if (bandpass) {
                c.phi = phi;
                c.car = 0.0f;
            }
        }
        JSDR_HIP_TRY(hipDeviceSynchronize());
        if (h->hist[0].zero() != JSDR_OK || h->hist[1].zero() != JSDR_OK) return JSDR_ERR;
        JSDR_HIP_TRY(hipDeviceSynchronize());
        if (w_out) memcpy(w_out, w, sizeof(w));
        if (phi_out) *phi_out = h->ch[0].phi;
        return JSDR_OK;
    }
    h->flo = flo;
    h->fhi = fhi;
    if (demod_weights_of(h->rate, flo, fhi, h->wfir, &h->phi)) h->car = 0.0f;
    JSDR_HIP_TRY(hipDeviceSynchronize());
    if (h->hist[0].zero() != JSDR_OK || h->hist[1].zero() != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipDeviceSynchronize());
    if (w_out) memcpy(w_out, h->wfir, sizeof(h->wfir));
    if (phi_out) *phi_out = h->phi;
    return JSDR_OK;
}

int jsdr_demod_batch_i16(jsdr_demod *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc,
                         int16_t *audio_dev, int64_t audio_stride_i16, void *stream)
{
    if (h && h->chan)
        return demod_chan_run<false>(h, raw_dev, nullptr, stream_stride_i16, nsamples, ic, qc, audio_dev, audio_stride_i16,
                                     as_stream(stream));
    return demod_run<false>(h, raw_dev, nullptr, stream_stride_i16, nsamples, ic, qc, audio_dev, audio_stride_i16,
                            as_stream(stream));
}

int jsdr_demod_batch_f32(jsdr_demod *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples, int16_t *audio_dev,
                         int64_t audio_stride_i16, void *stream)
{
    if (h && h->chan)
        return demod_chan_run<true>(h, nullptr, iq_dev, stream_stride_f32, nsamples, 0, 0, audio_dev, audio_stride_i16,
                                    as_stream(stream));
    return demod_run<true>(h, nullptr, iq_dev, stream_stride_f32, nsamples, 0, 0, audio_dev, audio_stride_i16,
                           as_stream(stream));
}

// IAudioHandler.receive(float[]) of a single-stream handle: one frame in, the frame's audio bytes out
int jsdr_demod_receive_f32(jsdr_demod *h, const float *buf_host, int16_t *audio_host)
{
    JSDR_REQUIRE(h && buf_host && audio_host, "jsdr_demod_receive_f32: null argument");
    if (h->chan) return demod_chan_receive(h, buf_host, audio_host);
    JSDR_REQUIRE(h->nstreams == 1, "jsdr_demod_receive_f32: the frame-by-frame form needs a 1-stream handle");
    const size_t in_bytes = sizeof(float) * 2 * (size_t)h->n, out_bytes = sizeof(int) * (size_t)h->n;
    if (!h->pin_tried) {  // the first receive() of the handle (PinnedStage, common.h)
        h->pin.alloc(in_bytes + out_bytes);
        h->pin_tried = true;
    }
    if (h->pin.p) {
        memcpy(h->pin.p, buf_host, in_bytes);
        SyncOnExit guard;  // (an error exit below must not leave the device reading or writing the stage)
        JSDR_HIP_TRY(hipMemcpyAsync(h->stage_in.p, h->pin.p, in_bytes, hipMemcpyHostToDevice, 0));
        if (demod_run<true>(h, nullptr, h->stage_in.p, 2 * (int64_t)h->n, h->n, 0, 0, reinterpret_cast<int16_t *>(h->stage_out.p),
                            2 * (int64_t)h->n, 0) != JSDR_OK)
            return JSDR_ERR;
        JSDR_HIP_TRY(hipMemcpyAsync(h->pin.p + in_bytes, h->stage_out.p, out_bytes, hipMemcpyDeviceToHost, 0));
        JSDR_HIP_TRY(hipStreamSynchronize(0));
        guard.armed = false;
        memcpy(audio_host, h->pin.p + in_bytes, out_bytes);
        return JSDR_OK;
    }
    JSDR_HIP_TRY(hipMemcpy(h->stage_in.p, buf_host, in_bytes, hipMemcpyHostToDevice));
    if (demod_run<true>(h, nullptr, h->stage_in.p, 2 * (int64_t)h->n, h->n, 0, 0, reinterpret_cast<int16_t *>(h->stage_out.p),
                        2 * (int64_t)h->n, 0) != JSDR_OK)
        return JSDR_ERR;
    JSDR_HIP_TRY(hipMemcpy(audio_host, h->stage_out.p, out_bytes, hipMemcpyDeviceToHost));
    return JSDR_OK;
}

// the reference's `max` and `avg` fields as the last frame of the last call left them (:465-467)
int jsdr_demod_frame_stats(jsdr_demod *h, int stream, float *max_out, float *avg_out)
{
    JSDR_REQUIRE(h && max_out && avg_out, "jsdr_demod_frame_stats: null argument");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_demod_frame_stats: stream %d outside 0..%d", stream, h->nstreams - 1);
    JSDR_REQUIRE(h->last_nfr > 0, "jsdr_demod_frame_stats: nothing processed yet");
    float v[2];
    JSDR_HIP_TRY(hipDeviceSynchronize());
    JSDR_HIP_TRY(hipMemcpy(v, h->stats.p + 2 * ((size_t)stream * h->last_nfr + (h->last_nfr - 1)), sizeof(v), hipMemcpyDeviceToHost));
    *max_out = v[0];
    *avg_out = v[1];
    return JSDR_OK;
}

int jsdr_demod_state(jsdr_demod *h, float *car_out, float *phi_out)
{
    JSDR_REQUIRE(h, "jsdr_demod_state: null handle");
    if (car_out) *car_out = h->chan ? h->ch[0].car : h->car;  // a channel handle: channel 0
    if (phi_out) *phi_out = h->chan ? h->ch[0].phi : h->phi;
    return JSDR_OK;
}

int jsdr_demod_create_channels(jsdr_demod **out, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                               int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_demod_create_channels: null handle pointer");
    *out = nullptr;
    JSDR_REQUIRE(rate > 0 && nsamples_per_frame > 0, "jsdr_demod_create_channels: rate and nsamples_per_frame must be positive");
    JSDR_REQUIRE(ninputs >= 1, "jsdr_demod_create_channels: ninputs = %d, at least 1", ninputs);
    JSDR_REQUIRE(nchannels >= 1 && nchannels <= DCHAN_MAX, "jsdr_demod_create_channels: nchannels = %d outside 1..%d", nchannels,
                 (int)DCHAN_MAX);
    if (max_batch_samples <= 0) max_batch_samples = nsamples_per_frame;
    JSDR_REQUIRE(max_batch_samples % nsamples_per_frame == 0, "jsdr_demod_create_channels: max_batch_samples must be whole frames");
    const long long S = (long long)ninputs * nchannels, nf = max_batch_samples / nsamples_per_frame;
    JSDR_REQUIRE(S <= 65535, "jsdr_demod_create_channels: ninputs * nchannels = %lld streams, at most 65535", S);
    JSDR_REQUIRE(nf <= 65535, "jsdr_demod_create_channels: max_batch_samples is %lld frames, at most 65535", nf);
    JSDR_REQUIRE(S * nf < (1LL << 31) && nf * ((nsamples_per_frame + DTILE - 1) / DTILE) < (1LL << 31),
                 "jsdr_demod_create_channels: batch too large");
    jsdr_demod *h = new jsdr_demod();
    h->chan = true;
    h->rate = rate;
    h->n = nsamples_per_frame;
    h->nin = ninputs;
    h->nch = nchannels;
    h->nstreams = (int)S;
    h->max_batch = max_batch_samples;
    h->ch.resize((size_t)nchannels);
    h->nco_pitch = (max_batch_samples + 8 + 1) & ~1LL;  // even: every table 16-byte aligned; spare slots past each
    const size_t tab = (size_t)nchannels * (size_t)h->nco_pitch, nfs = (size_t)S * (size_t)nf;
    bool ok = true;
    for (int k = 0; k < 2; k++)
        ok = ok && h->hist[k].alloc((size_t)S * DHALO) == JSDR_OK && h->lilq[k].alloc((size_t)S) == JSDR_OK &&
             h->hist[k].zero() == JSDR_OK && h->lilq[k].zero() == JSDR_OK;
    for (int k = 0; k < 2; k++)
        ok = ok && h->nco[k].alloc(tab) == JSDR_OK && h->nco[k].zero() == JSDR_OK && h->car_dev[k].alloc(tab) == JSDR_OK &&
             h->car_pinned[k].alloc(sizeof(float) * tab) && h->ev_table[k].create(hipEventDisableTiming) == JSDR_OK &&
             h->ev_used[k].create(hipEventDisableTiming) == JSDR_OK;
    ok = ok && h->copy_stream.create(hipStreamNonBlocking) == JSDR_OK && h->ev_done.create(hipEventDisableTiming) == JSDR_OK &&
         h->ev_clear.create(hipEventDisableTiming) == JSDR_OK;
    ok = ok && h->favg.alloc(nfs) == JSDR_OK && h->stats.alloc(2 * nfs) == JSDR_OK && h->fmax.alloc(nfs) == JSDR_OK &&
         h->stage_in.alloc(2 * (size_t)h->n) == JSDR_OK && h->stage_out.alloc((size_t)h->n * nchannels) == JSDR_OK &&
         h->favg.zero() == JSDR_OK && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        jsdr_demod_destroy(h);
        return JSDR_ERR;
    }
    *out = h;
    return JSDR_OK;
}

int jsdr_demod_channel_info(jsdr_demod *h, int *ninputs, int *nchannels)
{
    JSDR_REQUIRE(h && ninputs && nchannels, "jsdr_demod_channel_info: null argument");
    *ninputs = h->chan ? h->nin : h->nstreams;
    *nchannels = h->chan ? h->nch : 1;
    return JSDR_OK;
}

#define DEMOD_CHANNEL_OK(fn)                                                                                                   \
    JSDR_REQUIRE(h, fn ": null handle");                                                                                       \
    JSDR_REQUIRE(channel >= 0 && channel < (h->chan ? h->nch : 1), fn ": channel %d outside 0..%d", channel,                 \
                 (h->chan ? h->nch : 1) - 1)

int jsdr_demod_configure_channel(jsdr_demod *h, int channel, int mode, int dofir, int dodwn, int doagc)
{
    DEMOD_CHANNEL_OK("jsdr_demod_configure_channel");
    JSDR_REQUIRE(mode >= MODE_OFF && mode <= MODE_WFM, "jsdr_demod_configure_channel: mode %d outside 0..4 (demod.java:39-43)", mode);
    if (!h->chan) return jsdr_demod_configure(h, mode, dofir, dodwn, doagc);
    jsdr_demod::Chan &c = h->ch[channel];
    c.mode = mode;
    c.dofir = dofir != 0;
    c.dodwn = dodwn != 0;
    c.doagc = doagc != 0;
    return JSDR_OK;
}

// weights() for one channel: its ring cleared on every input after the handle's pending calls (the next call waits for
// that, nothing else does); the other channels carry on
int jsdr_demod_channel_weights(jsdr_demod *h, int channel, int flo, int fhi, float w_out[21], float *phi_out)
{
    DEMOD_CHANNEL_OK("jsdr_demod_channel_weights");
    if (!h->chan) return jsdr_demod_weights(h, flo, fhi, w_out, phi_out);
    jsdr_demod::Chan c = h->ch[channel];
    c.flo = flo;
    c.fhi = fhi;
    if (demod_weights_of(h->rate, flo, fhi, c.w, &c.phi)) c.car = 0.0f;
    if (h->done_any) JSDR_HIP_TRY(hipStreamWaitEvent(h->copy_stream, h->ev_done, 0));
    JSDR_HIP_TRY(hipMemset2DAsync(h->hist[h->cur].p + (size_t)channel * DHALO, sizeof(float2) * DHALO * (size_t)h->nch, 0,
                                  sizeof(float2) * DHALO, (size_t)h->nin, h->copy_stream));
    JSDR_HIP_TRY(hipEventRecord(h->ev_clear, h->copy_stream));
    h->clear_pending = true;
    h->ch[channel] = c;
    if (w_out) memcpy(w_out, c.w, sizeof(c.w));
    if (phi_out) *phi_out = c.phi;
    return JSDR_OK;
}

int jsdr_demod_get_channel(jsdr_demod *h, int channel, int *mode, int *dofir, int *dodwn, int *doagc, int *flo, int *fhi)
{
    DEMOD_CHANNEL_OK("jsdr_demod_get_channel");
    JSDR_REQUIRE(mode && dofir && dodwn && doagc && flo && fhi, "jsdr_demod_get_channel: null argument");
    if (!h->chan) {
        *mode = h->mode, *dofir = h->dofir, *dodwn = h->dodwn, *doagc = h->doagc, *flo = h->flo, *fhi = h->fhi;
        return JSDR_OK;
    }
    const jsdr_demod::Chan &c = h->ch[channel];
    *mode = c.mode, *dofir = c.dofir, *dodwn = c.dodwn, *doagc = c.doagc, *flo = c.flo, *fhi = c.fhi;
    return JSDR_OK;
}

int jsdr_demod_channel_state(jsdr_demod *h, int channel, float *car_out, float *phi_out)
{
    DEMOD_CHANNEL_OK("jsdr_demod_channel_state");
    JSDR_REQUIRE(car_out && phi_out, "jsdr_demod_channel_state: null argument");
    *car_out = h->chan ? h->ch[channel].car : h->car;
    *phi_out = h->chan ? h->ch[channel].phi : h->phi;
    return JSDR_OK;
}

}  // extern "C"
