// phase_scope.hip -- phase.paintComponent's arithmetic (phase.java:75-116) over batches of IQ frames: jsdr_phase_scope_i16 / _f32.
// One launch over raw[stream][stride]; a frame is a workgroup's work item and is read from memory once: max|x| (:75-80) on the way
// in, then the column means (:93-99, 104-105) and the painter's four integers a column (:102, 107, 109) from the frame's LDS image.
// Compiled with -ffp-contract=off: the schedule's `pos += step`, the sums, the quotients and the products round one by one, as
// Java's do.
#include "common.h"
#include "phase_handle.h"
#include "waterfall_dev.h"

namespace jsdr {

enum { SC_I16 = 0, SC_F32 = 1 };
constexpr int SC_T = 256;             // threads a workgroup
constexpr int SC_LDS_MAX_N = 8192;    // frames up to here keep their image in LDS (8n bytes: 64 KiB, two workgroups a CU)

struct ScopeArgs {
    const void *in;         // int16 (I, Q) pairs or floats
    long long off0_step;    // what a workgroup's input offset grows by from one of its rows to the next (values), before the wrap
    long long wrap;         // ... and what a step past a stream's last frame adds: stride - fps * 2n
    long long stride, fps, rows;
    long long step_j;       // gridDim.x % fps
    int n, ic, qc, ncol;
    float half, quarter;    // (float)(size/2), (float)(getHeight()/4)
    const int2 *tab;        // [ncol] {first sample, samples}
    float *max_out;         // [rows]
    float2 *avg;            // [rows][ncol] or null
    int4 *pts;              // [rows][ncol] or null
};

// the schedule of (n, step) into the handle's table: phase_walk, one thread.  Stream-ordered behind the readers of the table it replaces.
__global__ void k_phase_table(int2 *__restrict__ tab, int n, float step)
{
    phase_walk(n, step, [&](int c, int, int first, int count) { tab[c] = make_int2(first, count); });
}

// IMG: the converted frame is kept in LDS (float[2n]) and the columns are walked there; !IMG (k_phase_scope_g): frames past the LDS
// budget read their samples again from global memory -- the frame has just been read, an L2 hit -- and convert them again.
template <int IN, bool IMG>
__global__ __launch_bounds__(SC_T) void k_phase_scope(ScopeArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    [[maybe_unused]] float *img = reinterpret_cast<float *>(smem);
    __shared__ float red[2][SC_T / 64];  // a frame's per-wave maxima; two sets, frames alternate (!IMG has no barrier at a frame's end)
    const int tid = threadIdx.x;
    const int W = IN == SC_I16 ? a.n : 2 * a.n;  // 4-byte words a frame: an int16 pair, or a float

    long long r = blockIdx.x;
    if (r >= a.rows) return;
    // (stream, frame) of the first row by one division; additions from there on
    long long j = r % a.fps;
    long long off = (r / a.fps) * a.stride + j * 2 * a.n;
    for (int it = 0; r < a.rows; r += gridDim.x, it ^= 1) {
        const unsigned *p = IN == SC_I16 ? reinterpret_cast<const unsigned *>(static_cast<const int16_t *>(a.in) + off)
                                         : reinterpret_cast<const unsigned *>(static_cast<const float *>(a.in) + off);
        float m = -1.0f;  // phase.java:75
        auto amax = [&](float x) {
            const float v = fabsf(x);
            if (m < v) m = v;  // :78 -- never admits a NaN, so the order is free
        };
        // word w of the frame as the sample it holds (int16: as jsdr_convert_i16 takes it) or the float
        [[maybe_unused]] auto pair16 = [&](unsigned v) {
            const int si = java_short_add((int)(short)(v & 0xffff), a.ic), sq = java_short_add((int)v >> 16, a.qc);
            return make_float2(i16_to_float_java(si), i16_to_float_java(sq));
        };
        auto take = [&](int w, unsigned v) {
            if constexpr (IN == SC_I16) {
                const float2 f = pair16(v);
                amax(f.x);
                amax(f.y);
                if constexpr (IMG) reinterpret_cast<float2 *>(img)[w] = f;
            } else {
                const float f = __uint_as_float(v);
                amax(f);
                if constexpr (IMG) img[w] = f;
            }
        };
        auto take4 = [&](int w, uint4 v) {
            if constexpr (IN == SC_I16) {
                take(w, v.x);
                take(w + 1, v.y);
                take(w + 2, v.z);
                take(w + 3, v.w);
            } else {
                const float f0 = __uint_as_float(v.x), f1 = __uint_as_float(v.y), f2 = __uint_as_float(v.z), f3 = __uint_as_float(v.w);
                amax(f0);
                amax(f1);
                amax(f2);
                amax(f3);
                if constexpr (IMG) {  // (w is even: a float frame starts on a pair)
                    *reinterpret_cast<float2 *>(img + w) = make_float2(f0, f1);
                    *reinterpret_cast<float2 *>(img + w + 2) = make_float2(f2, f3);
                }
            }
        };
        // ---- fetch and convert: 16-byte loads between the frame's first and last 16-byte boundary, single words outside
        int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
        if (head > W) head = W;
        const int nvec = (W - head) >> 2, t0 = head + 4 * nvec;
        const uint4 *pv = reinterpret_cast<const uint4 *>(p + head);
        int v = tid;
        for (; v + SC_T < nvec; v += 2 * SC_T) {  // two loads of a thread in flight together
            const uint4 x0 = pv[v], x1 = pv[v + SC_T];
            take4(head + 4 * v, x0);
            take4(head + 4 * (v + SC_T), x1);
        }
        if (v < nvec) take4(head + 4 * v, pv[v]);
        if (tid < head) take(tid, p[tid]);
        if (t0 + tid < W) take(t0 + tid, p[t0 + tid]);
        // ---- the frame's maximum: across the wave, then across the waves through LDS
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float x = __shfl_xor(m, o, 64);
            if (m < x) m = x;
        }
        if ((tid & 63) == 0) red[it][tid >> 6] = m;
        __syncthreads();  // (the one barrier between the frame's way in and its columns: the maxima and the image)
        m = red[it][0];
#pragma unroll
        for (int w = 1; w < SC_T / 64; w++) {
            const float x = red[it][w];
            if (m < x) m = x;
        }
        if (tid == 0) a.max_out[r] = m;
        // ---- columns: a lane a column, in sample order
        if (a.ncol > 0) {
            const float hiq = a.quarter / m, hph = a.half / m;  // :85-86
            auto sample = [&](int k) {
                if constexpr (IMG)
                    return reinterpret_cast<const float2 *>(img)[k];
                else if constexpr (IN == SC_I16)
                    return pair16(p[k]);
                else
                    return reinterpret_cast<const float2 *>(p)[k];
            };
            for (int c = tid; c < a.ncol; c += SC_T) {
                const int2 fc = a.tab[c];
                float si = 0.0f, sq = 0.0f;
                float2 e = make_float2(0.0f, 0.0f);
                for (int k = 0; k < fc.y; k++) {
                    e = sample(fc.x + k);
                    si += e.x;  // :94-95
                    sq += e.y;
                }
                const float cnt = (float)fc.y;
                const float ai = si / cnt, aq = sq / cnt;  // :104-105
                const long long o = r * a.ncol + c;
                if (a.avg) a.avg[o] = make_float2(ai, aq);
                // :107, 109 the lines' ends; :102 the dot, from the column's closing sample
                if (a.pts) a.pts[o] = make_int4(java_f2i(ai * hiq), java_f2i(aq * hiq), java_f2i(e.x * hph), java_f2i(e.y * hph));
            }
        }
        if constexpr (IMG) __syncthreads();  // the next frame overwrites the image
        off += a.off0_step;
        j += a.step_j;
        if (j >= a.fps) {
            j -= a.fps;
            off += a.wrap;
        }
    }
}

template <int IN>
static int scope_launch(bool img, int grid, size_t lds, hipStream_t s, const ScopeArgs &a)
{
    if (img) {
        JSDR_LDS_ATTR((k_phase_scope<IN, true>), lds);  // (8192 samples: 64 KiB of image beside the static words)
        hipLaunchKernelGGL((k_phase_scope<IN, true>), dim3(grid), dim3(SC_T), lds, s, a);
    } else {
        hipLaunchKernelGGL((k_phase_scope<IN, false>), dim3(grid), dim3(SC_T), 0, s, a);
    }
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

static int scope_run(const char *who, const char *in_name, const char *stride_name, jsdr_phase *h, const void *in_dev, int in_kind,
                     int nstreams, int64_t stride, int64_t fps, int ic, int qc, int bx, int half_size, int quarter_height,
                     float *max_dev, float *avg_dev, int32_t *pts_dev, hipStream_t s)
{
    JSDR_REQUIRE(h, "%s: null handle", who);
    JSDR_REQUIRE(in_dev, "%s: null %s", who, in_name);
    JSDR_REQUIRE(max_dev, "%s: null max_dev", who);
    JSDR_REQUIRE(nstreams > 0, "%s: nstreams=%d is not positive", who, nstreams);
    JSDR_REQUIRE(fps >= 0, "%s: frames_per_stream=%lld is negative", who, (long long)fps);
    JSDR_REQUIRE(fps <= 2147483647LL / nstreams, "%s: rows = nstreams * frames_per_stream = %d * %lld do not fit 31 bits", who, nstreams,
                 (long long)fps);
    JSDR_REQUIRE(bx >= 0, "%s: bx=%d is negative", who, bx);
    const long long n = h->n;
    if (nstreams > 1) {
        JSDR_REQUIRE((stride & 1) == 0, "%s: %s=%lld is odd (a stream starts on an IQ pair)", who, stride_name, (long long)stride);
        JSDR_REQUIRE(stride >= fps * 2 * n, "%s: %s=%lld is below a stream's %lld frames of %lld values", who, stride_name,
                     (long long)stride, (long long)fps, 2 * n);
    }
    const uintptr_t pair = in_kind == SC_I16 ? 4 : 8;
    JSDR_REQUIRE((reinterpret_cast<uintptr_t>(in_dev) & (pair - 1)) == 0, "%s: %s is not aligned to an IQ pair (%d bytes)", who, in_name, (int)pair);
    JSDR_REQUIRE((reinterpret_cast<uintptr_t>(max_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(avg_dev) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(pts_dev) & 15) == 0,
                 "%s: max_dev / avg_dev / pts_dev must be aligned to 4 / 8 / 16 bytes, a row entry", who);
    if (fps == 0) return JSDR_OK;
    JSDR_REQUIRE(n > 0, "%s: the handle has no frame size", who);

    if (!h->tab.p) {  // the first scope call: the one allocation
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
            (void)hipGetLastError();
            cus = 256;
        }
        // (zeroed: an entry is either empty or a column of some schedule of this n -- inside the frame whatever happens)
        if (h->tab.alloc((size_t)n) != JSDR_OK || h->tab.zero(s) != JSDR_OK) {
            h->tab.release();
            return JSDR_ERR;
        }
        h->num_cu = cus;
        h->tab_bx = -1;
    }
    if (bx != h->tab_bx) {
        const float step = phase_step((int)n, bx);
        const int ncol = phase_walk((int)n, step, [](int, int, int, int) {});
        if (ncol > 0) {
            hipLaunchKernelGGL(k_phase_table, dim3(1), dim3(1), 0, s, h->tab.p, (int)n, step);
            JSDR_LAUNCH_CHECK();
        }
        h->tab_bx = bx;
        h->tab_ncol = ncol;
    }

    const bool img = n <= SC_LDS_MAX_N;
    const size_t lds = img ? (size_t)8 * (size_t)n : 0;
    const long long rows = (long long)nstreams * fps;
    // a few resident workgroups a CU: eight (the CU's 32 waves), or as many images as its LDS holds
    long long per_cu = img ? (long long)(160 * 1024) / (long long)(lds + 64) : 8;
    per_cu = per_cu > 8 ? 8 : per_cu < 1 ? 1 : per_cu;
    long long grid = (long long)h->num_cu * per_cu;
    if (grid > rows) grid = rows;

    ScopeArgs a;
    a.in = in_dev;
    a.stride = nstreams > 1 ? (long long)stride : fps * 2 * n;
    a.fps = fps;
    a.rows = rows;
    a.step_j = grid % fps;
    a.off0_step = (grid / fps) * a.stride + a.step_j * 2 * n;
    a.wrap = a.stride - fps * 2 * n;
    a.n = (int)n;
    a.ic = ic;
    a.qc = qc;
    a.ncol = (avg_dev || pts_dev) ? h->tab_ncol : 0;
    a.half = (float)half_size;
    a.quarter = (float)quarter_height;
    a.tab = h->tab.p;
    a.max_out = max_dev;
    a.avg = reinterpret_cast<float2 *>(avg_dev);
    a.pts = reinterpret_cast<int4 *>(pts_dev);
    if ((in_kind == SC_I16 ? scope_launch<SC_I16>(img, (int)grid, lds, s, a) : scope_launch<SC_F32>(img, (int)grid, lds, s, a)) != JSDR_OK)
        return JSDR_ERR;
    h->scope_kernel = img ? "k_phase_scope" : "k_phase_scope_g";
    return JSDR_OK;
}

}  // namespace jsdr

using namespace jsdr;

extern "C" {

int jsdr_phase_layout(int n, int bx, int32_t *pix_host, int32_t *first_host, int32_t *count_host, int cap, int *ncol)
{
    JSDR_REQUIRE(ncol, "jsdr_phase_layout: null ncol");
    *ncol = 0;
    JSDR_REQUIRE(n > 0 && n <= 0x3fffffff, "jsdr_phase_layout: n=%d is outside 1 .. 2^30 - 1", n);
    JSDR_REQUIRE(bx >= 0, "jsdr_phase_layout: bx=%d is negative", bx);
    const float step = phase_step(n, bx);
    const int k = phase_walk(n, step, [](int, int, int, int) {});
    *ncol = k;
    if (!pix_host && !first_host && !count_host) return JSDR_OK;
    JSDR_REQUIRE(k <= cap, "jsdr_phase_layout: %d columns exceed the caller's cap=%d", k, cap);
    phase_walk(n, step, [&](int c, int pix, int first, int count) {
        if (pix_host) pix_host[c] = pix;
        if (first_host) first_host[c] = first;
        if (count_host) count_host[c] = count;
    });
    return JSDR_OK;
}

int jsdr_phase_scope_i16(jsdr_phase *h, const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16, int64_t frames_per_stream,
                         int ic, int qc, int bx, int half_size, int quarter_height, float *max_dev, float *avg_dev, int32_t *pts_dev,
                         void *stream)
{
    return scope_run("jsdr_phase_scope_i16", "raw_dev", "stream_stride_i16", h, raw_dev, SC_I16, nstreams, stream_stride_i16,
                     frames_per_stream, ic, qc, bx, half_size, quarter_height, max_dev, avg_dev, pts_dev, as_stream(stream));
}

int jsdr_phase_scope_f32(jsdr_phase *h, const float *iq_dev, int nstreams, int64_t stream_stride_f32, int64_t frames_per_stream, int bx,
                         int half_size, int quarter_height, float *max_dev, float *avg_dev, int32_t *pts_dev, void *stream)
{
    return scope_run("jsdr_phase_scope_f32", "iq_dev", "stream_stride_f32", h, iq_dev, SC_F32, nstreams, stream_stride_f32,
                     frames_per_stream, 0, 0, bx, half_size, quarter_height, max_dev, avg_dev, pts_dev, as_stream(stream));
}

const char *jsdr_phase_scope_kernel(jsdr_phase *h) { return h ? h->scope_kernel : ""; }

}  // extern "C"
