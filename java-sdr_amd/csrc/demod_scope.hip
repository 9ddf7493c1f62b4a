// demod_scope.hip -- what demod.paintComponent (demod.java:509-558) draws from a frame, for the frames of a batch call: the
// magenta audio trace (getAbsMax over sam[], :519-531) and the green spectrum of the pre-detector IQ, the dbg ring (:534-555).
// Compiled with -ffp-contract=off like demod.hip: every product and sum is the one demod.hip's kernels (and the reference)
// compute, in their order.
//
// The passes run AFTER the batch call's own launches (demod_run, untouched), on rows of a chunk of frames:
//   k_demod_scope_front  one workgroup a tile, k_demod_front's geometry: demod_tile again, from the caller's input, the
//                        history and FM state of BEFORE the call and the call's carrier table, keeping the mixed IQ (dbg[],
//                        :436-437); the final float of a sample is k_demod_out's expression over the frame's stats row
//   k_demod_trace        one lane a pixel column: getAbsMax (:569-578) as written -- sam[2i] against the Qs of samples i, i+1, ..
//   k_demod_spec         one lane a pixel column: getMax (:560-567) over the PSD rows jsdr_fft_batch_f32 wrote for the dbg rows
//   k_demod_scope_layout the column schedules of (n, width), one lane a column
#include "common.h"
#include "demod.h"
#include "demod_dev.h"

namespace jsdr {

struct DemodScopeRows {
    const float *stats;  // [S * nfr][2] (max, avg) of the call
    long long row0;      // first row of the pass
    float2 *dbg;         // [nrows][n]
    float *fin;          // [nrows][n], or null
};

template <bool F32IN>
__global__ __launch_bounds__(256) void k_demod_scope_front(DemodArgs a, DemodScopeRows sc)
{
    constexpr int PER = DPER;
    __shared__ float2 xs[DXS];
    __shared__ float2 last[256];
    const int tid = threadIdx.x;
    const int tiles_per_frame = (a.n + DTILE - 1) / DTILE;
    const int rloc = blockIdx.x / tiles_per_frame;
    const int j = blockIdx.x - rloc * tiles_per_frame;
    const long long row = sc.row0 + rloc;
    const int s = (int)(row / a.nfr);
    const int f = (int)(row - (long long)s * a.nfr);
    const int len = (a.n - j * DTILE) < DTILE ? (a.n - j * DTILE) : DTILE;
    const int t0 = tid * PER;
    float dv[PER];
    v2f m[PER];
    unsigned mbits = 0;
    demod_tile<F32IN, false, true>(a, s, f, j, xs, last, dv, mbits, m);
    const size_t at = (size_t)rloc * (size_t)a.n + (size_t)j * DTILE + t0;  // within the pass's rows
    float2 *dbg = sc.dbg + at;
    if (t0 + PER <= len && (reinterpret_cast<uintptr_t>(dbg) & 15) == 0) {
#pragma unroll
        for (int u = 0; u < PER; u += 2) reinterpret_cast<float4 *>(dbg)[u / 2] = make_float4(m[u].x, m[u].y, m[u + 1].x, m[u + 1].y);
    } else {
#pragma unroll
        for (int u = 0; u < PER; u++)
            if (t0 + u < len) dbg[u] = make_float2(m[u].x, m[u].y);
    }
    if (!sc.fin) return;
    // :465-472 as k_demod_out / k_demod_fused form it: max already less avg in AM
    const float mx = sc.stats[2 * row];
    const float avg = sc.stats[2 * row + 1];
    const float scale = a.c.doagc ? 1.0f / mx : 1.0f;
    float o[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        float x = dv[u];
        if (a.c.mode == MODE_AM) x = x - avg;
        o[u] = x * scale;
    }
    float *fin = sc.fin + at;
    if (t0 + PER <= len && (reinterpret_cast<uintptr_t>(fin) & 15) == 0) {
        reinterpret_cast<float4 *>(fin)[0] = make_float4(o[0], o[1], o[2], o[3]);
        reinterpret_cast<float4 *>(fin)[1] = make_float4(o[4], o[5], o[6], o[7]);
    } else {
#pragma unroll
        for (int u = 0; u < PER; u++)
            if (t0 + u < len) fin[u] = o[u];
    }
}

// :519-531.  Entry 0 is the polyline's start, H/4; entry x + 1 is y of column x.  getAbsMax(sam, 2i, (int)scale, 2) walks
// idx = 2i + 1, 2i + 3, .. < 2i + (int)scale: the Qs of samples i, i + 1, .. -- count / 2 of them -- against sam[2i], strict >,
// a NaN never wins and, once r is NaN, nothing does
__global__ __launch_bounds__(256) void k_demod_trace(const float *__restrict__ fin, const float2 *__restrict__ dbg, int n,
                                                     int mode_off, int nrows, int width, int quarter, float h,
                                                     const int *__restrict__ tab, int *__restrict__ out)
{
    const int bpr = (width + 255) / 256;
    const int rloc = blockIdx.x / bpr;
    const int x = (blockIdx.x - rloc * bpr) * 256 + threadIdx.x;
    if (x >= width || rloc >= nrows) return;
    int y = quarter;
    if (x > 0) {
        const int i = tab[x - 1], cnt = tab[width + x - 1];
        const size_t base = (size_t)rloc * (size_t)n;
        float r = fin[base + i];
        float c = fabsf(r);
        const int nq = cnt / 2 < n - i ? cnt / 2 : n - i;  // (the layout check has refused a schedule that would leave the row)
        for (int k = 0; k < nq; k++) {
            const float q = mode_off ? 0.0f : dbg[base + i + k].y;
            if (fabsf(q) > c) r = q;
            c = fabsf(r);
        }
        y = (int)((unsigned)quarter - (unsigned)demod_f2i(r * h));
    }
    out[(size_t)rloc * (size_t)width + x] = y;
}

// :544-555.  Entry 0 is H/2 + (int)(psd[0] * h); entry m is H/2 + (int)(getMax(psd, i, (int)pi) * h)
__global__ __launch_bounds__(256) void k_demod_spec(const float *__restrict__ psd, int n, int nrows, int width, int half, float h,
                                                    const int *__restrict__ tab, int *__restrict__ out)
{
    const int bpr = (width + 255) / 256;
    const int rloc = blockIdx.x / bpr;
    const int x = (blockIdx.x - rloc * bpr) * 256 + threadIdx.x;
    if (x >= width || rloc >= nrows) return;
    const float *row = psd + (size_t)rloc * (size_t)(n + 2);
    const int i = tab[2 * width + x], cnt = tab[3 * width + x];  // (0, 0) at entry 0
    float r = row[i];
    const int end = i + cnt < n ? i + cnt : n;  // (as above)
    for (int k = i + 1; k < end; k++) {
        const float v = row[k];
        if (v > r) r = v;
    }
    out[(size_t)rloc * (size_t)width + x] = (int)((unsigned)half + (unsigned)demod_f2i(r * h));
}

__global__ __launch_bounds__(256) void k_demod_scope_layout(int width, float scale, float pi, int *__restrict__ tab)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= width) return;
    const bool col = x < width - 1;
    tab[x] = col ? dscope_trace_first(x, scale) : 0;
    tab[width + x] = col ? (int)scale : 0;
    tab[2 * width + x] = x ? dscope_spec_first(x, pi) : 0;
    tab[3 * width + x] = x ? (int)pi : 0;
}

int launch_demod_scope_layout(int n, int width, int *tab, hipStream_t st)
{
    hipLaunchKernelGGL(k_demod_scope_layout, dim3((unsigned)((width + 255) / 256)), dim3(256), 0, st, width, dscope_scale(n, width),
                       dscope_pi(n, width), tab);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_demod_scope_front(const DemodArgs &a, bool f32in, const float *stats, long long row0, int nrows, float2 *dbg_rows,
                             float *fin_rows, hipStream_t st)
{
    const long long tiles = (a.n + DTILE - 1) / DTILE;
    JSDR_REQUIRE(tiles * nrows < (1LL << 31), "demod scope: %d frames of %lld tiles in one pass", nrows, tiles);
    DemodScopeRows sc;
    sc.stats = stats;
    sc.row0 = row0;
    sc.dbg = dbg_rows;
    sc.fin = fin_rows;
    const dim3 grid((unsigned)(tiles * nrows));
    if (f32in)
        hipLaunchKernelGGL(k_demod_scope_front<true>, grid, dim3(256), 0, st, a, sc);
    else
        hipLaunchKernelGGL(k_demod_scope_front<false>, grid, dim3(256), 0, st, a, sc);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_demod_trace(const float *fin_rows, const float2 *dbg_rows, int n, bool mode_off, int nrows, int width, int quarter,
                       const int *tab, int32_t *trace_rows, hipStream_t st)
{
    const long long blocks = (long long)((width + 255) / 256) * nrows;
    JSDR_REQUIRE(blocks < (1LL << 31), "demod scope: %d rows of width %d in one pass", nrows, width);
    hipLaunchKernelGGL(k_demod_trace, dim3((unsigned)blocks), dim3(256), 0, st, fin_rows, dbg_rows, n, mode_off ? 1 : 0, nrows, width,
                       quarter, (float)quarter, tab, trace_rows);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_demod_spec(const float *psd_rows, int n, int nrows, int width, int half, const int *tab, int32_t *spec_rows,
                      hipStream_t st)
{
    const long long blocks = (long long)((width + 255) / 256) * nrows;
    JSDR_REQUIRE(blocks < (1LL << 31), "demod scope: %d rows of width %d in one pass", nrows, width);
    hipLaunchKernelGGL(k_demod_spec, dim3((unsigned)blocks), dim3(256), 0, st, psd_rows, n, nrows, width, half,
                       (float)half / -100.0f, tab, spec_rows);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
