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
// Kernels: k_demod_front / k_demod_fused (raw -> demodulated float per sample + per-frame max; fused: straight to int16),
// k_demod_mean (AM only), k_demod_out (-> int16 L,R), k_demod_state (history for the next call), k_demod_nco.
// Kernels and their launchers (demod.h) only: the handle that calls them is demod_handle.h's, in host units of its own
// (demod_call.hip, demod_control.hip, demod_scope_host.hip; the pure part in demod_host.hip).  The channel handles' kernels
// are in demod_chan.hip, the scope's in demod_scope.hip.
#include "common.h"
#include "demod.h"
#include "demod_dev.h"
#include <math.h>

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

// ---- the launchers (demod.h): what the handle's host units (demod_handle.h) see of the kernels above
template <bool F32IN>
static void launch_fused(const DemodArgs &a, int tiles, int nstreams, int *out, long long out_stride_pairs, float *stats,
                         hipStream_t st)
{
    const dim3 grid((unsigned)a.nfr, (unsigned)nstreams);  // (streams fastest instead, for carrier-table locality: measured, no gain)
    switch (tiles) {
        case 1: hipLaunchKernelGGL((k_demod_fused<F32IN, 1>), grid, dim3(256), 0, st, a, out, out_stride_pairs, stats); break;
        case 2: hipLaunchKernelGGL((k_demod_fused<F32IN, 2>), grid, dim3(256), 0, st, a, out, out_stride_pairs, stats); break;
        case 3: hipLaunchKernelGGL((k_demod_fused<F32IN, 3>), grid, dim3(256), 0, st, a, out, out_stride_pairs, stats); break;
        case 4: hipLaunchKernelGGL((k_demod_fused<F32IN, 4>), grid, dim3(256), 0, st, a, out, out_stride_pairs, stats); break;
        default: hipLaunchKernelGGL((k_demod_fused<F32IN, 5>), grid, dim3(256), 0, st, a, out, out_stride_pairs, stats); break;
    }
}

int launch_demod_front(const DemodArgs &a, bool f32in, bool fused, int nstreams, int *out, long long out_stride_pairs,
                       float *stats, hipStream_t st)
{
    const int tiles = (a.n + DTILE - 1) / DTILE;
    if (fused) {
        if (f32in)
            launch_fused<true>(a, tiles, nstreams, out, out_stride_pairs, stats, st);
        else
            launch_fused<false>(a, tiles, nstreams, out, out_stride_pairs, stats, st);
    } else {
        const dim3 grid((unsigned)(tiles * a.nfr), (unsigned)nstreams);
        if (f32in)
            hipLaunchKernelGGL(k_demod_front<true>, grid, dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(k_demod_front<false>, grid, dim3(256), 0, st, a);
    }
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_demod_state(const DemodArgs &a, bool f32in, float2 *hist_new, float2 *lilq_new, int nstreams, hipStream_t st)
{
    if (f32in)
        hipLaunchKernelGGL(k_demod_state<true>, dim3((unsigned)nstreams), dim3(64), 0, st, a, hist_new, lilq_new, nstreams);
    else
        hipLaunchKernelGGL(k_demod_state<false>, dim3((unsigned)nstreams), dim3(64), 0, st, a, hist_new, lilq_new, nstreams);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_demod_nco(const float *car, long long n, float2 *nco, hipStream_t st)
{
    hipLaunchKernelGGL(k_demod_nco, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, car, n, nco);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_demod_mean(const float *d, long long L, int n, int nfr, long long nframes_total, float *favg, hipStream_t st)
{
    hipLaunchKernelGGL(k_demod_mean, dim3((unsigned)((nframes_total + 63) / 64)), dim3(64), 0, st, d, L, n, nfr, nframes_total, favg);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_demod_out(const DemodArgs &a, int nstreams, const float *favg, int *out, long long out_stride_pairs, float *stats,
                     hipStream_t st)
{
    hipLaunchKernelGGL(k_demod_out, dim3((unsigned)((a.n + 1023) / 1024), (unsigned)a.nfr, (unsigned)nstreams), dim3(256), 0, st, a.d,
                       a.L, a.n, a.nfr, a.c.mode, a.c.doagc, a.fmax_bits, favg, out, out_stride_pairs, stats);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
