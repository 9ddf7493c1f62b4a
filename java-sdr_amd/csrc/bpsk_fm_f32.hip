// bpsk_fm_f32.hip -- tune mode, float input: k_fm_f32, the front end and the matched filter in ONE kernel for the frames of
// IAudioHandler.receive(float[]) taken as they are (x = (double)f: no DC correction, no scaling), and k_fm_prep_f32, its
// streams' edge images and the next call's input history.  jsdr_bpsk_batch_f32's hot path (bpsk_call.hip).
//
// k_fm_f32 is k_fm (bpsk_fm.hip) with a float window: the same tile (FM_NB blocks of 65 outputs + 64 of halo in LDS), the
// same jobs of R outputs a lane, the same walk newest -> oldest and the same matched half, so every floating-point operation
// and its order are those of k_front<F32IN> + k_matched and (fi,fq) stay bit-identical to the reference.  What differs:
//   window     a lane's NS samples are NS float2 = (NS + 1) / 2 float4 -- 29 at /10 where the int16 kernel holds 15 int4 --
//              which do not fit beside the accumulators at four waves a SIMD.  The float4s are consumed newest first, so the
//              window is requested in PARTS of FM32_PQ float4: two parts are in flight at the start, and the part after them
//              is requested into a part's registers as soon as its arithmetic is done -- under the next part's arithmetic.
//              The returns are in order, so waiting for a part never waits for the one requested behind it.
//   conversion one v_cvt_f64_f32 per component; no packed-FP32 step, no DC path
//   edges      the edge images are float2 (k_fm_prep_f32), the 26-sample history is the float form (bits of the pair)
// No FAST form: the fast variant's certification re-reads int16 input, its handles refuse float batches.
//
// Compiled with -ffp-contract=off.  Reads dm_taps of its copy of the tables (matched_block, the short-call matched half).
#include "bpsk_units.h"
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

namespace jsdr {
namespace fm32 { __constant__ BpskConst c_bpsk; }  // this unit's copy of the tables, under this unit's name (bpsk_units.h)
using fm32::c_bpsk;
}  // namespace jsdr
#include "bpsk_matched.h"

namespace jsdr {

#ifndef JSDR_FM32_PQ
#define JSDR_FM32_PQ 6
#endif
enum { FM32_PQ = JSDR_FM32_PQ };  // float4 (two samples) per window part; two parts are held in registers

// The stream's edge images (E[0 .. 2*FM_EDGE) = samples -FM_EDGE .. FM_EDGE-1, E[2*FM_EDGE .. 4*FM_EDGE) = samples L-FM_EDGE ..
// L+FM_EDGE-1 as float pairs: the previous call's 26 samples before sample 0, zero before them and beyond the last sample)
// and k_hist_in's float part (the call's last 26 samples, bit for bit) in ONE launch: both only read the call's input and the
// previous call's history and write disjoint buffers.
__global__ void k_fm_prep_f32(EdgeF32Args e, HistArgs hi)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int nedge = e.nstreams * 4 * FM_EDGE;
    if (t < nedge) {
        const int s = t / (4 * FM_EDGE), i = t % (4 * FM_EDGE);
        const int n = i < 2 * FM_EDGE ? i - FM_EDGE : e.nsamples - FM_EDGE + (i - 2 * FM_EDGE);
        float2 w = make_float2(0.0f, 0.0f);
        if (n >= 0 && n < e.nsamples) {
            w = e.rawf[(long long)s * e.stride_pairs + n];
        } else if (n < 0 && n >= -26) {
            const int2 h = e.hist[(long long)s * 32 + 26 + n];
            w = make_float2(__int_as_float(h.x), __int_as_float(h.y));
        }
        e.edges[(long long)s * (4 * FM_EDGE) + i] = w;
        return;
    }
    const int u = t - nedge;
    const int s = u >> 5, i = u & 31;
    if (s >= hi.nstreams || i >= 26) return;
    const long long n = hi.nsamples - 26 + i;
    int2 v;
    if (n < 0) {
        v = hi.hist_old[(long long)s * 32 + (26 + n)];
    } else {
        const float2 f = hi.rawf[(long long)s * hi.stride_pairs + n];
        v = make_int2(__float_as_int(f.x), __float_as_int(f.y));
    }
    hi.hist_new[(long long)s * 32 + i] = v;
}

// SMALL: the instantiation for short calls (at most FM_THREADS outputs), the matched half as one output per thread (see k_fm)
template <int D, int R, bool MIX, bool SMALL = false>
__global__ __launch_bounds__(FM_THREADS, 2) void k_fm_f32(FmF32Args fa)
{
    const FmArgs &a = fa.a;
    constexpr int RD = D * R, NS = RD - D + 27, NQ = (NS + 1) / 2;
    constexpr int PQ = FM32_PQ, NP = (NQ + PQ - 1) / PQ;
    constexpr int JOBS = (FM_NT + R - 1) / R, ROUNDS = (JOBS + FM_THREADS - 1) / FM_THREADS;
    static_assert(2 * NQ <= FM_EDGE, "a window must fit an edge image's half");
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *X = reinterpret_cast<double2 *>(smem);                    // [FM_NT]: X[t] = sample G - 64 + t
    double *sc = reinterpret_cast<double *>(smem + FM_NT * sizeof(double2));  // [512]
    for (int i = threadIdx.x; i < 512; i += FM_THREADS) sc[i] = a.sincos[i];
    const long long nwork = (long long)a.ntiles * a.nstreams;
    // the ticket form of a launch held to a CU share, as k_fm's: item blockIdx.x first, then gridDim.x + ticket; thread 0 takes the
    // ticket behind the front half and hands it round through LDS at the tile's last barrier
    const bool tickets = a.tickets != nullptr;
    int *tkL = reinterpret_cast<int *>(sc + 512);  // [1]
#pragma unroll 1
    for (long long work = blockIdx.x; work < nwork; work = tickets ? (long long)gridDim.x + (unsigned)__builtin_amdgcn_readfirstlane(tkL[0]) : work + gridDim.x) {
    const int s = (int)(work / a.ntiles);
    const long long G = a.tile0 + (long long)(65 * FM_NB) * (work % a.ntiles);
    const int jrel0 = (int)(G - 64 - a.g_first);  // call-relative output index of X[0] (negative in the first tile)
    const float2 *raw = fa.rawf + (long long)s * a.stride_pairs;
    const float2 *edges = fa.edges + (long long)s * (4 * FM_EDGE);
    const double2 *dmh_old = a.dmh_old + (long long)s * 64;
    const int Lm1 = a.nsamples - 1, nds = a.nds, P = a.tper;
    const double HOWARD = 0.9 * 32768.0;  // :469
    // tile-uniform base into the unwrapped tuner table (k_fm): window sample m of ANY job of this tile uses entry e0 + m
    int e0 = 0;
    if constexpr (MIX) {
        const long long v = (long long)a.first_out + (long long)D * jrel0;
        e0 = (int)(((v % P) + P) % P);
    }
    typedef const __attribute__((address_space(4))) double *const_tab_t;  // (scalar loads: see k_fm)
    const_tab_t tb = (const_tab_t)(a.tcs + e0);  // tb[2m] = cos, tb[2m+1] = sin
    __syncthreads();  // sin/cos table
    // ================================================================================ front half
#pragma unroll 1
    for (int round = 0; round < ROUNDS; round++) {
        const int job = threadIdx.x + FM_THREADS * round;
        const int t0 = R * job;
        if (t0 >= FM_NT) break;
        const int j0 = jrel0 + t0;                   // first output of the job, call relative
        const int n0 = a.first_out + D * j0 - 26;    // its window's first sample
        // `none`, `regular` and the edge images: as k_fm.  A window is read as 2 NQ samples (one more than NS when NS is odd)
        const bool none = j0 + R <= 0 || j0 >= nds || nds <= 0;
        const bool regular = j0 >= 0 && j0 + R <= nds;
        if (!none) {
            const float2 *wp = raw + n0;
            if (n0 < 0) wp = edges + (n0 + FM_EDGE);
            else if (n0 + 2 * NQ - 1 > Lm1) wp = edges + 2 * FM_EDGE + (n0 - (a.nsamples - FM_EDGE));
            unsigned kv4[(R + 3) / 4];  // R byte indices, four to a register: requested with the window's first parts
#pragma unroll
            for (int k = 0; k < (R + 3) / 4; k++) kv4[k] = 0;
            if (regular) {
#pragma unroll
                for (int r = 0; r < R; r++) kv4[r / 4] |= (unsigned)a.kvco[j0 + r] << (8 * (r % 4));
            } else {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int j = j0 + r;
                    kv4[r / 4] |= (unsigned)a.kvco[j < 0 ? 0 : (j >= nds ? nds - 1 : j)] << (8 * (r % 4));
                }
            }
            // part p (0 = newest) holds float4 q = NQ-1 - PQ p - k, k = 0 .. PQ-1, in W[p & 1][k]; float4 q = samples 2q, 2q+1
            float4 W[2][PQ];
#pragma unroll
            for (int p = 0; p < 2 && p < NP; p++) {
#pragma unroll
                for (int k = 0; k < PQ; k++) {
                    const int q = NQ - 1 - PQ * p - k;
                    if (q >= 0) W[p][k] = *reinterpret_cast<const float4 *>(wp + 2 * q);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            double ai[R], aq[R];
            double vc[R], vs[R];  // the outputs' VCO (cos, sin): LDS reads issued under the last float4's arithmetic
#pragma unroll
            for (int r = 0; r < R; r++) {
                ai[r] = 0.0;
                aq[r] = 0.0;
            }
#pragma unroll
            for (int p = 0; p < NP; p++) {
#pragma unroll
                for (int k = 0; k < PQ; k++) {
                    const int q = NQ - 1 - PQ * p - k;
                    if (q >= 0) {
                        const float4 w4 = W[p & 1][k];
                        if (q == 0) {
#pragma unroll
                            for (int r = 0; r < R; r++) {
                                const int kv = (kv4[r / 4] >> (8 * (r % 4))) & 0xff;
                                vc[r] = sc[kv];
                                vs[r] = sc[256 + kv];
                            }
                        }
#pragma unroll
                        for (int t = 1; t >= 0; t--) {
                            const int m = 2 * q + t;
                            if (m < NS) {
                                double di = (double)(t ? w4.z : w4.x);  // (double)buf[n*2]  :372
                                double dq = (double)(t ? w4.w : w4.y);
                                if constexpr (MIX) {  // :388-390 component-wise, not a complex multiply
                                    di = di * tb[2 * m];
                                    dq = dq * tb[2 * m + 1];
                                }
#pragma unroll
                                for (int r = 0; r < R; r++) {
                                    if (m >= D * r && m <= D * r + 26) {  // age D*r+26-m in the window of output r
                                        const double tp = ds_tap(D * r + 26 - m);
                                        ai[r] += di * tp;
                                        aq[r] += dq * tp;
                                    }
                                }
                            }
                        }
                        if ((k & 1) || q == 0) {  // every four samples, as k_fm's quads
#pragma unroll
                            for (int r = 0; r < R; r++) asm volatile("" : "+v"(ai[r]), "+v"(aq[r])::"memory");  // sums are due here
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
                if (p + 2 < NP) {  // the part's registers are free: the part after the next goes out under the next one's arithmetic
#pragma unroll
                    for (int k = 0; k < PQ; k++) {
                        const int q = NQ - 1 - PQ * (p + 2) - k;
                        if (q >= 0) W[p & 1][k] = *reinterpret_cast<const float4 *>(wp + 2 * q);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (regular) {
#pragma unroll
                for (int r = 0; r < R; r++) {  // x HOWARD_FUDGE_FACTOR (:486), VCO mix (:515-516)
                    const double oi = ai[r] * HOWARD, oq = aq[r] * HOWARD;
                    if (FM_NT % R == 0 || t0 + r < FM_NT) X[t0 + r] = make_double2(oi * vc[r], oq * vs[r]);
                }
            } else {  // a job that straddles output 0 or the call's last output: one or two per stream and call
                double oi[R], oq[R];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    oi[r] = ai[r] * HOWARD * vc[r];
                    oq[r] = aq[r] * HOWARD * vs[r];
                }
#pragma unroll 1
                for (int r = 0; r < R; r++) {
                    const int t = t0 + r, j = j0 + r;
                    double2 val = make_double2(0.0, 0.0);
                    if (j >= 0 && j < nds) {
                        // (run-time r: a select chain, not an indexed register file)
                        val.x = r == 0 ? oi[0] : r == 1 ? oi[1] : r == 2 ? oi[2] : r == 3 ? oi[3] : oi[R - 1];
                        val.y = r == 0 ? oq[0] : r == 1 ? oq[1] : r == 2 ? oq[2] : r == 3 ? oq[3] : oq[R - 1];
                    } else if (j >= -64 && j < 0) {
                        val = dmh_old[64 + j];
                    }
                    if (t < FM_NT) X[t] = val;
                }
            }
        } else {
#pragma unroll 1
            for (int r = 0; r < R; r++) {
                const int t = t0 + r, j = j0 + r;
                const double2 val = (j >= -64 && j < 0) ? dmh_old[64 + j] : make_double2(0.0, 0.0);
                if (t < FM_NT) X[t] = val;
            }
        }
    }
    __syncthreads();
    unsigned tk = 0;
    if (tickets && threadIdx.x == 0) tk = atomicAdd(a.tickets, 1u);
    // ---- the call's last 64 VCO-mixed samples are the next call's halo; every sample is owned by one tile
    if (jrel0 + FM_NT > nds - 64) {  // uniform
        double2 *dmh_new = a.dmh_new + (long long)s * 64;
        for (int t = 64 + threadIdx.x; t < FM_NT; t += FM_THREADS) {
            const int j = jrel0 + t;
            if (j >= nds - 64 && j < nds && j >= 0) dmh_new[j - (nds - 64)] = X[t];
        }
        if (work % a.ntiles == 0 && nds < 64 && (int)threadIdx.x < 64 - nds) dmh_new[threadIdx.x] = dmh_old[threadIdx.x + nds];
    }
    // ================================================================================ matched filter (as k_fm's)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int blk = lane < FM_NB ? lane : FM_NB - 1;  // lanes 62, 63 shadow block 61 and store nothing
    const double2 *xl = X + 64 + 65 * blk;            // &X[s0]
    double2 *y = a.y + (long long)s * a.y_stride;
    if constexpr (SMALL) {
        // one output per thread in the reference's ring-slot order (:519-523): (s0, s0-1, .., g-64) then (g, .., s0+1)
        const int rel = (int)threadIdx.x, t = rel - jrel0;
        if (rel < nds && t >= 64 && t < FM_NT) {
            const long long g = a.g_first + rel;
            const int u = (int)(((g - 64) % 65 + 65) % 65);
            const double2 *xg = X + t;  // &X[g]
            const double *f = c_bpsk.dm_taps;
            double yi = 0.0, yq = 0.0;
            for (int i = 0; i <= 64 - u; i++) {  // s0, s0-1, .., g-64: ages u .. 64
                const double2 x = xg[-(u + i)];
                const double tp = f[u + i];
                yi += x.x * tp;
                yq += x.y * tp;
            }
            for (int m = 0; m < u; m++) {        // g, g-1, .., s0+1: ages 0 .. u-1
                const double2 x = xg[-m];
                const double tp = f[m];
                yi += x.x * tp;
                yq += x.y * tp;
            }
            y[rel] = make_double2(yi, yq);
        }
    } else {
        // the tile's outputs leave through the image, dead once every wave has walked its blocks: coalesced 16-byte stores
        double ai[9], aq[9];
        int u0 = 0, nout = 9;
        if (wave == 0) {
            matched_block<9, false>(xl, 0, ai, aq);
        } else {
            u0 = 9 + 8 * (wave - 1);
            nout = 8;
            double bi[8], bq[8];
            matched_block<8, false>(xl, u0, bi, bq);
#pragma unroll
            for (int r = 0; r < 8; r++) {
                ai[r] = bi[r];
                aq[r] = bq[r];
            }
        }
        __syncthreads();  // every wave has finished reading the image
        if (lane < FM_NB) {
#pragma unroll
            for (int r = 0; r < 9; r++)
                if (r < nout) X[65 * blk + u0 + r] = make_double2(ai[r], aq[r]);
        }
        __syncthreads();
        const int relb = jrel0 + 64;  // call-relative index of the tile's first output
        for (int o = (int)threadIdx.x; o < 65 * FM_NB; o += FM_THREADS) {
            const int rel = relb + o;
            if (rel >= 0 && rel < nds) y[rel] = X[o];
        }
    }
    {
        int zlate = 0;  // (pinned here, behind the matched half: see k_fm)
        asm volatile("" : "+v"(zlate));
        if (tickets && threadIdx.x == 0) tkL[0] = (int)tk + zlate;
    }
    __syncthreads();  // the next work item reuses the image, and takes its number from tkL
    }
}

// =============================================================================================== launchers
int bpsk_fm_f32_upload_constants(const BpskConst &bc)
{
    JSDR_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_bpsk), &bc, sizeof(bc)));
    return JSDR_OK;
}

int launch_fm_prep_f32(const EdgeF32Args &ea, const HistArgs &ha, hipStream_t st)
{
    hipLaunchKernelGGL(k_fm_prep_f32, dim3((unsigned)(((long long)ea.nstreams * (4 * FM_EDGE + 32) + 255) / 256)), dim3(256), 0, st, ea, ha);
    return launched();
}

template <int D, int R>
static int launch_fm_f32_t(const FmF32Args &a_in, bool mix, int nstreams, hipStream_t st, long long *items, long long *grid_out)
{
    const size_t lds = (size_t)FM_NT * sizeof(double2) + 512 * sizeof(double) + sizeof(double);  // image, sin / cos table, ticket
    const long long span = 65LL * FM_NB;
    const long long ntiles = (a_in.a.g_first + a_in.a.nds - a_in.a.tile0 + span - 1) / span;
    FmF32Args a = a_in;
    a.a.ntiles = (int)ntiles;
    a.a.nstreams = nstreams;
    long long gx = ntiles * nstreams;
    if (a.a.grid_limit > 0 && gx > a.a.grid_limit) gx = a.a.grid_limit;
    *items = ntiles * nstreams;
    *grid_out = gx;
    // held to a share, the workgroups take their tiles by ticket; a launch with a workgroup per tile has nothing to hand out
    if (!(a.a.grid_limit > 0 && gx < ntiles * nstreams && ntiles * nstreams + gx < 0x7fffffffLL)) a.a.tickets = nullptr;
    if (a.a.tickets) JSDR_HIP_TRY(hipMemsetAsync(a.a.tickets, 0, sizeof(unsigned), st));
    const dim3 grid((unsigned)gx), block(FM_THREADS);
#define JSDR_FM32_LAUNCH(MIX, SMALL)                                              \
    do {                                                                          \
        JSDR_LDS_ATTR((k_fm_f32<D, R, MIX, SMALL>), lds);                         \
        hipLaunchKernelGGL((k_fm_f32<D, R, MIX, SMALL>), grid, block, lds, st, a); \
    } while (0)
    if (a.a.nds <= FM_THREADS && ntiles == 1) {  // a short call: the one-output-per-thread matched half
        if (mix) JSDR_FM32_LAUNCH(true, true); else JSDR_FM32_LAUNCH(false, true);
    } else {
        if (mix) JSDR_FM32_LAUNCH(true, false); else JSDR_FM32_LAUNCH(false, false);
    }
#undef JSDR_FM32_LAUNCH
    return launched();
}

int launch_fm_f32(const FmF32Args &a, int decim, bool mix, int nstreams, hipStream_t st, long long *items, long long *grid)
{
    switch (decim) {
        case 4: return launch_fm_f32_t<4, 5>(a, mix, nstreams, st, items, grid);
        case 5: return launch_fm_f32_t<5, 4>(a, mix, nstreams, st, items, grid);
        case 10: return launch_fm_f32_t<10, 4>(a, mix, nstreams, st, items, grid);
        case 20: return launch_fm_f32_t<20, 4>(a, mix, nstreams, st, items, grid);
    }
    set_error("bpsk: unsupported decimation %d", decim);
    return JSDR_ERR;
}

}  // namespace jsdr
