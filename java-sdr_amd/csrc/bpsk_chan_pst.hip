// bpsk_chan_pst.hip -- the front end of a tuned channel handle (jsdr_bpsk_create_tuned_channels): ninputs x nchannels lock-step
// demodulators in the tune mode, channel c of input i is row i * nchannels + c, every row with its OWN tuning, walked on the
// device (k_tuner_walk, bpsk_pst.hip), and every input read ONCE.  Exact-order FP64 (-ffp-contract=off).
//
// k_chan_front_pst : one workgroup = up to 256 consecutive decimated outputs of ONE input (k_chan_front's tile).  The raw samples
//                    their 27-tap windows cover are read once, DC-corrected and converted as JavaAudio does (or taken as the float
//                    input) and parked in LDS as float2 -- k_chan_front's image.  Then, channel after channel of the input:
//                    phase 1 (bpsk_pst_phase1.h, k_front_pst's) expands the tile's 9-bit table indices from the ROW's checkpoints
//                    into the index row in LDS; phase 2: every lane owns one output and walks its window newest -> oldest:
//                    (double)f x sc9[k] (:388-390 / :395), x taps[age], summed in that order (:479-483), x HOWARD (:486), the
//                    shared VCO factor (:515-516), into the row's dm -- k_front_pst's products and sums, one for one (it forms
//                    a sample's mixed double once and keeps it; here it is formed in every window the sample falls into, the
//                    same double each time).  Groups of channels sharing each LDS read of a sample, as k_chan_front's CG, were
//                    measured and are slower here at every tile size: their index rows cost the tile its outputs.
//
// k_hist_in keeps the 26-sample history per INPUT; k_matched, k_dm_history, the tail, sync and FEC run on the rows unchanged.
// The planned and the ramp form (k_chan_front_pst_plan, k_chan_front_pst_ramp) are the same body with PLAN / RAMP set, as in bpsk_pst.hip.
#include "common.h"
#include "bpsk_tuner.h"
#include "bpsk_pst.h"

namespace jsdr {

// the LDS a workgroup may take: a quarter of a CU's 160 KB, four workgroups a CU (DESIGN.md 7 has the tile shapes measured;
// tools/build_define.sh -DJSDR_CPST_LDS= builds another for A/B timing)
#ifndef JSDR_CPST_LDS
#define JSDR_CPST_LDS 40960
#endif
enum { CPST_THREADS = 256, CPST_LDS = JSDR_CPST_LDS };

// the tile's samples, read once: DC-corrected and converted (:372-373), or the float input as it is
template <bool F32IN>
__device__ __forceinline__ void chan_pst_park(const PstChanFrontArgs &a, int in, long long n_lo, int cnt, float2 *x)
{
    const int *raw = a.raw + (long long)in * a.stride_pairs;
    const int2 *hist = a.hist + (long long)in * 32;
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
        const long long n = n_lo + e;  // < L: the newest sample of the last output is at most L - 1
        if constexpr (F32IN) {
            if (n >= 0) {
                x[e] = reinterpret_cast<const float2 *>(a.raw)[(long long)in * a.stride_pairs + n];
            } else {
                const int2 h = hist[26 + n];  // the float pair's bits (k_hist_in)
                x[e] = make_float2(__int_as_float(h.x), __int_as_float(h.y));
            }
        } else {
            int w;
            if (n >= 0) {
                w = raw[n];
                const int si = java_short_add((int)(short)(w & 0xffff), a.ic);
                const int sq = java_short_add(w >> 16, a.qc);
                w = (si & 0xffff) | (sq << 16);
            } else {
                w = hist[26 + n].x;  // kept DC-corrected by k_hist_in
            }
            x[e] = make_float2(i16_to_float_java((int)(short)(w & 0xffff)), i16_to_float_java(w >> 16));
        }
    }
}

// phase 2: output j of row s, whose table indices are k9[cap]
__device__ __forceinline__ void chan_pst_taps(const PstChanFrontArgs &a, const double *sc, const double *taps, const float2 *x,
                                              const unsigned short *k9, long long s, long long j, int kv)
{
    const double HOWARD = 0.9 * 32768.0;                // :469
    const int e_new = a.decim * (int)threadIdx.x + 26;  // the sample that completes output j
    const float2 *xw = x + e_new;                       // xw[-age] = the sample `age` before it
    const unsigned short *kw = k9 + e_new;
    double fi = 0.0, fq = 0.0;
#pragma unroll 3  // (three taps an iteration: unrolled whole, the window's LDS reads are hoisted together and take registers)
    for (int age = 0; age < 27; age++) {
        const float2 v = xw[-age];
        const int k = kw[-age];
        double di = (double)v.x, dq = (double)v.y;  // (double)buf[n*2]  :372
        di = di * sc[k];                             // :388-390 / :395
        dq = dq * sc[257 + k];
        const double tp = taps[age];
        fi += di * tp;
        fq += dq * tp;
    }
    const double oi = fi * HOWARD, oq = fq * HOWARD;  // :486
    a.dm[s * a.dm_stride + 64 + j] = make_double2(oi * sc[kv], oq * sc[257 + kv]);  // :515-516
}

template <bool F32IN>
__global__ __launch_bounds__(CPST_THREADS) void k_chan_front_pst(PstChanFrontArgs a)
{
    constexpr bool PLAN = false, RAMP = false;
    const PstPlanArgs p{};
    const PstRampArgs r{};
#include "bpsk_chan_pst_body.h"
}

template <bool F32IN>
__global__ __launch_bounds__(CPST_THREADS) void k_chan_front_pst_plan(PstChanFrontArgs a, PstPlanArgs p)
{
    constexpr bool PLAN = true, RAMP = false;
    const PstRampArgs r{};
#include "bpsk_chan_pst_body.h"
}

template <bool F32IN>
__global__ __launch_bounds__(CPST_THREADS) void k_chan_front_pst_ramp(PstChanFrontArgs a, PstPlanArgs p, PstRampArgs r)
{
    constexpr bool PLAN = true, RAMP = true;
#include "bpsk_chan_pst_body.h"
}

// LDS of a workgroup of nout outputs at decimation D: the tables, the phase scratch, the float2 image, the index row
static size_t chan_pst_lds(long long nout, int D)
{
    const size_t cap = (size_t)(nout - 1) * (size_t)D + 27;
    return (514 + 28) * sizeof(double) + (cap + ((cap - 1) >> 6)) * sizeof(double) + cap * (sizeof(float2) + sizeof(unsigned short));
}

int launch_chan_front_pst(const PstChanFrontArgs &a_in, int ninputs, bool f32in, const PstPlanArgs *plan, const PstRampArgs *ramp, hipStream_t st)
{
    PstChanFrontArgs a = a_in;
    // outputs per workgroup: as many as fit CPST_LDS at 8 bytes of sample, 8 1/8 of phase and 2 of index a sample -- 200 at
    // decimation 10, 100 at 20, 256 (the lanes) from decimation 7 down
    long long nout = CPST_THREADS;
    while (nout >= 1 && chan_pst_lds(nout, a.decim) > CPST_LDS) nout--;
    if (nout < 1) {
        set_error("bpsk tuned channels: decimation %d is too large for the tuned channel front end", a.decim);
        return JSDR_ERR;
    }
    a.nout = (int)nout;
    const size_t lds = chan_pst_lds(nout, a.decim);
    const long long gx = (a.nds + nout - 1) / nout;
    const dim3 grid((unsigned)gx, (unsigned)ninputs), block(CPST_THREADS);
    if (plan && ramp && f32in) {
        JSDR_LDS_ATTR((k_chan_front_pst_ramp<true>), lds);
        hipLaunchKernelGGL((k_chan_front_pst_ramp<true>), grid, block, lds, st, a, *plan, *ramp);
    } else if (plan && ramp) {
        JSDR_LDS_ATTR((k_chan_front_pst_ramp<false>), lds);
        hipLaunchKernelGGL((k_chan_front_pst_ramp<false>), grid, block, lds, st, a, *plan, *ramp);
    } else if (plan && f32in) {
        JSDR_LDS_ATTR((k_chan_front_pst_plan<true>), lds);
        hipLaunchKernelGGL((k_chan_front_pst_plan<true>), grid, block, lds, st, a, *plan);
    } else if (plan) {
        JSDR_LDS_ATTR((k_chan_front_pst_plan<false>), lds);
        hipLaunchKernelGGL((k_chan_front_pst_plan<false>), grid, block, lds, st, a, *plan);
    } else if (f32in) {
        JSDR_LDS_ATTR((k_chan_front_pst<true>), lds);
        hipLaunchKernelGGL((k_chan_front_pst<true>), grid, block, lds, st, a);
    } else {
        JSDR_LDS_ATTR((k_chan_front_pst<false>), lds);
        hipLaunchKernelGGL((k_chan_front_pst<false>), grid, block, lds, st, a);
    }
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
