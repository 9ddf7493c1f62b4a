// bpsk_pst.hip -- the front end of a tuned handle (jsdr_bpsk_create_tuned): nstreams lock-step demodulators in the tune mode
// (doBufferTune, FUNcubeBPSKDemod.java:366-397), every stream with its OWN tuning.  Exact-order FP64 (-ffp-contract=off).
//
// The tuner recurrence (:384-390, bpsk_tuner.h) rounds state-dependently and cannot be spread over lanes, but it does not
// depend on the input.  So it is walked per stream, once a call, on the device:
//
//   k_tuner_walk : one lane per stream walks the L samples of the call in order (one FP64 add, compare and conditional
//                  subtract a sample) and leaves tuPhase as it stands before every PST_C-th sample (the checkpoints: 8 bytes
//                  per PST_C samples and stream), the stream's new tuPhase, and the 9-bit table indices of the call's last
//                  26 samples -- the factors the next call's first windows were mixed with, whatever the tuning is by then.
//   k_front_pst  : one workgroup = up to 256 consecutive decimated outputs of ONE stream (k_chan_front's tile).
//                  Phase 1: the tile's 26 + tile samples get their indices -- a lane per checkpoint steps PST_C samples from
//                  it and leaves the phases in LDS (the dependent chain, short), then every lane turns phases into indices
//                  (the correctly rounded FP64 division, spread over the workgroup); samples before the call take the kept
//                  indices.  Then the samples are read once, DC-corrected and converted as JavaAudio does (or taken as the
//                  float input), multiplied by their factors sc9[k] / sc9[257 + k] -- entry 256 = (1.0, 1.0), the exact
//                  pass-through of :395 -- and parked in LDS as doubles.  The product of a sample and its factor is the same
//                  double in every window the sample falls into, so it is formed once a sample and not once a tap.
//                  Phase 2: every lane owns one output and sums its 27 taps newest -> oldest, each product and sum rounded by
//                  itself (:479-483), x HOWARD (:486), the shared VCO factor (:515-516), into the stream's dm row --
//                  k_front_split's arithmetic per output, operation for operation.
//
// k_hist_in, k_matched, k_dm_history, the tail, sync and FEC run on the rows unchanged.
//
// A call with a tuning plan (jsdr_bpsk_plan_stream_tunings: stream s takes a new tuPhaseInc at sample n of the call, PstPlanArgs)
// runs the planned forms k_tuner_walk_plan and k_front_pst_plan<F32IN> -- the same two bodies, instantiated with PLAN = true; a call
// without one launches k_tuner_walk and k_front_pst<F32IN>, whose code the plan does not touch.  The planned walk's lane keeps
// the position of its stream's next entry: a checkpoint block in which no lane of the wave has an entry runs the plain loop, and
// one that has steps with a position compare a sample (taken by the whole wave, so that the wave walks one loop and not two).
// Beside each checkpoint it leaves the number of the stream's entries before the block's first sample (4 bytes), and the
// increment the stream came into the call with; phase 1 of the planned front end starts a block from those and switches at the
// entries inside it, as the walk did.  Nothing is kept per sample.
//
// A call with a ramp plan (jsdr_bpsk_plan_stream_ramps, PstRampArgs: from its sample on an entry's tuning moves by its slope a
// sample) runs the third forms k_tuner_walk_ramp and k_front_pst_ramp<F32IN>, the same bodies with RAMP = true.  Under a slope
// tuPhaseInc is the sample's own -- tuner_ramp_inc (bpsk_tuner.h): a product, a sum and tuner_inc's true FP64 division, none of
// which waits for the tuPhase chain -- so a block takes the per-sample loop where it holds an entry OR lies under a slope (in the
// walk: in some lane of the wave; lanes under no slope keep their increment).  The checkpoints say as much as for steps: the
// entry count before a block names the entry in effect, whose position gives the block's first k.  Nothing more is stored.
#include "common.h"
#include "bpsk_tuner.h"
#include "bpsk_pst.h"

namespace jsdr {

enum { PST_THREADS = 256, PST_WALK_THREADS = 64 };

// The two kernels' bodies are stated once each, in bpsk_pst_walk_body.h and bpsk_pst_front_body.h, and included between the braces
// of the plain, the planned and the ramp form with PLAN and RAMP set: a body handed its kernel's argument struct as a function argument compiles to
// other (equivalent) code than one that reads it in place, and the plain forms' code objects are pinned (tools/kernel_asm_diff.py).
// RAMP: the entry in effect in the walk's lane -- its tuning, slope and position; no slope: the lane's increment stands.  (Declared by
// the three forms in front of the body: a local the body declares itself moves the planned form's instructions about.)
struct PstRampAt {
    double t = 0.0, s = 0.0;
    long long at = 0;
};

__global__ __launch_bounds__(PST_WALK_THREADS) void k_tuner_walk(TunerWalkArgs a)
{
    constexpr bool PLAN = false, RAMP = false;
    const PstPlanArgs p{};
    const PstRampArgs r{};
    PstRampAt ra;
#include "bpsk_pst_walk_body.h"
}

__global__ __launch_bounds__(PST_WALK_THREADS) void k_tuner_walk_plan(TunerWalkArgs a, PstPlanArgs p)
{
    constexpr bool PLAN = true, RAMP = false;
    const PstRampArgs r{};
    PstRampAt ra;
#include "bpsk_pst_walk_body.h"
}

__global__ __launch_bounds__(PST_WALK_THREADS) void k_tuner_walk_ramp(TunerWalkArgs a, PstPlanArgs p, PstRampArgs r)
{
    constexpr bool PLAN = true, RAMP = true;
    PstRampAt ra;
#include "bpsk_pst_walk_body.h"
}

template <bool F32IN>
__global__ __launch_bounds__(PST_THREADS) void k_front_pst(PstFrontArgs a)
{
    constexpr bool PLAN = false, RAMP = false;
    const PstPlanArgs p{};
    const PstRampArgs r{};
#include "bpsk_pst_front_body.h"
}

template <bool F32IN>
__global__ __launch_bounds__(PST_THREADS) void k_front_pst_plan(PstFrontArgs a, PstPlanArgs p)
{
    constexpr bool PLAN = true, RAMP = false;
    const PstRampArgs r{};
#include "bpsk_pst_front_body.h"
}

template <bool F32IN>
__global__ __launch_bounds__(PST_THREADS) void k_front_pst_ramp(PstFrontArgs a, PstPlanArgs p, PstRampArgs r)
{
    constexpr bool PLAN = true, RAMP = true;
#include "bpsk_pst_front_body.h"
}

// actionPerformed's dmMaxCorr = 0 (:190) on the streams one action names
__global__ void k_reset_maxcorr_list(TailState *st, const int *ids, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st[ids[i]].dmMaxCorr = 0;
}

int launch_tuner_walk(const TunerWalkArgs &a, const PstPlanArgs *plan, const PstRampArgs *ramp, hipStream_t st)
{
    const dim3 grid((unsigned)((a.nstreams + PST_WALK_THREADS - 1) / PST_WALK_THREADS));
    if (plan && ramp)
        hipLaunchKernelGGL(k_tuner_walk_ramp, grid, dim3(PST_WALK_THREADS), 0, st, a, *plan, *ramp);
    else if (plan)
        hipLaunchKernelGGL(k_tuner_walk_plan, grid, dim3(PST_WALK_THREADS), 0, st, a, *plan);
    else
        hipLaunchKernelGGL(k_tuner_walk, grid, dim3(PST_WALK_THREADS), 0, st, a);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_front_pst(const PstFrontArgs &a_in, int nstreams, bool f32in, const PstPlanArgs *plan, const PstRampArgs *ramp, hipStream_t st)
{
    PstFrontArgs a = a_in;
    // outputs per workgroup: 256, fewer where a tile's samples (16 bytes of mixed doubles and 2 of index each) would not fit
    // 64 KB of LDS (decimations above 13)
    const size_t fixed = (514 + 28) * sizeof(double), per = sizeof(double2) + sizeof(unsigned short);
    const int cap = (int)((65536 - fixed) / per);
    long long nout = (cap - 27) / a.decim + 1;
    if (nout > PST_THREADS) nout = PST_THREADS;
    if (nout < 1) {
        set_error("bpsk tuned: decimation %d is too large for the tuned front end", a.decim);
        return JSDR_ERR;
    }
    a.nout = (int)nout;
    const size_t lds = fixed + ((size_t)(nout - 1) * a.decim + 27) * per;
    const long long gx = (a.nds + nout - 1) / nout;
    const dim3 grid((unsigned)gx, (unsigned)nstreams);
    if (plan && ramp && f32in) {
        JSDR_LDS_ATTR((k_front_pst_ramp<true>), lds);
        hipLaunchKernelGGL((k_front_pst_ramp<true>), grid, dim3(PST_THREADS), lds, st, a, *plan, *ramp);
    } else if (plan && ramp) {
        JSDR_LDS_ATTR((k_front_pst_ramp<false>), lds);
        hipLaunchKernelGGL((k_front_pst_ramp<false>), grid, dim3(PST_THREADS), lds, st, a, *plan, *ramp);
    } else if (plan && f32in) {
        JSDR_LDS_ATTR((k_front_pst_plan<true>), lds);
        hipLaunchKernelGGL((k_front_pst_plan<true>), grid, dim3(PST_THREADS), lds, st, a, *plan);
    } else if (plan) {
        JSDR_LDS_ATTR((k_front_pst_plan<false>), lds);
        hipLaunchKernelGGL((k_front_pst_plan<false>), grid, dim3(PST_THREADS), lds, st, a, *plan);
    } else if (f32in) {
        JSDR_LDS_ATTR((k_front_pst<true>), lds);
        hipLaunchKernelGGL((k_front_pst<true>), dim3((unsigned)gx, (unsigned)nstreams), dim3(PST_THREADS), lds, st, a);
    } else {
        JSDR_LDS_ATTR((k_front_pst<false>), lds);
        hipLaunchKernelGGL((k_front_pst<false>), dim3((unsigned)gx, (unsigned)nstreams), dim3(PST_THREADS), lds, st, a);
    }
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_reset_maxcorr_list(TailState *st, const int *ids, int n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_reset_maxcorr_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, st, ids, n);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
