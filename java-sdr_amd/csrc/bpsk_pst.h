// bpsk_pst.h -- the front end of a tuned handle (jsdr_bpsk_create_tuned: every stream its own tuning), bpsk_pst.hip, as
// bpsk_call_pst.hip starts it.
#pragma once
#include "common.h"
#include "bpsk_kernels.h"

namespace jsdr {

// samples between two checkpoints of the walk: 8 bytes per PST_C samples and stream is what the tuner costs in memory
// (1/8 byte a sample, against 4 of the int16 input)
enum { PST_C = 64 };

constexpr long long PST_NO_ENTRY = 0x7fffffffffffffffLL;  // the position of "no further entry"

// where the phase of the tile's sample e is parked: one double of padding per 64, so that the lanes of phase 1 (64 samples
// apart) do not all store into one LDS bank
__device__ __forceinline__ int pst_slot(int e) { return e + (e >> 6); }

struct TunerWalkArgs {
    double *tu;                    // [S] tuPhase: read at the start, the call's end value written back
    const double *inc;             // [S] tuPhaseInc
    double *ckpt;                  // [S][ckpt_stride]: tuPhase as it stands BEFORE sample c * PST_C of the call
    long long ckpt_stride;
    long long nsamples;            // L
    const unsigned short *kh_old;  // [S][32]: the 9-bit indices of the 26 samples before the call
    unsigned short *kh_new;        // [S][32]: ... of the 26 samples before the next one
    int nstreams;
};

struct PstFrontArgs {
    const int *raw;                // int16 pairs as dwords, [S][stride_pairs]; k_front_pst<true>: float2 samples
    long long stride_pairs;
    int ic, qc;
    const int2 *hist;              // [S][32]: the 26 inputs before the call (k_hist_in)
    const double *inc;             // [S]
    const double *ckpt;            // [S][ckpt_stride], k_tuner_walk's
    long long ckpt_stride;
    const unsigned short *kh_old;  // [S][32]
    const unsigned char *kvco;     // [nds] shared VCO table index
    const double *sc9;             // cos[0..256], sin[0..256], (1.0, 1.0) at 256
    const double *ds_taps;         // [27]
    double2 *dm;                   // [S][dm_stride]: 64 history + nds VCO-mixed samples
    long long dm_stride;
    long long nds;
    int first_out;                 // input index whose arrival completes output 0
    int decim;
    int nout;                      // outputs per workgroup (set by the launcher)
};

// A tuning plan on the device (jsdr_bpsk_plan_stream_tunings), as the planned forms k_tuner_walk_plan / k_front_pst_plan read it:
// stream s's entries are off[s] .. off[s + 1] - 1; entry e says "from sample pos[e] of the call on, tuPhaseInc = inc[e]" (the
// advance of sample pos[e] is the first at it); pos ascends strictly within a stream and every pos lies inside the call.
struct PstPlanArgs {
    const long long *off;  // [S + 1]
    const long long *pos;  // [off[S]]
    const double *inc;     // [off[S]] 2 pi tuning / rate, the double the host writes for a tuning set between calls
    double *inc0;          // [S] the walk leaves tuPhaseInc as the stream came into the call (before its first entry)
    int *ckpt_e;           // [S][ckpt_stride] the walk leaves the number of the stream's entries before sample c * PST_C
    double *inc_out;       // [S] the walk leaves tuPhaseInc as the stream goes out of the call (the handle's tuPhaseInc array)
};

// A ramp plan (jsdr_bpsk_plan_stream_ramps), beside PstPlanArgs, as the ramp forms k_tuner_walk_ramp / k_front_pst_ramp read it:
// entry e says "sample n >= pos[e] of the call has tuning tuning[e] + (double)(n - pos[e]) * slope[e]" (tuner_ramp_tuning; a slope
// of zero: tuning[e] itself) until the stream's next entry, and tuPhaseInc is tuner_inc of it.  PstPlanArgs::inc is not read.
struct PstRampArgs {
    const double *tuning;  // [off[S]] Hz
    const double *slope;   // [off[S]] Hz per sample
    double rate;           // the sample rate, as the double tuPhaseInc is divided by
};

// The front end of a tuned channel handle (jsdr_bpsk_create_tuned_channels, bpsk_chan_pst.hip): nch channels per input, channel c
// of input i is row i * nch + c of the walk's arrays and of dm; the input and its history are per INPUT, as k_chan_front's.
struct PstChanFrontArgs {
    const int *raw;                // int16 pairs as dwords, [ninputs][stride_pairs]; k_chan_front_pst<true>: float2 samples
    long long stride_pairs;        // between inputs
    int ic, qc;
    const int2 *hist;              // [ninputs][32]: the 26 inputs before the call (k_hist_in)
    const double *inc;             // [ninputs * nch]
    const double *ckpt;            // [ninputs * nch][ckpt_stride], k_tuner_walk's
    long long ckpt_stride;
    const unsigned short *kh_old;  // [ninputs * nch][32]
    const unsigned char *kvco;     // [nds] shared VCO table index
    const double *sc9;             // cos[0..256], sin[0..256], (1.0, 1.0) at 256
    const double *ds_taps;         // [27]
    double2 *dm;                   // [ninputs * nch][dm_stride]: 64 history + nds VCO-mixed samples
    long long dm_stride;
    long long nds;
    int first_out;                 // input index whose arrival completes output 0
    int decim;
    int nch;                       // channels per input
    int nout;                      // outputs per workgroup (set by the launcher)
};

// plan: null for a call without one (the kernels of such a call do not know of plans); ramp: null, or with plan for a ramp plan
int launch_chan_front_pst(const PstChanFrontArgs &a, int ninputs, bool f32in, const PstPlanArgs *plan, const PstRampArgs *ramp, hipStream_t st);
int launch_tuner_walk(const TunerWalkArgs &a, const PstPlanArgs *plan, const PstRampArgs *ramp, hipStream_t st);
int launch_front_pst(const PstFrontArgs &a, int nstreams, bool f32in, const PstPlanArgs *plan, const PstRampArgs *ramp, hipStream_t st);
// dmMaxCorr = 0 (:190) in the n streams ids[] names
int launch_reset_maxcorr_list(TailState *st, const int *ids, int n, hipStream_t stream);

}  // namespace jsdr
