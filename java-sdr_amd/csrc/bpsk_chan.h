// bpsk_chan.h -- the channel handle's tune-mode front end (bpsk_chan.hip), launched from bpsk_call_chan.hip.
#pragma once
#include "common.h"

namespace jsdr {

enum { CHAN_MAX = 16 };

struct ChanFrontArgs {
    const int *raw;                     // int16 pairs as dwords, [ninputs][stride_pairs]; k_chan_front<.., F32IN>: float2 samples
    long long stride_pairs;             // between inputs
    int ic, qc;
    const int2 *hist;                   // [ninputs][32]: the 26 inputs before this call, DC-corrected int16 pair (.x) or float2 bits
    const unsigned short *k9[CHAN_MAX]; // per channel: 9-bit tuner index table (256: pass-through)
    int per[CHAN_MAX];                  // per channel: period of k9 (entry (n + 26) mod per), or 0: k9[26 + n]
    int nch;                            // channels this launch takes ...
    int nch_all;                        // ... of the handle's channels per input: stream = input * nch_all + chan_of[c]
    int chan_of[CHAN_MAX];              // (a handle whose channels are all in the tune mode: nch_all = nch, chan_of[c] = c)
    const unsigned char *kvco;          // [nds] shared VCO table index
    const double *sc9;                  // cos[0..256], sin[0..256], (1.0, 1.0) at 256
    const double *ds_taps;              // [27]
    double2 *dm;                        // [ninputs * nch][dm_stride]: 64 history + nds VCO-mixed samples
    long long dm_stride;
    long long nds;
    int first_out;                      // input index whose arrival completes output 0
    int decim;
    int nout;                           // outputs per workgroup (set by the launcher)
};

int launch_chan_front(const ChanFrontArgs &a, int ninputs, bool f32in, hipStream_t st);

}  // namespace jsdr
