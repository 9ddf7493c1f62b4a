// bpsk_chan_pst_body.h -- the body of k_chan_front_pst<F32IN>, k_chan_front_pst_plan<F32IN> and k_chan_front_pst_ramp<F32IN>
// (bpsk_chan_pst.hip), included between their braces as bpsk_pst_front_body.h is.  In scope: PstChanFrontArgs a, PstPlanArgs p,
// PstRampArgs r, constexpr bool F32IN, PLAN, RAMP.
    extern __shared__ __align__(16) unsigned char smem[];
    double *sc = reinterpret_cast<double *>(smem);                        // [514] cos[0..256], sin[0..256]
    double *taps = sc + 514;                                              // [27]
    const int D = a.decim;
    const int cap = (a.nout - 1) * D + 27;
    double *tus = taps + 28;                                              // [pst_slot(cap - 1) + 1] the phases of the channel under way
    float2 *x = reinterpret_cast<float2 *>(tus + pst_slot(cap - 1) + 1);  // [cap] the tile's samples, converted
    unsigned short *k9 = reinterpret_cast<unsigned short *>(x + cap);     // [cap] the table indices of the channel under way
    for (int i = threadIdx.x; i < 514; i += blockDim.x) sc[i] = a.sc9[i];
    if (threadIdx.x < 27) taps[threadIdx.x] = a.ds_taps[threadIdx.x];
    const int in = blockIdx.y;
    const long long j0 = (long long)blockIdx.x * a.nout;
    const long long jend = (j0 + a.nout < a.nds) ? j0 + a.nout : a.nds;
    const long long n_lo = (long long)a.first_out + (long long)D * j0 - 26;  // input index of x[0] (>= -26)
    const int cnt = (int)((jend - 1 - j0) * D + 27);                         // <= cap
    chan_pst_park<F32IN>(a, in, n_lo, cnt, x);
    const long long j = j0 + threadIdx.x;  // (a lane past the tile's last output waits at the barriers with the others)
    const int kv = j < jend ? a.kvco[j] : 0;
    for (int c = 0; c < a.nch; c++) {  // a channel at a time through tus and k9
        const int s = in * a.nch + c;
#include "bpsk_pst_phase1.h"
        if (j < jend) chan_pst_taps(a, sc, taps, x, k9, s, j, kv);
        __syncthreads();  // from here on tus and k9 are the next channel's
    }
