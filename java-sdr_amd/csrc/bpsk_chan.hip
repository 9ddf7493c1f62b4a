// bpsk_chan.hip -- the tune-mode front end of a channel handle (jsdr_bpsk_create_channels): ninputs x nchannels
// demodulators, channel c of input i is stream i * nchannels + c.  Exact-order FP64 (-ffp-contract=off).
//
// One workgroup = up to 256 consecutive decimated outputs of ONE input.  The raw samples their 27-tap windows cover are
// read from memory once, DC-corrected and converted int16 -> float (JavaAudio's rule) once, and parked in LDS as float2
// (exact: (double)f is what the reference multiplies); float input (F32IN, jsdr_bpsk_batch_f32) IS that image and is parked as read.  Then every thread owns one output and walks its window newest ->
// oldest (FUNcubeBPSKDemod.java:479-483) for every channel of the input, CG channels at a time with their accumulator pairs
// in registers, so one LDS read of a sample serves CG channels.  Per channel and sample the tuner factor (:388-390,
// component-wise) comes from a 9-bit index into cos[0..256] / sin[0..256] whose entry 256 is (1.0, 1.0): a sample the
// reference passes through unmixed (:395) is multiplied by 1.0, which changes nothing.  The index table of a channel is
// either periodic (an exact cycle, index (n + 26) mod per) or one entry per sample of the call, 26 history samples first
// (k_front_split's table: after a retune, or a tuning whose cycle is longer than 256 samples).
// Then x HOWARD (:486) and the shared VCO mix (:515-516) into dm[stream][64 + j]: k_matched, k_dm_history, k_tail and the
// FEC forms run on those rows unchanged.  Every product and sum is the one k_front_any / k_front_reg do, in their order.
#include "common.h"
#include "bpsk_chan.h"

namespace jsdr {

enum { CHAN_THREADS = 256, CHAN_CG = 4 };

template <int CG, bool F32IN = false>
__global__ __launch_bounds__(CHAN_THREADS) void k_chan_front(ChanFrontArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double *sc = reinterpret_cast<double *>(smem);           // [514] cos[0..256], sin[0..256]
    double *taps = sc + 514;                                 // [27]
    float2 *x = reinterpret_cast<float2 *>(taps + 28);       // [(nout - 1) D + 27] converted samples of this tile
    for (int i = threadIdx.x; i < 514; i += blockDim.x) sc[i] = a.sc9[i];
    if (threadIdx.x < 27) taps[threadIdx.x] = a.ds_taps[threadIdx.x];
    const int in = blockIdx.y;
    const int D = a.decim;
    const long long j0 = (long long)blockIdx.x * a.nout;
    const long long jend = (j0 + a.nout < a.nds) ? j0 + a.nout : a.nds;
    const long long n_lo = (long long)a.first_out + (long long)D * j0 - 26;  // input index of x[0] (>= -26)
    const int cnt = (int)((jend - 1 - j0) * D + 27);
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
            continue;
        }
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
    __syncthreads();
    const long long j = j0 + threadIdx.x;
    if (j >= jend) return;
    const double HOWARD = 0.9 * 32768.0;  // :469
    const long long n_new = (long long)a.first_out + (long long)D * j;  // the input whose arrival completes output j
    const float2 *xw = x + (long long)D * threadIdx.x + 26;             // xw[-age] = sample n_new - age
    const int kv = a.kvco[j];
    const double vc = sc[kv], vs = sc[257 + kv];
    for (int c0 = 0; c0 < a.nch; c0 += CG) {
        double fi[CG], fq[CG];
        int idx[CG];
#pragma unroll
        for (int u = 0; u < CG; u++) {
            fi[u] = 0.0;
            fq[u] = 0.0;
            const int c = c0 + u < a.nch ? c0 + u : c0;
            const int per = a.per[c];
            // periodic: entry (n + 26) mod per; otherwise entry n + 26 of the call's table
            idx[u] = per > 0 ? (int)((n_new + 26) % per) : (int)(n_new + 26);
        }
        for (int age = 0; age < 27; age++) {
            const float2 v = xw[-age];
            const double tp = taps[age];
#pragma unroll
            for (int u = 0; u < CG; u++) {
                const int c = c0 + u < a.nch ? c0 + u : c0;
                const int k = a.k9[c][idx[u]];
                double di = (double)v.x, dq = (double)v.y;  // (double)buf[n*2]  :372
                di = di * sc[k];                             // :388-390
                dq = dq * sc[257 + k];
                fi[u] += di * tp;
                fq[u] += dq * tp;
                const int per = a.per[c];
                idx[u] = per > 0 ? (idx[u] == 0 ? per - 1 : idx[u] - 1) : idx[u] - 1;
            }
        }
#pragma unroll
        for (int u = 0; u < CG; u++) {
            const int c = c0 + u;
            if (c < a.nch) {
                const double oi = fi[u] * HOWARD, oq = fq[u] * HOWARD;  // :486
                a.dm[((long long)in * a.nch_all + a.chan_of[c]) * a.dm_stride + 64 + j] = make_double2(oi * vc, oq * vs);  // :515-516
            }
        }
    }
}

int launch_chan_front(const ChanFrontArgs &a_in, int ninputs, bool f32in, hipStream_t st)
{
    ChanFrontArgs a = a_in;
    // outputs per workgroup: 256, fewer where a tile's samples would not fit 64 KB of LDS (decimations above 31)
    const int cap = (int)((65536 - (514 + 28) * sizeof(double)) / sizeof(float2));
    long long nout = (cap - 27) / a.decim + 1;
    if (nout > CHAN_THREADS) nout = CHAN_THREADS;
    if (nout < 1) {
        set_error("bpsk channels: decimation %d is too large for the channel front end", a.decim);
        return JSDR_ERR;
    }
    a.nout = (int)nout;
    const size_t lds = (514 + 28) * sizeof(double) + ((size_t)(nout - 1) * a.decim + 27) * sizeof(float2);
    const long long gx = (a.nds + nout - 1) / nout;
    if (f32in) {
        JSDR_LDS_ATTR((k_chan_front<CHAN_CG, true>), lds);
        hipLaunchKernelGGL((k_chan_front<CHAN_CG, true>), dim3((unsigned)gx, (unsigned)ninputs), dim3(CHAN_THREADS), lds, st, a);
    } else {
        JSDR_LDS_ATTR((k_chan_front<CHAN_CG, false>), lds);
        hipLaunchKernelGGL((k_chan_front<CHAN_CG, false>), dim3((unsigned)gx, (unsigned)ninputs), dim3(CHAN_THREADS), lds, st, a);
    }
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
