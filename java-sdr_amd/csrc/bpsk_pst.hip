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
#include "common.h"
#include "bpsk_tuner.h"
#include "bpsk_pst.h"

namespace jsdr {

enum { PST_THREADS = 256, PST_WALK_THREADS = 64 };

__global__ __launch_bounds__(PST_WALK_THREADS) void k_tuner_walk(TunerWalkArgs a)
{
    const int s = blockIdx.x * PST_WALK_THREADS + threadIdx.x;
    if (s >= a.nstreams) return;
    const long long L = a.nsamples;
    double tu = a.tu[s];
    const double inc = a.inc[s];
    double *ck = a.ckpt + (long long)s * a.ckpt_stride;
    const unsigned short *ko = a.kh_old + (long long)s * 32;
    unsigned short *kn = a.kh_new + (long long)s * 32;
    const long long keep = L < 26 ? L : 26;  // samples of this call among the 26 before the next one
    for (int i = 0; i < 26 - (int)keep; i++) kn[i] = ko[i + L];  // (a call shorter than the history: the rest moves up)
    const long long nmain = L - keep;
    for (long long c = 0; c * PST_C < L; c++) {
        ck[c] = tu;  // c < ckpt_stride: L <= max_batch_samples
        const long long n1 = (c + 1) * PST_C < L ? (c + 1) * PST_C : L;
        for (long long n = c * PST_C; n < n1; n++) {
            tuner_advance(tu, inc);
            if (n >= nmain) kn[26 - (L - n)] = (unsigned short)tuner_k9(tu);  // (uniform: the division runs 26 times a call)
        }
    }
    a.tu[s] = tu;
}

// where the phase of the tile's sample e is parked: one double of padding per 64, so that the lanes of phase 1 (64 samples
// apart) do not all store into one LDS bank
__device__ __forceinline__ int pst_slot(int e) { return e + (e >> 6); }

template <bool F32IN>
__global__ __launch_bounds__(PST_THREADS) void k_front_pst(PstFrontArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double *sc = reinterpret_cast<double *>(smem);            // [514] cos[0..256], sin[0..256]
    double *taps = sc + 514;                                  // [27]
    double2 *x = reinterpret_cast<double2 *>(taps + 28);      // [cap] the tile's samples, mixed
    double *tus = reinterpret_cast<double *>(x);              // ... before that, their phases (pst_slot)
    const int D = a.decim;
    const int cap = (a.nout - 1) * D + 27;
    unsigned short *k9 = reinterpret_cast<unsigned short *>(x + cap);  // [cap] their table indices
    for (int i = threadIdx.x; i < 514; i += blockDim.x) sc[i] = a.sc9[i];
    if (threadIdx.x < 27) taps[threadIdx.x] = a.ds_taps[threadIdx.x];
    const int s = blockIdx.y;
    const long long j0 = (long long)blockIdx.x * a.nout;
    const long long jend = (j0 + a.nout < a.nds) ? j0 + a.nout : a.nds;
    const long long n_lo = (long long)a.first_out + (long long)D * j0 - 26;  // input index of x[0] (>= -26)
    const int cnt = (int)((jend - 1 - j0) * D + 27);                         // <= cap
    // ---- phase 1: the phases of the tile's samples of this call, PST_C of them a lane from the checkpoint before them
    const long long n_first = n_lo < 0 ? 0 : n_lo;
    const long long n_last = n_lo + cnt - 1;  // the newest sample of the tile's last output: 0 <= n_last < L
    const double inc = a.inc[s];
    const double *ck = a.ckpt + (long long)s * a.ckpt_stride;
    for (long long c = n_first / PST_C + threadIdx.x; c <= n_last / PST_C; c += blockDim.x) {
        double tu = ck[c];
        const long long nb = c * PST_C;
        for (int i = 0; i < PST_C; i++) {
            tuner_advance(tu, inc);
            const long long n = nb + i;
            if (n >= n_first && n <= n_last) tus[pst_slot((int)(n - n_lo))] = tu;
        }
    }
    __syncthreads();
    const unsigned short *ko = a.kh_old + (long long)s * 32;
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
        const long long n = n_lo + e;
        k9[e] = n < 0 ? ko[26 + n] : (unsigned short)tuner_k9(tus[pst_slot(e)]);
    }
    __syncthreads();
    // ---- the samples, read once, converted and mixed (:372-373, :388-390 / :395)
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const int2 *hist = a.hist + (long long)s * 32;
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
        const long long n = n_lo + e;
        float2 f;
        if constexpr (F32IN) {
            if (n >= 0) {
                f = reinterpret_cast<const float2 *>(a.raw)[(long long)s * a.stride_pairs + n];
            } else {
                const int2 h = hist[26 + n];  // the float pair's bits (k_hist_in)
                f = make_float2(__int_as_float(h.x), __int_as_float(h.y));
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
            f = make_float2(i16_to_float_java((int)(short)(w & 0xffff)), i16_to_float_java(w >> 16));
        }
        const int k = k9[e];
        double di = (double)f.x, dq = (double)f.y;
        di = di * sc[k];
        dq = dq * sc[257 + k];
        x[e] = make_double2(di, dq);
    }
    __syncthreads();
    // ---- phase 2: one output a lane
    const long long j = j0 + threadIdx.x;
    if (j >= jend) return;
    const double HOWARD = 0.9 * 32768.0;                         // :469
    const double2 *xw = x + (long long)D * threadIdx.x + 26;     // xw[-age] = the sample `age` before the one that completes output j
    double fi = 0.0, fq = 0.0;
    for (int age = 0; age < 27; age++) {
        const double2 v = xw[-age];
        const double tp = taps[age];
        fi += v.x * tp;
        fq += v.y * tp;
    }
    const double oi = fi * HOWARD, oq = fq * HOWARD;  // :486
    const int kv = a.kvco[j];
    a.dm[(long long)s * a.dm_stride + 64 + j] = make_double2(oi * sc[kv], oq * sc[257 + kv]);  // :515-516
}

// actionPerformed's dmMaxCorr = 0 (:190) on the streams one action names
__global__ void k_reset_maxcorr_list(TailState *st, const int *ids, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st[ids[i]].dmMaxCorr = 0;
}

int launch_tuner_walk(const TunerWalkArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_tuner_walk, dim3((unsigned)((a.nstreams + PST_WALK_THREADS - 1) / PST_WALK_THREADS)), dim3(PST_WALK_THREADS), 0, st, a);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_front_pst(const PstFrontArgs &a_in, int nstreams, bool f32in, hipStream_t st)
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
    if (f32in) {
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
