// bpsk_front.hip -- tune mode, the front end on its own: int16 / float -> double, tuner mix, 27-tap low-pass at the
// decimated instants (newest-first order, FUNcubeBPSKDemod.java:479-483), x HOWARD_FUDGE_FACTOR, VCO mix -> dm[s][64+j].
//
//   k_front       : generic, and float input (int16 input takes k_front_reg, bpsk_front_reg.hip, where that applies)
//   k_front_any   : any decimation;  k_front_split: a call that straddles the tuner's sign test (after a retune)
//   k_hist_in, k_hist_convert : the 26-sample input history between calls
//   k_seam_hist, k_seam_q     : jsdr_bpsk_set_mode, tune -> FFT-acquire
//   k_chan_seam_hist          : the same seam on one channel of a live channel handle (jsdr_bpsk_create_live_channels)
// and their launchers (bpsk_kernels.h).
//
// One of the four units of the tune-mode pipeline, which is cut by kernel family so that an edit to one family recompiles
// that family only: bpsk_front.hip, bpsk_front_reg.hip, bpsk_fm.hip, bpsk_tail.hip (the pipeline's overview is at the top
// of the last).  Compiled with -ffp-contract=off: every double product and sum is rounded separately, in the reference's
// order.  Reads ds_taps of its copy of the tables (k_front_any, k_front_split).
#include "bpsk_units.h"
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

namespace jsdr {

namespace front { __constant__ BpskConst c_bpsk; }  // this unit's copy of the tables, under this unit's name (bpsk_units.h)
using front::c_bpsk;

// ------------------------------------------------------------------------------------------- k_front
// int16 -> float -> double, tuner mix, 27-tap low-pass at the decimated instants, x HOWARD, VCO mix.
//
// One wave = one tile of 64*R consecutive outputs of one stream (R = RD/D outputs per lane).
//   stage : the wave copies the tile's raw IQ dwords (4 B/sample, fully coalesced, loads issued in batches
//           of 8) and tuner indices (1 B/sample) into LDS -- 5 B per sample instead of the 16 B of a mixed
//           double2.  Lane l's span starts at sample RD*l; one pad dword (four pad bytes for the indices)
//           per span makes the lane stride odd in dwords: the per-lane reads below are conflict-free.
//   walk  : every lane walks ITS OWN samples from newest to oldest in blocks of D (one output period).
//           A sample at offset t of block b belongs to the windows of outputs b, b-1, .. with ages
//           26-t, 26-t-D, .. (compile-time constants), so the 27-tap sums of NACC = 26/D+1 outputs are in
//           flight at once in rotating register accumulators.  Walking backwards in time makes every
//           output accumulate ages 0,1,..,26: the reference's newest-first order (:479-483).  Each sample
//           is converted and mixed once per lane, in registers; no LDS traffic per multiply-add.
// Samples before the start of the call come from the raw history kept by k_hist_in.
template <int D, int RD>
struct FrontGeom {
    static_assert(RD % D == 0, "a lane span must hold whole outputs");
    static constexpr int R = RD / D;                 // outputs per lane
    static constexpr int NACC = 26 / D + 1;          // outputs whose windows contain one sample
    static_assert(R >= NACC, "span too short for the rotating accumulators");
    static constexpr int NT = 64 * RD - D + 27;      // samples per wave tile
    static constexpr int RSTR = RD + 1;              // elements between lane spans (raw)
    static constexpr int KSTR = RD + 4;              // bytes between lane spans (tuner indices)
    static constexpr int RAW_EL = 64 * RSTR + 32;    // raw elements per wave
    static constexpr int K_BYTES = 64 * KSTR + 64;
};


template <bool F32IN>
struct FrontElem {
    using type = int;
};
template <>
struct FrontElem<true> {
    using type = float2;
};

// one block of D samples (newest first): outputs b-JLO .. b-JHI take part
template <int D, int RD, bool F32IN, bool MIX, int JLO, int JHI, int NACC>
__device__ __forceinline__ void front_block(int b, const typename FrontElem<F32IN>::type *xl, const unsigned char *kl,
                                            const double *sc, double (&ai)[NACC], double (&aq)[NACC])
{
#pragma unroll
    for (int t = D - 1; t >= 0; t--) {
        if (26 - t - D * JLO >= 0) {  // the sample lies in at least one participating window (compile time)
            const int m = D * b + t;
            const int wrap = (m >= RD) ? 1 : 0;
            double di, dq;
            if constexpr (F32IN) {
                const float2 f = xl[m + wrap];
                di = (double)f.x;  // (double)buf[n*2]  :372
                dq = (double)f.y;
            } else {
                const int w = xl[m + wrap];
                di = (double)i16_to_float_java((int)(short)(w & 0xffff));
                dq = (double)i16_to_float_java(w >> 16);
            }
            if constexpr (MIX) {  // :388-390 component-wise, not a complex multiply (a template flag, not a
                                  // branch: the block stays one basic block and its LDS reads pipeline)
                const int k = kl[m + 4 * wrap];
                di = di * sc[k];
                dq = dq * sc[256 + k];
            }
#pragma unroll
            for (int j = JLO; j <= JHI; j++) {
                if (26 - t - D * j >= 0) {  // age of this sample in the window of output b-j
                    const double tp = ds_tap(26 - t - D * j);
                    ai[j] += di * tp;
                    aq[j] += dq * tp;
                }
            }
        }
    }
}

template <int D, int RD, bool F32IN, bool MIX>
__global__ __launch_bounds__(128, 4) void k_front(FrontArgs a)
{
    using G = FrontGeom<D, RD>;
    using Elem = typename FrontElem<F32IN>::type;
    constexpr int R = G::R, NACC = G::NACC;
    extern __shared__ __align__(16) unsigned char smem[];
    double *sc = reinterpret_cast<double *>(smem);  // [512]
    for (int i = threadIdx.x; i < 512; i += blockDim.x) sc[i] = a.sincos[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    constexpr size_t WAVE_BYTES = (size_t)G::RAW_EL * sizeof(Elem) + G::K_BYTES;
    unsigned char *wbase = smem + 512 * sizeof(double) + wave * WAVE_BYTES;
    Elem *rawL = reinterpret_cast<Elem *>(wbase);
    unsigned char *kL = wbase + (size_t)G::RAW_EL * sizeof(Elem);
    const int s = blockIdx.y;
    const long long ntiles = (a.nds + 64 * R - 1) / (64 * R);
    const double HOWARD = 0.9 * 32768.0;  // :469
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const float2 *rawf = a.rawf + (long long)s * a.stride_pairs;
    const int2 *hist = a.hist + (long long)s * 32;
    const long long L = a.nsamples;
    for (long long tile = (long long)blockIdx.x * nwave + wave; tile < ntiles; tile += (long long)gridDim.x * nwave) {
        const long long j0 = tile * 64 * R;
        const long long lo = (long long)a.first_out + (long long)D * j0 - 26;  // input index of tile sample 0
        // ---- stage raw samples + tuner indices: 8 independent loads in flight per lane
        constexpr int NIT = (G::NT + 63) / 64;
#pragma unroll 1
        for (int it0 = 0; it0 < NIT; it0 += 8) {
            Elem w[8];
            unsigned char kk[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int e = (it0 + u) * 64 + lane;
                const long long n = lo + e;
                const bool inr = (n >= 0) && (n < L);
                const long long idx = inr ? n : 0;
                if constexpr (F32IN) w[u] = rawf[idx]; else w[u] = raw[idx];
                kk[u] = a.ktu[26 + idx];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int e = (it0 + u) * 64 + lane;
                const long long n = lo + e;
                const bool inr = (n >= 0) && (n < L);
                if (e < G::NT) {
                    Elem v = w[u];
                    if constexpr (F32IN) {
                        if (!inr) v = make_float2(0.f, 0.f);
                    } else {
                        int si = java_short_add((int)(short)(v & 0xffff), a.ic);
                        int sq = java_short_add(v >> 16, a.qc);
                        v = inr ? ((si & 0xffff) | (sq << 16)) : 0;
                    }
                    const int span = e / RD;
                    rawL[e + span] = v;
                    kL[e + 4 * span] = inr ? kk[u] : (unsigned char)0;
                }
            }
        }
        if (lo < 0) {  // first tile of the call: the 26 inputs before it come from the history
            const int e = lane;
            const long long n = lo + e;
            if (n < 0) {
                const int2 h = hist[26 + n];
                const int span = e / RD;
                if constexpr (F32IN) rawL[e + span] = make_float2(__int_as_float(h.x), __int_as_float(h.y));
                else rawL[e + span] = h.x;
                kL[e + 4 * span] = a.ktu[26 + n];
            }
        }
        JSDR_WAVE_SYNC();
        // ---- walk this lane's span from newest to oldest, one output period per block
        const Elem *xl = rawL + G::RSTR * lane;
        const unsigned char *kl = kL + G::KSTR * lane;
        double ai[NACC], aq[NACC];
#pragma unroll
        for (int j = 0; j < NACC; j++) {
            ai[j] = 0.0;
            aq[j] = 0.0;
        }
        const long long jl = j0 + (long long)R * lane;
        auto finish = [&](int b) {  // output b is complete: x HOWARD (:486), VCO mix (:515-516), rotate
            const long long j = jl + b;
            if (j < a.nds) {
                const double oi = ai[0] * HOWARD, oq = aq[0] * HOWARD;
                if (a.ds_dbg) a.ds_dbg[(long long)s * a.nds + j] = make_double2(oi, oq);
                const int kv = a.kvco[j];
                a.dm[(long long)s * a.dm_stride + 64 + j] = make_double2(oi * sc[kv], oq * sc[256 + kv]);
            }
#pragma unroll
            for (int j2 = 0; j2 + 1 < NACC; j2++) {
                ai[j2] = ai[j2 + 1];
                aq[j2] = aq[j2 + 1];
            }
            ai[NACC - 1] = 0.0;
            aq[NACC - 1] = 0.0;
        };
        auto rotate_only = [&]() {
#pragma unroll
            for (int j2 = 0; j2 + 1 < NACC; j2++) {
                ai[j2] = ai[j2 + 1];
                aq[j2] = aq[j2 + 1];
            }
            ai[NACC - 1] = 0.0;
            aq[NACC - 1] = 0.0;
        };
        // top blocks b = R-1+k (k = NACC-1 .. 1): only outputs <= R-1 exist, i.e. j >= k
        if constexpr (NACC >= 7) { front_block<D, RD, F32IN, MIX, 6, NACC - 1, NACC>(R + 5, xl, kl, sc, ai, aq); rotate_only(); }
        if constexpr (NACC >= 6) { front_block<D, RD, F32IN, MIX, 5, NACC - 1, NACC>(R + 4, xl, kl, sc, ai, aq); rotate_only(); }
        if constexpr (NACC >= 5) { front_block<D, RD, F32IN, MIX, 4, NACC - 1, NACC>(R + 3, xl, kl, sc, ai, aq); rotate_only(); }
        if constexpr (NACC >= 4) { front_block<D, RD, F32IN, MIX, 3, NACC - 1, NACC>(R + 2, xl, kl, sc, ai, aq); rotate_only(); }
        if constexpr (NACC >= 3) { front_block<D, RD, F32IN, MIX, 2, NACC - 1, NACC>(R + 1, xl, kl, sc, ai, aq); rotate_only(); }
        if constexpr (NACC >= 2) { front_block<D, RD, F32IN, MIX, 1, NACC - 1, NACC>(R + 0, xl, kl, sc, ai, aq); rotate_only(); }
        // main blocks: every window exists
#pragma unroll 1
        for (int b = R - 1; b >= NACC - 1; b--) {
            front_block<D, RD, F32IN, MIX, 0, NACC - 1, NACC>(b, xl, kl, sc, ai, aq);
            finish(b);
        }
        // bottom blocks b = NACC-2 .. 0: outputs below 0 belong to the previous lane
        if constexpr (NACC >= 7) { front_block<D, RD, F32IN, MIX, 0, 5, NACC>(5, xl, kl, sc, ai, aq); finish(5); }
        if constexpr (NACC >= 6) { front_block<D, RD, F32IN, MIX, 0, 4, NACC>(4, xl, kl, sc, ai, aq); finish(4); }
        if constexpr (NACC >= 5) { front_block<D, RD, F32IN, MIX, 0, 3, NACC>(3, xl, kl, sc, ai, aq); finish(3); }
        if constexpr (NACC >= 4) { front_block<D, RD, F32IN, MIX, 0, 2, NACC>(2, xl, kl, sc, ai, aq); finish(2); }
        if constexpr (NACC >= 3) { front_block<D, RD, F32IN, MIX, 0, 1, NACC>(1, xl, kl, sc, ai, aq); finish(1); }
        if constexpr (NACC >= 2) { front_block<D, RD, F32IN, MIX, 0, 0, NACC>(0, xl, kl, sc, ai, aq); finish(0); }
        if constexpr (NACC == 1) { /* D >= 27: every block is a main block */ }
        JSDR_WAVE_SYNC();
    }
}

// ------------------------------------------------------------------------------------------- k_front_any
// The front end for ANY decimation rate / 9600 (the reference's audio-rate is a free integer, JavaAudio.java:49,59: 32 kHz
// gives 3, 22.05 kHz 2, 64 kHz 6 ...): one thread per output, its 27-sample window walked newest -> oldest (:479-483) with the
// decimation a run-time value.  Same conversions, same operand order as k_front; no staging, no register blocking -- the
// rates java-sdr ships defaults for (44.1 / 48 / 96 / 192 kHz: decimation 4, 5, 10, 20) have the specialised kernels.
template <bool F32IN>
__global__ __launch_bounds__(256) void k_front_any(FrontArgs a, int D)
{
    __shared__ double sc[512];
    for (int i = threadIdx.x; i < 512; i += blockDim.x) sc[i] = a.sincos[i];
    __syncthreads();
    const int s = blockIdx.y;
    const double HOWARD = 0.9 * 32768.0;  // :469
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const float2 *rawf = a.rawf + (long long)s * a.stride_pairs;
    const int2 *hist = a.hist + (long long)s * 32;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < a.nds; j += (long long)gridDim.x * blockDim.x) {
        const long long n_new = (long long)a.first_out + (long long)D * j;  // the input whose arrival completes output j
        double fi = 0.0, fq = 0.0;
        for (int age = 0; age < DS_N; age++) {
            const long long n = n_new - age;  // >= -26: before the call, the history k_hist_in kept (zeros at the stream's start)
            double di, dq;
            if constexpr (F32IN) {
                float2 f;
                if (n >= 0) {
                    f = rawf[n];
                } else {
                    const int2 h = hist[26 + n];
                    f = make_float2(__int_as_float(h.x), __int_as_float(h.y));
                }
                di = (double)f.x;  // (double)buf[n*2]  :372
                dq = (double)f.y;
            } else {
                int w;
                if (n >= 0) {
                    w = raw[n];
                    const int si = java_short_add((int)(short)(w & 0xffff), a.ic);
                    const int sq = java_short_add(w >> 16, a.qc);
                    w = (si & 0xffff) | (sq << 16);
                } else {
                    w = hist[26 + n].x;  // kept DC-corrected
                }
                di = (double)i16_to_float_java((int)(short)(w & 0xffff));
                dq = (double)i16_to_float_java(w >> 16);
            }
            if (a.mix) {  // :388-390 component-wise, not a complex multiply
                const int k = a.ktu[26 + n];
                di = di * sc[k];
                dq = dq * sc[256 + k];
            }
            const double tp = c_bpsk.ds_taps[age];
            fi += di * tp;
            fq += dq * tp;
        }
        const double oi = fi * HOWARD, oq = fq * HOWARD;  // :486
        if (a.ds_dbg) a.ds_dbg[(long long)s * a.nds + j] = make_double2(oi, oq);
        const int kv = a.kvco[j];
        a.dm[(long long)s * a.dm_stride + 64 + j] = make_double2(oi * sc[kv], oq * sc[256 + kv]);  // :515-516
    }
}

// ------------------------------------------------------------------------------------------- k_front_split
// The front end of a call whose samples are not all on one side of the tuner's sign test (:388): after a retune
// (jsdr_bpsk_set_tuning) tuPhase may walk through 0 inside a call, or the 26 history samples may have been taken on the
// other side.  k_front_any's loop, one thread per output, with a 9-bit tuner index per sample: entries 0..255 are the
// reference's tables, entry 256 is (1.0, 1.0), which passes the sample through exactly (i * 1.0 == i): RxDownSample(i, q)
// of :395.  sc9 = cos[0..256] then sin[0..256].  dh (the first tune call after FFT-acquire frames): the history is the FFT
// path's doubles (I == Q, unmixed) instead of raw samples.  Runs only for calls right after an action, never in the steady state.
template <bool F32IN>
__global__ __launch_bounds__(256) void k_front_split(FrontArgs a, const unsigned short *ktu9, const double *sc9, int D,
                                                     const FftFrontState *dh)
{
    __shared__ double sc[514];
    for (int i = threadIdx.x; i < 514; i += blockDim.x) sc[i] = sc9[i];
    __syncthreads();
    const int s = blockIdx.y;
    const double HOWARD = 0.9 * 32768.0;  // :469
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const float2 *rawf = a.rawf + (long long)s * a.stride_pairs;
    const int2 *hist = a.hist + (long long)s * 32;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < a.nds; j += (long long)gridDim.x * blockDim.x) {
        const long long n_new = (long long)a.first_out + (long long)D * j;
        double fi = 0.0, fq = 0.0;
        for (int age = 0; age < DS_N; age++) {
            const long long n = n_new - age;  // >= -26
            double di, dq;
            if (n < 0 && dh) {  // the first tune call after FFT-acquire frames: dsBuf holds their re values (I == Q, :464)
                di = dh[s].hist[26 + n];
                dq = di;
            } else if constexpr (F32IN) {
                float2 f;
                if (n >= 0) {
                    f = rawf[n];
                } else {
                    const int2 h = hist[26 + n];
                    f = make_float2(__int_as_float(h.x), __int_as_float(h.y));
                }
                di = (double)f.x;
                dq = (double)f.y;
            } else {
                int w;
                if (n >= 0) {
                    w = raw[n];
                    const int si = java_short_add((int)(short)(w & 0xffff), a.ic);
                    const int sq = java_short_add(w >> 16, a.qc);
                    w = (si & 0xffff) | (sq << 16);
                } else {
                    w = hist[26 + n].x;
                }
                di = (double)i16_to_float_java((int)(short)(w & 0xffff));
                dq = (double)i16_to_float_java(w >> 16);
            }
            const int k = ktu9[26 + n];
            di = di * sc[k];
            dq = dq * sc[257 + k];
            const double tp = c_bpsk.ds_taps[age];
            fi += di * tp;
            fq += dq * tp;
        }
        const double oi = fi * HOWARD, oq = fq * HOWARD;  // :486
        const int kv = a.kvco[j];
        a.dm[(long long)s * a.dm_stride + 64 + j] = make_double2(oi * sc[kv], oq * sc[257 + kv]);  // :515-516
    }
}

// jsdr_bpsk_set_mode, tune -> FFT-acquire: the tune path's dsBuf as two columns of doubles, mixed exactly as k_front mixes
// them (or passed through, :395) -- I into the FFT state's history, Q into a copy of the FFT state for the second run
__global__ __launch_bounds__(32) void k_seam_hist(const int2 *hist, int is_float, const double *sincos, SeamHist sh, FftFrontState *st,
                                                  FftFrontState *st2)
{
    const int s = blockIdx.x, t = threadIdx.x;
    if (t < 26) {
        const int2 hv = hist[(long long)s * 32 + t];
        double di, dq;
        if (is_float) {
            di = (double)__int_as_float(hv.x);
            dq = (double)__int_as_float(hv.y);
        } else {
            di = (double)i16_to_float_java((int)(short)(hv.x & 0xffff));
            dq = (double)i16_to_float_java(hv.x >> 16);
        }
        if (sh.mhist[t]) {
            const int k = sh.khist[t];
            di = di * sincos[k];
            dq = dq * sincos[256 + k];
        }
        st[s].hist[t] = di;
        st2[s].hist[t] = dq;
    }
    if (t == 0) {
        st2[s].avePeakPower = st[s].avePeakPower;
        st2[s].aveCentreBin = st[s].aveCentreBin;
        st2[s].centreBin = st[s].centreBin;
    }
}

// ... and the Q rail of the outputs whose windows reach into that history, from the second run's row
__global__ __launch_bounds__(64) void k_seam_q(double2 *dm, long long dm_stride, const double2 *dm2, long long dm2_stride, int J)
{
    const int s = blockIdx.x, j = threadIdx.x;
    if (j < J) dm[(long long)s * dm_stride + 64 + j].y = dm2[(long long)s * dm2_stride + 64 + j].y;
}

// jsdr_bpsk_create_live_channels, tune -> FFT-acquire on ONE channel: k_seam_hist on the channel geometry.  One block per INPUT:
// the input's raw 26-sample history (kept per input on every call) mixed with that channel's 26 history indices exactly as
// k_chan_front mixes them -- 9-bit indices into sc9, whose entry 256 is (1.0, 1.0): x * 1.0 == x, the pass-through of :395 -- the
// I column into the channel's rows of the FFT state (channel-major: st is the channel's first row), the Q column into the copy
// k_acq_edges_seam reads.  avePeakPower, aveCentreBin and centreBin stay as the channel's last FFT-acquire frame left them.
__global__ __launch_bounds__(32) void k_chan_seam_hist(const int2 *hist, int is_float, const double *sc9, ChanSeamHist sh,
                                                       FftFrontState *st, double *qcol)
{
    const int i = blockIdx.x, t = threadIdx.x;
    if (t < 26) {
        const int2 hv = hist[(long long)i * 32 + t];
        double di, dq;
        if (is_float) {
            di = (double)__int_as_float(hv.x);
            dq = (double)__int_as_float(hv.y);
        } else {
            di = (double)i16_to_float_java((int)(short)(hv.x & 0xffff));
            dq = (double)i16_to_float_java(hv.x >> 16);
        }
        const int k = sh.k9[t];
        di = di * sc9[k];
        dq = dq * sc9[257 + k];
        st[i].hist[t] = di;
        qcol[(long long)i * 26 + t] = dq;
    }
}

// keep the 26 most recent inputs (DC-corrected int16 pair, or the float pair) for the next call
__global__ void k_hist_in(HistArgs a)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    int s = t >> 5, i = t & 31;
    if (s >= a.nstreams || i >= 26) return;
    long long n = a.nsamples - 26 + i;
    int2 v;
    if (n < 0) {
        v = a.hist_old[(long long)s * 32 + (26 + n)];
    } else if (a.rawf) {
        float2 f = a.rawf[(long long)s * a.stride_pairs + n];
        v = make_int2(__float_as_int(f.x), __float_as_int(f.y));
    } else {
        int w = a.raw[(long long)s * a.stride_pairs + n];
        int si = java_short_add((int)(short)(w & 0xffff), a.ic);
        int sq = java_short_add(w >> 16, a.qc);
        v = make_int2((si & 0xffff) | (sq << 16), 0);
    }
    a.hist_new[(long long)s * 32 + i] = v;
}

// The 26-sample input history is kept in the form of the input that produced it (DC-corrected int16 pair in .x, or the
// float pair's bits).  A handle fed through the other form next (receive(float[]) after int16 batches or the other way
// round) gets it converted: int16 -> float is JavaAudio's rule; float -> int16 exists exactly when the float is some
// (float)s/32767f (what IAudioHandler delivers, JavaAudio.java:281-288) -- anything else is reported (bad[0] != 0).
__global__ void k_hist_convert(int2 *hist, int nstreams, int to_float, int *bad)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = t >> 5, i = t & 31;
    if (s >= nstreams || i >= 26) return;
    int2 v = hist[(long long)s * 32 + i];
    if (to_float) {
        const float fi = i16_to_float_java((int)(short)(v.x & 0xffff)), fq = i16_to_float_java(v.x >> 16);
        v = make_int2(__float_as_int(fi), __float_as_int(fq));
    } else {
        const float fi = __int_as_float(v.x), fq = __int_as_float(v.y);
        const int si = (int)rintf(fi * 32767.0f), sq = (int)rintf(fq * 32767.0f);
        const bool ok = si >= -32768 && si <= 32767 && sq >= -32768 && sq <= 32767 && i16_to_float_java(si) == fi &&
                        i16_to_float_java(sq) == fq;
        if (!ok) atomicOr(bad, 1);
        v = make_int2((si & 0xffff) | (sq << 16), 0);
    }
    hist[(long long)s * 32 + i] = v;
}

// =============================================================================================== launchers
// What the handle's call (bpsk_call.hip) starts (bpsk_kernels.h): the grid, the LDS and the template choice of each kernel.

int bpsk_front_upload_constants(const BpskConst &bc)
{
    JSDR_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_bpsk), &bc, sizeof(bc)));
    return JSDR_OK;
}

template <int D, int RD, bool F32IN, bool MIX>
static void launch_front_t(const FrontArgs &fa, int nstreams, long long nds, hipStream_t st)
{
    using G = FrontGeom<D, RD>;
    constexpr int WAVES = 2;
    constexpr size_t elem = F32IN ? sizeof(float2) : sizeof(int);
    const size_t lds = 512 * sizeof(double) + WAVES * ((size_t)G::RAW_EL * elem + G::K_BYTES);
    long long ntiles = (nds + 64 * G::R - 1) / (64 * G::R);
    long long gx = (ntiles + WAVES - 1) / WAVES;
    if (gx > 2048) gx = 2048;
    if (gx < 1) gx = 1;
    (void)ensure_dynamic_lds(reinterpret_cast<const void *>(k_front<D, RD, F32IN, MIX>), lds);
    hipLaunchKernelGGL((k_front<D, RD, F32IN, MIX>), dim3((unsigned)gx, (unsigned)nstreams), dim3(64 * WAVES), lds, st,
                       fa);
}

// one decimation's front end: the register-staged kernel where it applies (lane span RD_REG), the generic one (RD) elsewhere
template <int D, int RD_REG, int RD>
static const char *launch_front_d(const FrontArgs &fa, int nstreams, bool fast, hipStream_t st)
{
    if (launch_front_reg<D, RD_REG>(fa, nstreams, fa.nds, fast, st)) return "k_front_reg";
    if (fa.rawf) {
        if (fa.mix) launch_front_t<D, RD, true, true>(fa, nstreams, fa.nds, st);
        else launch_front_t<D, RD, true, false>(fa, nstreams, fa.nds, st);
    } else {
        if (fa.mix) launch_front_t<D, RD, false, true>(fa, nstreams, fa.nds, st);
        else launch_front_t<D, RD, false, false>(fa, nstreams, fa.nds, st);
    }
    return "k_front";
}

const char *launch_front(const FrontArgs &fa, int decim, int nstreams, bool fast, hipStream_t st)
{
    const char *name = "k_front_any";
    switch (decim) {
        case 4: name = launch_front_d<4, 20, 40>(fa, nstreams, fast, st); break;
        case 5: name = launch_front_d<5, 20, 40>(fa, nstreams, fast, st); break;
        case 10: name = launch_front_d<10, 40, 40>(fa, nstreams, fast, st); break;
        case 20: name = launch_front_d<20, 80, 80>(fa, nstreams, fast, st); break;
        default: {  // any other rate
            long long gx = (fa.nds + 255) / 256;
            if (gx > 4096) gx = 4096;
            if (fa.rawf)
                hipLaunchKernelGGL(k_front_any<true>, dim3((unsigned)gx, (unsigned)nstreams), dim3(256), 0, st, fa, decim);
            else
                hipLaunchKernelGGL(k_front_any<false>, dim3((unsigned)gx, (unsigned)nstreams), dim3(256), 0, st, fa, decim);
        }
    }
    JSDR_LAUNCH_CHECK_NAMED();
    return name;
}

int launch_front_split(const FrontArgs &fa, const unsigned short *ktu9, const double *sc9, int decim, const FftFrontState *dhist,
                       int nstreams, hipStream_t st)
{
    long long gx = (fa.nds + 255) / 256;
    if (gx > 4096) gx = 4096;
    if (fa.rawf)
        hipLaunchKernelGGL(k_front_split<true>, dim3((unsigned)gx, (unsigned)nstreams), dim3(256), 0, st, fa, ktu9, sc9, decim, dhist);
    else
        hipLaunchKernelGGL(k_front_split<false>, dim3((unsigned)gx, (unsigned)nstreams), dim3(256), 0, st, fa, ktu9, sc9, decim, dhist);
    return launched();
}

int launch_seam_hist(const int2 *hist, int is_float, const double *sincos, const SeamHist &sh, FftFrontState *st, FftFrontState *st2,
                     int nstreams, hipStream_t stream)
{
    hipLaunchKernelGGL(k_seam_hist, dim3((unsigned)nstreams), dim3(32), 0, stream, hist, is_float, sincos, sh, st, st2);
    return launched();
}

int launch_seam_q(double2 *dm, long long dm_stride, const double2 *dm2, long long dm2_stride, int J, int nstreams, hipStream_t st)
{
    hipLaunchKernelGGL(k_seam_q, dim3((unsigned)nstreams), dim3(64), 0, st, dm, dm_stride, dm2, dm2_stride, J);
    return launched();
}

int launch_chan_seam_hist(const int2 *hist, int is_float, const double *sc9, const ChanSeamHist &sh, FftFrontState *st, double *qcol,
                          int ninputs, hipStream_t stream)
{
    hipLaunchKernelGGL(k_chan_seam_hist, dim3((unsigned)ninputs), dim3(32), 0, stream, hist, is_float, sc9, sh, st, qcol);
    return launched();
}

int launch_hist_in(const HistArgs &ha, hipStream_t st)
{
    hipLaunchKernelGGL(k_hist_in, dim3((unsigned)((ha.nstreams * 32 + 255) / 256)), dim3(256), 0, st, ha);
    return launched();
}

int launch_hist_convert(int2 *hist, int nstreams, int to_float, int *bad, hipStream_t st)
{
    hipLaunchKernelGGL(k_hist_convert, dim3((unsigned)((nstreams * 32 + 255) / 256)), dim3(256), 0, st, hist, nstreams, to_float, bad);
    return launched();
}

}  // namespace jsdr
