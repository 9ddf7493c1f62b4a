// bpsk.hip -- FUNcubeBPSKDemod.receive() chain for batches of independent streams, exact-order FP64: the device code.
//
// Reference: FUNcubeBPSKDemod.java:357-595 (receive -> doBufferTune -> RxMixTuner -> RxDownSample ->
// RxDemodulate), constants :26-96, tables :159-162.  This translation unit is compiled with
// -ffp-contract=off: every double product and sum is rounded separately, in the reference's order, so
// the slicer bits are bit-identical to the Java arithmetic by construction (tests compare with the
// oracle's restatement).
//
// Pipeline per batch of L input samples x S streams (all on one HIP stream):
//   host        : input-independent schedules (tuner / VCO table indices per sample) in exact double,
//                 cached while the phase state repeats (it is an exact 8-cycle at 12 kHz / 96 kHz) -- bpsk_handle.hip
//   k_front*    : int16 -> float -> double, tuner mix, 27-tap low-pass at the decimated instants
//                 (newest-first order, :479-483), x HOWARD_FUDGE_FACTOR, VCO mix  -> dm[s][64+j]
//                 (k_fm: fused with the matched filter, the default for int16 input with a periodic tuner schedule;
//                 k_front_reg: register-staged lane windows; k_front: generic, float input; bpsk_fft.hip /
//                 bpsk_fftm.hip: FFT-acquire mode)
//   k_matched   : 65-tap matched filter in RING-SLOT order with rotated taps (:519-523) -> y[s][j]=(fi,fq)
//   k_tail      : bit-energy IIRs, peak tracking, differential slicer (:534-593) -> bits
//   k_sync      : 65-symbol sync correlation at stride 80 over the 5200-bit window (:556-560)
//   k_sync_fin  : trigger ordering, dmCorr / dmMaxCorr bookkeeping (:567-572)
//   k_fec_bpsk  : FECDecode of every triggered window (fec.hip)
// DESIGN.md has the lane/LDS mapping of each kernel and its roofline.
//
// All of these kernels stay in this ONE translation unit (they share __constant__ c_bpsk and the build has no relocatable
// device code).  The handle, the host scheduler and the C ABI are in bpsk_handle.hip, which sees this file through
// bpsk_kernels.h: the argument structs and the launch_* functions at the end of this file.
#include "bpsk_kernels.h"
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

namespace jsdr {

__constant__ BpskConst c_bpsk;

#define JSDR_WAVE_SYNC()                                      \
    do {                                                      \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                      \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)


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

// jsdr_bpsk_set_tuning / _set_mode: dmMaxCorr = 0 (:189) in every stream
__global__ void k_reset_maxcorr(TailState *st, int nstreams)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nstreams) st[s].dmMaxCorr = 0;
}

// lane-span geometry of the register-staged front end: a lane owns RD samples = R outputs, its window NS samples
template <int D, int RD>
struct FrontDmaGeom {
    static_assert(RD % D == 0 && RD % 4 == 0, "lane span: whole outputs, whole quads");
    static constexpr int R = RD / D;
    static constexpr int NS = RD - D + 27;
    static constexpr int NSQ = (NS + 3) / 4;
    static constexpr int NT = 64 * RD - D + 27;
};

// ------------------------------------------------------------------------------------------- k_front_reg
// The int16 fast path without an LDS image: lane l of a tile reads ITS OWN window of NS = RD-D+27 samples
// (RD*l .. RD*l+NS-1) straight into registers with 16-byte loads, newest quad first, and walks it while the older
// quads are still in flight (vmcnt counts them down in issue order).  The overlap of neighbouring windows (26
// samples) is served by L1/L2, not by HBM.  Against an LDS image of the tile (round 1's k_front_dma): no LDS but the 4 KB sin/cos table, so occupancy
// is set by registers alone and does not collapse when the side stream's kernels hold LDS on the same CU --
// the LDS-image kernel was latency bound and its time went with 1/occupancy.  Same arithmetic, same order.
// PER: the tuner index is periodic in the sample number with a period that divides the lane span RD (verified by
// the host over every sample of the call): the (cos, sin) pair of window sample m sits at the compile-time offset m
// from a wave-uniform base of an unwrapped table -- scalar loads and SGPR operands instead of the 1 B/sample index
// stream, the per-sample index arithmetic and the LDS lookups.  FAST: fused multiply-add per tap (the
// margin-certified variant).  The samples are converted two at a time on the packed FP32 pipe (fm_convert).
template <int D, int RD, bool MIX, bool DC, bool PER = false, bool FAST = false>
__global__ __launch_bounds__(256) void k_front_reg(FrontArgs a)
{
    using G = FrontDmaGeom<D, RD>;
    constexpr int R = G::R;
    __shared__ double sc[512];
    for (int i = threadIdx.x; i < 512; i += blockDim.x) sc[i] = a.sincos[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int s = blockIdx.y;
    const long long ntiles = (a.nds + 64 * R - 1) / (64 * R);
    const double HOWARD = 0.9 * 32768.0;  // :469
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const int2 *hist = a.hist + (long long)s * 32;
    const int Lm1 = (int)(a.nsamples - 1);
    for (long long tile = (long long)blockIdx.x * nwave + wave; tile < ntiles; tile += (long long)gridDim.x * nwave) {
        const long long j0 = tile * 64 * R;
        const int n0 = a.first_out + (int)(D * j0) - 26 + RD * lane;  // input index of this lane's sample 0
        typedef const __attribute__((address_space(4))) double *const_tab_t;
        const_tab_t tb = nullptr;
        if constexpr (PER && MIX) {  // entry of this wave's sample 0 (RD*lane is a multiple of the period)
            const long long v = (long long)a.first_out + (long long)D * j0;
            const int e0 = __builtin_amdgcn_readfirstlane((int)(((v % a.tper) + a.tper) % a.tper));
            tb = (const_tab_t)(a.tcs + e0);  // tb[2m] = cos, tb[2m+1] = sin
        }
        // ---- this lane's window, newest quad first
        int4 W[G::NSQ];
        unsigned K[G::NSQ];
        const bool inside = n0 >= 0 && n0 + 4 * G::NSQ - 1 <= Lm1;
        if (inside) {
#pragma unroll
            for (int q = G::NSQ - 1; q >= 0; q--) {
                W[q] = *reinterpret_cast<const int4 *>(raw + n0 + 4 * q);  // 4-byte aligned 16-byte load
                if constexpr (!PER) K[q] = *reinterpret_cast<const unsigned *>(a.ktu + 26 + n0 + 4 * q);
            }
        } else {  // first / last window of the call: history before sample 0, clamp beyond the last one
#pragma unroll
            for (int q = G::NSQ - 1; q >= 0; q--) {
                int w[4];
                unsigned k4 = 0;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int n = n0 + 4 * q + t;
                    if (n < 0) {
                        int hw = (n >= -26) ? hist[26 + n].x : 0;
                        if constexpr (DC) {  // stored corrected: undo this call's correction, the walk re-applies it
                            const int si = (int)(short)((hw & 0xffff) - a.ic);
                            const int sq = (int)(short)((hw >> 16) - a.qc);
                            hw = (si & 0xffff) | (sq << 16);
                        }
                        w[t] = hw;
                    } else {
                        w[t] = raw[n > Lm1 ? Lm1 : n];
                    }
                    const int nk = n < -26 ? -26 : (n > Lm1 ? Lm1 : n);
                    if constexpr (!PER) k4 |= (unsigned)a.ktu[26 + nk] << (8 * t);
                }
                W[q] = make_int4(w[0], w[1], w[2], w[3]);
                K[q] = k4;
            }
        }
        // ---- walk from newest to oldest; sin/cos entries one quad ahead (LDS latency)
        double ai[R], aq[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            ai[r] = 0.0;
            aq[r] = 0.0;
        }
        double CS[G::NSQ][8];
        auto load_sc = [&](int q) {
            if constexpr (MIX && !PER) {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int k = (K[q] >> (8 * t)) & 0xff;
                    CS[q][2 * t] = sc[k];
                    CS[q][2 * t + 1] = sc[256 + k];
                }
            }
        };
        load_sc(G::NSQ - 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = G::NSQ - 1; q >= 0; q--) {
            if (q - 1 >= 0) load_sc(q - 1);
            const int4 w4 = W[q];
#pragma unroll
            for (int t = 3; t >= 0; t--) {
                const int m = 4 * q + t;
                if (m < G::NS) {
                    const int w = (t == 0) ? w4.x : (t == 1) ? w4.y : (t == 2) ? w4.z : w4.w;
                    double di, dq;
                    fm_convert(w, a.ic, a.qc, DC, di, dq);
                    if constexpr (MIX) {  // :388-390 component-wise, not a complex multiply
                        if constexpr (PER) {
                            di = di * tb[2 * m];
                            dq = dq * tb[2 * m + 1];
                        } else {
                            di = di * CS[q][2 * t];
                            dq = dq * CS[q][2 * t + 1];
                        }
                    }
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        if (m >= D * r && m <= D * r + 26) {  // sample m has age D*r+26-m in the window of output r
                            const double tp = ds_tap(D * r + 26 - m);
                            if constexpr (FAST) {
                                ai[r] = __builtin_fma(di, tp, ai[r]);
                                aq[r] = __builtin_fma(dq, tp, aq[r]);
                            } else {
                                ai[r] += di * tp;
                                aq[r] += dq * tp;
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) asm volatile("" : "+v"(ai[r]), "+v"(aq[r])::"memory");  // sums are due here
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- x HOWARD_FUDGE_FACTOR (:486), VCO mix (:515-516)
        const long long jl = j0 + (long long)R * lane;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const long long j = jl + r;
            if (j < a.nds) {
                const double oi = ai[r] * HOWARD, oq = aq[r] * HOWARD;
                if (a.ds_dbg) a.ds_dbg[(long long)s * a.nds + j] = make_double2(oi, oq);
                const int kv = a.kvco[j];
                a.dm[(long long)s * a.dm_stride + 64 + j] = make_double2(oi * sc[kv], oq * sc[256 + kv]);
            }
        }
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

// ------------------------------------------------------------------------------------------- k_matched
// 65-tap matched filter, summed in ring-slot order n=0..64 with tap 65-dmPos+n (:519-523).  In time
// terms (g = global index of a 9600 Hz sample, slot(g) = (64-g) mod 65): the window [g-64, g] holds one
// sample s0 with slot 0; the reference adds s0, s0-1, .., g-64 (ages g-s0 .. 64) and then g, g-1, .., s0+1
// (ages 0 .. g-s0-1).  All outputs g = s0+u, u = 0..64, share s0.  Lane l of a workgroup owns the block
// s0 = G + 65 l; wave w computes R consecutive u for all 64 blocks with R accumulators per rail held in
// registers: at every step all lanes need the SAME taps (scalar loads) and one double2 from LDS
// (stride 65 elements -> conflict-free), which is then used 4R times.  Edge steps where an output has
// run out of taps are peeled at compile time, so exactly 65 products are summed per output, in order.

// FAST: one fused multiply-add per tap instead of the reference's separately rounded product and sum (the
// margin-certified variant); the exact-order form is the default everywhere.
template <int R, bool FAST = false>
__device__ __forceinline__ void matched_block(const double2 *xl /* &X[s0] of this lane */, int u0, double (&ai)[R],
                                              double (&aq)[R])
{
    const double *f = c_bpsk.dm_taps;
#pragma unroll
    for (int r = 0; r < R; r++) {
        ai[r] = 0.0;
        aq[r] = 0.0;
    }
    // phase 1: s = s0 - i, ages u+i.  main part: every output still has a tap
    const int n1 = 66 - u0 - R;
    int i = 0;
#ifndef JSDR_MATCHED_NO_CHUNKS
    // eight steps at a time: their 8+R-1 taps come in with one pair of scalar loads and their eight samples with eight
    // LDS reads in flight together -- as a plain loop the compiler reloads all R taps every other step and waits for each
    // load on the spot (lgkmcnt counts scalar loads and LDS reads together).  Same products, same order.
    for (; i + 8 <= n1; i += 8) {
        double tw[8 + R - 1];
#pragma unroll
        for (int k = 0; k < 8 + R - 1; k++) tw[k] = f[u0 + i + k];
        double2 v8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v8[k] = xl[-(i + k)];
#pragma unroll
        for (int k = 0; k < 8; k++) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                if constexpr (FAST) {
                    ai[r] = __builtin_fma(v8[k].x, tw[k + r], ai[r]);
                    aq[r] = __builtin_fma(v8[k].y, tw[k + r], aq[r]);
                } else {
                    ai[r] += v8[k].x * tw[k + r];
                    aq[r] += v8[k].y * tw[k + r];
                }
            }
        }
    }
#endif
    for (; i < n1; i++) {
        double2 v = xl[-i];
#pragma unroll
        for (int r = 0; r < R; r++) {
            double t = f[u0 + i + r];
            if constexpr (FAST) {
                ai[r] = __builtin_fma(v.x, t, ai[r]);
                aq[r] = __builtin_fma(v.y, t, aq[r]);
            } else {
                ai[r] += v.x * t;
                aq[r] += v.y * t;
            }
        }
    }
    // phase 1 tail: outputs drop out from the top (age would exceed 64)
#pragma unroll
    for (int q = 0; q < R - 1; q++) {
        const int i2 = n1 + q;
        double2 v = xl[-i2];
#pragma unroll
        for (int r = 0; r < R - 1 - q; r++) {
            double t = f[u0 + i2 + r];
            if constexpr (FAST) {
                ai[r] = __builtin_fma(v.x, t, ai[r]);
                aq[r] = __builtin_fma(v.y, t, aq[r]);
            } else {
                ai[r] += v.x * t;
                aq[r] += v.y * t;
            }
        }
    }
    // phase 2 head: s = s0 + u0 + R-1-q, only outputs with u >= s-s0 take part, age = u-(s-s0)
#pragma unroll
    for (int q = 0; q < R - 1; q++) {
        double2 v = xl[u0 + R - 1 - q];
#pragma unroll
        for (int r = R - 1 - q; r < R; r++) {
            double t = f[r - (R - 1 - q)];
            if constexpr (FAST) {
                ai[r] = __builtin_fma(v.x, t, ai[r]);
                aq[r] = __builtin_fma(v.y, t, aq[r]);
            } else {
                ai[r] += v.x * t;
                aq[r] += v.y * t;
            }
        }
    }
    // phase 2 main: s = s0 + u0 - m, m = 0..u0-1, age = r + m
    int m = 0;
#ifndef JSDR_MATCHED_NO_CHUNKS
    for (; m + 8 <= u0; m += 8) {
        double tw[8 + R - 1];
#pragma unroll
        for (int k = 0; k < 8 + R - 1; k++) tw[k] = f[m + k];
        double2 v8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v8[k] = xl[u0 - (m + k)];
#pragma unroll
        for (int k = 0; k < 8; k++) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                if constexpr (FAST) {
                    ai[r] = __builtin_fma(v8[k].x, tw[k + r], ai[r]);
                    aq[r] = __builtin_fma(v8[k].y, tw[k + r], aq[r]);
                } else {
                    ai[r] += v8[k].x * tw[k + r];
                    aq[r] += v8[k].y * tw[k + r];
                }
            }
        }
    }
#endif
    for (; m < u0; m++) {
        double2 v = xl[u0 - m];
#pragma unroll
        for (int r = 0; r < R; r++) {
            double t = f[r + m];
            if constexpr (FAST) {
                ai[r] = __builtin_fma(v.x, t, ai[r]);
                aq[r] = __builtin_fma(v.y, t, aq[r]);
            } else {
                ai[r] += v.x * t;
                aq[r] += v.y * t;
            }
        }
    }
}

template <bool FAST>
__global__ __launch_bounds__(512) void k_matched(MatchedArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *X = reinterpret_cast<double2 *>(smem);  // [64 + 4160]: X[i] = sample (G - 64 + i)
    const int s = blockIdx.y;
    const long long G = a.tile0 + 4160LL * blockIdx.x;
    const double2 *dm = a.dm + (long long)s * a.dm_stride;
    {
        // all nine loads of a thread are in flight before the first LDS store: as a plain loop the compiler issues
        // one load, waits for it, stores, and pays the full memory latency nine times per workgroup
        constexpr int NLD = (64 + 4160 + 511) / 512;
        double2 v[NLD];
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            const int i = threadIdx.x + 512 * q;
            const long long rel = (G - 64 + i) - a.g_first;  // index relative to the first new sample
            const bool in = i < 64 + 4160 && rel >= -64 && rel < a.nds;
            // clamped address, masked value: no branch between the loads
            const double2 x = dm[64 + (in ? rel : 0)];
            v[q] = in ? x : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            const int i = threadIdx.x + 512 * q;
            if (i < 64 + 4160) X[i] = v[q];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double2 *xl = X + 64 + 65 * lane;  // &X[s0]
    const long long s0 = G + 65LL * lane;
    double2 *y = a.y + (long long)s * a.y_stride;
    if (wave == 0) {
        double ai[9], aq[9];
        matched_block<9, FAST>(xl, 0, ai, aq);
#pragma unroll
        for (int r = 0; r < 9; r++) {
            long long rel = s0 + r - a.g_first;
            if (rel >= 0 && rel < a.nds) y[rel] = make_double2(ai[r], aq[r]);
        }
    } else {
        const int u0 = 9 + 8 * (wave - 1);
        double ai[8], aq[8];
        matched_block<8, FAST>(xl, u0, ai, aq);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            long long rel = s0 + u0 + r - a.g_first;
            if (rel >= 0 && rel < a.nds) y[rel] = make_double2(ai[r], aq[r]);
        }
    }
}

// keep the last 64 VCO-mixed samples as the next call's history (one wave per stream; loads before stores)
__global__ __launch_bounds__(64) void k_dm_history(double2 *dm, long long dm_stride, long long nds, int nstreams)
{
    int s = blockIdx.x;
    if (s >= nstreams) return;
    double2 *p = dm + (long long)s * dm_stride;
    double2 v = p[nds + threadIdx.x];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    p[threadIdx.x] = v;
}

// ------------------------------------------------------------------------------------------- k_fm
// Front end and matched filter in ONE kernel: int16 IQ -> tuner mix -> 27-tap /D low-pass -> x HOWARD -> VCO mix
// (k_front_reg's arithmetic) -> 65-tap matched filter in ring-slot order (k_matched's) -> y = (fi,fq).  The VCO-mixed
// 9600 Hz samples of a tile never leave the CU: the front half writes them into the LDS image the matched filter
// reads (16 B per 9600 Hz sample that used to go to HBM and come back: 3.4 GB per 1024 x 2^20 batch), and the
// 1 B/sample tuner-index stream is gone as well -- the tuner table index is periodic in the sample number (an
// exact 8-cycle at 12 kHz / 96 kHz; the host verifies the period over every sample of the call), so the (cos, sin)
// pair of window sample m sits at a COMPILE-TIME offset from a tile-uniform base in an unwrapped table: scalar
// loads, SGPR operands, no per-sample index arithmetic and no LDS lookups.
//
//   tile   : NB = 62 blocks of 65 outputs (k_matched's lane = block mapping) + 64 samples of halo = 4094 VCO-mixed
//            samples = 65.5 KB of LDS; 512 threads; two workgroups per CU.
//   front  : 1024 jobs of R = 4 outputs (two rounds of 512 threads, 99.9 % of the lanes busy); a lane reads ITS
//            OWN 57-sample window with 4-byte aligned 16-byte loads, newest quad first, converts I and Q of a
//            sample together (packed FP32: the same IEEE operations as the scalar form, two per instruction) and
//            walks newest -> oldest with the R accumulator pairs in registers (:479-483).  The halo is recomputed
//            (1.6 %); before the call's first sample it comes from the 64 samples the previous call saved.  Windows
//            that reach into the previous call's 26 samples or past the last sample are read from the stream's edge
//            images (k_fm_edges) with the same loads, so every job -- edge or not -- takes the same arithmetic in the
//            same pass; the VCO table indices come in with the window and their table reads are issued under the last
//            quad's arithmetic.
//   matched: as k_matched, from the LDS image.
// (Compile-time timing probes, never defined in the product build (java-sdr_amd/build.py): each of them only REMOVES
// work -- a half of the kernel, a load, a store, a barrier -- and none changes an address that is still accessed; the
// one probe that did (JSDR_X_COAL, round 2) faulted and was deleted.  A probe that needs "wrong data" keeps the
// kernel's own bounds.)
// Where the time goes (2048 streams x 2^20 samples, alone, tools/build_define.sh with -DJSDR_X_NOFRONT / _NOMATCHED /
// _CLK): front half 2.15 ms + matched half 2.12 ms = the kernel's 4.3-4.4 ms; the matched half issues FP64 at ~95 % of
// the chip's measured rate, the front half at ~80 % (1.94 ms with its window loads replaced by constants: the loads'
// latency costs a tenth of it); coalesced window addresses or a register-resident tuner table change nothing.
// Every floating-point operation and its order are those of k_front_reg + k_matched (FAST = false), so (fi,fq)
// stay bit-identical to the reference.  Used when the input is int16, the tuner schedule is periodic with a period
// that divides the lane span (or the tuner is off, tuning <= 0); everything else takes the three-kernel path.

#ifdef JSDR_X_CLK  // timing experiment: s_memtime ticks (10 ns) per phase, summed over every wave of the launch
__device__ unsigned long long g_fm_clk[256][64];  // [blockIdx & 255][phase]: same-address atomics serialise
#define FM_CLK(i)                                                                          \
    do {                                                                                   \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                      \
        clk_acc_[i] += now_ - clk_last_;                                                   \
        clk_last_ = now_;                                                                  \
    } while (0)
#else
#define FM_CLK(i) do {} while (0)
#endif

// The stream's edge images for k_fm: E[0 .. 2*FM_EDGE) = samples -FM_EDGE .. FM_EDGE-1, E[2*FM_EDGE .. 4*FM_EDGE) = samples
// L-FM_EDGE .. L+FM_EDGE-1 as raw int16 pairs: the previous call's 26 samples before sample 0 (kept DC-corrected: the
// correction is taken off again, k_fm's conversion re-applies it -- 16-bit wrap-around both ways, so exactly the stored
// value), zero before them and beyond the last sample.
__global__ void k_fm_edges(EdgeArgs a)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = t / (4 * FM_EDGE), i = t % (4 * FM_EDGE);
    if (s >= a.nstreams) return;
    const int n = i < 2 * FM_EDGE ? i - FM_EDGE : a.nsamples - FM_EDGE + (i - 2 * FM_EDGE);
    int w = 0;
    if (n >= 0 && n < a.nsamples) {
        w = a.raw[(long long)s * a.stride_pairs + n];
    } else if (n < 0 && n >= -26) {
        w = a.hist[(long long)s * 32 + 26 + n].x;
        if (a.dc) {
            const int si = (int)(short)((w & 0xffff) - a.ic);
            const int sq = (int)(short)((w >> 16) - a.qc);
            w = (si & 0xffff) | (sq << 16);
        }
    }
    a.edges[(long long)s * (4 * FM_EDGE) + i] = w;
}

// k_fm_edges and k_hist_in in ONE launch (the k_fm path): both only read the call's input and the previous call's history,
// and write disjoint buffers (the edge images, the next call's history) -- one dependent launch less per call.
// ... and, in the receive() form, the schedule's tables: they travel behind the frame in ONE host->device copy and are put
// where the kernels read them here (two byte ranges at most: the VCO indices and the unwrapped tuner table).
__global__ void k_fm_prep(EdgeArgs e, HistArgs hi, ScatterArgs sc)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int nedge = e.nstreams * 4 * FM_EDGE;
    {
        const int v = t - nedge - 32 * e.nstreams;
        if (v >= 0) {
            if (v < sc.bytes[0]) sc.dst[0][v] = sc.src[0][v];
            else if (v - sc.bytes[0] < sc.bytes[1]) sc.dst[1][v - sc.bytes[0]] = sc.src[1][v - sc.bytes[0]];
            return;
        }
    }
    if (t < nedge) {
        const int s = t / (4 * FM_EDGE), i = t % (4 * FM_EDGE);
        const int n = i < 2 * FM_EDGE ? i - FM_EDGE : e.nsamples - FM_EDGE + (i - 2 * FM_EDGE);
        int w = 0;
        if (n >= 0 && n < e.nsamples) {
            w = e.raw[(long long)s * e.stride_pairs + n];
        } else if (n < 0 && n >= -26) {
            w = e.hist[(long long)s * 32 + 26 + n].x;
            if (e.dc) {
                const int si = (int)(short)((w & 0xffff) - e.ic);
                const int sq = (int)(short)((w >> 16) - e.qc);
                w = (si & 0xffff) | (sq << 16);
            }
        }
        e.edges[(long long)s * (4 * FM_EDGE) + i] = w;
        return;
    }
    // ---- k_hist_in's part (int16 input only on this path)
    const int u = t - nedge;
    const int s = u >> 5, i = u & 31;
    if (s >= hi.nstreams || i >= 26) return;
    const long long n = hi.nsamples - 26 + i;
    int2 v;
    if (n < 0) {
        v = hi.hist_old[(long long)s * 32 + (26 + n)];
    } else {
        const int w = hi.raw[(long long)s * hi.stride_pairs + n];
        const int si = java_short_add((int)(short)(w & 0xffff), hi.ic);
        const int sq = java_short_add(w >> 16, hi.qc);
        v = make_int2((si & 0xffff) | (sq << 16), 0);
    }
    hi.hist_new[(long long)s * 32 + i] = v;
}

// SMALL: the instantiation for SHORT calls (at most FM_THREADS outputs: the receive() form) -- the matched half as one
// output per thread; a kernel of its own so that its loop does not sit in the batch kernel's register allocation (as a
// run-time branch it cost the batch kernel its fourth wave per SIMD: 123 -> 131 VGPRs, 16.8 -> 20.1 ms at 8192 streams)
template <int D, int R, bool MIX, bool DC, bool FAST, bool SMALL = false>
#ifndef JSDR_FM_MINWAVES
#define JSDR_FM_MINWAVES 2
#endif
__global__ __launch_bounds__(FM_THREADS, JSDR_FM_MINWAVES) void k_fm(FmArgs a)
{
    constexpr int RD = D * R, NS = RD - D + 27, NSQ = (NS + 3) / 4;
    constexpr int JOBS = (FM_NT + R - 1) / R, ROUNDS = (JOBS + FM_THREADS - 1) / FM_THREADS;
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *X = reinterpret_cast<double2 *>(smem);                    // [FM_NT]: X[t] = sample G - 64 + t
    double *sc = reinterpret_cast<double *>(smem + FM_NT * sizeof(double2));  // [512]
    for (int i = threadIdx.x; i < 512; i += FM_THREADS) sc[i] = a.sincos[i];
#ifdef JSDR_X_CLK
    unsigned long long clk_acc_[6] = {0, 0, 0, 0, 0, 0}, clk_last_ = 0;
#endif
    const long long nwork = (long long)a.ntiles * a.nstreams;
#pragma unroll 1
    for (long long work = blockIdx.x; work < nwork; work += gridDim.x) {
    const int s = (int)(work / a.ntiles);
    const long long G = a.tile0 + (long long)(65 * FM_NB) * (work % a.ntiles);
    const int jrel0 = (int)(G - 64 - a.g_first);  // call-relative output index of X[0] (negative in the first tile)
#ifdef JSDR_X_FM_SMALLSET  // timing probe (round 5): every stream reads one of 16 streams' samples -- 64 MB, served by the memory-side cache
    const int *raw = a.raw + (long long)(s & 15) * a.stride_pairs;
#else
    const int *raw = a.raw + (long long)s * a.stride_pairs;
#endif
    const int *edges = a.edges + (long long)s * (4 * FM_EDGE);
    const double2 *dmh_old = a.dmh_old + (long long)s * 64;
    const int Lm1 = a.nsamples - 1, nds = a.nds, P = a.tper;
    const double HOWARD = 0.9 * 32768.0;  // :469
    // tile-uniform base into the unwrapped tuner table: window sample m of ANY job of this tile uses entry e0 + m
    // (the lane span RD is a multiple of the period)
    int e0 = 0;
    if constexpr (MIX) {
        const long long v = (long long)a.first_out + (long long)D * jrel0;
        e0 = (int)(((v % P) + P) % P);
    }
    // constant address space: the table is read-only for the launch, and only loads the compiler may assume invariant
    // become scalar loads (a plain global pointer in a kernel that also stores gives 57 vector loads per job)
    typedef const __attribute__((address_space(4))) double *const_tab_t;
    const_tab_t tb = (const_tab_t)(a.tcs + e0);  // tb[2m] = cos, tb[2m+1] = sin
    float amx = 0.0f;  // FAST: largest |sample| this lane converts
    __syncthreads();  // sin/cos table
#ifdef JSDR_X_CLK
    clk_last_ = __builtin_amdgcn_s_memtime();
#endif
    // ================================================================================ front half
#ifdef JSDR_X_NOFRONT
    if (a.nds < 0)
#endif
#pragma unroll 1
    for (int round = 0; round < ROUNDS; round++) {
        const int job = threadIdx.x + FM_THREADS * round;
        const int t0 = R * job;
        if (t0 >= FM_NT) break;
        const int j0 = jrel0 + t0;                   // first output of the job, call relative
        const int n0 = a.first_out + D * j0 - 26;    // its window's first sample
        // `none`: no output of the job is filtered here (the halo before output 0, slots past the call's last output).
        // Every other job takes the same arithmetic in the same pass.  A window that reaches back into the previous
        // call's 26 samples, or past the last sample, is read from the stream's EDGE IMAGE instead of the input -- 256
        // samples around sample 0 (history, then input) and 256 around the last one (zero beyond), laid out by
        // k_fm_edges before this kernel -- with the same fifteen loads; outputs that are not this call's (a job that
        // straddles output 0 or the last output) are replaced at the store.  (These jobs used to run a
        // one-output-at-a-time loop of dependent loads after the others had finished: one of them held its workgroup
        // for longer than a whole regular tile takes.  The tile's last job, which owns fewer than R image slots when R
        // does not divide FM_NT, drops the surplus at the store -- on the old edge path it cost every tile ~7 us.)
        const bool none = j0 + R <= 0 || j0 >= nds || nds <= 0;
        const bool regular = j0 >= 0 && j0 + R <= nds;
        if (!none) {
            int4 W[NSQ];
            const int *wp = raw + n0;
            if (n0 < 0) wp = edges + (n0 + FM_EDGE);
            else if (n0 + 4 * NSQ - 1 > Lm1) wp = edges + 2 * FM_EDGE + (n0 - (a.nsamples - FM_EDGE));
            // the VCO table indices of the job's outputs come in WITH the window: left where they are used, after the
            // last quad, the load was issued there and waited for on the spot -- a full memory latency at the end of
            // every round (nothing may cross the quads' scheduling barriers, so the source order decides)
            unsigned kv4[(R + 3) / 4];  // R byte indices, four to a register
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
#pragma unroll
            for (int q = NSQ - 1; q >= 0; q--) W[q] = *reinterpret_cast<const int4 *>(wp + 4 * q);
#ifndef JSDR_FM_NOPIN
            __builtin_amdgcn_sched_barrier(0);
#endif
            double ai[R], aq[R];
            double vc[R], vs[R];  // the outputs' VCO (cos, sin): LDS reads issued under the last quad's arithmetic
#pragma unroll
            for (int r = 0; r < R; r++) {
                ai[r] = 0.0;
                aq[r] = 0.0;
            }
#pragma unroll
            for (int q = NSQ - 1; q >= 0; q--) {
                const int4 w4 = W[q];
                if (q == 0) {
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const int kv = (kv4[r / 4] >> (8 * (r % 4))) & 0xff;
                        vc[r] = sc[kv];
                        vs[r] = sc[256 + kv];
                    }
                }
#pragma unroll
                for (int t = 3; t >= 0; t--) {
                    const int m = 4 * q + t;
                    if (m < NS) {
                        const int w = (t == 0) ? w4.x : (t == 1) ? w4.y : (t == 2) ? w4.z : w4.w;
                        double di, dq;
                        fm_convert(w, a.ic, a.qc, DC, di, dq, FAST ? &amx : nullptr);
                        if constexpr (MIX) {  // :388-390 component-wise, not a complex multiply
                            di = di * tb[2 * m];
                            dq = dq * tb[2 * m + 1];
                        }
#pragma unroll
                        for (int r = 0; r < R; r++) {
                            if (m >= D * r && m <= D * r + 26) {  // age D*r+26-m in the window of output r
                                const double tp = ds_tap(D * r + 26 - m);
                                if constexpr (FAST) {
                                    ai[r] = __builtin_fma(di, tp, ai[r]);
                                    aq[r] = __builtin_fma(dq, tp, aq[r]);
                                } else {
                                    ai[r] += di * tp;
                                    aq[r] += dq * tp;
                                }
                            }
                        }
                    }
                }
#ifndef JSDR_FM_NOPIN
#pragma unroll
                for (int r = 0; r < R; r++) asm volatile("" : "+v"(ai[r]), "+v"(aq[r])::"memory");  // sums are due here
                if constexpr (FAST) asm volatile("" : "+v"(amx));  // (or the maxima sink to the end of the round with all 114 floats alive)
                __builtin_amdgcn_sched_barrier(0);
#endif
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
    if constexpr (FAST) {  // non-negative floats order like their bit patterns
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) amx = fmaxf(amx, __shfl_xor(amx, off, 64));
        if ((threadIdx.x & 63) == 0 && amx > 0.0f) atomicMax(a.amax + s, __float_as_int(amx));
    }
    FM_CLK(1);  // front half
    __syncthreads();
    FM_CLK(3);  // barrier after the front half
    // ---- the call's last 64 VCO-mixed samples are the next call's halo; every sample is owned by one tile
    if (jrel0 + FM_NT > nds - 64) {  // uniform
        double2 *dmh_new = a.dmh_new + (long long)s * 64;
        for (int t = 64 + threadIdx.x; t < FM_NT; t += FM_THREADS) {
            const int j = jrel0 + t;
            if (j >= nds - 64 && j < nds && j >= 0) dmh_new[j - (nds - 64)] = X[t];
        }
        if (work % a.ntiles == 0 && nds < 64 && (int)threadIdx.x < 64 - nds) dmh_new[threadIdx.x] = dmh_old[threadIdx.x + nds];
    }
    // ================================================================================ matched filter
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int blk = lane < FM_NB ? lane : FM_NB - 1;  // lanes 62, 63 shadow block 61 and store nothing
    const double2 *xl = X + 64 + 65 * blk;            // &X[s0]
    const int rel0 = jrel0 + 64 + 65 * blk;           // call-relative index of s0
    double2 *y = a.y + (long long)s * a.y_stride;
    if constexpr (SMALL) {
        // A SHORT call (the receive() form: 205 outputs of a 2048-sample frame): one output per thread, the reference's
        // ring-slot order (:519-523) as a per-thread loop over the image -- (s0, s0-1, .., g-64) then (g, .., s0+1) with
        // s0 = g - u the sample in ring slot 0 -- instead of the lane-per-block mapping, whose eight waves each walk all
        // 65 taps for 62 blocks of which a short call fills four (19 us of a 70 us receive).  Same operands, same order:
        // the same doubles (this is tail_exact_sample's second half).
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
                if constexpr (FAST) {
                    yi = __builtin_fma(x.x, tp, yi);
                    yq = __builtin_fma(x.y, tp, yq);
                } else {
                    yi += x.x * tp;
                    yq += x.y * tp;
                }
            }
            for (int m = 0; m < u; m++) {        // g, g-1, .., s0+1: ages 0 .. u-1
                const double2 x = xg[-m];
                const double tp = f[m];
                if constexpr (FAST) {
                    yi = __builtin_fma(x.x, tp, yi);
                    yq = __builtin_fma(x.y, tp, yq);
                } else {
                    yi += x.x * tp;
                    yq += x.y * tp;
                }
            }
            y[rel] = make_double2(yi, yq);
        }
    } else {
#ifdef JSDR_X_NOMATCHED
    if (a.nds < 0)
#endif
#ifndef JSDR_FM_DIRECT_STORE  // (the old lane-strided stores: 17.08 vs 16.86 ms at 8192 streams, one session)
    // The tile's 65 * FM_NB outputs leave through the image, which is dead once every wave has walked its blocks: a lane's
    // outputs go to LDS at its block's stride (65 slots: conflict-free), and the workgroup then stores the tile's outputs
    // -- contiguous in y -- as fully coalesced 16-byte accesses, instead of one 16-byte store per lane at a 1040-byte stride
    {
        double ai[9], aq[9];
        int u0 = 0, nout = 9;
        if (wave == 0) {
            matched_block<9, FAST>(xl, 0, ai, aq);
        } else {
            u0 = 9 + 8 * (wave - 1);
            nout = 8;
            double bi[8], bq[8];
            matched_block<8, FAST>(xl, u0, bi, bq);
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
#else
    if (wave == 0) {
        double ai[9], aq[9];
        matched_block<9, FAST>(xl, 0, ai, aq);
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int rel = rel0 + r;
            if (lane < FM_NB && rel >= 0 && rel < nds) y[rel] = make_double2(ai[r], aq[r]);
        }
    } else {
        const int u0 = 9 + 8 * (wave - 1);
        double ai[8], aq[8];
        matched_block<8, FAST>(xl, u0, ai, aq);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int rel = rel0 + u0 + r;
            if (lane < FM_NB && rel >= 0 && rel < nds) y[rel] = make_double2(ai[r], aq[r]);
        }
    }
#endif
    }
    FM_CLK(4);  // matched half
    __syncthreads();  // the next work item reuses the image
    FM_CLK(5);  // barrier after the matched half
    }
#ifdef JSDR_X_CLK
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < 6; i++) atomicAdd(&g_fm_clk[blockIdx.x & 255][(threadIdx.x >> 6) * 8 + i], clk_acc_[i]);
#endif
}

// ------------------------------------------------------------------------------------------- k_tail
// One wave per stream, the 9600 Hz tail (:534-593) in chunks of 64 bit periods (512 samples).
// The bit clock is input independent and exactly periodic (bitPos == g mod 8, a new peak is measured
// after every g == 7 mod 8; verified on the host at create time).  The only truly serial arithmetic is
// the nine first-order IIRs (eight dmEnergy channels :535, dmEnergyOut :538); everything else is taken
// out of their loop:
//   parallel : coalesced load of the chunk (prefetched one chunk ahead), energy1 = fi*fi+fq*fq     (:534)
//   serial   : 64 steps; lanes 0..7 advance dmEnergy[lane], lane 8 advances dmEnergyOut SPECULATING that
//              the peak position stays where it is (decision point = bitPos v in every period)
//   parallel : lane = period: first-maximum argmax of the eight energies after that period (:586-592)
//   check    : if every new peak equals v the speculation held (the steady state of a locked demodulator):
//              decision points are (period, v).  Otherwise (rare: acquisition, fades) the chunk is replayed
//              by the scalar state machine of :537,:577-579 and dmEnergyOut is recomputed from its saved value
//   parallel : lane = decision: differential detector, sqrt, threshold, bit (:539-545), ordered compaction

// (fi,fq) of the 9600 Hz sample g in EXACT order, by the whole wave, from the call's raw input: the 65 VCO-mixed samples
// g-64..g (27-tap low-pass each, :479-483, one per lane) through LDS, then the 65 products in ring-slot order (:519-523).
// The cold path of the fast variant: only samples whose 65-sample window lies inside this call (j0 >= 7, checked by the
// caller, keeps every input index >= 0).
__device__ __forceinline__ double2 tail_exact_sample(const TailArgs &a, int s, long long g, double2 *dmL, int lane)
{
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const double HOWARD = 0.9 * 32768.0;
    const bool dc = (a.ic != 0) || (a.qc != 0);
    for (int i = lane; i < 65; i += 64) {
        const long long j = g - 64 + i - a.g_first;  // call-relative index of the decimated sample
        double fi = 0.0, fq = 0.0;
        for (int age = 0; age < 27; age++) {
            const long long n = (long long)a.first_out + (long long)a.decim * j - age;
            double di, dq;
            fm_convert(raw[n], a.ic, a.qc, dc, di, dq);
            if (a.mix) {
                const double2 cs = a.tcs[(int)((n + 26) % a.tper)];
                di = di * cs.x;
                dq = dq * cs.y;
            }
            const double tp = c_bpsk.ds_taps[age];
            fi += di * tp;
            fq += dq * tp;
        }
        const double oi = fi * HOWARD, oq = fq * HOWARD;
        const int kv = a.kvco[j];
        dmL[i] = make_double2(oi * a.sincos[kv], oq * a.sincos[256 + kv]);
    }
    JSDR_WAVE_SYNC();
    const int u = (int)(((g - 64) % 65 + 65) % 65);  // g = s0 + u, s0 the sample in ring slot 0
    const double *f = c_bpsk.dm_taps;
    double yi = 0.0, yq = 0.0;
    for (int i = 0; i <= 64 - u; i++) {  // s0, s0-1, .., g-64: ages u .. 64
        const double2 x = dmL[64 - u - i];
        yi += x.x * f[u + i];
        yq += x.y * f[u + i];
    }
    for (int m = 0; m < u; m++) {        // g, g-1, .., s0+1: ages 0 .. u-1
        const double2 x = dmL[64 - m];
        yi += x.x * f[m];
        yq += x.y * f[m];
    }
    JSDR_WAVE_SYNC();
    return make_double2(yi, yq);
}

#ifdef JSDR_X_T8CLK  // timing experiment: s_memtime ticks per phase, summed over every wave of every launch
__device__ unsigned long long g_t8_clk[8];
#define T8_CLK(i)                                                     \
    do {                                                              \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        t8acc_[i] += now_ - t8last_;                                  \
        t8last_ = now_;                                               \
    } while (0)
#else
#define T8_CLK(i) do {} while (0)
#endif
// CERT = the fast variant's tail: the same arithmetic on (fi,fq) that carry a bounded error |d| <= ey, plus, for every
// data-dependent decision, a margin that covers the worst case of that error (DESIGN.md "fast variant"):
//   argmax of the eight smoothed energies (:586-592): certified when the winner leads by more than twice the bound on
//     an energy's error; otherwise the stream is marked uncertified (the IIR state cannot be redone locally)
//   energy2 > 100 (:544) and di < 0 (:545): when inside the margin, the two (fi,fq) samples of the detector are
//     recomputed from the raw input in exact order and the decision is taken on those
template <bool CERT>
__global__ __launch_bounds__(64) void k_tail(TailArgs a)
{
    // (fi,fq) of the chunk's 64 samples at the bit position the peak tracker holds when the chunk starts -- the
    // differential detector's inputs while the demodulator is locked; a decision anywhere else (acquisition, a moving
    // peak) reads its sample from y.  The whole chunk (8 KB) used to sit here: with 10 KB instead of 17 KB a CU holds
    // sixteen of these one-wave workgroups instead of nine, and the kernel is occupancy x latency bound.
    __shared__ double2 ydL[64];        // [period]
    // The exact kernel serves handles of fewer than 2048 streams since round 4 (k_tail8 takes the others): a wave per SIMD at
    // most, so LDS no longer decides how many of these workgroups a CU holds -- the whole chunk's (fi,fq) stay here for the
    // decisions that fall on another bit position (acquisition, fades, the FFT-acquire mode's frame seams) instead of being
    // read again from y (two dependent L2 round trips per chunk: with the serial state machine below, 27 us a chunk unlocked
    // against 3 us locked).  The fast variant's tail (CERT) runs at 8192 streams and keeps the small footprint.
    constexpr bool ALLY = !CERT;
    __shared__ double2 yAll[ALLY ? 512 : 1];
    // The chains' work area, in place and ROW PER CHAIN: before the chain, row c < 8 holds the inputs of dmEnergy[c] --
    // energy1 x 1/200 of the sample at bit position c of every period (the products are taken lane-parallel when the chunk
    // is staged, not by the nine chain lanes one at a time) -- and row 8 energy1 x 1/800 of the sample at position v, for
    // dmEnergyOut; afterwards dmEnergy[c] after every period (a chain has the inputs of its next eight links in registers
    // before it overwrites them).  A chain lane reads and writes ITS row two periods per LDS instruction: the kernel is
    // bound by the number of LDS instructions its twenty waves per CU issue (SQ counters: half of a wave's life spent
    // waiting on lgkmcnt), and one 8-byte access per link in each direction was most of them.  6 KB a workgroup.
    __shared__ __align__(16) double eT[9][72];  // [chain][period]; 72: rows 16-byte aligned, two-way conflicts at worst
    __shared__ unsigned char maskL[64];
    __shared__ short declist[136];
    __shared__ double2 dmL[CERT ? 66 : 1];
    const int lane = threadIdx.x;
    const int s = blockIdx.x;
    if (s >= a.nstreams) return;
#ifdef JSDR_X_T8CLK
    unsigned long long t8acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t8last_ = __builtin_amdgcn_s_memtime();
#endif
    TailState *sp = &a.st[s];
    double emax = CERT ? sp->emax : 0.0;
    long long last_g = CERT ? sp->last_g : -1;
    int uncert = 0;
    long long redone = 0;
    const double2 *y = a.y + (long long)s * a.y_stride;
    signed char *blog = a.bitlog_new + (long long)s * a.bitlog_stride;
    const int nbits_prev = sp->nbits_prev;
    const int cntBit0 = sp->cntBit;
    // carry the 5200-bit shift register (dmFECCorr, :503) over from the previous call's log
    {
        // (the source is byte aligned only; 82 byte loads per lane, in two batches kept in flight together -- a
        // load / wait / store loop would pay the memory latency 82 times before the first chunk starts)
        const signed char *old = a.bitlog_old + (long long)s * a.bitlog_stride + nbits_prev;
        constexpr int NQ = (HIST_BITS + 63) / 64, HALF = (NQ + 1) / 2;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            signed char t[HALF];
#pragma unroll
            for (int q = 0; q < HALF; q++) {
                const int i = lane + 64 * (h * HALF + q);
                t[q] = old[i < HIST_BITS ? i : HIST_BITS - 1];
            }
#pragma unroll
            for (int q = 0; q < HALF; q++) {
                const int i = lane + 64 * (h * HALF + q);
                if (i < HIST_BITS) blog[i] = t[q];
            }
        }
    }
    const double K1 = 1.0 - 1.0 / 200.0, S1 = 1.0 / 200.0;  // BIT_SMOOTH1 (:89)
    const double K2 = 1.0 - 1.0 / 800.0, S2 = 1.0 / 800.0;  // BIT_SMOOTH2 (:90)
    // lanes 0..7 carry dmEnergy[lane], lane 8 carries dmEnergyOut
    double e = (lane < 8) ? sp->dmEnergy[lane] : sp->dmEnergyOut;
    const double Kc = (lane < 8) ? K1 : K2;
    int peakPos = __builtin_amdgcn_readfirstlane(sp->peakPos);
    int newPeak = __builtin_amdgcn_readfirstlane(sp->newPeak);
    double lastI = sp->lastI, lastQ = sp->lastQ, energy1 = sp->energy1, energy2 = sp->energy2;
    int nbits = 0;
    const long long g_first = a.g_first, g_end = a.g_first + a.nds;
    const long long M_first = g_first >> 3, M_last = (g_end - 1) >> 3;

    double2 pre[8];
    auto fetch = [&](long long MB) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            long long g = 8 * MB + k * 64 + lane;
            pre[k] = (g >= g_first && g < g_end) ? y[g - g_first] : make_double2(0.0, 0.0);
        }
    };
    if (a.nds > 0) fetch(M_first);

    for (long long MB = M_first; MB <= M_last && a.nds > 0; MB += 64) {
        // ---------------- stage the prefetched chunk, start fetching the next one
        const int v = peakPos;
#pragma unroll
        for (int k = 0; k < 8; k++) {  // sample k*64 + lane = period k*8 + lane/8, position lane%8
            const double en = pre[k].x * pre[k].x + pre[k].y * pre[k].y;  // :534
            if constexpr (ALLY) yAll[k * 64 + lane] = pre[k];
            eT[lane & 7][k * 8 + (lane >> 3)] = en * S1;
            if ((lane & 7) == v) {
                ydL[k * 8 + (lane >> 3)] = pre[k];
                eT[8][k * 8 + (lane >> 3)] = en * S2;
            }
        }
        JSDR_WAVE_SYNC();
        const double2 *ychunk = y + (8 * MB - g_first);  // sample i of the chunk (only in-range samples are ever decisions)
        auto ysample = [&](int pos) {
            if constexpr (ALLY) return yAll[pos];
            else return (pos & 7) == v ? ydL[pos >> 3] : ychunk[pos];
        };
        double m_en = 0.0, m_d = 0.0, m_e2 = 0.0;  // this chunk's margins
        if constexpr (CERT) {
            double em = 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const double en = pre[k].x * pre[k].x + pre[k].y * pre[k].y;
                em = en > em ? en : em;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double o = __shfl_xor(em, off, 64);
                em = o > em ? o : em;
            }
            emax = em > emax ? em : emax;
            // |fi|,|fq| <= sqrt(emax); u = 2^-53.  energy1: 2 sqrt2 sqrt(emax) ey + 7 u emax; through the IIR (gain 1, 3
            // roundings a link, 1/(1-K) = 200 links deep): + 1200 u emax.  di, dq: 4 sqrt(emax) ey + 7 u emax.
            // (all linear in the input: the full-scale bound ey shrinks with the stream's largest sample so far)
            const double sq = sqrt(emax), U = 1.1102230246251565e-16;
            const double eys = a.ey * ((double)__int_as_float(a.amax[s]) * (1.0000001 / 32767.0));
            m_en = a.argmax_scale * 2.0 * (2.83 * sq * eys + 2.0 * eys * eys + 1207.0 * U * emax);
            m_d = a.margin_scale * (4.1 * sq * eys + 2.0 * eys * eys + 7.0 * U * emax);
            m_e2 = 1.5 * m_d + (m_d > 0.0 ? 4.0e-14 : 0.0);
        }
        if (MB + 64 <= M_last) fetch(MB + 64);
        const int nper = (int)((M_last - MB + 1) < 64 ? (M_last - MB + 1) : 64);
        const bool interior = (8 * MB >= g_first) && (8 * (MB + 64) <= g_end);  // every sample of all 64 periods is in range (uniform)
        T8_CLK(0);  // staging
        // ---------------- serial IIRs, speculating that the peak position stays at v
        const bool spec = (newPeak == peakPos);
        const double e_in = e;
        {
            const int idx = (lane < 8) ? lane : v;
            const int col = (lane < 8) ? lane : 8;
            const long long glane = 8 * MB + idx;
            const bool lane_iir = lane < 8, lane_out = (lane == 8) && spec;
            const bool lane_on = lane_iir || lane_out;
            // the 64 energies this lane will fold in, fetched up front: the serial chain below then touches
            // registers only (an LDS read per step would put ~100 cycles of latency on every link of the chain)
#ifndef JSDR_TAIL_XS
#define JSDR_TAIL_XS 8
#endif
            // (a few at a time: the preload is 16 VGPRs instead of 128 -- at 8192 streams the tail is occupancy x latency
            //  bound, and what counts is how many of these one-wave workgroups a CU holds)
            constexpr int XS = JSDR_TAIL_XS;
            const int pfirst = (glane < g_first) ? 1 : 0;  // period 0 of the chunk lacks this lane's sample
#pragma unroll
            for (int p0 = 0; p0 < 64; p0 += XS) {
                double xs[XS];
#pragma unroll
                for (int p = 0; p < XS; p += 2) {  // (the x S products were taken at staging)
                    const double2 x2 = *reinterpret_cast<const double2 *>(&eT[col][p0 + p]);
                    xs[p] = x2.x;
                    xs[p + 1] = x2.y;
                }
                // (pinned: left to itself the compiler sinks the reads back into the chain, one LDS wait per two steps)
#pragma unroll
                for (int p = 0; p < XS; p++) asm volatile("" : "+v"(xs[p]));
                // only the first and the last period of a call can be partial; everywhere else, with the peak position
                // settled (the locked demodulator), a link of the chain is one multiply and one add.  The energies go to
                // LDS as they fall out (stores are not on the chain; a register copy of all 64 would double the kernel's
                // footprint beside the kernels it overlaps with).
                if (interior && spec) {
                    // lanes 0..8 only, under ONE exec mask for the whole chain (a mask per store costs an exec write and
                    // its hazard on every link); lane 8 (dmEnergyOut) stores into the rows' pad column, which nobody reads
                    if (lane <= 8) {
#pragma unroll
                        for (int p = 0; p < XS; p += 2) {
                            const double e0 = (e * Kc) + xs[p];  // :535 / :538
                            e = (e0 * Kc) + xs[p + 1];
                            *reinterpret_cast<double2 *>(&eT[lane][p0 + p]) = make_double2(e0, e);
                        }
                    }
                } else {
#pragma unroll
                    for (int p = 0; p < XS; p++) {
                        const double ne = (e * Kc) + xs[p];
                        const bool ok = lane_on && (p0 + p >= pfirst) && (glane + 8 * (p0 + p) < g_end);
                        if (ok) e = ne;
                        if (lane_iir) eT[lane][p0 + p] = e;
                    }
                }
            }
        }
        JSDR_WAVE_SYNC();
        T8_CLK(1);  // chains
        // ---------------- new peak after every period whose last sample (bitPos 7) is in range (:582-593)
        int np = -1;
        if (lane < nper) {
            const long long g7 = 8 * (MB + lane) + 7;
            if (g7 >= g_first && g7 < g_end) {
                double bv = eT[0][lane], sv = -1.0e300;
                np = 0;
#pragma unroll
                for (int c = 1; c < 8; c++) {
                    double ov = eT[c][lane];
                    if (ov > bv) {  // strict: the first maximum wins
                        sv = bv;
                        bv = ov;
                        np = c;
                    } else if (CERT && ov > sv) {
                        sv = ov;
                    }
                }
                if constexpr (CERT) {
                    // (m_en == 0: nothing but zeros has gone through the fast kernels, both variants hold the same numbers)
                    if (!(bv - sv > m_en) && m_en > 0.0) uncert = 1;  // the order of the two largest is not certain
                }
            }
        }
        T8_CLK(2);  // argmax
        bool replay = false;
        const bool bad = (np >= 0) && (np != v);
        const bool held = spec && (__ballot(bad) == 0ull);
        // A locked stream away from the call's edges: every period has its one decision at bit position v, in period
        // order -- the decision list is known without the mask / prefix-sum / list round trips through LDS.
        const bool fastd = held && interior;
        int nd = 64;
        if (!fastd) {
            if (held) {
                if (lane < nper) {
                    const long long g = 8 * (MB + lane) + v;
                    maskL[lane] = (g >= g_first && g < g_end) ? (unsigned char)(1 << v) : (unsigned char)0;
                }
                // peakPos stays v; every measured peak was v, so newPeak stays v as well
            } else {
                // The peak moved (acquisition, fades, frame seams of the FFT-acquire mode).  The peakPos/newPeak
                // machine of :537,:577-579,:592 is integer only -- its inputs are the per-period argmax values np,
                // which do not depend on dmEnergyOut -- so it runs as scalar code over the periods, one mask per
                // period; dmEnergyOut is then redone from its saved value along the decision list further down.
                // Walking the bit positions cfirst..clast of a period: a decision where c == peakPos (:537); at c ==
                // (peakPos+4)&7 peakPos = newPeak (dmHalfTable, :500,:577-578), after which a second decision can fall at the NEW
                // peakPos if that position is still to come.  In closed form (k_tail8's; branch-free, scalar).
                // Away from the call's edges every period is whole and measured, and then the machine is not serial at all:
                // whenever peakPos != newPeak the switch position (peakPos+4)&7 lies inside the period, so peakPos leaves every
                // period equal to the newPeak it entered with, which is the peak measured one period earlier --
                //     newPeak(p) = np[p-1],  peakPos(p) = np[p-2]   (the chunk's first two periods take the carried state)
                // and each lane writes down its own period's decisions (the scalar walk over 64 periods was most of the 27 us an
                // unlocked chunk took, against 3 us for a locked one).
                int mymask_r = 0;
                if (interior) {
                    const int up1 = __shfl_up(np, 1, 64), up2 = __shfl_up(np, 2, 64);
                    const int nwv = lane == 0 ? newPeak : up1;
                    const int pkv = lane == 0 ? peakPos : (lane == 1 ? newPeak : up2);
                    const int h = (pkv + 4) & 7;
                    const bool diff = pkv != nwv;
                    const bool d1 = !(diff && h < pkv);
                    const bool d2 = diff && nwv > h;
                    mymask_r = (d1 ? 1 << pkv : 0) | (d2 ? 1 << nwv : 0);
                    peakPos = __builtin_amdgcn_readlane(np, 62);
                    newPeak = __builtin_amdgcn_readlane(np, 63);
                } else
                for (int p = 0; p < nper; p++) {
                    const long long gbase = 8 * (MB + p);
                    const int cfirst = (gbase < g_first) ? (int)(g_first - gbase) : 0;
                    const int clast = (gbase + 7 >= g_end) ? (int)(g_end - 1 - gbase) : 7;
                    const int h = (peakPos + 4) & 7;
                    const bool pin = peakPos >= cfirst && peakPos <= clast;
                    const bool hin = h >= cfirst && h <= clast && peakPos != newPeak;
                    const bool d1 = pin && !(hin && h < peakPos);  // the old peakPos decides unless the switch came first
                    const bool d2 = hin && newPeak > h && newPeak <= clast;
                    const int mask = (d1 ? 1 << peakPos : 0) | (d2 ? 1 << newPeak : 0);
                    peakPos = hin ? newPeak : peakPos;
                    if (lane == p) mymask_r = mask;
                    if (clast == 7) newPeak = __builtin_amdgcn_readlane(np, p);
                }
                if (lane < 64) maskL[lane] = (unsigned char)mymask_r;
                replay = true;
            }
            JSDR_WAVE_SYNC();
            // ---------------- decision list of the chunk, in time order
            const int mymask = (lane < nper) ? (int)maskL[lane] : 0;
            const int mycnt = __popc(mymask);
            // inclusive prefix sum over lanes: a period holds at most two decisions, so two ballots count them (six dependent
            // cross-lane adds before)
            const unsigned long long b1 = __ballot(mycnt >= 1), b2 = __ballot(mycnt >= 2);
            const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
            const int pre_sum = __popcll(b1 & upto) + __popcll(b2 & upto);
            nd = __popcll(b1) + __popcll(b2);
            {
                int pos = pre_sum - mycnt;
                int m = mymask;
                while (m) {
                    int c = __ffs(m) - 1;
                    m &= m - 1;
                    declist[pos++] = (short)(lane * 8 + c);
                }
            }
            JSDR_WAVE_SYNC();
            if (replay) {
                // dmEnergyOut (:538) over the decisions in time order: the products x*S2 lane-parallel, the chain
                // e = e*K2 + (x*S2) on broadcast values, in the reference's operation order
                double xa = 0.0, xb = 0.0;
                auto en_of = [&](int pos) {  // energy1 of the chunk's sample pos, as :534 forms it
                    const double2 q = ysample(pos);
                    return q.x * q.x + q.y * q.y;
                };
                if (lane < nd) xa = en_of(declist[lane]) * S2;
                if (lane + 64 < nd) xb = en_of(declist[lane + 64]) * S2;
                double eo = __shfl(e_in, 8, 64);
                // (lane indices as constants, sixteen links per uniform test: as a counted loop every link paid the hazards
                //  of a lane select in an SGPR and a branch)
                auto chain = [&](double xs, int cnt) {
#pragma unroll 1
                    for (int d0 = 0; d0 < 64; d0 += 16) {
                        if (d0 >= cnt) break;
#pragma unroll
                        for (int u = 0; u < 16; u++) {
                            const int lo = __builtin_amdgcn_readlane(__double2loint(xs), u);
                            const int hi = __builtin_amdgcn_readlane(__double2hiint(xs), u);
                            const double ne = (eo * K2) + __hiloint2double(hi, lo);
                            eo = (d0 + u < cnt) ? ne : eo;
                        }
                        // the next sixteen inputs move down to lanes 0..15
                        xs = __hiloint2double(__shfl_down(__double2hiint(xs), 16, 64), __shfl_down(__double2loint(xs), 16, 64));
                    }
                };
                chain(xa, nd < 64 ? nd : 64);
                if (nd > 64) chain(xb, nd - 64);
                if (lane == 8) e = eo;
            }
        }
        T8_CLK(3);  // machine, list, replay
        // ---------------- parallel: differential detector per decision (:539-545)
        for (int d0 = 0; d0 < nd; d0 += 64) {
            const int d = d0 + lane;
            const bool have = d < nd;
            double2 cur = make_double2(0.0, 0.0), prv = make_double2(lastI, lastQ);
            if (have) {
                cur = fastd ? ydL[d] : ysample((int)declist[d]);
                if (d > 0) prv = fastd ? ydL[d - 1] : ysample((int)declist[d - 1]);
            }
            double di = -((prv.x * cur.x) + (prv.y * cur.y));
            double dq = (prv.x * cur.y) - (prv.y * cur.x);
            double e2 = sqrt((di * di) + (dq * dq));
            if constexpr (CERT) {
                const bool unsure = have && (fabs(e2 - 100.0) <= m_e2 || (e2 > 100.0 && fabs(di) <= m_d));
                unsigned long long um = __ballot(unsure);
                if (um) {  // cold: redo those decisions on (fi,fq) recomputed from the raw input in exact order
                    const int ci = have ? (fastd ? 8 * d + v : (int)declist[d]) : 0;
                    const int pi = (have && d > 0) ? (fastd ? 8 * (d - 1) + v : (int)declist[d - 1]) : -1;
                    while (um) {
                        const int L = __ffsll((long long)um) - 1;
                        um &= um - 1ull;
                        const long long gc = 8 * MB + __shfl(ci, L, 64);
                        const int pl = __shfl(pi, L, 64);
                        const long long gp = pl >= 0 ? 8 * MB + pl : last_g;
                        // both windows (65 VCO-mixed samples of 27 inputs each) must lie inside this call
                        const bool can = gp >= 0 && gp - 64 - a.g_first >= 7 && gc - 64 - a.g_first >= 7 && gc < a.g_first + a.nds &&
                                         (a.mix == 0 || a.tper > 0);
                        if (!can) {
                            // (the first samples of a call reach back into the previous one) not recomputable: the decision
                            // stands if it clears the margin proper -- margin_scale only widens what is sent to the redo
                            const double e2L = __shfl(e2, L, 64), diL = __shfl(di, L, 64);
                            if (fabs(e2L - 100.0) <= m_e2 / a.margin_scale || (e2L > 100.0 && fabs(diL) <= m_d / a.margin_scale)) uncert = 1;
                            continue;
                        }
                        // (one inlined instance in a two-trip loop: a call would put the kernel on the function-call ABI --
                        //  256 VGPRs, a stack, one wave per SIMD)
                        double2 ec = make_double2(0.0, 0.0), ep = make_double2(0.0, 0.0);
#pragma unroll 1
                        for (int which = 0; which < 2; which++) {
                            const double2 r = tail_exact_sample(a, s, which ? gp : gc, dmL, lane);
                            if (which) ep = r; else ec = r;
                        }
                        if (lane == L) {
                            di = -((ep.x * ec.x) + (ep.y * ec.y));
                            dq = (ep.x * ec.y) - (ep.y * ec.x);
                            e2 = sqrt((di * di) + (dq * dq));
                        }
                        redone++;
                    }
                }
            }
            const bool valid = have && (e2 > 100.0);
            const unsigned long long vm = __ballot(valid);
            if (valid) {
                int rank = __popcll(vm & ((1ull << lane) - 1ull));
                int pos = nbits + rank;
                if (pos < a.max_bits) blog[HIST_BITS + pos] = (di < 0.0) ? (signed char)1 : (signed char)-1;
            }
            nbits += __popcll(vm);
            // the last decision of the chunk defines dmLastIQ / energy2 for what follows
            const int lastd = nd - 1 - d0;
            if (lastd >= 0 && lastd < 64) {
                energy2 = __shfl(e2, lastd, 64);
                lastI = __shfl(cur.x, lastd, 64);
                lastQ = __shfl(cur.y, lastd, 64);
                if constexpr (CERT) {
                    const int li = have ? (fastd ? 8 * d + v : (int)declist[d]) : 0;
                    last_g = 8 * MB + __shfl(li, lastd, 64);
                }
            }
        }
        JSDR_WAVE_SYNC();
    }
#ifdef JSDR_X_T8CLK
    T8_CLK(4);  // detector (of the last chunk; the others' land on "staging")
    if (lane == 0)
        for (int i = 0; i < 6; i++) atomicAdd(&g_t8_clk[i], t8acc_[i]);
#endif
    // energy1 = that of the last sample processed (:534)
    if (a.nds > 0) {
        const double2 q = y[a.nds - 1];
        energy1 = q.x * q.x + q.y * q.y;
    }
    // ---------------- write back
    const bool any_uncert = CERT && (__ballot(uncert != 0) != 0ull);
    const double e8 = __shfl(e, 8, 64);
    if (lane < 8) sp->dmEnergy[lane] = e;
    if (lane == 0) {
        sp->dmEnergyOut = e8;
        sp->lastI = lastI;
        sp->lastQ = lastQ;
        sp->energy1 = energy1;
        sp->energy2 = energy2;
        sp->peakPos = peakPos;
        sp->newPeak = newPeak;
        const int nb = nbits < a.max_bits ? nbits : a.max_bits;
        sp->cntBit = cntBit0 + nb;
        sp->nbits_prev = nb;
        if (nbits > a.max_bits) sp->overflow = 1;
        a.nbits[s] = nb;
        if constexpr (CERT) {
            sp->emax = emax;
            sp->last_g = last_g;
            sp->redone += redone;
            if (any_uncert) sp->uncertified = 1;
        }
    }
}

// ------------------------------------------------------------------------------------------- k_tail8
// The exact-order tail (:534-593) with EIGHT STREAMS PER WAVE: lane = 8 x (stream of the wave) + bit position.  k_tail
// (one wave per stream) keeps nine of its 64 lanes busy while the nine IIR chains run and moves every energy through
// LDS twice to get it to a chain lane and back; here the eight dmEnergy chains of eight streams ARE the 64 lanes, and a
// lane reads the samples of its own bit position straight from y (the eight lanes of a stream read 128 contiguous
// bytes per period) -- no transposition on the way in.  Per chunk of CH bit periods:
//   A  every lane: energy1 (:534), its dmEnergy link (:535) and -- speculating that its position is the peak -- a
//      dmEnergyOut link (:538); the chain values go to an LDS image for the argmax, the (fi,fq) of the lanes that sit on
//      the peak position to a small LDS list; the next chunk's samples are requested as this chunk's are consumed
//   B  lane = (stream, period): first-maximum argmax of the eight energies after the period (:586-592)
//   fast path (every stream of the wave locked: peakPos == newPeak == every measured peak): the decisions are (period,
//      peakPos); lane = (stream, decision): differential detector, threshold, bit (:539-545), ordered compaction
//   general path (acquisition, fades, the frame seams of the FFT-acquire mode): the peakPos / newPeak machine (:537,
//      :577-579,:592) in closed form per period (at most two decisions fall into one period), lane-replicated per stream;
//      the decision samples re-read from y (L2), dmEnergyOut re-run over them in time order, the detector lane-parallel
//      over the 2 CH decision slots -- no per-stream scalar loop, the eight streams of the wave go through it together
// energy2 = sqrt(di^2+dq^2) > 100 (:543-544) is decided as di^2+dq^2 > 10000: sqrt is correctly rounded and monotone,
// sqrt(10000) = 100 exactly and sqrt(nextafter(10000)) = 100 + 9.1e-15 rounds to the double above 100
// (tests/test_host_logic.py checks the neighbourhood); the square root itself is taken once, for the state the call leaves.
template <int CH, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_tail8(TailArgs a)
{
#ifdef JSDR_X_T8CLK
    unsigned long long t8acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t8last_ = __builtin_amdgcn_s_memtime();
#endif
    static_assert(CH == 16, "two decision slots per period in one 64-bit mask, one nibble per period in another");
    constexpr int ROW = 82;  // doubles per period of the energy image: 8 streams x 10 (8 used) + 2 -> conflict-free b128 reads
    __shared__ __align__(16) double EoL_[WPB][CH * ROW];
    __shared__ __align__(16) double2 FQL_[WPB][8][CH];
    __shared__ __align__(16) unsigned char NPL_[WPB][8][CH];
    // (WPB waves per workgroup, each on its own: a workgroup of four puts one wave on every SIMD of a CU, so that the four
    //  take the registers ONE workgroup of the kernel they run beside leaves free -- four one-wave workgroups land on four CUs)
    const int wv = WPB > 1 ? (int)(threadIdx.x >> 6) : 0, wblk = (int)blockIdx.x * WPB + wv;
    double *EoL = EoL_[wv];
    double2 (*FQL)[CH] = FQL_[wv];
    unsigned char (*NPL)[CH] = NPL_[wv];
    double *X2L = EoL;                                               // general path, once the argmax has read the image:
    double2 *CURL = reinterpret_cast<double2 *>(EoL + 8 * 2 * CH);   // [8][2 CH] each
    static_assert(8 * 2 * CH * 3 <= CH * ROW, "work areas fit the dead energy image");
    const int lane = threadIdx.x & 63, s8 = lane >> 3, c = lane & 7;
    const int S = a.nstreams;
    const int sraw = wblk * 8 + s8;
    const bool live = sraw < S;
    const int s = live ? sraw : S - 1;  // (surplus lanes of the last wave shadow its last stream and store nothing)
    TailState *sp = &a.st[s];
    const int nds = (int)a.nds;
    const long long g_first = a.g_first;
    // ---- carry the 5200-bit shift register (dmFECCorr, :503) over from the previous call's log: the whole wave per stream,
    // dwords (the rows are 16-byte aligned, the source starts at any byte)
    for (int t = 0; t < 8; t++) {
        const int st = wblk * 8 + t;
        if (st >= S) break;
        const int nprev = __builtin_amdgcn_readfirstlane(a.st[st].nbits_prev);
        const signed char *old = a.bitlog_old + (long long)st * a.bitlog_stride + nprev;
        const int sh = (int)(reinterpret_cast<unsigned long long>(old) & 3ull);
        const unsigned *ow = reinterpret_cast<const unsigned *>(old - sh);
        unsigned *nw32 = reinterpret_cast<unsigned *>(a.bitlog_new + (long long)st * a.bitlog_stride);
        constexpr int NW = HIST_BITS / 4, NIT = (NW + 63) / 64;
        unsigned lo[NIT], hi[NIT];
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            const int i = lane + 64 * q;
            const int ic = i < NW ? i : NW - 1;
            lo[q] = ow[ic];
            hi[q] = ow[ic + 1];
        }
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            const int i = lane + 64 * q;
            if (i < NW) nw32[i] = __builtin_amdgcn_alignbyte(hi[q], lo[q], (unsigned)sh);
        }
    }
    const double K1 = 1.0 - 1.0 / 200.0, S1 = 1.0 / 200.0;  // BIT_SMOOTH1 (:89)
    const double K2 = 1.0 - 1.0 / 800.0, S2 = 1.0 / 800.0;  // BIT_SMOOTH2 (:90)
    double e = sp->dmEnergy[c];
    double eo = sp->dmEnergyOut;
    int pk = sp->peakPos, nw = sp->newPeak;
    double lastI = sp->lastI, lastQ = sp->lastQ;
    const int cntBit0 = sp->cntBit;
    int nbits = 0;
    int ord_last = -1;    // this lane's latest decision (ordinal within the call) and its di^2 + dq^2: the stream's last one
    double x_last = 0.0;  // gives energy2 (:543)
    const long long M_first = g_first >> 3, M_last = (g_first + nds - 1) >> 3;
    const double2 *ys = a.y + (long long)s * a.y_stride;
    signed char *blog = a.bitlog_new + (long long)s * a.bitlog_stride;
    int rel0 = (int)(8 * M_first - g_first);  // call-relative index of the chunk's sample 0 (-7 .. 0 for the first chunk)
    // (reads before sample 0 and past the last one stay inside the buffers' slack, Y_PAD; what they return is never used)
    // The call's first period may start and its last may end anywhere (range masks, uniform over the streams).  One code path:
    // with the masks under a branch -- or two sample buffers picked by a branch -- the compiler reconciles the register
    // assignment of the requests in flight where the paths meet, with copies behind an s_waitcnt vmcnt(0): the whole memory
    // latency per chunk (3.0 ms at 8192 streams where the reads alone take 2.2).
    // (the state is due HERE, before the first requests go out: a loop-carried value that is still on its way at the loop's
    //  entry makes the compiler wait for it -- and for everything requested before it -- in EVERY iteration)
    asm volatile("" : "+v"(e), "+v"(eo), "+v"(lastI), "+v"(lastQ), "+v"(pk), "+v"(nw));
    double2 F[CH];
    if (nds > 0) {
        const double2 *p0 = ys + (rel0 + c);
#pragma unroll
        for (int p = 0; p < CH; p++) F[p] = p0[8 * p];
    }
    T8_CLK(0);  // shift register, state, first requests
    for (long long MB = M_first; MB <= M_last && nds > 0; MB += CH, rel0 += 8 * CH) {
        const int v = pk;
        const bool mine = c == v;
        double eo_l = eo;
        const double2 *pn = ys + (rel0 + 8 * CH + c);
        // ---------------- A: the chains; a sample's register is asked for the next chunk's as soon as it has been read
#pragma unroll
        for (int p = 0; p < CH; p++) {
            const double2 f = F[p];
            const double en = (f.x * f.x) + (f.y * f.y);  // :534
            if (mine) FQL[s8][p] = f;
            double x1 = en * S1, x2 = en * S2;
            asm volatile("" : "+v"(x1), "+v"(x2));  // (due HERE: nothing of the sample may be needed below the request)
            // (the sample's last use lies ABOVE the request that overwrites it: scheduled the other way round -- the scheduler's
            //  preference -- the new sample needs registers of its own and comes home through copies behind an s_waitcnt
            //  vmcnt(0) at the loop's back edge: the whole memory latency per chunk)
            __builtin_amdgcn_sched_barrier(0);
#ifndef JSDR_X_T8_NOLOAD  // (timing probe: the first chunk's samples over and over -- the kernel without its HBM reads)
            F[p] = pn[8 * p];
#endif
            __builtin_amdgcn_sched_barrier(0);
            const double ne = (e * K1) + x1;       // :535
            const double no = (eo_l * K2) + x2;    // :538, were this lane's position the peak
            const bool inr = (unsigned)(rel0 + 8 * p + c) < (unsigned)nds;
            e = inr ? ne : e;
            eo_l = inr ? no : eo_l;
            EoL[p * ROW + s8 * 10 + c] = e;
        }
        JSDR_WAVE_SYNC();
        T8_CLK(1);  // A
#ifdef JSDR_X_T8_LOADONLY  // (timing probe: the reads and the chains only)
        if (nds > 0) continue;
#endif
        // ---------------- B: new peak after every period whose last sample is in range (:582-593); lane = (stream, period)
        bool fail = pk != nw;
#pragma unroll
        for (int i = 0; i < CH / 8; i++) {
            const int p = 8 * i + c;
            const double2 *row = reinterpret_cast<const double2 *>(&EoL[p * ROW + s8 * 10]);
            const double2 q0 = row[0], q1 = row[1], q2 = row[2], q3 = row[3];
            double bv = q0.x;
            int np = 0;
            if (q0.y > bv) { bv = q0.y; np = 1; }  // strict: the first maximum wins
            if (q1.x > bv) { bv = q1.x; np = 2; }
            if (q1.y > bv) { bv = q1.y; np = 3; }
            if (q2.x > bv) { bv = q2.x; np = 4; }
            if (q2.y > bv) { bv = q2.y; np = 5; }
            if (q3.x > bv) { bv = q3.x; np = 6; }
            if (q3.y > bv) { bv = q3.y; np = 7; }
            const bool meas = rel0 + 8 * p + 7 < nds;
            np = meas ? np : 8;
            NPL[s8][p] = (unsigned char)np;
            fail = fail || (meas && np != v);
        }
        const bool general = __ballot(fail) != 0ull;
        JSDR_WAVE_SYNC();
        T8_CLK(2);  // B
        const int ord0 = 2 * (int)(MB - M_first) * 1;  // ordinal of the chunk's slot 0 (two slots per period)
        if (!general) {
            // ---------------- locked: one decision per period, at bit position v
            eo = __shfl(eo_l, 8 * s8 + v, 64);
#pragma unroll
            for (int i = 0; i < CH / 8; i++) {
                const int p = 8 * i + c;
                const int drel = rel0 + 8 * p + v;
                const bool inr = drel >= 0 && drel < nds;
                const double2 cur = FQL[s8][p];
                const double2 pv = FQL[s8][p > 0 ? p - 1 : 0];
                const bool from_state = p == 0 || drel < 8;  // the decision before this one fell into an earlier chunk or call
                const double pI = from_state ? lastI : pv.x, pQ = from_state ? lastQ : pv.y;
                const double di = -((pI * cur.x) + (pQ * cur.y));  // :539
                const double dq = (pI * cur.y) - (pQ * cur.x);     // :540
                const double x = (di * di) + (dq * dq);
                const bool valid = inr && x > 10000.0;             // energy2 > 100 (:544)
                const unsigned vm = (unsigned)(__ballot(valid) >> (8 * s8)) & 0xffu;
                if (valid && live) {
                    const int pos = nbits + __popc(vm & ((1u << c) - 1u));
                    if (pos < a.max_bits) blog[HIST_BITS + pos] = (di < 0.0) ? (signed char)1 : (signed char)-1;  // :545
                }
                nbits += __popc(vm);
                if (inr) {
                    ord_last = ord0 + 2 * p;
                    x_last = x;
                }
            }
            {   // dmLastIQ (:541-542) = the chunk's last decision sample
                int plast = (nds - 1 - rel0 - v) >> 3;  // (arithmetic shift: floor)
                plast = plast < CH - 1 ? plast : CH - 1;
                const int pfirst = rel0 + v >= 0 ? 0 : 1;
                const double2 l = FQL[s8][plast > 0 ? plast : 0];
                if (plast >= pfirst) {
                    lastI = l.x;
                    lastQ = l.y;
                }
            }
            T8_CLK(3);  // locked
        } else {
            // ---------------- general: the peakPos / newPeak machine per period, in closed form.  Walking the bit positions
            // cf..cl of a period (:537,:577-579): a decision where c == peakPos; at c == (peakPos+4)&7 peakPos = newPeak, after
            // which a second decision can fall at the NEW peakPos if that position is still to come.
            unsigned long long smask = 0ull;  // bit 2p+k: decision slot k of period p is taken
            unsigned long long pos1 = 0ull, pos2 = 0ull;  // nibble p: the bit position of slot 0 / slot 1
            {
                const uint4 n4 = *reinterpret_cast<const uint4 *>(&NPL[s8][0]);
#pragma unroll
                for (int p = 0; p < CH; p++) {
                    const unsigned w = p < 4 ? n4.x : (p < 8 ? n4.y : (p < 12 ? n4.z : n4.w));
                    const int np = (int)((w >> (8 * (p & 3))) & 0xffu);
                    int cf = -(rel0 + 8 * p), cl = nds - 1 - (rel0 + 8 * p);
                    cf = cf < 0 ? 0 : cf;    // first / last bit position of the period that belongs to the call
                    cl = cl > 7 ? 7 : cl;    // (cl < cf: none of it does)
                    const int h = (pk + 4) & 7;
                    const bool pin = pk >= cf && pk <= cl;
                    const bool hin = h >= cf && h <= cl && pk != nw;
                    // the old peakPos decides unless the switch came first (h < peakPos and h inside the period)
                    const bool d1 = pin && !(hin && h < pk);
                    const bool d2 = hin && nw > h && nw <= cl;
                    if (d1) {
                        smask |= 1ull << (2 * p);
                        pos1 |= (unsigned long long)pk << (4 * p);
                    }
                    if (d2) {
                        smask |= 1ull << (2 * p + 1);
                        pos2 |= (unsigned long long)nw << (4 * p);
                    }
                    pk = hin ? nw : pk;
                    nw = np < 8 ? np : nw;  // :592
                }
            }
            // the decision samples, lane = (stream, slot); dmEnergyOut's inputs and the samples themselves go to LDS
            double2 cur[2 * CH / 8];
            bool has[2 * CH / 8];
#pragma unroll
            for (int r = 0; r < 2 * CH / 8; r++) {
                const int slot = 8 * r + c, p = slot >> 1;
                has[r] = ((smask >> slot) & 1ull) != 0ull;
                const int cpos = (int)((((slot & 1) ? pos2 : pos1) >> (4 * p)) & 15ull);
                const int rel = has[r] ? rel0 + 8 * p + cpos : 0;
                cur[r] = ys[rel];
            }
#pragma unroll
            for (int r = 0; r < 2 * CH / 8; r++) {
                const int slot = 8 * r + c;
                const double en = (cur[r].x * cur[r].x) + (cur[r].y * cur[r].y);
                X2L[s8 * 2 * CH + slot] = en * S2;
                CURL[s8 * 2 * CH + slot] = cur[r];
            }
            JSDR_WAVE_SYNC();
            // dmEnergyOut (:538) over the decisions in time order (lane-replicated per stream)
            {
                const double2 *x2 = reinterpret_cast<const double2 *>(&X2L[s8 * 2 * CH]);
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const double2 xx = x2[q];
                    const double n0 = (eo * K2) + xx.x;
                    eo = ((smask >> (2 * q)) & 1ull) ? n0 : eo;
                    const double n1 = (eo * K2) + xx.y;
                    eo = ((smask >> (2 * q + 1)) & 1ull) ? n1 : eo;
                }
            }
            // detector per slot; the previous decision is the nearest taken slot below (or the state)
#pragma unroll
            for (int r = 0; r < 2 * CH / 8; r++) {
                const int slot = 8 * r + c;
                const unsigned long long below = smask & ((1ull << slot) - 1ull);
                const int prev = below ? 63 - __clzll((long long)below) : 0;
                const double2 pv = CURL[s8 * 2 * CH + prev];
                const double pI = below ? pv.x : lastI, pQ = below ? pv.y : lastQ;
                const double di = -((pI * cur[r].x) + (pQ * cur[r].y));
                const double dq = (pI * cur[r].y) - (pQ * cur[r].x);
                const double x = (di * di) + (dq * dq);
                const bool valid = has[r] && x > 10000.0;
                const unsigned vm = (unsigned)(__ballot(valid) >> (8 * s8)) & 0xffu;
                if (valid && live) {
                    const int pos = nbits + __popc(vm & ((1u << c) - 1u));
                    if (pos < a.max_bits) blog[HIST_BITS + pos] = (di < 0.0) ? (signed char)1 : (signed char)-1;
                }
                nbits += __popc(vm);
                if (has[r]) {
                    ord_last = ord0 + slot;
                    x_last = x;
                }
            }
            if (smask) {
                const double2 l = CURL[s8 * 2 * CH + (63 - __clzll((long long)smask))];
                lastI = l.x;
                lastQ = l.y;
            }
            T8_CLK(4);  // general
        }
        JSDR_WAVE_SYNC();
    }
    // ---------------- what the call leaves
    double energy1 = sp->energy1, energy2 = sp->energy2;
    if (nds > 0) {
        const double2 q = ys[nds - 1];
        energy1 = (q.x * q.x) + (q.y * q.y);  // that of the last sample processed (:534)
    }
    {   // energy2 (:543) of the stream's last decision: the lane of the stream that holds the highest ordinal
        int o = ord_last;
        double x = x_last;
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            const int oo = __shfl_xor(o, off, 64);
            const double xo = __shfl_xor(x, off, 64);
            if (oo > o) {
                o = oo;
                x = xo;
            }
        }
        if (o >= 0) energy2 = sqrt(x);
    }
    if (live) {
        sp->dmEnergy[c] = e;
        if (c == 0) {
            sp->dmEnergyOut = eo;
            sp->lastI = lastI;
            sp->lastQ = lastQ;
            sp->energy1 = energy1;
            sp->energy2 = energy2;
            sp->peakPos = pk;
            sp->newPeak = nw;
            const int nb = nbits < a.max_bits ? nbits : a.max_bits;
            sp->cntBit = cntBit0 + nb;
            sp->nbits_prev = nb;
            if (nbits > a.max_bits) sp->overflow = 1;
            a.nbits[s] = nb;
        }
    }
#ifdef JSDR_X_T8CLK
    T8_CLK(5);  // write-back
    if (lane == 0)
        for (int i = 0; i < 6; i++) atomicAdd(&g_t8_clk[i], t8acc_[i]);
#endif
}

// ------------------------------------------------------------------------------------------- k_sync
// sync-vector correlation for every new bit (:556-559): window = the 5200 most recent bits, 65 taps at
// stride 80.  corr[b] kept (int8) for the dmMaxCorr bookkeeping; hits (>=45, :560) go to a per-stream list.
__global__ void k_sync(SyncArgs a)
{
    const int s = blockIdx.y;
    const int nb = a.nbits[s];
    const signed char *bl = a.bitlog + (long long)s * a.bitlog_stride;
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += gridDim.x * blockDim.x) {
        const signed char *w = bl + b + 1;  // dmFECCorr after shifting bit b in
        int c = 0;
#pragma unroll 5
        for (int n = 0; n < SYNC_N; n++) c += (int)w[n * 80] * (int)c_bpsk.sync[n];
        a.corr[(long long)s * a.max_bits + b] = (signed char)c;
    }
}

// k_sync_t: the same correlations from a TRANSPOSED image of the stream's bit log in LDS.  Window p of output b is
// W[b + 80 n], W[p] = bitlog[1 + p]: with T[p mod 80][p div 80] = W[p] the 65 bytes of an output are CONTIGUOUS in row
// b mod 80 from column b div 80 -- eighteen aligned dword reads, a byte alignment and seventeen v_dot4_i32_i8 against
// the packed sync vector instead of 65 strided byte loads and 65 multiply-adds (integer arithmetic: same sums).  One
// workgroup per stream; the row stride is 4 * odd so that the rows of 32 consecutive outputs fall on 32 different banks.
// Its first wave then orders the hits and leaves dmCorr / dmMaxCorr (sync_fin_wave below; a kernel of its own until
// round 3: one dependent launch less per call): the workgroup's correlations are read back from global memory behind a
// device-scope release / acquire pair around the barrier.
__device__ __forceinline__ void sync_fin_wave(int s, int lane, int nb, const signed char *c, int *trig_count, int *trig_bits,
                                              int trig_cap, TailState *st);
__global__ __launch_bounds__(256) void k_sync_t(SyncArgs a, int row_stride, SyncFinArgs f)
{
    extern __shared__ __align__(16) unsigned char smem[];
    signed char *T = reinterpret_cast<signed char *>(smem);  // [80][row_stride]
    const int s = blockIdx.x;
    const int nb = a.nbits[s];
    if (nb <= 0) {  // no new bit: no hit, dmCorr / dmMaxCorr stay (what sync_fin_wave does with nb = 0)
        if (f.fuse && threadIdx.x == 0) f.trig_count[s] = 0;
        return;
    }
    const int np = HIST_BITS - 1 + nb;  // W[0 .. np), W = the stream's log from byte 1: the last window ends at W[nb-1 + 80*64]
    {
        // the log comes in as 16-byte loads, eight per thread in flight (the rows are 16-byte aligned; W[p] is byte p + 1 of
        // the row): as a byte-at-a-time loop every one of its 120 iterations waited for its own load
        const uint4 *row16 = reinterpret_cast<const uint4 *>(a.bitlog + (long long)s * a.bitlog_stride);
        const int n16 = (np + 1 + 15) / 16;
        for (int i0 = 0; i0 < n16; i0 += 256 * 8) {
            uint4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int i = i0 + 256 * u + (int)threadIdx.x;
                v[u] = row16[i < n16 ? i : n16 - 1];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int i = i0 + 256 * u + (int)threadIdx.x;
                if (i < n16) {
                    const int p0 = 16 * i - 1;  // W index of the quad's first byte
                    int r = (p0 + 80) % 80, q = (p0 + 80) / 80 - 1;
                    const unsigned w4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                    for (int b = 0; b < 16; b++) {
                        const int p = p0 + b;
                        if (p >= 0 && p < np) T[r * row_stride + q] = (signed char)((w4[b >> 2] >> (8 * (b & 3))) & 0xffu);
                        r += 1;
                        if (r >= 80) {
                            r = 0;
                            q += 1;
                        }
                    }
                }
            }
        }
    }
    // packed sync vector: bytes 4i .. 4i+3 (zero beyond 64)
    int S4[17];
#pragma unroll
    for (int i = 0; i < 17; i++) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (4 * i + k < SYNC_N) v |= ((int)c_bpsk.sync[4 * i + k] & 0xff) << (8 * k);
        S4[i] = v;
    }
    __syncthreads();
    {
        int b = threadIdx.x, r = b % 80, q0 = b / 80;
        for (; b < nb; b += 256) {
            const int *row = reinterpret_cast<const int *>(T + r * row_stride + (q0 & ~3));
            const int sh = q0 & 3;
            int d[18];
#pragma unroll
            for (int i = 0; i < 18; i++) d[i] = row[i];
            int c = 0;
#pragma unroll
            for (int i = 0; i < 17; i++) {
                const int w = (int)__builtin_amdgcn_alignbyte((unsigned)d[i + 1], (unsigned)d[i], (unsigned)sh);
                c = __builtin_amdgcn_sdot4(w, S4[i], c, false);
            }
            a.corr[(long long)s * a.max_bits + b] = (signed char)c;
            r += 256 % 80;
            q0 += 256 / 80;
            if (r >= 80) {
                r -= 80;
                q0 += 1;
            }
        }
    }
    if (!f.fuse) return;  // (uniform)
    __threadfence();  // release: every wave's correlations are visible device-wide ...
    __syncthreads();
    if (threadIdx.x < 64) {
        __threadfence();  // ... acquire: and read from there, not from a stale L1 line
        sync_fin_wave(s, (int)threadIdx.x, nb, a.corr + (long long)s * a.max_bits, f.trig_count, f.trig_bits, f.trig_cap, f.st);
    }
}

// the hits (correlation >= 45, :560) in bit order -- one wave per stream walks the correlations 64 at a time, a ballot
// and a prefix count give every hit its slot: deterministic, and when a call holds more hits than the handle has room
// for it is the FIRST trig_cap that are kept (the stream is flagged; the getters then fail instead of returning a
// truncated result).  Then dmCorr / dmMaxCorr exactly as the serial loop leaves them (:556-572): after a hit dmMaxCorr
// restarts from 0 (:567) and immediately takes that bit's correlation (:571-572).
__device__ __forceinline__ void sync_fin_wave(int s, int lane, int nb, const signed char *c, int *trig_count, int *trig_bits,
                                              int trig_cap, TailState *st)
{
    int nt = 0, last_hit = -1;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + lane;
        const bool hit = b < nb && (int)c[b] >= 45;
        const unsigned long long m = __ballot(hit);
        if (hit) {
            const int slot = nt + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < trig_cap) trig_bits[s * trig_cap + slot] = b;
        }
        if (m) last_hit = b0 + 63 - __clzll(m);
        nt += __popcll(m);
    }
    int from = 0, best = st[s].dmMaxCorr;
    if (nt > 0) {
        from = last_hit;
        best = 0;
    }
    for (int b = from + lane; b < nb; b += 64) best = best > (int)c[b] ? best : (int)c[b];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        int o = __shfl_xor(best, off, 64);
        best = best > o ? best : o;
    }
    if (lane == 0) {
        if (nb > 0) st[s].dmCorr = c[nb - 1];
        st[s].dmMaxCorr = best;
        st[s].cntFEC += nt;  // the reference counts every hit (:566), decoded or not
        if (nt > trig_cap) {
            st[s].overflow = 1;
            nt = trig_cap;
        }
        trig_count[s] = nt;
    }
}

// after the strided k_sync (the fallback for calls whose bit log does not fit a workgroup's LDS); k_sync_t does this itself
__global__ __launch_bounds__(64) void k_sync_fin(const int *nbits, const signed char *corr, int max_bits, int *trig_count,
                                                 int *trig_bits, int trig_cap, TailState *st, int nstreams)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= nstreams) return;
    sync_fin_wave(s, lane, nbits[s], corr + (long long)s * max_bits, trig_count, trig_bits, trig_cap, st);
}


// slot = int32 header[16] | int8 bits[slot_bits] | trig_cap x {int32 rc, int32 bit_index, uint8 data[256]}
// header: nbits, nfec, cntRaw, cntDS, cntBit, cntFEC, cntDec, dmErrBits, dmCorr, dmMaxCorr, decodeOK, overflow (a stream
// that overflowed its per-call bit / FEC capacity: its slot is incomplete), uncertified (fast variant: a decision of this
// stream could not be certified), 0...
__global__ void k_pack_slots(unsigned char *slots, long long slot_bytes, int slot_bits, int trig_cap, const TailState *st,
                             const int *nbits, const signed char *bitlog, long long bitlog_stride, const int *trig_count,
                             const int *trig_bits, const int *fec_rc, const unsigned char *fec_data, const int *fec_last,
                             const int *cnt_dec, int n_in, int n_ds)
{
    const int s = blockIdx.x;
    unsigned char *slot = slots + (long long)s * slot_bytes;
    int *hdr = reinterpret_cast<int *>(slot);
    const int nb = nbits[s], nt = trig_count[s];
    if (threadIdx.x < 16) {
        int v = 0;
        switch (threadIdx.x) {
            case 0: v = nb; break;
            case 1: v = nt; break;
            case 2: v = n_in; break;
            case 3: v = n_ds; break;
            case 4: v = st[s].cntBit; break;
            case 5: v = st[s].cntFEC; break;
            case 6: v = cnt_dec[s]; break;
            case 7: v = fec_last[2 * s]; break;
            case 8: v = st[s].dmCorr; break;
            case 9: v = st[s].dmMaxCorr; break;
            case 10: v = fec_last[2 * s + 1]; break;
            case 11: v = st[s].overflow; break;
            case 12: v = st[s].uncertified; break;
            default: v = 0;
        }
        hdr[threadIdx.x] = v;
    }
    const signed char *bl = bitlog + (long long)s * bitlog_stride + HIST_BITS;
    for (int i = threadIdx.x; i < slot_bits; i += blockDim.x) slot[64 + i] = (i < nb) ? (unsigned char)bl[i] : 0;
    unsigned char *f = slot + 64 + slot_bits;
    for (int t = 0; t < trig_cap; t++) {
        int *fh = reinterpret_cast<int *>(f + t * 264);
        if (threadIdx.x == 0) {
            fh[0] = (t < nt) ? fec_rc[s * trig_cap + t] : 0;
            fh[1] = (t < nt) ? trig_bits[s * trig_cap + t] + 1 : 0;
        }
        for (int i = threadIdx.x; i < 256; i += blockDim.x)
            f[t * 264 + 8 + i] = (t < nt) ? fec_data[((long long)s * trig_cap + t) * 256 + i] : 0;
    }
}
}  // namespace jsdr

using namespace jsdr;

// ---- the 1-stream receive() forms publish their results for a concurrent reader (jsdr_bpsk_snapshot_read).  What the
// four getters behind the snapshot fetch with eleven small blocking copies (each a round trip to the device: ~130 us of
// a 290 us receive) is packed by ONE tiny kernel at the end of the side stream's work and comes back in ONE copy.
// (C linkage: the symbol profiles and traces have always shown)
extern "C" __global__ void k_snapshot_pack(SnapPack *out, const TailState *st, const int *fec_last, const int *cnt_dec, const int *nbits,
                                const FftFrontState *fs, const unsigned char *decoded, const signed char *bits_new)
{
    const int i = threadIdx.x;
    if (i == 0) {
        out->t = st[0];
        out->last[0] = fec_last[0];
        out->last[1] = fec_last[1];
        out->cdec = cnt_dec[0];
        out->nbits = nbits[0];
        out->centreBin = fs ? fs[0].centreBin : 0;
        out->pad = 0;
        out->avePeakPower = fs ? fs[0].avePeakPower : 0.0;
        out->aveCentreBin = fs ? fs[0].aveCentreBin : 0.0;
    }
    if (i < 256) out->decoded[i] = decoded[i];
    const int nb = nbits[0];
    for (int k = i; k < 512; k += blockDim.x) out->bits[k] = k < nb ? bits_new[k] : (signed char)0;
}

// actionPerformed on channel `ch` (-1: every channel) of a channel handle, after the handle's pending work: tuning (and
// tuPhaseInc, :189) and / or doUp, and dmMaxCorr = 0 (:190) in the streams of those channels on every input.  tuPhase and
// every other piece of state carry on; the other channels are not touched.  The one step that can fail comes first.
__global__ void k_reset_maxcorr_chan(TailState *st, int nin, int nch, int ch)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nin * nch && (ch < 0 || s % nch == ch)) st[s].dmMaxCorr = 0;
}

// =============================================================================================== launchers
// What bpsk_handle.hip starts (bpsk_kernels.h): the grid, the LDS and the template choice of each kernel.
namespace jsdr {

// JSDR_LAUNCH_CHECK for the launchers that return the name of the kernel they launched
#define JSDR_LAUNCH_CHECK_NAMED()                                                                                        \
    do {                                                                                                                 \
        hipError_t _e = hipGetLastError();                                                                               \
        if (_e != hipSuccess) {                                                                                          \
            ::jsdr::set_error("hipGetLastError() failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__);        \
            return nullptr;                                                                                              \
        }                                                                                                                \
    } while (0)

static int launched()
{
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int bpsk_upload_constants(const BpskConst &bc)
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

bool front_reg_enabled()
{
    static const bool reg = [] {
        const char *e = knob("JSDR_FRONT_REG");  // JSDR_FRONT_REG=0: the generic kernel instead
        return !e || atoi(e) != 0;
    }();
    return reg;
}

// can the register-staged kernel take this call?  (int16 input, 32-bit sample indices, at least one full window)
static bool front_reg_applies(const FrontArgs &fa)
{
    return front_reg_enabled() && !fa.rawf && fa.nsamples <= 0x3fffffffLL && fa.nsamples >= 64;
}

template <int D, int RD, bool MIX, bool DC, bool PER, bool FAST>
static void launch_front_reg_k(const FrontArgs &fa, int nstreams, long long nds, hipStream_t st)
{
    using G = FrontDmaGeom<D, RD>;
    // block size and tiles per wave make no difference between 1..4 waves and 1..10 tiles (swept; within 5 %)
    constexpr int WAVES = 4;
    const long long ntiles = (nds + 64 * G::R - 1) / (64 * G::R);
    long long gx = (ntiles + WAVES * 5 - 1) / (WAVES * 5);  // five tiles per wave
    if (gx > 2048) gx = 2048;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL((k_front_reg<D, RD, MIX, DC, PER, FAST>), dim3((unsigned)gx, (unsigned)nstreams), dim3(64 * WAVES), 0, st, fa);
}

// the register-staged fast path (int16 input) at every rate: 44.1 / 48 / 96 / 192 kHz
template <int D, int RD>
static bool launch_front_reg(const FrontArgs &fa, int nstreams, long long nds, bool fast, hipStream_t st)
{
    if (!front_reg_applies(fa)) return false;
    const bool dc = (fa.ic != 0) || (fa.qc != 0);
    const bool per = fa.mix && fa.tcs != nullptr;
#define JSDR_REG(MIX, DC, PER, FAST) launch_front_reg_k<D, RD, MIX, DC, PER, FAST>(fa, nstreams, nds, st)
    if (!fa.mix) {
        if (fast) { if (dc) JSDR_REG(false, true, false, true); else JSDR_REG(false, false, false, true); }
        else { if (dc) JSDR_REG(false, true, false, false); else JSDR_REG(false, false, false, false); }
    } else if (per) {
        if (fast) { if (dc) JSDR_REG(true, true, true, true); else JSDR_REG(true, false, true, true); }
        else { if (dc) JSDR_REG(true, true, true, false); else JSDR_REG(true, false, true, false); }
    } else {
        if (fast) { if (dc) JSDR_REG(true, true, false, true); else JSDR_REG(true, false, false, true); }
        else { if (dc) JSDR_REG(true, true, false, false); else JSDR_REG(true, false, false, false); }
    }
#undef JSDR_REG
    return true;
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

int launch_matched(const MatchedArgs &ma, int nstreams, hipStream_t st)
{
    const long long ntiles = (ma.g_first + ma.nds - ma.tile0 + 4159) / 4160;
    const size_t lds = (64 + 4160) * sizeof(double2);
    JSDR_LDS_ATTR(k_matched<false>, lds);
    JSDR_LDS_ATTR(k_matched<true>, lds);
    hipLaunchKernelGGL(k_matched<false>, dim3((unsigned)ntiles, (unsigned)nstreams), dim3(512), lds, st, ma);
    return launched();
}

int launch_dm_history(double2 *dm, long long dm_stride, long long nds, int nstreams, hipStream_t st)
{
    hipLaunchKernelGGL(k_dm_history, dim3((unsigned)nstreams), dim3(64), 0, st, dm, dm_stride, nds, nstreams);
    return launched();
}

int launch_fm_prep(const EdgeArgs &ea, const HistArgs &ha, const ScatterArgs &sc, hipStream_t st)
{
    hipLaunchKernelGGL(k_fm_prep, dim3((unsigned)(((long long)ea.nstreams * (4 * FM_EDGE + 32) + sc.bytes[0] + sc.bytes[1] + 255) / 256)),
                       dim3(256), 0, st, ea, ha, sc);
    return launched();
}

template <int D, int R>
static int launch_fm_t(const FmArgs &a_in, bool mix, bool dc, bool fast, int nstreams, hipStream_t st, long long *items, long long *grid_out)
{
    const size_t lds = (size_t)FM_NT * sizeof(double2) + 512 * sizeof(double);
    const long long span = 65LL * FM_NB;
    const long long ntiles = (a_in.g_first + a_in.nds - a_in.tile0 + span - 1) / span;
    FmArgs a = a_in;
    a.ntiles = (int)ntiles;
    a.nstreams = nstreams;
    static const long long grid_cap = [] {
        const char *e = knob("JSDR_FM_GRID");  // tuning knob: total workgroups (default: one per tile)
        return e ? atoll(e) : 0LL;
    }();
    long long gx = ntiles * nstreams;
    if (grid_cap > 0 && gx > grid_cap) gx = grid_cap;
    if (a.grid_limit > 0 && gx > a.grid_limit) gx = a.grid_limit;
    *items = ntiles * nstreams;
    *grid_out = gx;
    const dim3 grid((unsigned)gx), block(FM_THREADS);
#define JSDR_FM_LAUNCH(MIX, DC, FAST, SMALL)                                                                    \
    do {                                                                                                        \
        JSDR_LDS_ATTR((k_fm<D, R, MIX, DC, FAST, SMALL>), lds);                                                 \
        hipLaunchKernelGGL((k_fm<D, R, MIX, DC, FAST, SMALL>), grid, block, lds, st, a);                        \
    } while (0)
    if (!fast && a.nds <= FM_THREADS && ntiles == 1) {  // a short call (receive()): the one-output-per-thread matched half
        if (mix) { if (dc) JSDR_FM_LAUNCH(true, true, false, true); else JSDR_FM_LAUNCH(true, false, false, true); }
        else { if (dc) JSDR_FM_LAUNCH(false, true, false, true); else JSDR_FM_LAUNCH(false, false, false, true); }
    } else if (fast) {
        if (mix) { if (dc) JSDR_FM_LAUNCH(true, true, true, false); else JSDR_FM_LAUNCH(true, false, true, false); }
        else { if (dc) JSDR_FM_LAUNCH(false, true, true, false); else JSDR_FM_LAUNCH(false, false, true, false); }
    } else {
        if (mix) { if (dc) JSDR_FM_LAUNCH(true, true, false, false); else JSDR_FM_LAUNCH(true, false, false, false); }
        else { if (dc) JSDR_FM_LAUNCH(false, true, false, false); else JSDR_FM_LAUNCH(false, false, false, false); }
    }
#undef JSDR_FM_LAUNCH
    return launched();
}

int launch_fm(const FmArgs &a, int decim, bool mix, bool dc, bool fast, int nstreams, hipStream_t st, long long *items, long long *grid)
{
    switch (decim) {
        case 4: return launch_fm_t<4, 5>(a, mix, dc, fast, nstreams, st, items, grid);
        case 5: return launch_fm_t<5, 4>(a, mix, dc, fast, nstreams, st, items, grid);
        case 10: return launch_fm_t<10, 4>(a, mix, dc, fast, nstreams, st, items, grid);
        case 20: return launch_fm_t<20, 4>(a, mix, dc, fast, nstreams, st, items, grid);
    }
    set_error("bpsk: unsupported decimation %d", decim);
    return JSDR_ERR;
}

// cert: the fast variant's margin-certified tail (k_tail<true>); otherwise k_tail8 from 2048 streams, k_tail below
const char *launch_tail(const TailArgs &ta, bool cert, hipStream_t ts)
{
    const int S = ta.nstreams;
    static const bool use_tail8 = [] {
        const char *e = knob("JSDR_TAIL8");  // JSDR_TAIL8=0: the one-wave-per-stream tail (A/B timing)
        return !e || atoi(e) != 0;
    }();
    static const bool force_tail8 = [] {
        const char *e = knob("JSDR_TAIL8");  // JSDR_TAIL8=2: k_tail8 whatever the number of streams (the tests' small handles)
        return e && atoi(e) == 2;
    }();
    const char *name = "k_tail";
    if (cert)
        hipLaunchKernelGGL(k_tail<true>, dim3((unsigned)S), dim3(64), 0, ts, ta);
    else if (use_tail8 && (S >= 2048 || force_tail8))
        // (below ~2000 streams there are too few waves of eight streams to fill the chip and a wave's own latency per chunk
        //  decides: 1024 streams, FFT-acquire lines of round 4: locked 0.64 ms (k_tail) against 1.6, unlocked 5.6 against 3.5)
    {
        static const int wpb = [] {
            const char *e = knob("JSDR_TAIL8_WPB");  // JSDR_TAIL8_WPB=1: one-wave workgroups (A/B timing)
            return e ? atoi(e) : 4;
        }();
        const unsigned waves = (unsigned)((S + 7) / 8);
        if (wpb == 1)
            hipLaunchKernelGGL((k_tail8<16, 1>), dim3(waves), dim3(64), 0, ts, ta);
        else
            hipLaunchKernelGGL((k_tail8<16, 4>), dim3((waves + 3) / 4), dim3(256), 0, ts, ta);
        name = "k_tail8";
    }
    else
        hipLaunchKernelGGL(k_tail<false>, dim3((unsigned)S), dim3(64), 0, ts, ta);
    JSDR_LAUNCH_CHECK_NAMED();
    return name;
}

// k_sync_t's row stride (bytes, 4 * odd) and LDS for a handle whose calls slice at most max_bits bits
static size_t sync_t_lds(int max_bits, int *row_stride)
{
    int cols = (HIST_BITS + max_bits + 79) / 80 + 72;  // + the 18 dwords an output reads past its first column
    int rs = (cols + 3) & ~3;
    if (((rs / 4) & 1) == 0) rs += 4;  // 4 * odd
    *row_stride = rs;
    return (size_t)80 * rs + 16;
}

// transposed-image kernel when the stream's log fits a workgroup's LDS (always, up to ~8M samples a call)
bool sync_t_applies(int max_bits)
{
    static const bool use_t = [] {
        const char *e = knob("JSDR_SYNC_T");  // JSDR_SYNC_T=0: the strided kernel
        return !e || atoi(e) != 0;
    }();
    int rs = 0;
    return use_t && sync_t_lds(max_bits, &rs) <= 150 * 1024;
}

int launch_sync_t(const SyncArgs &sa, const SyncFinArgs &sf, int nstreams, hipStream_t st)
{
    int rs = 0;
    const size_t lds = sync_t_lds(sa.max_bits, &rs);
    JSDR_LDS_ATTR(k_sync_t, lds);
    hipLaunchKernelGGL(k_sync_t, dim3((unsigned)nstreams), dim3(256), lds, st, sa, rs, sf);
    return launched();
}

int launch_sync(const SyncArgs &sa, long long nds, int nstreams, hipStream_t st)
{
    int gx = (sa.max_bits + 255) / 256;
    long long maxnew = nds / 4 + 8;
    if ((long long)gx * 256 > maxnew + 255) gx = (int)((maxnew + 255) / 256);
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_sync, dim3((unsigned)gx, (unsigned)nstreams), dim3(256), 0, st, sa);
    return launched();
}

int launch_sync_fin(const SyncArgs &sa, const SyncFinArgs &sf, int nstreams, hipStream_t st)
{
    hipLaunchKernelGGL(k_sync_fin, dim3((unsigned)nstreams), dim3(64), 0, st, sa.nbits, sa.corr, sa.max_bits, sf.trig_count, sf.trig_bits,
                       sf.trig_cap, sf.st, nstreams);
    return launched();
}

int launch_reset_maxcorr(TailState *st, int nstreams, hipStream_t stream)
{
    hipLaunchKernelGGL(k_reset_maxcorr, dim3((unsigned)((nstreams + 255) / 256)), dim3(256), 0, stream, st, nstreams);  // :190
    return launched();
}

int launch_reset_maxcorr_chan(TailState *st, int nin, int nch, int ch, hipStream_t stream)
{
    hipLaunchKernelGGL(k_reset_maxcorr_chan, dim3((unsigned)((nin * nch + 255) / 256)), dim3(256), 0, stream, st, nin, nch, ch);
    return launched();
}

int launch_snapshot_pack(SnapPack *out, const TailState *st, const int *fec_last, const int *cnt_dec, const int *nbits,
                         const FftFrontState *fs, const unsigned char *decoded, const signed char *bits_new, hipStream_t stream)
{
    hipLaunchKernelGGL(k_snapshot_pack, dim3(1), dim3(256), 0, stream, out, st, fec_last, cnt_dec, nbits, fs, decoded, bits_new);
    return launched();
}

int launch_pack_slots(unsigned char *slots, long long slot_bytes, int slot_bits, int trig_cap, const TailState *st, const int *nbits,
                      const signed char *bitlog, long long bitlog_stride, const int *trig_count, const int *trig_bits, const int *fec_rc,
                      const unsigned char *fec_data, const int *fec_last, const int *cnt_dec, int n_in, int n_ds, int nstreams, hipStream_t stream)
{
    hipLaunchKernelGGL(k_pack_slots, dim3((unsigned)nstreams), dim3(256), 0, stream, slots, slot_bytes, slot_bits, trig_cap, st, nbits, bitlog,
                       bitlog_stride, trig_count, trig_bits, fec_rc, fec_data, fec_last, cnt_dec, n_in, n_ds);
    return launched();
}

void bpsk_debug_clocks_report()
{
#ifdef JSDR_X_T8CLK
    {
        unsigned long long cc[8] = {0};
        if (hipMemcpyFromSymbol(cc, HIP_SYMBOL(g_t8_clk), sizeof(cc)) == hipSuccess) {
            static const char *nm[6] = {"prologue", "A chains", "B argmax", "locked", "general", "write-back"};
            unsigned long long tot = 0;
            for (int i = 0; i < 6; i++) tot += cc[i];
            for (int i = 0; i < 6; i++) fprintf(stderr, "k_tail8 clk %-12s %14llu ticks %5.1f%%\n", nm[i], cc[i], 100.0 * cc[i] / (tot ? tot : 1));
            memset(cc, 0, sizeof(cc));
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_t8_clk), cc, sizeof(cc));
        }
    }
#endif
#ifdef JSDR_X_CLK
    {
        static unsigned long long cc[256][64];
        if (hipMemcpyFromSymbol(cc, HIP_SYMBOL(g_fm_clk), sizeof(cc)) == hipSuccess) {
            static const char *nm[6] = {"-", "front half", "-", "barrier front", "matched", "barrier matched"};
            for (int i = 0; i < 6; i++) {
                if (i == 0 || i == 2) continue;
                fprintf(stderr, "k_fm clk %-16s", nm[i]);
                for (int w = 0; w < 8; w++) {
                    unsigned long long c = 0, tot = 0;
                    for (int b = 0; b < 256; b++) {
                        c += cc[b][w * 8 + i];
                        for (int k = 0; k < 6; k++) tot += cc[b][w * 8 + k];
                    }
                    fprintf(stderr, " w%d %5.1f%%", w, 100.0 * c / (tot ? tot : 1));
                }
                fprintf(stderr, "\n");
            }
            memset(cc, 0, sizeof(cc));
            hipMemcpyToSymbol(HIP_SYMBOL(g_fm_clk), cc, sizeof(cc));
        }
    }
#endif
}

}  // namespace jsdr
