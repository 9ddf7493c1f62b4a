// bpsk_acq_dev.h -- device helpers of the three-phase FFT-acquire kernels (bpsk_acq.hip, bpsk_acq_chan.hip): the LDS image of a
// frame, the oracle's butterflies grouped into passes, the LDS-only barrier, the wave maximum.
#pragma once
#include "bpsk_fft.h"
#include <math.h>

namespace jsdr {

// ---- LDS image of a frame: element e at 16-byte slot (e & ~15) | ((e & 15) ^ key(e >> 4)), key(r) = (r ^ r>>4 ^ r>>8) & 15.
// Every pass reads / writes elements e0 | (H m), m = 0..2^G-1, lanes over e0: within a row of 16 the XOR is a permutation
// (consecutive lanes -> distinct bank groups), and rows that differ in ANY nibble get different keys, so the first pass --
// a lane owns a whole row, eight lanes of a store are eight rows apart in bits 4.. after the bit reversal of the coalesced
// loads -- stores conflict-free as well.  No padding: four 2048-sample frames are 128 KB of a CU's 160.
__host__ __device__ constexpr int acq_key(int row) { return (row ^ (row >> 4) ^ (row >> 8)) & 15; }
__device__ __forceinline__ int acq_slot(int e) { return (e & ~15) | ((e & 15) ^ acq_key(e >> 4)); }
// element e0 | HM, HM a multiple of 16 whose bits are clear in e0 (every pass: e0 = base + j, HM = H m): the key splits into
// key(e0 >> 4) ^ key(HM >> 4), and with m an unrolled loop index the second half folds to a constant
__device__ __forceinline__ int acq_slot_hm(int e0, int HM)
{
    return ((e0 & ~15) + HM) | (((e0 & 15) ^ acq_key(e0 >> 4)) ^ acq_key(HM >> 4));
}

template <int BITS>
__device__ __forceinline__ int acq_brev(int x)
{
    return BITS == 0 ? 0 : (int)(__brev((unsigned)x) >> (32 - (BITS ? BITS : 1)));
}

constexpr int ACQ_TWL = 256;  // stages with wing <= 128 read their twiddles from an LDS copy of tw[0..254]

// twiddle jj of the stage with wing HALF: tw[HALF - 1 + jj] = W_n^(jj n / (2 HALF))
template <int HALF, bool UNIFORM>
__device__ __forceinline__ double2 acq_tw(const double2 *TsL, const double2 *__restrict__ tsg, int jj)
{
    if (!UNIFORM && 2 * HALF <= ACQ_TWL) return TsL[HALF - 1 + jj];
    if (UNIFORM) {  // the same entry in every lane: a scalar load
        typedef const __attribute__((address_space(4))) double *ctab_t;
        ctab_t t = (ctab_t)tsg;
        return make_double2(t[2 * (HALF - 1 + jj)], t[2 * (HALF - 1 + jj) + 1]);
    }
    return tsg[(unsigned)(HALF - 1 + jj)];
}

// G consecutive stages of the network on the 2^G values v[m] = x[base + j + HALF0 m]: the oracle's butterfly, unchanged
template <int G, int HALF0, bool INVERSE, bool UNIFORM>
__device__ __forceinline__ void acq_stages(double2 (&v)[1 << G], int j, const double2 *TsL, const double2 *__restrict__ tsg)
{
    constexpr int M = 1 << G;
#pragma unroll
    for (int t = 0; t < G; t++) {
#ifdef JSDR_ACQ_STAGE_FENCE
        if (!UNIFORM) __builtin_amdgcn_sched_barrier(0);  // a stage's twiddles are requested when the stage before is done, not all up front
#endif
        double2 w[M / 2];
#pragma unroll
        for (int u = 0; u < (1 << t); u++) {
            if (t == 0) w[u] = acq_tw<HALF0, UNIFORM>(TsL, tsg, j + HALF0 * u);
            if (t == 1) w[u] = acq_tw<HALF0 * 2, UNIFORM>(TsL, tsg, j + HALF0 * u);
            if (t == 2) w[u] = acq_tw<HALF0 * 4, UNIFORM>(TsL, tsg, j + HALF0 * u);
            if (t == 3) w[u] = acq_tw<HALF0 * 8, UNIFORM>(TsL, tsg, j + HALF0 * u);
        }
#pragma unroll
        for (int m = 0; m < M; m++) {
            if ((m >> t) & 1) continue;
            const double2 wv = w[m & ((1 << t) - 1)];
            const double wr = wv.x;
            const double wi = INVERSE ? -wv.y : wv.y;
            const double2 bq = v[m + (1 << t)];
            const double p1 = wr * bq.x, p2 = wi * bq.y, p3 = wr * bq.y, p4 = wi * bq.x;
            const double tr = p1 - p2;
            const double ti = p3 + p4;
            const double2 aq = v[m];
            v[m] = make_double2(aq.x + tr, aq.y + ti);
            v[m + (1 << t)] = make_double2(aq.x - tr, aq.y - ti);
        }
    }
}

// The first FOUR stages (wings 1, 2, 4, 8) of the FORWARD transform on sixteen converted int16 samples, the multiplications by
// the table's trivial twiddles 1 = (1, -0) and -i = (0, -1) not performed (w = 1: t = b; w = -i: t = (b.y, -b.x)).  Same
// results to the last bit, signs of zeros included, because no value in this part of the network is ever -0.0: a converted
// int16 sample is never -0.0, and a sum or a difference is -0.0 only if an operand already is (bpsk_fft.hip dit_first3_i16
// has the argument in full).  Float input may hold -0.0f and takes acq_stages.
__device__ __forceinline__ void acq_first4_i16(double2 (&v)[16], const double2 (&w)[8])  // w = tw[4], tw[6], tw[8..10], tw[12..14]
{
    auto bf1 = [](double2 &a, double2 &b) {
        const double2 x = a, y = b;
        a = make_double2(x.x + y.x, x.y + y.y);
        b = make_double2(x.x - y.x, x.y - y.y);
    };
    auto bfi = [](double2 &a, double2 &b) {
        const double2 x = a, y = b;
        a = make_double2(x.x + y.y, x.y - y.x);
        b = make_double2(x.x - y.y, x.y + y.x);
    };
    auto bfw = [](double2 &a, double2 &b, const double2 w) {
        const double2 x = a, y = b;
        const double p1 = w.x * y.x, p2 = w.y * y.y, p3 = w.x * y.y, p4 = w.y * y.x;
        const double tr = p1 - p2, ti = p3 + p4;
        a = make_double2(x.x + tr, x.y + ti);
        b = make_double2(x.x - tr, x.y - ti);
    };
#pragma unroll
    for (int h = 0; h < 16; h += 8) {
        // wing 1: tw[0] = 1
        bf1(v[h + 0], v[h + 1]);
        bf1(v[h + 2], v[h + 3]);
        bf1(v[h + 4], v[h + 5]);
        bf1(v[h + 6], v[h + 7]);
        // wing 2: tw[1] = 1, tw[2] = -i
        bf1(v[h + 0], v[h + 2]);
        bfi(v[h + 1], v[h + 3]);
        bf1(v[h + 4], v[h + 6]);
        bfi(v[h + 5], v[h + 7]);
        // wing 4: tw[3] = 1, tw[4] = W8, tw[5] = -i, tw[6] = W8^3
        bf1(v[h + 0], v[h + 4]);
        bfw(v[h + 1], v[h + 5], w[0]);
        bfi(v[h + 2], v[h + 6]);
        bfw(v[h + 3], v[h + 7], w[1]);
    }
    // wing 8: tw[7 + j] = W16^j; j = 0: 1, j = 4: -i
    bf1(v[0], v[8]);
    bfw(v[1], v[9], w[2]);
    bfw(v[2], v[10], w[3]);
    bfw(v[3], v[11], w[4]);
    bfi(v[4], v[12]);
    bfw(v[5], v[13], w[5]);
    bfw(v[6], v[14], w[6]);
    bfw(v[7], v[15], w[7]);
}

// The workgroup barrier of these kernels orders LDS traffic ONLY.  __syncthreads() is a workgroup-scope release / acquire
// fence pair around s_barrier, and the release half waits for EVERY outstanding memory operation of the wave (s_waitcnt
// vmcnt(0)): the next frame's samples requested a moment ago, the spectrum rows and boxcar sums just stored -- a round trip to
// HBM at every barrier, with two waves a SIMD to cover it.  Nothing a thread of these kernels writes to global memory is read
// by another thread of the same launch, so the barrier waits for the wave's LDS operations and nothing else.
template <int T>
__device__ __forceinline__ void acq_barrier()
{
    if constexpr (T <= 64) {  // one wave per frame: its own LDS order is all there is to keep
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    } else {
#ifdef JSDR_X_ACQ_NOBAR  // (timing probe only, wrong data: what lock-step at the barriers costs)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
    }
}

// one LDS round trip in the middle of a transform: G stages starting at wing HALF0 over the whole frame, in place (a thread
// writes the slots it read)
template <int G, int HALF0, bool INVERSE, int LOGN>
__device__ __forceinline__ void acq_mid_pass(double2 *X, const double2 *TsL, const double2 *__restrict__ tsg, int tid)
{
    constexpr int N = 1 << LOGN, T = N / 16, M = 1 << G, NG = 16 >> G;
    static_assert(HALF0 % 16 == 0, "the passes behind the first move whole rows");
#pragma unroll
    for (int it = 0; it < NG; it++) {
        const int q = tid + T * it;
        const int j = q & (HALF0 - 1);
        const int e0 = ((q - j) << G) + j;
        double2 v[M];
#pragma unroll
        for (int m = 0; m < M; m++) v[m] = X[acq_slot_hm(e0, HALF0 * m)];
        acq_stages<G, HALF0, INVERSE, false>(v, j, TsL, tsg);
#pragma unroll
        for (int m = 0; m < M; m++) X[acq_slot_hm(e0, HALF0 * m)] = v[m];
    }
}

// the grouping of a transform's stages into passes: 4 in registers first, then G2 (4), then what is left
template <int LOGN>
struct AcqPlan {
    static_assert(LOGN >= 10 && LOGN <= 13, "frames of 1024 .. 8192 samples");
    static constexpr int G3 = LOGN == 13 ? 3 : LOGN - 8;  // third pass
    static constexpr int G4 = LOGN == 13 ? 2 : 0;         // fourth pass (8192 samples only)
    static constexpr int GL = G4 ? G4 : G3;               // the last pass's stages
};

// ---- twiddles a thread keeps in registers for the whole launch: the G stages of a pass that starts at wing HALF0, for group
// position j -- stage t, entry u at w[(1 << t) - 1 + u] = tw[(HALF0 << t) - 1 + j + HALF0 u].  The frame loop then holds no
// global load but the samples' own: on this part VMEM operations return in order, so a wait for a twiddle requested after the
// next frame's samples is a wait for those samples (a round trip to HBM at two waves a SIMD).
template <int G, int HALF0>
__device__ __forceinline__ void acq_load_tw(double2 (&w)[(1 << G) - 1], int j, const double2 *tsg_)
{
    // through a pointer the compiler cannot see through: loads it can prove invariant are sunk to their first use, below the
    // barrier's memory clobber and below the next frame's samples -- the very order these requests are here to avoid
    // (as an integer, and back into the GLOBAL address space: a laundered generic pointer gives flat loads, which count as LDS
    //  operations too and make every wait a wait for everything)
    typedef double d2v_ __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(1))) const d2v_ gbl_d2v_;
    unsigned long long ta = (unsigned long long)tsg_;
    asm volatile("" : "+s"(ta));
    gbl_d2v_ *tsg = (gbl_d2v_ *)ta;
#pragma unroll
    for (int t = 0; t < G; t++)
#pragma unroll
        for (int u = 0; u < (1 << t); u++) {
            const d2v_ x = tsg[(unsigned)((HALF0 << t) - 1 + j + HALF0 * u)];
            w[(1 << t) - 1 + u] = make_double2(x.x, x.y);
        }
}
// stages [T0, T1) of such a pass on v[m] = x[base + j + HALF0 m], twiddles from the thread's registers
template <int G, int T0, int T1, bool INVERSE>
__device__ __forceinline__ void acq_stages_w(double2 (&v)[1 << G], const double2 (&w)[(1 << G) - 1])
{
    constexpr int M = 1 << G;
#pragma unroll
    for (int t = T0; t < T1; t++) {
#pragma unroll
        for (int m = 0; m < M; m++) {
            if ((m >> t) & 1) continue;
            const double2 wv = w[(1 << t) - 1 + (m & ((1 << t) - 1))];
            const double wr = wv.x;
            const double wi = INVERSE ? -wv.y : wv.y;
            const double2 bq = v[m + (1 << t)];
            const double p1 = wr * bq.x, p2 = wi * bq.y, p3 = wr * bq.y, p4 = wi * bq.x;
            const double tr = p1 - p2;
            const double ti = p3 + p4;
            const double2 aq = v[m];
            v[m] = make_double2(aq.x + tr, aq.y + ti);
            v[m + (1 << t)] = make_double2(aq.x - tr, aq.y - ti);
        }
    }
}

// the largest of the wave's non-negative doubles, in every lane: row shifts and row broadcasts on the two halves (DPP moves
// cost an instruction each; the shuffle form goes through the LDS crossbar, ~100 cycles a step with nothing to cover it)
__device__ __forceinline__ double acq_wave_max(double v)
{
#define ACQ_DPP_MAX(ctrl, rmask)                                                                                  \
    {                                                                                                             \
        const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), ctrl, rmask, 0xf, false); \
        const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), ctrl, rmask, 0xf, false); \
        v = fmax(v, __hiloint2double(hi, lo));                                                                    \
    }
    ACQ_DPP_MAX(0x111, 0xf)  // row_shr:1
    ACQ_DPP_MAX(0x112, 0xf)  // row_shr:2
    ACQ_DPP_MAX(0x114, 0xf)  // row_shr:4
    ACQ_DPP_MAX(0x118, 0xf)  // row_shr:8 -- lane 15 of every row holds its row's maximum
    ACQ_DPP_MAX(0x142, 0xa)  // row_bcast:15 into rows 1 and 3
    ACQ_DPP_MAX(0x143, 0xc)  // row_bcast:31 into rows 2 and 3 -- lane 63 holds the wave's
#undef ACQ_DPP_MAX
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

typedef const __attribute__((address_space(4))) double *acq_ctab_t;  // constant address space: uniform entries become scalar loads
__device__ __forceinline__ double2 acq_tw_s(const double2 *tsg, int i)
{
    acq_ctab_t t = (acq_ctab_t)tsg;
    return make_double2(t[2 * i], t[2 * i + 1]);
}

}  // namespace jsdr
