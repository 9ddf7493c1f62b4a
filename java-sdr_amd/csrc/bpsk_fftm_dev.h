// bpsk_fftm_dev.h -- the mixed-radix front ends' pass library, device code only: the typed LDS and global views, every Stockham
// pass of a frame held as a double2 image in one workgroup's LDS (fm_pass*, fm_first*, fm_inv_*, fm_pass_generic, the fm_passr_*
// forms), fm_table and fm_forward.  The kernels built from it: k_front_fftm, k_acqm_fwd and k_acqm_inv (bpsk_fftm.hip), k_front_fftm2
// (bpsk_fftm2.hip) and k_front_fft2x (bpsk_fft2x.hip).  Include only from those kernel units, compiled with
// -ffp-contract=off: every product and sum rounds by itself, as Java's do.
//
// The transform is the oracle's mixed-radix definition (oracle/o_fft.c, fft_f64_mixed): Stockham autosort passes with radices
// 4,..,(2),3..,5.. in this order, the same per-pass twiddle tables (long double + one rounding, exact on the axes; the plan and
// the tables are bpsk_fftplan.hip's), the same fixed-order 2/3/4/5-point butterflies, the inverse as conj o forward o conj.
#pragma once
#include "bpsk_fftplan.h"
#include "bpsk_radix.h"
#include <math.h>

namespace jsdr {

// timing probe only (never in the product build): the passes without their workgroup barriers -- wrong data, unchanged
// addresses -- to see what lock-step at the barriers costs
#ifdef JSDR_X_NOBAR
#define FM_PASS_SYNC() __builtin_amdgcn_wave_barrier()
#else
#define FM_PASS_SYNC() __syncthreads()
#endif

#ifndef JSDR_FM_T
#define JSDR_FM_T 768
#endif
constexpr int FM_T = JSDR_FM_T;  // (probe builds: -DJSDR_FM_T=1024)

// Typed views of the LDS image and of the twiddle tables.  The passes are separate (noinline) functions: through a plain
// `double2 *` parameter the compiler has to treat every access as a FLAT one -- a 64-bit address computation per element,
// a null check per pointer conversion, flat loads that tie the LDS and the vector-memory counters together.  With the
// address space in the type an access is a ds_read / ds_write on a 32-bit offset with an immediate, or a global_load.
typedef double d2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) d2v lds_d2v;
typedef __attribute__((address_space(3))) double lds_f64;
typedef __attribute__((address_space(1))) const d2v gbl_d2v;
typedef __attribute__((address_space(1))) const int gbl_i32;
typedef __attribute__((address_space(1))) const f2v gbl_f2v;
// (bpsk_fft.h's float sample conversion, for a sample read through the typed view)
__device__ __forceinline__ double2 acq_sample(const f2v w) { return acq_sample(make_float2(w.x, w.y)); }

struct LdsRef {
    lds_d2v *q;
    __device__ __forceinline__ operator double2() const
    {
        const d2v v = *q;
        return make_double2(v.x, v.y);
    }
    __device__ __forceinline__ void operator=(const double2 &v) const
    {
        d2v t;
        t.x = v.x;
        t.y = v.y;
        *q = t;
    }
    __device__ __forceinline__ void put_x(double x) const { *reinterpret_cast<lds_f64 *>(q) = x; }
};
struct LdsArr {
    lds_d2v *p;
    __device__ __forceinline__ LdsRef operator[](int i) const { return LdsRef{p + i}; }
    __device__ __forceinline__ LdsArr operator+(int i) const { return LdsArr{p + i}; }
};
struct GblArr {
    gbl_d2v *p;
    __device__ __forceinline__ double2 operator[](int i) const
    {
        const d2v v = p[i];
        return make_double2(v.x, v.y);
    }
    __device__ __forceinline__ GblArr operator+(int i) const { return GblArr{p + i}; }
};
// (the low half of a flat address inside the LDS aperture is the LDS offset)
__device__ __forceinline__ LdsArr lds_arr(const void *generic) { return LdsArr{(lds_d2v *)(unsigned)(unsigned long long)generic}; }
__device__ __forceinline__ GblArr gbl_arr(const double2 *g) { return GblArr{(gbl_d2v *)(unsigned long long)g}; }

// one Stockham pass, in place: every butterfly of the pass is in registers before the first store
// NN / PP: frame size and stride as compile-time constants for the two default frames (9600, 4800): every LDS offset
// becomes an immediate, `b mod P` a mask or a constant multiply-high, and the butterfly count per thread is the
// frame's, not the largest frame's.  0 = run-time values (any other supported n).
template <int R, int NN = 0, int PP = 0, class TW = const double2 *, int NIMG = 1>
__device__ __attribute__((noinline)) void fm_pass(LdsArr X0, TW tw, int n_rt, int P_rt, unsigned pmagic, int tid)
{
    static_assert(NIMG == 1 || NN != 0, "several images: compile-time frame size");
    constexpr int ITERS = ((NIMG * ((NN ? NN : FM_NMAX) / R)) + FM_T - 1) / FM_T;
    const int n = NN ? NN : n_rt;
    const int P = PP ? PP : P_rt;
    const int nb = n / R;
    double2 v[ITERS][R];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
        const int b = bb - img * nb;
        const LdsArr X = X0 + img * NN;
        if (bb < NIMG * nb) {
            const int k = PP ? (b % PP) : (P == 1) ? 0 : b - (int)__umulhi((unsigned)b, pmagic) * P;  // b % P without the division sequence
#pragma unroll
            for (int j = 0; j < R; j++) {
                v[it][j] = X[b + j * nb];
                if (j >= 1 && P > 1) v[it][j] = cdmul(v[it][j], tw[k * j]);
            }
            dft_r<R>(v[it]);
        }
    }
    FM_PASS_SYNC();
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
        const int b = bb - img * nb;
        const LdsArr X = X0 + img * NN;
        if (bb < NIMG * nb) {
            const int k = PP ? (b % PP) : (P == 1) ? 0 : b - (int)__umulhi((unsigned)b, pmagic) * P;  // (2^32/1 does not fit the magic)
            const int j0 = (b - k) * R + k;
#pragma unroll
            for (int q = 0; q < R; q++) X[j0 + q * P] = v[it][q];
        }
    }
    FM_PASS_SYNC();
}

// The LAST pass of the inverse transform: RxDownSample reads nothing but re/n (FUNcubeBPSKDemod.java:461-463), so only the
// real part of every output is formed (the imaginary halves of the 5-point butterfly -- a third of its operations --
// have no reader and are not computed) and it is stored already scaled: X[i].x = re * (1/n), once per sample instead of
// once per tap that reads it.  Same operands, same operations, same order for everything that IS computed.
// TT: the two-dimensional tables of an odd half (fm_pass_t): tw[(j-1) P + k] instead of tw[k j]
// COMPACT: the scaled real parts leave as a plain array of doubles over the (dead) image -- sample t at double slot
// FM_RB0 + t, the previous frame's last 26 samples (hist) copied in front of them at FM_RB0 - 26 .. FM_RB0 - 1 -- so that a
// RxDownSample window, history included, is ONE contiguous run of 27 doubles: 14 conflict-free 16-byte reads per output
// instead of 27 eight-byte reads at a 160-byte lane stride (16 lanes on the same banks).
constexpr int FM_RB0 = 32;
// COMPACT == 2: the samples go straight to an array in global memory (the even samples of a 2 m frame, k_front_fft2x)
// NIMG (round 6, here and in the passes below): the pass over NIMG images at once -- frames f and f + 1 of a stream side by side in
// LDS, image i at X + i NN -- so that a frame of 4800 samples fills the 768 threads' work items as one of 9600 does (a pass pair of
// ONE 4800-sample frame has 300 items)
template <int NN, int PP, bool TT = false, int COMPACT = 0, class TW = const double2 *, int NIMG = 1>
__device__ __attribute__((noinline)) void fm_pass5_real(LdsArr X, TW tw, double norm, int tid, const double *hist_ = nullptr,
                                                         double *gout = nullptr)
{
    constexpr int R = 5, nb = NN / R, ITERS = (NIMG * nb + FM_T - 1) / FM_T;
    double o[ITERS][R];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        if (bb < NIMG * nb) {
            const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
            const int b = bb - img * nb;
            const LdsArr Xi = X + img * NN;
            const int k = b % PP;
            double2 v[R];
#pragma unroll
            for (int j = 0; j < R; j++) {
                v[j] = Xi[b + j * nb];
                if (j >= 1) v[j] = cdmul(v[j], TT ? tw[(j - 1) * PP + k] : tw[k * j]);
            }
            dft_r<R>(v);
#pragma unroll
            for (int q = 0; q < R; q++) o[it][q] = v[q].x * norm;
        }
    }
    FM_PASS_SYNC();
    lds_f64 *Rb0 = reinterpret_cast<lds_f64 *>(X.p);
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        if (bb < NIMG * nb) {
            const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
            const int b = bb - img * nb;
            const LdsArr Xi = X + img * NN;
            lds_f64 *Rbi = Rb0 + img * (2 * NN);
            const int k = b % PP;
            const int j0 = (b - k) * R + k;
#pragma unroll
            for (int q = 0; q < R; q++) {
                if (COMPACT == 2)
                    gout[j0 + q * PP] = o[it][q];
                else if (COMPACT == 1)
                    Rbi[FM_RB0 + j0 + q * PP] = o[it][q];
                else
                    Xi[j0 + q * PP].put_x(o[it][q]);
            }
        }
    }
    lds_f64 *Rb = Rb0;
    if (COMPACT == 1 && hist_ != nullptr) {
        const lds_f64 *hist = (const lds_f64 *)(unsigned)(unsigned long long)hist_;
        if (tid < 26) Rb[FM_RB0 - 26 + tid] = hist[tid];
    }
    if (COMPACT == 2) __threadfence_block();
    FM_PASS_SYNC();
}

// The LAST pass of the forward transform: of the n bins only those the front end can read are formed -- |X| over
// [beg+24, end-24) (:425-427, the boxcar's reach) and the 204 bins around a centre bin (:458), which the rule and its
// clamps keep in [102, end-1] (:444-453): everything below need_end = end + 102, end = n/4 (lower band) or n/2 (upper).  A
// butterfly whose only needed output is q = 0 forms (x0 + a1) + a2 alone (32 of its 72 operations); all others run in
// full and store what is read.
// need_end: outputs [0, need_end) of THIS transform are read (a half transform of a 2 m frame holds every second bin)
template <int NN, int PP, bool TT = false, class TW = const double2 *, int NIMG = 1>
__device__ __attribute__((noinline)) void fm_pass5_band(LdsArr X, TW tw, int need_end, int tid)
{
    constexpr int R = 5, nb = NN / R, ITERS = (NIMG * nb + FM_T - 1) / FM_T;
    static_assert(PP == nb, "the last pass: one butterfly per k");
    double2 v[ITERS][R];
    unsigned need[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
        const int b = bb - img * nb;  // == k
        const LdsArr Xi = X + img * NN;
        need[it] = 0u;
        if (bb < NIMG * nb) {
#pragma unroll
            for (int q = 0; q < R; q++) {
                const int bin = b + q * PP;
                if (bin < need_end) need[it] |= 1u << q;
            }
#pragma unroll
            for (int j = 0; j < R; j++) {
                v[it][j] = Xi[b + j * nb];
                if (j >= 1) v[it][j] = cdmul(v[it][j], TT ? tw[(j - 1) * PP + b] : tw[b * j]);
            }
            if (need[it] & ~1u) {
                dft_r<R>(v[it]);
            } else {
                // output 0 alone, as dft_r<5> forms it: (x0 + a1) + a2 with a1 = v1 + v4, a2 = v2 + v3
                const double2 a1 = cdadd(v[it][1], v[it][4]), a2 = cdadd(v[it][2], v[it][3]);
                v[it][0] = make_double2((v[it][0].x + a1.x) + a2.x, (v[it][0].y + a1.y) + a2.y);
            }
        }
    }
    FM_PASS_SYNC();
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        if (bb < NIMG * nb) {
            const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
            const int b = bb - img * nb;
            const LdsArr Xi = X + img * NN;
#pragma unroll
            for (int q = 0; q < R; q++)
                if (need[it] & (1u << q)) Xi[b + q * PP] = v[it][q];
        }
    }
    FM_PASS_SYNC();
}

// The first THREE passes (4, 4, 4) of the inverse transform of the default frames, straight from the gathered bins.
// After them the image holds C = n/64 blocks of 64: block m = the 64-point transform of z[m + C i], i < 64, of which only
// z[m] (i = 0), z[m + C] (i = 1, if m + C < 204) and z[m + 2C] (i = 2, if m + 2C < 204) are not the zeroed array's.  An
// input that is alone in its butterfly passes through it unchanged (a + 0 = a; 0 * w = 0), so passes 1 and 2 only copy,
// and in pass 3 butterfly k < 16 of block m takes v0 = z[m], v1 = z[m + C] T64[k], v2 = z[m + 2C] T64[2k], v3 = 0:
//     a = v0 + v2, b = v0 - v2, c = d = v1:   out[k] = a + c, out[k+32] = a - c, out[k+16] = b - i d, out[k+48] = b + i d
// -- the operations the three general passes perform on these operands, minus the ones whose second operand is a zero of
// the zeroed array.  (Those return their first operand; only the SIGN of an exact zero can differ from the general
// passes' -- a sum of zeros -- and a zero's sign reaches nothing RxDownSample computes: its accumulators start at +0.0 and
// x + (+-0) = x.)  Replaces fm_first_from_bins + fm_pass2<4,4>: one LDS round trip and two thirds of a transform's
// radix-4 arithmetic less per frame.  z = conj of the spectrum bin (the inverse is conj o forward o conj).
// src / CONJ: where the 204 values z[0..203] come from -- the spectrum image itself (conjugated on the way, CONJ) or a
// small array of already conjugated values beside the image.  tw1[k * s1], tw2[k * s2]: the pass-3 twiddles of inputs
// 1 and 2 -- T64[k], T64[2k] for a transform with the ordinary tables, U[k], U[16 + k] for an odd half's (fm_pass_t).
// src_d1 (NIMG == 2): where the second image's 204 values start, relative to src0
template <int NN, bool CONJ, class TW1, class TW2, int NIMG = 1>
__device__ __attribute__((noinline)) void fm_inv_blocks(LdsArr X, LdsArr src0, TW1 tw1, int s1, TW2 tw2, int s2, int tid, int src_d1 = 0)
{
    constexpr int C = NN / 64, NITEM = C * 16, ITERS = (NIMG * NITEM + FM_T - 1) / FM_T;
    static_assert(3 * C > 204, "at most three of a block's 64 inputs come from the 204 bins");
    double2 z0[ITERS], z1[ITERS], z2[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int idd = it * FM_T + tid;
        const int img = (NIMG > 1 && idd >= NITEM) ? 1 : 0;
        const int id = idd - img * NITEM;
        const LdsArr src = src0 + img * src_d1;
        const int m = id >> 4;
        z0[it] = z1[it] = z2[it] = make_double2(0.0, 0.0);
        if (idd < NIMG * NITEM) {
            const double2 a = src[m];
            z0[it] = make_double2(a.x, CONJ ? -a.y : a.y);
            if (m + C < 204) {
                const double2 b = src[m + C];
                z1[it] = make_double2(b.x, CONJ ? -b.y : b.y);
            }
            if (m + 2 * C < 204) {
                const double2 c = src[m + 2 * C];
                z2[it] = make_double2(c.x, CONJ ? -c.y : c.y);
            }
        }
    }
    FM_PASS_SYNC();  // every bin is in registers before the image is overwritten
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int idd = it * FM_T + tid;
        if (idd < NIMG * NITEM) {
            const int img = (NIMG > 1 && idd >= NITEM) ? 1 : 0;
            const int id = idd - img * NITEM;
            const int m = id >> 4, k = id & 15;
            double2 a = z0[it], b = z0[it];
            if (m + 2 * C < 204) {
                const double2 v2 = cdmul(z2[it], tw2[k * s2]);
                a = cdadd(z0[it], v2);
                b = cdsub(z0[it], v2);
            }
            const LdsArr o = X + (img * NN + 64 * m + k);
            if (m + C < 204) {
                const double2 v1 = cdmul(z1[it], tw1[k * s1]);
                o[0] = cdadd(a, v1);
                o[32] = cdsub(a, v1);
                o[16] = make_double2(b.x + v1.y, b.y - v1.x);
                o[48] = make_double2(b.x - v1.y, b.y + v1.x);
            } else {
                o[0] = a;
                o[32] = a;
                o[16] = b;
                o[48] = b;
            }
        }
    }
    FM_PASS_SYNC();
}

// n = 9600: the first FOUR passes (4, 4, 4, 2) of the inverse transform straight from the gathered bins.  With C = 150 a
// block of 64 (see fm_inv_blocks) has at most TWO live inputs -- block m holds E_m[k + 16 c] = z[m] (+, -i, -, +i) v1,
// v1 = z[m + 150] T64[k] for m < 54, and plainly z[m] in every slot for 54 <= m < 150.  Pass 4 (radix 2, stride 64) pairs
// block m < 75 with block m + 75 (always of the plain kind):
//     out[128 m + kk] = E_m[kk] + w,  out[128 m + kk + 64] = E_m[kk] - w,   w = z[m + 75] T128[kk],  kk < 64
// -- the general passes' operations on these operands, minus those whose second operand is a zero of the zeroed array (as
// in fm_inv_blocks).  An item (m, k < 16) forms the eight outputs kk = k + 16 c, c < 4: 1200 items, one LDS round trip for
// four passes; what follows is fm_pass2<3, 5> and the real-parts-only last pass.
template <bool CONJ, class TW64, class TW128>
__device__ __attribute__((noinline)) void fm_inv_blocks128_9600(LdsArr X, LdsArr src, TW64 t64, TW128 t128, int tid)
{
    constexpr int NITEM = 75 * 16, ITERS = (NITEM + FM_T - 1) / FM_T;
    double2 z0[ITERS], zc[ITERS], z1[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int id = it * FM_T + tid;
        const int m = id >> 4;
        z0[it] = zc[it] = z1[it] = make_double2(0.0, 0.0);
        if (id < NITEM) {
            const double2 a = src[m], c = src[m + 75];
            z0[it] = make_double2(a.x, CONJ ? -a.y : a.y);
            zc[it] = make_double2(c.x, CONJ ? -c.y : c.y);
            if (m < 54) {
                const double2 b = src[m + 150];
                z1[it] = make_double2(b.x, CONJ ? -b.y : b.y);
            }
        }
    }
    FM_PASS_SYNC();  // every bin is in registers before the image is overwritten
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int id = it * FM_T + tid;
        if (id < NITEM) {
            const int m = id >> 4, k = id & 15;
            double2 e[4] = {z0[it], z0[it], z0[it], z0[it]};
            if (m < 54) {
                const double2 v1 = cdmul(z1[it], t64[k]);
                e[0] = cdadd(z0[it], v1);
                e[2] = cdsub(z0[it], v1);
                e[1] = make_double2(z0[it].x + v1.y, z0[it].y - v1.x);
                e[3] = make_double2(z0[it].x - v1.y, z0[it].y + v1.x);
            }
            const LdsArr o = X + (128 * m + k);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const double2 w = cdmul(zc[it], t128[k + 16 * c]);
                o[16 * c] = cdadd(e[c], w);
                o[16 * c + 64] = cdsub(e[c], w);
            }
        }
    }
    FM_PASS_SYNC();
}

// TWO consecutive Stockham passes (radix R1 at stride P, then R2 at stride P*R1) in one LDS round trip.  The R1*R2
// points of a group are closed under both passes: group g = m0*P + k1 (k1 < P) takes the R2 first-pass butterflies
// b1 = g + j2*(n/(R1 R2)) -- their outputs q1 feed the R1 second-pass butterflies b2 = m0*P*R1 + (k1 + q1*P), which
// write z[m0*P*R1*R2 + k1 + q1*P + q2*P*R1].  Same operands, same tables, same operation order as fm_pass<R1>
// followed by fm_pass<R2>: only the intermediate image stays in registers (an LDS store costs 13 cycles per wave
// instruction, and the image is written once per pass).
// the image between the fused first two passes (fm_first2_from_raw: a thread stores 16 consecutive slots) and the pass
// pair that reads it: slot s lives at s ^ ((s >> 4) & 7) -- the stores of eight neighbouring lanes then fall into eight
// different 16-byte bank groups, and so do the reads of eight consecutive slots (an aligned run of 8 is permuted in place)
__device__ __forceinline__ int fm_swz(int s) { return s ^ ((s >> 4) & 7); }

// SWZ_IN: the image read is the swizzled one
template <int R1, int R2, int NN = 0, int PP = 0, bool SWZ_IN = false, class TW1 = const double2 *, class TW2 = const double2 *, int NIMG = 1>
__device__ __attribute__((noinline)) void fm_pass2(LdsArr X0, TW1 tw1, TW2 tw2, int n_rt, int P_rt, unsigned pmagic, int tid)
{
    constexpr int RR = R1 * R2;
    static_assert(NIMG == 1 || NN != 0, "several images: compile-time frame size");
    constexpr int ITERS = ((NIMG * ((NN ? NN : FM_NMAX) / RR)) + FM_T - 1) / FM_T;
    const int n = NN ? NN : n_rt;
    const int P = PP ? PP : P_rt;
    const int ng = n / RR, nb1 = n / R1;
    double2 v[ITERS][R2][R1];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int gg = it * FM_T + tid;
        const int img = (NIMG > 1 && gg >= ng) ? 1 : 0;
        const int g = gg - img * ng;
        const LdsArr X = X0 + img * NN;
        if (gg < NIMG * ng) {
            const int k1 = PP ? (g % PP) : (P == 1) ? 0 : g - (int)__umulhi((unsigned)g, pmagic) * P;
#pragma unroll
            for (int j2 = 0; j2 < R2; j2++) {
                const int b1 = g + j2 * ng;
#pragma unroll
                for (int j1 = 0; j1 < R1; j1++) {
                    v[it][j2][j1] = X[SWZ_IN ? fm_swz(b1 + j1 * nb1) : b1 + j1 * nb1];
                    if (j1 >= 1 && P > 1) v[it][j2][j1] = cdmul(v[it][j2][j1], tw1[k1 * j1]);
                }
                dft_r<R1>(v[it][j2]);
            }
            __builtin_amdgcn_sched_barrier(0);  // the second stage's twiddles are fetched after the first stage's are dead
#pragma unroll
            for (int q1 = 0; q1 < R1; q1++) {
                const int k2 = k1 + q1 * P;
                double2 w[R2];
#pragma unroll
                for (int j2 = 0; j2 < R2; j2++) {
                    w[j2] = v[it][j2][q1];
                    if (j2 >= 1) w[j2] = cdmul(w[j2], tw2[k2 * j2]);
                }
                dft_r<R2>(w);
#pragma unroll
                for (int q2 = 0; q2 < R2; q2++) v[it][q2][q1] = w[q2];
            }
        }
    }
    FM_PASS_SYNC();
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int gg = it * FM_T + tid;
        const int img = (NIMG > 1 && gg >= ng) ? 1 : 0;
        const int g = gg - img * ng;
        const LdsArr X = X0 + img * NN;
        if (gg < NIMG * ng) {
            const int k1 = PP ? (g % PP) : (P == 1) ? 0 : g - (int)__umulhi((unsigned)g, pmagic) * P;
            const LdsArr z = X + ((g - k1) * RR + k1);
#pragma unroll
            for (int q2 = 0; q2 < R2; q2++)
#pragma unroll
                for (int q1 = 0; q1 < R1; q1++) z[q1 * P + q2 * P * R1] = v[it][q2][q1];
        }
    }
    FM_PASS_SYNC();
}

// The first pass stores X[4b + q]: lane stride 4 slots, so the 8 lanes of a 16-byte-store group share two bank groups
// (4-way conflict, 32 LDS cycles per wave store instead of 8).  Rotating which output a lane stores in which
// instruction -- output (i + (lane >> 1)) & 3 in instruction i -- puts the 8 lanes on 8 different bank groups; the
// rotation is two conditional-move stages over the four values.
__device__ __forceinline__ void fm_store4_rotated(LdsArr X, int b, const double2 (&v)[4], int tid)
{
    const int r = (tid >> 1) & 3;
    double2 w[4], t[4], u[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        w[i] = v[i];
        // fresh values: LLVM otherwise turns "select of array elements" into a dynamically indexed private array (scratch)
        asm volatile("" : "+v"(w[i].x), "+v"(w[i].y));
    }
    // (component by component on values: `c ? a[i] : a[j]` on the structs is an lvalue select, i.e. an address select)
    const bool c1 = (r & 1) != 0, c2 = (r & 2) != 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double ax = w[(i + 1) & 3].x, ay = w[(i + 1) & 3].y, bx = w[i].x, by = w[i].y;
        t[i] = make_double2(c1 ? ax : bx, c1 ? ay : by);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double ax = t[(i + 2) & 3].x, ay = t[(i + 2) & 3].y, bx = t[i].x, by = t[i].y;
        u[i] = make_double2(c2 ? ax : bx, c2 ? ay : by);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) X[4 * b + ((i + r) & 3)] = u[i];
}

// The first pass (radix 4, stride 1, no twiddles) of the default frames, fused with what produces its input: the
// forward transform's straight from the frame's samples in global memory (x[b + j n/4], converted as :416-421), the
// inverse's from the 204 gathered bins (only input 0 of the butterflies b < 204 is not the zeroed array's (0, -0)).
// Same butterflies on the same operands as fm_pass<4>; what goes away is one LDS write of the whole image, one read
// of it and two barriers per transform.
template <int NN, bool F32IN, int NIMG = 1>
__device__ __attribute__((noinline)) void fm_first_from_raw(LdsArr X0, const int *raw_, const float2 *rawf_, int ic, int qc, int tid)
{
    constexpr int nb = NN / 4, ITERS = (NIMG * nb + FM_T - 1) / FM_T;
    gbl_i32 *raw = (gbl_i32 *)(unsigned long long)raw_;
    gbl_f2v *rawf = (gbl_f2v *)(unsigned long long)rawf_;
    int w[ITERS][4];
    f2v wf[ITERS][4];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        int bb = it * FM_T + tid;
        bb = bb < NIMG * nb ? bb : NIMG * nb - 1;
        const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
        const int b = bb - img * nb + img * NN;  // (the second image's frame follows the first in memory)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (F32IN)
                wf[it][j] = rawf[b + j * nb];
            else
                w[it][j] = raw[b + j * nb];
        }
    }
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
        const int b = bb - img * nb;
        const LdsArr X = X0 + img * NN;
        if (bb < NIMG * nb) {
            double2 v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                v[j] = F32IN ? acq_sample(wf[it][j]) : acq_sample(w[it][j], ic, qc);
            }
            dft_r<4>(v);
            fm_store4_rotated(X, b, v, tid);
        }
    }
    __syncthreads();
}

// The first TWO passes (4, 4; strides 1 and 4) of the forward transform straight from the frame's samples: group g < n/16
// holds x[g + j2 n/16 + j1 n/4] -- four first-pass butterflies (no twiddles at stride 1), their outputs q1 through the
// four second-pass butterflies (T16[q1 j2]) -- and stores its 16 results at slots 16 g + q1 + 4 q2 of the SWIZZLED image
// (fm_swz).  The operations of fm_first_from_raw followed by fm_pass<4, n, 4>, on the same operands in the same order;
// what goes away is one LDS write and one read of the whole image, two barriers, and the first pass's rotated stores.
template <int NN, bool F32IN, class TW2>
__device__ __attribute__((noinline)) void fm_first2_from_raw(LdsArr X, const int *raw_, const float2 *rawf_, int ic, int qc, TW2 tw2,
                                                              int tid)
{
    constexpr int ng = NN / 16, nb1 = NN / 4;
    static_assert(ng <= FM_T, "one group per thread");
    gbl_i32 *raw = (gbl_i32 *)(unsigned long long)raw_;
    gbl_f2v *rawf = (gbl_f2v *)(unsigned long long)rawf_;
    const int g = tid < ng ? tid : ng - 1;
    int w[4][4];
    f2v wf[4][4];
#pragma unroll
    for (int j2 = 0; j2 < 4; j2++)
#pragma unroll
        for (int j1 = 0; j1 < 4; j1++) {
            if (F32IN)
                wf[j2][j1] = rawf[g + j2 * ng + j1 * nb1];
            else
                w[j2][j1] = raw[g + j2 * ng + j1 * nb1];
        }
    const bool dc = (ic != 0) || (qc != 0);
    if (tid < ng) {
        double2 v[4][4];
#pragma unroll
        for (int j2 = 0; j2 < 4; j2++) {
#pragma unroll
            for (int j1 = 0; j1 < 4; j1++) {
                if (F32IN)
                    v[j2][j1] = make_double2((double)wf[j2][j1].x, (double)wf[j2][j1].y);
                else  // (the pair at once, the correction skipped when there is none: common.h)
                    fm_convert(w[j2][j1], ic, qc, dc, v[j2][j1].x, v[j2][j1].y);
            }
            dft_r<4>(v[j2]);
        }
#pragma unroll
        for (int q1 = 0; q1 < 4; q1++) {
            double2 u[4];
#pragma unroll
            for (int j2 = 0; j2 < 4; j2++) {
                u[j2] = v[j2][q1];
                if (j2 >= 1) u[j2] = cdmul(u[j2], tw2[q1 * j2]);
            }
            dft_r<4>(u);
#pragma unroll
            for (int q2 = 0; q2 < 4; q2++) X[fm_swz(16 * tid + q1 + 4 * q2)] = u[q2];
        }
    }
    __syncthreads();
}

// The same in two steps (round 6, n = 9600): the frame's samples are REQUESTED a phase early -- at the top of the previous frame's
// RxDownSample, whose loop runs for longer than the round trip to memory takes and waits for nothing of its own -- and the two passes
// find them in registers.  With one workgroup a CU nothing else covers that latency: it was paid in full at the top of every frame.
struct FmRaw16 {
    int w[16];
    f2v wf[16];
};
template <int NN, bool F32IN>
__device__ __forceinline__ void fm_first2_request(FmRaw16 &r, const int *raw_, const float2 *rawf_, int tid)
{
    constexpr int ng = NN / 16, nb1 = NN / 4;
    gbl_i32 *raw = (gbl_i32 *)(unsigned long long)raw_;
    gbl_f2v *rawf = (gbl_f2v *)(unsigned long long)rawf_;
    const int g = tid < ng ? tid : ng - 1;
#pragma unroll
    for (int j2 = 0; j2 < 4; j2++)
#pragma unroll
        for (int j1 = 0; j1 < 4; j1++) {
            if (F32IN)
                r.wf[4 * j2 + j1] = rawf[g + j2 * ng + j1 * nb1];
            else
                r.w[4 * j2 + j1] = raw[g + j2 * ng + j1 * nb1];
        }
}
template <int NN, bool F32IN, class TW2>
__device__ __forceinline__ void fm_first2_from_regs(LdsArr X, const FmRaw16 &r, int ic, int qc, TW2 tw2, int tid)
{
    constexpr int ng = NN / 16;
    const bool dc = (ic != 0) || (qc != 0);
    if (tid < ng) {
        double2 v[4][4];
#pragma unroll
        for (int j2 = 0; j2 < 4; j2++) {
#pragma unroll
            for (int j1 = 0; j1 < 4; j1++) {
                if (F32IN)
                    v[j2][j1] = make_double2((double)r.wf[4 * j2 + j1].x, (double)r.wf[4 * j2 + j1].y);
                else
                    fm_convert(r.w[4 * j2 + j1], ic, qc, dc, v[j2][j1].x, v[j2][j1].y);
            }
            dft_r<4>(v[j2]);
        }
#pragma unroll
        for (int q1 = 0; q1 < 4; q1++) {
            double2 u[4];
#pragma unroll
            for (int j2 = 0; j2 < 4; j2++) {
                u[j2] = v[j2][q1];
                if (j2 >= 1) u[j2] = cdmul(u[j2], tw2[q1 * j2]);
            }
            dft_r<4>(u);
#pragma unroll
            for (int q2 = 0; q2 < 4; q2++) X[fm_swz(16 * tid + q1 + 4 * q2)] = u[q2];
        }
    }
    __syncthreads();
}

// fm_first_from_raw<NN, F32IN, 2> in the same two steps (the paired kernel): d1 = where the second image's frame starts relative to
// the first's (NN, or 0 when the call's last frame stands alone: the second image is then a copy, computed and dropped)
template <int NN, bool F32IN>
__device__ __forceinline__ void fm_first_request2(FmRaw16 &r, const int *raw_, const float2 *rawf_, int d1, int tid)
{
    constexpr int nb = NN / 4, ITERS = (2 * nb + FM_T - 1) / FM_T;
    static_assert(ITERS * 4 <= 16, "sixteen samples a thread");
    gbl_i32 *raw = (gbl_i32 *)(unsigned long long)raw_;
    gbl_f2v *rawf = (gbl_f2v *)(unsigned long long)rawf_;
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        int bb = it * FM_T + tid;
        bb = bb < 2 * nb ? bb : 2 * nb - 1;
        const int img = bb >= nb ? 1 : 0;
        const int b = bb - img * nb + img * d1;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (F32IN)
                r.wf[4 * it + j] = rawf[b + j * nb];
            else
                r.w[4 * it + j] = raw[b + j * nb];
        }
    }
}
template <int NN, bool F32IN>
__device__ __forceinline__ void fm_first_from_regs2(LdsArr X0, const FmRaw16 &r, int ic, int qc, int tid)
{
    constexpr int nb = NN / 4, ITERS = (2 * nb + FM_T - 1) / FM_T;
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        const int img = bb >= nb ? 1 : 0;
        const int b = bb - img * nb;
        const LdsArr X = X0 + img * NN;
        if (bb < 2 * nb) {
            double2 v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                v[j] = F32IN ? acq_sample(r.wf[4 * it + j]) : acq_sample(r.w[4 * it + j], ic, qc);
            }
            dft_r<4>(v);
            fm_store4_rotated(X, b, v, tid);
        }
    }
    __syncthreads();
}

// The same for one half of a frame of 2 NN samples (k_front_fft2x): the frame's radix-2 first pass, X_c[h] = x[h] +/- x[h + NN]
// (dft_r<2>), feeds the half's first two passes directly -- 32 samples per thread in flight at once (as a load / convert /
// store loop the half paid the HBM latency thirteen times).  ODD: the half of the odd bins, whose passes multiply EVERY
// input j >= 1 by the two-dimensional tables U_p[(j-1) P' + k'] (fm_pass_t) -- tw0 = U_0 (stride 1), tw1 = U_1 (stride 4);
// the even half has no stride-1 twiddles and tw1 = T16.
template <int NN, bool F32IN, bool ODD>
__device__ __attribute__((noinline)) void fm_first2x_from_raw(LdsArr X, const int *raw_, const float2 *rawf_, int ic, int qc, GblArr tw0,
                                                               GblArr tw1, int tid)
{
    constexpr int ng = NN / 16, nb1 = NN / 4;
    static_assert(ng <= FM_T, "one group per thread");
    gbl_i32 *raw = (gbl_i32 *)(unsigned long long)raw_;
    gbl_f2v *rawf = (gbl_f2v *)(unsigned long long)rawf_;
    const int g = tid < ng ? tid : ng - 1;
    const bool dc = (ic != 0) || (qc != 0);
    double2 v[4][4];
#pragma unroll
    for (int j2 = 0; j2 < 4; j2++) {
        int w0[4], w1[4];
        f2v f0[4], f1[4];
#pragma unroll
        for (int j1 = 0; j1 < 4; j1++) {
            const int h = g + j2 * ng + j1 * nb1;
            if (F32IN) {
                f0[j1] = rawf[h];
                f1[j1] = rawf[h + NN];
            } else {
                // (the frame's SECOND read -- the odd half's -- is its last use: marked so, like the dm stores, to leave the L2 to the
                //  per-stream scratch of the even halves.  Counter traffic 27.7 -> 26.8 GB a step, the kernel 15.58 -> 15.4 ms: the 32
                //  workgroups of an XCD still cycle 7 MB of frame + scratch through a 4 MB L2)
                if (ODD) {
                    w0[j1] = __builtin_nontemporal_load(&raw[h]);
                    w1[j1] = __builtin_nontemporal_load(&raw[h + NN]);
                } else {
                    w0[j1] = raw[h];
                    w1[j1] = raw[h + NN];
                }
            }
        }
#pragma unroll
        for (int j1 = 0; j1 < 4; j1++) {
            double2 a, b;
            if (F32IN) {
                a = make_double2((double)f0[j1].x, (double)f0[j1].y);
                b = make_double2((double)f1[j1].x, (double)f1[j1].y);
            } else {
                fm_convert(w0[j1], ic, qc, dc, a.x, a.y);
                fm_convert(w1[j1], ic, qc, dc, b.x, b.y);
            }
            v[j2][j1] = ODD ? cdsub(a, b) : cdadd(a, b);
        }
    }
    if (tid < ng) {
#pragma unroll
        for (int j2 = 0; j2 < 4; j2++) {
            if (ODD) {
#pragma unroll
                for (int j1 = 1; j1 < 4; j1++) v[j2][j1] = cdmul(v[j2][j1], tw0[j1 - 1]);
            }
            dft_r<4>(v[j2]);
        }
#pragma unroll
        for (int q1 = 0; q1 < 4; q1++) {
            double2 u[4];
#pragma unroll
            for (int j2 = 0; j2 < 4; j2++) {
                u[j2] = v[j2][q1];
                if (j2 >= 1) u[j2] = cdmul(u[j2], ODD ? tw1[(j2 - 1) * 4 + q1] : tw1[q1 * j2]);
            }
            dft_r<4>(u);
#pragma unroll
            for (int q2 = 0; q2 < 4; q2++) X[fm_swz(16 * tid + q1 + 4 * q2)] = u[q2];
        }
    }
    __syncthreads();
}

template <int NN>
__device__ __attribute__((noinline)) void fm_first_from_bins(LdsArr X, double2 in0, int tid)
{
    constexpr int nb = NN / 4, ITERS = (nb + FM_T - 1) / FM_T;
    static_assert(FM_T >= 204, "butterfly b < 204 belongs to thread b");
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int b = it * FM_T + tid;
        if (b < nb) {
            const double2 Z = make_double2(0.0, -0.0);  // conj of the zeroed array
            double2 v[4] = {it == 0 ? in0 : Z, Z, Z, Z};
            dft_r<4>(v);
            fm_store4_rotated(X, b, v, tid);
        }
    }
    __syncthreads();
}

// A pass whose radix is a prime above 7 (round 5; the oracle's generic branch in fft_f64_mixed_forward): one thread per OUTPUT,
//   out[(b - k) r + k + q P] = v_0 + v_1 W[q mod r] + ... + v_{r-1} W[(r-1) q mod r],   v_j = X[b + j nb] (x T[k j] for j >= 1, P > 1)
// every product a full complex multiply, summed left to right -- the same operations in the same order as the oracle, the
// twiddled inputs re-formed for every output (identical values).  Out of place: outputs go to the stream's scratch in
// global memory, then back into the image.  O(n r) multiplications a pass: a correctness path (11.025 kHz: n = 1102 = 2 19 29).
__device__ __attribute__((noinline)) void fm_pass_generic(LdsArr X, const double2 *tw, const double2 *wr, double2 *G, int n, int P, int r,
                                                          int tid)
{
    const int nb = n / r;
    for (int o = tid; o < n; o += FM_T) {
        const int q = o / nb, b = o - q * nb;  // outputs of one q are contiguous over b: neighbouring threads read neighbouring inputs
        const int k = b % P;
        double2 acc = X[b];
        int m = 0;  // (j q) mod r
        for (int j = 1; j < r; j++) {
            m += q;
            if (m >= r) m -= r;
            double2 v = X[b + j * nb];
            if (P > 1) v = cdmul(v, tw[k * j]);
            acc = cdadd(acc, cdmul(v, wr[m]));
        }
        G[(b - k) * r + k + q * P] = acc;
    }
    __syncthreads();
    for (int i = tid; i < n; i += FM_T) X[i] = G[i];
    __syncthreads();
}

// ---- round 5: the 4410-sample frame of a 44.1 kHz card (2 . 3 . 3 . 5 . 7 . 7, the oracle's order) with compile-time passes.
// fm_passr_real / fm_passr_band: fm_pass5_real / fm_pass5_band for any radix (the last pass of 4410 is a radix-7 one).
template <int R, int NN, int PP, int COMPACT, class TW, int NIMG = 1>
__device__ __attribute__((noinline)) void fm_passr_real(LdsArr X, TW tw, double norm, int tid, const double *hist_)
{
    constexpr int nb = NN / R, ITERS = (NIMG * nb + FM_T - 1) / FM_T;
    static_assert(COMPACT == 1, "compact real samples");
    double o[ITERS][R];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        if (bb < NIMG * nb) {
            const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
            const int b = bb - img * nb;
            const LdsArr Xi = X + img * NN;
            const int k = b % PP;
            double2 v[R];
#pragma unroll
            for (int j = 0; j < R; j++) {
                v[j] = Xi[b + j * nb];
                if (j >= 1) v[j] = cdmul(v[j], tw[k * j]);
            }
            dft_r<R>(v);  // (only the real parts are read: the imaginary halves have no reader and are not formed)
#pragma unroll
            for (int q = 0; q < R; q++) o[it][q] = v[q].x * norm;
        }
    }
    FM_PASS_SYNC();
    lds_f64 *Rb = reinterpret_cast<lds_f64 *>(X.p);
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        if (bb < NIMG * nb) {
            const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
            const int b = bb - img * nb;
            const int k = b % PP;
            const int j0 = (b - k) * R + k;
#pragma unroll
            for (int q = 0; q < R; q++) Rb[img * (2 * NN) + FM_RB0 + j0 + q * PP] = o[it][q];
        }
    }
    if (hist_ != nullptr) {
        const lds_f64 *hist = (const lds_f64 *)(unsigned)(unsigned long long)hist_;
        if (tid < 26) Rb[FM_RB0 - 26 + tid] = hist[tid];
    }
    FM_PASS_SYNC();
}

template <int R, int NN, int PP, class TW, int NIMG = 1>
__device__ __attribute__((noinline)) void fm_passr_band(LdsArr X, TW tw, int need_end, int tid)
{
    constexpr int nb = NN / R, ITERS = (NIMG * nb + FM_T - 1) / FM_T;
    static_assert(PP == nb, "the last pass: one butterfly per k");
    double2 v[ITERS][R];
    unsigned need[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
        const int b = bb - img * nb;  // == k
        const LdsArr Xi = X + img * NN;
        need[it] = 0u;
        if (bb < NIMG * nb) {
#pragma unroll
            for (int q = 0; q < R; q++)
                if (b + q * PP < need_end) need[it] |= 1u << q;
            if (need[it]) {  // (a butterfly none of whose outputs is read is not formed: its inputs are dead after this pass)
#pragma unroll
                for (int j = 0; j < R; j++) {
                    v[it][j] = Xi[b + j * nb];
                    if (j >= 1) v[it][j] = cdmul(v[it][j], tw[b * j]);
                }
                dft_r<R>(v[it]);
            }
        }
    }
    FM_PASS_SYNC();
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int bb = it * FM_T + tid;
        if (bb < NIMG * nb) {
            const int img = (NIMG > 1 && bb >= nb) ? 1 : 0;
            const int b = bb - img * nb;
            const LdsArr Xi = X + img * NN;
#pragma unroll
            for (int q = 0; q < R; q++)
                if (need[it] & (1u << q)) Xi[b + q * PP] = v[it][q];
        }
    }
    FM_PASS_SYNC();
}

// The first pass pair (R1, R2; strides 1 and R1) of the INVERSE transform straight from the 204 gathered bins: what
// fm_pass2<R1, R2, NN, 1> computes on the zeroed, conjugated array of FUNcubeBPSKDemod.java:458 -- element i = conj(bin i) for
// i < 204, (0.0, -0.0) elsewhere -- without that array ever being written: item g reads element g + j2 NN/(R1 R2) + j1 NN/R1,
// which is a bin only for j1 = j2 = 0 and g < 204.  The same operations on the same operand values (the zeros included: a
// zero's sign is whatever the general pass would have produced), one LDS write of the image instead of zero-fill + scatter +
// read + write.  src: the spectrum image itself (X + centreBin - 102); every bin is in registers before the first store.
template <int R1, int R2, int NN, class TW2, int NIMG = 1>
__device__ __attribute__((noinline)) void fm_inv_pair_from_bins(LdsArr X, LdsArr src0, TW2 tw2, int tid, int src_d1 = 0)
{
    constexpr int RR = R1 * R2, ng = NN / RR, ITERS = (NIMG * ng + FM_T - 1) / FM_T;
    static_assert(ng >= 204 && FM_T >= 204, "item g < 204 holds bin g, in the first round");
    double2 v[ITERS][R2][R1];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int gg = it * FM_T + tid;
        const int img = (NIMG > 1 && gg >= ng) ? 1 : 0;
        const int g = gg - img * ng;
        if (gg < NIMG * ng) {
#pragma unroll
            for (int j2 = 0; j2 < R2; j2++) {
#pragma unroll
                for (int j1 = 0; j1 < R1; j1++) v[it][j2][j1] = make_double2(0.0, -0.0);
            }
            if ((NIMG > 1 || it == 0) && g < 204) {
                const double2 a = (src0 + img * src_d1)[g];
                v[it][0][0] = make_double2(a.x, -a.y);
            }
#pragma unroll
            for (int j2 = 0; j2 < R2; j2++) dft_r<R1>(v[it][j2]);  // (stride 1: no twiddles in the first pass)
#pragma unroll
            for (int q1 = 0; q1 < R1; q1++) {
                const int k2 = q1;  // k1 + q1 P with k1 = 0, P = 1
                double2 w[R2];
#pragma unroll
                for (int j2 = 0; j2 < R2; j2++) {
                    w[j2] = v[it][j2][q1];
                    if (j2 >= 1) w[j2] = cdmul(w[j2], tw2[k2 * j2]);
                }
                dft_r<R2>(w);
#pragma unroll
                for (int q2 = 0; q2 < R2; q2++) v[it][q2][q1] = w[q2];
            }
        }
    }
    __syncthreads();  // every bin has been read from the image
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int gg = it * FM_T + tid;
        if (gg < NIMG * ng) {
            const int img = (NIMG > 1 && gg >= ng) ? 1 : 0;
            const int g = gg - img * ng;
            const LdsArr z = X + (img * NN + g * RR);
#pragma unroll
            for (int q2 = 0; q2 < R2; q2++)
#pragma unroll
                for (int q1 = 0; q1 < R1; q1++) z[q1 + q2 * R1] = v[it][q2][q1];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ const double2 *fm_table(const double2 *twL, const FftmArgs &a, int p, int P)
{
    // the narrow tables sit in LDS: a pass that starts with a round trip to L2 for its twiddles costs ~2 us,
    // 14 times per frame, with nothing else to run on the CU
    return (a.tw_off[p] + P * a.rad[p] <= a.lds_tw) ? twL + a.tw_off[p] : a.f.tw + a.tw_off[p];
}

// first_done: the caller has already run the first pass (fm_first_from_*, default frames only)
// mode (default frames): FM_FULL the whole transform; FM_FWD_BAND the forward transform of the front end, last pass
// restricted to the outputs [0, need_end) that are read; FM_INV_REAL the inverse transform after fm_inv_blocks
// (passes 1-3 done), last pass real parts only, scaled by norm
// LDSTW: the tables of the first passes are in LDS (k_front_fftm; a.lds_tw entries) -- for the default frames that is a
// compile-time fact (fft_pass_args refuses any other split): fft_plan_build lays the tables out back to back,
//   n = 9600: radices 4,4,4,2,3,5,5, lengths 4,16,64,128,384 | 1920,9600, offsets 0,4,20,84,212 | 596,2516
//   n = 4800: radices 4,4,4,3,5,5,   lengths 4,16,64,192,960 | 4800,      offsets 0,4,20,84,276 | 1236
constexpr int FM_LDS_TW_9600 = 596, FM_LDS_TW_4800 = 1236;
enum { FM_FULL = 0, FM_FWD_BAND = 1, FM_INV_REAL = 2 };
template <bool LDSTW>
__device__ __forceinline__ void fm_forward(LdsArr X, const double2 *twL, const FftmArgs &a, int tid, bool first_done,
                                           int mode = FM_FULL, int need_end = 0, double norm = 1.0, const double *hist = nullptr,
                                           double *gout = nullptr)
{
    const GblArr g = gbl_arr(a.f.tw);
    // the reference's two default frames: the plan is known (fft_radices: 4,4,4,2,3,5,5 / 4,4,4,3,5,5)
    if (a.f.n == 9600) {
        if constexpr (LDSTW) {
            if (mode == FM_INV_REAL) {
                // k_front_fftm's inverse transform: passes 1-4 came from fm_inv_blocks128_9600
                fm_pass2<3, 5, 9600, 128>(X, lds_arr(twL) + 212, g + 596, 9600, 128, 0u, tid);
                fm_pass5_real<9600, 1920, false, 1>(X, g + 2516, norm, tid, hist);
                return;
            }
            if (mode == FM_FWD_BAND && first_done) {
                // k_front_fftm's forward transform: passes 1-2 came from fm_first2_from_raw (swizzled image); the other
                // five go as 4,2 | 3,5 | 5 -- three LDS round trips, 1200 / 640 / 1920 work items for the 768 threads
                const LdsArr t = lds_arr(twL);
                fm_pass2<4, 2, 9600, 16, true>(X, t + 20, t + 84, 9600, 16, 0u, tid);
                fm_pass2<3, 5, 9600, 128>(X, t + 212, g + 596, 9600, 128, 0u, tid);
                fm_pass5_band<9600, 1920>(X, g + 2516, need_end, tid);
                return;
            }
        } else {
            if (mode == FM_INV_REAL && gout != nullptr) {  // k_front_fft2x's even half after fm_inv_blocks128_9600; samples to gout
                fm_pass2<3, 5, 9600, 128>(X, g + 212, g + 596, 9600, 128, 0u, tid);
                fm_pass5_real<9600, 1920, false, 2>(X, g + 2516, norm, tid, nullptr, gout);
                return;
            }
            if (mode == FM_FWD_BAND && first_done) {  // k_front_fft2x's even half after fm_first2x_from_raw: the same, tables in L2
                fm_pass2<4, 2, 9600, 16, true>(X, g + 20, g + 84, 9600, 16, 0u, tid);
                fm_pass2<3, 5, 9600, 128>(X, g + 212, g + 596, 9600, 128, 0u, tid);
                fm_pass5_band<9600, 1920>(X, g + 2516, need_end, tid);
                return;
            }
        }
        auto head = [&](auto t) {
            if (mode != FM_INV_REAL) {
                if (!first_done) fm_pass<4, 9600, 1>(X, t, 9600, 1, 0u, tid);
                fm_pass2<4, 4, 9600, 4>(X, t + 4, t + 20, 9600, 4, 0u, tid);
            }
            fm_pass2<2, 3, 9600, 64>(X, t + 84, t + 212, 9600, 64, 0u, tid);
        };
        if constexpr (LDSTW)
            head(lds_arr(twL));
        else
            head(g);
        fm_pass<5, 9600, 384>(X, g + 596, 9600, 384, 0u, tid);
        if (mode == FM_FWD_BAND)
            fm_pass5_band<9600, 1920>(X, g + 2516, need_end, tid);
        else if (mode == FM_INV_REAL)
            fm_pass5_real<9600, 1920, false, LDSTW ? 1 : 0>(X, g + 2516, norm, tid, hist);  // (k_front_fftm: compact real samples)
        else
            fm_pass<5, 9600, 1920>(X, g + 2516, 9600, 1920, 0u, tid);
        return;
    }
    if (a.f.n == 4800) {
        auto head = [&](auto t) {
            if (mode != FM_INV_REAL) {
                if (!first_done) fm_pass<4, 4800, 1>(X, t, 4800, 1, 0u, tid);
                fm_pass2<4, 4, 4800, 4>(X, t + 4, t + 20, 4800, 4, 0u, tid);
            }
            fm_pass2<3, 5, 4800, 64>(X, t + 84, t + 276, 4800, 64, 0u, tid);
        };
        if constexpr (LDSTW)
            head(lds_arr(twL));
        else
            head(g);
        if (mode == FM_FWD_BAND)
            fm_pass5_band<4800, 960>(X, g + 1236, need_end, tid);
        else if (mode == FM_INV_REAL)
            fm_pass5_real<4800, 960, false, LDSTW ? 1 : 0>(X, g + 1236, norm, tid, hist);
        else
            fm_pass<5, 4800, 960>(X, g + 1236, 4800, 960, 0u, tid);
        return;
    }
    if (a.f.n == 4410) {
        // radices 2,3,3,5,7,7; table lengths 2,6,18,90,630,4410 at offsets 0,2,8,26,116,746, ALL in LDS (fft_pass_args
        // checks it): [2,3] [3,5] [7] [7] -- four LDS round trips with compile-time strides instead of the run-time plan's five
        if constexpr (LDSTW) {
            const LdsArr t = lds_arr(twL);
            if (mode != FM_INV_REAL) fm_pass2<2, 3, 4410, 1>(X, t, t + 2, 4410, 1, 0u, tid);  // (the inverse's came from the bins)
            fm_pass2<3, 5, 4410, 6>(X, t + 8, t + 26, 4410, 6, 0u, tid);
            fm_pass<7, 4410, 90>(X, t + 116, 4410, 90, 0u, tid);
            if (mode == FM_FWD_BAND)
                fm_passr_band<7, 4410, 630>(X, t + 746, need_end, tid);
            else if (mode == FM_INV_REAL)
                fm_passr_real<7, 4410, 630, 1>(X, t + 746, norm, tid, hist);
            else
                fm_pass<7, 4410, 630>(X, t + 746, 4410, 630, 0u, tid);
            return;
        }
    }
    // any other frame: run-time plan, tables wherever fm_table finds them (flat accesses)
    int P = 1;
    for (int p = 0; p < a.np;) {
        const int r = a.rad[p];
        const double2 *tw = fm_table(twL, a, p, P);
        // after the first pass (whose stores would all hit one bank group as a pair), consecutive passes go in pairs
        const int r2 = (p >= 1 && p + 1 < a.np) ? a.rad[p + 1] : 0;
        const int pair = r * 8 + r2;
        if (pair == 4 * 8 + 4 || pair == 4 * 8 + 2 || pair == 2 * 8 + 3 || pair == 3 * 8 + 5) {
            const double2 *tw2 = fm_table(twL, a, p + 1, P * r);
            if (pair == 4 * 8 + 4)
                fm_pass2<4, 4>(X, tw, tw2, a.f.n, P, a.pmagic[p], tid);
            else if (pair == 4 * 8 + 2)
                fm_pass2<4, 2>(X, tw, tw2, a.f.n, P, a.pmagic[p], tid);
            else if (pair == 2 * 8 + 3)
                fm_pass2<2, 3>(X, tw, tw2, a.f.n, P, a.pmagic[p], tid);
            else
                fm_pass2<3, 5>(X, tw, tw2, a.f.n, P, a.pmagic[p], tid);
            P *= r * r2;
            p += 2;
            continue;
        }
        if (r > 7)
            fm_pass_generic(X, tw, a.f.tw + a.wr_off[p], a.gscratch + (long long)blockIdx.x * a.gscratch_stride, a.f.n, P, r, tid);
        else if (r == 4)
            fm_pass<4>(X, tw, a.f.n, P, a.pmagic[p], tid);
        else if (r == 2)
            fm_pass<2>(X, tw, a.f.n, P, a.pmagic[p], tid);
        else if (r == 3)
            fm_pass<3>(X, tw, a.f.n, P, a.pmagic[p], tid);
        else if (r == 7)
            fm_pass<7>(X, tw, a.f.n, P, a.pmagic[p], tid);
        else
            fm_pass<5>(X, tw, a.f.n, P, a.pmagic[p], tid);
        P *= r;
        p += 1;
    }
}

}  // namespace jsdr
