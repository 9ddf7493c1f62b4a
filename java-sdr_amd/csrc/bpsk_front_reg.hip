// bpsk_front_reg.hip -- tune mode, the front end on its own for int16 input: k_front_reg, register-staged lane windows
// (48 instantiations: by far the longest compile of the front end, hence a unit of its own), and its launcher, which
// bpsk_front.hip's launch_front tries first (bpsk_units.h).
//
// One of the four units of the tune-mode pipeline, which is cut by kernel family so that an edit to one family recompiles
// that family only: bpsk_front.hip, bpsk_front_reg.hip, bpsk_fm.hip, bpsk_tail.hip (the pipeline's overview is at the top
// of the last).  Compiled with -ffp-contract=off.  Reads none of the tables in __constant__ memory: the 27 taps are
// compile-time constants (ds_tap(), bpsk_fft.h).
#include "bpsk_units.h"
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

namespace jsdr {

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

// =============================================================================================== launchers
// What bpsk_front.hip's launch_front starts (bpsk_units.h): the grid and the template choice of k_front_reg.

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
bool launch_front_reg(const FrontArgs &fa, int nstreams, long long nds, bool fast, hipStream_t st)
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

// the rates launch_front (bpsk_front.hip) dispatches on
template bool launch_front_reg<4, 20>(const FrontArgs &, int, long long, bool, hipStream_t);
template bool launch_front_reg<5, 20>(const FrontArgs &, int, long long, bool, hipStream_t);
template bool launch_front_reg<10, 40>(const FrontArgs &, int, long long, bool, hipStream_t);
template bool launch_front_reg<20, 80>(const FrontArgs &, int, long long, bool, hipStream_t);

}  // namespace jsdr
