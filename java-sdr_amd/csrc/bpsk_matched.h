// bpsk_matched.h -- matched_block, the register-blocked 65-tap matched filter of k_matched and of the fused kernels' matched
// halves (bpsk_fm.hip: k_matched, k_fm; bpsk_fm_f32.hip: k_fm_f32).  Text shared by those units: it reads `c_bpsk.dm_taps` of
// the INCLUDING unit's copy of the tables (bpsk_units.h), so include it after that unit's `using <unit>::c_bpsk;`.
#pragma once

namespace jsdr {

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
    // phase 1: s = s0 - i, ages u+i.  main part: every output still has a tap
    const int n1 = 66 - u0 - R;  // >= 1
    // step i = 0 is every accumulator's first product.  The reference's `0.0 + x*t` is written as fma(x, t, +0.0): the same
    // double (a non-zero product is rounded once either way, a zero product of either sign gives +0 either way) in one
    // instruction instead of two; the compiler may not do that itself, for the signed zero.
    {
        const double2 v = xl[0];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const double t = f[u0 + r];
            ai[r] = __builtin_fma(v.x, t, 0.0);
            aq[r] = __builtin_fma(v.y, t, 0.0);
        }
    }
    int i = 1;
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

}  // namespace jsdr
