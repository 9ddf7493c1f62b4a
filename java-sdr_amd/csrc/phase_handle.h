// phase_handle.h -- the phase.java handle (fir_phase.hip creates and destroys it, phase_scope.hip adds the batched scope's
// schedule table to it) and the painter's column schedule, stated once for the host and the device.
#pragma once
#include "common.h"

struct jsdr_phase {
    int n = 0;
    jsdr::DevBuf<float> dpy;   // [2n] the frame
    jsdr::DevBuf<float> dmax;  // [1]
    float max = -1.0f;         // phase.java:75: `float max = -1` before the first frame
    bool have = false;
    // jsdr_phase_scope_*: {first sample, samples} of every closed column of (n, tab_bx), built on the device by k_phase_table.
    // Allocated for n columns (a sample closes at most one) at the first scope call, never at create.
    jsdr::DevBuf<int2> tab;
    int tab_bx = -1;    // the bx the table was last (asked to be) built for; -1: none yet
    int tab_ncol = 0;   // its columns, as the host's walk counts them
    const char *scope_kernel = "";  // what the last scope call launched
    int num_cu = 0;                 // of the device of the first scope call
};

namespace jsdr {

// Java (int) of a float on either side: truncate toward zero, saturate, NaN -> 0 (java_f2i of waterfall_dev.h, for the host too)
__host__ __device__ inline int phase_f2i(float v)
{
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return (-2147483647 - 1);
    return (int)v;
}

// phase.java:81: float step = (float)(bx*2)/(float)dpy.length  (bx*2 wraps as Java's int does)
inline float phase_step(int n, int bx) { return (float)(int)((unsigned)bx * 2u) / (float)(2 * n); }

// phase.java:84, 93-99, 110-114: `pos += step` in float, a column closes at the sample where (int)pos > lpix.
// emit(column, pix, first sample, samples) for every closed column, in order; returns their number.  Samples behind the last
// closed column belong to none.  Compiled with -ffp-contract=off wherever it is used (there is nothing to contract: one add).
template <class EMIT>
__host__ __device__ inline int phase_walk(int n, float step, EMIT emit)
{
    float pos = 0;
    int lpix = 0, acnt = 0, start = 0, ncol = 0;
    for (int s = 0; s < n; s++) {
        acnt += 1;
        pos += step;
        const int p = phase_f2i(pos);
        if (p > lpix) {
            emit(ncol, p, start, acnt);
            ncol++;
            lpix = p;
            acnt = 0;
            start = s + 1;
        }
    }
    return ncol;
}

}  // namespace jsdr
