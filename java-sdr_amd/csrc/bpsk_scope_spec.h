// bpsk_scope_spec.h -- what bpsk_scope.hip (the scope's host side) and bpsk_scope_spec.hip (the painter's two spectra, one
// workgroup a row) share: the Java cast, the spectra kernels' arguments, their launcher and the rule that says which kernel
// form serves a row length.
#pragma once
#include "bpsk_fftplan.h"
#include <stdint.h>

namespace jsdr {
#pragma GCC visibility push(hidden)

// Java's (int) of a double: truncates, saturates, NaN -> 0
__device__ __forceinline__ int java_d2i(double v)
{
    if (v != v) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (-2147483647 - 1);
    return (int)v;
}

constexpr int SPEC_WIDTH_MAX = 32768;  // plot widths 1 .. 32768
constexpr int SPEC_POW2_MIN = 64, SPEC_POW2_MAX = 8192;  // the radix-2 network in LDS
constexpr int SPEC_SMALL_MAX = 512, SPEC_MID_MAX = 2048;  // mixed-radix rows: one wave, four waves, twelve waves a row

// One launch: the rows [S][c][len] at `rows` (frame f of stream s at row s c + f), transformed, and what is asked for of
//   spec [S frames][width], peak [S frames][2], psd [S frames][len]
// stored at output row s frames + f0 + f (the c frames of a pass are frames f0 .. f0 + c - 1 of the call).
struct ScopeSpecArgs {
    const double2 *rows;
    int len, c, frames, f0;
    int width;    // Wp
    double pi;    // (double)(len / 2) / (double)Wp
    int l;        // (int)pi
    int32_t *spec;
    double *peak;
    double *psd;
    int logn;     // len = 2^logn: the radix-2 network on tw = fft_twiddles_f64's table; 0: the Stockham passes of m
    const double2 *tw;
    FftmArgs m;   // np, rad, tw_off, wr_off, pmagic (fft_pass_args); m.f.tw = tw, m.f.n = len
};

// the kernel form that serves rows of len points, by name; nullptr: none (jsdr_hip.h "The BPSK scope's spectra")
const char *scope_spec_form(int len);
// the plan of such a row, its tables in w (fft_plan_build_row)
int launch_scope_spec(const ScopeSpecArgs &a, long long nrows, hipStream_t st);

// i and l of column m under the painter's double arithmetic (:286-300): first = (int)(pi m), count = (int)pi, (0, 0) at m = 0
inline void scope_spec_column(int len, int width, int m, int &first, int &count)
{
    const double pi = (double)(len / 2) / (double)width;
    first = m == 0 ? 0 : (int)(pi * (double)m);
    count = m == 0 ? 0 : (int)pi;
}

#pragma GCC visibility pop
}  // namespace jsdr
