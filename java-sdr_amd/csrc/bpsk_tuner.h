// bpsk_tuner.h -- the input-independent recurrences of FUNcubeBPSKDemod, each stated once for the host and the device: the tuner
// of doBufferTune (:384-390), the VCO of the demodulator (:511-516) and tuPhaseInc (:189 / :196).  The host scheduler
// (bpsk_sched.hip), jsdr_bpsk_tuner_walk_host and the two kernels of a tuned handle (bpsk_pst.hip: k_tuner_walk, k_front_pst)
// all step them through these functions.
//
// The tuner phase moves on and wraps with ONE subtraction, and the table index is the product tu * 256.0 divided by 2 pi --
// multiplied, then divided, never multiplied by a reciprocal -- and truncated.  Every unit that includes this is compiled with
// -ffp-contract=off: each operation rounds by itself, as Java's do, and the device's FP64 add, multiply and divide are IEEE's,
// so host and device produce the same doubles and the same indices.
// The index is 9 bits wide: 0 .. 255 are the reference's sin / cos tables, 256 is the sample the reference passes through
// unmixed (tuPhase <= 0, :388 / :395) -- entry 256 of the kernels' table is (1.0, 1.0).
#pragma once
#include "common.h"
#include <string.h>

namespace jsdr {

constexpr double TUNER_PI = 3.14159265358979323846;  // Math.PI

// tuPhaseInc = 2 pi tuning / rate, evaluated left to right   (:189 / :196)
inline double tuner_inc(double tuning, int rate) { return 2.0 * TUNER_PI * tuning / (double)rate; }

// Sample k of a ramp entry (jsdr_bpsk_plan_stream_ramps): its tuning -- one product and one sum, each rounded by itself; a slope of
// zero takes the entry's tuning itself, with no arithmetic -- and its tuPhaseInc: tuner_inc of that tuning, the division a true
// division by the rate (as a double), never a product with a reciprocal.  The host mirror, the handle's end-of-call tuning and
// the ramp forms of the two kernels of a tuned handle all step a ramp through these two.
__host__ __device__ inline double tuner_ramp_tuning(double tuning, double slope, long long k)
{
    return slope == 0.0 ? tuning : tuning + (double)k * slope;
}
__host__ __device__ inline double tuner_ramp_inc(double tuning, double slope, long long k, double rate)
{
    return 2.0 * TUNER_PI * tuner_ramp_tuning(tuning, slope, k) / rate;
}

// tuPhase += tuPhaseInc; if (tuPhase > 2 pi) tuPhase -= 2 pi   (:384-385)
__host__ __device__ inline void tuner_advance(double &tu, double inc)
{
    const double two_pi = 2.0 * TUNER_PI;
    tu += inc;
    if (tu > two_pi) tu -= two_pi;
}

// the table index of a sample mixed at phase tu (:388-390), 256 where it passes through (:395)
__host__ __device__ inline int tuner_k9(double tu)
{
    const double two_pi = 2.0 * TUNER_PI;
    return tu > 0.0 ? (int)(tu * (double)256 / two_pi) % 256 : 256;
}

// one sample: the phase moves on, then gives the sample's index
__host__ __device__ inline int tuner_step(double &tu, double inc)
{
    tuner_advance(tu, inc);
    return tuner_k9(tu);
}

// ------------------------------------------------------------------------------------------- the 8-phase tuner's exact factors
// At a tuning of an eighth of the rate (12 kHz / 96 kHz) the index walks 32, 64, .., 224, 0: phase ph <-> table index 32 ph.  Five
// of the sixteen (phase, rail) factors are exact -- cos: 1.0 at phase 0, -1.0 at 4; sin: 0.0 at 0, 1.0 at 2, -1.0 at 6 -- and the
// rest are whatever Math.cos / Math.sin gave (cos at 2 is 6.1e-17, not 0).  A product with +-1.0 is +-the sample and a product
// with 0.0 of a FINITE sample is +-0, which k_fm's specialised form builds in (bpsk_fm.hip).  The host finds the classes by bit
// pattern, from the table the schedule was built with; nothing here assumes what a libm returns.
enum { TC_GEN = 0, TC_ONE = 1, TC_MONE = 2, TC_ZERO = 3 };
constexpr int tuner8_class(int ph, int rail)  // rail 0: cos, 1: sin
{
    return rail == 0 ? ((ph & 7) == 0 ? TC_ONE : (ph & 7) == 4 ? TC_MONE : TC_GEN)
                     : ((ph & 7) == 0 ? TC_ZERO : (ph & 7) == 2 ? TC_ONE : (ph & 7) == 6 ? TC_MONE : TC_GEN);
}
inline int tuner_factor_class(double v)
{
    unsigned long long b;
    memcpy(&b, &v, sizeof(b));
    return b == 0x3ff0000000000000ULL ? TC_ONE : b == 0xbff0000000000000ULL ? TC_MONE : (b << 1) == 0 ? TC_ZERO : TC_GEN;
}
// tab[0 .. 8): one period of (cos, sin) factors.  The rotation r (0 .. 7) with class(tab[e]) == tuner8_class(e + r) for both rails
// of every entry -- the pattern has one ZERO, so there is at most one -- or -1 where the classes are not that pattern.
inline int tuner8_rotation(const double2 *tab)
{
    for (int r = 0; r < 8; r++) {
        bool ok = true;
        for (int e = 0; e < 8 && ok; e++)
            ok = tuner_factor_class(tab[e].x) == tuner8_class(e + r, 0) && tuner_factor_class(tab[e].y) == tuner8_class(e + r, 1);
        if (ok) return r;
    }
    return -1;
}

// one decimated sample of the VCO: vcoPhase += VCO_PHASE_INC; if (vcoPhase > 2 pi) vcoPhase -= 2 pi; the table index of the
// sample (:511-516).  VCO_PHASE_INC = 2 pi 1200 / 9600 (:88)
__host__ __device__ inline int vco_step(double &vco)
{
    const double two_pi = 2.0 * TUNER_PI;
    const double vinc = 2.0 * TUNER_PI * 1200.0 / (double)9600;
    vco += vinc;
    if (vco > two_pi) vco -= two_pi;
    return (int)(vco * (double)256 / two_pi) % 256;
}

}  // namespace jsdr
