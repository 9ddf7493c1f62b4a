// bpsk_fftplan.h -- the FFT-acquire plan of a frame of n samples, stated once: which front end serves the frame, its Stockham
// radix list, its per-pass twiddle tables with their offsets, and the device-side pass arguments filled from them.
//
// Five front ends serve doBufferFFT (FUNcubeBPSKDemod.java:406-464): the power-of-two kernels (bpsk_fft.hip / bpsk_acq.hip), the
// mixed-radix ones of a frame that fits one workgroup's LDS (bpsk_fftm.hip, bpsk_fftm2.hip), the 2 m one
// (bpsk_fft2x.hip) and the any-frame passes (bpsk_acqg.hip).  fft_front_kind chooses, fft_plan_build leaves the tables in `w` and
// everything a launcher needs in one FftPlan, fixed at create; a launcher copies the plan's filled arguments and adds the call's.
// The radices and the tables are the oracle's (oracle/o_fft.c: jo_fft_mixed_radices, jo_fft_mixed_table, jo_fft_twiddles_f64):
// they decide bit-identity.  No device, no HIP runtime call and no handle in here: tests/test_bpsk_fftplan_host.py drives the unit
// without a GPU.
#pragma once
#include "bpsk_fft.h"
#include <vector>

namespace jsdr {
// (internal to the library: nothing here is part of what libjsdr_hip.so exports)
#pragma GCC visibility push(hidden)

// the FFT-acquire front end that serves a frame size (fft_front_kind)
// (FRONT_ROW: no front end of FFT-acquire -- the plan of a plain row transform, fft_plan_build_row)
enum FftFront { FRONT_POW2, FRONT_FFTM, FRONT_FFT2X, FRONT_GEN, FRONT_NONE, FRONT_ROW };

constexpr int FM_NMAX = 9600;      // the largest frame whose double2 image fits a workgroup's LDS
constexpr int FM_MAXPASS = 12;     // passes of such a frame: the bound of the kernels' argument arrays
constexpr int FFT_MAXPASS = 32;    // passes of any frame up to 2^22 samples (the oracle's own bound): the plan's
constexpr size_t FM_LDS_BYTES = (size_t)160 * 1024;

// ------------------------------------------------------------------------------------------- what the LDS kernels are given
struct FftmArgs {
    FftFrontArgs f;  // n, raw, state, dm, ... (logn unused; f.tw = concatenated per-pass tables)
    int np;
    int rad[FM_MAXPASS];
    int tw_off[FM_MAXPASS];  // offset of pass p's table T[m] = exp(-2 pi i m/(P r)), m < P r
    unsigned pmagic[FM_MAXPASS];  // b / P == (b * pmagic) >> 32 for b < 2^16 (P = product of the earlier radices)
    int lds_tw;              // the tables of the first passes, lds_tw entries in all, are copied to LDS
    // round 5: a prime radix above 7 (fm_pass_generic): wr_off[p] = offset of W[m] = exp(-2 pi i m/r), m < r; the pass is
    // out of place through a per-stream scratch of n elements in global memory
    int wr_off[FM_MAXPASS];
    double2 *gscratch;
    long long gscratch_stride;
};

struct Fft2xArgs {
    FftmArgs sub;             // the m-point plan (sub.f.n = m) and everything else of the front end
    int n;                    // 2 m
    int tw1_off[FM_MAXPASS];  // c = 1 tables, [(j-1) P' + k'] = T_{2 P' r}[(2 k' + 1) j], behind the m-point tables in sub.f.tw
    double2 *ek;              // [S][ek_stride]
    double *r0;               // [S][r0_stride]
    long long ek_stride, r0_stride;
};

// Dynamic LDS of the mixed-radix kernels without their twiddle tables; what is left of FM_LDS_BYTES is the tables' room.  The
// kernels carve the same bytes up (k_front_fftm, k_acqm_fwd, k_acqm_inv; k_front_fftm2):
//   one frame : image [n] double2 | hist [32] double | redv [16] double | redi [16] int | tables | 64 spare bytes
//   a pair    : images [2 n]      | hist [32]        | redv [2][16]     | redi [2][16]  | tables | 64 spare bytes
constexpr size_t fm_lds_fixed(int n) { return sizeof(double2) * (size_t)n + sizeof(double) * (32 + 16) + sizeof(int) * 16 + 64; }
constexpr size_t fm2_lds_fixed(int n) { return sizeof(double2) * 2 * (size_t)n + sizeof(double) * (32 + 32) + sizeof(int) * 32 + 64; }

// ------------------------------------------------------------------------------------------- the plan
struct FftPlan {
    int n = 0;
    FftFront kind = FRONT_NONE;
    int logn = 0;  // n = 2^logn (FRONT_POW2, or FRONT_GEN on a power of two): the radix-2 network on fft_twiddles_f64's table, no passes
    // every other frame: the Stockham passes of the transform (FRONT_FFT2X: of its m = n / 2 point halves, the leading radix 2 left out)
    int np = 0;
    int rad[FFT_MAXPASS] = {0};
    int tw_off[FFT_MAXPASS] = {0};   // pass p's table T[m] = exp(-2 pi i m / (P r)), m < P r
    int wr_off[FFT_MAXPASS] = {0};   // a prime radix above 7: W[m] = exp(-2 pi i m / r), m < r (0: none)
    int tw1_off[FFT_MAXPASS] = {0};  // FRONT_FFT2X: pass p's c = 1 table U_p (fft_plan_build)
    // the LDS kernels' pass arguments (fft_pass_args), filled once: a launcher copies them and adds the call's own
    FftmArgs args = {};
    int lds_tw_pair = 0;  // args.lds_tw of the two-frame form (k_front_fftm2)
};

// the oracle's jo_fft_mixed_radices: 4.., (2), 3.., 5.., 7.., every other prime factor ascending; frames above 9600 samples start
// with one radix-2 pass.  Returns the number of passes, 0: more than FFT_MAXPASS, or n < 2.
int fft_radices(int n, int *rad);
// the oracle's jo_fft_mixed_table: T[m] = exp(-2 pi i m / len), m < len, long double and one rounding, exact on the axes
void fft_table(double2 *t, int len);
// per-stage twiddles of the radix-2 network (the oracle's jo_fft_twiddles_f64)
void fft_twiddles_f64(std::vector<double2> &w, int n);

// Which front end serves a frame of n samples at a decimation of decim (the rule: bpsk_fftplan.hip), FRONT_NONE: none
FftFront fft_front_kind(int n, int decim, bool chan_form, int force_gen = -1);
// the predicates it is built from
bool fftm_supported(int n);   // any n of 416 .. 9600 that is not a power of two
bool fft2x_supported(int n);  // n = 2 m above 9600, m such a frame with 16 | m and no factor 7
bool acqm_supported(int n);   // the default frames 9600 / 4800 / 4410: the three-phase form of the mixed-radix kernels
bool acqg_supported(int n);   // any frame of 416 .. 2^22 samples whose prime factors r above 7 keep n r within 2^31
bool fftm_pairs(int n, int nframes);  // launch_front_fftm takes the call's frames two at a time (k_front_fftm2)
// scratch in global memory, in elements per stream (fftm, fft2x) or bytes per (stream, frame) of a launch (acqg)
size_t fftm_scratch(int n);  // n where the plan holds a prime radix above 7, else 0
size_t fft2x_scratch_ek(int n);
size_t fft2x_scratch_r0(int n);
size_t acqg_image_bytes(int n);

// The plan of a frame of n samples for the front end `kind`, its tables in w: the pass tables back to back, the r-point tables
// of the prime radices above 7 behind them, FRONT_FFT2X's c = 1 tables behind those.  false: the frame is not `kind`'s.
bool fft_plan_build(FftPlan &pl, std::vector<double2> &w, int n, FftFront kind);
// The plan of the oracle's transform of a row of n points outside FFT-acquire (the BPSK scope's spectra, bpsk_scope_spec.hip),
// kind FRONT_ROW: any n of 2 .. 9600 with at most FM_MAXPASS passes, below fftm_supported's 416 as well -- a power of two
// gets fft_twiddles_f64's table, every other n the pass tables of fft_plan_build with every table read from L2 (lds_tw = 0).
// fft_front_kind never chooses it and fftm_supported does not know of it.  false: no such plan.
bool fft_plan_build_row(FftPlan &pl, std::vector<double2> &w, int n);

// The pass arguments of the LDS kernels from a plan: rad, tw_off, wr_off, pmagic, and lds_tw -- the longest prefix of the pass
// tables that fits lds_room bytes.  false: the plan has more than FM_MAXPASS passes, or the tables of a default frame (9600 /
// 4800 / 4410) are not where the kernels' compile-time offsets (fm_forward) say -- `pair`: k_front_fftm2's split.
bool fft_pass_args(FftmArgs &aa, const FftPlan &pl, size_t lds_room, bool pair = false);

#pragma GCC visibility pop
}  // namespace jsdr
