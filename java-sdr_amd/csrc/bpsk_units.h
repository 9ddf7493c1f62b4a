// bpsk_units.h -- what the tune-mode pipeline's translation units (bpsk_front.hip, bpsk_front_reg.hip, bpsk_fm.hip,
// bpsk_fm_f32.hip, bpsk_tail.hip) share beyond bpsk_kernels.h.  Internal to those five: the handle sees bpsk_kernels.h only.
//
// The build has no relocatable device code, so a __constant__ object cannot be shared between units: each unit whose kernels
// read the tables holds its own copy, `namespace <unit> { __constant__ BpskConst c_bpsk; }` -- the whole struct, so a field
// sits at the same offset in every unit -- and fills it in its part of bpsk_upload_constants() below.  The copies are kept
// apart by the unit's namespace and not by `static`: the compiler addresses an internal-linkage __constant__ object that
// host code names (hipMemcpyToSymbol) through the GOT, one more scalar load at every site that reads it, where an
// external one is reached pc-relative -- the kernels' code as it was in one unit.  (bpsk_front_reg.hip has no copy:
// k_front_reg's taps are compile-time constants, ds_tap().)
#pragma once
#include "bpsk_kernels.h"

namespace jsdr {

#define JSDR_WAVE_SYNC()                                      \
    do {                                                      \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                      \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)

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

// each unit's part of the two calls that span the units: bpsk_upload_constants() and bpsk_debug_clocks_report() are in
// bpsk_tail.hip and call these (hidden: the library exports what it exported as one unit)
__attribute__((visibility("hidden"))) int bpsk_front_upload_constants(const BpskConst &bc);
__attribute__((visibility("hidden"))) int bpsk_fm_upload_constants(const BpskConst &bc);
__attribute__((visibility("hidden"))) int bpsk_fm_f32_upload_constants(const BpskConst &bc);
__attribute__((visibility("hidden"))) void bpsk_fm_clocks_report();  // JSDR_X_CLK

// bpsk_front_reg.hip's launcher as bpsk_front.hip's launch_front calls it (instantiated there for the four rates)
template <int D, int RD>
__attribute__((visibility("hidden"))) bool launch_front_reg(const FrontArgs &fa, int nstreams, long long nds, bool fast, hipStream_t st);

}  // namespace jsdr
