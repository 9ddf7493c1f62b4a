// demod.h -- the demod.java chain's constants and kernel arguments, and the launchers of its three kernel units: demod.hip
// (the ordinary handle's kernels), demod_chan.hip (the channel handles') and demod_scope.hip (the scope's).  The handle's
// host units (demod_handle.h) reach the kernels through these.
#pragma once
#include "common.h"

namespace jsdr {

enum { MODE_OFF = 0, MODE_RAW = 1, MODE_AM = 2, MODE_NFM = 3, MODE_WFM = 4 };  // demod.java:39-43
constexpr int DHALO = 21;   // 20 older samples of the 21-tap filter + the FM detector's previous sample
constexpr int DTILE = 2048;
constexpr int DPER = DTILE / 256;  // 8 samples per thread and tile

// LDS image of the tile's filter input: one pad slot per 8 so that the 8-sample lane stride of the blocked
// filter walks distinct banks
__device__ __forceinline__ int xpad8(int i) { return i + (i >> 3); }

typedef float v2f __attribute__((ext_vector_type(2)));

// Java's (int) of a float -- NaN -> 0, out of range saturates, else truncation -- is what v_cvt_i32_f32 does by
// itself (C's (int) is undefined out of range, so the compiler may not assume it: spelled out, the three cases
// cost five more instructions per sample)
__device__ __forceinline__ int demod_f2i(float v)
{
    int r;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

// (short)(sam * 32767f) to both channels (:478-481): the low half of the int, twice
__device__ __forceinline__ int demod_lr(float x) { const int sv = demod_f2i(x * 32767.0f); return (int)__builtin_amdgcn_perm((unsigned)sv, (unsigned)sv, 0x01000100u); }

// ---- the ordinary handle's kernels (demod.hip)
struct DemodArgs;  // demod_dev.h
// k_demod_fused (fused: every mode but AM, frames of up to 5 tiles -- raw samples to int16 audio at out, the frames' (max, avg)
// to stats) or k_demod_front (one tile per workgroup to a.d, a.fmax_bits zeroed before)
int launch_demod_front(const DemodArgs &a, bool f32in, bool fused, int nstreams, int *out, long long out_stride_pairs,
                       float *stats, hipStream_t st);
int launch_demod_state(const DemodArgs &a, bool f32in, float2 *hist_new, float2 *lilq_new, int nstreams, hipStream_t st);
// the unfused form's second pass: a.d, a.fmax_bits and favg (k_demod_mean's, AM) to int16 audio
int launch_demod_out(const DemodArgs &a, int nstreams, const float *favg, int *out, long long out_stride_pairs, float *stats,
                     hipStream_t st);
// both kinds of handle: (cos, sin) of n carrier phases; the AM mean of nframes_total frames of n floats in rows of L
int launch_demod_nco(const float *car, long long n, float2 *nco, hipStream_t st);
int launch_demod_mean(const float *d, long long L, int n, int nfr, long long nframes_total, float *favg, hipStream_t st);

// ---- channel handles (jsdr_demod_create_channels): ninputs x K receivers, channel c of input i is stream i * K + c
enum { DCHAN_MAX = 16 };

struct DemodChanConst {
    float w[21];
    float fmgain;
    int mode, dofir, dodwn, doagc;
    int nco_row;  // row of the call's carrier table (dodwn)
    int dslot;    // slot of this channel's float rows in d (AM, or every channel of a long frame); -1: none
};

struct DemodChanArgs {
    const int *raw;            // int16 pairs [ninputs][stride_pairs]
    const float2 *rawf;        // or float pairs
    long long stride_pairs;    // between INPUTS
    long long L;               // samples per input in this call
    int n, nfr, ic, qc;
    int ninputs, K;
    const float2 *hist;        // [ninputs * K][21] filter input before the call
    const float2 *lilq;        // [ninputs * K] FM detector state before the call
    const float2 *nco;         // [rows][nco_pitch] (cos, sin) of each distinct carrier table
    long long nco_pitch;
    float *d;                  // [dslots * ninputs][L], row dslot * ninputs + i
    unsigned *fmax_bits;       // [dslots * ninputs][nfr]
    int *out;                  // int16 (L,R) pairs, row i * K + c
    long long out_stride_pairs;
    float *stats;              // [ninputs * K][nfr] (max, avg)
    int slot_chan[DCHAN_MAX];  // channel of each dslot
    DemodChanConst c[DCHAN_MAX];
};

// k_demod_chan (frames of up to 5 tiles: one workgroup per frame of one input) or k_demod_chan_front (one per tile, every
// channel to d); then k_demod_chan_state
int launch_demod_chan(const DemodChanArgs &a, bool f32in, bool fused, hipStream_t st);
int launch_demod_chan_state(const DemodChanArgs &a, bool f32in, float2 *hist_new, float2 *lilq_new, hipStream_t st);
// the AM mean subtraction / AGC / int16 output of the d rows (favg: k_demod_mean's result for the AM rows)
int launch_demod_chan_out(const DemodChanArgs &a, int drows, const float *favg, hipStream_t st);

// ---- the demod scope (jsdr_demod_scope_*, demod_scope.hip): demod.paintComponent's trace and spectrum (:509-558) per frame
constexpr int DSCOPE_WIDTH_MAX = 32768;
constexpr size_t DSCOPE_SCRATCH_BYTES = (size_t)64 << 20;  // the handle's rows of one pass: dbg, final floats and PSD together

// the two column schedules in the reference's float arithmetic, one statement each: host (jsdr_demod_scope_layout) and device
// (k_demod_scope_layout) round the one product alike
__host__ __device__ inline int dscope_trace_first(int x, float scale) { return (int)((float)x * scale); }  // :527
__host__ __device__ inline int dscope_spec_first(int m, float pi) { return (int)(pi * (float)m); }         // :550
inline float dscope_scale(int n, int width) { return (float)(n / width); }                                  // :519
inline float dscope_pi(int n, int width) { return (float)n / (float)width; }                                // :544

// tab = int[4][width]: trace_first, trace_count, spec_first, spec_count (jsdr_demod_scope_layout's four arrays), filled on `st`
int launch_demod_scope_layout(int n, int width, int *tab, hipStream_t st);
// rows [row0, row0 + nrows) of the call `a` describes (row = stream * a.nfr + frame; a.hist / a.lilq / a.nco as they were
// BEFORE the call, stats = its (max, avg) rows): the mixed IQ to dbg_rows[nrows][n], the final floats to fin_rows[nrows][n]
// (may be null)
int launch_demod_scope_front(const DemodArgs &a, bool f32in, const float *stats, long long row0, int nrows, float2 *dbg_rows,
                             float *fin_rows, hipStream_t st);
// trace_rows[nrows][width] from the final floats and the Qs (mode_off: every Q is 0); quarter = H/4
int launch_demod_trace(const float *fin_rows, const float2 *dbg_rows, int n, bool mode_off, int nrows, int width, int quarter,
                       const int *tab, int32_t *trace_rows, hipStream_t st);
// spec_rows[nrows][width] from PSD rows of n + 2 floats; half = H/2
int launch_demod_spec(const float *psd_rows, int n, int nrows, int width, int half, const int *tab, int32_t *spec_rows,
                      hipStream_t st);

}  // namespace jsdr
