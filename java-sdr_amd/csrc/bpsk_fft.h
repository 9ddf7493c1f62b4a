// bpsk_fft.h -- interface of the FFT-acquire front ends (bpsk_fft.hip, bpsk_acq*.hip, bpsk_fftm*.hip, bpsk_fft2x.hip) used by
// the pipeline host code (bpsk_handle.h's units), and the frame stages their kernels share
#pragma once
#include "bpsk_acq_rule.h"
#include <vector>

namespace jsdr {

struct FftFrontState {
    double avePeakPower;   // :403
    double aveCentreBin;   // :404
    int centreBin;         // :405
    int pad;
    double hist[26];       // the 26 values fed to RxDownSample before the next frame (re of the inverse FFT)
};

struct FftFrontArgs {
    const int *raw;            // int16 pairs, [S][stride]
    const float2 *rawf;        // or float frames
    long long stride_pairs;
    int nframes;               // frames in this call
    int n, logn;               // samples per frame
    int ic, qc;
    int do_up;
    int decim;
    int first_out;             // input index (within the call) that completes output 0
    const double2 *vco_cs;     // [nds] (cos, sin) of the VCO phase table entry of every decimated sample
    const double2 *tw;         // [n-1] per-stage (cos, -sin), fft_twiddles_f64
    FftFrontState *st;         // [S]
    double2 *dm;               // [S][dm_stride]
    long long dm_stride;
    long long nds;
    const double *ds_taps;     // [27]
    long long *phase_clk;      // diagnostics: [8] cycle counts per phase of stream 0's workgroup, or null
};

// dsFilter (FUNcubeBPSKDemod.java:27-55, symmetric: first 14 of 27), device-side copy with a static initialiser:
// indexed with compile-time constants in the front-end kernels, so the taps fold into the instruction stream (14
// distinct values) instead of occupying 54 SGPRs or an LDS read per multiply
static __constant__ constexpr float kDsHalf[14] = {-6.103515625000e-004F, -1.220703125000e-004F, +2.380371093750e-003F,
                                        +6.164550781250e-003F, +7.324218750000e-003F, +7.629394531250e-004F,
                                        -1.464843750000e-002F, -3.112792968750e-002F, -3.225708007813e-002F,
                                        -1.617431640625e-003F, +6.463623046875e-002F, +1.502380371094e-001F,
                                        +2.231445312500e-001F, +2.518310546875e-001F};
__device__ __forceinline__ double ds_tap(int n) { return (double)kDsHalf[n < 14 ? n : 26 - n]; }
// bit n: tap n is +-2^k, so a product with it is exact and `a + d*tap` is the same double as fma(d, tap, a) -- which the
// exact-order filters (-ffp-contract=off) then write themselves (k_fm).  Derived from the table: today taps 1 and 25 (-2^-13).
constexpr unsigned ds_pow2_mask()
{
    unsigned mask = 0;
    for (int n = 0; n < 27; n++) {
        float v = kDsHalf[n < 14 ? n : 26 - n];
        v = v < 0 ? -v : v;
        if (v == 0) continue;
        while (v < 1) v *= 2;
        while (v >= 2) v /= 2;
        if (v == 1) mask |= 1u << n;
    }
    return mask;
}
constexpr unsigned kDsPow2Mask = ds_pow2_mask();
static_assert(kDsPow2Mask == ((1u << 1) | (1u << 25)), "dsFilter: taps 1 and 25 are the powers of two");

// Two adjacent 100-wide boxcar sums from the same 51 aligned 16-byte reads w[0..50] (w[0].x = P[i-50]):
//   a0 = P[i-50] + ... + P[i+49],  a1 = P[i-49] + ... + P[i+50], each in ascending order (:433-437).
// The window comes in chunks of 8 reads, the next chunk in flight while the current one is summed: as a plain loop
// the compiler waits for every read before its four additions (fifty LDS latencies per pair); left alone with the
// unrolled loop it hoists all 51 reads (204 registers, spilled).  Chunk C is a template parameter so that every
// register index is a compile-time constant.
template <int C>
__device__ __forceinline__ void boxcar_chunk(const double2 *w, const double2 (&cur)[8], double &a0, double &a1, double &prev_y)
{
    constexpr int NCH = 7;  // 7 chunks of 8 cover w[0..50]
    double2 nxt[8];
    if constexpr (C + 1 < NCH) {
#pragma unroll
        for (int u = 0; u < 8; u++)
            if ((C + 1) * 8 + u <= 50) nxt[u] = w[(C + 1) * 8 + u];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int k = C * 8 + u;  // element w[k]
        if (k <= 50) {
            const double2 e = cur[u];
            if (k >= 1) {
                a0 += prev_y;
                a1 += prev_y;
            }
            if (k < 50) a0 += e.x;
            if (k >= 1) a1 += e.x;
            prev_y = e.y;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (C + 1 < NCH) boxcar_chunk<C + 1>(w, nxt, a0, a1, prev_y);
}

__device__ __forceinline__ void boxcar_pair(const double2 *w, double &a0, double &a1)
{
    double2 first[8];
#pragma unroll
    for (int u = 0; u < 8; u++) first[u] = w[u];
    double prev_y = 0.0;
    a0 = 0.0;
    a1 = 0.0;
    boxcar_chunk<0>(w, first, a0, a1, prev_y);
}

// The wave's FIRST MAXIMUM of the boxcar search (:439-442): every lane brings its own best (value > 0 at index >= 0, or 0.0 at -1);
// out comes, in every lane, the largest value and the LOWEST index that holds it (or 0.0 / -1).  DPP row shifts and row broadcasts
// (an instruction each) instead of __shfl_xor's round trips through the LDS crossbar: a 64-lane reduction of (double, int) by
// shuffles is 18 dependent ds_bpermute, ~2000 cycles with nothing to cover them -- twice a frame in the mixed-radix front ends.
__device__ __forceinline__ void wave_first_max(double &bestv, int &besti)
{
    double v = bestv;
#define JSDR_DPP_MAX(ctrl, rmask)                                                                                \
    {                                                                                                             \
        const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), ctrl, rmask, 0xf, false); \
        const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), ctrl, rmask, 0xf, false); \
        v = fmax(v, __hiloint2double(hi, lo));                                                                    \
    }
    JSDR_DPP_MAX(0x111, 0xf)  // row_shr:1
    JSDR_DPP_MAX(0x112, 0xf)  // row_shr:2
    JSDR_DPP_MAX(0x114, 0xf)  // row_shr:4
    JSDR_DPP_MAX(0x118, 0xf)  // row_shr:8 -- lane 15 of every row holds its row's maximum
    JSDR_DPP_MAX(0x142, 0xa)  // row_bcast:15 into rows 1 and 3
    JSDR_DPP_MAX(0x143, 0xc)  // row_bcast:31 into rows 2 and 3 -- lane 63 holds the wave's
#undef JSDR_DPP_MAX
    const double mv = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
    // the lowest index among the lanes that hold it (a lane's index ascends with its rounds, not with the lane: no "first lane" here)
    int c = (besti >= 0 && bestv == mv) ? besti : 0x7fffffff;
#define JSDR_DPP_MIN(ctrl, rmask)                                                    \
    {                                                                                 \
        const int o = __builtin_amdgcn_update_dpp(c, c, ctrl, rmask, 0xf, false);    \
        c = o < c ? o : c;                                                            \
    }
    JSDR_DPP_MIN(0x111, 0xf)
    JSDR_DPP_MIN(0x112, 0xf)
    JSDR_DPP_MIN(0x114, 0xf)
    JSDR_DPP_MIN(0x118, 0xf)
    JSDR_DPP_MIN(0x142, 0xa)
    JSDR_DPP_MIN(0x143, 0xc)
#undef JSDR_DPP_MIN
    const int mi = __builtin_amdgcn_readlane(c, 63);
    bestv = mi == 0x7fffffff ? 0.0 : mv;
    besti = mi == 0x7fffffff ? -1 : mi;
}

// ---- the frame stages every FFT-acquire front end shares (bpsk_fft.hip, bpsk_fftm.hip and its siblings, bpsk_acq*.hip); the scalar rules they
// step are bpsk_acq_rule.h's

// :416-421 -- a sample of the frame as the transform's input: (double) of JavaAudio's float sample, int16 words with the
// DC corrections ic / qc added as Java shorts
__device__ __forceinline__ double2 acq_sample(int w, int ic, int qc)
{
    return make_double2((double)i16_to_float_java(java_short_add((int)(short)(w & 0xffff), ic)),
                        (double)i16_to_float_java(java_short_add(w >> 16, qc)));
}
__device__ __forceinline__ double2 acq_sample(const float2 w)
{
    return make_double2((double)w.x, (double)w.y);
}

// One step of the boxcar search (:433-442): the pair of sums (boxcar_pair) at i (even) and i + 1, stored to ai[0] and ai[1]
// where they lie in [beg + 75, end - 75), and the thread's first maximum brought up to date (i ascends within a thread).
__device__ __forceinline__ void boxcar_put(double a0, double a1, double *ai, int i, int beg, int end, double &bestv, int &besti)
{
    asm volatile("" : "+v"(a0), "+v"(a1));  // due here: sunk into the conditional uses below, the sums drag all 51 reads along
    if (i >= beg + 75) {
        ai[0] = a0;
        first_max_update(bestv, besti, a0, i);
    }
    if (i + 1 < end - 75) {
        ai[1] = a1;
        first_max_update(bestv, besti, a1, i + 1);
    }
}

// The workgroup's first maximum (maxBin, binPos), uniform, from its NW waves' in (redv, redi)[wave] behind a workgroup barrier:
// they meet in lanes 0 .. NW - 1 of every wave (the same combine: larger value, then smaller index; an empty candidate never
// wins) -- as an NW-step loop run by every thread this cost the SIMDs 3.6k cycles a frame at NW = 12.
template <int NW>
__device__ __forceinline__ void wg_first_max(const double *redv, const int *redi, int lane, double &maxBin, int &binPos)
{
    double mv = 0.0;
    int mi = -1;
    if (lane < NW) {
        mv = redv[lane];
        mi = redi[lane];
    }
    wave_first_max(mv, mi);
    maxBin = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(mv)), __builtin_amdgcn_readfirstlane(__double2loint(mv)));
    binPos = __builtin_amdgcn_readfirstlane(mi);
}

// RxDownSample (:470-492) for the window that ends at w[0], newest first (:479-483): 27 samples at w[0], w[-1], ..
__device__ __forceinline__ double ds_sample(const double &x) { return x; }
__device__ __forceinline__ double ds_sample(const double2 &x) { return x.x; }  // the real parts of an image
template <class T>
__device__ __forceinline__ double ds_window(const T *w)
{
    double fi = 0.0;
#pragma unroll
    for (int k = 0; k < 27; k++) fi += ds_sample(w[-k]) * ds_tap(k);
    return fi;
}
// The same from the COMPACT samples of a frame -- sample t at double slot rb0 + t of Rb, the previous frame's last 26 in front
// of them, so that every window is one contiguous run -- for the window that ends at sample e.  With an even decimation
// (even_d) every window of a call ends on the same parity par = (first_out - t0) & 1 (frames are even): the 27 samples
// e - 26 .. e are 14 aligned 16-byte reads, d[i] = slot ((e + rb0 - 26) & ~1) + i.
__device__ __forceinline__ double ds_window_compact(const double *Rb, int rb0, int e, bool even_d, int par)
{
    double fi = 0.0;
    if (even_d) {
        const double2 *w2 = reinterpret_cast<const double2 *>(Rb + ((e + rb0 - 26) & ~1));
        double d[28];
#pragma unroll
        for (int i = 0; i < 14; i++) {
            const double2 t = w2[i];
            d[2 * i] = t.x;
            d[2 * i + 1] = t.y;
        }
        if (par) {
#pragma unroll
            for (int k = 0; k < 27; k++) fi += d[27 - k] * ds_tap(k);  // newest first (:479-483)
        } else {
#pragma unroll
            for (int k = 0; k < 27; k++) fi += d[26 - k] * ds_tap(k);
        }
    } else {
        const double *w = Rb + (rb0 + e);
#pragma unroll
        for (int k = 0; k < 27; k++) fi += w[-k] * ds_tap(k);
    }
    return fi;
}

// the three numbers a stream carries from frame to frame (:403-405)
__device__ __forceinline__ void acq_state_load(const FftFrontState *sp, double &avePeakPower, double &aveCentreBin, int &centreBin)
{
    avePeakPower = sp->avePeakPower;
    aveCentreBin = sp->aveCentreBin;
    centreBin = sp->centreBin;
}
__device__ __forceinline__ void acq_state_store(FftFrontState *sp, double avePeakPower, double aveCentreBin, int centreBin)
{
    sp->avePeakPower = avePeakPower;
    sp->aveCentreBin = aveCentreBin;
    sp->centreBin = centreBin;
}

// diagnostics (JSDR_FFT_PHASECLK=1; never in the product's default path): the thread for which `timing` holds accumulates the
// clock ticks of every phase in acc[] (LDS); `tprev` is the tick the phase began at
#define ACQ_PHASE(acc, k)                            \
    if (timing) {                                    \
        const long long now_ = (long long)clock64(); \
        acc[k] += now_ - tprev;                      \
        tprev = now_;                                \
    }

int launch_front_fft(const FftFrontArgs &a, int nstreams, hipStream_t st);
// round 6 (bpsk_acq.hip): the same front end in three phases -- forward transform + boxcar per frame, one scan per stream,
// inverse transform + RxDownSample per frame -- for calls of two or more frames per stream; frames of 1024 .. 8192 samples
bool acq3_supported(int n);
size_t acq3_frame_bytes(int n, int do_up);  // scratch per (stream, frame) of one launch
// what the phases hand each other, per frame id g = s * F + f (F = frames per stream in this launch)
struct AcqPeak {
    double maxBin;
    int binPos;
    int pad;
};

struct AcqArgs {
    const int *raw;        // int16 pairs [S][stride]
    const float2 *rawf;    // or float frames
    long long stride_pairs;
    int ic, qc;
    int S, F, f0;          // streams, frames per stream in this launch, index of its first frame within the call
    int n, do_up, decim;
    long long first_out, nds;
    const double2 *vco_cs;
    const double2 *tw;
    FftFrontState *st;
    double2 *dm;
    long long dm_stride;
    double2 *spec;         // [S F][nsb]: do_up ? bins [0, 204) then [n/4 - 26, n/2 + 28) : bins [0, max(n/4 + 28, 204))
    int nsb;
    double *aband;         // [S F][na]: boxcar sums over [beg + 75, end - 75)
    int na;
    AcqPeak *peak;         // [S F]
    int *cbin;             // [S F] the frame's centre bin (phase B)
    double *edges;         // [S F][52]: the frame's first 26 and last 26 real samples re / n (phase C)
    int nwg;               // persistent workgroups of phases A and C
    unsigned *tickets;     // [2] run counters of k_acq_fwd / k_acq_inv, zero at launch: a workgroup takes its frames in runs of `run`
    int run;               // consecutive frames per ticket (>= 2)
    int rps;               // runs per stream = ceil(F / run): a run lies inside one stream
    long long *clk;        // diagnostics (JSDR_FFT_PHASECLK=1): [16] clock ticks per phase of workgroup 0, k_acq_fwd [0..7], k_acq_inv [8..15]; or null
};

// where bin b of a frame sits in its spec row, or -1
__device__ __forceinline__ int acq_spec_index(int b, int n, int do_up)
{
    if (!do_up) return b < n / 4 + 28 ? b : -1;
    if (b < 204) return b;
    const int lo = n / 4 - 26;
    return (b >= lo && b < n / 2 + 28) ? 204 + (b - lo) : -1;
}

// The frame's plan (bpsk_fftplan.h: the front end that serves it, its passes, its tables' offsets, fixed at create) comes with
// every launch below that is not the power-of-two kernels' own; which frames each front end takes: fft_front_kind there.
struct FftPlan;
// the default mixed-radix frames (9600 / 4800 / 4410) in the same three phases: bpsk_fftm.hip has the two frame-parallel kernels
// (which 0: k_acqm_fwd, 1: k_acqm_inv), built from k_front_fftm's passes
int launch_acqm(const AcqArgs &a, const FftFrontArgs &fa, const FftPlan &pl, int num_cu, int which, hipStream_t st);
// per-phase timing hook (bench.py's per-kernel figures): phase 0..3 = k_acq_fwd, k_acq_scan, k_acq_inv, k_acq_edges
struct AcqProf {
    void *ctx = nullptr;
    void (*mark)(void *ctx, int phase, bool begin, hipStream_t st) = nullptr;
};
// ANY other frame (bpsk_acqg.hip, a FRONT_GEN plan): phases A and C with the frame's image in global memory, one launch per pass
// of the oracle's transform -- powers of two outside 1024 .. 8192, frames above 9600 samples that are not twice a 16 | m,
// 2^a 3^b 5^c one (17640, 38400), and the LDS front ends' frames at the decimations they do not take; its scratch per (stream,
// frame) of one launch: acqg_image_bytes on top of acq3_frame_bytes
int launch_acqg(const AcqArgs &a, const FftPlan &pl, double2 *img, int which, hipStream_t st);
int launch_acq3(const FftFrontArgs &a, int nstreams, unsigned char *scratch, size_t scratch_bytes, int chunk_frames, int num_cu,
                hipStream_t st, const AcqProf &prof, const FftPlan &plan);
// the channel handle's form (bpsk_acq_chan.hip): the forward phase once per INPUT and frame, scan / inverse / edges once per FFT
// channel over that channel's streams (one per input), by the same kernels through strided arguments
enum { ACQ_PART_FWD = 1, ACQ_PART_SCAN = 2, ACQ_PART_INV = 4, ACQ_PART_EDGES = 8, ACQ_PARTS_ALL = 15 };
void acq3_row_layout(int n, int do_up, int *nsb, int *na);
int launch_acq3_parts(AcqArgs &a, const FftFrontArgs &fa, int parts, int num_cu, hipStream_t st, const AcqProf &prof, const FftPlan &plan,
                      double2 *img);
struct AcqChanArgs {
    int nin = 0, nch = 0;      // inputs, channels per input: stream = input * nch + channel
    int nfft = 0;              // FFT-acquire channels ...
    int chan[16] = {0};        // ... which they are ...
    int up[16] = {0};          // ... and the band each searches (doUp)
    FftFrontState *st = nullptr;  // [nch][nin]: CHANNEL-major, so that one channel's streams are consecutive
    // a live channel handle's call in which FFT channel k carries the tune -> FFT-acquire seam: the Q column of the tune path's
    // history, [nin][26] (k_chan_seam_hist), and the outputs of the call's first frame whose windows reach into it (k_acq_edges_seam)
    const double *seam_q[16] = {nullptr};
    int seam_J = 0;
    long long fwd_frames = 0, inv_frames = 0;  // out: frames transformed forward / inverted by the call
    const char *fwd_name = "";                 // out: the forward kernel
};
size_t acq3c_frame_bytes(int n, int band_mask, bool generic);  // scratch per (input, frame) of one launch
int launch_acq3_chan(const FftFrontArgs &fa, AcqChanArgs &ca, unsigned char *scratch, size_t scratch_bytes, int chunk_frames, int num_cu,
                     hipStream_t st, const AcqProf &prof, const FftPlan &plan);
extern int g_acq_last_grid[4];  // workgroups of the last k_acq_fwd / k_acq_inv launch, and how many of each a CU holds
// frames that are not a power of two (bpsk_fftm.hip, a FRONT_FFTM plan): any n with 416 <= n <= 9600 (2^a 3^b 5^c 7^d through the
// radix passes, any other prime factor through a pass that is the DFT's definition and needs fftm_scratch(n) elements of scratch
// per stream, gscratch); a call that fftm_pairs takes goes on to launch_front_fftm2 (bpsk_fftm2.hip: two frames at a time)
int launch_front_fftm(const FftFrontArgs &a, const FftPlan &pl, double2 *gscratch, int nstreams, hipStream_t st);
int launch_front_fftm2(const FftFrontArgs &a, const FftPlan &pl, int nstreams, hipStream_t st);
// frames of 2 m samples, m an LDS-sized mixed-radix frame (n = 19200 at 192 kHz; bpsk_fft2x.hip, a FRONT_FFT2X plan): two m-point
// halves per transform, fft2x_scratch_ek / _r0 elements of scratch per stream
int launch_front_fft2x(const FftFrontArgs &a, const FftPlan &pl, double2 *ek, double *r0, int nstreams, hipStream_t st);

}  // namespace jsdr
