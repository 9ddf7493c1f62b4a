// bpsk_fm.hip -- tune mode, the matched filter: 65 taps in RING-SLOT order with rotated taps
// (FUNcubeBPSKDemod.java:519-523) -> y[s][j] = (fi,fq).
//
//   k_matched     : from the dm rows the front end (bpsk_front.hip) wrote;  k_dm_history: the 64 samples kept between calls
//   k_fm          : front end and matched filter in ONE kernel, the default for int16 input with a periodic tuner schedule
//   k_fm_prep, k_fm_edges : the stream's edge images and the input history for k_fm
// and their launchers (bpsk_kernels.h), and the JSDR_X_CLK timing probe's counters.
//
// One of the four units of the tune-mode pipeline, which is cut by kernel family so that an edit to one family recompiles
// that family only: bpsk_front.hip, bpsk_front_reg.hip, bpsk_fm.hip, bpsk_tail.hip (the pipeline's overview is at the top
// of the last).  Compiled with -ffp-contract=off.  Reads dm_taps of its copy of the tables (matched_block, k_fm's
// short-call matched half).
#include "bpsk_units.h"
#include "bpsk_tuner.h"  // the 8-phase tuner's factor classes (k_fm's PH forms)
#include <math.h>
#include <type_traits>
#include <stddef.h>
#include <stdlib.h>

namespace jsdr {
namespace fm { __constant__ BpskConst c_bpsk; }  // this unit's copy of the tables, under this unit's name (bpsk_units.h)
using fm::c_bpsk;
}  // namespace jsdr
#include "bpsk_matched.h"  // matched_block: k_matched's and k_fm's 65-tap filter, shared with bpsk_fm_f32.hip

namespace jsdr {


template <bool FAST>
__global__ __launch_bounds__(512) void k_matched(MatchedArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *X = reinterpret_cast<double2 *>(smem);  // [64 + 4160]: X[i] = sample (G - 64 + i)
    const int s = blockIdx.y;
    const long long G = a.tile0 + 4160LL * blockIdx.x;
    const double2 *dm = a.dm + (long long)s * a.dm_stride;
    {
        // all nine loads of a thread are in flight before the first LDS store: as a plain loop the compiler issues
        // one load, waits for it, stores, and pays the full memory latency nine times per workgroup
        constexpr int NLD = (64 + 4160 + 511) / 512;
        double2 v[NLD];
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            const int i = threadIdx.x + 512 * q;
            const long long rel = (G - 64 + i) - a.g_first;  // index relative to the first new sample
            const bool in = i < 64 + 4160 && rel >= -64 && rel < a.nds;
            // clamped address, masked value: no branch between the loads
            const double2 x = dm[64 + (in ? rel : 0)];
            v[q] = in ? x : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            const int i = threadIdx.x + 512 * q;
            if (i < 64 + 4160) X[i] = v[q];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double2 *xl = X + 64 + 65 * lane;  // &X[s0]
    const long long s0 = G + 65LL * lane;
    double2 *y = a.y + (long long)s * a.y_stride;
    if (wave == 0) {
        double ai[9], aq[9];
        matched_block<9, FAST>(xl, 0, ai, aq);
#pragma unroll
        for (int r = 0; r < 9; r++) {
            long long rel = s0 + r - a.g_first;
            if (rel >= 0 && rel < a.nds) y[rel] = make_double2(ai[r], aq[r]);
        }
    } else {
        const int u0 = 9 + 8 * (wave - 1);
        double ai[8], aq[8];
        matched_block<8, FAST>(xl, u0, ai, aq);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            long long rel = s0 + u0 + r - a.g_first;
            if (rel >= 0 && rel < a.nds) y[rel] = make_double2(ai[r], aq[r]);
        }
    }
}

// keep the last 64 VCO-mixed samples as the next call's history (one wave per stream; loads before stores)
__global__ __launch_bounds__(64) void k_dm_history(double2 *dm, long long dm_stride, long long nds, int nstreams)
{
    int s = blockIdx.x;
    if (s >= nstreams) return;
    double2 *p = dm + (long long)s * dm_stride;
    double2 v = p[nds + threadIdx.x];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    p[threadIdx.x] = v;
}

// ------------------------------------------------------------------------------------------- k_fm
// Front end and matched filter in ONE kernel: int16 IQ -> tuner mix -> 27-tap /D low-pass -> x HOWARD -> VCO mix
// (k_front_reg's arithmetic) -> 65-tap matched filter in ring-slot order (k_matched's) -> y = (fi,fq).  The VCO-mixed
// 9600 Hz samples of a tile never leave the CU: the front half writes them into the LDS image the matched filter
// reads (16 B per 9600 Hz sample that used to go to HBM and come back: 3.4 GB per 1024 x 2^20 batch), and the
// 1 B/sample tuner-index stream is gone as well -- the tuner table index is periodic in the sample number (an
// exact 8-cycle at 12 kHz / 96 kHz; the host verifies the period over every sample of the call), so the (cos, sin)
// pair of window sample m sits at a COMPILE-TIME offset from a tile-uniform base in an unwrapped table: scalar
// loads, SGPR operands, no per-sample index arithmetic and no LDS lookups.
//
//   tile   : NB = 62 blocks of 65 outputs (k_matched's lane = block mapping) + 64 samples of halo = 4094 VCO-mixed
//            samples = 65.5 KB of LDS; 512 threads; two workgroups per CU.
//   front  : 1024 jobs of R = 4 outputs (two rounds of 512 threads, 99.9 % of the lanes busy); a lane reads ITS
//            OWN 57-sample window with 4-byte aligned 16-byte loads, newest quad first, converts I and Q of a
//            sample together (packed FP32: the same IEEE operations as the scalar form, two per instruction) and
//            walks newest -> oldest with the R accumulator pairs in registers (:479-483).  The halo is recomputed
//            (1.6 %); before the call's first sample it comes from the 64 samples the previous call saved.  Windows
//            that reach into the previous call's 26 samples or past the last sample are read from the stream's edge
//            images (k_fm_edges) with the same loads, so every job -- edge or not -- takes the same arithmetic in the
//            same pass; the VCO table indices come in with the window and their table reads are issued under the last
//            quad's arithmetic.
//   matched: as k_matched, from the LDS image.
// (Compile-time timing probes, never defined in the product build (java-sdr_amd/build.py): each of them only REMOVES
// work -- a half of the kernel, a load, a store, a barrier -- and none changes an address that is still accessed; the
// one probe that did (JSDR_X_COAL, round 2) faulted and was deleted.  A probe that needs "wrong data" keeps the
// kernel's own bounds.)
// Where the time goes (2048 streams x 2^20 samples, alone, tools/build_define.sh with -DJSDR_X_NOFRONT / _NOMATCHED /
// _CLK): front half 2.15 ms + matched half 2.12 ms = the kernel's 4.3-4.4 ms; the matched half issues FP64 at ~95 % of
// the chip's measured rate, the front half at ~80 % (1.94 ms with its window loads replaced by constants: the loads'
// latency costs a tenth of it); coalesced window addresses or a register-resident tuner table change nothing.
// Every floating-point operation and its order are those of k_front_reg + k_matched (FAST = false), so (fi,fq)
// stay bit-identical to the reference.  Used when the input is int16, the tuner schedule is periodic with a period
// that divides the lane span (or the tuner is off, tuning <= 0); everything else takes the three-kernel path.

#ifdef JSDR_X_CLK  // timing experiment: s_memtime ticks (10 ns) per phase, summed over every wave of the launch
__device__ unsigned long long g_fm_clk[256][64];  // [blockIdx & 255][phase]: same-address atomics serialise
#define FM_CLK(i)                                                                          \
    do {                                                                                   \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                      \
        clk_acc_[i] += now_ - clk_last_;                                                   \
        clk_last_ = now_;                                                                  \
    } while (0)
#else
#define FM_CLK(i) do {} while (0)
#endif

#ifdef JSDR_X_WGCLK  // timing probe: every workgroup's first and last s_memrealtime tick (10 ns, one clock for the chip) and its tiles, a row per launch
constexpr int WGCLK_SLOTS = 128, WGCLK_WGS = 1024;
__device__ unsigned long long g_fm_wgclk[WGCLK_SLOTS][WGCLK_WGS][3];
static long long g_wgclk_log[WGCLK_SLOTS][4];  // per launch row: tiles, grid, ticket form, launch number
#endif

// The stream's edge images for k_fm: E[0 .. 2*FM_EDGE) = samples -FM_EDGE .. FM_EDGE-1, E[2*FM_EDGE .. 4*FM_EDGE) = samples
// L-FM_EDGE .. L+FM_EDGE-1 as raw int16 pairs: the previous call's 26 samples before sample 0 (kept DC-corrected: the
// correction is taken off again, k_fm's conversion re-applies it -- 16-bit wrap-around both ways, so exactly the stored
// value), zero before them and beyond the last sample.
__global__ void k_fm_edges(EdgeArgs a)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = t / (4 * FM_EDGE), i = t % (4 * FM_EDGE);
    if (s >= a.nstreams) return;
    const int n = i < 2 * FM_EDGE ? i - FM_EDGE : a.nsamples - FM_EDGE + (i - 2 * FM_EDGE);
    int w = 0;
    if (n >= 0 && n < a.nsamples) {
        w = a.raw[(long long)s * a.stride_pairs + n];
    } else if (n < 0 && n >= -26) {
        w = a.hist[(long long)s * 32 + 26 + n].x;
        if (a.dc) {
            const int si = (int)(short)((w & 0xffff) - a.ic);
            const int sq = (int)(short)((w >> 16) - a.qc);
            w = (si & 0xffff) | (sq << 16);
        }
    }
    a.edges[(long long)s * (4 * FM_EDGE) + i] = w;
}

// k_fm_edges and k_hist_in in ONE launch (the k_fm path): both only read the call's input and the previous call's history,
// and write disjoint buffers (the edge images, the next call's history) -- one dependent launch less per call.
// ... and, in the receive() form, the schedule's tables: they travel behind the frame in ONE host->device copy and are put
// where the kernels read them here (two byte ranges at most: the VCO indices and the unwrapped tuner table).
__global__ void k_fm_prep(EdgeArgs e, HistArgs hi, ScatterArgs sc)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int nedge = e.nstreams * 4 * FM_EDGE;
    {
        const int v = t - nedge - 32 * e.nstreams;
        if (v >= 0) {
            if (v < sc.bytes[0]) sc.dst[0][v] = sc.src[0][v];
            else if (v - sc.bytes[0] < sc.bytes[1]) sc.dst[1][v - sc.bytes[0]] = sc.src[1][v - sc.bytes[0]];
            return;
        }
    }
    if (t < nedge) {
        const int s = t / (4 * FM_EDGE), i = t % (4 * FM_EDGE);
        const int n = i < 2 * FM_EDGE ? i - FM_EDGE : e.nsamples - FM_EDGE + (i - 2 * FM_EDGE);
        int w = 0;
        if (n >= 0 && n < e.nsamples) {
            w = e.raw[(long long)s * e.stride_pairs + n];
        } else if (n < 0 && n >= -26) {
            w = e.hist[(long long)s * 32 + 26 + n].x;
            if (e.dc) {
                const int si = (int)(short)((w & 0xffff) - e.ic);
                const int sq = (int)(short)((w >> 16) - e.qc);
                w = (si & 0xffff) | (sq << 16);
            }
        }
        e.edges[(long long)s * (4 * FM_EDGE) + i] = w;
        return;
    }
    // ---- k_hist_in's part (int16 input only on this path)
    const int u = t - nedge;
    const int s = u >> 5, i = u & 31;
    if (s >= hi.nstreams || i >= 26) return;
    const long long n = hi.nsamples - 26 + i;
    int2 v;
    if (n < 0) {
        v = hi.hist_old[(long long)s * 32 + (26 + n)];
    } else {
        const int w = hi.raw[(long long)s * hi.stride_pairs + n];
        const int si = java_short_add((int)(short)(w & 0xffff), hi.ic);
        const int sq = java_short_add(w >> 16, hi.qc);
        v = make_int2((si & 0xffff) | (sq << 16), 0);
    }
    hi.hist_new[(long long)s * 32 + i] = v;
}

// SMALL: the instantiation for SHORT calls (at most FM_THREADS outputs: the receive() form) -- the matched half as one
// output per thread; a kernel of its own so that its loop does not sit in the batch kernel's register allocation (as a
// run-time branch it cost the batch kernel its fourth wave per SIMD: 123 -> 131 VGPRs, 16.8 -> 20.1 ms at 8192 streams)
//
// PH >= 0: the form for the 8-PHASE TUNER (12 kHz / 96 kHz: an exact 8-cycle over table entries of which five are 1.0, -1.0 or
// 0.0; bpsk_tuner.h).  Window sample m of a tile whose sample 0 is at phase p has the factors of phase p + m, and the front
// loop is unrolled over m, so with p known at compile time the class of every factor is a constant:
//   +-1.0 : no tuner product (d * +-1.0 is +-d), and EVERY tap of that sample and rail is one fma with +-tap.  d is a float and
//           has at most 24 significant bits, a tap is k 2^-15 with |k| < 2^14 (ds_taps_are_short below): d * tap is exact in
//           double, so fma(d, +-tap, acc) rounds once what acc + RN(RN(d * +-1.0) * tap) rounds once -- the same double.
//   0.0   : nothing at all for that rail of that sample.  The int16 sample is finite, so its product is +-0 and so is every tap
//           product; an accumulator starts at +0.0 and never becomes -0 (a rounded sum is -0 only when both terms are), so
//           adding +-0 leaves it as it is.  (The float kernel, whose input may be NaN or Inf, has no such form.)
//   other : as in the generic form.
// Tiles are 65 FM_NB D samples apart, which is 4 mod 8: one launch sees the phases p and p + 4, whose classes differ (sin is 0.0
// at phase 0 and 1.2e-16 at phase 4).  The instantiation PH = p mod 4 holds both bodies and a tile branches to its own.  The
// launcher takes this form only where the host has found exactly these classes in the schedule's table, by bit pattern
// (Schedule::trot); every other call takes PH = -1: the class tests below fold away and leave the generic arithmetic,
// operation for operation.
constexpr bool ds_taps_are_short()
{
    for (int n = 0; n < 14; n++) {
        const float k = kDsHalf[n] * 32768.0f;
        if (k != (float)(int)k || k >= 16384.0f || k <= -16384.0f) return false;
    }
    return true;
}
static_assert(ds_taps_are_short(), "dsFilter: every tap times 2^15 is an integer of magnitude below 2^14 (k_fm's +-1.0 fmas are exact)");

template <int D, int R, bool MIX, bool DC, bool FAST, bool SMALL = false, int PH = -1>
#ifndef JSDR_FM_MINWAVES
#define JSDR_FM_MINWAVES 2
#endif
__global__ __launch_bounds__(FM_THREADS, JSDR_FM_MINWAVES) void k_fm(FmArgs a)
{
    constexpr int RD = D * R, NS = RD - D + 27, NSQ = (NS + 3) / 4;
    constexpr int JOBS = (FM_NT + R - 1) / R, ROUNDS = (JOBS + FM_THREADS - 1) / FM_THREADS;
    static_assert(PH < 0 || (MIX && !FAST && PH < 4 && (D * R) % 8 == 0 && (65 * FM_NB * D) % 8 == 4),
                  "k_fm<PH>: the lane span is whole periods and a tile is half a period past the one before");
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *X = reinterpret_cast<double2 *>(smem);                    // [FM_NT]: X[t] = sample G - 64 + t
    double *sc = reinterpret_cast<double *>(smem + FM_NT * sizeof(double2));  // [512]
    for (int i = threadIdx.x; i < 512; i += FM_THREADS) sc[i] = a.sincos[i];
#ifdef JSDR_X_CLK
    unsigned long long clk_acc_[6] = {0, 0, 0, 0, 0, 0}, clk_last_ = 0;
#endif
#ifdef JSDR_X_WGCLK
    const unsigned long long wgclk0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long wgclk_n = 0;
#endif
    const long long nwork = (long long)a.ntiles * a.nstreams;
    // The TICKET form (a.tickets: the launch is held to a CU share, jsdr_bpsk_set_cu_share -- persistent workgroups beside another
    // kernel's): a statically shared launch lasts as long as its slowest workgroup, and here a workgroup's pace depends on whom it
    // shares its CU with and on when it was placed, so the tiles are handed out as the workgroups get through them.  Work item
    // blockIdx.x first, then gridDim.x + ticket: one atomicAdd of thread 0 on the launch's counter (zeroed on the stream in front of
    // the launch), taken behind the front half and handed round through LDS at the tile's last barrier -- a whole matched half after
    // the request, so nobody waits for its round trip.  (Taken at the top of the tile its answer is one register more where the
    // kernel has most alive, in the front half: 113-115 VGPRs against 111-113.)  Measured at the headline step, beside k_fft and
    // k_tail8 (profiles/r09_ticket_handout.md): the workgroups of a launch used to end between 24.1 and 27.6 ms, and end within 25 us
    // of each other at 27.0 ms; the step went from 33.26-33.34 to 32.98-33.03 ms on one part and from 36.2-36.4 to 34.0-34.1 on a
    // slower one.  (k_fft keeps its fixed stride: its ticket form -- alone or together with this one -- made the step slower.)
    const bool tickets = a.tickets != nullptr;
    int *tkL = reinterpret_cast<int *>(sc + 512);  // [1]
#pragma unroll 1
    for (long long work = blockIdx.x; work < nwork; work = tickets ? (long long)gridDim.x + (unsigned)__builtin_amdgcn_readfirstlane(tkL[0]) : work + gridDim.x) {
    const int s = (int)(work / a.ntiles);
    const long long G = a.tile0 + (long long)(65 * FM_NB) * (work % a.ntiles);
    const int jrel0 = (int)(G - 64 - a.g_first);  // call-relative output index of X[0] (negative in the first tile)
#ifdef JSDR_X_FM_SMALLSET  // timing probe (round 5): every stream reads one of 16 streams' samples -- 64 MB, served by the memory-side cache
    const int *raw = a.raw + (long long)(s & 15) * a.stride_pairs;
#else
    const int *raw = a.raw + (long long)s * a.stride_pairs;
#endif
    const int *edges = a.edges + (long long)s * (4 * FM_EDGE);
    const double2 *dmh_old = a.dmh_old + (long long)s * 64;
    const int Lm1 = a.nsamples - 1, nds = a.nds, P = a.tper;
    // :469 HOWARD_FUDGE_FACTOR = 0.9 * 32768, times the 2^-15 that takes out the conversion's scale (fm_convert_2p15: di, dq
    // and with them the tuner products and the 27-tap sums are 2^15 times the reference's, exactly; the product with
    // HOWARD * 2^-15 -- an exact constant -- is then the reference's double)
    const double HOWARD = 0.9 * 32768.0 * (double)I16_2P15_UNSCALE;
    // tile-uniform base into the unwrapped tuner table: window sample m of ANY job of this tile uses entry e0 + m
    // (the lane span RD is a multiple of the period)
    int e0 = 0;
    if constexpr (MIX) {
        const long long v = (long long)a.first_out + (long long)D * jrel0;
        e0 = (int)(((v % P) + P) % P);
    }
    // constant address space: the table is read-only for the launch, and only loads the compiler may assume invariant
    // become scalar loads (a plain global pointer in a kernel that also stores gives 57 vector loads per job)
    typedef const __attribute__((address_space(4))) double *const_tab_t;
    const_tab_t tb = (const_tab_t)(a.tcs + e0);  // tb[2m] = cos, tb[2m+1] = sin
    float amx = 0.0f;  // FAST: largest |sample| this lane converts
    __syncthreads();  // sin/cos table
#ifdef JSDR_X_CLK
    clk_last_ = __builtin_amdgcn_s_memtime();
#endif
    // ================================================================================ front half
    // (a generic lambda: the round loop's text once, instantiated for the phases of this kernel; PHC < 0: the generic arithmetic)
    auto front = [&](auto phc) __attribute__((always_inline)) {
    constexpr int PHC = decltype(phc)::value;
#ifdef JSDR_X_NOFRONT
    if (a.nds < 0)
#endif
#pragma unroll 1
    for (int round = 0; round < ROUNDS; round++) {
        const int job = threadIdx.x + FM_THREADS * round;
        const int t0 = R * job;
        if (t0 >= FM_NT) break;
        const int j0 = jrel0 + t0;                   // first output of the job, call relative
        const int n0 = a.first_out + D * j0 - 26;    // its window's first sample
        // `none`: no output of the job is filtered here (the halo before output 0, slots past the call's last output).
        // Every other job takes the same arithmetic in the same pass.  A window that reaches back into the previous
        // call's 26 samples, or past the last sample, is read from the stream's EDGE IMAGE instead of the input -- 256
        // samples around sample 0 (history, then input) and 256 around the last one (zero beyond), laid out by
        // k_fm_edges before this kernel -- with the same fifteen loads; outputs that are not this call's (a job that
        // straddles output 0 or the last output) are replaced at the store.  (These jobs used to run a
        // one-output-at-a-time loop of dependent loads after the others had finished: one of them held its workgroup
        // for longer than a whole regular tile takes.  The tile's last job, which owns fewer than R image slots when R
        // does not divide FM_NT, drops the surplus at the store -- on the old edge path it cost every tile ~7 us.)
        const bool none = j0 + R <= 0 || j0 >= nds || nds <= 0;
        const bool regular = j0 >= 0 && j0 + R <= nds;
        if (!none) {
            int4 W[NSQ];
            const int *wp = raw + n0;
            if (n0 < 0) wp = edges + (n0 + FM_EDGE);
            else if (n0 + 4 * NSQ - 1 > Lm1) wp = edges + 2 * FM_EDGE + (n0 - (a.nsamples - FM_EDGE));
            // the VCO table indices of the job's outputs come in WITH the window: left where they are used, after the
            // last quad, the load was issued there and waited for on the spot -- a full memory latency at the end of
            // every round (nothing may cross the quads' scheduling barriers, so the source order decides)
            unsigned kv4[(R + 3) / 4];  // R byte indices, four to a register
#pragma unroll
            for (int k = 0; k < (R + 3) / 4; k++) kv4[k] = 0;
            if (regular) {
#pragma unroll
                for (int r = 0; r < R; r++) kv4[r / 4] |= (unsigned)a.kvco[j0 + r] << (8 * (r % 4));
            } else {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int j = j0 + r;
                    kv4[r / 4] |= (unsigned)a.kvco[j < 0 ? 0 : (j >= nds ? nds - 1 : j)] << (8 * (r % 4));
                }
            }
#pragma unroll
            for (int q = NSQ - 1; q >= 0; q--) W[q] = *reinterpret_cast<const int4 *>(wp + 4 * q);
#ifndef JSDR_FM_NOPIN
            __builtin_amdgcn_sched_barrier(0);
#endif
            double ai[R], aq[R];
            double vc[R], vs[R];  // the outputs' VCO (cos, sin): LDS reads issued under the last quad's arithmetic
#pragma unroll
            for (int r = 0; r < R; r++) {
                ai[r] = 0.0;
                aq[r] = 0.0;
            }
#pragma unroll
            for (int q = NSQ - 1; q >= 0; q--) {
                const int4 w4 = W[q];
                if (q == 0) {
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const int kv = (kv4[r / 4] >> (8 * (r % 4))) & 0xff;
                        vc[r] = sc[kv];
                        vs[r] = sc[256 + kv];
                    }
                }
#pragma unroll
                for (int t = 3; t >= 0; t--) {
                    const int m = 4 * q + t;
                    if (m < NS) {
                        const int w = (t == 0) ? w4.x : (t == 1) ? w4.y : (t == 2) ? w4.z : w4.w;
                        double di, dq;
                        fm_convert_2p15(w, a.ic, a.qc, DC, di, dq, FAST ? &amx : nullptr);  // 2^15 x the reference's (HOWARD)
                        // the factors' classes: constants once the loops are unrolled
                        const int ci = PHC >= 0 ? tuner8_class(PHC + m, 0) : TC_GEN, cq = PHC >= 0 ? tuner8_class(PHC + m, 1) : TC_GEN;
                        if constexpr (MIX) {  // :388-390 component-wise, not a complex multiply
                            if (ci == TC_GEN) di = di * tb[2 * m];
                            if (cq == TC_GEN) dq = dq * tb[2 * m + 1];
                        }
#pragma unroll
                        for (int r = 0; r < R; r++) {
                            if (m >= D * r && m <= D * r + 26) {  // age D*r+26-m in the window of output r
                                const int age = D * r + 26 - m;
                                const double tp = ds_tap(age);
                                // exact order, and still one instruction where the fma IS the separately rounded pair:
                                // the output's first tap (the sum is +0.0: a product of either sign of zero gives +0
                                // both ways) and a tap that is a power of two (the product is exact)
                                const bool same = age == 0 || ((kDsPow2Mask >> age) & 1);
                                // ... and every tap of a sample whose tuner factor is +-1.0 (the sign goes to the tap); none
                                // where it is 0.0
                                if (FAST || same || ci != TC_GEN) {
                                    if (ci != TC_ZERO) ai[r] = __builtin_fma(di, ci == TC_MONE ? -tp : tp, ai[r]);
                                } else {
                                    ai[r] += di * tp;
                                }
                                if (FAST || same || cq != TC_GEN) {
                                    if (cq != TC_ZERO) aq[r] = __builtin_fma(dq, cq == TC_MONE ? -tp : tp, aq[r]);
                                } else {
                                    aq[r] += dq * tp;
                                }
                            }
                        }
                    }
                }
#ifndef JSDR_FM_NOPIN
#pragma unroll
                for (int r = 0; r < R; r++) asm volatile("" : "+v"(ai[r]), "+v"(aq[r])::"memory");  // sums are due here
                if constexpr (FAST) asm volatile("" : "+v"(amx));  // (or the maxima sink to the end of the round with all 114 floats alive)
                __builtin_amdgcn_sched_barrier(0);
#endif
            }
            if (regular) {
#pragma unroll
                for (int r = 0; r < R; r++) {  // x HOWARD_FUDGE_FACTOR (:486), VCO mix (:515-516)
                    const double oi = ai[r] * HOWARD, oq = aq[r] * HOWARD;
                    if (FM_NT % R == 0 || t0 + r < FM_NT) X[t0 + r] = make_double2(oi * vc[r], oq * vs[r]);
                }
            } else {  // a job that straddles output 0 or the call's last output: one or two per stream and call
                double oi[R], oq[R];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    oi[r] = ai[r] * HOWARD * vc[r];
                    oq[r] = aq[r] * HOWARD * vs[r];
                }
#pragma unroll 1
                for (int r = 0; r < R; r++) {
                    const int t = t0 + r, j = j0 + r;
                    double2 val = make_double2(0.0, 0.0);
                    if (j >= 0 && j < nds) {
                        // (run-time r: a select chain, not an indexed register file)
                        val.x = r == 0 ? oi[0] : r == 1 ? oi[1] : r == 2 ? oi[2] : r == 3 ? oi[3] : oi[R - 1];
                        val.y = r == 0 ? oq[0] : r == 1 ? oq[1] : r == 2 ? oq[2] : r == 3 ? oq[3] : oq[R - 1];
                    } else if (j >= -64 && j < 0) {
                        val = dmh_old[64 + j];
                    }
                    if (t < FM_NT) X[t] = val;
                }
            }
        } else {
#pragma unroll 1
            for (int r = 0; r < R; r++) {
                const int t = t0 + r, j = j0 + r;
                const double2 val = (j >= -64 && j < 0) ? dmh_old[64 + j] : make_double2(0.0, 0.0);
                if (t < FM_NT) X[t] = val;
            }
        }
    }
    };
    if constexpr (PH < 0) {
        front(std::integral_constant<int, -1>{});
    } else {  // tile-uniform: the phase of the tile's window sample 0 is PH or PH + 4
        if (((e0 + a.trot) & 7) == PH) front(std::integral_constant<int, PH>{});
        else front(std::integral_constant<int, PH + 4>{});
    }
    if constexpr (FAST) {  // non-negative floats order like their bit patterns
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) amx = fmaxf(amx, __shfl_xor(amx, off, 64));
        if ((threadIdx.x & 63) == 0 && amx > 0.0f) atomicMax(a.amax + s, __float_as_int(amx));
    }
    FM_CLK(1);  // front half
    __syncthreads();
    FM_CLK(3);  // barrier after the front half
    unsigned tk = 0;
    if (tickets && threadIdx.x == 0) tk = atomicAdd(a.tickets, 1u);
    // ---- the call's last 64 VCO-mixed samples are the next call's halo; every sample is owned by one tile
    if (jrel0 + FM_NT > nds - 64) {  // uniform
        double2 *dmh_new = a.dmh_new + (long long)s * 64;
        for (int t = 64 + threadIdx.x; t < FM_NT; t += FM_THREADS) {
            const int j = jrel0 + t;
            if (j >= nds - 64 && j < nds && j >= 0) dmh_new[j - (nds - 64)] = X[t];
        }
        if (work % a.ntiles == 0 && nds < 64 && (int)threadIdx.x < 64 - nds) dmh_new[threadIdx.x] = dmh_old[threadIdx.x + nds];
    }
    // ================================================================================ matched filter
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int blk = lane < FM_NB ? lane : FM_NB - 1;  // lanes 62, 63 shadow block 61 and store nothing
    const double2 *xl = X + 64 + 65 * blk;            // &X[s0]
    const int rel0 = jrel0 + 64 + 65 * blk;           // call-relative index of s0
    double2 *y = a.y + (long long)s * a.y_stride;
    if constexpr (SMALL) {
        // A SHORT call (the receive() form: 205 outputs of a 2048-sample frame): one output per thread, the reference's
        // ring-slot order (:519-523) as a per-thread loop over the image -- (s0, s0-1, .., g-64) then (g, .., s0+1) with
        // s0 = g - u the sample in ring slot 0 -- instead of the lane-per-block mapping, whose eight waves each walk all
        // 65 taps for 62 blocks of which a short call fills four (19 us of a 70 us receive).  Same operands, same order:
        // the same doubles (this is tail_exact_sample's second half).
        const int rel = (int)threadIdx.x, t = rel - jrel0;
        if (rel < nds && t >= 64 && t < FM_NT) {
            const long long g = a.g_first + rel;
            const int u = (int)(((g - 64) % 65 + 65) % 65);
            const double2 *xg = X + t;  // &X[g]
            const double *f = c_bpsk.dm_taps;
            double yi = 0.0, yq = 0.0;
            for (int i = 0; i <= 64 - u; i++) {  // s0, s0-1, .., g-64: ages u .. 64
                const double2 x = xg[-(u + i)];
                const double tp = f[u + i];
                if constexpr (FAST) {
                    yi = __builtin_fma(x.x, tp, yi);
                    yq = __builtin_fma(x.y, tp, yq);
                } else {
                    yi += x.x * tp;
                    yq += x.y * tp;
                }
            }
            for (int m = 0; m < u; m++) {        // g, g-1, .., s0+1: ages 0 .. u-1
                const double2 x = xg[-m];
                const double tp = f[m];
                if constexpr (FAST) {
                    yi = __builtin_fma(x.x, tp, yi);
                    yq = __builtin_fma(x.y, tp, yq);
                } else {
                    yi += x.x * tp;
                    yq += x.y * tp;
                }
            }
            y[rel] = make_double2(yi, yq);
        }
    } else {
#ifdef JSDR_X_NOMATCHED
    if (a.nds < 0)
#endif
#ifndef JSDR_FM_DIRECT_STORE  // (the old lane-strided stores: 17.08 vs 16.86 ms at 8192 streams, one session)
    // The tile's 65 * FM_NB outputs leave through the image, which is dead once every wave has walked its blocks: a lane's
    // outputs go to LDS at its block's stride (65 slots: conflict-free), and the workgroup then stores the tile's outputs
    // -- contiguous in y -- as fully coalesced 16-byte accesses, instead of one 16-byte store per lane at a 1040-byte stride
    {
        double ai[9], aq[9];
        int u0 = 0, nout = 9;
        if (wave == 0) {
            matched_block<9, FAST>(xl, 0, ai, aq);
        } else {
            u0 = 9 + 8 * (wave - 1);
            nout = 8;
            double bi[8], bq[8];
            matched_block<8, FAST>(xl, u0, bi, bq);
#pragma unroll
            for (int r = 0; r < 8; r++) {
                ai[r] = bi[r];
                aq[r] = bq[r];
            }
        }
        __syncthreads();  // every wave has finished reading the image
        if (lane < FM_NB) {
#pragma unroll
            for (int r = 0; r < 9; r++)
                if (r < nout) X[65 * blk + u0 + r] = make_double2(ai[r], aq[r]);
        }
        __syncthreads();
        const int relb = jrel0 + 64;  // call-relative index of the tile's first output
        for (int o = (int)threadIdx.x; o < 65 * FM_NB; o += FM_THREADS) {
            const int rel = relb + o;
            if (rel >= 0 && rel < nds) y[rel] = X[o];
        }
    }
#else
    if (wave == 0) {
        double ai[9], aq[9];
        matched_block<9, FAST>(xl, 0, ai, aq);
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int rel = rel0 + r;
            if (lane < FM_NB && rel >= 0 && rel < nds) y[rel] = make_double2(ai[r], aq[r]);
        }
    } else {
        const int u0 = 9 + 8 * (wave - 1);
        double ai[8], aq[8];
        matched_block<8, FAST>(xl, u0, ai, aq);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int rel = rel0 + u0 + r;
            if (lane < FM_NB && rel >= 0 && rel < nds) y[rel] = make_double2(ai[r], aq[r]);
        }
    }
#endif
    }
    FM_CLK(4);  // matched half
    {
        // (pinned here by an opaque zero: left alone the compiler moves this store up beside the atomic -- same condition -- and
        //  waits for the ticket's round trip on the spot, as in bpsk_acq.hip)
        int zlate = 0;
        asm volatile("" : "+v"(zlate));
        if (tickets && threadIdx.x == 0) tkL[0] = (int)tk + zlate;
    }
    __syncthreads();  // the next work item reuses the image, and takes its number from tkL (written next behind the next matched half)
    FM_CLK(5);  // barrier after the matched half
#ifdef JSDR_X_WGCLK
    wgclk_n++;
#endif
    }
#ifdef JSDR_X_WGCLK
    if (threadIdx.x == 0 && blockIdx.x < WGCLK_WGS) {
        unsigned long long *c = g_fm_wgclk[a.wgclk_slot][blockIdx.x];
        c[0] = wgclk0;
        c[1] = __builtin_amdgcn_s_memrealtime();
        c[2] = wgclk_n;
    }
#endif
#ifdef JSDR_X_CLK
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < 6; i++) atomicAdd(&g_fm_clk[blockIdx.x & 255][(threadIdx.x >> 6) * 8 + i], clk_acc_[i]);
#endif
}

// =============================================================================================== launchers
// What the handle's call (bpsk_call.hip) starts (bpsk_kernels.h): the grid, the LDS and the template choice of each kernel.

int bpsk_fm_upload_constants(const BpskConst &bc)
{
    JSDR_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_bpsk), &bc, sizeof(bc)));
    return JSDR_OK;
}

int launch_matched(const MatchedArgs &ma, int nstreams, hipStream_t st)
{
    const long long ntiles = (ma.g_first + ma.nds - ma.tile0 + 4159) / 4160;
    const size_t lds = (64 + 4160) * sizeof(double2);
    JSDR_LDS_ATTR(k_matched<false>, lds);
    JSDR_LDS_ATTR(k_matched<true>, lds);
    hipLaunchKernelGGL(k_matched<false>, dim3((unsigned)ntiles, (unsigned)nstreams), dim3(512), lds, st, ma);
    return launched();
}

int launch_dm_history(double2 *dm, long long dm_stride, long long nds, int nstreams, hipStream_t st)
{
    hipLaunchKernelGGL(k_dm_history, dim3((unsigned)nstreams), dim3(64), 0, st, dm, dm_stride, nds, nstreams);
    return launched();
}

int launch_fm_prep(const EdgeArgs &ea, const HistArgs &ha, const ScatterArgs &sc, hipStream_t st)
{
    hipLaunchKernelGGL(k_fm_prep, dim3((unsigned)(((long long)ea.nstreams * (4 * FM_EDGE + 32) + sc.bytes[0] + sc.bytes[1] + 255) / 256)),
                       dim3(256), 0, st, ea, ha, sc);
    return launched();
}

template <int D, int R>
static int launch_fm_t(const FmArgs &a_in, bool mix, bool dc, bool fast, int nstreams, hipStream_t st, long long *items, long long *grid_out,
                       int *phase)
{
    *phase = -1;
    const size_t lds = (size_t)FM_NT * sizeof(double2) + 512 * sizeof(double) + sizeof(double);  // image, sin / cos table, ticket
    const long long span = 65LL * FM_NB;
    const long long ntiles = (a_in.g_first + a_in.nds - a_in.tile0 + span - 1) / span;
    FmArgs a = a_in;
    a.ntiles = (int)ntiles;
    a.nstreams = nstreams;
    static const long long grid_cap = [] {
        const char *e = knob("JSDR_FM_GRID");  // tuning knob: total workgroups (default: one per tile)
        return e ? atoll(e) : 0LL;
    }();
    long long gx = ntiles * nstreams;
    if (grid_cap > 0 && gx > grid_cap) gx = grid_cap;
    if (a.grid_limit > 0 && gx > a.grid_limit) gx = a.grid_limit;
    *items = ntiles * nstreams;
    *grid_out = gx;
    // held to a share, the workgroups take their tiles by ticket (k_fm); a launch with a workgroup per tile has nothing to hand out
    if (!(a.grid_limit > 0 && gx < ntiles * nstreams && ntiles * nstreams + gx < 0x7fffffffLL)) a.tickets = nullptr;
#ifdef JSDR_X_WGCLK
    {
        static int wgclk_seq = 0;
        static const bool wgclk_static = getenv("JSDR_X_WGCLK_STATIC") != nullptr;  // the probe's "before": the share without tickets
        if (wgclk_static) a.tickets = nullptr;
        a.wgclk_slot = wgclk_seq % WGCLK_SLOTS;
        g_wgclk_log[a.wgclk_slot][0] = ntiles * nstreams;
        g_wgclk_log[a.wgclk_slot][1] = gx;
        g_wgclk_log[a.wgclk_slot][2] = a.tickets != nullptr;
        g_wgclk_log[a.wgclk_slot][3] = wgclk_seq++;
    }
#endif
    if (a.tickets) JSDR_HIP_TRY(hipMemsetAsync(a.tickets, 0, sizeof(unsigned), st));
    const dim3 grid((unsigned)gx), block(FM_THREADS);
#define JSDR_FM_LAUNCH_PH(MIX, DC, FAST, SMALL, PH)                                                             \
    do {                                                                                                        \
        JSDR_LDS_ATTR((k_fm<D, R, MIX, DC, FAST, SMALL, PH>), lds);                                             \
        hipLaunchKernelGGL((k_fm<D, R, MIX, DC, FAST, SMALL, PH>), grid, block, lds, st, a);                    \
    } while (0)
#define JSDR_FM_LAUNCH(MIX, DC, FAST, SMALL) JSDR_FM_LAUNCH_PH(MIX, DC, FAST, SMALL, -1)
    const bool small = !fast && a.nds <= FM_THREADS && ntiles == 1;
    if constexpr (D == 10) {
        // the 8-phase tuner's form (k_fm<PH>): exact variant, the batch kernel, a table whose factors the host has classified
        if (mix && !fast && !small && a.trot >= 0 && a.tper == 8) {
            const long long v = (long long)a.first_out + (long long)D * (a.tile0 - 64 - a.g_first);  // k_fm's e0 of tile 0
            const int p0 = (int)((((v % 8) + 8) % 8 + a.trot) & 7);
            *phase = p0;
            switch (p0 & 3) {
                case 0: if (dc) JSDR_FM_LAUNCH_PH(true, true, false, false, 0); else JSDR_FM_LAUNCH_PH(true, false, false, false, 0); break;
                case 1: if (dc) JSDR_FM_LAUNCH_PH(true, true, false, false, 1); else JSDR_FM_LAUNCH_PH(true, false, false, false, 1); break;
                case 2: if (dc) JSDR_FM_LAUNCH_PH(true, true, false, false, 2); else JSDR_FM_LAUNCH_PH(true, false, false, false, 2); break;
                default: if (dc) JSDR_FM_LAUNCH_PH(true, true, false, false, 3); else JSDR_FM_LAUNCH_PH(true, false, false, false, 3); break;
            }
            return launched();
        }
    }
    if (small && a.nds <= FM_THREADS && ntiles == 1) {  // a short call (receive()): the one-output-per-thread matched half
        if (mix) { if (dc) JSDR_FM_LAUNCH(true, true, false, true); else JSDR_FM_LAUNCH(true, false, false, true); }
        else { if (dc) JSDR_FM_LAUNCH(false, true, false, true); else JSDR_FM_LAUNCH(false, false, false, true); }
    } else if (fast) {
        if (mix) { if (dc) JSDR_FM_LAUNCH(true, true, true, false); else JSDR_FM_LAUNCH(true, false, true, false); }
        else { if (dc) JSDR_FM_LAUNCH(false, true, true, false); else JSDR_FM_LAUNCH(false, false, true, false); }
    } else {
        if (mix) { if (dc) JSDR_FM_LAUNCH(true, true, false, false); else JSDR_FM_LAUNCH(true, false, false, false); }
        else { if (dc) JSDR_FM_LAUNCH(false, true, false, false); else JSDR_FM_LAUNCH(false, false, false, false); }
    }
#undef JSDR_FM_LAUNCH
#undef JSDR_FM_LAUNCH_PH
    return launched();
}

int launch_fm(const FmArgs &a, int decim, bool mix, bool dc, bool fast, int nstreams, hipStream_t st, long long *items, long long *grid,
              int *phase)
{
    switch (decim) {
        case 4: return launch_fm_t<4, 5>(a, mix, dc, fast, nstreams, st, items, grid, phase);
        case 5: return launch_fm_t<5, 4>(a, mix, dc, fast, nstreams, st, items, grid, phase);
        case 10: return launch_fm_t<10, 4>(a, mix, dc, fast, nstreams, st, items, grid, phase);
        case 20: return launch_fm_t<20, 4>(a, mix, dc, fast, nstreams, st, items, grid, phase);
    }
    set_error("bpsk: unsupported decimation %d", decim);
    return JSDR_ERR;
}

void bpsk_fm_clocks_report()
{
#ifdef JSDR_X_WGCLK
    {
        const char *path = getenv("JSDR_X_WGCLK_OUT_FM");
        FILE *f = fopen(path ? path : "wgclk_fm.csv", "w");
        static unsigned long long cc[WGCLK_SLOTS][WGCLK_WGS][3];
        if (f && hipMemcpyFromSymbol(cc, HIP_SYMBOL(g_fm_wgclk), sizeof(cc)) == hipSuccess) {
            fprintf(f, "launch,items,grid,ticket,wg,t0,t1,n\n");
            for (int sl = 0; sl < WGCLK_SLOTS; sl++)
                for (int w = 0; w < WGCLK_WGS && w < g_wgclk_log[sl][1]; w++)
                    fprintf(f, "%lld,%lld,%lld,%lld,%d,%llu,%llu,%llu\n", g_wgclk_log[sl][3], g_wgclk_log[sl][0], g_wgclk_log[sl][1],
                            g_wgclk_log[sl][2], w, cc[sl][w][0], cc[sl][w][1], cc[sl][w][2]);
        }
        if (f) fclose(f);
    }
#endif
#ifdef JSDR_X_CLK
    {
        static unsigned long long cc[256][64];
        if (hipMemcpyFromSymbol(cc, HIP_SYMBOL(g_fm_clk), sizeof(cc)) == hipSuccess) {
            static const char *nm[6] = {"-", "front half", "-", "barrier front", "matched", "barrier matched"};
            for (int i = 0; i < 6; i++) {
                if (i == 0 || i == 2) continue;
                fprintf(stderr, "k_fm clk %-16s", nm[i]);
                for (int w = 0; w < 8; w++) {
                    unsigned long long c = 0, tot = 0;
                    for (int b = 0; b < 256; b++) {
                        c += cc[b][w * 8 + i];
                        for (int k = 0; k < 6; k++) tot += cc[b][w * 8 + k];
                    }
                    fprintf(stderr, " w%d %5.1f%%", w, 100.0 * c / (tot ? tot : 1));
                }
                fprintf(stderr, "\n");
            }
            memset(cc, 0, sizeof(cc));
            hipMemcpyToSymbol(HIP_SYMBOL(g_fm_clk), cc, sizeof(cc));
        }
    }
#endif
}

}  // namespace jsdr
