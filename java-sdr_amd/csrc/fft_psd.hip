// fft_psd.hip -- batched complex forward FFT + PSD + argmax: the fft.java waterfall path.
//
// Replaces fft.receive (fft.java:190-228) and the JTransforms FloatFFT_1D.complexForward call inside
// it (fft.java:194-195), with the int16 -> float rule of JavaAudio.java:276-293 fused into the load.
//
// MI355X mapping (DESIGN.md "fft kernel"): one frame = T threads of a 256/512-thread workgroup; the
// frame is transformed by a 2..4 pass Stockham autosort FFT with radix-16/8/4 butterflies held in
// registers; passes exchange through one padded LDS image per frame (pad 1 float2 per 16 so that the
// stride-16 stores of pass 1 and the stride-N/R loads of the next pass are bank-conflict free).
// Global loads are one dword (I,Q int16 pair) per lane, 256 contiguous bytes per wave instruction;
// PSD stores likewise.  HBM traffic = 4 B in + 4 B out per sample: the kernel is HBM bound.
// Float arithmetic may contract to FMA here: parity for this path is the 1e-5 (peak-normalised)
// tolerance of BASELINE.json, JTransforms' own rounding being unknowable (source absent).
//
// k_fft_pix (jsdr_fft_waterfall_*) is the same frame loop with waterfall.paintLine (waterfall.java:87-109) fused behind it: the
// last pass leaves the frame's dB row in its LDS image, the frame's threads pool it into pixels, and no PSD row is stored.
#include "fft_common.h"
#include "waterfall_dev.h"
#include <math.h>
#include <stdlib.h>
#include <vector>

namespace jsdr {

// ------------------------------------------------------------------ kernel
// Twiddle tables of pass with radix R and P = product of earlier radices (P > 1):
//   P*R <= 512 : "direct"  D[(r-1)*P + k] = (w, w') with w = exp(-2 pi i k r/(P R)), w' = (-w.y, w.x), 1 <= r < R, k < P
//                          (k fastest: conflict-free 16-byte reads; a*w = a.x*w + a.y*w' is two packed instructions)
//   else       : "base"    B[k]       = exp(-2 pi i k  /(P R)), k < P; powers r=2.. by repeated products
constexpr bool tw_direct(int P, int R) { return P * R <= 512; }
constexpr int tw_size(int P, int R) { return P <= 1 ? 0 : (tw_direct(P, R) ? 2 * P * (R - 1) : P); }  // in float2 units
constexpr int tw_total(int R0, int R1, int R2, int R3)
{
    return tw_size(R0, R1) + (R2 > 1 ? tw_size(R0 * R1, R2) : 0) + (R3 > 1 ? tw_size(R0 * R1 * R2, R3) : 0);
}

constexpr int ilog2_c(int n) { return n <= 1 ? 0 : 1 + ilog2_c(n / 2); }

template <int R, int P>
__device__ __forceinline__ void apply_twiddles(float2 *v, int k, const float2 *tab)
{
    if constexpr (P > 1) {
        if constexpr (tw_direct(P, R)) {
#pragma unroll
            for (int r = 1; r < R; r++) {
                const float4 t = reinterpret_cast<const float4 *>(tab)[(r - 1) * P + k];
                v[r] = cmul2(v[r], make_float2(t.x, t.y), make_float2(t.z, t.w));
            }
        } else {
            float2 w1 = tab[k];
            float2 w[R], wq[R];  // wq = (-w.y, w.x): a*w = a.x*w + a.y*wq, two packed instructions
            w[1] = w1;
            wq[1] = cquad(w1);
#pragma unroll
            for (int r = 2; r < R; r++) {
                w[r] = (r & 1) ? cmul2(w[r - 1], w1, wq[1]) : cmul2(w[r / 2], w[r / 2], wq[r / 2]);
                wq[r] = cquad(w[r]);
            }
#pragma unroll
            for (int r = 1; r < R; r++) v[r] = cmul2(v[r], w[r], wq[r]);
        }
    }
}

template <int R, int... Rs>
__device__ __forceinline__ void store_lds(float2 *dst, const float2 *v, int j0, int p, std::integer_sequence<int, Rs...>)
{
    ((dst[lds_pad(j0 + Rs * p)] = v[cx_bitrev(Rs, R)]), ...);
}

// A frame's first-pass inputs as they come from memory: one (I,Q) int16 pair or one float pair per point.  They are
// fetched ONE FRAME AHEAD, just before the previous frame's last pass: that pass holds one small butterfly at a time
// (registers to spare), and a load issued before the PSD stores does not queue behind them -- loads and stores share
// the in-order vmcnt counter, so a frame's loads issued after the previous frame's stores waited for those stores'
// acknowledgements first (measured on 2048 streams: 4.02 ms, without the loads 3.41, without the stores 3.36, without
// both 2.76: memory time simply added to the arithmetic).
template <int IN>
struct RawPoint {
    using type = int;
};
template <>
struct RawPoint<IN_F32> {
    using type = float2;
};
template <int N, int T, int IN, int R, class FR>
__device__ __forceinline__ void fft_fetch(const FftArgs &a, FR frame, int tid, typename RawPoint<IN>::type (&w)[R])
{
    constexpr int NB = N / R;
    static_assert(NB == T, "one first-pass butterfly per thread");
    const typename RawPoint<IN>::type *src = reinterpret_cast<const typename RawPoint<IN>::type *>(a.in) +
#ifdef JSDR_X_FFT_SMALLSET  // timing probe (round 5): every frame reads one of 8192 frames -- 64 MB, served by the memory-side cache
        (frame_row(frame) & 8191) * N;
#else
        frame_in(frame, N);
#endif
    using RAW = typename RawPoint<IN>::type;
    [[maybe_unused]] const WaveRow row = wave_row(src, N * (unsigned)sizeof(RAW));  // (whole waves a frame: `src` is a scalar)
#pragma unroll
    for (int r = 0; r < R; r++) {
#ifdef JSDR_X_FFT_NOLOAD  // timing experiment: no input loads (wrong data)
        if constexpr (IN == IN_I16) w[r] = (tid + r * NB) * 2654435761u + (int)(size_t)src;
        else w[r] = make_float2((float)(tid + r), (float)(size_t)src);
#else
        if constexpr (frame_is_waves(T)) w[r] = wave_row_load<RAW>(row, tid * (unsigned)sizeof(RAW), r * NB * (unsigned)sizeof(RAW));
        else w[r] = src[tid + r * NB];
#endif
    }
}

// One Stockham pass of one frame by T threads.  Each thread owns ITERS = (N/R)/T butterflies, loads
// them all (global for the first pass, LDS otherwise), transforms in registers, and only after a
// barrier (every load of the in-place image has landed) writes its outputs.
//
// The int16 path's scale (SC): its first pass converts with i16_to_float_java_2p15 (common.h) -- one fma per value where
// the reference rule takes a multiply and an fma -- so its butterflies (P = 1: no table; sums and constant products only)
// run on values that are EXACTLY 2^15 times the float path's.  The second pass takes the factor out in the multiply it does
// anyway: the int16 launch's copy of that pass's "direct" table is pre-multiplied by 2^-15 (jsdr_fft::tw_i16; exact, and
// (2^15 a) * (2^-15 w) is the same real product, hence the same float), and element 0 of each butterfly, which has no
// twiddle, gets one packed multiply.  From there on every value is bit for bit the float path's
// (tests/test_gpu_fft_i16_scaled.py).  SC_IN: this (first) pass produces scaled values; SC_OUT: this (second) pass removes
// the scale.  A plan whose second pass is not "direct" keeps the two-instruction conversion.
enum { SC_NONE = 0, SC_IN = 1, SC_OUT = 2 };

// OUT_PIX (k_fft_pix): the frame's dB row never leaves the CU -- the last pass writes it over the frame's LDS image and the
// epilogue of fft_frame pools it into waterfall pixels (waterfall_dev.h)
struct FftPixArgs : FftArgs {
    unsigned *pix;      // [nframes][width]
    float *maxo;        // [nframes][width] pooled maxima, unrotated; may be null
    float *peak;        // [nframes][2] = {Hz, max dB}; may be null
    int width;
    unsigned peak_rgb;
};

// fft.java:205-207: 10*log10((re^2+im^2) * (2/N)^2) = 10*log10(2) * (log2(re^2+im^2) + 2 - 2*log2(N)):
// N is a power of two, so the scale is an exact integer offset of the base-2 logarithm.  Stated once: the PSD form stores
// this value and the pixel form pools it, and the two must round (and contract) alike to the bit.
template <int N>
__device__ __forceinline__ float psd_db(float2 x)
{
    constexpr float L2 = 3.0102999566398120f;
    constexpr float OFF = 3.0102999566398120f * (2.0f - 2.0f * (float)ilog2_c(N));
    return L2 * __log2f(x.x * x.x + x.y * x.y) + OFF;
}

// the dB row of OUT_PIX in the frame's LDS image, as float[N]: one pad float per 32, so that the pooling reads of
// neighbouring pixels -- a power-of-two stride of bins between lanes at the usual widths -- fall on 32 different banks
// (ds_read_b32 is served in two groups of 32 lanes over 32 banks), and the writes, 32 consecutive bins a group, stay so
__device__ __forceinline__ int row_pad(int idx) { return idx + (idx >> 5); }
constexpr bool fft_i16_scaled(int R0, int R1) { return tw_direct(R0, R1); }

template <int N, int T, int IN, int OUT, int R, int P, bool FIRST, bool LAST, class RAW = int, int SC = SC_NONE, class FR>
__device__ __forceinline__ void fft_pass(const FftArgs &a, FR frame, bool active, int tid, float2 *buf,
                                         const float2 *tab, Best &best, const RAW *raw = nullptr)
{
    constexpr int NB = N / R;
    static_assert(NB % T == 0, "butterflies per pass must be a multiple of the threads per frame");
    constexpr int ITERS = NB / T;
    // the last pass writes to global memory, not to the LDS image: its butterflies need not all be in flight
    // before the first store, so they are processed one at a time (half the live registers at ITERS = 2)
    // (OUT_PIX: the last pass writes its dB values over the image it reads -- a float row, fft_frame -- so it is shaped like
    //  the passes before it: everything loaded and transformed, a barrier, then the outputs)
    constexpr bool TO_LDS = !LAST || OUT == OUT_PIX;
    constexpr int GROUP = TO_LDS ? ITERS : 1;
#pragma unroll
    for (int g0 = 0; g0 < ITERS; g0 += GROUP) {
        float2 v[GROUP][R];
#pragma unroll
        for (int gi = 0; gi < GROUP; gi++) {
            const int b = (g0 + gi) * T + tid;
            if constexpr (FIRST) {
                if (active) {
                    if constexpr (IN == IN_I16) {
                        const RAW *w = raw;
                        auto cvt = [](int s) { return SC == SC_IN ? i16_to_float_java_2p15(s) : i16_to_float_java(s); };
                        if ((a.ic | a.qc) == 0) {  // uniform: no DC correction (the usual case), two adds per sample less
#pragma unroll
                            for (int r = 0; r < R; r++)
                                v[gi][r] = make_float2(cvt((int)(short)(w[r] & 0xffff)), cvt(w[r] >> 16));
                        } else {
#pragma unroll
                            for (int r = 0; r < R; r++) {
                                int si = java_short_add((int)(short)(w[r] & 0xffff), a.ic);
                                int sq = java_short_add(w[r] >> 16, a.qc);
                                v[gi][r] = make_float2(cvt(si), cvt(sq));
                            }
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < R; r++) v[gi][r] = raw[r];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < R; r++) v[gi][r] = make_float2(0.f, 0.f);
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; r++) v[gi][r] = buf[lds_pad(b + r * NB)];
            }
            if constexpr (SC == SC_OUT) v[gi][0] = from_v(to_v(v[gi][0]) * I16_2P15_UNSCALE);
            apply_twiddles<R, P>(v[gi], b & (P - 1), tab);
            dft_reg<R>(v[gi]);
        }
        if constexpr (!FIRST && TO_LDS) __syncthreads();
#pragma unroll
        for (int gi = 0; gi < GROUP; gi++) {
            const int b = (g0 + gi) * T + tid;
            const int k = b & (P - 1);
            const int j0 = (b - k) * R + k;
            if constexpr (!LAST) {
                store_lds<R>(buf, v[gi], j0, P, std::make_integer_sequence<int, R>{});
            } else if (active) {
                if constexpr (OUT == OUT_SPEC) {
                    float2 *dst = reinterpret_cast<float2 *>(a.out) + frame_out(frame, N);
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        if constexpr (frame_is_waves(T))
                            wave_row_store(wave_row(dst, N * 8u), j0 * 8u, r * P * 8u, v[gi][cx_bitrev(r, R)]);
                        else
                            dst[j0 + r * P] = v[gi][cx_bitrev(r, R)];
                    }
                } else {
                    float *dst = a.out + frame_out(frame, N + 2);
                    float db[R];
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        db[r] = psd_db<N>(v[gi][cx_bitrev(r, R)]);
                        if constexpr (OUT == OUT_PIX) {
                            reinterpret_cast<float *>(buf)[row_pad(j0 + r * P)] = db[r];
                        } else {
#ifndef JSDR_X_FFT_NOSTORE  // timing experiment: no PSD stores (the argmax keeps the arithmetic alive)
                            // (nontemporal stores: 1.99 -> 2.39 ms, measured r02; 8-byte stores through a DPP exchange between
                            //  neighbouring lanes: 15.5 -> 16.1 ms at 8192 streams, r03)
                            if constexpr (frame_is_waves(T)) wave_row_store(wave_row(dst, (N + 2) * 4u), j0 * 4u, r * P * 4u, db[r]);
                            else dst[j0 + r * P] = db[r];
#endif
                        }
                    }
                    // first strict maximum of this thread's bins (fft.java:208-211): the group's maximum
                    // (fmaxf ignores NaN, like the reference's '>'), then the lowest bin that holds it
                    // (bins ascend with r), folded into the running best once per group
                    float gm = db[0];
#pragma unroll
                    for (int r = 1; r < R; r++) gm = fmaxf(gm, db[r]);
                    int gk = 0x7fffffff;
#pragma unroll
                    for (int r = R - 1; r >= 0; r--) gk = (db[r] == gm) ? j0 + r * P : gk;
                    const bool take = (gm > best.v) | ((gm == best.v) & (gk < best.k));  // branch-free
                    best.v = take ? gm : best.v;
                    best.k = take ? gk : best.k;
                }
            }
        }
    }
    if constexpr (!LAST) __syncthreads();
}

// One frame, executed by T threads (tid in [0,T)).  `raw` holds the frame's first-pass inputs (fft_fetch); before the
// last pass the NEXT frame's inputs are fetched into it.
template <int N, int T, int IN, int OUT, int R0, int R1, int R2, int R3, class ARGS, class FR, class FN>
__device__ __forceinline__ void fft_frame(const ARGS &a, FR frame, FN next, int tid, float2 *buf,
                                          const float2 *tw_lds, float *red_val, int *red_idx, int frame_in_block,
                                          typename RawPoint<IN>::type (&raw)[R0])
{
    using RAW = typename RawPoint<IN>::type;
    constexpr bool active = true;
    constexpr int NPASS = (R1 == 1) ? 1 : (R2 == 1) ? 2 : (R3 == 1) ? 3 : 4;
    static_assert(NPASS >= 2, "the first pass must not be the last");
    static_assert(R0 * R1 * R2 * R3 == N, "radix plan must multiply to N");
    Best best;
    best.v = -3.402823466e+38f;
    best.k = 0x7fffffff;
    constexpr int O1 = 0, O2 = tw_size(R0, R1), O3 = O2 + tw_size(R0 * R1, R2);
    constexpr bool SC = IN == IN_I16 && fft_i16_scaled(R0, R1);
    fft_pass<N, T, IN, OUT, R0, 1, true, false, RAW, SC ? SC_IN : SC_NONE>(a, frame, active, tid, buf, tw_lds, best, raw);
    // (unconditional: a workgroup's last frame fetches itself again -- with a branch around the loads the compiler cannot
    //  count what is in flight at the loop head and waits for everything, the previous frame's stores included)
    auto prefetch = [&] { fft_fetch<N, T, IN, R0>(a, next, tid, raw); };
    if constexpr (NPASS == 2) prefetch();
    fft_pass<N, T, IN, OUT, R1, R0, false, NPASS == 2, int, SC ? SC_OUT : SC_NONE>(a, frame, active, tid, buf, tw_lds + O1, best);
    if constexpr (NPASS >= 3) {
        if constexpr (NPASS == 3) prefetch();
        fft_pass<N, T, IN, OUT, R2, R0 * R1, false, NPASS == 3>(a, frame, active, tid, buf, tw_lds + O2, best);
    }
    if constexpr (NPASS >= 4) {
        prefetch();
        fft_pass<N, T, IN, OUT, R3, R0 * R1 * R2, false, NPASS == 4>(a, frame, active, tid, buf, tw_lds + O3, best);
    }

    // OUT_PIX: the last pass left the frame's dB row over the image, float[N] behind row_pad.  (The next frame's fetch is in
    // flight in `raw` and is not touched before the next first pass.)
    [[maybe_unused]] const float *row = reinterpret_cast<const float *>(buf);
    static_assert(N + (N >> 5) + 1 <= 2 * lds_frame_elems(N), "the padded row fits the image");

    if constexpr (OUT == OUT_PSD || OUT == OUT_PIX) {
        // first strict maximum (fft.java:208-211): highest value, lowest bin on ties; none if all -inf
        float bestv = best.v;
        int bestk = best.k;
        constexpr int W = (T < 64) ? T : 64;
        if constexpr (frame_is_waves(T)) {
            // whole waves: two reductions in registers (wave_reduce_i32, fft_common.h) -- the wave's maximum M, then the lowest
            // bin among the lanes that hold it -- where a butterfly of (value, bin) exchanges took six LDS round trips.
            // The maximum is taken over integer keys (f32_order_key), which order as the merge's '>' / '==' pair does on every
            // value that arrives here: a thread's best.v starts at -FLT_MAX and is replaced only by a gm with gm > best.v,
            // which no NaN and no -inf satisfies, so the lanes hold -FLT_MAX, finite values and +inf -- no NaN, and on floats
            // that are not NaN the key's order is the float order.  (+0 and -0, equal to '==', have two keys; psd_db's last
            // operation is an fma with the non-zero addend OFF, whose exact zero rounds to +0: -0 is never a dB value.)  So equal
            // keys are equal values, M is the bits of the value the merge kept, and a lane that never took a bin holds
            // k = INT_MAX, which is also what a lane below M contributes to the second reduction.  (v_max_f32 on a value that
            // came through a DPP move gets a canonicalising v_max in front of it at every step; v_max_i32 does not, and the
            // four rows combine in scalar registers.)
            const int key = f32_order_key(__builtin_bit_cast(int, bestv));
            const int mkey = wave_reduce_i32<true>(key);
            bestk = wave_reduce_i32<false>(key == mkey ? bestk : 0x7fffffff);
            bestv = __builtin_bit_cast(float, f32_order_key(mkey));
        } else {
#pragma unroll
            for (int off = W / 2; off >= 1; off >>= 1) {
                float ov = __shfl_xor(bestv, off, W);
                int ok = __shfl_xor(bestk, off, W);
                const bool take = (ov > bestv) | ((ov == bestv) & (ok < bestk));  // branch-free
                bestv = take ? ov : bestv;
                bestk = take ? ok : bestk;
            }
        }
        if constexpr (T > 64) {
            constexpr int NW = T / 64;
            int fb = frame_in_block, wv = tid >> 6;
            if constexpr (OUT == OUT_PIX) {
                // both are the same in every lane of a wave: as scalars the two LDS addresses below are made where they are used.
                // As vector registers they are kept across the frame loop, the 2048-point kernel spills them at its 128 registers,
                // and the reload -- a memory load -- waits for the next frame's fetch on its way.
                fb = __builtin_amdgcn_readfirstlane(fb);
                wv = __builtin_amdgcn_readfirstlane(wv);
            }
            if ((tid & 63) == 0) {
                red_val[fb * NW + wv] = bestv;
                red_idx[fb * NW + wv] = bestk;
            }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < NW; w++) {
                    float ov = red_val[fb * NW + w];
                    int ok = red_idx[fb * NW + w];
                    if (ov > bestv || (ov == bestv && ok < bestk)) {
                        bestv = ov;
                        bestk = ok;
                    }
                }
            }
        }
        if (tid == 0 && active) {
            // fft.java:201-224: m starts at -Float.MAX_VALUE, p at -1; Hz in wrapping int arithmetic
            int p = (bestv > -3.402823466e+38f) ? 2 * bestk : -1;
            float m = (p >= 0) ? bestv : -3.402823466e+38f;
            const int datlen = 2 * N;
            if (p >= datlen / 2) p -= datlen;
            int hz = (int)((unsigned)p * (unsigned)a.rate) / datlen;
            if constexpr (OUT == OUT_PIX) {
                if (a.peak) {
                    a.peak[frame_row(frame) * 2] = (float)hz;
                    a.peak[frame_row(frame) * 2 + 1] = m;
                }
            } else {
                float *dst = a.out + frame_out(frame, N + 2);
                dst[N] = (float)hz;
                dst[N + 1] = m;
            }
        }
    }

    if constexpr (OUT == OUT_PIX) {
        // waterfall.paintLine over the row: the frame's T threads take pixels tid, tid + T, ... -- a wave writes a contiguous
        // run of the rotated row (two where the rotation wraps inside it).  The row is complete behind the barrier of the
        // reduction above where the frame spans waves, behind this one where it does not.
        if constexpr (T <= 64) __syncthreads();
        const int width = a.width, half = width / 2;
        const float step = wf_step(N, width);
        const int l = java_f2i(step);
        const WfColour colour = wf_colour(a.peak_rgb);
        unsigned *prow = a.pix + frame_row(frame) * width;
        float *mrow = a.maxo ? a.maxo + frame_row(frame) * width : nullptr;
        for (int p = tid; p < width; p += T) {
            const float r = wf_getmax([&](int i) { return row[row_pad(i)]; }, java_f2i((float)p * step), l);
            if (mrow) mrow[p] = r;
            const int q = p + half;  // (p + width / 2) % width
            prow[q >= width ? q - width : q] = wf_pixel(r, colour);
        }
    }
}

#ifdef JSDR_X_WGCLK  // timing probe (round 9, never defined in the product build): every workgroup's first and last s_memrealtime tick
                     // (10 ns, one clock for the chip -- s_memtime counts shader clocks from a base of its own on every XCD) and its
                     // frame groups, a row per launch; written to a file when a handle goes (profiles/r09_ticket_handout.md)
constexpr int WGCLK_SLOTS = 128, WGCLK_WGS = 1024;
__device__ unsigned long long g_fft_wgclk[WGCLK_SLOTS][WGCLK_WGS][3];
#endif

// TWG: the twiddle tables are read from global memory (L1 / L2) instead of a per-workgroup copy in LDS
template <int N, int T, int FPB, int IN, int OUT, int R0, int R1, int R2, int R3, bool TWG = false>
__global__ __launch_bounds__(T *FPB, (N == 2048 ? 4 : 1)) void k_fft(FftArgs a)
{
#include "fft_block_body.h"
}

// the fused fft.receive + waterfall.paintLine form: k_fft's frame loop with OUT_PIX.  (8192: three waves a SIMD as k_fft has
// them -- left alone the int16 form takes 170 registers, two more than that allows, and a CU holds one workgroup, not two)
template <int N, int T, int FPB, int IN, int R0, int R1, int R2, int R3>
__global__ __launch_bounds__(T *FPB, (N == 2048 ? 4 : N == 8192 ? 3 : 1)) void k_fft_pix(FftPixArgs a)
{
    constexpr int OUT = OUT_PIX;
    constexpr bool TWG = false;
#include "fft_block_body.h"
}

// The strided form of both (jsdr_fft_batch_streams_* / jsdr_fft_waterfall_streams_*; ARGS = Strided<FftArgs> / Strided<FftPixArgs>):
// the same frame loop with a position where k_fft has a frame number.  Each of a workgroup's FPB frames maps on its own -- a
// group of frames straddles two streams -- by one division when the workgroup starts; the persistent loop walks from there
// (StreamGeom, fft_common.h).  What a surplus part-workgroup redoes is the launch's last frame, as in k_fft.
//   T >= 64, a wave holds one frame: the frame's slot in the workgroup is made a scalar, and with it the whole position -- the
//            walk is scalar arithmetic and takes no vector register from the frame loop.
//   T <  64, a wave holds 64 / T frames with a position each: the positions live in LDS, a slot a frame, and are read where
//            they are used -- the offset of the next frame's input at its fetch (which is also where the walk steps: before
//            the last pass, registers to spare), the row's offset at the stores.  As vector registers they were live through
//            every pass and cost the 64- to 256-point kernels a wave a SIMD.  A frame's threads are lanes of one wave: they
//            read and write their slot in step, all the same values.
struct LdsFrame {
    const long long *slot;  // {j, in, out: of the frame being fetched or fetched last; out of the frame in flight}
    long long f;            // the frame in flight (clamped): the row of the packed outputs
};
struct LdsNext {
    long long *slot;
    const StreamGeom *g;
    long long step;
    bool more, past;  // the workgroup has a further group of frames; that one lies past the launch's last frame
};
__device__ __forceinline__ long long frame_out(const LdsFrame &p, int) { return p.slot[3]; }
__device__ __forceinline__ long long frame_row(const LdsFrame &p) { return p.f; }
__device__ __forceinline__ long long frame_in(const LdsNext &q, int)
{
    if (!q.more) return q.slot[1];  // the last group fetches itself again
    FramePos p;
    p.f = 0;
    p.j = q.slot[0];
    p.in = q.slot[1];
    p.out = q.slot[2];
    stream_step(*q.g, p, q.step);
    if (q.past) {
        p.in = q.g->last_in;
        p.out = q.g->last_out;
    }
    q.slot[0] = p.j;
    q.slot[1] = p.in;
    q.slot[2] = p.out;
    return p.in;
}

template <int N, int T, int FPB, int IN, int OUT, int R0, int R1, int R2, int R3, class ARGS>
__global__ __launch_bounds__(T *FPB, (N == 2048 ? 4 : (N == 8192 && OUT == OUT_PIX) ? 3 : N == 64 ? 8 : (N == 4096 && OUT == OUT_PSD) ? 4 : (N == 128 && OUT == OUT_PIX && IN == IN_F32) ? 6 : 1)) void k_fft_streams(ARGS a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int FE = lds_frame_elems(N);
    constexpr int TWN = tw_total(R0, R1, R2, R3);
    float2 *tw_own = reinterpret_cast<float2 *>(smem);                    // [TWN]
    float2 *bufs = tw_own + TWN;                                          // [FPB][FE]
    float *red_val = reinterpret_cast<float *>(bufs + (size_t)FPB * FE);  // [FPB*NW]
    int *red_idx = reinterpret_cast<int *>(red_val + FPB * ((T + 63) / 64));
    [[maybe_unused]] long long *slots = reinterpret_cast<long long *>(red_idx + FPB * ((T + 63) / 64));  // [FPB][4], T < 64

    const int tid_b = threadIdx.x;
    for (int i = tid_b; i < TWN; i += T * FPB) tw_own[i] = a.tw[i];
    __syncthreads();

    int fib = FPB == 1 ? 0 : tid_b / T;  // (said outright where the workgroup is one frame: the 4096-point kernel fits its 128 registers with it)
    const int tid = tid_b - fib * T;
    if constexpr (T >= 64 && FPB > 1) fib = __builtin_amdgcn_readfirstlane(fib);
    float2 *buf = bufs + (size_t)fib * FE;
    const long long ngroups = (a.nframes + FPB - 1) / FPB;
    const long long step = (long long)gridDim.x * FPB;
    if ((long long)blockIdx.x >= ngroups) return;
    auto clamped = [&](FramePos p) {
        if (p.f >= a.nframes) {
            p.f = a.nframes - 1;
            p.in = a.g.last_in;
            p.out = a.g.last_out;
        }
        return p;
    };
    typename RawPoint<IN>::type raw[R0];
    if constexpr (T >= 64) {
        FramePos walk = stream_pos(a.g, (long long)blockIdx.x * FPB + fib);  // (unclamped: the walk goes on from where it is)
        FramePos cur = clamped(walk);
        fft_fetch<N, T, IN, R0>(a, cur, tid, raw);
        for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
            FramePos next = cur;
            if (g + gridDim.x < ngroups) {
                stream_step(a.g, walk, step);
                next = clamped(walk);
            }
            fft_frame<N, T, IN, OUT, R0, R1, R2, R3>(a, cur, next, tid, buf, tw_own, red_val, red_idx, fib, raw);
            __syncthreads();
            cur = next;
        }
    } else {
        long long *slot = slots + 4 * fib;
        {
            const FramePos first = clamped(stream_pos(a.g, (long long)blockIdx.x * FPB + fib));
            slot[0] = first.j;
            slot[1] = first.in;
            slot[2] = first.out;
            fft_fetch<N, T, IN, R0>(a, first, tid, raw);
        }
        for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
            slot[3] = slot[2];
            const long long f = g * FPB + fib, fn = f + step;
            const LdsFrame cur = {slot, f < a.nframes ? f : a.nframes - 1};
            const LdsNext next = {slot, &a.g, step, g + gridDim.x < ngroups, fn >= a.nframes};
            fft_frame<N, T, IN, OUT, R0, R1, R2, R3>(a, cur, next, tid, buf, tw_own, red_val, red_idx, fib, raw);
            __syncthreads();
        }
    }
}

template <int N, int FPB, int T, int R0, int R1, int R2, int R3, bool TWG = false>
constexpr size_t fft_lds_bytes()
{
    return sizeof(float2) * ((TWG ? (size_t)0 : (size_t)tw_total(R0, R1, R2, R3)) + (size_t)FPB * lds_frame_elems(N)) +
           (sizeof(float) + sizeof(int)) * FPB * ((T + 63) / 64);
}

struct Launcher {
    void (*launch)(const FftArgs &, int grid, hipStream_t) = nullptr;
    void (*launch_pix)(const FftPixArgs &, int grid, hipStream_t) = nullptr;  // out == OUT_PIX
    void (*launch_s)(const Strided<FftArgs> &, int grid, hipStream_t) = nullptr;         // k_fft_streams, out == OUT_PSD
    void (*launch_pix_s)(const Strided<FftPixArgs> &, int grid, hipStream_t) = nullptr;  // k_fft_streams, out == OUT_PIX
    int frames_per_block = 0;
    size_t lds_bytes = 0;
    int block = 0;
    int radix[4] = {1, 1, 1, 1};
};

template <int N, int T, int FPB, int IN, int OUT, int R0, int R1, int R2, int R3, bool TWG = false>
static void launch_impl(const FftArgs &a, int grid, hipStream_t s)
{
    constexpr size_t lds = fft_lds_bytes<N, FPB, T, R0, R1, R2, R3, TWG>();
    hipLaunchKernelGGL((k_fft<N, T, FPB, IN, OUT, R0, R1, R2, R3, TWG>), dim3(grid), dim3(T * FPB), lds, s, a);
}

template <int N, int T, int FPB, int IN, int R0, int R1, int R2, int R3>
static void launch_pix_impl(const FftPixArgs &a, int grid, hipStream_t s)
{
    constexpr size_t lds = fft_lds_bytes<N, FPB, T, R0, R1, R2, R3, false>();
    hipLaunchKernelGGL((k_fft_pix<N, T, FPB, IN, R0, R1, R2, R3>), dim3(grid), dim3(T * FPB), lds, s, a);
}

template <int N, int T, int FPB, int IN, int OUT, int R0, int R1, int R2, int R3, class ARGS>
static void launch_streams_impl(const ARGS &a, int grid, hipStream_t s)
{
    constexpr size_t lds = fft_lds_bytes<N, FPB, T, R0, R1, R2, R3, false>() + (T < 64 ? sizeof(long long) * 4 * FPB : 0);
    hipLaunchKernelGGL((k_fft_streams<N, T, FPB, IN, OUT, R0, R1, R2, R3, ARGS>), dim3(grid), dim3(T * FPB), lds, s, a);
}

template <int N, int T, int FPB, int R0, int R1, int R2, int R3, bool TWG = false>
static Launcher make_launcher(int in, int out)
{
    Launcher l;
    l.frames_per_block = FPB;
    l.block = T * FPB;
    l.lds_bytes = fft_lds_bytes<N, FPB, T, R0, R1, R2, R3, TWG>();
    l.radix[0] = R0;
    l.radix[1] = R1;
    l.radix[2] = R2;
    l.radix[3] = R3;
    if (in == IN_I16 && out == OUT_PSD) l.launch = launch_impl<N, T, FPB, IN_I16, OUT_PSD, R0, R1, R2, R3, TWG>;
    if (in == IN_F32 && out == OUT_PSD) l.launch = launch_impl<N, T, FPB, IN_F32, OUT_PSD, R0, R1, R2, R3, TWG>;
    if (in == IN_F32 && out == OUT_SPEC) l.launch = launch_impl<N, T, FPB, IN_F32, OUT_SPEC, R0, R1, R2, R3, TWG>;
    if constexpr (!TWG) {
        if (in == IN_I16 && out == OUT_PIX) l.launch_pix = launch_pix_impl<N, T, FPB, IN_I16, R0, R1, R2, R3>;
        if (in == IN_F32 && out == OUT_PIX) l.launch_pix = launch_pix_impl<N, T, FPB, IN_F32, R0, R1, R2, R3>;
        if (in == IN_I16 && out == OUT_PSD) l.launch_s = launch_streams_impl<N, T, FPB, IN_I16, OUT_PSD, R0, R1, R2, R3, Strided<FftArgs>>;
        if (in == IN_F32 && out == OUT_PSD) l.launch_s = launch_streams_impl<N, T, FPB, IN_F32, OUT_PSD, R0, R1, R2, R3, Strided<FftArgs>>;
        if (in == IN_I16 && out == OUT_PIX) l.launch_pix_s = launch_streams_impl<N, T, FPB, IN_I16, OUT_PIX, R0, R1, R2, R3, Strided<FftPixArgs>>;
        if (in == IN_F32 && out == OUT_PIX) l.launch_pix_s = launch_streams_impl<N, T, FPB, IN_F32, OUT_PIX, R0, R1, R2, R3, Strided<FftPixArgs>>;
    }
    return l;
}

static Launcher pick_launcher(int n, int in, int out)
{
    switch (n) {
        case 64: return make_launcher<64, 8, 32, 8, 8, 1, 1>(in, out);
        case 128: return make_launcher<128, 8, 32, 16, 8, 1, 1>(in, out);
        case 256: return make_launcher<256, 16, 16, 16, 16, 1, 1>(in, out);
        case 512: return make_launcher<512, 64, 4, 8, 8, 8, 1>(in, out);
        case 1024: return make_launcher<1024, 64, 4, 16, 8, 8, 1>(in, out);
        // (round 5, measured and not kept -- profiles/r05_experiments.md: one frame per 128-thread workgroup with the tables in LDS
        //  17.0-17.1 ms, one frame with the tables read from global memory (make_launcher<..., true>) 16.7-17.3, two frames with
        //  global tables 17.05, against 15.8 for this form)
        case 2048: return make_launcher<2048, 128, 2, 16, 16, 8, 1>(in, out);
        case 4096: return make_launcher<4096, 256, 1, 16, 16, 16, 1>(in, out);
        case 8192: return make_launcher<8192, 512, 1, 16, 16, 8, 4>(in, out);
        default: return Launcher();
    }
}

// jsdr_fft_waterfall_* on a frame size the fused kernel does not serve: what k_waterfall does not write -- the pooled maxima,
// unrotated (fft.paintComponent's getMax, fft.java:147), and the row's two trailing floats -- from the PSD rows of a chunk.
// One workgroup a frame, grid-stride; the rows were written a kernel ago and are read from cache.
__global__ __launch_bounds__(256) void k_waterfall_aux(const float *__restrict__ psd, long long nframes, int n, int width,
                                                       float *__restrict__ maxo, float *__restrict__ peak)
{
    const float step = wf_step(n, width);
    const int l = java_f2i(step);
    for (long long frame = blockIdx.x; frame < nframes; frame += gridDim.x) {
        const float *a = psd + frame * (n + 2);
        if (maxo)
            for (int p = threadIdx.x; p < width; p += 256)
                maxo[frame * width + p] = wf_getmax([&](int i) { return a[i]; }, java_f2i((float)p * step), l);
        if (peak && threadIdx.x < 2) peak[frame * 2 + threadIdx.x] = a[n + threadIdx.x];
    }
}

}  // namespace jsdr

using namespace jsdr;

struct jsdr_fft {
    int n = 0;
    int rate = 0;
    DevBuf<float2> tw;
    DevBuf<float2> tw_i16;           // k_fft's int16 launches: `tw` with the second pass's segment times 2^-15 (fft_pass, SC)
    DevBuf<unsigned char> in_stage;  // one frame, for the host-buffer receive() forms
    DevBuf<float> out_stage;
    PinnedStage pin;                 // [frame in (8 n bytes) | psd out (4 (n + 2) bytes)] for the receive() forms
    bool pin_lazy_done = false;      // the stage is allocated at the first receive()
    int num_cu = 256;
    bool mixed = false;  // non power-of-two frame: fft_mixed.hip
    MixedPlan mplan;
    bool rt = false;      // any other 2^a 3^b 5^c 7^d frame up to 9800 samples: fft_rt.hip
    bool direct = false;  // any other frame size: fft_any.hip
    long long last_items = 0, last_grid = 0;  // jsdr_fft_last_launch
    int share_wgs_per_cu = 0;  // jsdr_fft_set_cu_share: workgroups per CU the batch kernel is held to (0: all it can use)
    // jsdr_fft_waterfall_*: frames the fused kernel does not serve go through PSD rows of the handle's own, WF_CHUNK at the most
    DevBuf<float> wf_rows;
    std::string wf_kernel;  // jsdr_fft_waterfall_kernel
};
constexpr long long WF_CHUNK = 1024;

#ifdef JSDR_X_WGCLK
static long long g_wgclk_log[WGCLK_SLOTS][3];  // per launch row: frame groups, grid, launch number
static void fft_wgclk_report()
{
    const char *path = getenv("JSDR_X_WGCLK_OUT");
    FILE *f = fopen(path ? path : "wgclk_fft.csv", "w");
    static unsigned long long cc[WGCLK_SLOTS][WGCLK_WGS][3];
    if (f && hipMemcpyFromSymbol(cc, HIP_SYMBOL(g_fft_wgclk), sizeof(cc)) == hipSuccess) {
        fprintf(f, "launch,items,grid,ticket,wg,t0,t1,n\n");
        for (int sl = 0; sl < WGCLK_SLOTS; sl++)
            for (int w = 0; w < WGCLK_WGS && w < g_wgclk_log[sl][1]; w++)
                fprintf(f, "%lld,%lld,%lld,0,%d,%llu,%llu,%llu\n", g_wgclk_log[sl][2], g_wgclk_log[sl][0], g_wgclk_log[sl][1], w,
                        cc[sl][w][0], cc[sl][w][1], cc[sl][w][2]);
    }
    if (f) fclose(f);
}
#endif

template <class ARGS>
static int fft_launch_pow2(jsdr_fft *h, ARGS &a, int in_kind, int out_kind, hipStream_t s);

static int fft_run(jsdr_fft *h, const void *in_dev, int in_kind, int out_kind, long long nframes, int ic, int qc,
                   float *out_dev, hipStream_t s)
{
    JSDR_REQUIRE(h, "fft: null handle");
    JSDR_REQUIRE(in_dev && out_dev, "fft: null buffer");
    JSDR_REQUIRE(nframes >= 0, "fft: negative frame count");
    if (nframes == 0) return JSDR_OK;
    FftArgs a;
    if (h->rt) {
        a.in = in_dev;
        a.out = out_dev;
        a.tw = h->tw.p;
        a.nframes = nframes;
        a.rate = h->rate;
        a.ic = ic;
        a.qc = qc;
        return rt_launch(a, h->n, in_kind, out_kind, h->num_cu, s);
    }
    if (h->direct) {
        a.in = in_dev;
        a.out = out_dev;
        a.tw = nullptr;
        a.nframes = nframes;
        a.rate = h->rate;
        a.ic = ic;
        a.qc = qc;
        return dft_any_launch(a, h->n, in_kind, out_kind, h->num_cu, s);
    }
    if (h->mixed) {
        a.in = in_dev;
        a.out = out_dev;
        a.tw = h->tw.p;
        a.nframes = nframes;
        a.rate = h->rate;
        a.ic = ic;
        a.qc = qc;
        if (h->mplan.split2)
            return mixed_launch_split2(h->mplan, a, in_kind, out_kind, h->num_cu, s);
        static const int mgrid = [] { const char *e = knob("JSDR_MIXED_GRID"); return e ? atoi(e) : 16; }();  // workgroups per CU: shorter workgroups balance the tail (2: 3.84, 16: 3.56 ms at n = 9600)
        long long cap = (long long)h->num_cu * mgrid;
        return mixed_launch(h->mplan, a, in_kind, out_kind, (int)(nframes < cap ? nframes : cap), s);
    }
    a.in = in_dev;
    a.out = out_dev;
    a.tw = in_kind == IN_I16 ? h->tw_i16.p : h->tw.p;
    a.nframes = nframes;
    a.rate = h->rate;
    a.ic = ic;
    a.qc = qc;
    return fft_launch_pow2(h, a, in_kind, out_kind, s);
}

// frames [f0, f0 + nframes) of a strided call (StreamRows) into PSD rows: the strided instantiation of the handle's kernel
struct StreamRows {
    long long fps;         // frames per stream
    long long in_stride;   // points between two streams' first frames
    long long out_stride;  // floats between two streams' first PSD rows
};
static int fft_run_streams(jsdr_fft *h, const void *in_dev, int in_kind, const StreamRows &r, long long f0, long long nframes,
                           long long out_base, int ic, int qc, float *out_dev, hipStream_t s)
{
    Strided<FftArgs> a;
    a.in = in_dev;
    a.out = out_dev;
    a.tw = h->direct ? nullptr : (!h->rt && !h->mixed && in_kind == IN_I16) ? h->tw_i16.p : h->tw.p;
    a.nframes = nframes;
    a.rate = h->rate;
    a.ic = ic;
    a.qc = qc;
    a.g = stream_geom(h->n, r.fps, r.in_stride, r.out_stride, f0, nframes, out_base);
    if (h->rt) return rt_launch_streams(a, h->n, in_kind, h->num_cu, s);
    if (h->direct) return dft_any_launch_streams(a, h->n, in_kind, h->num_cu, s);
    if (h->mixed) {
        if (h->mplan.split2) return mixed_launch_split2_streams(h->mplan, a, in_kind, h->num_cu, s);
        static const int mgrid = [] { const char *e = knob("JSDR_MIXED_GRID"); return e ? atoi(e) : 16; }();  // (as fft_run)
        const long long cap = (long long)h->num_cu * mgrid;
        return mixed_launch_streams(h->mplan, a, in_kind, (int)(nframes < cap ? nframes : cap), s);
    }
    return fft_launch_pow2(h, a, in_kind, OUT_PSD, s);
}

// the power-of-two kernel, PSD / spectrum (FftArgs) or pixel form (FftPixArgs), contiguous or Strided<>: one launch geometry for all
template <class ARGS>
static int fft_launch_pow2(jsdr_fft *h, ARGS &a, int in_kind, int out_kind, hipStream_t s)
{
    const long long nframes = a.nframes;
    Launcher l = pick_launcher(h->n, in_kind, out_kind);
    constexpr bool PIX = std::is_base_of<FftPixArgs, ARGS>::value, STR = is_strided<ARGS>::value;
    const auto launch = [&] {
        if constexpr (PIX && STR) return l.launch_pix_s;
        else if constexpr (STR) return l.launch_s;
        else if constexpr (PIX) return l.launch_pix;
        else return l.launch;
    }();
    JSDR_REQUIRE(launch != nullptr, "fft: no kernel for n=%d in=%d out=%d", h->n, in_kind, out_kind);
    long long groups = (nframes + l.frames_per_block - 1) / l.frames_per_block;
    // enough workgroups to fill every CU at the LDS-limited occupancy, grid-stride over the rest
    long long per_cu = (long long)(160 * 1024 / l.lds_bytes);
    if (per_cu < 1) per_cu = 1;
    if (per_cu * l.block > 2048) per_cu = 2048 / l.block;
    static const int mult = [] {
        const char *e = knob("JSDR_FFT_GRID_MULT");  // tuning knob: workgroups per resident slot
        const int v = e ? atoi(e) : 0;
        return v > 0 ? v : 4;
    }();
    long long cap = (long long)h->num_cu * per_cu * mult;
    static const int abs_grid = [] {
        const char *e = knob("JSDR_FFT_GRID_ABS");  // tuning knob: total workgroups (co-residency experiments: 2 per CU = 512)
        return e ? atoi(e) : 0;
    }();
    if (abs_grid > 0) cap = abs_grid;
    // a caller that runs the demodulator BESIDE this kernel (jsdr_fft_set_cu_share): exactly that many persistent workgroups
    // per CU, so that both kernels' workgroups are resident from the start whichever is launched first
    if (h->share_wgs_per_cu > 0) cap = (long long)h->num_cu * h->share_wgs_per_cu;
    int grid = (int)(groups < cap ? groups : cap);
    h->last_items = groups;
    h->last_grid = grid;
#ifdef JSDR_X_WGCLK
    {
        static int wgclk_seq = 0;
        a.wgclk_slot = wgclk_seq % WGCLK_SLOTS;
        g_wgclk_log[a.wgclk_slot][0] = groups;
        g_wgclk_log[a.wgclk_slot][1] = grid;
        g_wgclk_log[a.wgclk_slot][2] = wgclk_seq++;
    }
#endif
    if constexpr (STR) stream_geom_step(a.g, (long long)grid * l.frames_per_block);
    launch(a, grid, s);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

extern "C" {

int jsdr_fft_create(jsdr_fft **out, int n, int rate)
{
    JSDR_REQUIRE(out, "jsdr_fft_create: null handle pointer");
    *out = nullptr;
    MixedPlan mp;
    const bool pow2 = n >= 64 && n <= 8192 && (n & (n - 1)) == 0;
    const bool mixed = !pow2 && mixed_plan(n, mp);
    const bool rt = !pow2 && !mixed && rt_supported(n);
    const bool direct = !pow2 && !mixed && !rt && dft_any_supported(n);
    JSDR_REQUIRE(pow2 || mixed || rt || direct,
                 "jsdr_fft_create: n=%d unsupported (2 .. 20000 samples)", n);
    JSDR_REQUIRE(rate > 0, "jsdr_fft_create: rate must be positive");
    int dev = 0;
    JSDR_HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    JSDR_HIP_TRY(hipGetDeviceProperties(&prop, dev));
    jsdr_fft *h = new jsdr_fft();
    h->n = n;
    h->rate = rate;
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (direct) {  // no tables: the twiddles are computed where they are used
        h->direct = true;
        if (h->in_stage.alloc((size_t)n * 8) != JSDR_OK || h->out_stage.alloc((size_t)n + 2) != JSDR_OK) {
            jsdr_fft_destroy(h);
            return JSDR_ERR;
        }
        *out = h;
        return JSDR_OK;
    }
    if (rt) {
        h->rt = true;
        std::vector<float2> rtw;
        rt_twiddles(n, rtw);
        if (h->tw.alloc(rtw.size() ? rtw.size() : 1) != JSDR_OK || h->in_stage.alloc((size_t)n * 8) != JSDR_OK ||
            h->out_stage.alloc((size_t)n + 2) != JSDR_OK ||
            (rtw.size() && hipMemcpy(h->tw.p, rtw.data(), sizeof(float2) * rtw.size(), hipMemcpyHostToDevice) != hipSuccess)) {
            set_error("jsdr_fft_create: run-time-plan setup failed");
            jsdr_fft_destroy(h);
            return JSDR_ERR;
        }
        *out = h;
        return JSDR_OK;
    }
    if (mixed) {
        h->mixed = true;
        h->mplan = mp;
        std::vector<float2> mtw((size_t)mp.tw_count);
        mixed_twiddles(mp, mtw.data());
        if (h->tw.alloc(mtw.size()) != JSDR_OK || h->in_stage.alloc((size_t)n * 8) != JSDR_OK ||
            h->out_stage.alloc((size_t)n + 2) != JSDR_OK ||
            hipMemcpy(h->tw.p, mtw.data(), sizeof(float2) * mtw.size(), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("jsdr_fft_create: mixed-radix setup failed");
            jsdr_fft_destroy(h);
            return JSDR_ERR;
        }
        *out = h;
        return JSDR_OK;
    }
    // per-pass twiddle tables in the layout fft_pass expects (tw_direct / tw_size above)
    Launcher l = pick_launcher(n, IN_I16, OUT_PSD);
    std::vector<float2> tw;
    int P = l.radix[0];
    for (int pass = 1; pass < 4 && l.radix[pass] > 1; pass++) {
        const int R = l.radix[pass];
        const double base = -2.0 * 3.14159265358979323846 / ((double)P * (double)R);
        if (tw_direct(P, R)) {
            for (int r = 1; r < R; r++)  // row 0 is all ones and never read (and its 256 bytes decide whether a
                                         // fourth 2048-point workgroup fits a CU's LDS)
                for (int k = 0; k < P; k++) {
                    double ang = base * (double)k * (double)r;
                    const float2 w = make_float2((float)cos(ang), (float)sin(ang));
                    tw.push_back(w);
                    tw.push_back(make_float2(-w.y, w.x));
                }
        } else {
            for (int k = 0; k < P; k++) {
                double ang = base * (double)k;
                tw.push_back(make_float2((float)cos(ang), (float)sin(ang)));
            }
        }
        P *= R;
    }
    if ((int)tw.size() != tw_total(l.radix[0], l.radix[1], l.radix[2], l.radix[3])) {
        set_error("jsdr_fft_create: internal twiddle layout mismatch (%d)", (int)tw.size());
        delete h;
        return JSDR_ERR;
    }
    // the int16 launches' copy: the second pass's segment (the table's first) takes the conversion's 2^15 out again
    std::vector<float2> tw16(tw);
    if (fft_i16_scaled(l.radix[0], l.radix[1]))
        for (int i = 0; i < tw_size(l.radix[0], l.radix[1]); i++)
            tw16[i] = make_float2(tw16[i].x * I16_2P15_UNSCALE, tw16[i].y * I16_2P15_UNSCALE);
    if (h->tw.alloc(tw.size()) != JSDR_OK || h->tw_i16.alloc(tw16.size()) != JSDR_OK ||
        h->in_stage.alloc((size_t)n * 8) != JSDR_OK || h->out_stage.alloc((size_t)n + 2) != JSDR_OK) {
        jsdr_fft_destroy(h);
        return JSDR_ERR;
    }
    if (hipMemcpy(h->tw.p, tw.data(), sizeof(float2) * tw.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->tw_i16.p, tw16.data(), sizeof(float2) * tw16.size(), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("jsdr_fft_create: twiddle upload failed");
        jsdr_fft_destroy(h);
        return JSDR_ERR;
    }
    *out = h;
    return JSDR_OK;
}

int jsdr_fft_destroy(jsdr_fft *h)
{
#ifdef JSDR_X_WGCLK
    if (h) {
        (void)hipDeviceSynchronize();
        fft_wgclk_report();
    }
#endif
    delete h;
    return JSDR_OK;
}

int jsdr_fft_batch_f32(jsdr_fft *h, const float *iq_dev, int64_t nframes, float *psd_dev, void *stream)
{
    return fft_run(h, iq_dev, IN_F32, OUT_PSD, nframes, 0, 0, psd_dev, as_stream(stream));
}

int jsdr_fft_set_cu_share(jsdr_fft *h, int wgs_per_cu)
{
    JSDR_REQUIRE(h && wgs_per_cu >= 0 && wgs_per_cu <= 16, "jsdr_fft_set_cu_share: bad argument");
    h->share_wgs_per_cu = wgs_per_cu;
    return JSDR_OK;
}

const char *jsdr_fft_kernel(jsdr_fft *h)
{
    if (!h) return "";
    return h->rt ? "k_fft_rt" : h->direct ? "k_dft_any" : h->mixed ? (h->mplan.split2 ? "k_fft_mixed_dual" : "k_fft_mixed") : "k_fft";
}

int jsdr_fft_last_launch(jsdr_fft *h, int64_t *work_items, int64_t *workgroups)
{
    JSDR_REQUIRE(h && work_items && workgroups, "jsdr_fft_last_launch: null argument");
    *work_items = h->last_items;
    *workgroups = h->last_grid;
    return JSDR_OK;
}

int jsdr_fft_batch_i16(jsdr_fft *h, const int16_t *raw_dev, int64_t nframes, int ic, int qc, float *psd_dev,
                       void *stream)
{
    return fft_run(h, raw_dev, IN_I16, OUT_PSD, nframes, ic, qc, psd_dev, as_stream(stream));
}

int jsdr_fft_spectrum_f32(jsdr_fft *h, const float *iq_dev, int64_t nframes, float *spec_dev, void *stream)
{
    return fft_run(h, iq_dev, IN_F32, OUT_SPEC, nframes, 0, 0, spec_dev, as_stream(stream));
}

// fft.receive + waterfall.paintLine of a batch: the fused kernel where the frame is a power of two, otherwise the handle's
// batch kernel into PSD rows of the handle's own (WF_CHUNK at a time), k_waterfall over them and k_waterfall_aux for the rest
static const char *fft_waterfall_name(jsdr_fft *h)
{
    const bool pow2 = !h->rt && !h->direct && !h->mixed;
    h->wf_kernel = pow2 ? std::string("k_fft_pix") : std::string(jsdr_fft_kernel(h)) + "+k_waterfall";
    return h->wf_kernel.c_str();
}

// (sr: the frames are those of a strided call, nframes of them in all, and the rows of every output are packed in that order)
static int fft_waterfall(const char *who, jsdr_fft *h, const void *in_dev, int in_kind, long long nframes, int ic, int qc,
                         int width, uint32_t peak_rgb, uint32_t *pix_dev, float *max_dev, float *peak_dev, hipStream_t s,
                         const StreamRows *sr = nullptr)
{
    JSDR_REQUIRE(h, "%s: null handle", who);
    JSDR_REQUIRE(in_dev, "%s: null %s", who, in_kind == IN_I16 ? "raw_dev" : "iq_dev");
    JSDR_REQUIRE(pix_dev, "%s: null pix_dev", who);
    JSDR_REQUIRE(width > 0, "%s: width=%d must be positive", who, width);
    JSDR_REQUIRE(nframes >= 0, "%s: nframes=%lld is negative", who, nframes);
    if (nframes == 0) return JSDR_OK;
    if (!h->rt && !h->direct && !h->mixed) {
        FftPixArgs a;
        a.in = in_dev;
        a.out = nullptr;
        a.tw = in_kind == IN_I16 ? h->tw_i16.p : h->tw.p;
        a.nframes = nframes;
        a.rate = h->rate;
        a.ic = ic;
        a.qc = qc;
        a.pix = reinterpret_cast<unsigned *>(pix_dev);
        a.maxo = max_dev;
        a.peak = peak_dev;
        a.width = width;
        a.peak_rgb = (unsigned)peak_rgb;
        if (sr) {
            Strided<FftPixArgs> b;
            static_cast<FftPixArgs &>(b) = a;
            b.g = stream_geom(h->n, sr->fps, sr->in_stride, sr->out_stride, 0, nframes, 0);
            return fft_launch_pow2(h, b, in_kind, OUT_PIX, s);
        }
        return fft_launch_pow2(h, a, in_kind, OUT_PIX, s);
    }
    const long long n = h->n, rows = nframes < WF_CHUNK ? nframes : WF_CHUNK;
    // (a larger chunk than any before: the release inside alloc waits for the device, so no earlier call still uses the rows)
    if (h->wf_rows.n < (size_t)(rows * (n + 2)) && h->wf_rows.alloc((size_t)(rows * (n + 2))) != JSDR_OK) return JSDR_ERR;
    const size_t in_frame = (size_t)n * (in_kind == IN_I16 ? 2 * sizeof(int16_t) : 2 * sizeof(float));
    for (long long f0 = 0; f0 < nframes; f0 += WF_CHUNK) {
        const long long nf = nframes - f0 < WF_CHUNK ? nframes - f0 : WF_CHUNK;
        // (a strided call's chunk holds the end of one stream and the start of the next wherever fps does not divide WF_CHUNK)
        if ((sr ? fft_run_streams(h, in_dev, in_kind, *sr, f0, nf, -f0 * (n + 2), ic, qc, h->wf_rows.p, s)
                : fft_run(h, static_cast<const unsigned char *>(in_dev) + (size_t)f0 * in_frame, in_kind, OUT_PSD, nf, ic, qc,
                          h->wf_rows.p, s)) != JSDR_OK)
            return JSDR_ERR;
        if (jsdr_waterfall_lines(h->wf_rows.p, nf, (int)n, width, peak_rgb, pix_dev + f0 * width, s) != JSDR_OK) return JSDR_ERR;
        if (max_dev || peak_dev) {
            hipLaunchKernelGGL(k_waterfall_aux, dim3((unsigned)nf), dim3(256), 0, s, h->wf_rows.p, nf, (int)n, width,
                               max_dev ? max_dev + f0 * width : nullptr, peak_dev ? peak_dev + f0 * 2 : nullptr);
            JSDR_LAUNCH_CHECK();
        }
    }
    return JSDR_OK;
}

// one frame from / to host buffers: through the handle's pinned stage when it has one (PinnedStage, common.h)
static int fft_receive(jsdr_fft *h, const void *in_host, size_t in_bytes, int in_kind, int ic, int qc, float *psd_host)
{
    const size_t out_bytes = sizeof(float) * ((size_t)h->n + 2), in_room = (size_t)h->n * 8;
    if (h->pin.p && h->pin.bytes >= in_room + out_bytes) {
        memcpy(h->pin.p, in_host, in_bytes);
        SyncOnExit guard;  // (an error exit below must not leave the device reading or writing the stage)
        JSDR_HIP_TRY(hipMemcpyAsync(h->in_stage.p, h->pin.p, in_bytes, hipMemcpyHostToDevice, 0));
        if (fft_run(h, h->in_stage.p, in_kind, OUT_PSD, 1, ic, qc, h->out_stage.p, 0) != JSDR_OK) return JSDR_ERR;
        JSDR_HIP_TRY(hipMemcpyAsync(h->pin.p + in_room, h->out_stage.p, out_bytes, hipMemcpyDeviceToHost, 0));
        JSDR_HIP_TRY(hipStreamSynchronize(0));
        guard.armed = false;
        memcpy(psd_host, h->pin.p + in_room, out_bytes);
        return JSDR_OK;
    }
    JSDR_HIP_TRY(hipMemcpy(h->in_stage.p, in_host, in_bytes, hipMemcpyHostToDevice));
    if (fft_run(h, h->in_stage.p, in_kind, OUT_PSD, 1, ic, qc, h->out_stage.p, 0) != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipMemcpy(psd_host, h->out_stage.p, out_bytes, hipMemcpyDeviceToHost));
    return JSDR_OK;
}

int jsdr_fft_receive_f32(jsdr_fft *h, const float *iq_host, float *psd_host)
{
    JSDR_REQUIRE(h && iq_host && psd_host, "jsdr_fft_receive_f32: null argument");
    if (!h->pin_lazy_done && !h->pin.p) {  // the first receive() of a handle: batch-only handles never pin anything
        h->pin.alloc((size_t)h->n * 8 + sizeof(float) * ((size_t)h->n + 2));
        h->pin_lazy_done = true;
    }
    return fft_receive(h, iq_host, sizeof(float) * 2 * (size_t)h->n, IN_F32, 0, 0, psd_host);
}

int jsdr_fft_receive_i16(jsdr_fft *h, const int16_t *raw_host, int ic, int qc, float *psd_host)
{
    JSDR_REQUIRE(h && raw_host && psd_host, "jsdr_fft_receive_i16: null argument");
    if (!h->pin_lazy_done && !h->pin.p) {
        h->pin.alloc((size_t)h->n * 8 + sizeof(float) * ((size_t)h->n + 2));
        h->pin_lazy_done = true;
    }
    return fft_receive(h, raw_host, sizeof(int16_t) * 2 * (size_t)h->n, IN_I16, ic, qc, psd_host);
}

int jsdr_fft_waterfall_i16(jsdr_fft *h, const int16_t *raw_dev, int64_t nframes, int ic, int qc, int width, uint32_t peak_rgb,
                           uint32_t *pix_dev, float *max_dev, float *peak_dev, void *stream)
{
    return fft_waterfall("jsdr_fft_waterfall_i16", h, raw_dev, IN_I16, nframes, ic, qc, width, peak_rgb, pix_dev, max_dev,
                         peak_dev, as_stream(stream));
}

int jsdr_fft_waterfall_f32(jsdr_fft *h, const float *iq_dev, int64_t nframes, int width, uint32_t peak_rgb, uint32_t *pix_dev,
                           float *max_dev, float *peak_dev, void *stream)
{
    return fft_waterfall("jsdr_fft_waterfall_f32", h, iq_dev, IN_F32, nframes, 0, 0, width, peak_rgb, pix_dev, max_dev, peak_dev,
                         as_stream(stream));
}

const char *jsdr_fft_waterfall_kernel(jsdr_fft *h) { return h ? fft_waterfall_name(h) : ""; }

// ------------------------------------------------------------------ raw[stream][stride]: the strided forms of the four batch calls
// JSDR_FFT_STREAMS_FORCE=1 (A/B knob, tools/ab_fft_streams.py): packed rows take the strided instantiation as well.  Read at
// every call: the tool alternates the two forms within one process.
static bool fft_streams_forced()
{
    const char *e = knob("JSDR_FFT_STREAMS_FORCE");
    return e && atoi(e) != 0;
}

// the arguments the four share; on JSDR_OK `r` is the geometry and *packed says that the rows are one contiguous run
static int fft_streams_args(const char *who, jsdr_fft *h, const void *in_dev, int in_kind, int nstreams, int64_t in_stride,
                            int64_t fps, bool want_psd, const float *psd_dev, int64_t psd_stride, StreamRows &r, bool *packed)
{
    const char *in_name = in_kind == IN_I16 ? "raw_dev" : "iq_dev", *stride_name = in_kind == IN_I16 ? "stream_stride_i16" : "stream_stride_f32";
    JSDR_REQUIRE(h, "%s: null handle", who);
    JSDR_REQUIRE(in_dev, "%s: null %s", who, in_name);
    JSDR_REQUIRE(!want_psd || psd_dev, "%s: null psd_dev", who);
    JSDR_REQUIRE(nstreams > 0, "%s: nstreams=%d must be positive", who, nstreams);
    JSDR_REQUIRE(fps >= 0, "%s: frames_per_stream=%lld is negative", who, (long long)fps);
    const long long n = h->n;
    if (nstreams > 1) {
        JSDR_REQUIRE((in_stride & 1) == 0, "%s: %s=%lld is odd (I and Q alternate)", who, stride_name, (long long)in_stride);
        JSDR_REQUIRE(in_stride >= fps * 2 * n, "%s: %s=%lld is below a stream's %lld frames of %lld values", who, stride_name,
                     (long long)in_stride, (long long)fps, 2 * n);
    }
    JSDR_REQUIRE(!want_psd || psd_stride == 0 || psd_stride >= fps * (n + 2), "%s: psd_stream_stride_f32=%lld is below a stream's %lld rows of %lld floats",
                 who, (long long)psd_stride, (long long)fps, n + 2);
    r.fps = fps;
    r.in_stride = nstreams > 1 ? in_stride / 2 : fps * n;
    r.out_stride = want_psd && psd_stride != 0 ? psd_stride : fps * (n + 2);
    *packed = nstreams == 1 || (r.in_stride == fps * n && r.out_stride == fps * (n + 2));
    return JSDR_OK;
}

static int fft_batch_streams(const char *who, jsdr_fft *h, const void *in_dev, int in_kind, int nstreams, int64_t in_stride,
                             int64_t fps, int ic, int qc, float *psd_dev, int64_t psd_stride, hipStream_t s)
{
    StreamRows r;
    bool packed = false;
    if (fft_streams_args(who, h, in_dev, in_kind, nstreams, in_stride, fps, true, psd_dev, psd_stride, r, &packed) != JSDR_OK) return JSDR_ERR;
    if (fps == 0) return JSDR_OK;
    // rows that are in fact packed are the contiguous call's: the same launch, the same kernel
    if (packed && !fft_streams_forced()) return fft_run(h, in_dev, in_kind, OUT_PSD, nstreams * fps, ic, qc, psd_dev, s);
    return fft_run_streams(h, in_dev, in_kind, r, 0, nstreams * fps, 0, ic, qc, psd_dev, s);
}

static int fft_waterfall_streams(const char *who, jsdr_fft *h, const void *in_dev, int in_kind, int nstreams, int64_t in_stride,
                                 int64_t fps, int ic, int qc, int width, uint32_t peak_rgb, uint32_t *pix_dev, float *max_dev,
                                 float *peak_dev, hipStream_t s)
{
    StreamRows r;
    bool packed = false;
    if (fft_streams_args(who, h, in_dev, in_kind, nstreams, in_stride, fps, false, nullptr, 0, r, &packed) != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(pix_dev, "%s: null pix_dev", who);
    JSDR_REQUIRE(width > 0, "%s: width=%d must be positive", who, width);
    if (fps == 0) return JSDR_OK;
    return fft_waterfall(who, h, in_dev, in_kind, nstreams * fps, ic, qc, width, peak_rgb, pix_dev, max_dev, peak_dev, s,
                         packed && !fft_streams_forced() ? nullptr : &r);
}

int jsdr_fft_batch_streams_i16(jsdr_fft *h, const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16, int64_t frames_per_stream,
                               int ic, int qc, float *psd_dev, int64_t psd_stream_stride_f32, void *stream)
{
    return fft_batch_streams("jsdr_fft_batch_streams_i16", h, raw_dev, IN_I16, nstreams, stream_stride_i16, frames_per_stream, ic, qc,
                             psd_dev, psd_stream_stride_f32, as_stream(stream));
}

int jsdr_fft_batch_streams_f32(jsdr_fft *h, const float *iq_dev, int nstreams, int64_t stream_stride_f32, int64_t frames_per_stream,
                               float *psd_dev, int64_t psd_stream_stride_f32, void *stream)
{
    return fft_batch_streams("jsdr_fft_batch_streams_f32", h, iq_dev, IN_F32, nstreams, stream_stride_f32, frames_per_stream, 0, 0,
                             psd_dev, psd_stream_stride_f32, as_stream(stream));
}

int jsdr_fft_waterfall_streams_i16(jsdr_fft *h, const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16,
                                   int64_t frames_per_stream, int ic, int qc, int width, uint32_t peak_rgb, uint32_t *pix_dev,
                                   float *max_dev, float *peak_dev, void *stream)
{
    return fft_waterfall_streams("jsdr_fft_waterfall_streams_i16", h, raw_dev, IN_I16, nstreams, stream_stride_i16, frames_per_stream,
                                 ic, qc, width, peak_rgb, pix_dev, max_dev, peak_dev, as_stream(stream));
}

int jsdr_fft_waterfall_streams_f32(jsdr_fft *h, const float *iq_dev, int nstreams, int64_t stream_stride_f32,
                                   int64_t frames_per_stream, int width, uint32_t peak_rgb, uint32_t *pix_dev, float *max_dev,
                                   float *peak_dev, void *stream)
{
    return fft_waterfall_streams("jsdr_fft_waterfall_streams_f32", h, iq_dev, IN_F32, nstreams, stream_stride_f32, frames_per_stream,
                                 0, 0, width, peak_rgb, pix_dev, max_dev, peak_dev, as_stream(stream));
}

}  // extern "C"
