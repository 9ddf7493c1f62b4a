// fft_common.h -- device helpers shared by the power-of-two (fft_psd.hip) and mixed-radix (fft_mixed.hip)
// spectrum kernels: compile-time twiddles, in-register radix-2^k DFT, LDS padding.
#pragma once
#include "common.h"
#include <type_traits>
#include <utility>
#include <vector>

namespace jsdr {

// ------------------------------------------------------------------ compile-time twiddles
constexpr double cx_pi = 3.14159265358979323846264338327950288;

constexpr double cx_sin_small(double x)  // |x| <= pi/4
{
    double x2 = x * x, term = x, sum = x;
    for (int i = 1; i < 12; i++) {
        term *= -x2 / ((2 * i) * (2 * i + 1));
        sum += term;
    }
    return sum;
}
constexpr double cx_cos_small(double x)
{
    double x2 = x * x, term = 1.0, sum = 1.0;
    for (int i = 1; i < 12; i++) {
        term *= -x2 / ((2 * i - 1) * (2 * i));
        sum += term;
    }
    return sum;
}
// cos/sin of 2*pi*j/len for 0 <= j < len, exact symmetries first
constexpr double cx_cos_turn(int j, int len)
{
    j %= len;
    if (8 * j <= len) return cx_cos_small(2 * cx_pi * j / len);
    if (8 * j <= 3 * len) return -cx_sin_small(2 * cx_pi * (j - 0.25 * len) / len);
    if (8 * j <= 5 * len) return -cx_cos_small(2 * cx_pi * (j - 0.5 * len) / len);
    if (8 * j <= 7 * len) return cx_sin_small(2 * cx_pi * (j - 0.75 * len) / len);
    return cx_cos_small(2 * cx_pi * (j - len) / len);
}
constexpr double cx_sin_turn(int j, int len) { return cx_cos_turn(4 * j + 3 * len, 4 * len); }

// Complex arithmetic on the native two-float vector type: the IR then holds <2 x float> operations from the
// start, i.e. v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32.  Two rules keep register shuffles out (measured on
// the ISA): a half swap must be a shufflevector (it folds into op_sel), and a sign on ONE half must sit in a
// constant pair such as (1,-1) (a whole-vector negation folds into neg_lo/neg_hi, a partial one becomes
// v_xor + v_mov).
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f to_v(float2 a) { return (v2f){a.x, a.y}; }
__device__ __forceinline__ float2 from_v(v2f v) { return make_float2(v.x, v.y); }
__device__ __forceinline__ v2f vswap(v2f v) { return __builtin_shufflevector(v, v, 1, 0); }
__device__ __forceinline__ v2f vfma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return from_v(to_v(a) + to_v(b)); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return from_v(to_v(a) - to_v(b)); }
// a * w with w' = (-w.y, w.x) supplied: (a.x w.x - a.y w.y, a.x w.y + a.y w.x) = a.x * w + a.y * w'
__device__ __forceinline__ float2 cmul2(float2 a, float2 w, float2 wq)
{
    const v2f va = to_v(a);
    return from_v(vfma(__builtin_shufflevector(va, va, 1, 1), to_v(wq), __builtin_shufflevector(va, va, 0, 0) * to_v(w)));
}
// w' = (-w.y, w.x) = swap(w) * (-1, 1)
__device__ __forceinline__ float2 cquad(float2 w) { return from_v(vswap(to_v(w)) * (v2f){-1.0f, 1.0f}); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return cmul2(a, w, cquad(w)); }

// d * exp(-2 pi i J/LEN) with the trivial cases folded
template <int LEN, int J>
__device__ __forceinline__ float2 mul_w(float2 d)
{
    const v2f vd = to_v(d);
    if constexpr (J == 0) {
        return d;
    } else if constexpr (4 * J == LEN) {  // (d.y, -d.x)
        return from_v(vswap(vd) * (v2f){1.0f, -1.0f});
    } else if constexpr (8 * J == LEN) {  // ((d.x + d.y) c, (d.y - d.x) c)
        constexpr float c = (float)0.70710678118654752440;
        return from_v(vfma(vswap(vd), (v2f){c, -c}, vd * c));
    } else if constexpr (8 * J == 3 * LEN) {  // ((d.y - d.x) c, -(d.x + d.y) c)
        constexpr float c = (float)0.70710678118654752440;
        return from_v(vfma(vswap(vd), (v2f){c, -c}, vd * -c));
    } else {  // (d.x c + d.y s, d.y c - d.x s)
        constexpr float c = (float)cx_cos_turn(J, LEN);
        constexpr float s = (float)cx_sin_turn(J, LEN);
        return from_v(vfma(vswap(vd), (v2f){s, -s}, vd * c));
    }
}

template <int LEN, int BASE, int J>
__device__ __forceinline__ void bfly(float2 *x)
{
    constexpr int H = LEN / 2;
    float2 a = x[BASE + J], b = x[BASE + J + H];
    x[BASE + J] = cadd(a, b);
    x[BASE + J + H] = mul_w<LEN, J>(csub(a, b));
}
template <int LEN, int BASE, int... Js>
__device__ __forceinline__ void bfly_group(float2 *x, std::integer_sequence<int, Js...>)
{
    (bfly<LEN, BASE, Js>(x), ...);
}
template <int R, int LEN, int... Bs>
__device__ __forceinline__ void bfly_stage(float2 *x, std::integer_sequence<int, Bs...>)
{
    (bfly_group<LEN, Bs * LEN>(x, std::make_integer_sequence<int, LEN / 2>{}), ...);
}
// in-register radix-R DFT, decimation in frequency: natural order in, BIT-REVERSED order out
template <int R, int LEN = R>
__device__ __forceinline__ void dft_reg(float2 *x)
{
    if constexpr (LEN >= 2) {
        bfly_stage<R, LEN>(x, std::make_integer_sequence<int, R / LEN>{});
        dft_reg<R, LEN / 2>(x);
    }
}
constexpr int cx_bitrev(int v, int r)
{
    int o = 0;
    for (int b = 1; b < r; b <<= 1) {
        o = (o << 1) | (v & 1);
        v >>= 1;
    }
    return o;
}

__device__ __forceinline__ int lds_pad(int idx) { return idx + (idx >> 4); }
constexpr int lds_frame_elems(int n) { return n + (n >> 4) + 1; }


enum { IN_I16 = 0, IN_F32 = 1 };
enum { OUT_PSD = 0, OUT_SPEC = 1, OUT_PIX = 2 };  // OUT_PIX: waterfall pixel rows, the power-of-two kernel only (fft_psd.hip)

struct FftArgs {
    const void *in;      // int16 pairs or float pairs, [nframes][n]
    float *out;          // psd [nframes][n+2] or spectrum [nframes][2n]
    const float2 *tw;    // per-pass twiddle tables, concatenated
    long long nframes;
    int rate;
    int ic, qc;
    int split = 0;  // 1: frame f of the kernel is the even (f&1 == 0) / odd half of input frame f>>1 (2N samples)
#ifdef JSDR_X_WGCLK
    int wgclk_slot = 0;  // timing probe (fft_psd.hip): the launch's row of the per-workgroup start / end ticks
#endif
};

// ------------------------------------------------------------------ strided batches (jsdr_fft_batch_streams_* / jsdr_fft_waterfall_streams_*)
// The launch's frame k is frame j of stream s with (s, j) = ((f0 + k) / fps, (f0 + k) % fps); it is read at point
// s * in_stride + j * n of the input and its PSD row is written at float out_base + s * out_stride + j * (n + 2).  A workgroup
// divides ONCE, for the first frame it takes; from there it walks: a persistent workgroup's next frame is `step` frames on
// (the grid is known to the host, which states the step as offsets), and a walk that leaves its stream adds the gap.  What a
// frame costs is four 64-bit additions and a compare -- scalar ones where the frame is the same in every lane of a wave.
struct StreamGeom {
    long long fps;                 // frames per stream
    long long f0;                  // the launch's frame 0 in the call's numbering (the waterfall fallback goes in chunks)
    long long in_stride;           // points between the first frames of two streams
    long long out_stride;          // floats between the first PSD rows of two streams
    long long out_base;            // of the launch's output pointer (a chunk's rows are packed from its own frame 0: -f0 * (n + 2))
    long long step_j;              // the step as (streams, frames): its frames ...
    long long step_in, step_out;   // ... and what it adds to the two offsets while the walk stays inside fps
    long long wrap_in, wrap_out;   // added as well when j passes fps: stride - fps * row
    long long last_in, last_out;   // the launch's last frame (k_fft's surplus part-workgroup redoes it)
    int n;                         // points a frame (k_fft_mixed_dual's template N is half of it)
};
template <class BASE>
struct Strided : BASE {
    StreamGeom g;
};
template <class ARGS>
struct is_strided : std::false_type {};
template <class B>
struct is_strided<Strided<B>> : std::true_type {};
// host: the geometry of frames [f0, f0 + nf) of a call; strides in points / floats.  The step waits for the grid.
inline StreamGeom stream_geom(int n, long long fps, long long in_stride, long long out_stride, long long f0, long long nf, long long out_base)
{
    StreamGeom g = {};
    g.fps = fps;
    g.f0 = f0;
    g.in_stride = in_stride;
    g.out_stride = out_stride;
    g.out_base = out_base;
    g.wrap_in = in_stride - fps * n;
    g.wrap_out = out_stride - fps * (n + 2);
    const long long s = (f0 + nf - 1) / fps, j = (f0 + nf - 1) % fps;
    g.last_in = s * in_stride + j * n;
    g.last_out = out_base + s * out_stride + j * (n + 2);
    g.n = n;
    return g;
}
inline void stream_geom_step(StreamGeom &g, long long step)
{
    const long long ss = step / g.fps;
    g.step_j = step % g.fps;
    g.step_in = ss * g.in_stride + g.step_j * g.n;
    g.step_out = ss * g.out_stride + g.step_j * (g.n + 2);
}
struct FramePos {
    long long f;        // the launch's frame number: the loop bound, and the row of the packed waterfall outputs
    long long j;        // frame within its stream
    long long in, out;  // offsets, as above
};
__device__ __forceinline__ FramePos stream_pos(const StreamGeom &g, long long f)
{
    FramePos p;
    const unsigned long long G = (unsigned long long)(g.f0 + f), s = G / (unsigned long long)g.fps;
    p.f = f;
    p.j = (long long)(G - s * (unsigned long long)g.fps);
    p.in = (long long)s * g.in_stride + p.j * g.n;
    p.out = g.out_base + (long long)s * g.out_stride + p.j * (g.n + 2);
    return p;
}
__device__ __forceinline__ void stream_step(const StreamGeom &g, FramePos &p, long long step)
{
    p.f += step;
    p.j += g.step_j;
    p.in += g.step_in;
    p.out += g.step_out;
    if (p.j >= g.fps) {
        p.j -= g.fps;
        p.in += g.wrap_in;
        p.out += g.wrap_out;
    }
}

// A kernel's frame is a number (contiguous batches: frame f lies at f * row) or a FramePos (strided ones); the kernels state
// their frame loop and their addresses through these, and each instantiation gets its own form at compile time.
__device__ __forceinline__ long long frame_first(const FftArgs &, long long f) { return f; }
__device__ __forceinline__ bool frame_more(const FftArgs &a, long long f) { return f < a.nframes; }
__device__ __forceinline__ void frame_next(const FftArgs &, long long &f, long long step) { f += step; }
template <class B>
__device__ __forceinline__ FramePos frame_first(const Strided<B> &a, long long f) { return stream_pos(a.g, f); }
template <class B>
__device__ __forceinline__ bool frame_more(const Strided<B> &a, const FramePos &p) { return p.f < a.nframes; }
template <class B>
__device__ __forceinline__ void frame_next(const Strided<B> &a, FramePos &p, long long step) { stream_step(a.g, p, step); }
__device__ __forceinline__ long long frame_in(long long f, int n) { return f * n; }               // points
__device__ __forceinline__ long long frame_in(const FramePos &p, int) { return p.in; }
__device__ __forceinline__ long long frame_out(long long f, int row) { return f * row; }          // floats (float2 of a spectrum)
__device__ __forceinline__ long long frame_out(const FramePos &p, int) { return p.out; }
__device__ __forceinline__ long long frame_row(long long f) { return f; }                         // row of a packed output
__device__ __forceinline__ long long frame_row(const FramePos &p) { return p.f; }

struct Best {
    float v;
    int k;
};

// A frame of T threads with T a multiple of 64 is whole waves: its slot in the workgroup, its number, the clamp of a surplus
// part-workgroup, the next frame and every row base made from them are the same in all 64 lanes.  The compiler cannot see that
// through threadIdx.x / T; the slot is said to be a scalar (v_readfirstlane) and the rest follows in scalar registers.
constexpr bool frame_is_waves(int T) { return T % 64 == 0; }

// A row of global memory whose base is the same in every lane of a wave, addressed as scalar base + unsigned 32-bit lane
// offset + constant: a buffer resource (the base and the row's size in four scalar registers), the lane's byte offset in ONE
// vector register that never changes, the constant in a scalar register.  No 64-bit address is built per frame or per access.
// (Stated as `base + zext(offset)` on a plain pointer the compiler hoists the zero-extension and the lane's part of the sum
// out of the frame loop, and inside the loop builds base + 64-bit vector offset again -- the global saddr form is matched
// only where the zero-extension stands in the block of the access.)  The resource carries the row's size: an access outside
// [0, bytes) reads zero or is dropped by the hardware.
using WaveRow = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ WaveRow wave_row(const void *base, unsigned bytes)
{
    // (word 3: 32-bit untyped data, the raw-buffer setting of the gfx9 family; stride 0, so the range check is in bytes)
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}
template <class V>
__device__ __forceinline__ V wave_row_load(WaveRow row, unsigned lane_bytes, unsigned const_bytes)
{
    static_assert(sizeof(V) == 4 || sizeof(V) == 8, "one or two dwords a lane");
    if constexpr (sizeof(V) == 4) return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b32(row, lane_bytes, const_bytes, 0));
    else return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(row, lane_bytes, const_bytes, 0));
}
template <class V>
__device__ __forceinline__ void wave_row_store(WaveRow row, unsigned lane_bytes, unsigned const_bytes, V v)
{
    static_assert(sizeof(V) == 4 || sizeof(V) == 8, "one or two dwords a lane");
    if constexpr (sizeof(V) == 4)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), row, lane_bytes, const_bytes, 0);
    else
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b64(row, 0, 0, 0)), v), row,
                                              lane_bytes, const_bytes, 0);
}

// ------------------------------------------------------------------ first maximum over the 64 lanes of a wave, no LDS
// Inside a row of 16 lanes four DPP steps whose partners are an involution each (the quad's neighbour, the quad's other pair,
// the mirrored half row, the mirrored row) leave the row's result in all 16 lanes; the four rows are read as scalars
// (v_readlane) and combined, so the result is the same in every lane.
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int x)
{
    // (every lane has a partner under these four controls: bound_ctrl and `old` decide nothing, and in this form the move folds
    //  into the v_max_i32 / v_min_i32 that uses it)
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true);
}
constexpr int DPP_QUAD_1032 = 0xB1, DPP_QUAD_2301 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;
template <bool MAX, int CTRL>
__device__ __forceinline__ int pick_dpp(int x)
{
    const int o = dpp_i32<CTRL>(x);
    return MAX ? (o > x ? o : x) : (o < x ? o : x);
}
template <bool MAX>
__device__ __forceinline__ int wave_reduce_i32(int x)
{
    x = pick_dpp<MAX, DPP_QUAD_1032>(x);
    x = pick_dpp<MAX, DPP_QUAD_2301>(x);
    x = pick_dpp<MAX, DPP_ROW_HALF_MIRROR>(x);
    x = pick_dpp<MAX, DPP_ROW_MIRROR>(x);
    const int r0 = __builtin_amdgcn_readlane(x, 0), r1 = __builtin_amdgcn_readlane(x, 16);
    const int r2 = __builtin_amdgcn_readlane(x, 32), r3 = __builtin_amdgcn_readlane(x, 48);
    const int a = MAX ? (r0 > r1 ? r0 : r1) : (r0 < r1 ? r0 : r1), b = MAX ? (r2 > r3 ? r2 : r3) : (r2 < r3 ? r2 : r3);
    return MAX ? (a > b ? a : b) : (a < b ? a : b);
}
// The bits of a float that is not a NaN as a signed integer that orders as the float does (negative floats run backwards as
// integers: their magnitude bits are flipped); its own inverse.  +0 and -0, equal as floats, get the keys 0 and -1.
__device__ __forceinline__ int f32_order_key(int bits) { return bits ^ (int)((unsigned)(bits >> 31) >> 1); }

// mixed-radix path (fft_mixed.hip): n = 4800, 9600 -- java-sdr's default 48 kHz / 96 kHz frames
struct MixedPlan {
    int n = 0, nrad = 0, radix[6] = {1, 1, 1, 1, 1, 1};
    int threads = 0;
    size_t lds_bytes = 0;
    int tw_count = 0;
    // n = 2*half (19200 = 2*9600): two half-size transforms of the even / odd samples + one radix-2 combine pass
    bool split2 = false;
    int half_tw_count = 0;  // the half plan's tables come first; `half` combine twiddles follow
};
bool mixed_plan(int n, MixedPlan &p);
void mixed_twiddles(const MixedPlan &p, float2 *out);
int mixed_launch(const MixedPlan &p, const FftArgs &a, int in_kind, int out_kind, int grid, hipStream_t st);
// split2 plans: half-size spectra of `nframes` frames into tmp [2*nframes][n/2], then the combine pass
int mixed_launch_split2(const MixedPlan &p, const FftArgs &a, int in_kind, int out_kind, int num_cu, hipStream_t st);

// any other composite n up to 9800 (fft_rt.hip): Stockham passes with a run-time radix plan (2^a 3^b 5^c 7^d in registers,
// a larger prime factor as a pass of that radix by the DFT's definition)
bool rt_supported(int n);
void rt_twiddles(int n, std::vector<float2> &w);
int rt_launch(const FftArgs &a, int n, int in_kind, int out_kind, int num_cu, hipStream_t st);

// what is left -- prime frame sizes, frames above 9800 samples (fft_any.hip): the DFT itself, double accumulation
bool dft_any_supported(int n);
int dft_any_launch(const FftArgs &a, int n, int in_kind, int out_kind, int num_cu, hipStream_t st);

// the strided forms of the four (PSD rows only): the same kernels' strided instantiations on the same grids
int mixed_launch_streams(const MixedPlan &p, const Strided<FftArgs> &a, int in_kind, int grid, hipStream_t st);
int mixed_launch_split2_streams(const MixedPlan &p, const Strided<FftArgs> &a, int in_kind, int num_cu, hipStream_t st);
int rt_launch_streams(const Strided<FftArgs> &a, int n, int in_kind, int num_cu, hipStream_t st);
int dft_any_launch_streams(const Strided<FftArgs> &a, int n, int in_kind, int num_cu, hipStream_t st);

}  // namespace jsdr
