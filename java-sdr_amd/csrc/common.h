// common.h -- internal helpers shared by the libjsdr_hip.so translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <string>
#include <type_traits>
#include <utility>
#include "../../include/jsdr_hip.h"

namespace jsdr {

void set_error(const char *fmt, ...);

#define JSDR_HIP_TRY(expr)                                                                         \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            ::jsdr::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,     \
                              __LINE__);                                                           \
            (void)hipGetLastError(); /* reported: the next launch check must not find it again */  \
            return JSDR_ERR;                                                                       \
        }                                                                                          \
    } while (0)

#define JSDR_REQUIRE(cond, ...)                                                                    \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            ::jsdr::set_error(__VA_ARGS__);                                                        \
            return JSDR_ERR;                                                                       \
        }                                                                                          \
    } while (0)

// launch-error check that is safe under stream capture (no sync)
#define JSDR_LAUNCH_CHECK() JSDR_HIP_TRY(hipGetLastError())

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// A kernel whose dynamic LDS exceeds the default needs hipFuncAttributeMaxDynamicSharedMemorySize -- per DEVICE: a process that hosts
// several GPUs (jsdr_group_*, one host thread per device) must set it on each of them, and from whichever thread gets there first.
// Remembers (device, kernel) -> bytes under a mutex and calls hipFuncSetAttribute only when a larger size comes along.
int ensure_dynamic_lds(const void *kernel, size_t bytes);
#define JSDR_LDS_ATTR(kernel, bytes)                                                                       \
    do {                                                                                                   \
        if (::jsdr::ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), (bytes)) != JSDR_OK) return JSDR_ERR; \
    } while (0)

// Tuning and test knobs (JSDR_TAIL8, JSDR_NO_OVERLAP, JSDR_FFT_GRID_ABS, ... : A/B timing in tools/, forcing a kernel in tests/)
// are read through this: the library is DEAF to all of them unless JSDR_KNOBS=1 is set as well, so a stray variable in a
// production environment changes nothing (ADVICE / VERDICT r4: "17 getenv knobs live in the shipped library").  bench.py
// refuses to measure with JSDR_KNOBS set unless it is told so (--allow-knobs, used by tools/ab_*.sh only).
static inline const char *knob(const char *name)
{
    static const bool on = [] {
        const char *e = getenv("JSDR_KNOBS");
        return e && e[0] == '1' && e[1] == 0;
    }();
    return on ? getenv(name) : nullptr;
}

// ---- ownership ------------------------------------------------------------------------------------------------------
// Device memory, pinned memory, streams and events are held by the move-only types below: a handle's members and a
// function's locals give back what they hold when they go, on every way out.  NO object of these types may have static or
// namespace-scope storage (there is none): its destructor would call into HIP while the process exits, after the runtime
// has been torn down.
//
// What they hold at the moment, process-wide (jsdr_live_resources; what a caller got from jsdr_malloc or
// jsdr_stream_create is the caller's and is not counted).
inline std::atomic<int64_t> live_dev_bufs{0}, live_dev_bytes{0}, live_pinned{0}, live_objects{0};

// A HIP object (stream, event) and the call that destroys it.  Converts to the bare handle, so it is passed to HIP as one.
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
    H h = H();
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = H(); }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            reset();
            h = o.h;
            o.h = H();
        }
        return *this;
    }
    ~Owned() { reset(); }
    void adopt(H fresh)
    {
        reset();
        h = fresh;
        if (h) live_objects++;
    }
    void reset()
    {
        if (h) {
            (void)Destroy(h);
            live_objects--;
        }
        h = H();
    }
    operator H() const { return h; }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    int create(unsigned flags)
    {
        hipStream_t s = nullptr;
        JSDR_HIP_TRY(hipStreamCreateWithFlags(&s, flags));
        adopt(s);
        return JSDR_OK;
    }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    int create(unsigned flags = hipEventDefault)  // (hipEventCreate is hipEventCreateWithFlags with hipEventDefault)
    {
        hipEvent_t e = nullptr;
        JSDR_HIP_TRY(hipEventCreateWithFlags(&e, flags));
        adopt(e);
        return JSDR_OK;
    }
};

// A device buffer and its owner: released when it goes, or early with release().
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p, n = o.n;
            o.p = nullptr, o.n = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int alloc(size_t count)
    {
        release();
        if (count == 0) return JSDR_OK;
        JSDR_HIP_TRY(hipMalloc((void **)&p, count * sizeof(T)));
        n = count;
        live_dev_bufs++;
        live_dev_bytes += (int64_t)(n * sizeof(T));
        return JSDR_OK;
    }
    int zero(hipStream_t s = 0)
    {
        if (p) JSDR_HIP_TRY(hipMemsetAsync(p, 0, n * sizeof(T), s));
        return JSDR_OK;
    }
    void release()
    {
        if (p) {
            (void)hipFree(p);
            live_dev_bufs--;
            live_dev_bytes -= (int64_t)(n * sizeof(T));
        }
        p = nullptr;
        n = 0;
    }
};

// A pinned host buffer for the frame-at-a-time receive() forms: a copy from / to pageable memory is staged by the runtime
// and costs a multiple of the transfer (BPSK receive(): 115 -> 71 us per frame with every copy through pinned memory).
// The caller's buffer is memcpy'd in / out on the host; the device copies are asynchronous on `st` and the receive
// synchronises before it returns, so the buffer is free again at the next call.  No pinned memory: falls back to
// the blocking pageable copies.  Owns what it holds, like DevBuf.
template <class T>
struct Pinned {
    T *p = nullptr;
    size_t bytes = 0;
    Pinned() = default;
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
    Pinned(Pinned &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    Pinned &operator=(Pinned &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p, bytes = o.bytes;
            o.p = nullptr, o.bytes = 0;
        }
        return *this;
    }
    ~Pinned() { release(); }
    bool alloc(size_t n)
    {
        release();
        void *q = nullptr;
        if (n && hipHostMalloc(&q, n, hipHostMallocDefault) == hipSuccess) {
            p = static_cast<T *>(q);
            bytes = n;
            live_pinned++;
        } else {
            (void)hipGetLastError();
        }
        return p != nullptr;
    }
    void release()
    {
        if (p) {
            (void)hipHostFree(p);
            live_pinned--;
        }
        p = nullptr;
        bytes = 0;
    }
};
using PinnedStage = Pinned<unsigned char>;

static_assert(!std::is_copy_constructible<DevBuf<int>>::value && std::is_nothrow_move_constructible<DevBuf<int>>::value, "DevBuf is move-only");
static_assert(!std::is_copy_constructible<Stream>::value && std::is_nothrow_move_constructible<Stream>::value, "Stream is move-only");
static_assert(!std::is_copy_constructible<Event>::value && std::is_nothrow_move_constructible<Event>::value, "Event is move-only");
static_assert(!std::is_copy_constructible<PinnedStage>::value && std::is_nothrow_move_constructible<PinnedStage>::value, "PinnedStage is move-only");

// Once a receive() has queued an asynchronous copy from / to its pinned stage, EVERY way out waits for the device: the next
// call memcpy's into the same stage.  Disarmed on the path that has synchronised itself.
struct SyncOnExit {
    bool armed = true;
    ~SyncOnExit()
    {
        if (armed) (void)hipDeviceSynchronize();
    }
};

// ---- int16 -> float, JavaAudio.java:281-288:  (float)s / (float)Short.MAX_VALUE -----------------
// IEEE-correct float division costs ~10 VALU ops (v_div_scale/fmas/fixup).  For the 65536 possible
// dividends and the constant divisor 32767 the quotient is q = fma(a, rh, a*rl) with rh = RN(1/d) and
// rl = RN(1/d - rh): rh+rl carries 1/d to 2^-48 and no a/32767 lies that close to a rounding boundary.
// Checked for every input in exact rational arithmetic and on the GPU against the CPU's
// division (tests/test_gpu_fft.py, all 65536 inputs).
// (k_fm and k_fft's int16 path convert with i16_to_float_java_2p15 below, one instruction instead of two; every other
//  caller uses this form.)
__device__ __forceinline__ float i16_to_float_java(int s)
{
    const float rh = 0x1.0002p-15f;
    const float rl = 0x1.0002p-45f;
    const float a = (float)s;
    return __builtin_fmaf(a, rh, a * rl);
}

// 2^15 * i16_to_float_java(s), EXACTLY, in one fused multiply-add: RN(a + a*c) with c = RN(1/32767) = 0x1.0002p-15f is
// 32768 * RN(a / 32767) for every int16 a (a * (1 + c) carries 32768/32767 to 2^-46 relative, and no quotient lies that
// close to a rounding boundary; one ulp more in c fails for four inputs).  Proved for all 65536 inputs in exact rational
// arithmetic by tests/test_i16_scaled_convert.py.  A caller carries the factor 2^15 -- an exact scaling, which commutes
// with every rounded multiply, add and fma as long as nothing overflows or goes subnormal -- through its linear
// arithmetic and takes it out in a constant that is multiplied in anyway (k_fm: HOWARD; k_fft: the second pass's
// twiddles).
constexpr float I16_2P15_UNSCALE = 0x1p-15f;
__device__ __forceinline__ float i16_to_float_java_2p15(int s)
{
    const float a = (float)s;
    return __builtin_fmaf(a, 0x1.0002p-15f, a);
}

// `short s = getShort(); s += (short)corr;` -- 16-bit wrap-around add
__device__ __forceinline__ int java_short_add(int s, int corr)
{
    return (int)(short)(s + (int)(short)corr);
}

// int16 pair -> (double)((float)s / 32767f) for I and Q (JavaAudio.java:281-288, FUNcubeBPSKDemod.java:372-373)
// amax (optional): running maximum of |s| over the samples converted, as a float (the fast variant scales its error
// bound with the stream's actual input amplitude)
__device__ __forceinline__ void fm_convert(int w, int ic, int qc, bool dc, double &di, double &dq, float *amax = nullptr)
{
    int si = (int)(short)(w & 0xffff), sq = w >> 16;
    if (dc) {
        si = java_short_add(si, ic);
        sq = java_short_add(sq, qc);
    }
    // (float)s / 32767f for I and Q at once: q = fma(a, rh, a * rl) (common.h) on the native two-float vector --
    // v_pk_mul_f32 + v_pk_fma_f32 round each half exactly as the scalar instructions do
    typedef float v2f __attribute__((ext_vector_type(2)));
    const v2f a = {(float)si, (float)sq};
    if (amax) *amax = fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), *amax);  // v_max3_f32 with |.| modifiers: one instruction
    const v2f rh = {0x1.0002p-15f, 0x1.0002p-15f}, rl = {0x1.0002p-45f, 0x1.0002p-45f};
    const v2f q = __builtin_elementwise_fma(a, rh, a * rl);
    di = (double)q.x;
    dq = (double)q.y;
}

// fm_convert with the quotients SCALED by 2^15 (i16_to_float_java_2p15: one v_pk_fma_f32, no v_pk_mul_f32): di, dq are
// exactly 32768 times what fm_convert gives; amax is taken from (float)s and is the same.
__device__ __forceinline__ void fm_convert_2p15(int w, int ic, int qc, bool dc, double &di, double &dq, float *amax = nullptr)
{
    int si = (int)(short)(w & 0xffff), sq = w >> 16;
    if (dc) {
        si = java_short_add(si, ic);
        sq = java_short_add(sq, qc);
    }
    typedef float v2f __attribute__((ext_vector_type(2)));
    const v2f a = {(float)si, (float)sq};
    if (amax) *amax = fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), *amax);
    const v2f c = {0x1.0002p-15f, 0x1.0002p-15f};
    const v2f q = __builtin_elementwise_fma(a, c, a);
    di = (double)q.x;
    dq = (double)q.y;
}

}  // namespace jsdr
