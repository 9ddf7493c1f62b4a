// demod_dev.h -- the device side of one tile of the demod.java chain, shared by demod.hip (k_demod_front, k_demod_fused,
// k_demod_state) and demod_scope.hip (k_demod_scope_front): the call's arguments, the sample fetch, filter() + mixer at one
// sample, and the tile itself.  Units that include it are compiled with -ffp-contract=off.
#pragma once
#include "common.h"
#include "demod.h"

namespace jsdr {

struct DemodConst {
    float w[21];
    float fmgain;
    int mode, dofir, dodwn, doagc;
};

struct DemodArgs {
    const int *raw;        // int16 pairs [S][stride]
    const float2 *rawf;    // or float pairs
    long long stride_pairs;
    long long L;           // samples per stream in this call
    int n;                 // samples per frame
    int nfr;               // frames per stream in this call
    int ic, qc;
    const float2 *hist;    // [S][21] filter input before the call
    const float2 *lilq;    // [S] FM detector state before the call
    const float2 *nco;     // [L] (cos, sin) of the carrier phase per sample (dodwn)
    float *d;              // [S][L] demodulated value per sample (sam[s] after :441-462)
    unsigned *fmax_bits;   // [S][nfr] bit pattern of max |d| (zeroed before launch)
    DemodConst c;
};

template <bool F32IN>
__device__ __forceinline__ float2 demod_in(const DemodArgs &a, const int *raw, const float2 *rawf, const float2 *hist,
                                           long long g)
{
    if (g < 0) return hist[DHALO + g];
    if (F32IN) return rawf[g];
    const int w = raw[g];
    return make_float2(i16_to_float_java(java_short_add((int)(short)(w & 0xffff), a.ic)),
                       i16_to_float_java(java_short_add(w >> 16, a.qc)));
}

// filter() (:378-396) + mixer (:423-434) at ONE sample whose window sits in xs[first .. first+20] (newest last);
// used for the sample just before a tile and for the state kernel
template <class IDX>
__device__ __forceinline__ float2 demod_mixed_at(const DemodConst &c, const float2 *xs, IDX idx, int newest, const float2 *nco,
                                                 long long g)
{
    float2 v = xs[idx(newest)];
    if (c.dofir) {
        float oi = 0.0f, oq = 0.0f;
#pragma unroll
        for (int k = 0; k < 21; k++) {  // ring order: the newest sample meets w[0]
            const float2 x = xs[idx(newest - k)];
            oi = oi + x.x * c.w[k];
            oq = oq + x.y * c.w[k];
        }
        v = make_float2(oi, oq);
    }
    if (c.dodwn) {
        const float2 cs = nco[g];
        v = make_float2(v.x * cs.x - v.y * cs.y, v.x * cs.y + v.y * cs.x);
    }
    return v;
}

// the sample just before the tile: xs[xpad8(20)] is x(g0 - 1)
__device__ __forceinline__ float2 demod_mixed(const DemodConst &c, const float2 *xs, const float2 *nco, long long g)
{
    return demod_mixed_at(c, xs, [](int i) { return xpad8(i); }, DHALO - 1, nco, g);
}

// One tile = 2048 samples of one frame of one stream; every thread owns 8 CONSECUTIVE samples: their 21-tap
// windows overlap, so 28 LDS reads feed 8 outputs (3.5 per sample instead of 21), and I/Q ride in one packed
// register pair: acc = acc + x*w is v_pk_mul_f32 + v_pk_add_f32, each half rounded separately exactly like the
// reference's two scalar statements (:388-389).
constexpr int DXS = DTILE + DHALO + (DTILE + DHALO) / 8 + 1;

// tile j of frame f of stream s -> this thread's 8 detected samples dv[] (sam[s] after :441-462) and the running
// maximum of their magnitudes; xs / last are the workgroup's LDS (two barriers inside, none after).
// KEEP: the 8 filtered + mixed samples themselves (what :436-437 save into dbg[]) go to mixed[] as well.
template <bool F32IN, bool CHAINED, bool KEEP = false>
__device__ __forceinline__ void demod_tile(const DemodArgs &a, const int s, const int f, const int j, float2 *xs, float2 *last,
                                           float (&dv)[DPER], unsigned &mbits, v2f *mixed = nullptr)
{
    constexpr int PER = DPER;
    const int tid = threadIdx.x;
    const long long g0 = (long long)f * a.n + (long long)j * DTILE;
    const int len = (a.n - j * DTILE) < DTILE ? (a.n - j * DTILE) : DTILE;
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const float2 *rawf = a.rawf + (long long)s * a.stride_pairs;
    const float2 *hist = a.hist + (long long)s * DHALO;
    // FM detector across tiles of one workgroup: the previous tile's last sample, read before the staging barrier
    // below lets anyone overwrite it
    float2 carried = make_float2(0.0f, 0.0f);
    if (CHAINED && tid == 0) carried = last[255];
    // xs[xpad8(i)] = x(g0 - 21 + i); beyond the tile's end: zeros (their outputs are never stored)
    if (g0 >= DHALO) {
        // every tile but the call's first: all nine loads of a thread are in flight before the first conversion /
        // LDS store (as a plain loop the compiler waits for each load in turn: nine memory latencies per tile)
        // addressing: one uniform base per tile and a 32-bit offset per load, clamped inside the call (values
        // beyond the tile's end are dropped below)
        constexpr int NLD = (DTILE + DHALO + 255) / 256;
        const long long room = a.L - 1 - (g0 - DHALO);
        const unsigned relmax = (unsigned)(room < (long long)(DTILE + DHALO - 1) ? room : (long long)(DTILE + DHALO - 1));
        const int *rb = raw + (g0 - DHALO);
        const float2 *rbf = rawf + (g0 - DHALO);
        int w[NLD];
        float2 wf[NLD];
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            unsigned rel = (unsigned)(tid + 256 * q);
            rel = rel < relmax ? rel : relmax;
            if (F32IN)
                wf[q] = rbf[rel];
            else
                w[q] = rb[rel];
        }
        const bool full = len == DTILE;  // every tile of a frame but a ragged last one
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            const int i = tid + 256 * q;
            float2 v;
            if (F32IN)
                v = wf[q];
            else
                v = make_float2(i16_to_float_java(java_short_add((int)(short)(w[q] & 0xffff), a.ic)),
                                i16_to_float_java(java_short_add(w[q] >> 16, a.qc)));
            // xpad8(tid + 256 q) = xpad8(tid) + 288 q: one address register, constant offsets
            float2 *slot = xs + (tid + (tid >> 3)) + 288 * q;
            if (full) {
                if (q < NLD - 1 || i < DTILE + DHALO) *slot = v;
            } else if (i < DTILE + DHALO) {
                *slot = (i < len + DHALO) ? v : make_float2(0.0f, 0.0f);
            }
        }
    } else {
        for (int i = tid; i < DTILE + DHALO; i += 256)
            xs[xpad8(i)] = (i < len + DHALO) ? demod_in<F32IN>(a, raw, rawf, hist, g0 - DHALO + i) : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    const int t0 = tid * PER;  // first sample of this thread within the tile
    v2f m[PER];                // filtered + mixed samples
    if (a.c.dofir) {
        v2f x[PER + 20];  // x[q] = input sample t0 - 20 + q
#pragma unroll
        for (int q = 0; q < PER + 20; q++) {
            // xpad8(8 tid + c) = 9 tid + c + (c >> 3)
            const float2 v = xs[9 * tid + (1 + q) + ((1 + q) >> 3)];
            x[q] = (v2f){v.x, v.y};
        }
#pragma unroll
        for (int u = 0; u < PER; u++) {
            v2f acc = (v2f){0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 21; k++) acc = acc + x[u + 20 - k] * a.c.w[k];  // ring order: newest sample meets w[0]
            m[u] = acc;
        }
    } else {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const float2 v = xs[9 * tid + (DHALO + u) + ((DHALO + u) >> 3)];
            m[u] = (v2f){v.x, v.y};
        }
    }
    if (a.c.dodwn) {  // :423-434
        const float2 *nc = a.nco + g0 + t0;
        float2 cs[PER];
        if (((g0 + t0) & 1) == 0) {  // 16-byte aligned pairs (always, unless the frame length is odd)
#pragma unroll
            for (int u = 0; u < PER; u += 2) {
                // (an odd tile end reads one entry past its last sample: inside the table, which has spare slots)
                const float4 c2 = (t0 + u < len) ? reinterpret_cast<const float4 *>(nc)[u / 2] : make_float4(1.0f, 0.0f, 1.0f, 0.0f);
                cs[u] = make_float2(c2.x, c2.y);
                cs[u + 1] = make_float2(c2.z, c2.w);
            }
        } else {
#pragma unroll
            for (int u = 0; u < PER; u++) cs[u] = (t0 + u < len) ? nc[u] : make_float2(1.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < PER; u++) {
            // (x*c - y*s, x*s + y*c) as x*(c, s) + (-y, y)*(s, c): two packed products and one packed sum (x - y == x + (-y) exactly)
            const v2f v = m[u];
            const v2f c = (v2f){cs[u].x, cs[u].y};
            const v2f ny = (v2f){-v.y, v.y};
            m[u] = __builtin_shufflevector(v, v, 0, 0) * c + ny * __builtin_shufflevector(c, c, 1, 0);
        }
    }
    if (KEEP) {
#pragma unroll
        for (int u = 0; u < PER; u++) mixed[u] = m[u];
    }
    // the FM detector's previous sample: the neighbour thread's last one; thread 0 recomputes it from the halo,
    // or takes the carried state at the first sample of the call
    float2 prev = make_float2(0.0f, 0.0f);
    if (a.c.mode == MODE_NFM || a.c.mode == MODE_WFM) {
        last[tid] = make_float2(m[PER - 1].x, m[PER - 1].y);
        __syncthreads();
        if (tid > 0)
            prev = last[tid - 1];
        else if (CHAINED)
            prev = carried;
        else if (g0 > 0)
            prev = demod_mixed(a.c, xs, a.nco, g0 - 1);
        else
            prev = a.lilq[s];
    }
    // max |d| travels as a bit pattern: non-negative floats order like unsigned ints, and any NaN beats every
    // number -- Math.max's NaN propagation (:463) for free
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const v2f mm = m[u];
        if (a.c.mode == MODE_OFF) {
            dv[u] = 0.0f;
        } else if (a.c.mode == MODE_RAW) {
            dv[u] = mm.x;
        } else if (a.c.mode == MODE_AM) {
            // :449 (float)Math.sqrt((double)..): the correctly rounded double root of a float, rounded to float, IS the
            // correctly rounded float root (53 >= 2*24 + 2 bits), which is what sqrtf compiles to here (v_sqrt_f32
            // plus a one-ulp fix-up; __fsqrt_rn is NOT correctly rounded) -- all FP32, no v_rsq_f64 chain
            dv[u] = __builtin_sqrtf(mm.x * mm.x + mm.y * mm.y);
        } else {
            dv[u] = ((prev.x * mm.y) - (prev.y * mm.x)) * a.c.fmgain;
            prev = make_float2(mm.x, mm.y);
        }
        if (t0 + u < len) {
            const unsigned bb = __float_as_uint(dv[u]) & 0x7fffffffu;
            mbits = bb > mbits ? bb : mbits;
        }
    }
}

}  // namespace jsdr
