// demod_chan.hip -- the demod.java chain (demod.hip) for channel handles (jsdr_demod_create_channels): ninputs x K
// independently tuned receivers, channel c of input i is stream i * K + c.  Compiled with -ffp-contract=off like
// demod.hip: every product and sum below is the one demod.hip's kernels (and the reference) compute, in their order.
//
// k_demod_chan: one workgroup = one frame (at most 5 tiles) of ONE input, inputs fastest in the grid (the K carrier rows of a
// frame, 16 KB each, are then read from L2 by every input's workgroup; frames fastest re-read them from memory per input).  The frame's samples and the 21 before it are
// read from memory once, DC-corrected and converted once, and parked in LDS in demod_tile's padded image.  At the call's
// first frames (those that start fewer than 21 samples into the call) the samples before the call are each channel's own
// history (hist[i*K + c]): all K of them are staged with the frame and copied into the halo slots before that channel runs.  Then the workgroup walks the channels, uniformly, so
// mode and switch branches are scalar: per channel and tile the blocked 21-tap filter, the channel's carrier row, the
// detector (the FM previous sample from the neighbour lane, or recomputed from the image), the frame maximum, AGC and
// the int16 stores.  AM channels (their running mean needs the whole frame first) write floats and the frame maximum to
// d and finish in k_demod_mean + k_demod_chan_out.
// k_demod_chan_front: frames of more than 5 tiles, one workgroup per tile of one input, every channel to d.
#include "common.h"
#include "demod.h"

namespace jsdr {

// filter() (:378-396) + mixer (:423-434) at ONE sample whose window sits in xs[idx(newest - 20) .. idx(newest)]
template <class IDX>
__device__ __forceinline__ float2 chan_mixed_at(const DemodChanConst &c, const float2 *xs, IDX idx, int newest, const float2 *nco,
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

template <bool F32IN>
__device__ __forceinline__ float2 chan_convert(const DemodChanArgs &a, int w, float2 wf)
{
    if (F32IN) return wf;
    return make_float2(i16_to_float_java(java_short_add((int)(short)(w & 0xffff), a.ic)),
                       i16_to_float_java(java_short_add(w >> 16, a.qc)));
}

// xs[xpad8(e)] = x(w0 + e) for e < NE: samples up to nwin (exclusive), zeros beyond; e with w0 + e < 0 (the call's first
// window) are left for the channel halos.  hh[c * 21 + k] = hist[(in * K + c) * 21 + k] when w0 < 0.
template <bool F32IN, int NE>
__device__ __forceinline__ void chan_stage(const DemodChanArgs &a, int in, long long w0, int nwin, float2 *xs, float2 *hh)
{
    const int tid = threadIdx.x;
    const int *rb = a.raw + (long long)in * a.stride_pairs + w0;
    const float2 *rbf = a.rawf + (long long)in * a.stride_pairs + w0;
    const int elo = w0 < 0 ? (int)-w0 : 0;
    constexpr int NLD = (NE + 255) / 256;
    constexpr int CH = 9;  // loads in flight per thread before the first conversion
#pragma unroll
    for (int q0 = 0; q0 < NLD; q0 += CH) {
        int w[CH];
        float2 wf[CH];
#pragma unroll
        for (int q = 0; q < CH; q++) {
            if (q0 + q < NLD) {
                int e = tid + 256 * (q0 + q);
                e = e < nwin - 1 ? e : nwin - 1;
                e = e > elo ? e : elo;
                if (F32IN)
                    wf[q] = rbf[e];
                else
                    w[q] = rb[e];
            }
        }
#pragma unroll
        for (int q = 0; q < CH; q++) {
            const int e = tid + 256 * (q0 + q);
            if (q0 + q < NLD && e < NE) {
                const float2 v = (e < nwin && e >= elo) ? chan_convert<F32IN>(a, w[q], wf[q]) : make_float2(0.0f, 0.0f);
                xs[(tid + (tid >> 3)) + 288 * (q0 + q)] = v;  // xpad8(tid + 256 q)
            }
        }
    }
    if (w0 < 0) {
        const float2 *hist = a.hist + (long long)in * a.K * DHALO;
        for (int e = tid; e < a.K * DHALO; e += 256) hh[e] = hist[e];
    }
}

// the window's samples before the call (w0 < 0: the call's first 21 samples, which frames shorter than 21 samples share)
// are channel c's own history: xs[xpad8(e)] = x(w0 + e) = hist[(in * K + c) * 21 + 21 + w0 + e] for e < -w0.  Uniform in
// the workgroup; barriers on both sides (the previous channel may still read those slots).
__device__ __forceinline__ void chan_halo(float2 *xs, const float2 *hh, int c, long long w0)
{
    if (w0 >= 0) return;
    __syncthreads();
    if (threadIdx.x < -w0) xs[xpad8(threadIdx.x)] = hh[c * DHALO + DHALO + (int)w0 + threadIdx.x];
    __syncthreads();
}

// one channel on one tile: xt[xpad8(i)] = x(g0 - 21 + i); this thread's 8 detected samples and the running maximum of
// their magnitudes.  last: 256 slots no other tile of this channel uses until a barrier has passed.  prev0: the FM
// detector state before the call (thread 0 at g0 == 0).
__device__ __forceinline__ void chan_tile(const DemodChanConst &c, const float2 *xt, const float2 *nco, long long g0, int len,
                                          float2 *last, float2 prev0, float (&dv)[DPER], unsigned &mbits)
{
    constexpr int PER = DPER;
    const int tid = threadIdx.x;
    const int t0 = tid * PER;
    v2f m[PER];
    if (c.dofir) {
        v2f x[PER + 20];  // x[q] = input sample t0 - 20 + q
#pragma unroll
        for (int q = 0; q < PER + 20; q++) {
            const float2 v = xt[9 * tid + (1 + q) + ((1 + q) >> 3)];
            x[q] = (v2f){v.x, v.y};
        }
#pragma unroll
        for (int u = 0; u < PER; u++) {
            v2f acc = (v2f){0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 21; k++) acc = acc + x[u + 20 - k] * c.w[k];  // ring order: newest sample meets w[0]
            m[u] = acc;
        }
    } else {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const float2 v = xt[9 * tid + (DHALO + u) + ((DHALO + u) >> 3)];
            m[u] = (v2f){v.x, v.y};
        }
    }
    if (c.dodwn) {  // :423-434
        const float2 *nc = nco + g0 + t0;
        float2 cs[PER];
        if (((g0 + t0) & 1) == 0) {  // 16-byte aligned pairs (rows are an even number of entries apart)
#pragma unroll
            for (int u = 0; u < PER; u += 2) {
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
            const v2f v = m[u];
            const v2f cc = (v2f){cs[u].x, cs[u].y};
            const v2f ny = (v2f){-v.y, v.y};
            m[u] = __builtin_shufflevector(v, v, 0, 0) * cc + ny * __builtin_shufflevector(cc, cc, 1, 0);
        }
    }
    float2 prev = make_float2(0.0f, 0.0f);
    if (c.mode == MODE_NFM || c.mode == MODE_WFM) {
        last[tid] = make_float2(m[PER - 1].x, m[PER - 1].y);
        __syncthreads();
        if (tid > 0)
            prev = last[tid - 1];
        else if (g0 > 0)
            prev = chan_mixed_at(c, xt, [](int i) { return xpad8(i); }, DHALO - 1, nco, g0 - 1);
        else
            prev = prev0;
    }
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const v2f mm = m[u];
        if (c.mode == MODE_OFF) {
            dv[u] = 0.0f;
        } else if (c.mode == MODE_RAW) {
            dv[u] = mm.x;
        } else if (c.mode == MODE_AM) {
            dv[u] = __builtin_sqrtf(mm.x * mm.x + mm.y * mm.y);  // :449, as demod_tile
        } else {
            dv[u] = ((prev.x * mm.y) - (prev.y * mm.x)) * c.fmgain;
            prev = make_float2(mm.x, mm.y);
        }
        if (t0 + u < len) {
            const unsigned bb = __float_as_uint(dv[u]) & 0x7fffffffu;
            mbits = bb > mbits ? bb : mbits;
        }
    }
}

// the workgroup's maximum; red: 4 slots no other maximum uses until a barrier has passed
__device__ __forceinline__ unsigned chan_block_max(unsigned mbits, unsigned *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o = __shfl_xor(mbits, off, 64);
        mbits = o > mbits ? o : mbits;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mbits;
    __syncthreads();
    unsigned mx = red[0];
    for (int w = 1; w < 4; w++) mx = red[w] > mx ? red[w] : mx;
    return mx;
}

// a thread's 8 floats of one tile to a d row
__device__ __forceinline__ void chan_store_d(float *drow, long long g, int t0, int len, const float (&dv)[DPER])
{
    float *d = drow + g;
    if (t0 + DPER <= len && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
        reinterpret_cast<float4 *>(d)[0] = make_float4(dv[0], dv[1], dv[2], dv[3]);
        reinterpret_cast<float4 *>(d)[1] = make_float4(dv[4], dv[5], dv[6], dv[7]);
    } else {
#pragma unroll
        for (int u = 0; u < DPER; u++)
            if (t0 + u < len) d[u] = dv[u];
    }
}

template <bool F32IN, int NT>
__global__ __launch_bounds__(256) void k_demod_chan(DemodChanArgs a)
{
    constexpr int PER = DPER;
    constexpr int NE = NT * DTILE + DHALO;
    __shared__ float2 xs[NE + (NE - 1) / 8];
    __shared__ float2 hh[DCHAN_MAX * DHALO];
    __shared__ float2 last[2][256];
    __shared__ unsigned red[2][4];
    const int tid = threadIdx.x;
    const int in = blockIdx.x, f = blockIdx.y;  // inputs fastest: workgroups in flight share the frame's carrier rows
    const int K = a.K;
    const long long fs = (long long)f * a.n;
    const int t0 = tid * PER;
    chan_stage<F32IN, NE>(a, in, fs - DHALO, a.n + DHALO, xs, hh);
    __syncthreads();
    for (int c = 0; c < K; c++) {
        const DemodChanConst &cc = a.c[c];
        const long long s = (long long)in * K + c;
        chan_halo(xs, hh, c, fs - DHALO);  // this channel's own samples before the call
        const float2 prev0 = (f == 0 && tid == 0 && (cc.mode == MODE_NFM || cc.mode == MODE_WFM)) ? a.lilq[s] : make_float2(0.0f, 0.0f);
        const float2 *nco = a.nco + (long long)cc.nco_row * a.nco_pitch;
        float dv[NT][PER];
        unsigned mbits = 0;
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int len = (a.n - j * DTILE) < DTILE ? (a.n - j * DTILE) : DTILE;
            chan_tile(cc, xs + (DTILE + DTILE / 8) * j, nco, fs + (long long)j * DTILE, len, last[j & 1], prev0, dv[j], mbits);
        }
        const unsigned mxb = chan_block_max(mbits, red[c & 1]);
        if (cc.dslot >= 0) {  // AM: k_demod_mean + k_demod_chan_out finish the frame
            const long long row = (long long)cc.dslot * a.ninputs + in;
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const int len = (a.n - j * DTILE) < DTILE ? (a.n - j * DTILE) : DTILE;
                chan_store_d(a.d + row * a.L, fs + (long long)j * DTILE + t0, t0, len, dv[j]);
            }
            if (tid == 0) a.fmax_bits[row * a.nfr + f] = mxb;
            continue;
        }
        const float mx = __uint_as_float(mxb);
        const float scale = cc.doagc ? 1.0f / mx : 1.0f;
        const long long F = s * a.nfr + f;
        if (tid == 0) {  // the reference's `max` / `avg` fields after the frame
            a.stats[2 * F] = mx;
            a.stats[2 * F + 1] = 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int len = (a.n - j * DTILE) < DTILE ? (a.n - j * DTILE) : DTILE;
            const long long g = fs + (long long)j * DTILE + t0;
            int *dst = a.out + s * a.out_stride_pairs + g;
            int o[PER];
#pragma unroll
            for (int u = 0; u < PER; u++) o[u] = demod_lr(dv[j][u] * scale);
            if (t0 + PER <= len && (((s * a.out_stride_pairs + g) & 3) == 0)) {
                reinterpret_cast<int4 *>(dst)[0] = make_int4(o[0], o[1], o[2], o[3]);
                reinterpret_cast<int4 *>(dst)[1] = make_int4(o[4], o[5], o[6], o[7]);
            } else {
#pragma unroll
                for (int u = 0; u < PER; u++)
                    if (t0 + u < len) dst[u] = o[u];
            }
        }
    }
}

// frames of more than 5 tiles: one tile of one input per workgroup, every channel's floats and tile maximum to d / fmax_bits
// (zeroed before the launch); k_demod_mean (AM rows) and k_demod_chan_out finish the frames
template <bool F32IN>
__global__ __launch_bounds__(256) void k_demod_chan_front(DemodChanArgs a)
{
    constexpr int PER = DPER;
    constexpr int NE = DTILE + DHALO;
    __shared__ float2 xs[NE + (NE - 1) / 8];
    __shared__ float2 hh[DCHAN_MAX * DHALO];
    __shared__ float2 last[256];
    __shared__ unsigned red[2][4];
    const int tid = threadIdx.x;
    const int in = blockIdx.y;
    const int K = a.K;
    const int tiles_per_frame = (a.n + DTILE - 1) / DTILE;
    const int f = blockIdx.x / tiles_per_frame;
    const int j = blockIdx.x - f * tiles_per_frame;
    const long long g0 = (long long)f * a.n + (long long)j * DTILE;
    const int len = (a.n - j * DTILE) < DTILE ? (a.n - j * DTILE) : DTILE;
    const int t0 = tid * PER;
    chan_stage<F32IN, NE>(a, in, g0 - DHALO, len + DHALO, xs, hh);
    __syncthreads();
    for (int c = 0; c < K; c++) {
        const DemodChanConst &cc = a.c[c];
        const long long s = (long long)in * K + c;
        chan_halo(xs, hh, c, g0 - DHALO);
        const float2 prev0 = (g0 == 0 && tid == 0 && (cc.mode == MODE_NFM || cc.mode == MODE_WFM)) ? a.lilq[s] : make_float2(0.0f, 0.0f);
        float dv[PER];
        unsigned mbits = 0;
        // (one tile per channel: the block maximum's barrier separates two uses of `last`)
        chan_tile(cc, xs, a.nco + (long long)cc.nco_row * a.nco_pitch, g0, len, last, prev0, dv, mbits);
        const long long row = (long long)cc.dslot * a.ninputs + in;
        chan_store_d(a.d + row * a.L, g0 + t0, t0, len, dv);
        const unsigned mx = chan_block_max(mbits, red[c & 1]);
        if (tid == 0) atomicMax(&a.fmax_bits[row * a.nfr + f], mx);
    }
}

// history for the next call, per stream (i, c) with that channel's switches: the ring only while its filter runs, the
// FM detector's last sample only in the FM modes (k_demod_state)
template <bool F32IN>
__global__ __launch_bounds__(64) void k_demod_chan_state(DemodChanArgs a, float2 *hist_new, float2 *lilq_new)
{
    __shared__ float2 xs[2 * DHALO];
    const int s = blockIdx.x;
    const int tid = threadIdx.x;
    const int in = s / a.K, c = s - in * a.K;
    const DemodChanConst &cc = a.c[c];
    const int *raw = a.raw + (long long)in * a.stride_pairs;
    const float2 *rawf = a.rawf + (long long)in * a.stride_pairs;
    const float2 *hist = a.hist + (long long)s * DHALO;
    if (tid < 2 * DHALO) {  // xs[i] = x(L - 42 + i)
        const long long g = a.L - 2 * DHALO + tid;
        float2 v = make_float2(0.0f, 0.0f);
        if (g >= 0)
            v = chan_convert<F32IN>(a, F32IN ? 0 : raw[g], F32IN ? rawf[g] : make_float2(0.0f, 0.0f));
        else if (g >= -DHALO)
            v = hist[DHALO + g];
        xs[tid] = v;
    }
    __syncthreads();
    if (tid < DHALO) hist_new[(long long)s * DHALO + tid] = cc.dofir ? xs[DHALO + tid] : hist[tid];
    if (tid == 0) {
        const bool fm = cc.mode == MODE_NFM || cc.mode == MODE_WFM;
        lilq_new[s] = (fm && a.L > 0) ? chan_mixed_at(cc, xs, [](int i) { return i; }, 2 * DHALO - 1,
                                                      a.nco + (long long)cc.nco_row * a.nco_pitch, a.L - 1)
                                      : a.lilq[s];
    }
}

// :465-481 for the d rows (k_demod_out with the row -> stream map): grid (chunks of 1024 samples, frame, row)
__global__ __launch_bounds__(256) void k_demod_chan_out(DemodChanArgs a, const float *__restrict__ favg)
{
    const int f = blockIdx.y, row = blockIdx.z;
    const int slot = row / a.ninputs, in = row - slot * a.ninputs;
    const int c = a.slot_chan[slot];
    const int mode = a.c[c].mode, doagc = a.c[c].doagc;
    const long long s = (long long)in * a.K + c;
    const int n = a.n;
    const long long F = (long long)row * a.nfr + f;
    float mx = __uint_as_float(a.fmax_bits[F]);
    const float avg = (mode == MODE_AM) ? favg[F] : 0.0f;
    if (mode == MODE_AM) mx -= avg;
    const float scale = doagc ? 1.0f / mx : 1.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long FS = s * a.nfr + f;
        a.stats[2 * FS] = mx;
        a.stats[2 * FS + 1] = avg;
    }
    const int t = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (t >= n) return;
    const long long g = (long long)f * n + t;
    const float *src = a.d + (long long)row * a.L + g;
    int *dst = a.out + s * a.out_stride_pairs + g;
    float v[4];
    const bool vec = (t + 4 <= n) && ((((long long)row * a.L + g) & 3) == 0) && (((s * a.out_stride_pairs + g) & 3) == 0);
    if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(src);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = (t + u < n) ? src[u] : 0.0f;
    }
    int o[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        float x = v[u];
        if (mode == MODE_AM) x = x - avg;
        o[u] = demod_lr(x * scale);
    }
    if (vec) {
        *reinterpret_cast<int4 *>(dst) = make_int4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (t + u < n) dst[u] = o[u];
    }
}

template <bool F32IN>
static void launch_fused(const DemodChanArgs &a, int tiles, hipStream_t st)
{
    const dim3 grid((unsigned)a.ninputs, (unsigned)a.nfr);
    switch (tiles) {
        case 1: hipLaunchKernelGGL((k_demod_chan<F32IN, 1>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_demod_chan<F32IN, 2>), grid, dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL((k_demod_chan<F32IN, 3>), grid, dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_demod_chan<F32IN, 4>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((k_demod_chan<F32IN, 5>), grid, dim3(256), 0, st, a); break;
    }
}

int launch_demod_chan(const DemodChanArgs &a, bool f32in, bool fused, hipStream_t st)
{
    const int tiles = (a.n + DTILE - 1) / DTILE;
    if (fused) {
        if (f32in)
            launch_fused<true>(a, tiles, st);
        else
            launch_fused<false>(a, tiles, st);
    } else {
        const dim3 grid((unsigned)(tiles * a.nfr), (unsigned)a.ninputs);
        if (f32in)
            hipLaunchKernelGGL(k_demod_chan_front<true>, grid, dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(k_demod_chan_front<false>, grid, dim3(256), 0, st, a);
    }
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_demod_chan_state(const DemodChanArgs &a, bool f32in, float2 *hist_new, float2 *lilq_new, hipStream_t st)
{
    const dim3 grid((unsigned)(a.ninputs * a.K));
    if (f32in)
        hipLaunchKernelGGL(k_demod_chan_state<true>, grid, dim3(64), 0, st, a, hist_new, lilq_new);
    else
        hipLaunchKernelGGL(k_demod_chan_state<false>, grid, dim3(64), 0, st, a, hist_new, lilq_new);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_demod_chan_out(const DemodChanArgs &a, int drows, const float *favg, hipStream_t st)
{
    hipLaunchKernelGGL(k_demod_chan_out, dim3((unsigned)((a.n + 1023) / 1024), (unsigned)a.nfr, (unsigned)drows), dim3(256), 0, st,
                       a, favg);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
