// bpsk_scope_spec.hip -- the second half of FUNcubeBPSKDemod.paintComponent's panel (FUNcubeBPSKDemod.java:270-327): the green
// spectrum of the `tuned` ring and the cyan one of the `downSmpl` ring, for every frame row of a scope call
// (jsdr_bpsk_scope_spectra_i16 / _f32; the host side is bpsk_scope.hip's).  Compiled with -ffp-contract=off: every product and
// sum is one IEEE double operation, in the oracle's order.
//
// One workgroup takes one row of len complex doubles: the row is read once, 16 bytes a lane, into an LDS image and transformed
// there as the oracle's jo_fft_f64 (oracle/o_fft.c) transforms it --
//   k_bpsk_spec_pow2<LOGN>   len = 2^LOGN, 64 .. 8192: the bit-reversed radix-2 network on fft_twiddles_f64's table, four stages
//                            in registers on a row of 16 (bpsk_acq_dev.h: acq_stages, the image under acq_slot), then passes of
//                            up to four stages in place; len / 16 threads, 64 at least
//   k_bpsk_spec_mixed<T, M>  any other len up to M: the Stockham passes in the oracle's radix order from the row's plan
//                            (fft_plan_build_row), a pass in place through registers -- every butterfly of the pass is read before
//                            the barrier and written behind it -- radices 2, 3, 4, 5, 7 as bpsk_radix.h's dft_r, a prime radix above
//                            7 as the oracle's definition (o_fft.c:207-227: a full complex multiply even by W[0], summed left to
//                            right), one thread an output, its sums held in registers across the barrier: no second image and no
//                            scratch in global memory.  T = 64 threads for len <= 512 (L = 204, 102, 409: one wave a row, as many
//                            rows a CU as its waves), 256 for len <= 2048, 768 for len <= 9600.
// -- and the epilogue runs in the same kernel: |Y| of every bin through registers into the image's first len doubles (and to
// psd_dev), the strict first maximum over all len bins (first_max_update, wave_first_max, wg_first_max: a NaN never wins, ties go
// to the lowest bin), then one lane a column for getMax and the cast (:293-299).  Only what is asked for is stored.
#include "bpsk_scope_spec.h"
#include "bpsk_acq_dev.h"
#include "bpsk_radix.h"

namespace jsdr {
#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------------------------------- the epilogue
// X: the transformed image, bin k at X[slot(k)]; P = the same bytes as doubles.  red: [16] doubles, [16] ints.
template <int T, int ITERS, class SLOT>
__device__ __forceinline__ void spec_epilogue(double2 *X, double *red, const ScopeSpecArgs &a, long long orow, int tid, SLOT slot)
{
    double *P = reinterpret_cast<double *>(X);
    int *redi = reinterpret_cast<int *>(red + 16);
    const int len = a.len;
    double p[ITERS];
    double bestv = 0.0;  // :274-275
    int besti = -1;
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int k = it * T + tid;
        p[it] = 0.0;
        if (k < len) {
            const double2 z = X[slot(k)];
            p[it] = sqrt(z.x * z.x + z.y * z.y);  // :277
            first_max_update(bestv, besti, p[it], k);  // (k ascends within a thread)
        }
    }
    __syncthreads();  // every bin is in registers before the image becomes psd[]
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int k = it * T + tid;
        if (k < len) {
            P[k] = p[it];
            if (a.psd) a.psd[orow * len + k] = p[it];
        }
    }
    if (!a.peak && !a.spec) return;
    wave_first_max(bestv, besti);
    if constexpr (T > 64) {
        if ((tid & 63) == 0) {
            red[tid >> 6] = bestv;
            redi[tid >> 6] = besti;
        }
        __syncthreads();
        wg_first_max<T / 64>(red, redi, tid & 63, bestv, besti);
    } else {
        __syncthreads();
    }
    const double mx = bestv;              // 0.0 where no bin is above 0 (silence, a row of NaN)
    const int mo = besti < 0 ? 0 : besti;
    if (a.peak && tid == 0) {
        a.peak[2 * orow] = mx;
        a.peak[2 * orow + 1] = (double)mo;
    }
    if (!a.spec) return;
    const double ys = 100.0 / mx;  // :293
    for (int m = tid; m < a.width; m += T) {
        double d;
        if (m == 0) {
            d = P[0];  // :294
        } else {
            const int i = (int)(a.pi * (double)m);  // :296
            d = P[i];                               // getMax (:348-355)
            for (int j = i + 1; j < i + a.l; j++)
                if (d < P[j]) d = P[j];
        }
        a.spec[orow * a.width + m] = java_d2i(d * ys);
    }
}

// ------------------------------------------------------------------------------------------- powers of two
template <int G, int HALF0, int LOGN, int T>
__device__ __forceinline__ void spec_mid_pass(double2 *X, const double2 *TsL, const double2 *__restrict__ tsg, int tid)
{
    constexpr int N = 1 << LOGN, M = 1 << G, NQ = N >> G;
    static_assert(HALF0 % 16 == 0, "the passes behind the first move whole rows");
#pragma unroll
    for (int q = tid; q < NQ; q += T) {
        const int j = q & (HALF0 - 1);
        const int e0 = ((q - j) << G) + j;
        double2 v[M];
#pragma unroll
        for (int m = 0; m < M; m++) v[m] = X[acq_slot_hm(e0, HALF0 * m)];
        acq_stages<G, HALF0, false, false>(v, j, TsL, tsg);
#pragma unroll
        for (int m = 0; m < M; m++) X[acq_slot_hm(e0, HALF0 * m)] = v[m];
    }
    __syncthreads();
}

// the stages behind the first DONE, in passes of four stages at most, as even as they come
template <int LOGN, int DONE, int T>
__device__ __forceinline__ void spec_rest(double2 *X, const double2 *TsL, const double2 *__restrict__ tsg, int tid)
{
    if constexpr (DONE < LOGN) {
        constexpr int REM = LOGN - DONE, NP = (REM + 3) / 4, G = (REM + NP - 1) / NP;
        spec_mid_pass<G, 1 << DONE, LOGN, T>(X, TsL, tsg, tid);
        spec_rest<LOGN, DONE + G, T>(X, TsL, tsg, tid);
    }
}

template <int LOGN>
struct SpecPow2 {
    static constexpr int N = 1 << LOGN, T = N / 16 < 64 ? 64 : N / 16;
    static constexpr int TWL = N - 1 < ACQ_TWL ? N - 1 : ACQ_TWL - 1;  // table entries copied to LDS
    static constexpr size_t LDS = sizeof(double2) * (size_t)(N + ACQ_TWL) + sizeof(double) * 16 + sizeof(int) * 16;
};

template <int LOGN>
__global__ __launch_bounds__(SpecPow2<LOGN>::T) void k_bpsk_spec_pow2(ScopeSpecArgs a)
{
    constexpr int N = SpecPow2<LOGN>::N, T = SpecPow2<LOGN>::T;
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *X = reinterpret_cast<double2 *>(smem);  // [N] under acq_slot
    double2 *TsL = X + N;                            // [ACQ_TWL]
    double *red = reinterpret_cast<double *>(TsL + ACQ_TWL);
    const int tid = threadIdx.x;
    const long long row = blockIdx.x;
    const int s = (int)(row / a.c), f = (int)(row - (long long)s * a.c);
    const long long orow = (long long)s * a.frames + a.f0 + f;
    const double2 *in = a.rows + row * N;
    for (int i = tid; i < N; i += T) X[acq_slot(i)] = in[i];
    for (int i = tid; i < SpecPow2<LOGN>::TWL; i += T) TsL[i] = a.tw[i];
    __syncthreads();
    // wings 1, 2, 4, 8 on the row of 16 elements e = 16 q + m of the bit-reversed order
    double2 v[16];
    const int q = tid;
    if (q < N / 16) {
#pragma unroll
        for (int m = 0; m < 16; m++) v[m] = X[acq_slot(acq_brev<LOGN>(16 * q + m))];
        acq_stages<4, 1, false, false>(v, 0, TsL, a.tw);
    }
    __syncthreads();  // every element has been read from its natural slot
    if (q < N / 16) {
#pragma unroll
        for (int m = 0; m < 16; m++) X[acq_slot(16 * q + m)] = v[m];
    }
    __syncthreads();
    spec_rest<LOGN, 4, T>(X, TsL, a.tw, tid);
    spec_epilogue<T, (N + T - 1) / T>(X, red, a, orow, tid, [](int k) { return acq_slot(k); });
}

// ------------------------------------------------------------------------------------------- any other length
// b mod P without the division sequence (fft_pass_args: exact for b < 2^16)
__device__ __forceinline__ int spec_mod(int b, int P, unsigned pmagic) { return P == 1 ? 0 : b - (int)__umulhi((unsigned)b, pmagic) * P; }

// one Stockham pass of radix R, in place: every butterfly of the pass is in registers before the first store (the oracle's
// loop body, o_fft.c:232-241)
template <int R, int T, int NMAX>
__device__ __forceinline__ void spec_pass(double2 *X, const double2 *__restrict__ tw, int n, int P, unsigned pmagic, int tid)
{
    constexpr int ITERS = (NMAX / R + T - 1) / T;
    const int nb = n / R;
    double2 v[ITERS][R];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int b = it * T + tid;
        if (b < nb) {
            const int k = spec_mod(b, P, pmagic);
#pragma unroll
            for (int j = 0; j < R; j++) {
                v[it][j] = X[b + j * nb];
                if (j >= 1 && P > 1) v[it][j] = cdmul(v[it][j], tw[k * j]);
            }
            dft_r<R>(v[it]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int b = it * T + tid;
        if (b < nb) {
            const int k = spec_mod(b, P, pmagic);
            const int j0 = (b - k) * R + k;
#pragma unroll
            for (int qq = 0; qq < R; qq++) X[j0 + qq * P] = v[it][qq];
        }
    }
    __syncthreads();
}

// a prime radix above 7 (o_fft.c:207-227), one thread an output:
//   out[(b - k) r + k + q P] = v_0 + v_1 W[q mod r] + ... + v_{r-1} W[(r-1) q mod r],  v_j = X[b + j nb] (x T[k j] for j >= 1, P > 1)
// the twiddled inputs formed again for every output (the same values), the sums in registers across the barrier
template <int T, int NMAX>
__device__ __forceinline__ void spec_pass_prime(double2 *X, const double2 *__restrict__ tw, const double2 *__restrict__ wr, int n, int P,
                                                int r, unsigned pmagic, int tid)
{
    constexpr int ITERS = (NMAX + T - 1) / T;
    const int nb = n / r;
    double2 acc[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int o = it * T + tid;
        acc[it] = make_double2(0.0, 0.0);
        if (o < n) {
            const int q = o / nb, b = o - q * nb;  // outputs of one q are contiguous over b
            const int k = spec_mod(b, P, pmagic);
            double2 s = X[b];
            int m = 0;  // (j q) mod r
            for (int j = 1; j < r; j++) {
                m += q;
                if (m >= r) m -= r;
                double2 x = X[b + j * nb];
                if (P > 1) x = cdmul(x, tw[k * j]);
                s = cdadd(s, cdmul(x, wr[m]));
            }
            acc[it] = s;
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int o = it * T + tid;
        if (o < n) {
            const int q = o / nb, b = o - q * nb;
            const int k = spec_mod(b, P, pmagic);
            X[(b - k) * r + k + q * P] = acc[it];
        }
    }
    __syncthreads();
}

template <int T, int NMAX>
__global__ __launch_bounds__(T) void k_bpsk_spec_mixed(ScopeSpecArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *X = reinterpret_cast<double2 *>(smem);  // [len]
    const int n = a.len;
    double *red = reinterpret_cast<double *>(X + n);
    const int tid = threadIdx.x;
    const long long row = blockIdx.x;
    const int s = (int)(row / a.c), f = (int)(row - (long long)s * a.c);
    const long long orow = (long long)s * a.frames + a.f0 + f;
    const double2 *in = a.rows + row * n;
    for (int i = tid; i < n; i += T) X[i] = in[i];
    __syncthreads();
    int P = 1;
    for (int p = 0; p < a.m.np; p++) {
        const int r = a.m.rad[p];
        const double2 *tw = a.tw + a.m.tw_off[p];
        const unsigned pm = a.m.pmagic[p];
        if (r == 4)
            spec_pass<4, T, NMAX>(X, tw, n, P, pm, tid);
        else if (r == 2)
            spec_pass<2, T, NMAX>(X, tw, n, P, pm, tid);
        else if (r == 3)
            spec_pass<3, T, NMAX>(X, tw, n, P, pm, tid);
        else if (r == 5)
            spec_pass<5, T, NMAX>(X, tw, n, P, pm, tid);
        else if (r == 7)
            spec_pass<7, T, NMAX>(X, tw, n, P, pm, tid);
        else
            spec_pass_prime<T, NMAX>(X, tw, a.tw + a.m.wr_off[p], n, P, r, pm, tid);
        P *= r;
    }
    spec_epilogue<T, (NMAX + T - 1) / T>(X, red, a, orow, tid, [](int k) { return k; });
}

#pragma GCC visibility pop

// ------------------------------------------------------------------------------------------- the launcher
static bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

const char *scope_spec_form(int len)
{
    if (is_pow2(len)) return (len >= SPEC_POW2_MIN && len <= SPEC_POW2_MAX) ? "k_bpsk_spec_pow2" : nullptr;
    int rad[FFT_MAXPASS];
    const int np = len >= 2 && len <= FM_NMAX ? fft_radices(len, rad) : 0;
    if (np < 1 || np > FM_MAXPASS) return nullptr;
    return len <= SPEC_SMALL_MAX ? "k_bpsk_spec_mixed64" : len <= SPEC_MID_MAX ? "k_bpsk_spec_mixed256" : "k_bpsk_spec_mixed768";
}

template <int LOGN>
static int launch_pow2(const ScopeSpecArgs &a, long long nrows, hipStream_t st)
{
    JSDR_LDS_ATTR(k_bpsk_spec_pow2<LOGN>, SpecPow2<LOGN>::LDS);
    hipLaunchKernelGGL(k_bpsk_spec_pow2<LOGN>, dim3((unsigned)nrows), dim3(SpecPow2<LOGN>::T), SpecPow2<LOGN>::LDS, st, a);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

template <int T, int NMAX>
static int launch_mixed(const ScopeSpecArgs &a, long long nrows, hipStream_t st)
{
    const size_t lds = sizeof(double2) * (size_t)a.len + sizeof(double) * 16 + sizeof(int) * 16;
    JSDR_LDS_ATTR((k_bpsk_spec_mixed<T, NMAX>), lds);
    hipLaunchKernelGGL((k_bpsk_spec_mixed<T, NMAX>), dim3((unsigned)nrows), dim3(T), lds, st, a);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_scope_spec(const ScopeSpecArgs &a, long long nrows, hipStream_t st)
{
    JSDR_REQUIRE(scope_spec_form(a.len) && nrows > 0 && nrows < (1LL << 31) && a.c > 0, "launch_scope_spec: internal: no kernel form for "
                 "%lld rows of %d points", nrows, a.len);
    if (a.logn) {
        JSDR_REQUIRE((1 << a.logn) == a.len, "launch_scope_spec: internal: logn=%d of a row of %d points", a.logn, a.len);
        switch (a.logn) {
        case 6: return launch_pow2<6>(a, nrows, st);
        case 7: return launch_pow2<7>(a, nrows, st);
        case 8: return launch_pow2<8>(a, nrows, st);
        case 9: return launch_pow2<9>(a, nrows, st);
        case 10: return launch_pow2<10>(a, nrows, st);
        case 11: return launch_pow2<11>(a, nrows, st);
        case 12: return launch_pow2<12>(a, nrows, st);
        default: return launch_pow2<13>(a, nrows, st);
        }
    }
    JSDR_REQUIRE(a.m.np >= 1 && a.m.np <= FM_MAXPASS && a.m.f.n == a.len, "launch_scope_spec: internal: the plan is not the row's (%d points)",
                 a.len);
    if (a.len <= SPEC_SMALL_MAX) return launch_mixed<64, SPEC_SMALL_MAX>(a, nrows, st);
    if (a.len <= SPEC_MID_MAX) return launch_mixed<256, SPEC_MID_MAX>(a, nrows, st);
    return launch_mixed<768, FM_NMAX>(a, nrows, st);
}

}  // namespace jsdr
