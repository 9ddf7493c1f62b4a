// bpsk_fft2x.hip -- the FFT-acquire front end for frames of 2 m samples, m a mixed-radix frame that fits a workgroup's LDS
// (n = 19200 at 192 kHz): k_front_fft2x, on the passes of bpsk_fftm_dev.h and the c = 1 passes below.  Compiled with
// -ffp-contract=off.
#include "bpsk_fftm_dev.h"

namespace jsdr {

// ============================================================================================== frames of 2 m samples
// n = 19200 (192 kHz with java-sdr's default buffer, JavaAudio.java:58-59: the FUNcube Dongle Pro+ frame): 307 KB as
// double2, twice a workgroup's LDS.  The oracle's transform for n > 9600 starts with ONE radix-2 pass
// (jo_fft_mixed_radices), which splits it into two INDEPENDENT m = n/2 point halves: half c (0 / 1) holds, pass after
// pass, the elements of parity c, and ends as the even / odd output bins.  In half-array coordinates every later
// pass is the m-point Stockham pass; only its twiddles differ: T_{2P'r}[(2k'+c) j] instead of T_{P'r}[k' j] -- for c = 0
// the same numbers (the m-point tables; the long-double arguments scale by an exact 2), for c = 1 a table of its own.
// So a frame is four m-point transforms in the one LDS image (forward c = 0, 1, inverse c = 0, 1); what has to
// outlive the image goes through a per-stream scratch in global memory (L2 sized: 154 KB):
//   ek : the even bins the 204-bin gather may need (bins below n/2 + 102) -- written after the forward c = 0 half
//   r0 : the even output samples re * (1/n) of the inverse -- read by RxDownSample beside the odd ones in LDS
// Same butterflies, same tables, same order as the oracle's fft_f64_mixed with radices 2,4,4,4,2,3,5,5: bit-identical
// centre bins, traces, bits.  Not tuned: single passes for the c = 1 halves, twiddles from L2.
// (Fft2xArgs: bpsk_fftplan.h)

// one Stockham pass with a two-dimensional twiddle table tw[(j-1) P + k], every input j >= 1 multiplied (also at P = 1)
template <int R>
__device__ __attribute__((noinline)) void fm_pass_t(LdsArr X, GblArr tw, int n, int P, unsigned pmagic, int tid)
{
    constexpr int ITERS = ((FM_NMAX / R) + FM_T - 1) / FM_T;
    const int nb = n / R;
    double2 v[ITERS][R];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int b = it * FM_T + tid;
        if (b < nb) {
            const int k = (P == 1) ? 0 : b - (int)__umulhi((unsigned)b, pmagic) * P;
#pragma unroll
            for (int j = 0; j < R; j++) {
                v[it][j] = X[b + j * nb];
                if (j >= 1) v[it][j] = cdmul(v[it][j], tw[(j - 1) * P + k]);
            }
            dft_r<R>(v[it]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int b = it * FM_T + tid;
        if (b < nb) {
            const int k = (P == 1) ? 0 : b - (int)__umulhi((unsigned)b, pmagic) * P;
            const int j0 = (b - k) * R + k;
#pragma unroll
            for (int q = 0; q < R; q++) X[j0 + q * P] = v[it][q];
        }
    }
    __syncthreads();
}

// two consecutive passes of an odd half in one LDS round trip: fm_pass2 with the two-dimensional tables
template <int R1, int R2, int NN, int PP, bool SWZ_IN = false>
__device__ __attribute__((noinline)) void fm_pass2_t(LdsArr X, GblArr tw1, GblArr tw2, int tid)
{
    constexpr int RR = R1 * R2;
    constexpr int ITERS = ((NN / RR) + FM_T - 1) / FM_T;
    constexpr int ng = NN / RR, nb1 = NN / R1, P = PP, P2 = PP * R1;
    double2 v[ITERS][R2][R1];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int g = it * FM_T + tid;
        if (g < ng) {
            const int k1 = g % PP;
#pragma unroll
            for (int j2 = 0; j2 < R2; j2++) {
                const int b1 = g + j2 * ng;
#pragma unroll
                for (int j1 = 0; j1 < R1; j1++) {
                    v[it][j2][j1] = X[SWZ_IN ? fm_swz(b1 + j1 * nb1) : b1 + j1 * nb1];
                    if (j1 >= 1) v[it][j2][j1] = cdmul(v[it][j2][j1], tw1[(j1 - 1) * P + k1]);
                }
                dft_r<R1>(v[it][j2]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q1 = 0; q1 < R1; q1++) {
                const int k2 = k1 + q1 * P;
                double2 w[R2];
#pragma unroll
                for (int j2 = 0; j2 < R2; j2++) {
                    w[j2] = v[it][j2][q1];
                    if (j2 >= 1) w[j2] = cdmul(w[j2], tw2[(j2 - 1) * P2 + k2]);
                }
                dft_r<R2>(w);
#pragma unroll
                for (int q2 = 0; q2 < R2; q2++) v[it][q2][q1] = w[q2];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int g = it * FM_T + tid;
        if (g < ng) {
            const int k1 = g % PP;
            const LdsArr z = X + ((g - k1) * RR + k1);
#pragma unroll
            for (int q2 = 0; q2 < R2; q2++)
#pragma unroll
                for (int q1 = 0; q1 < R1; q1++) z[q1 * P + q2 * P * R1] = v[it][q2][q1];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void fm_forward_odd(LdsArr X, const Fft2xArgs &a, int tid, int mode = FM_FULL, int need_end = 0,
                                               double norm = 1.0, bool first2_done = false)
{
    const FftmArgs &m = a.sub;
    if (m.f.n == 9600) {  // the 192 kHz default: the 9600-point plan 4 | 4,4 | 2,3 | 5 | 5 with pass pairs, as fm_forward
        const GblArr t = gbl_arr(m.f.tw);
        if (mode == FM_INV_REAL && first2_done) {  // after fm_inv_blocks128_9600 with the odd tables; compact real samples
            fm_pass2_t<3, 5, 9600, 128>(X, t + a.tw1_off[4], t + a.tw1_off[5], tid);
            fm_pass5_real<9600, 1920, true, 1>(X, t + a.tw1_off[6], norm, tid);
            return;
        }
        if (mode == FM_FWD_BAND && first2_done) {  // after fm_first2x_from_raw<.., ODD>: 4,2 | 3,5 | 5 as fm_forward
            fm_pass2_t<4, 2, 9600, 16, true>(X, t + a.tw1_off[2], t + a.tw1_off[3], tid);
            fm_pass2_t<3, 5, 9600, 128>(X, t + a.tw1_off[4], t + a.tw1_off[5], tid);
            fm_pass5_band<9600, 1920, true>(X, t + a.tw1_off[6], need_end, tid);
            return;
        }
        if (mode != FM_INV_REAL) {
            fm_pass_t<4>(X, t + a.tw1_off[0], 9600, 1, 0u, tid);
            fm_pass2_t<4, 4, 9600, 4>(X, t + a.tw1_off[1], t + a.tw1_off[2], tid);
        }
        fm_pass2_t<2, 3, 9600, 64>(X, t + a.tw1_off[3], t + a.tw1_off[4], tid);
        fm_pass_t<5>(X, t + a.tw1_off[5], 9600, 384, m.pmagic[5], tid);
        if (mode == FM_FWD_BAND)
            fm_pass5_band<9600, 1920, true>(X, t + a.tw1_off[6], need_end, tid);
        else if (mode == FM_INV_REAL)
            fm_pass5_real<9600, 1920, true>(X, t + a.tw1_off[6], norm, tid);
        else
            fm_pass_t<5>(X, t + a.tw1_off[6], 9600, 1920, m.pmagic[6], tid);
        return;
    }
    int P = 1;
    for (int p = 0; p < m.np; p++) {
        const int r = m.rad[p];
        const GblArr tw = gbl_arr(m.f.tw + a.tw1_off[p]);
        if (r == 4)
            fm_pass_t<4>(X, tw, m.f.n, P, m.pmagic[p], tid);
        else if (r == 2)
            fm_pass_t<2>(X, tw, m.f.n, P, m.pmagic[p], tid);
        else if (r == 3)
            fm_pass_t<3>(X, tw, m.f.n, P, m.pmagic[p], tid);
        else
            fm_pass_t<5>(X, tw, m.f.n, P, m.pmagic[p], tid);
        P *= r;
    }
}

template <bool F32IN>
__global__ __launch_bounds__(FM_T) void k_front_fft2x(Fft2xArgs aa)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const FftFrontArgs &a = aa.sub.f;
    const int n = aa.n, m = n / 2;
    double2 *X = reinterpret_cast<double2 *>(smem);      // [m]: one half at a time
    const LdsArr XL = lds_arr(smem);                     // the same image for the passes (typed view)
    double *hist = reinterpret_cast<double *>(X + m);    // [64]: [0,26) the previous frame's last 26 scaled samples
    double *redv = hist + 64;
    int *redi = reinterpret_cast<int *>(redv + 16);
    double2 *zb = reinterpret_cast<double2 *>(redi + 16);  // [204] the gathered bins, conjugated (default frame only)
    const bool pruned = (m == 9600);  // the 192 kHz default: pruned passes (fm_inv_blocks, fm_pass5_band / _real)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x;
    const int beg = acq_band_beg(n, a.do_up), end = acq_band_end(n, a.do_up);
    const int pbase = beg + 24, abase = beg + 74;
    // |X| and the boxcar sums live behind the odd bins the gather may still need (bins < n/2 + 102 <=> slot < m/2 + 51)
    double *P = reinterpret_cast<double *>(X + (m / 2 + 56));
    double *A = P + (n / 4 - 48);
    FftFrontState *sp = &a.st[s];
    if (tid < 26) hist[tid] = sp->hist[tid];
    double avePeakPower, aveCentreBin;
    int centreBin;
    acq_state_load(sp, avePeakPower, aveCentreBin, centreBin);
    const int D = a.decim;
    const double norm = 1.0 / (double)n;
    const int *__restrict__ raw = a.raw + (long long)s * a.stride_pairs;
    const float2 *__restrict__ rawf = a.rawf + (long long)s * a.stride_pairs;
    double2 *dm = a.dm + (long long)s * a.dm_stride;
    double2 *ek = aa.ek + (long long)s * aa.ek_stride;
    double *r0 = aa.r0 + (long long)s * aa.r0_stride;
    const int nek = m / 2 + 52;
    __syncthreads();

    // the radix-2 first pass straight from the frame's samples: X[b] = x[b] +/- x[b + m]   (:416-421, dft_r<2>)
    auto load_half = [&](long long t0, int c, int tf) {
        for (int b = tf; b < m; b += FM_T) {
            const double2 v0 = F32IN ? acq_sample(rawf[t0 + b]) : acq_sample(raw[t0 + b], a.ic, a.qc);
            const double2 v1 = F32IN ? acq_sample(rawf[t0 + b + m]) : acq_sample(raw[t0 + b + m], a.ic, a.qc);
            X[b] = c ? cdsub(v0, v1) : cdadd(v0, v1);
        }
        __syncthreads();
    };
    // bin `bin` of the full spectrum after both forward halves: even bins from the scratch, odd ones from the image
    auto spectrum = [&](int bin) -> double2 { return (bin & 1) ? X[bin >> 1] : ek[bin >> 1]; };

    for (int f = 0; f < a.nframes; f++) {
        const long long t0 = (long long)f * n;
        int tf = tid;
        asm volatile("" : "+v"(tf));
        // ---- forward, even bins
        // bins below end + 102 are read (see fm_pass5_band): even bin 2 i <=> output i of this half
        const int need_even = (end + 102 + 1) / 2, need_odd = (end + 102) / 2;
        if (pruned) {
            const GblArr tg = gbl_arr(aa.sub.f.tw);
            fm_first2x_from_raw<9600, F32IN, false>(XL, raw + t0, rawf + t0, a.ic, a.qc, tg, tg + 4, tf);
            fm_forward<false>(XL, nullptr, aa.sub, tf, true, FM_FWD_BAND, need_even);
        } else {
            load_half(t0, 0, tf);
            fm_forward<false>(XL, nullptr, aa.sub, tf, false, FM_FULL, need_even);
        }
        for (int i = tf; i < (pruned ? need_even : nek); i += FM_T) ek[i] = X[i];
        __threadfence_block();
        __syncthreads();
        // ---- forward, odd bins
        if (pruned) {
            const GblArr tg = gbl_arr(aa.sub.f.tw);
            fm_first2x_from_raw<9600, F32IN, true>(XL, raw + t0, rawf + t0, a.ic, a.qc, tg + aa.tw1_off[0], tg + aa.tw1_off[1], tf);
            fm_forward_odd(XL, aa, tf, FM_FWD_BAND, need_odd, 1.0, true);
        } else {
            load_half(t0, 1, tf);
            fm_forward_odd(XL, aa, tf, FM_FULL, need_odd);
        }
        // ---- |X| over the band the boxcar reads (:425-427)
        // (pbase is even: even bins come from the scratch, odd ones from the image -- one loop each, no per-bin branch)
        for (int i = pbase + 2 * tf; i < end - 24; i += 2 * FM_T) {
            const double2 v = ek[i >> 1];
            P[i - pbase] = sqrt(v.x * v.x + v.y * v.y);
        }
        for (int i = pbase + 1 + 2 * tf; i < end - 24; i += 2 * FM_T) {
            const double2 v = X[i >> 1];
            P[i - pbase] = sqrt(v.x * v.x + v.y * v.y);
        }
        __syncthreads();
        // ---- 100-wide boxcar, first maximum (:433-442)
        double bestv = 0.0;
        int besti = -1;
        for (int i = beg + 74 + 2 * tf; i < end - 75; i += 2 * FM_T) {
            const double2 *w = reinterpret_cast<const double2 *>(P + (i - 50 - pbase));
            double a0, a1;
            boxcar_pair(w, a0, a1);
            boxcar_put(a0, a1, A + (i - abase), i, beg, end, bestv, besti);
        }
        wave_first_max(bestv, besti);
        if (lane == 0) {
            redv[wave] = bestv;
            redi[wave] = besti;
        }
        __syncthreads();
        // ---- centre-bin rule (:444-453)
        {
            double maxBin;
            int binPos;
            wg_first_max<FM_T / 64>(redv, redi, lane, maxBin, binPos);
            centreBin = centre_bin_clamp(centreBin, end);
            const double atc = acq_band_filled(centreBin, beg, end) ? A[centreBin - abase] : 0.0;
            centre_bin_step(avePeakPower, aveCentreBin, centreBin, atc, maxBin, binPos);
        }
        // ---- 204 bins around the centre to bin 0 of a zeroed array (:458); inverse (:459) as conj o forward o conj
        double2 keep = make_double2(0.0, -0.0);  // conj of the zeroed array
        if (tf < 204) {
            const double2 v = spectrum(centreBin - 102 + tf);
            keep = make_double2(v.x, -v.y);
        }
        __syncthreads();
        const double2 Z = make_double2(0.0, -0.0);
        if (pruned) {
            // The radix-2 first pass leaves z[b] + Z = z[b] in the even half and z[b] - Z = z[b] in the odd one (b < 204, zeros
            // elsewhere): both halves start from the same 204 values, and their first three passes come straight from
            // them (fm_inv_blocks) -- the even half with the 9600-point tables, the odd one with its own
            if (tf < 204) zb[tf] = keep;
            __syncthreads();
            // (four passes, 4,4,4,2: fm_inv_blocks128_9600; the even half's samples re / n (:462) go straight to the scratch, the
            //  odd half's stay in LDS as a compact array of doubles -- sample 2 i + 1 at slot FM_RB0 + i)
            const GblArr tg = gbl_arr(aa.sub.f.tw);
            fm_inv_blocks128_9600<false>(XL, lds_arr(zb), tg + 20, tg + 84, tf);
            fm_forward<false>(XL, nullptr, aa.sub, tf, true, FM_INV_REAL, 0, norm, nullptr, r0);
            fm_inv_blocks128_9600<false>(XL, lds_arr(zb), tg + aa.tw1_off[2], tg + aa.tw1_off[3], tf);  // U_2[k], U_3[kk]
            fm_forward_odd(XL, aa, tf, FM_INV_REAL, 0, norm, true);
        } else {
            // even output samples: first-pass sums z[b] + z[b + m], z[b + m] being the zeroed array's
            for (int b = tf; b < m; b += FM_T) X[b] = cdadd(b < 204 ? keep : Z, Z);
            __syncthreads();
            fm_forward<false>(XL, nullptr, aa.sub, tf, false);
            for (int i = tf; i < m; i += FM_T) r0[i] = X[i].x * norm;  // re = X.x / n (:462), sample 2 i
            __threadfence_block();
            __syncthreads();
            // odd output samples: first-pass differences
            for (int b = tf; b < m; b += FM_T) X[b] = cdsub(b < 204 ? keep : Z, Z);
            __syncthreads();
            fm_forward_odd(XL, aa, tf);
            for (int i = tf; i < m; i += FM_T) X[i].x = X[i].x * norm;  // re = X.x / n (:462), sample 2 i + 1
            __syncthreads();
        }
        // ---- RxDownSample(re, re) (:461-463, :470-492): sample t of the frame = r0[t/2] (t even) or X[t/2].x / n (t odd)
        const double *Ro = reinterpret_cast<const double *>(smem) + FM_RB0;  // pruned: the odd samples, compact
        auto sample = [&](int t) -> double {
            return t < 0 ? hist[26 + t] : ((t & 1) ? (pruned ? Ro[t >> 1] : X[t >> 1].x) : r0[t >> 1]);
        };
        {
            const long long jlo = ds_first_output(t0, a.first_out, D);
            // with an even decimation (20 at 192 kHz) every window of the call ends on the same parity (t0 is even): which
            // of the 27 taps read the scratch and which the image is then known at compile time
            const bool uniform_parity = (D & 1) == 0;
            const int epar = (int)((a.first_out - t0) & 1);
            for (long long j = jlo + tf;; j += FM_T) {
                const long long te = (long long)a.first_out + (long long)D * j;
                if (te >= t0 + n || j >= a.nds) break;
                const double2 cs = a.vco_cs[j];
                const int e = (int)(te - t0);
                double fi = 0.0;
                if (pruned && (D & 3) == 0 && e >= 27) {
                    // taps of one parity read a run of 14 even samples (scratch), the others a run of 14 odd ones (LDS), both
                    // ending at a slot whose parity is the same for every window of the call (D/2 is even: D = 20): eight aligned
                    // 16-byte reads each, the run picked out of them by a shift that is the same in every lane
                    const int hi_o = epar ? (e >> 1) : (e >> 1) - 1;  // odd samples:  slots hi_o - 13 .. hi_o
                    const int hi_e = epar ? ((e - 1) >> 1) : (e >> 1);  // even samples: slots hi_e - 13 .. hi_e
                    const int bo = (hi_o - 13) & ~1, be = (hi_e - 13) & ~1;
                    const bool sho = ((hi_o - 13) & 1) != 0, she = ((hi_e - 13) & 1) != 0;
                    const double2 *po = reinterpret_cast<const double2 *>(Ro + bo);
                    const double2 *pe = reinterpret_cast<const double2 *>(r0 + be);
                    double dod[16], dev[16];
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const double2 u = pe[i];
                        dev[2 * i] = u.x;
                        dev[2 * i + 1] = u.y;
                    }
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const double2 u = po[i];
                        dod[2 * i] = u.x;
                        dod[2 * i + 1] = u.y;
                    }
                    // sample q slots below the run's end: d[13 - q + shift]
                    if (epar) {
#pragma unroll
                        for (int k = 0; k < 27; k++) {
                            const int q = k >> 1;
                            const double x = (k & 1) ? (she ? dev[14 - q] : dev[13 - q]) : (sho ? dod[14 - q] : dod[13 - q]);
                            fi += x * ds_tap(k);  // newest first (:479-483)
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < 27; k++) {
                            const int q = (k & 1) ? ((k + 1) >> 1) - 1 : (k >> 1);
                            const double x = (k & 1) ? (sho ? dod[14 - q] : dod[13 - q]) : (she ? dev[14 - q] : dev[13 - q]);
                            fi += x * ds_tap(k);
                        }
                    }
                } else if (!pruned && uniform_parity && e >= 26) {
                    if (epar) {  // e odd: taps 0,2,.. read odd samples (image), taps 1,3,.. even ones (scratch)
                        const double2 *xo = X + (e >> 1);
                        const double *re = r0 + ((e - 1) >> 1);
#pragma unroll
                        for (int k = 0; k < 27; k++) fi += ((k & 1) ? re[-(k >> 1)] : xo[-(k >> 1)].x) * ds_tap(k);
                    } else {     // e even: taps 0,2,.. read even samples (scratch), taps 1,3,.. odd ones (image)
                        const double *re = r0 + (e >> 1);
                        const double2 *xo = X + ((e - 1) >> 1);
#pragma unroll
                        for (int k = 0; k < 27; k++) fi += ((k & 1) ? xo[-(k >> 1)].x : re[-(k >> 1)]) * ds_tap(k);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 27; k++) fi += sample(e - k) * ds_tap(k);  // newest first (:479-483)
                }
                const double o = fi * ACQ_HOWARD;
                __builtin_nontemporal_store(o * cs.x, &dm[64 + j].x);  // :515-516 (written once, read by the next kernel)
                __builtin_nontemporal_store(o * cs.y, &dm[64 + j].y);
            }
        }
        double hnew = 0.0;
        if (tf < 26) hnew = sample(n - 26 + tf);
        __syncthreads();
        if (tf < 26) hist[tf] = hnew;
        __syncthreads();
    }
    if (tid < 26) sp->hist[tid] = hist[tid];
    if (tid == 0) {
        acq_state_store(sp, avePeakPower, aveCentreBin, centreBin);
    }
}

// (dynamic LDS, as the kernel's top carves it up: the image [m] double2, hist [64] and redv [16] doubles, redi [16] ints, the
//  gathered bins zb [204] double2, 64 spare bytes)
static size_t fft2x_lds_bytes(int n)
{
    return sizeof(double2) * (size_t)(n / 2) + sizeof(double) * (64 + 16) + sizeof(int) * 16 + sizeof(double2) * 204 + 64;
}

int launch_front_fft2x(const FftFrontArgs &a, const FftPlan &pl, double2 *ek, double *r0, int nstreams, hipStream_t st)
{
    JSDR_REQUIRE(pl.kind == FRONT_FFT2X && pl.n == a.n, "launch_front_fft2x: the plan is not a 2 m one of %d samples", a.n);
    Fft2xArgs aa;
    aa.sub = pl.args;
    aa.sub.f = a;
    aa.sub.f.n = a.n / 2;
    aa.n = a.n;
    memcpy(aa.tw1_off, pl.tw1_off, sizeof(aa.tw1_off));
    aa.ek = ek;
    aa.r0 = r0;
    aa.ek_stride = (long long)fft2x_scratch_ek(a.n);
    aa.r0_stride = (long long)fft2x_scratch_r0(a.n);
    const size_t lds = fft2x_lds_bytes(a.n);
    if (a.rawf) {
        JSDR_LDS_ATTR(k_front_fft2x<true>, lds);
        hipLaunchKernelGGL(k_front_fft2x<true>, dim3((unsigned)nstreams), dim3(FM_T), lds, st, aa);
    } else {
        JSDR_LDS_ATTR(k_front_fft2x<false>, lds);
        hipLaunchKernelGGL(k_front_fft2x<false>, dim3((unsigned)nstreams), dim3(FM_T), lds, st, aa);
    }
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
