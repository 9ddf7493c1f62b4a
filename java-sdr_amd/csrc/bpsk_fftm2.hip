// bpsk_fftm2.hip -- the mixed-radix FFT-acquire front end (bpsk_fftm.hip) for the 4800- and 4410-sample frames, two frames of a
// stream at once: k_front_fftm2, on the passes of bpsk_fftm_dev.h.  Compiled with -ffp-contract=off.
#include "bpsk_fftm_dev.h"

namespace jsdr {

// ================================================================================== two frames of a stream at once (round 6)
// n = 4800 (the reference's default frame at 48 kHz) ran 30 % slower per sample than n = 9600: the same passes with half the work
// items -- a pass pair of one frame has 300 or 320 items for 768 threads -- and the same ~900-tick LDS round trip each.  Here a
// workgroup takes frames f and f + 1 of its stream TOGETHER: two images side by side in LDS (2 x 76.8 KB; the tables beyond the
// first 276 entries come from L2 as the 9600 frame's do), every pass over both (the NIMG forms of bpsk_fftm_dev.h), |X| / boxcar / argmax for
// both, then the centre-bin rule (:444-453) for f and, with its result, for f + 1 -- the only sequential step -- the inverse
// halves with each frame's own centre bin, and RxDownSample: frame f + 1's windows reach back into frame f's samples, which lie in
// the first image.  A call's odd last frame runs as a pair whose second half is computed and dropped.  Same operations on the same
// operands per frame as k_front_fftm.
// (This kernel states the frame stages itself and not through bpsk_fft.h / bpsk_acq_rule.h: on the shared ones its 4800 form
//  ran 7.7 % slower at unchanged resources, profiles/acq_stages_ab.md.)
template <int NN, bool F32IN>
__global__ __launch_bounds__(FM_T) void k_front_fftm2(FftmArgs aa)
{
    static_assert(NN == 4800 || NN == 4410, "frames of 4800 samples (48 kHz) or 4410 (44.1 kHz: passes [2,3] [3,5] [7] [7])");
    extern __shared__ __align__(16) unsigned char smem[];
    const FftFrontArgs &a = aa.f;
    constexpr int n = NN;
    double2 *X = reinterpret_cast<double2 *>(smem);  // [2 n]
    const LdsArr XL = lds_arr(smem);
    double *hist = reinterpret_cast<double *>(X + 2 * n);    // [32]
    double *redv = hist + 32;                                // [2][16] per-image, per-wave best value
    int *redi = reinterpret_cast<int *>(redv + 32);          // [2][16]
    double2 *twL = reinterpret_cast<double2 *>(redi + 32);   // [lds_tw]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < aa.lds_tw; i += FM_T) twL[i] = aa.f.tw[i];
    const int s = blockIdx.x;
    const int beg = a.do_up ? n / 4 : 0;
    const int end = a.do_up ? n / 2 : n / 4;
    const int pbase = beg + 24;
    const int abase = beg + 74;
    constexpr int POFF = 2 * (NN / 2 + 104);  // |X| over [beg + 24, end - 24) in the dead upper part of each image (double slots)
    constexpr int AOFF = POFF + (NN / 4 - 48);
    FftFrontState *sp = &a.st[s];
    if (tid < 26) hist[tid] = sp->hist[tid];
    double avePeakPower = sp->avePeakPower, aveCentreBin = sp->aveCentreBin;
    int centreBin = sp->centreBin;
    const double CFREQ_INV = (double)(1.0F - (2.0F / (1 + 1))), CFREQ_AVG = (double)(2.0F / (1 + 1));
    const double PSD_INV = (double)(1.0F - (2.0F / (10 + 1))), PSD_AVG = (double)(2.0F / (10 + 1));
    const double HOWARD = 0.9 * 32768.0;
    const int D = a.decim;
    const double norm = 1.0 / (double)n;
    const int *__restrict__ raw = a.raw + (long long)s * a.stride_pairs;
    const float2 *__restrict__ rawf = a.rawf + (long long)s * a.stride_pairs;
    double2 *dm = a.dm + (long long)s * a.dm_stride;
    const GblArr g = gbl_arr(a.tw);
    // diagnostics (JSDR_FFT_PHASECLK=1): thread 0 of stream 0 accumulates the clock ticks of every phase (k_front_fftm's slots)
    long long *clk = reinterpret_cast<long long *>(twL + aa.lds_tw);  // the 64 spare bytes behind the tables
    long long tprev = 0;
    const bool timing = a.phase_clk != nullptr && s == 0 && tid == 0;
    if (timing)
        for (int k = 0; k < 8; k++) clk[k] = 0;
#define PHASE(k)                                     \
    if (timing) {                                    \
        const long long now_ = (long long)clock64(); \
        clk[k] += now_ - tprev;                      \
        tprev = now_;                                \
    }
    __syncthreads();
    if (timing) tprev = (long long)clock64();
    // the next pair's samples are requested at the top of RxDownSample and found in registers here (see fm_first2_request)
    FmRaw16 pre;
    auto request = [&](long long t0q, bool two_q, int t_) {
        if constexpr (NN == 4800) {
            fm_first_request2<NN, F32IN>(pre, raw + t0q, rawf + t0q, two_q ? NN : 0, t_);
        } else {
            constexpr int NLD = (2 * NN + FM_T - 1) / FM_T;
            static_assert(NLD <= 16, "sixteen samples a thread");
#pragma unroll
            for (int q = 0; q < NLD; q++) {
                int t = t_ + q * FM_T;
                t = t < 2 * NN ? t : 2 * NN - 1;
                if (!two_q && t >= NN) t -= NN;  // (a single last frame: the second image is a copy)
                if (F32IN)
                    pre.wf[q] = reinterpret_cast<const f2v *>(rawf)[t0q + t];
                else
                    pre.w[q] = raw[t0q + t];
            }
        }
    };
    request(0, a.nframes >= 2, tid);

    for (int f = 0; f < a.nframes; f += 2) {
        const bool two = f + 1 < a.nframes;
        int tf = tid;
        asm volatile("" : "+v"(tf));  // (opaque per iteration: see k_front_fftm)
        const long long t0 = (long long)f * n;  // call-relative index of frame f's first sample
        // ---- both frames -> images (:416-421), forward transform (:422-423), the last pass for the bins below end + 102 only
        if constexpr (NN == 4800) {
            fm_first_from_regs2<NN, F32IN>(XL, pre, a.ic, a.qc, tf);  // (with the first pass; a single last frame comes twice)
            const LdsArr t = lds_arr(twL);
            fm_pass2<4, 4, NN, 4, false, LdsArr, LdsArr, 2>(XL, t + 4, t + 20, NN, 4, 0u, tf);
            fm_pass2<3, 5, NN, 64, false, LdsArr, GblArr, 2>(XL, t + 84, g + 276, NN, 64, 0u, tf);
            fm_pass5_band<NN, 960, false, GblArr, 2>(XL, g + 1236, end + 102, tf);
        } else {
            // natural order; frame f + 1 follows frame f in memory as image 1 follows image 0
            constexpr int NLD = (2 * NN + FM_T - 1) / FM_T;
#pragma unroll
            for (int q = 0; q < NLD; q++) {
                const int t = tf + q * FM_T;
                if (t < 2 * n) {
                    double di, dq;
                    if (F32IN) {
                        di = (double)pre.wf[q].x;
                        dq = (double)pre.wf[q].y;
                    } else {
                        di = (double)i16_to_float_java(java_short_add((int)(short)(pre.w[q] & 0xffff), a.ic));
                        dq = (double)i16_to_float_java(java_short_add(pre.w[q] >> 16, a.qc));
                    }
                    X[t] = make_double2(di, dq);
                }
            }
            __syncthreads();
            const LdsArr t = lds_arr(twL);
            fm_pass2<2, 3, NN, 1, false, LdsArr, LdsArr, 2>(XL, t, t + 2, NN, 1, 0u, tf);
            fm_pass2<3, 5, NN, 6, false, LdsArr, LdsArr, 2>(XL, t + 8, t + 26, NN, 6, 0u, tf);
            fm_pass<7, NN, 90, LdsArr, 2>(XL, t + 116, NN, 90, 0u, tf);
            fm_passr_band<7, NN, 630, GblArr, 2>(XL, g + 746, end + 102, tf);
        }
        PHASE(1)  // (with the load: the first pass comes straight from the samples)
        // ---- |X| (:425-427) over the band the boxcar reads, both images
        {
            const int cnt = end - 24 - pbase;
            for (int u = tf; u < 2 * cnt; u += FM_T) {
                const int img = u >= cnt ? 1 : 0;
                const int i = pbase + (u - img * cnt);
                const double2 v = X[img * n + i];
                reinterpret_cast<double *>(X + img * n)[POFF + (i - pbase)] = sqrt(v.x * v.x + v.y * v.y);
            }
        }
        __syncthreads();
        PHASE(6)
        // ---- boxcar + first maximum per image (:433-442): a thread's items of one image ascend
        double bestv[2] = {0.0, 0.0};
        int besti[2] = {-1, -1};
        {
            const int npair = (end - 75 - (beg + 74) + 1) / 2;
            for (int u = tf; u < 2 * npair; u += FM_T) {
                const int img = u >= npair ? 1 : 0;
                const int i = beg + 74 + 2 * (u - img * npair);
                double *Pi = reinterpret_cast<double *>(X + img * n) + POFF;
                double *Ai = reinterpret_cast<double *>(X + img * n) + AOFF;
                const double2 *w = reinterpret_cast<const double2 *>(Pi + (i - 50 - pbase));
                double a0, a1;
                boxcar_pair(w, a0, a1);
                asm volatile("" : "+v"(a0), "+v"(a1));
                double bv = img ? bestv[1] : bestv[0];
                int bi = img ? besti[1] : besti[0];
                if (i >= beg + 75) {
                    Ai[i - abase] = a0;
                    if (bv < a0) {
                        bv = a0;
                        bi = i;
                    }
                }
                if (i + 1 < end - 75) {
                    Ai[i + 1 - abase] = a1;
                    if (bv < a1) {
                        bv = a1;
                        bi = i + 1;
                    }
                }
                if (img) {
                    bestv[1] = bv;
                    besti[1] = bi;
                } else {
                    bestv[0] = bv;
                    besti[0] = bi;
                }
            }
        }
#pragma unroll
        for (int im = 0; im < 2; im++) {
            wave_first_max(bestv[im], besti[im]);
            if (lane == 0) {
                redv[im * 16 + wave] = bestv[im];
                redi[im * 16 + wave] = besti[im];
            }
        }
        __syncthreads();
        PHASE(7)
        // ---- centre-bin rule (:444-453) for frame f, then for frame f + 1, by every thread on the same values
        int cb[2];
#pragma unroll
        for (int im = 0; im < 2; im++) {
            double mv = 0.0;
            int mi = -1;
            if (lane < FM_T / 64) {
                mv = redv[im * 16 + lane];
                mi = redi[im * 16 + lane];
            }
            wave_first_max(mv, mi);
            const double maxBin = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(mv)),
                                                   __builtin_amdgcn_readfirstlane(__double2loint(mv)));
            const int binPos = __builtin_amdgcn_readfirstlane(mi);
            if (im == 0 || two) {
                if (centreBin < 0) centreBin = 0;
                if (centreBin > end - 1) centreBin = end - 1;
                const double *Ai = reinterpret_cast<const double *>(X + im * n) + AOFF;
                const double atc = (centreBin >= beg + 75 && centreBin < end - 75) ? Ai[centreBin - abase] : 0.0;
                avePeakPower = (PSD_AVG * atc) + (PSD_INV * avePeakPower);
                if (maxBin > (avePeakPower / 4) * 5 && binPos > 0) {
                    aveCentreBin = (CFREQ_AVG * (double)(float)binPos) + (CFREQ_INV * aveCentreBin);
                    centreBin = (int)(aveCentreBin + (double)1.0F);
                }
                if (centreBin < 102) centreBin = 102;
            }
            cb[im] = centreBin;
        }
        PHASE(2)
        // ---- 204 bins around each frame's centre to bin 0 of a zeroed array (:458), inverse transform (:459): passes 1-3 from the
        // bins, [3, 5], the last pass real parts only, scaled, compact
        if constexpr (NN == 4800) {
            const LdsArr t64 = lds_arr(twL) + 20;
            fm_inv_blocks<NN, true, LdsArr, LdsArr, 2>(XL, XL + (cb[0] - 102), t64, 1, t64, 2, tf, n + cb[1] - cb[0]);
            fm_pass2<3, 5, NN, 64, false, LdsArr, GblArr, 2>(XL, lds_arr(twL) + 84, g + 276, NN, 64, 0u, tf);
            fm_pass5_real<NN, 960, false, 1, GblArr, 2>(XL, g + 1236, norm, tf, hist);
        } else {
            const LdsArr t = lds_arr(twL);
            fm_inv_pair_from_bins<2, 3, NN, LdsArr, 2>(XL, XL + (cb[0] - 102), t + 2, tf, n + cb[1] - cb[0]);
            fm_pass2<3, 5, NN, 6, false, LdsArr, LdsArr, 2>(XL, t + 8, t + 26, NN, 6, 0u, tf);
            fm_pass<7, NN, 90, LdsArr, 2>(XL, t + 116, NN, 90, 0u, tf);
            fm_passr_real<7, NN, 630, 1, GblArr, 2>(XL, g + 746, norm, tf, hist);
        }
        PHASE(4)
        double *Rb0 = reinterpret_cast<double *>(smem);
        double *Rb1 = Rb0 + 2 * n;
        // (frame f + 1's windows reach back into frame f's last 26 samples)
        if (tf < 26) Rb1[FM_RB0 - 26 + tf] = Rb0[FM_RB0 + n - 26 + tf];
        __syncthreads();
        // ---- RxDownSample(re, re) (:461-463, :470-492) from the compact samples of frame f, then of frame f + 1
        {
            // (the last pair asks for itself again: a request under a branch would make every later wait the minimum over both paths)
            const bool more = f + 2 < a.nframes;
            request(more ? t0 + 2 * (long long)n : t0, more ? f + 3 < a.nframes : two, tf);
        }
#pragma unroll
        for (int im = 0; im < 2; im++) {
            if (im == 1 && !two) break;
            const double *Rb = im ? Rb1 : Rb0;
            const long long tq = t0 + (long long)im * n;
            long long jlo = (tq - a.first_out + D - 1) / D;
            if (tq <= a.first_out) jlo = 0;
            const bool even_d = (D & 1) == 0;
            const int par = (int)((a.first_out - tq) & 1);
            for (long long j = jlo + tf;; j += FM_T) {
                const long long te = (long long)a.first_out + (long long)D * j;  // window end, call-relative
                if (te >= tq + n || j >= a.nds) break;
                const double2 cs = a.vco_cs[j];
                const int e = (int)(te - tq);
                double fi = 0.0;
                if (even_d) {
                    const double2 *w2 = reinterpret_cast<const double2 *>(Rb + ((e + FM_RB0 - 26) & ~1));
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
                    const double *w = Rb + (FM_RB0 + e);
#pragma unroll
                    for (int k = 0; k < 27; k++) fi += w[-k] * ds_tap(k);
                }
                const double o = fi * HOWARD;
                dm[64 + j] = make_double2(o * cs.x, o * cs.y);  // :515-516
            }
        }
        if (tf < 26) hist[tf] = (two ? Rb1 : Rb0)[FM_RB0 + n - 26 + tf];
        __syncthreads();
        PHASE(5)
    }
#undef PHASE
    if (tid < 26) sp->hist[tid] = hist[tid];
    if (tid == 0) {
        sp->avePeakPower = avePeakPower;
        sp->aveCentreBin = aveCentreBin;
        sp->centreBin = centreBin;
        if (timing)
            for (int k = 0; k < 8; k++) a.phase_clk[k] = clk[k];
    }
}

// (dynamic LDS: fm2_lds_fixed(n), the layout carved up at the kernel's top, and the lds_tw table entries behind redi: the tables
//  of all passes but the last -- 4800: but the last two -- stay in LDS, the rest come from L2)
int launch_front_fftm2(const FftFrontArgs &a, const FftPlan &pl, int nstreams, hipStream_t st)
{
    JSDR_REQUIRE(pl.kind == FRONT_FFTM && pl.n == a.n && (a.n == 4800 || a.n == 4410), "launch_front_fftm2: frame of %d samples", a.n);
    FftmArgs aa = pl.args;
    aa.f = a;
    aa.lds_tw = pl.lds_tw_pair;
    const size_t lds2 = fm2_lds_fixed(a.n) + sizeof(double2) * (size_t)aa.lds_tw;
    const bool f32 = a.rawf != nullptr;
#define FM_LAUNCH2(NN, F32)                                                                                   \
    do {                                                                                                      \
        JSDR_LDS_ATTR((k_front_fftm2<NN, F32>), lds2);                                                        \
        hipLaunchKernelGGL((k_front_fftm2<NN, F32>), dim3((unsigned)nstreams), dim3(FM_T), lds2, st, aa);     \
    } while (0)
    if (a.n == 4800) {
        if (f32)
            FM_LAUNCH2(4800, true);
        else
            FM_LAUNCH2(4800, false);
    } else {
        if (f32)
            FM_LAUNCH2(4410, true);
        else
            FM_LAUNCH2(4410, false);
    }
#undef FM_LAUNCH2
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
