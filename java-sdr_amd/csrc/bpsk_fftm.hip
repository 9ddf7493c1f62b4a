// bpsk_fftm.hip -- FUNcubeBPSKDemod FFT-acquire front end (doBufferFFT, FUNcubeBPSKDemod.java:406-464) for frames
// that are NOT a power of two: n = 2^a 3^b 5^c up to 9600, i.e. the reference's own default frame
// (blen = rate*size/10 => n = 9600 at 96 kHz, 4800 at 48 kHz; JavaAudio.java:58-59).
//
// Compiled with -ffp-contract=off.  The transform is the oracle's mixed-radix definition (oracle/o_fft.c,
// fft_f64_mixed), pass by pass through bpsk_fftm_dev.h on the plan and the tables of bpsk_fftplan.hip -- so centre bins,
// traces, bits and FEC bytes are bit-identical to the oracle.  JTransforms' own rounding is unknowable (source absent): parity
// with the Java library itself is unpinned.
//
// MI355X mapping: one 768-thread workgroup per stream, persistent over the frames of the call (the centre-bin
// state is sequential).  The frame lives in LDS as double2[n] (153.6 KB at n = 9600: one workgroup per CU); a
// pass loads every butterfly into registers (<= 24 double2 per thread; 1024 threads would cap a thread at 128
// VGPRs and spill), barrier, stores to the autosort positions -- in place, no second image.  |X| and the boxcar sums of the searched quarter band reuse the dead
// upper part of the image.  The rest (boxcar, first maximum, centre-bin rule, 204 bins to bin 0, RxDownSample,
// VCO) is k_front_fft's, with run-time sizes.
//
// This unit holds the kernels of ONE image in the fm_lds_fixed layout: k_front_fftm, one frame at a time, and the same frame loop
// in three phases (k_acqm_fwd / k_acqm_inv, below).  They share a unit for a measured reason: compiled without k_front_fftm beside
// it, k_acqm_inv comes out as other machine code (profiles/fftplan_ab.md).  Its siblings on the same passes: bpsk_fftm2.hip (two
// frames of a stream at once), bpsk_fft2x.hip (frames of 2 m samples).
#include "bpsk_fftm_dev.h"

namespace jsdr {

template <bool F32IN>
__global__ __launch_bounds__(FM_T) void k_front_fftm(FftmArgs aa)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const FftFrontArgs &a = aa.f;
    const int n = a.n;
    double2 *X = reinterpret_cast<double2 *>(smem);      // [n]
    const LdsArr XL = lds_arr(smem);                     // the same image for the passes (typed view)
    // [32]; during RxDownSample slots 26..51 (over the argmax scratch behind it, dead by then) hold the frame's first 26
    // scaled samples, so that a window reaching back into the previous frame is one contiguous run as well
    double *hist = reinterpret_cast<double *>(X + n);
    double *redv = hist + 32;                            // [16] per-wave best value
    int *redi = reinterpret_cast<int *>(redv + 16);      // [16] per-wave best index
    double2 *twL = reinterpret_cast<double2 *>(redi + 16);  // [lds_tw] twiddle tables of the first passes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < aa.lds_tw; i += FM_T) twL[i] = aa.f.tw[i];
    const int s = blockIdx.x;
    const int beg = acq_band_beg(n, a.do_up), end = acq_band_end(n, a.do_up);
    // |X| over [beg+24, end-24) and the boxcar sums over [beg+74, end-74) live in the upper part of the image, dead
    // after the forward transform (bins up to n/2+101 are still gathered below); beg is a multiple of 4
    const int pbase = beg + 24;
    double *P = reinterpret_cast<double *>(X + (n / 2 + 104));
    double *A = P + (n / 4 - 48);
    const int abase = beg + 74;
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
    // diagnostics (JSDR_FFT_PHASECLK=1): thread 0 of stream 0 accumulates the clock ticks of every phase
    long long *clk = reinterpret_cast<long long *>(twL + aa.lds_tw);  // the 64 spare bytes behind the tables
    long long tprev = 0;
    const bool timing = a.phase_clk != nullptr && s == 0 && tid == 0;
    if (timing)
        for (int k = 0; k < 8; k++) clk[k] = 0;
    __syncthreads();
    if (timing) tprev = (long long)clock64();
    FmRaw16 pre;  // n = 9600: the next frame's samples, requested during RxDownSample
    if (n == 9600) fm_first2_request<9600, F32IN>(pre, raw, rawf, tid);

    for (int f = 0; f < a.nframes; f++) {
        const long long t0 = (long long)f * n;  // call-relative index of the frame's first sample
        // opaque per frame: nothing derived from the thread index is loop invariant, or LLVM hoists every address
        // of every phase out of the frame loop and spills them (the same trap as in k_front_fft)
        int tf = tid;
        asm volatile("" : "+v"(tf));
        const bool fused_first = (n == 9600 || n == 4800);
        const bool compact = fused_first || n == 4410;  // the inverse from the bins, compact real samples, windows as aligned runs
        if (n == 9600) {
            fm_first2_from_regs<9600, F32IN>(XL, pre, a.ic, a.qc, lds_arr(twL) + 4, tf);
        } else if (n == 4800) {
            fm_first_from_raw<4800, F32IN>(XL, raw + t0, rawf + t0, a.ic, a.qc, tf);
        } else {
            // ---- frame -> LDS, natural order (:416-421)
            {
                // all of a thread's samples in flight before the first conversion (a load / convert / store loop pays the
                // HBM latency once per sample: 13 times per frame)
                constexpr int NLD = (FM_NMAX + FM_T - 1) / FM_T;
                int w[NLD];
                float2 wf[NLD];
#pragma unroll
                for (int q = 0; q < NLD; q++) {
                    int t = tf + q * FM_T;
                    t = t < n ? t : n - 1;
                    if (F32IN)
                        wf[q] = rawf[t0 + t];
                    else
                        w[q] = raw[t0 + t];
                }
#pragma unroll
                for (int q = 0; q < NLD; q++) {
                    const int t = tf + q * FM_T;
                    if (t < n) {
                        X[t] = F32IN ? acq_sample(wf[q]) : acq_sample(w[q], a.ic, a.qc);
                    }
                }
            }
            __syncthreads();
        }
        ACQ_PHASE(clk, 0)
        fm_forward<true>(XL, twL, aa, tf, fused_first, compact ? FM_FWD_BAND : FM_FULL, end + 102);  // :422-423; bins < end + 102 are read
        ACQ_PHASE(clk, 1)
        // ---- |X| (:425-427) over the band the boxcar reads
        for (int i = pbase + tf; i < end - 24; i += FM_T) {
            const double2 v = X[i];
            P[i - pbase] = sqrt(v.x * v.x + v.y * v.y);
        }
        __syncthreads();
        ACQ_PHASE(clk, 6)
        // ---- 100-wide boxcar, summed j ascending for every i (:433-437); first maximum (:439-442).  A thread owns
        // the outputs i (even) and i+1: both windows come out of the same 51 aligned 16-byte reads.
        double bestv = 0.0;  // maxBin starts at 0.0, binPos at -1
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
        ACQ_PHASE(clk, 7)
        // ---- centre-bin rule (:444-453), evaluated by every thread on the same values
        {
            double maxBin;
            int binPos;
            wg_first_max<FM_T / 64>(redv, redi, lane, maxBin, binPos);
            centreBin = centre_bin_clamp(centreBin, end);
            const double atc = acq_band_filled(centreBin, beg, end) ? A[centreBin - abase] : 0.0;
            centre_bin_step(avePeakPower, aveCentreBin, centreBin, atc, maxBin, binPos);
        }
        ACQ_PHASE(clk, 2)
        // ---- 204 bins around the centre to bin 0 of a zeroed array (:458), inverse transform (:459) as
        // conj o forward o conj; only real parts are read afterwards, so the closing conjugation is dropped
        if (compact) {
            // default frames: passes 1-3 straight from the bins, last pass real parts only and already scaled by 1/n
            const LdsArr t64 = lds_arr(twL) + 20;  // the 64-entry table of pass 3
            if (n == 9600)
                fm_inv_blocks128_9600<true>(XL, XL + (centreBin - 102), t64, lds_arr(twL) + 84, tf);
            else if (n == 4800)
                fm_inv_blocks<4800, true>(XL, XL + (centreBin - 102), t64, 1, t64, 2, tf);
            else
                fm_inv_pair_from_bins<2, 3, 4410>(XL, XL + (centreBin - 102), lds_arr(twL) + 2, tf);  // 4410: the first pair
            ACQ_PHASE(clk, 3)
            fm_forward<true>(XL, twL, aa, tf, true, FM_INV_REAL, 0, norm, hist);
            ACQ_PHASE(clk, 4)
            // ---- RxDownSample(re, re) (:461-463, :470-492) from the compact samples: sample t of the frame at double slot
            // FM_RB0 + t, the previous frame's last 26 in front of them -- every window is one contiguous run
            {
                // (the last frame asks for itself again: a request under a branch would make every later wait the minimum over both paths)
                if (n == 9600) fm_first2_request<9600, F32IN>(pre, raw + (f + 1 < a.nframes ? t0 + n : t0), rawf + (f + 1 < a.nframes ? t0 + n : t0), tf);
                const double *Rb = reinterpret_cast<const double *>(smem);
                const long long jlo = ds_first_output(t0, a.first_out, D);
                const bool even_d = (D & 1) == 0;                 // then every window of the call ends on the same parity (n is even)
                const int par = (int)((a.first_out - t0) & 1);
                for (long long j = jlo + tf;; j += FM_T) {
                    const long long te = (long long)a.first_out + (long long)D * j;  // window end, call-relative
                    if (te >= t0 + n || j >= a.nds) break;
                    const double2 cs = a.vco_cs[j];
                    const int e = (int)(te - t0);  // 0..n-1 within the frame
                    const double fi = ds_window_compact(Rb, FM_RB0, e, even_d, par);
                    const double o = fi * ACQ_HOWARD;  // fi == fq: both rails get the same samples
                    dm[64 + j] = make_double2(o * cs.x, o * cs.y);  // :515-516
                }
                if (tf < 26) hist[tf] = Rb[FM_RB0 + n - 26 + tf];  // (nobody reads hist[] before the next frame's last pass)
                __syncthreads();  // every window is read before the next frame's first pass overwrites the image
            }
            ACQ_PHASE(clk, 5)
            continue;
        } else {
            double2 keep = make_double2(0.0, 0.0);
            if (tf < 204) keep = X[centreBin - 102 + tf];
            __syncthreads();
            for (int i = tf; i < n; i += FM_T) X[i] = make_double2(0.0, -0.0);  // conj of the zeroed array: -0.0 imaginary parts
            __syncthreads();
            if (tf < 204) X[tf] = make_double2(keep.x, -keep.y);
            __syncthreads();
            ACQ_PHASE(clk, 3)
            fm_forward<true>(XL, twL, aa, tf, false);
            for (int i = tf; i < n; i += FM_T) X[i].x = X[i].x * norm;  // re = X.x / n (:462)
            __syncthreads();
        }
        ACQ_PHASE(clk, 4)
        if (tf < 26) hist[26 + tf] = X[tf].x;
        __syncthreads();
        // ---- RxDownSample(re, re) (:461-463, :470-492): outputs whose window ends inside this frame
        {
            const long long jlo = ds_first_output(t0, a.first_out, D);
            for (long long j = jlo + tf;; j += FM_T) {
                const long long te = (long long)a.first_out + (long long)D * j;  // window end, call-relative
                if (te >= t0 + n || j >= a.nds) break;
                const double2 cs = a.vco_cs[j];
                const int e = (int)(te - t0);  // 0..n-1 within the frame
                // all but the first three windows of a frame: no history, constant offsets; those three: history, then the head of the frame
                const double fi = e >= 26 ? ds_window(X + e) : ds_window(hist + 26 + e);
                const double o = fi * ACQ_HOWARD;  // fi == fq: both rails get the same samples
                dm[64 + j] = make_double2(o * cs.x, o * cs.y);  // :515-516
            }
        }
        double hnew = 0.0;
        if (tf < 26) hnew = X[n - 26 + tf].x;
        __syncthreads();
        if (tf < 26) hist[tf] = hnew;
        __syncthreads();
        ACQ_PHASE(clk, 5)
    }
    if (tid < 26) sp->hist[tid] = hist[tid];
    if (tid == 0) {
        acq_state_store(sp, avePeakPower, aveCentreBin, centreBin);
        if (timing)
            for (int k = 0; k < 8; k++) a.phase_clk[k] = clk[k];
    }
}

// (dynamic LDS: fm_lds_fixed(n), the layout carved up at the kernel's top, and the lds_tw table entries behind redi)
int launch_front_fftm(const FftFrontArgs &a, const FftPlan &pl, double2 *gscratch, int nstreams, hipStream_t st)
{
    if (fftm_pairs(a.n, a.nframes)) return launch_front_fftm2(a, pl, nstreams, st);
    JSDR_REQUIRE(pl.kind == FRONT_FFTM && pl.n == a.n, "launch_front_fftm: the plan is not a mixed-radix one of %d samples", a.n);
    JSDR_REQUIRE(gscratch || pl.wr_off[pl.np - 1] == 0, "launch_front_fftm: a radix-%d pass without its scratch", pl.rad[pl.np - 1]);  // (a prime radix above 7 is the last)
    FftmArgs aa = pl.args;
    aa.f = a;
    aa.gscratch = gscratch;
    aa.gscratch_stride = a.n;
    const size_t lds = fm_lds_fixed(a.n) + sizeof(double2) * (size_t)aa.lds_tw;
    if (a.rawf) {
        JSDR_LDS_ATTR(k_front_fftm<true>, lds);
        hipLaunchKernelGGL(k_front_fftm<true>, dim3((unsigned)nstreams), dim3(FM_T), lds, st, aa);
    } else {
        JSDR_LDS_ATTR(k_front_fftm<false>, lds);
        hipLaunchKernelGGL(k_front_fftm<false>, dim3((unsigned)nstreams), dim3(FM_T), lds, st, aa);
    }
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

// ================================================================================== the default frames in three phases (round 6)
// k_front_fftm's frame loop cut where the reference's loop carries nothing (bpsk_acq.hip has the whole story): k_acqm_fwd is
// its forward half for ONE (stream, frame) -- transform, |X|, boxcar, first maximum -- and leaves what the scan (k_acq_scan) and
// the inverse half need; k_acqm_inv gathers the frame's 204 bins from that row, runs the inverse half and RxDownSample for the
// windows inside the frame (k_acq_edges does the ones that reach into the frame before).  Same passes, same tables, same
// image -- so a workgroup still owns a CU -- but the grid is frames: a call of few streams fills the chip (one recorded stream
// of 109 frames took 109 frame times in k_front_fftm and takes one here).  Frames of 9600 / 4800 / 4410 samples (the compact
// passes); a workgroup takes its frames one at a time from a ticket counter.
__device__ __forceinline__ long long acqm_ticket(unsigned *ctr, int *tkL, int tid)
{
    if (tid == 0) tkL[0] = (int)atomicAdd(ctr, 1u);
    __syncthreads();
    const long long g = tkL[0];
    __syncthreads();
    return g;
}

template <bool F32IN>
__global__ __launch_bounds__(FM_T) void k_acqm_fwd(FftmArgs aa, AcqArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int n = a.n;
    double2 *X = reinterpret_cast<double2 *>(smem);  // [n]
    const LdsArr XL = lds_arr(smem);
    double *hist = reinterpret_cast<double *>(X + n);  // [32] (unused here; the layout is k_front_fftm's)
    double *redv = hist + 32;                          // [16]
    int *redi = reinterpret_cast<int *>(redv + 16);    // [16]
    double2 *twL = reinterpret_cast<double2 *>(redi + 16);
    int *tkL = reinterpret_cast<int *>(twL + aa.lds_tw);  // (the 64 spare bytes behind the tables)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < aa.lds_tw; i += FM_T) twL[i] = aa.f.tw[i];
    const int beg = acq_band_beg(n, a.do_up), end = acq_band_end(n, a.do_up);
    const int pbase = beg + 24;
    double *P = reinterpret_cast<double *>(X + (n / 2 + 104));  // (the sums go straight to the frame's row in global memory)
    const long long nfr = (long long)a.S * a.F;
    __syncthreads();
    for (;;) {
        const long long g = acqm_ticket(a.tickets + 0, tkL, tid);
        if (g >= nfr) break;
        int tf = tid;
        asm volatile("" : "+v"(tf));
        const int s = (int)(g / a.F), f = (int)(g - (long long)s * a.F);
        const long long t0 = (long long)s * a.stride_pairs + (long long)(a.f0 + f) * n;
        if (n == 9600)
            fm_first2_from_raw<9600, F32IN>(XL, a.raw + t0, a.rawf + t0, a.ic, a.qc, lds_arr(twL) + 4, tf);
        else if (n == 4800)
            fm_first_from_raw<4800, F32IN>(XL, a.raw + t0, a.rawf + t0, a.ic, a.qc, tf);
        else {
            // n = 4410: the frame to LDS in natural order (:416-421), all of a thread's samples in flight before the first conversion
            constexpr int NLD = (4410 + FM_T - 1) / FM_T;
            int w[NLD];
            float2 wf[NLD];
#pragma unroll
            for (int q = 0; q < NLD; q++) {
                int t = tf + q * FM_T;
                t = t < n ? t : n - 1;
                if (F32IN)
                    wf[q] = a.rawf[t0 + t];
                else
                    w[q] = a.raw[t0 + t];
            }
#pragma unroll
            for (int q = 0; q < NLD; q++) {
                const int t = tf + q * FM_T;
                if (t < n) {
                    X[t] = F32IN ? acq_sample(wf[q]) : acq_sample(w[q], a.ic, a.qc);
                }
            }
            __syncthreads();
        }
        fm_forward<true>(XL, twL, aa, tf, n != 4410, FM_FWD_BAND, end + 102);  // :422-423; bins < end + 102 are formed
        // ---- the bins a gather can reach, to the frame's row (layout: acq_spec_index), and |X| over the band the boxcar reads
        {
            double2 *specg = a.spec + g * a.nsb;
            const int lo1 = a.do_up ? n / 4 - 26 : 0;
            for (int i = tf; i < a.nsb; i += FM_T) {
                const int b = a.do_up ? (i < 204 ? i : lo1 + (i - 204)) : i;
                specg[i] = X[b];
            }
        }
        for (int i = pbase + tf; i < end - 24; i += FM_T) {
            const double2 v = X[i];
            P[i - pbase] = sqrt(v.x * v.x + v.y * v.y);  // :425-427
        }
        __syncthreads();
        // ---- 100-wide boxcar, summed j ascending for every i (:433-437); first maximum (:439-442)
        double bestv = 0.0;
        int besti = -1;
        double *ab = a.aband + g * a.na;
        for (int i = beg + 74 + 2 * tf; i < end - 75; i += 2 * FM_T) {
            const double2 *w = reinterpret_cast<const double2 *>(P + (i - 50 - pbase));
            double a0, a1;
            boxcar_pair(w, a0, a1);
            boxcar_put(a0, a1, ab + (i - (beg + 75)), i, beg, end, bestv, besti);
        }
        wave_first_max(bestv, besti);
        if (lane == 0) {
            redv[wave] = bestv;
            redi[wave] = besti;
        }
        __syncthreads();
        if (tid == 0) {
            double mv = 0.0;
            int mi = -1;
            for (int w = 0; w < FM_T / 64; w++) first_max_merge(mv, mi, redv[w], redi[w]);
            AcqPeak pk;
            pk.maxBin = mv;
            pk.binPos = mi;
            pk.pad = 0;
            a.peak[g] = pk;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(FM_T) void k_acqm_inv(FftmArgs aa, AcqArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int n = a.n;
    double2 *X = reinterpret_cast<double2 *>(smem);
    const LdsArr XL = lds_arr(smem);
    double *hist = reinterpret_cast<double *>(X + n);  // [32]: zeros (the windows that reach before the frame are k_acq_edges')
    double *redv = hist + 32;
    int *redi = reinterpret_cast<int *>(redv + 16);
    double2 *twL = reinterpret_cast<double2 *>(redi + 16);
    int *tkL = reinterpret_cast<int *>(twL + aa.lds_tw);
    const int tid = threadIdx.x;
    for (int i = tid; i < aa.lds_tw; i += FM_T) twL[i] = aa.f.tw[i];
    if (tid < 32) hist[tid] = 0.0;
    const int D = a.decim;
    const double norm = 1.0 / (double)n;
    const int lo1 = a.do_up ? n / 4 - 26 : 0;
    const long long nfr = (long long)a.S * a.F;
    __syncthreads();
    for (;;) {
        const long long g = acqm_ticket(a.tickets + 1, tkL, tid);
        if (g >= nfr) break;
        int tf = tid;
        asm volatile("" : "+v"(tf));
        const int s = (int)(g / a.F), f = (int)(g - (long long)s * a.F);
        const long long t0 = (long long)(a.f0 + f) * n;  // call-relative index of the frame's first sample
        // ---- the 204 bins around the centre (:458) to the head of the image
        {
            const int c = a.cbin[g];
            int off = c - 102;
            if (a.do_up) off = (c == 102) ? 0 : 204 + (c - 102 - lo1);
            if (off < 0) off = 0;
            if (off + 204 > a.nsb) off = a.nsb - 204;
            const double2 *src = a.spec + g * a.nsb + off;
            if (tf < 204) X[tf] = src[tf];
        }
        __syncthreads();
        // ---- inverse transform (:459) as conj o forward o conj: the first passes straight from the bins, the last one real parts
        // only, scaled, compact (k_front_fftm's)
        {
            const LdsArr t64 = lds_arr(twL) + 20;
            if (n == 9600)
                fm_inv_blocks128_9600<true>(XL, XL, t64, lds_arr(twL) + 84, tf);
            else if (n == 4800)
                fm_inv_blocks<4800, true>(XL, XL, t64, 1, t64, 2, tf);
            else
                fm_inv_pair_from_bins<2, 3, 4410>(XL, XL, lds_arr(twL) + 2, tf);
        }
        fm_forward<true>(XL, twL, aa, tf, true, FM_INV_REAL, 0, norm, hist);
        // ---- the frame's first and last 26 samples (k_acq_edges), RxDownSample for the windows inside the frame (:461-463, :470-492)
        {
            const double *Rb = reinterpret_cast<const double *>(smem);
            if (tf < 26) {
                double *eg = a.edges + g * 52;
                eg[tf] = Rb[FM_RB0 + tf];
                eg[26 + tf] = Rb[FM_RB0 + n - 26 + tf];
            }
            const long long jlo = ds_first_output(t0, a.first_out, D);
            const bool even_d = (D & 1) == 0;
            const int par = (int)((a.first_out - t0) & 1);
            for (long long j = jlo + tf;; j += FM_T) {
                const long long te = (long long)a.first_out + (long long)D * j;  // window end, call-relative
                if (te >= t0 + n || j >= a.nds) break;
                const int e = (int)(te - t0);
                if (e < 26) continue;
                const double2 cs = a.vco_cs[j];
                const double fi = ds_window_compact(Rb, FM_RB0, e, even_d, par);
                const double o = fi * ACQ_HOWARD;
                a.dm[(long long)s * a.dm_stride + 64 + j] = make_double2(o * cs.x, o * cs.y);  // :515-516
            }
        }
        __syncthreads();
    }
}

// which 0: k_acqm_fwd, 1: k_acqm_inv
// (dynamic LDS: k_front_fftm's -- fm_lds_fixed(n), the layout carved up at the kernels' tops, and the lds_tw table entries)
int launch_acqm(const AcqArgs &a, const FftFrontArgs &fa, const FftPlan &pl, int num_cu, int which, hipStream_t st)
{
    JSDR_REQUIRE(acqm_supported(a.n) && pl.kind == FRONT_FFTM && pl.n == a.n, "launch_acqm: frame of %d samples", a.n);
    FftmArgs aa = pl.args;
    aa.f = fa;
    const size_t lds = fm_lds_fixed(a.n) + sizeof(double2) * (size_t)aa.lds_tw;
    const long long nfr = (long long)a.S * a.F;
    const int per_cu = lds > 80 * 1024 ? 1 : 2;
    long long grid = (long long)per_cu * num_cu;
    if (grid > nfr) grid = nfr;
    if (which == 0) {
        if (fa.rawf) {
            JSDR_LDS_ATTR(k_acqm_fwd<true>, lds);
            hipLaunchKernelGGL(k_acqm_fwd<true>, dim3((unsigned)grid), dim3(FM_T), lds, st, aa, a);
        } else {
            JSDR_LDS_ATTR(k_acqm_fwd<false>, lds);
            hipLaunchKernelGGL(k_acqm_fwd<false>, dim3((unsigned)grid), dim3(FM_T), lds, st, aa, a);
        }
    } else {
        JSDR_LDS_ATTR(k_acqm_inv, lds);
        hipLaunchKernelGGL(k_acqm_inv, dim3((unsigned)grid), dim3(FM_T), lds, st, aa, a);
    }
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
