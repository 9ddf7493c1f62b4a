// bpsk_handle.hip -- the jsdr_bpsk handle's lifecycle: the tap tables, FFT-acquire set-up, jsdr_bpsk_create and every
// jsdr_bpsk_create_*, jsdr_bpsk_destroy, the knobs.  Host code only; the struct and the other host units: bpsk_handle.h.
#include "bpsk_handle.h"
#include <math.h>
#include <cmath>
#include <stdlib.h>

// FUNcubeBPSKDemod.java:27-55, float literals widened (symmetric, first 14)
static const float h_ds_half[14] = {-6.103515625000e-004F, -1.220703125000e-004F, +2.380371093750e-003F,
                                    +6.164550781250e-003F, +7.324218750000e-003F, +7.629394531250e-004F,
                                    -1.464843750000e-002F, -3.112792968750e-002F, -3.225708007813e-002F,
                                    -1.617431640625e-003F, +6.463623046875e-002F, +1.502380371094e-001F,
                                    +2.231445312500e-001F, +2.518310546875e-001F};
// FUNcubeBPSKDemod.java:58-77 (symmetric, first 33)
static const float h_dm_half[33] = {
    -0.0101130691F, -0.0086975143F, -0.0038246093F, +0.0033563764F, +0.0107237026F, +0.0157790936F, +0.0164594107F,
    +0.0119213911F, +0.0030315224F, -0.0076488191F, -0.0164594107F, -0.0197184277F, -0.0150109226F, -0.0023082460F,
    +0.0154712381F, +0.0327423589F, +0.0424493086F, +0.0379940454F, +0.0154712381F, -0.0243701991F, -0.0750320094F,
    -0.1244834076F, -0.1568500423F, -0.1553748911F, -0.1061032953F, -0.0015013786F, +0.1568500423F, +0.3572048240F,
    +0.5786381191F, +0.7940228249F, +0.9744923010F, +1.0945250059F, +1.1366117829F};

// the bit clock (:581-584) must be the regular one the tail kernel assumes
static bool bit_clock_is_regular()
{
    const double inc = 1.0 / (double)9600, bt = 1.0 / (double)1200;
    double ph = 0.0;
    int pos = 0;
    for (int t = 0; t < 8 * 64; t++) {
        int expect = t & 7;
        if (pos != expect) return false;
        pos = (pos + 1) % 8;
        ph += inc;
        bool roll = false;
        if (ph >= bt) {
            ph -= bt;
            pos = 0;
            roll = true;
        }
        if (roll != (expect == 7)) return false;
        if (roll && ph != 0.0) return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------- FFT-acquire set-up
// (which front end serves a frame: fft_front_kind, bpsk_fftplan.hip)
// the frame rule's one text; `what`: "<entry point>: <what needs the frame>"
static int fft_frame_refused(const char *what, int n)
{
    set_error("%s needs a frame of 416 .. 4194304 samples whose prime factors r above 7 keep n r within 2^31 (got %d): below 416 the 204 "
              "gathered bins (FUNcubeBPSKDemod.java:458) do not end inside the frame", what, n);
    return JSDR_ERR;
}

// The FFT-acquire buffers of a handle: state zeroed (Java's field initialisers, :403-405), the twiddles and the plan of the
// frame's front end, the VCO factors' table -- at jsdr_bpsk_create for do_fft, for the FFT-acquire channels of a channel
// handle, or at the first live switch of a handle created in the tune mode; `seam`: and the scratch of the tune -> FFT seam
// (live switches only: the second run's state and row).  All or nothing: a failure leaves the handle as it was.
int jsdr::fft_mode_alloc(jsdr_bpsk *h, FftFront kind, bool seam)
{
    const int n = h->nsf;
    const size_t S = (size_t)h->nstreams;
    const long long stride2 = 64 + n / h->decim + 2 + 64;
    const bool want_seam = seam && !(h->fft_state2.p && h->dm2.p);
    if (h->fft_ready && !want_seam) return JSDR_OK;
    const bool gen = kind == FRONT_GEN, pow2 = kind == FRONT_POW2, f2x = kind == FRONT_FFT2X;
    DevBuf<FftFrontState> st, st2;
    DevBuf<double2> tw, vcs, ek, dm2;
    DevBuf<double> r0;
    std::vector<double2> w;
    FftPlan plan;
    bool ok = !want_seam || (st2.alloc(S) == JSDR_OK && dm2.alloc(S * (size_t)stride2) == JSDR_OK && st2.zero() == JSDR_OK && dm2.zero() == JSDR_OK);
    if (ok && !h->fft_ready) {
        ok = st.alloc(S) == JSDR_OK && vcs.alloc((size_t)h->max_ds) == JSDR_OK &&
             tw.alloc(gen ? 3 * (size_t)n + 64 : pow2 ? (size_t)n : (size_t)65536) == JSDR_OK &&
             (!f2x || (ek.alloc(S * fft2x_scratch_ek(n)) == JSDR_OK && r0.alloc(S * fft2x_scratch_r0(n)) == JSDR_OK)) &&
             // (a mixed-radix frame with a prime factor above 7: the out-of-place pass's scratch, in the 2 m front end's slot)
             (!(kind == FRONT_FFTM && fftm_scratch(n) > 0) || ek.alloc(S * fftm_scratch(n)) == JSDR_OK);
        if (ok) {
            ok = fft_plan_build(plan, w, n, kind) && w.size() <= tw.n && hipMemcpy(tw.p, w.data(), sizeof(double2) * w.size(), hipMemcpyHostToDevice) == hipSuccess &&
                 st.zero() == JSDR_OK;
        }
    }
    if (ok) ok = hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("jsdr_bpsk_set_mode: could not allocate the FFT-acquire buffers (%zu streams of %d-sample frames); the handle is unchanged",
                  S, n);
        return JSDR_ERR;
    }
    if (want_seam) {
        std::swap(h->fft_state2, st2);
        std::swap(h->dm2, dm2);
        h->dm2_stride = stride2;
    }
    if (!h->fft_ready) {
        std::swap(h->fft_state, st);
        std::swap(h->vco_cs, vcs);
        std::swap(h->fft_tw, tw);
        std::swap(h->fft2x_ek, ek);
        std::swap(h->fft2x_r0, r0);
        h->fft_plan = plan;
        h->fft_ready = true;
    }
    return JSDR_OK;
}

// JSDR_FFT_PHASECLK=1: the front ends' per-phase cycle counts of the handle's last launch, printed at destroy
static void bpsk_phase_clocks_report(const jsdr_bpsk *h)
{
    if (!h->phase_clk.p) return;
    static const char *const names_p2[8] = {"load+scatter", "forward FFT", "|X|", "boxcar+argmax", "centre-bin rule",
                                            "gather/zero", "inverse FFT", "scale+RxDownSample"};
    static const char *const names_mx[8] = {"load", "forward FFT", "centre-bin rule", "gather/zero/place", "inverse FFT",
                                            "RxDownSample", "|X|", "boxcar+argmax"};
    const char *const *names = (h->fft_plan.kind == FRONT_FFTM || h->fft_plan.kind == FRONT_FFT2X) ? names_mx : names_p2;
    long long c[16] = {0};
    if (hipDeviceSynchronize() == hipSuccess &&
        hipMemcpy(c, h->phase_clk.p, sizeof(c), hipMemcpyDeviceToHost) == hipSuccess) {
        if (h->acq_chunk > 0) {  // the three-phase front end ran: the last launch's workgroup 0 of k_acq_fwd / k_acq_inv
            static const char *const nf[6] = {"convert+pass 1", "pass 2", "last pass: loads", "last pass+|X|+spec", "boxcar", "argmax+peak"};
            static const char *const ni[5] = {"gather", "passes 1+2 fused", "last pass", "compact store", "edges+RxDownSample"};
            long long tf = 0, ti = 0;
            for (int k = 0; k < 6; k++) tf += c[k];
            for (int k = 0; k < 5; k++) ti += c[8 + k];
            for (int k = 0; k < 6; k++)
                fprintf(stderr, "[jsdr] k_acq_fwd phase %-20s %12lld ticks  %5.1f %%\n", nf[k], c[k], tf ? 100.0 * (double)c[k] / (double)tf : 0.0);
            for (int k = 0; k < 5; k++)
                fprintf(stderr, "[jsdr] k_acq_inv phase %-20s %12lld ticks  %5.1f %%\n", ni[k], c[8 + k], ti ? 100.0 * (double)c[8 + k] / (double)ti : 0.0);
            memset(c, 0, sizeof(c));
            // every k_acq_fwd workgroup's first and last tick (100 MHz): how many ran from the start, how far apart they ended
            std::vector<long long> w(2 * 4096);
            if (hipMemcpy(w.data(), h->phase_clk.p + 16, sizeof(long long) * w.size(), hipMemcpyDeviceToHost) == hipSuccess) {
                long long t0 = 0, e0 = 0, e1 = 0;
                int n = 0, late = 0;
                for (int i = 0; i < 4096; i++)
                    if (w[2 * i + 1]) {
                        if (!n || w[2 * i] < t0) t0 = w[2 * i];
                        if (!n || w[2 * i + 1] < e0) e0 = w[2 * i + 1];
                        if (!n || w[2 * i + 1] > e1) e1 = w[2 * i + 1];
                        n++;
                    }
                for (int i = 0; i < 4096; i++)
                    if (w[2 * i + 1] && w[2 * i] - t0 > (e1 - t0) / 10) late++;
                fprintf(stderr, "[jsdr] k_acq_fwd %d workgroups: %d started late (> 10 %% into the launch); first end %.3f ms, last end %.3f ms after the first start\n",
                        n, late, (double)(e0 - t0) / 1e5, (double)(e1 - t0) / 1e5);
            }
        }
        long long tot = 0;
        for (int k = 0; k < 8; k++) tot += c[k];
        for (int k = 0; k < 8; k++)
            fprintf(stderr, "[jsdr] k_front_fft phase %-20s %12lld ticks  %5.1f %%\n", names[k], c[k],
                    tot ? 100.0 * (double)c[k] / (double)tot : 0.0);
    }
}

// entry n of the tuner's and the VCO's tables (:159-162): double argument as in Java, correctly rounded function value
static double table_cos(int n) { return (double)cosl((long double)(n * 2.0 * TUNER_PI / 256)); }
static double table_sin(int n) { return (double)sinl((long double)(n * 2.0 * TUNER_PI / 256)); }

int jsdr_bpsk_create(jsdr_bpsk **out, int rate, int nsamples_per_frame, int tuning_hz, int do_fft, int do_up,
                     int nstreams, int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_bpsk_create: null handle pointer");
    *out = nullptr;
    JSDR_REQUIRE(rate >= 1, "jsdr_bpsk_create: rate %d", rate);
    // adsc.rate/DOWN_SAMPLE_RATE (:476), int division.  Below 9600 Hz (an 8 kHz card) the quotient is 0 and `++dsCnt >= 0`
    // holds for every sample: RxDownSample filters at every input, which is what a decimation of 1 does
    const int decim = rate / 9600 > 0 ? rate / 9600 : 1;
    // any rate the reference would take (:476: adsc.rate / DOWN_SAMPLE_RATE, whatever it is); 4, 5, 10, 20 -- the rates
    // java-sdr has defaults for -- take the specialised front ends, everything else the one-thread-per-output kernel.
    // FFT-acquire mode: the power-of-two and the 2 m front ends size their per-thread output lists for a decimation of at
    // least 4; the mixed-radix one (any other frame up to 9600 samples) loops and takes any.
    // Round 6: whatever those refuse -- and any other frame the oracle defines -- goes through the any-frame passes (bpsk_acqg.hip).
    JSDR_REQUIRE(nsamples_per_frame > 0 && nstreams > 0 && nstreams <= 65535, "jsdr_bpsk_create: bad geometry");
    if (max_batch_samples < nsamples_per_frame) max_batch_samples = nsamples_per_frame;
    FftFront front = FRONT_NONE;
    if (do_fft) {
        int force_gen = -1;
        if (const char *e = knob("JSDR_ACQG")) force_gen = atoi(e) != 0;  // (tests: the any-frame passes for a frame the LDS kernels take)
        front = fft_front_kind(nsamples_per_frame, decim, false, force_gen);
        if (front == FRONT_NONE) return fft_frame_refused("jsdr_bpsk_create: FFT-acquire mode", nsamples_per_frame);
    }
    JSDR_REQUIRE(bit_clock_is_regular(), "jsdr_bpsk_create: bit clock schedule is not the regular 8-cycle");
    if (fec_prepare() != JSDR_OK) return JSDR_ERR;
    jsdr_bpsk *h = new jsdr_bpsk();
    h->snap_seq[0].store(0);
    h->snap_seq[1].store(0);
    memset(h->snap, 0, sizeof(h->snap));
    h->rate = rate;
    h->nsf = nsamples_per_frame;
    h->tuning = tuning_hz;
    h->do_fft = do_fft;
    h->do_up = do_up;
    h->nstreams = nstreams;
    h->decim = decim;
    h->max_batch = max_batch_samples;
    h->max_ds = max_batch_samples / decim + 2;
    h->max_bits = (int)(h->max_ds / 4 + 16);
    // a legitimate frame yields one hit per 5200 bits; leave room for false alarms (FUNcubeBPSKDemod.java:560 has no limit,
    // so a call with more hits than this flags the stream instead of returning a truncated log)
    h->trig_cap = h->max_bits / 2600 + 4;
    if (h->trig_cap < MIN_TRIG) h->trig_cap = MIN_TRIG;
    h->tuPhaseInc = tuner_inc((double)tuning_hz, rate);  // :196
    while ((1 << h->logn) < nsamples_per_frame) h->logn++;
    if (do_fft) h->max_batch = (h->max_batch / nsamples_per_frame) * nsamples_per_frame;
    // one stream (the receive() drop-in): nothing of another stream to run beside the tail, and the hop to the side
    // stream costs a cross-stream event per call
    if (nstreams == 1) h->overlap = false;
    // FFT-acquire mode: the front ends hold a CU's whole LDS (one workgroup of a mixed-radix frame, four of a power-of-two
    // frame), so the side stream's kernels cannot run beside them -- they starve and delay it (measured, one session each,
    // tools/ab_overlap_acq.sh / ab_env.sh: a step 14.0 vs 14.9 ms at n = 9600, 17.5 vs 18.1 at 4800, no difference at 19200;
    // round 4: 11.4 vs 12.15 at n = 2048 -- k_sync_t takes 5.1 ms beside k_front_fft against 0.11 alone -- 11.6 vs 12.5 at 4096)
    if (do_fft) h->overlap = false;
    // round 6: beside the three-phase front end's kernels of the 1024- and 2048-sample frames (128-thread workgroups, two waves a
    // SIMD) the side section does overlap usefully -- the tail / sync / FEC of call k under the forward kernel of call k + 1: a step
    // 9.97 against 11.25 ms at n = 2048 (1024 x 2^20), 10.50 / 12.28 at 1024, 1.16 / 1.61 at 64 streams; at n = 4096 it loses again
    // (12.29 against 10.87) -- so a handle of such frames that takes calls of several frames keeps its side stream
    if (do_fft && nstreams > 1 && (nsamples_per_frame == 1024 || nsamples_per_frame == 2048) && max_batch_samples >= 2LL * nsamples_per_frame)
        h->overlap = true;
    if (const char *e = knob("JSDR_NO_OVERLAP")) h->overlap = atoi(e) == 0;
    if (const char *e = knob("JSDR_FM")) h->use_fm = atoi(e) != 0;
    if (const char *e = knob("JSDR_SCHED_PREFETCH")) h->prefetch_on = atoi(e) != 0;
    const size_t S = (size_t)nstreams;
    // FEC of a batch handle: the lane-per-block Viterbi (fec.hip, k_vitq) once there are enough blocks to fill waves of 64;
    // below that (and for the 1-stream receive() form, whose latency counts) one wave per block
    bool vitq = nstreams >= 256;
    if (const char *e = knob("JSDR_VITQ")) vitq = atoi(e) != 0 && nstreams > 1;
    h->dm_stride = 64 + h->max_ds + 64;
    h->y_stride = h->max_ds;
    h->bitlog_stride = (HIST_BITS + h->max_bits + 64 + 15) & ~15LL;  // (rows 16-byte aligned: k_tail8 carries the register over in dwords)
    bool ok = h->sincos.alloc(512) == JSDR_OK && h->ktu.alloc((size_t)h->max_batch + 8192) == JSDR_OK &&
              h->kvco.alloc(2 * (size_t)h->max_ds) == JSDR_OK && h->hist_in[0].alloc(S * 32) == JSDR_OK &&
              h->hist_in[1].alloc(S * 32) == JSDR_OK && h->dm.alloc(S * (size_t)h->dm_stride) == JSDR_OK &&
              h->y[0].alloc(S * (size_t)h->y_stride + 2 * Y_PAD) == JSDR_OK && h->y[1].alloc(S * (size_t)h->y_stride + 2 * Y_PAD) == JSDR_OK && h->tail.alloc(S) == JSDR_OK &&
              h->bitlog[0].alloc(S * (size_t)h->bitlog_stride) == JSDR_OK &&
              h->bitlog[1].alloc(S * (size_t)h->bitlog_stride) == JSDR_OK && h->nbits.alloc(S) == JSDR_OK &&
              h->trig_count.alloc(S) == JSDR_OK && h->trig_bits.alloc(S * h->trig_cap) == JSDR_OK &&
              h->fec_scratch.alloc(vitq ? (size_t)fec_vitq_scratch_words(nstreams, h->trig_cap) : S * h->trig_cap * (size_t)fec_dec_scratch_words()) == JSDR_OK && h->fec_done.alloc(S) == JSDR_OK &&
              (!vitq || (h->fec_vit.alloc(S * h->trig_cap * 320) == JSDR_OK && h->fec_work.alloc(S * h->trig_cap + 1) == JSDR_OK)) &&
              h->fec_rc.alloc(S * h->trig_cap) == JSDR_OK && h->fec_last.alloc(S * 2) == JSDR_OK &&
              h->cnt_dec.alloc(S) == JSDR_OK && h->corr.alloc(S * (size_t)h->max_bits) == JSDR_OK &&
              h->fec_data.alloc(S * h->trig_cap * 256) == JSDR_OK && h->decoded.alloc(S * 256) == JSDR_OK &&
              // (one frame; a 1-stream handle's receive() sends the schedule's tables behind it in the same copy)
              h->stage_raw.alloc((size_t)nsamples_per_frame * 2 + (nstreams == 1 ? ((do_fft ? sizeof(double2) : 1) * (size_t)h->max_ds + sizeof(double2) * (256 + FM_TABLE_SLACK) + 256) / 4 : 0)) == JSDR_OK &&
              h->ds_taps_dev.alloc(32) == JSDR_OK &&
              h->dmh[0].alloc(S * 64) == JSDR_OK && h->dmh[1].alloc(S * 64) == JSDR_OK && h->hist_bad.alloc(1) == JSDR_OK && h->amax.alloc(S) == JSDR_OK && h->fm_tickets.alloc(1) == JSDR_OK && h->fm_edges.alloc(S * 4 * FM_EDGE) == JSDR_OK && h->snap_dev.alloc(1) == JSDR_OK && h->tcs.alloc(2 * (256 + FM_TABLE_SLACK)) == JSDR_OK;
    if (ok && nstreams == 1) {
        // [frame | ktu | kvco | vco_cs | tcs] + alignment slack, then the SnapPack slot (not handed out by h2d_call)
        const size_t need = sizeof(float) * 2 * (size_t)nsamples_per_frame + ((size_t)h->max_batch + 26) + (size_t)h->max_ds +
                            (do_fft ? sizeof(double2) * (size_t)h->max_ds : 0) + sizeof(double2) * (256 + FM_TABLE_SLACK) + 8 * 64;
        const size_t arena = (need + 63) & ~(size_t)63;
        if (arena <= ((size_t)8 << 20) && h->pin.alloc(arena + sizeof(SnapPack))) h->pin_bytes = arena;
        else (void)hipGetLastError();  // no pinned memory: the pageable path serves
    }
    if (!ok) {
        jsdr_bpsk_destroy(h);
        return JSDR_ERR;
    }
    // tables (:159-162): Math.sin/cos are allowed 1 ulp; the host libm stands in (DESIGN.md "tables")
    std::vector<double> sc(512);
    for (int n = 0; n < 256; n++) {
        sc[n] = table_cos(n);
        sc[256 + n] = table_sin(n);
    }
    BpskConst bc;  // the kernels' constant tables: dsFilter, dmFilter, SYNC_VECTOR (jsdr_bpsk_table has them)
    memset(&bc, 0, sizeof(bc));
    double sync[SYNC_N];
    (void)jsdr_bpsk_table(0, bc.ds_taps, 32);
    (void)jsdr_bpsk_table(1, bc.dm_taps, 96);
    (void)jsdr_bpsk_table(2, sync, SYNC_N);
    for (int i = 0; i < SYNC_N; i++) bc.sync[i] = sync[i] > 0.0 ? 1 : -1;
    if (do_fft) {
        // (the tune <-> FFT seam's scratch comes with the first live switch, if there is one)
        if (fft_mode_alloc(h, front, false) != JSDR_OK) {
            set_error("jsdr_bpsk_create: FFT-mode initialisation failed");
            jsdr_bpsk_destroy(h);
            return JSDR_ERR;
        }
        if (const char *e = knob("JSDR_ACQ3")) h->acq_mode = atoi(e) != 0 ? 1 : 0;
        if (const char *e = knob("JSDR_FFT_PHASECLK"))
            if (atoi(e) != 0 && (h->phase_clk.alloc(16 + 2 * 4096) != JSDR_OK || h->phase_clk.zero() != JSDR_OK)) h->phase_clk.release();
    }
    if (hipMemcpy(h->ds_taps_dev.p, bc.ds_taps, sizeof(double) * 27, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("jsdr_bpsk_create: tap upload failed");
        jsdr_bpsk_destroy(h);
        return JSDR_ERR;
    }
    std::vector<TailState> ts(S);
    memset(ts.data(), 0, sizeof(TailState) * S);
    for (size_t i = 0; i < S; i++) {
        ts[i].dmEnergyOut = 1.0;  // :499
        ts[i].last_g = -1;
    }
    {
        // Worst-case error of (fi,fq) when both FIR stages use fused multiply-adds instead of the reference's separately
        // rounded products and sums (u = 2^-53; |x| <= 32768/32767, |cos|,|sin| <= 1):
        //   27-tap stage : |s' - s| <= (gamma_28 + gamma_27) T1,            T1 = sum |x_k| |t_k| <= 1.00004 sum|dsFilter|
        //   x HOWARD, VCO: |dm' - dm| <= 56 u T1 HOWARD + 4 u Dmax,         Dmax = HOWARD T1 bounds |dm|
        //   65-tap stage : |y' - y| <= (gamma_66 + gamma_65) F1 Dmax + F1 |dm' - dm|,   F1 = sum|dmFilter|
        double t1 = 0.0, f1 = 0.0;
        for (int i = 0; i < 27; i++) t1 += fabs(bc.ds_taps[i]);
        for (int i = 0; i < 65; i++) f1 += fabs(bc.dm_taps[i]);
        t1 *= 1.00004;
        const double U = 1.1102230246251565e-16, HOWARD = 0.9 * 32768.0, dmax = HOWARD * t1;
        h->fast_ey = 1.01 * U * f1 * (131.0 * dmax + 56.0 * t1 * HOWARD + 4.0 * dmax);
        if (const char *e = knob("JSDR_FAST_MARGIN_SCALE")) {
            const double v = atof(e);
            if (v >= 1.0) h->margin_scale = v;
        }
        if (const char *e = knob("JSDR_FAST_ARGMAX_SCALE")) {
            const double v = atof(e);
            if (v >= 1.0) h->argmax_scale = v;
        }
    }
    h->h_sincos = sc;
    bool up = hipMemcpy(h->sincos.p, sc.data(), sizeof(double) * 512, hipMemcpyHostToDevice) == hipSuccess &&
              bpsk_upload_constants(bc) == JSDR_OK &&
              hipMemcpy(h->tail.p, ts.data(), sizeof(TailState) * S, hipMemcpyHostToDevice) == hipSuccess &&
              h->hist_in[0].zero() == JSDR_OK && h->hist_in[1].zero() == JSDR_OK && h->dm.zero() == JSDR_OK &&
              h->dmh[0].zero() == JSDR_OK && h->dmh[1].zero() == JSDR_OK && h->tcs.zero() == JSDR_OK && h->amax.zero() == JSDR_OK &&
              h->bitlog[0].zero() == JSDR_OK && h->bitlog[1].zero() == JSDR_OK && h->decoded.zero() == JSDR_OK &&
              h->nbits.zero() == JSDR_OK && h->trig_count.zero() == JSDR_OK && h->fec_last.zero() == JSDR_OK && h->fec_done.zero() == JSDR_OK &&
              h->cnt_dec.zero() == JSDR_OK && h->y[0].zero() == JSDR_OK && h->y[1].zero() == JSDR_OK &&
              h->tail_stream.create(hipStreamNonBlocking) == JSDR_OK && h->ev_matched.create(hipEventDisableTiming) == JSDR_OK &&
              h->ev_tail_done[0].create(hipEventDisableTiming) == JSDR_OK && h->ev_tail_done[1].create(hipEventDisableTiming) == JSDR_OK &&
              h->ev_pack_done.create(hipEventDisableTiming) == JSDR_OK;
    if (!up || hipDeviceSynchronize() != hipSuccess) {
        set_error("jsdr_bpsk_create: device initialisation failed");
        jsdr_bpsk_destroy(h);
        return JSDR_ERR;
    }
    *out = h;
    return JSDR_OK;
}

// Nothing is freed or destroyed while work of the handle can still be in flight: the worker is joined and the device and the
// side stream are waited for first; then the members give back what they hold.
int jsdr_bpsk_destroy(jsdr_bpsk *h)
{
    if (!h) return JSDR_OK;
    if (h->worker.joinable()) h->worker.join();
    (void)hipDeviceSynchronize();
    if (h->tail_stream) (void)hipStreamSynchronize(h->tail_stream);
    bpsk_debug_clocks_report();
    bpsk_phase_clocks_report(h);
    delete h;
    return JSDR_OK;
}

int jsdr_bpsk_set_cu_share(jsdr_bpsk *h, int wgs_per_cu)
{
    JSDR_REQUIRE(h && wgs_per_cu >= 0 && wgs_per_cu <= 16, "jsdr_bpsk_set_cu_share: bad argument");
    if (wgs_per_cu > 0 && !device_cus(h)) return JSDR_ERR;
    h->share_wgs_per_cu = wgs_per_cu;
    return JSDR_OK;
}

int jsdr_bpsk_pair_shares(jsdr_bpsk *h, int *fft_wgs_per_cu, int *bpsk_wgs_per_cu)
{
    JSDR_REQUIRE(h && fft_wgs_per_cu && bpsk_wgs_per_cu, "jsdr_bpsk_pair_shares: null argument");
    // measured (DESIGN.md "the step", profiles/r04_experiments.md, r05_j_bench.json): the 2 + 1 split pays for the exact variant's
    // tune-mode kernel at 96 kHz / 2048-sample frames from 8192 streams per device (33.5 against 35.1 ms); at 4096 / 2048 / 1024
    // streams it is slower than one after the other (19.8 / 10.2 / 5.9 against 17.9 / 9.5 / 5.1), and so it is with the fast variant
    const bool pays = !h->do_fft && h->rate == 96000 && h->nsf == 2048 && h->variant == 0 && h->nstreams >= 8192;
    *fft_wgs_per_cu = pays ? 2 : 0;
    *bpsk_wgs_per_cu = pays ? 1 : 0;
    return JSDR_OK;
}

// the demodulator's constant tables as this library holds them (host side, no device needed): 0 = dsFilter[27]
// (FUNcubeBPSKDemod.java:27-55), 1 = dmFilter[65] (:58-77, one of the two identical copies), 2 = SYNC_VECTOR[65] (:79-81)
int jsdr_bpsk_table(int which, double *out, int cap)
{
    JSDR_REQUIRE(out, "jsdr_bpsk_table: null argument");
    const int n = which == 0 ? 27 : ((which == 1 || which == 2) ? 65 : ((which == 3 || which == 4) ? 256 : 0));
    JSDR_REQUIRE(n > 0 && cap >= n, "jsdr_bpsk_table: table %d needs room for %d values", which, n);
    if (which >= 3) {
        for (int i = 0; i < 256; i++) out[i] = which == 3 ? table_cos(i) : table_sin(i);
    } else if (which == 0) {
        for (int i = 0; i < 14; i++) out[i] = out[26 - i] = (double)h_ds_half[i];
    } else if (which == 1) {
        for (int i = 0; i < 33; i++) out[i] = out[64 - i] = (double)h_dm_half[i];
    } else {
        int sr = 0x7f;  // the sync LFSR (FECDecoder.java:600-605) == SYNC_VECTOR
        for (int i = 0; i < 65; i++) {
            out[i] = (sr & 64) ? 1.0 : -1.0;
            int v = sr & 0x48;
            v ^= v >> 4;
            v ^= v >> 2;
            v ^= v >> 1;
            sr = ((sr << 1) | (v & 1)) & 0xffff;
        }
    }
    return JSDR_OK;
}

// what every creator of a channel handle asks of its channel arguments, before any device work
static int chan_args_check(const char *who, int ninputs, int nchannels, const double *tuning_hz)
{
    JSDR_REQUIRE(nchannels >= 1 && nchannels <= CHAN_MAX, "%s: nchannels %d outside 1 .. %d", who, nchannels, (int)CHAN_MAX);
    JSDR_REQUIRE(ninputs >= 1 && (long long)ninputs * nchannels <= 65535, "%s: %d inputs x %d channels", who, ninputs, nchannels);
    JSDR_REQUIRE(tuning_hz, "%s: null tuning array", who);
    for (int c = 0; c < nchannels; c++)
        JSDR_REQUIRE(std::isfinite(tuning_hz[c]), "%s: tuning of channel %d (%g Hz) is not finite", who, c, tuning_hz[c]);
    return JSDR_OK;
}

int jsdr_bpsk_create_channels(jsdr_bpsk **out, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                              const double *tuning_hz, const int *do_up, int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_bpsk_create_channels: null handle pointer");
    *out = nullptr;
    if (chan_args_check("jsdr_bpsk_create_channels", ninputs, nchannels, tuning_hz) != JSDR_OK) return JSDR_ERR;
    if (max_batch_samples < nsamples_per_frame) max_batch_samples = nsamples_per_frame;
    JSDR_REQUIRE(max_batch_samples <= 0x3fffffffLL, "jsdr_bpsk_create_channels: max_batch_samples %lld above 2^30 - 1",
                 (long long)max_batch_samples);
    jsdr_bpsk *h = nullptr;
    if (jsdr_bpsk_create(&h, rate, nsamples_per_frame, 0, 0, do_up ? do_up[0] != 0 : 0, ninputs * nchannels, max_batch_samples) != JSDR_OK)
        return JSDR_ERR;
    h->nch = nchannels;
    h->nin = ninputs;
    h->use_fm = false;
    h->chan = std::vector<BpskChan>((size_t)nchannels);
    bool ok = sincos9_ensure(h) == JSDR_OK;
    for (int c = 0; c < nchannels && ok; c++) {
        BpskChan &cc = h->chan[c];
        cc.tuning = tuning_hz[c];
        cc.tuPhaseInc = tuner_inc(tuning_hz[c], rate);  // :196
        cc.do_up = do_up ? do_up[c] != 0 : 0;
        ok = cc.dev.alloc((size_t)h->max_batch + 26) == JSDR_OK;
    }
    if (!ok) {
        set_error("jsdr_bpsk_create_channels: device allocation failed (%d channels of %lld samples)", nchannels, (long long)h->max_batch);
        jsdr_bpsk_destroy(h);
        return JSDR_ERR;
    }
    h->tuning = h->chan[0].tuning;
    h->tuPhaseInc = h->chan[0].tuPhaseInc;
    h->do_up = h->chan[0].do_up;
    *out = h;
    return JSDR_OK;
}

int jsdr_bpsk_create_mode_channels(jsdr_bpsk **out, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                                   const double *tuning_hz, const int *do_fft, const int *do_up, int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_bpsk_create_mode_channels: null handle pointer");
    *out = nullptr;
    // every check before any device work
    if (chan_args_check("jsdr_bpsk_create_mode_channels", ninputs, nchannels, tuning_hz) != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(rate >= 1 && nsamples_per_frame > 0, "jsdr_bpsk_create_mode_channels: rate %d, frame of %d samples", rate, nsamples_per_frame);
    int nfft = 0;
    for (int c = 0; c < nchannels; c++) nfft += (do_fft && do_fft[c]) ? 1 : 0;
    FftFront front = FRONT_NONE;
    if (nfft > 0) {
        // the three-phase front ends' own frames, or any frame the any-frame passes take
        front = fft_front_kind(nsamples_per_frame, rate / 9600 > 0 ? rate / 9600 : 1, true);
        if (front == FRONT_NONE) return fft_frame_refused("jsdr_bpsk_create_mode_channels: an FFT-acquire channel", nsamples_per_frame);
    }
    jsdr_bpsk *h = nullptr;
    if (jsdr_bpsk_create_channels(&h, rate, nsamples_per_frame, ninputs, nchannels, tuning_hz, do_up, max_batch_samples) != JSDR_OK) return JSDR_ERR;
    h->mode_chan = true;
    if (nfft > 0) {
        // (no tune <-> FFT seam's scratch: a channel's mode never changes)
        if (fft_mode_alloc(h, front, false) != JSDR_OK) {
            jsdr_bpsk_destroy(h);
            return JSDR_ERR;
        }
        for (int c = 0; c < nchannels; c++) h->chan[c].do_fft = do_fft[c] ? 1 : 0;
        h->nfftch = nfft;
        h->max_batch = (h->max_batch / nsamples_per_frame) * nsamples_per_frame;  // calls are whole frames
    }
    *out = h;
    return JSDR_OK;
}

int jsdr_bpsk_create_live_channels(jsdr_bpsk **out, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                                   const double *tuning_hz, const int *do_fft, const int *do_up, int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_bpsk_create_live_channels: null handle pointer");
    *out = nullptr;
    // every check before any device work
    if (chan_args_check("jsdr_bpsk_create_live_channels", ninputs, nchannels, tuning_hz) != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(rate >= 1 && nsamples_per_frame > 0, "jsdr_bpsk_create_live_channels: rate %d, frame of %d samples", rate, nsamples_per_frame);
    // any channel may come to acquire: the frame must be one FFT-acquire takes, whatever the initial modes
    const FftFront front = fft_front_kind(nsamples_per_frame, rate / 9600 > 0 ? rate / 9600 : 1, true);
    if (front == FRONT_NONE) return fft_frame_refused("jsdr_bpsk_create_live_channels: a channel that may switch to FFT-acquire", nsamples_per_frame);
    jsdr_bpsk *h = nullptr;
    if (jsdr_bpsk_create_channels(&h, rate, nsamples_per_frame, ninputs, nchannels, tuning_hz, do_up, max_batch_samples) != JSDR_OK) return JSDR_ERR;
    h->mode_chan = true;
    h->live_chan = true;
    // everything a switch needs per channel and stream, for EVERY channel, now: the FFT state rows (zeroed: Java's field
    // initialisers) with the front end's tables, and the seam's Q columns.  (The tuner's host state and device slot of a channel
    // that starts in FFT-acquire are jsdr_bpsk_create_channels'.)
    if (fft_mode_alloc(h, front, true) != JSDR_OK || h->seam_q.alloc((size_t)h->nstreams * 26) != JSDR_OK || h->seam_q.zero() != JSDR_OK ||
        hipDeviceSynchronize() != hipSuccess) {
        jsdr_bpsk_destroy(h);
        return JSDR_ERR;
    }
    for (int c = 0; c < nchannels; c++) {
        h->chan[c].do_fft = (do_fft && do_fft[c]) ? 1 : 0;
        h->nfftch += h->chan[c].do_fft;
    }
    *out = h;
    return JSDR_OK;
}

int jsdr_bpsk_channel_info(jsdr_bpsk *h, int *ninputs, int *nchannels)
{
    JSDR_REQUIRE(h && ninputs && nchannels, "jsdr_bpsk_channel_info: null argument");
    *ninputs = h->nch > 0 ? h->nin : h->pst_nch > 0 ? h->pst_nin : h->nstreams;
    *nchannels = h->nch > 0 ? h->nch : h->pst_nch > 0 ? h->pst_nch : 1;
    return JSDR_OK;
}

int jsdr_bpsk_create_tuned(jsdr_bpsk **out, int rate, int nsamples_per_frame, int nstreams, const double *tuning_hz,
                           int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_bpsk_create_tuned: null handle pointer");
    *out = nullptr;
    // every check before any device work
    JSDR_REQUIRE(tuning_hz, "jsdr_bpsk_create_tuned: null tuning array");
    JSDR_REQUIRE(rate >= 1 && nsamples_per_frame > 0 && nstreams > 0 && nstreams <= 65535, "jsdr_bpsk_create_tuned: bad geometry (rate %d, "
                 "frame of %d samples, %d streams)", rate, nsamples_per_frame, nstreams);
    for (int s = 0; s < nstreams; s++)
        JSDR_REQUIRE(std::isfinite(tuning_hz[s]) && tuning_hz[s] < (double)rate, "jsdr_bpsk_create_tuned: tuning %g Hz of stream %d is not a "
                     "finite value below the rate (%d Hz)", tuning_hz[s], s, rate);
    jsdr_bpsk *h = nullptr;
    if (jsdr_bpsk_create(&h, rate, nsamples_per_frame, 0, 0, 0, nstreams, max_batch_samples) != JSDR_OK) return JSDR_ERR;
    h->pst = true;
    h->use_fm = false;
    const size_t S = (size_t)nstreams;
    h->pst_tuning.assign(tuning_hz, tuning_hz + nstreams);
    std::vector<double> inc(S);
    for (size_t s = 0; s < S; s++) inc[s] = tuner_inc(tuning_hz[s], rate);  // :196
    h->pst_ckpt_stride = h->max_batch / PST_C + 1;
    const bool ok = sincos9_ensure(h) == JSDR_OK && h->pst_tu.alloc(S) == JSDR_OK && h->pst_inc.alloc(S) == JSDR_OK &&
                    h->pst_ckpt.alloc(S * (size_t)h->pst_ckpt_stride) == JSDR_OK && h->pst_kh[0].alloc(S * 32) == JSDR_OK &&
                    h->pst_kh[1].alloc(S * 32) == JSDR_OK && h->pst_ids.alloc(S) == JSDR_OK && h->pst_tu.zero() == JSDR_OK &&
                    h->pst_kh[0].zero() == JSDR_OK && h->pst_kh[1].zero() == JSDR_OK &&
                    hipMemcpy(h->pst_inc.p, inc.data(), sizeof(double) * S, hipMemcpyHostToDevice) == hipSuccess &&
                    hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("jsdr_bpsk_create_tuned: device allocation failed (%d streams of %lld samples)", nstreams, (long long)h->max_batch);
        jsdr_bpsk_destroy(h);
        return JSDR_ERR;
    }
    *out = h;
    return JSDR_OK;
}

// A tuned handle whose streams are the channels of shared inputs: jsdr_bpsk_create_tuned's handle of ninputs x nchannels streams
// (walk, per-stream state, retunes, plans), fed by k_chan_front_pst from one row per INPUT.
int jsdr_bpsk_create_tuned_channels(jsdr_bpsk **out, int rate, int nsamples_per_frame, int ninputs, int nchannels, const double *tuning_hz,
                                    int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_bpsk_create_tuned_channels: null handle pointer");
    *out = nullptr;
    // every check before any device work
    JSDR_REQUIRE(tuning_hz, "jsdr_bpsk_create_tuned_channels: null tuning array");
    JSDR_REQUIRE(nchannels >= 1 && nchannels <= CHAN_MAX, "jsdr_bpsk_create_tuned_channels: nchannels %d outside 1 .. %d", nchannels, (int)CHAN_MAX);
    JSDR_REQUIRE(rate >= 1 && nsamples_per_frame > 0 && ninputs >= 1 && (long long)ninputs * nchannels <= 65535,
                 "jsdr_bpsk_create_tuned_channels: bad geometry (rate %d, frame of %d samples, %d inputs x %d channels; at most 65535 streams)",
                 rate, nsamples_per_frame, ninputs, nchannels);
    const int S = ninputs * nchannels;
    for (int s = 0; s < S; s++)
        JSDR_REQUIRE(std::isfinite(tuning_hz[s]) && tuning_hz[s] < (double)rate, "jsdr_bpsk_create_tuned_channels: tuning %g Hz of channel %d of "
                     "input %d is not a finite value below the rate (%d Hz)", tuning_hz[s], s % nchannels, s / nchannels, rate);
    jsdr_bpsk *h = nullptr;
    if (jsdr_bpsk_create_tuned(&h, rate, nsamples_per_frame, S, tuning_hz, max_batch_samples) != JSDR_OK) return JSDR_ERR;
    h->pst_nin = ninputs;
    h->pst_nch = nchannels;
    *out = h;
    return JSDR_OK;
}
