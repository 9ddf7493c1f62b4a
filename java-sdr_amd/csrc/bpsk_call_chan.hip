// bpsk_call_chan.hip -- a channel handle's call (jsdr_bpsk_create_channels and its kin): chan_run.  Host code only
// (bpsk_handle.h); the stages it shares with the other kinds of handle are bpsk_call.hip's.
#include "bpsk_handle.h"
#include <stddef.h>

// ------------------------------------------------------------------------------------------- channel handles
// Every channel's tuner schedule for a call of L samples (bpsk_sched.hip: kept where the state has come back, shared between
// equal keys, built in parallel), and the channels' state moved to the call's end.  *fresh[c]: the device copy must be sent.
static void chan_schedules(jsdr_bpsk *h, long long L, bool first, bool *fresh)
{
    ChanSchedule *sched[CHAN_MAX];
    ChanKey want[CHAN_MAX];
    for (int c = 0; c < h->nch; c++) {
        BpskChan &ch = h->chan[c];
        sched[c] = ch.do_fft ? nullptr : &ch.sched;  // doBufferFFT never runs the tuner (:406-464): tuPhase stands still
        want[c].tu0 = ch.tuPhase;
        want[c].inc = ch.tuPhaseInc;
        want[c].L = L;
        want[c].first = first;
        memcpy(want[c].hist0, ch.khist, sizeof(ch.khist));
    }
    h->sched_sync += chan_schedules(sched, want, h->nch, fresh);
    for (int c = 0; c < h->nch; c++) {
        BpskChan &ch = h->chan[c];
        if (ch.do_fft) continue;
        ch.tuPhase = ch.sched.tu1;
        memcpy(ch.khist, ch.sched.khist1, sizeof(ch.khist));
    }
}

// The shared VCO schedule (:511-516): the same for every channel and input.  Left in h->vco; returns the outputs of the call.
static long long chan_vco(jsdr_bpsk *h, long long L, bool *fresh)
{
    *fresh = vco_schedule(h->vco, h->vcoPhase, h->dsCnt, h->decim, L);
    h->vcoPhase = h->vco.vco1;
    h->dsCnt = h->vco.ds1;
    return (long long)h->vco.kvco.size();
}

// the bands the FFT-acquire channels search (bit 0: lower, bit 1: upper): what the three-phase scratch is cut for
static int chan_band_mask(const jsdr_bpsk *h)
{
    int mask = 0;
    for (int c = 0; c < h->nch; c++)
        if (h->chan[c].do_fft) mask |= h->chan[c].do_up ? 2 : 1;
    return mask;
}

// A live channel handle, "Track high" on a channel that has run FFT-acquire frames in the other band: until a frame's peak moves
// it (:447-450) the channel's centreBin is the other band's (clamped to this band's end, :444-445), and the 204 bins around it
// (:458) are not all in the rows the three-phase forward kernels keep of ONE band -- [0, n/4 + 28), or [0, 204) and
// [n/4 - 26, n/2 + 28): they hold what the rule can produce in that band.  Such a channel's frames go through the ordinary
// handle's one-kernel front end, which has the whole spectrum in LDS, over the channel's streams (one an input, rows strided as
// the per-channel launches stride them), and the call then waits for it and reads the centre bins: once every input's gathers
// inside the band's rows the channel is back in the three-phase launches.  Frames that only the any-frame passes take have no
// such kernel: they stay in the three-phase launches.
static bool chan_cb_foreign(const jsdr_bpsk *h, int c)
{
    return h->live_chan && h->chan[c].cb_band >= 0 && h->chan[c].cb_band != (h->chan[c].do_up ? 1 : 0);
}

static bool chan_fused_ok(const jsdr_bpsk *h)
{
    return h->fft_plan.kind != FRONT_GEN && fft_front_kind(h->nsf, h->decim, false, -1) == fft_front_kind(h->nsf, h->decim, true, -1);
}

static int chan_fused_front(jsdr_bpsk *h, const FftFrontArgs &xa, int c, bool names_call, bool hist_float, hipStream_t st)
{
    BpskChan &cc = h->chan[c];
    const int S = h->nin, n = h->nsf;
    FftFrontArgs x1 = xa;
    x1.do_up = cc.do_up;
    x1.st = h->fft_state.p + (size_t)c * (size_t)S;
    x1.dm = h->dm.p + (long long)c * h->dm_stride;
    x1.dm_stride = h->dm_stride * h->nch;
    x1.phase_clk = nullptr;
    const FftFront kind = h->fft_plan.kind;
    auto front = [&](const FftFrontArgs &x) {
        return kind == FRONT_FFT2X ? launch_front_fft2x(x, h->fft_plan, h->fft2x_ek.p, h->fft2x_r0.p, S, st)
                                   : (kind == FRONT_FFTM ? launch_front_fftm(x, h->fft_plan, h->fft2x_ek.p, S, st) : launch_front_fft(x, S, st));
    };
    const bool seam = cc.seam == SEAM_TO_FFT;
    if (seam) {
        // the call also carries the channel's tune -> FFT-acquire seam: the ordinary handle's way -- the I column into the channel's
        // state rows, a copy of those rows with the Q column (fft_state2's first rows), and below frame 0 once more from the copy
        // into dm2's rows, whose Q rail k_seam_q takes for the outputs that reach back
        ChanSeamHist sh;
        memcpy(sh.k9, cc.khist, sizeof(sh.k9));
        double *qcol = h->seam_q.p + (size_t)c * (size_t)S * 26;
        if (launch_chan_seam_hist(h->hist_in[h->hist_cur].p, hist_float ? 1 : 0, h->sincos9.p, sh, x1.st, qcol, S, st) != JSDR_OK) return JSDR_ERR;
        JSDR_HIP_TRY(hipMemcpyAsync(h->fft_state2.p, x1.st, sizeof(FftFrontState) * (size_t)S, hipMemcpyDeviceToDevice, st));
        unsigned char *hist2 = reinterpret_cast<unsigned char *>(h->fft_state2.p) + offsetof(FftFrontState, hist);
        JSDR_HIP_TRY(hipMemcpy2DAsync(hist2, sizeof(FftFrontState), qcol, sizeof(double) * 26, sizeof(double) * 26, (size_t)S,
                                      hipMemcpyDeviceToDevice, st));
    }
    {
        ProfScope ps(h, PK_FRONT, st);
        const char *name = kind == FRONT_FFT2X ? "k_front_fft2x" : (kind == FRONT_FFTM ? (fftm_pairs(x1.n, x1.nframes) ? "k_front_fftm2" : "k_front_fftm") : "k_front_fft");
        if (names_call) h->front_name = name;  // (no three-phase launch ran in the call)
        if (front(x1) != JSDR_OK) return JSDR_ERR;
        if (seam) {
            long long nds1 = 0;
            const long long J = seam_outputs((int)x1.first_out, n, h->decim, x1.nds, &nds1);
            if (J > 0) {
                FftFrontArgs x2 = x1;
                x2.nframes = 1;
                x2.st = h->fft_state2.p;
                x2.dm = h->dm2.p;
                x2.dm_stride = h->dm2_stride;
                x2.nds = nds1;
                if (front(x2) != JSDR_OK) return JSDR_ERR;
                if (launch_seam_q(x1.dm, x1.dm_stride, h->dm2.p, h->dm2_stride, (int)J, S, st) != JSDR_OK) return JSDR_ERR;
            }
        }
    }
    JSDR_HIP_TRY(hipStreamSynchronize(st));
    std::vector<FftFrontState> fs((size_t)S);
    JSDR_HIP_TRY(hipMemcpy(fs.data(), x1.st, sizeof(FftFrontState) * (size_t)S, hipMemcpyDeviceToHost));
    bool settled = true;
    for (int i = 0; i < S; i++) {
        const int b = fs[(size_t)i].centreBin;
        settled = settled && (cc.do_up ? (b == 102 || (b >= n / 4 + 76 && b <= n / 2 - 74)) : (b >= 102 && b <= n / 4 - 74));
    }
    if (settled) cc.cb_band = cc.do_up ? 1 : 0;
    return JSDR_OK;
}

// A call of a channel handle: every channel of every input through k_chan_front, then the per-stream matched filter, tail,
// sync and FEC exactly as bpsk_run launches them for an ordinary handle of ninputs x nchannels streams.
int jsdr::chan_run(jsdr_bpsk *h, const int16_t *raw_dev, const float *rawf_dev, long long stride_i16, long long L, int ic,
                   int qc, hipStream_t st)
{
    JSDR_REQUIRE((raw_dev != nullptr) != (rawf_dev != nullptr), "bpsk channels: null input");
    JSDR_REQUIRE(L > 0 && L <= h->max_batch, "bpsk: nsamples=%lld outside (0, max_batch_samples=%lld]", L, h->max_batch);
    JSDR_REQUIRE((stride_i16 & 1) == 0 && (h->nin == 1 || stride_i16 >= 2 * L),
                 "bpsk channels: input stride %lld too small for %lld samples", stride_i16, L);
    JSDR_REQUIRE(h->nfftch == 0 || (L % h->nsf) == 0, "bpsk channels: a handle with FFT-acquire channels needs whole frames (%lld %% %d != 0); "
                 "the handle is unchanged", L, h->nsf);
    // a live channel handle (jsdr_bpsk_create_live_channels): the channels whose first call after a switch this is
    int nto_tune = 0;  // (FFT-acquire -> tune; the others, tune -> FFT-acquire, are among the nfftch channels)
    for (int c = 0; c < h->nch; c++) nto_tune += h->chan[c].seam == SEAM_TO_TUNE ? 1 : 0;
    JSDR_REQUIRE(nto_tune == 0 || L >= 26, "bpsk channels: a channel's first tune-mode call after FFT-acquire frames needs at least 26 samples "
                 "(the input history is rebuilt from them); the handle is unchanged");
    if (h->nfftch > 0 && h->live_chan && h->acq_scratch.p && h->acq_mask != chan_band_mask(h)) {  // (cut for other bands: an action's
        h->acq_scratch.release();                                                                  //  re-cut did not come about)
        h->acq_chunk = 0;
    }
    if (h->nfftch > 0 && !h->acq_scratch.p) {
        // the one step of the call that can fail for want of memory comes before anything of the handle has moved on
        const int mask = chan_band_mask(h);
        // (per INPUT and frame)
        if (acq_scratch_ensure(h, acq3c_frame_bytes(h->nsf, mask, h->fft_plan.kind == FRONT_GEN), (size_t)h->nin, 4096) != JSDR_OK) return JSDR_ERR;
        h->acq_mask = mask;
    }
    // the inputs' 26-sample history in the form of this call's input (only the tune-mode channels read it; a channel on its first
    // tune call after FFT-acquire frames reads the FFT path's doubles instead).  A channel that switched tune -> FFT-acquire reads
    // it once more, below, in the form it has: converted with the others' or, when no channel is left to convert it for, the form
    // of the call that wrote it
    const bool hist_was_float = h->hist_is_float;
    const bool hist_read = h->nch - h->nfftch - nto_tune > 0;
    if (hist_read) {
        if (hist_form(h, rawf_dev != nullptr, h->nin, st) != JSDR_OK) return JSDR_ERR;
    } else {
        h->hist_is_float = rawf_dev != nullptr;
    }
    const bool seam_hist_float = hist_read ? h->hist_is_float : hist_was_float;
    const int first_out = h->decim - 1 - h->dsCnt;
    const long long g_first = h->n_ds;
    const bool first = h->n_in == 0;
    bool vfresh = false;
    const long long nds = chan_vco(h, L, &vfresh);
    JSDR_REQUIRE(nds <= h->max_ds, "bpsk: internal: %lld decimated samples exceed capacity %lld", nds, h->max_ds);
    bool fresh[CHAN_MAX];
    chan_schedules(h, L, first, fresh);
    if (vfresh && nds > 0)
        if (h2d_call(h, h->kvco.p, h->vco.kvco.data(), (size_t)nds, st) != JSDR_OK) return JSDR_ERR;
    for (int c = 0; c < h->nch; c++) {
        BpskChan &cc = h->chan[c];
        if (cc.seam == SEAM_TO_TUNE) {
            // k_front_split's table in the channel's device slot: the schedule's index of every sample of the call, 256 (pass-through)
            // for the 26 history samples -- they are the FFT path's unmixed doubles.  The slot no longer holds the schedule's table: see below
            expand_k9(cc.k9x, cc.sched.tab.data(), cc.sched.per, L, nullptr, 1, L);
            if (h2d_call(h, cc.dev.p, cc.k9x.data(), sizeof(unsigned short) * cc.k9x.size(), st) != JSDR_OK) return JSDR_ERR;
        } else if (fresh[c]) {
            if (h2d_call(h, cc.dev.p, cc.sched.tab.data(), sizeof(unsigned short) * cc.sched.tab.size(), st) != JSDR_OK) return JSDR_ERR;
        }
    }
    if (h->rx_frame_bytes) {  // receive(): the frame waits at the pinned arena's head
        JSDR_HIP_TRY(hipMemcpyAsync(h->stage_raw.p, h->pin.p, h->rx_frame_bytes, hipMemcpyHostToDevice, st));
        h->rx_frame_bytes = 0;
    }
    const int *raw = reinterpret_cast<const int *>(raw_dev);
    const float2 *rawf = reinterpret_cast<const float2 *>(rawf_dev);
    const long long stride_pairs = stride_i16 / 2;
    if (h->nfftch > 0 && vfresh && nds > 0)
        if (send_vco_cs(h, nds, st) != JSDR_OK) return JSDR_ERR;
    if (h->nfftch > 0) {
        // the FFT-acquire channels: one forward phase per input, scan / inverse / edges per channel (bpsk_acq_chan.hip)
        AcqChanArgs ca;
        ca.nin = h->nin;
        ca.nch = h->nch;
        int fused[CHAN_MAX], nfused = 0;
        for (int c = 0; c < h->nch; c++) {
            if (!h->chan[c].do_fft) continue;
            if (chan_cb_foreign(h, c) && chan_fused_ok(h)) {
                fused[nfused++] = c;  // (below: the centre bin it carries may gather outside its band's three-phase rows)
                continue;
            }
            ca.chan[ca.nfft] = c;
            ca.up[ca.nfft] = h->chan[c].do_up;
            if (h->chan[c].seam == SEAM_TO_FFT) {
                // the channel's first FFT-acquire call after the tune mode: dsBuf's I column into its FFT state rows, the Q column
                // beside them (k_chan_seam_hist); the Q rail of the outputs that reach into it comes from k_acq_edges_seam, behind
                // the channel's own edges in the call's first launch
                ChanSeamHist sh;
                memcpy(sh.k9, h->chan[c].khist, sizeof(sh.k9));
                double *qcol = h->seam_q.p + (size_t)c * (size_t)h->nin * 26;
                if (launch_chan_seam_hist(h->hist_in[h->hist_cur].p, seam_hist_float ? 1 : 0, h->sincos9.p, sh,
                                          h->fft_state.p + (size_t)c * (size_t)h->nin, qcol, h->nin, st) != JSDR_OK)
                    return JSDR_ERR;
                ca.seam_q[ca.nfft] = qcol;
                ca.seam_J = (int)seam_outputs(first_out, h->nsf, h->decim, nds);
            }
            ca.nfft++;
        }
        ca.st = h->fft_state.p;
        FftFrontArgs xa = fft_front_args(h, raw, rawf, stride_pairs, L, ic, qc, first_out, nds);
        xa.do_up = 0;  // (each channel's band is in ca.up)
        AcqLaunchCtx lc;
        acq_launch_ctx(h, lc);
        if (ca.nfft > 0 &&
            launch_acq3_chan(xa, ca, h->acq_scratch.p, h->acq_scratch.n, h->acq_chunk, device_cus(h), st, lc.prof, h->fft_plan) != JSDR_OK)
            return JSDR_ERR;
        h->acq_fwd_frames = ca.fwd_frames;
        h->acq_inv_frames = ca.inv_frames;
        h->front_name = ca.fwd_name;
        for (int k = 0; k < ca.nfft; k++)
            if (!chan_cb_foreign(h, ca.chan[k])) h->chan[ca.chan[k]].cb_band = ca.up[k] ? 1 : 0;
        for (int k = 0; k < nfused; k++)
            if (chan_fused_front(h, xa, fused[k], ca.nfft == 0 && k == 0, seam_hist_float, st) != JSDR_OK) return JSDR_ERR;
    }
    if (h->live_chan && h->nfftch == 0) h->acq_fwd_frames = h->acq_inv_frames = 0;  // (what a handle without FFT-acquire channels reports)
    if (nds > 0 && h->nch - h->nfftch - nto_tune > 0) {
        ChanFrontArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.raw = rawf ? reinterpret_cast<const int *>(rawf) : raw;
        fa.stride_pairs = stride_pairs;
        fa.ic = ic;
        fa.qc = qc;
        fa.hist = h->hist_in[h->hist_cur].p;
        for (int c = 0; c < h->nch; c++) {  // the tune-mode channels (all of them, but on a handle with FFT-acquire channels)
            if (h->chan[c].do_fft || h->chan[c].seam == SEAM_TO_TUNE) continue;
            fa.k9[fa.nch] = h->chan[c].dev.p;
            fa.per[fa.nch] = h->chan[c].sched.per;
            fa.chan_of[fa.nch] = c;
            fa.nch++;
        }
        fa.nch_all = h->nch;
        fa.kvco = h->kvco.p;
        fa.sc9 = h->sincos9.p;
        fa.ds_taps = h->ds_taps_dev.p;
        fa.dm = h->dm.p;
        fa.dm_stride = h->dm_stride;
        fa.nds = nds;
        fa.first_out = first_out;
        fa.decim = h->decim;
        ProfScope ps(h, PK_FRONT, st);
        if (h->nfftch == 0) h->front_name = "k_chan_front";
        if (launch_chan_front(fa, h->nin, rawf != nullptr, st) != JSDR_OK) return JSDR_ERR;
    }
    for (int c = 0; c < h->nch && nto_tune > 0; c++) {
        BpskChan &cc = h->chan[c];
        if (cc.seam != SEAM_TO_TUNE) continue;
        // the channel's first tune call after FFT-acquire frames: k_front_split over its streams (one per input), the double history
        // of its FFT state rows (I == Q, unmixed) in the raw one's place, its dm rows addressed as the per-channel FFT launches
        // address them
        if (nds > 0) {
            FrontArgs fs;
            fs.raw = raw;
            fs.rawf = rawf;
            fs.stride_pairs = stride_pairs;
            fs.nsamples = L;
            fs.ic = ic;
            fs.qc = qc;
            fs.mix = 1;
            fs.ktu = nullptr;
            fs.kvco = h->kvco.p;
            fs.sincos = h->sincos.p;
            fs.hist = h->hist_in[h->hist_cur].p;
            fs.dm = h->dm.p + (long long)c * h->dm_stride;
            fs.dm_stride = h->dm_stride * h->nch;
            fs.ds_dbg = nullptr;
            fs.nds = nds;
            fs.first_out = first_out;
            fs.tcs = nullptr;
            fs.tper = 0;
            ProfScope ps(h, PK_FRONT, st);
            if (h->nfftch == 0 && h->nch == nto_tune) h->front_name = "k_front_split";
            if (launch_front_split(fs, cc.dev.p, h->sincos9.p, h->decim, h->fft_state.p + (size_t)c * (size_t)h->nin, h->nin, st) != JSDR_OK)
                return JSDR_ERR;
        }
        cc.sched.valid = false;  // (its device slot holds this call's table, not the cached schedule's)
    }
    for (int c = 0; c < h->nch; c++) h->chan[c].seam = SEAM_NONE;  // every pending seam has been carried
    if (run_hist_in(h, hist_args(h, raw, rawf, stride_pairs, L, ic, qc, h->nin), st) != JSDR_OK) return JSDR_ERR;  // per input
    const int yb = h->y_cur;
    if (wait_tail(h, yb, st) != JSDR_OK) return JSDR_ERR;
    if (nds > 0 && run_matched(h, yb, nds, g_first, st) != JSDR_OK) return JSDR_ERR;
    if (finish_call(h, yb, L, nds, g_first, first_out, ic, qc, raw, stride_pairs, h->kvco.p, h->tcs.p, st) != JSDR_OK) return JSDR_ERR;
    h->tuPhase = h->chan[0].tuPhase;
    return JSDR_OK;
}
