// bpsk_control.hip -- live control of a jsdr_bpsk handle between two calls: tuning and mode of an ordinary, a channel and a
// tuned handle, per-stream tunings, tuning plans, and the host forms of the tuner walk.  Host code only (bpsk_handle.h).
#include "bpsk_handle.h"
#include <cmath>

// ------------------------------------------------------------------------------------------- live control
// FUNcubeBPSKDemod.actionPerformed (:177-190) between two calls.  Every check comes first: a refused call leaves the handle
// exactly as it was.  Then the handle's own work is waited for (the previous call's tail and FEC on the side stream finish
// with the settings they were launched with), the schedule prefetch is joined, and dmMaxCorr is zeroed in every stream.
// tuPhase, the down-sampler and matched-filter histories, vcoPhase, the tail state, the FEC register and the counters carry on.
// The schedules need no word from here: their keys hold tuPhaseInc and the mode, so one computed for the old settings does
// not match the next call.  The device copy of the tables is marked stale, which makes that call send its own.
int bpsk_live_check(jsdr_bpsk *h, int do_fft, const char *who)
{
    JSDR_REQUIRE(h, "%s: null handle", who);
    JSDR_REQUIRE(h->variant == JSDR_VARIANT_EXACT,
                 "%s: the fast variant has no live control (jsdr_bpsk_recover_uncertified replays from creation)", who);
    JSDR_REQUIRE(!(h->pst_nch > 0 && do_fft > 0), "%s: a tuned channel handle (jsdr_bpsk_create_tuned_channels) runs in the tune mode only; the "
                 "handle is unchanged", who);
    JSDR_REQUIRE(!(h->pst && do_fft > 0), "%s: a tuned handle (jsdr_bpsk_create_tuned) runs in the tune mode only; the handle is unchanged", who);
    if (do_fft > 0 && !h->do_fft) {
        JSDR_REQUIRE(fft_front_kind(h->nsf, h->decim, false) != FRONT_NONE, "%s: FFT-acquire mode cannot take this handle's frame size (%d "
                     "samples: it needs 416 .. 4194304 samples whose prime factors r above 7 keep n r within 2^31); the handle is unchanged",
                     who, h->nsf);
    }
    return JSDR_OK;
}

static int live_apply(jsdr_bpsk *h, double tuning, int do_fft, int do_up, bool zero_maxcorr)
{
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    if (h->worker.joinable()) h->worker.join();
    hipStream_t st = h->last_stream;
    // the one step that can fail comes first: nothing of the handle has changed when it does
    if (zero_maxcorr) {
        if (launch_reset_maxcorr(h->tail.p, h->nstreams, st) != JSDR_OK) return JSDR_ERR;  // :190
        JSDR_HIP_TRY(hipStreamSynchronize(st));
    }
    if (h->do_fft && (do_up != h->do_up || !do_fft) && h->acq_scratch.p) {
        // the three-phase scratch holds a frame's spectrum band, whose width depends on doUp: re-cut it into frames of the
        // new size, or drop it to be allocated again at the next call that needs it
        const size_t per = acq3_frame_bytes(h->nsf, do_up) + 64 + (h->fft_plan.kind == FRONT_GEN ? acqg_image_bytes(h->nsf) : 0);
        const long long chunk = (long long)((h->acq_scratch.n - 512) / (per * (size_t)h->nstreams));
        if (chunk >= 1) {
            h->acq_chunk = (int)(chunk < h->acq_chunk ? chunk : h->acq_chunk);
        } else {
            h->acq_scratch.release();
            h->acq_chunk = 0;
        }
    }
    if (do_fft != h->do_fft) {
        // the first call in the new mode carries the seam; a switch back before any call cancels it
        const int want = do_fft ? SEAM_TO_FFT : SEAM_TO_TUNE;
        h->seam = h->seam != SEAM_NONE ? SEAM_NONE : want;
        h->do_fft = do_fft;
    }
    h->tuning = tuning;
    h->do_up = do_up;
    h->tuPhaseInc = tuner_inc(tuning, h->rate);  // :189
    h->retuned = true;
    h->tables_on_device = false;
    return JSDR_OK;
}

// a channel's mode is fixed at creation: what a mode request for channel `ch` (-1: every channel) of a channel handle must match
static int chan_mode_check(jsdr_bpsk *h, int ch, int do_fft, const char *who)
{
    if (h->mode_chan)
        for (int c = 0; c < h->nch; c++)
            JSDR_REQUIRE((ch >= 0 && c != ch) || (do_fft != 0) == (h->chan[c].do_fft != 0), "%s: channel %d was created in %s; a channel's "
                         "mode is fixed at creation; the handle is unchanged", who, c, h->chan[c].do_fft ? "FFT-acquire" : "the tune mode");
    JSDR_REQUIRE(h->mode_chan || !do_fft, "%s: a channel handle runs in the tune mode only; the handle is unchanged", who);
    return JSDR_OK;
}

// do_fft (a live channel handle only, jsdr_bpsk_create_live_channels): the "FFT/Tune" action (:180-186) on the channels it changes
static int chan_apply(jsdr_bpsk *h, int ch, const double *tuning, const int *do_up, bool zero_maxcorr, const char *who,
                      const int *do_fft = nullptr)
{
    JSDR_REQUIRE(ch >= -1 && ch < h->nch, "%s: channel %d out of range (the handle has %d); the handle is unchanged", who, ch, h->nch);
    JSDR_REQUIRE(!tuning || std::isfinite(*tuning), "%s: tuning %g Hz is not finite; the handle is unchanged", who, tuning ? *tuning : 0.0);
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    if (h->live_chan && h->acq_scratch.p) {
        // the three-phase scratch is cut for the bands in use, which "FFT/Tune" and "Track high" may change: re-cut now, before
        // anything of the handle has changed -- if that cannot be had the action is refused
        int mask = 0;
        for (int c = 0; c < h->nch; c++) {
            const bool acted = ch < 0 || c == ch;
            const int f = (acted && do_fft) ? *do_fft : h->chan[c].do_fft;
            const int u = (acted && do_up) ? *do_up : h->chan[c].do_up;
            if (f) mask |= u ? 2 : 1;
        }
        if (mask != h->acq_mask) {
            h->acq_scratch.release();  // (never both: the scratch is the handle's largest buffer)
            h->acq_chunk = 0;
            if (mask != 0) {
                if (acq_scratch_ensure(h, acq3c_frame_bytes(h->nsf, mask, h->fft_plan.kind == FRONT_GEN), (size_t)h->nin, 4096) != JSDR_OK) {
                    set_error("%s: the FFT-acquire scratch could not be cut again for the bands in use; the handle is unchanged (its next "
                              "call allocates the scratch anew)", who);
                    return JSDR_ERR;
                }
                h->acq_mask = mask;
            }
        }
    }
    if (zero_maxcorr) {
        hipStream_t st = h->last_stream;
        if (launch_reset_maxcorr_chan(h->tail.p, h->nin, h->nch, ch, st) != JSDR_OK) return JSDR_ERR;
        JSDR_HIP_TRY(hipStreamSynchronize(st));
    }
    for (int c = 0; c < h->nch; c++) {
        if (ch >= 0 && c != ch) continue;
        BpskChan &cc = h->chan[c];
        if (tuning) {
            cc.tuning = *tuning;
            cc.tuPhaseInc = tuner_inc(*tuning, h->rate);  // :189
        }
        if (do_up) cc.do_up = *do_up;
        if (do_fft && (*do_fft != 0) != (cc.do_fft != 0)) {
            // the channel's first call in the new mode carries the seam; a switch back before any call cancels it.  tuPhase stands
            // still while the channel acquires and carries on from there
            const int want = *do_fft ? SEAM_TO_FFT : SEAM_TO_TUNE;
            cc.seam = cc.seam != SEAM_NONE ? SEAM_NONE : want;
            cc.do_fft = *do_fft ? 1 : 0;
        }
    }
    if (do_fft) {
        h->nfftch = 0;
        for (int c = 0; c < h->nch; c++) h->nfftch += h->chan[c].do_fft ? 1 : 0;
    }
    if (!h->live_chan && do_up && h->nfftch > 0 && h->acq_scratch.p) {
        // the three-phase scratch is cut for the bands in use ("Track high" on an FFT-acquire channel may change them): allocated
        // again at the next call
        h->acq_scratch.release();
        h->acq_chunk = 0;
    }
    h->tuning = h->chan[0].tuning;
    h->tuPhaseInc = h->chan[0].tuPhaseInc;
    h->do_up = h->chan[0].do_up;
    h->retuned = true;
    return JSDR_OK;
}

// A tuned handle (jsdr_bpsk_create_tuned): the tunings it takes.  At tuning >= rate tuPhaseInc >= 2 pi: the single subtraction of
// :385 no longer bounds tuPhase, and (int) of the table index leaves the range in which the host's and the device's casts agree.
static int pst_tuning_check(const jsdr_bpsk *h, const double *tunings, int count, int first, const char *who)
{
    for (int i = 0; i < count; i++)
        JSDR_REQUIRE(std::isfinite(tunings[i]) && tunings[i] < (double)h->rate, "%s: tuning %g Hz of stream %d is not a finite value below "
                     "the rate (%d Hz); the handle is unchanged", who, tunings[i], first + i, h->rate);
    return JSDR_OK;
}

// actionPerformed's tuning change (:177-190) on the streams first .. first + count - 1 of a tuned handle, after the handle's
// pending work: tuning, tuPhaseInc = 2 pi tuning / rate (:189) and, for an action, dmMaxCorr = 0 (:190) in those streams.  Their
// tuPhase, the indices their last 26 samples were mixed with and every other piece of state carry on; the other streams are not
// touched.  tunings: one value a stream, or null: `one` for all of them.  Every value has been checked by the caller.
static int pst_apply(jsdr_bpsk *h, int first, int count, const double *tunings, double one, bool zero_maxcorr)
{
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    std::vector<double> inc((size_t)count);
    for (int i = 0; i < count; i++) inc[(size_t)i] = tuner_inc(tunings ? tunings[i] : one, h->rate);  // :189
    if (zero_maxcorr) {
        std::vector<int> ids((size_t)count);
        for (int i = 0; i < count; i++) ids[(size_t)i] = first + i;
        hipStream_t st = h->last_stream;
        JSDR_HIP_TRY(hipMemcpy(h->pst_ids.p, ids.data(), sizeof(int) * (size_t)count, hipMemcpyHostToDevice));
        if (launch_reset_maxcorr_list(h->tail.p, h->pst_ids.p, count, st) != JSDR_OK) return JSDR_ERR;  // one launch, whatever the count
        JSDR_HIP_TRY(hipStreamSynchronize(st));
    }
    JSDR_HIP_TRY(hipMemcpy(h->pst_inc.p + first, inc.data(), sizeof(double) * (size_t)count, hipMemcpyHostToDevice));
    for (int i = 0; i < count; i++) h->pst_tuning[(size_t)(first + i)] = tunings ? tunings[i] : one;
    return JSDR_OK;
}

int jsdr_bpsk_set_variant(jsdr_bpsk *h, int variant)
{
    JSDR_REQUIRE(h, "jsdr_bpsk_set_variant: null handle");
    JSDR_REQUIRE(variant == JSDR_VARIANT_EXACT || variant == JSDR_VARIANT_FAST, "jsdr_bpsk_set_variant: unknown variant %d", variant);
    JSDR_REQUIRE(variant == JSDR_VARIANT_EXACT || h->nch == 0, "jsdr_bpsk_set_variant: a channel handle has no fast variant");
    JSDR_REQUIRE(variant == JSDR_VARIANT_EXACT || h->pst_nch == 0, "jsdr_bpsk_set_variant: a tuned channel handle "
                 "(jsdr_bpsk_create_tuned_channels) has no fast variant; the handle is unchanged");
    JSDR_REQUIRE(variant == JSDR_VARIANT_EXACT || !h->pst, "jsdr_bpsk_set_variant: a tuned handle has no fast variant");
    JSDR_REQUIRE(h->n_in == 0, "jsdr_bpsk_set_variant: the variant is fixed once samples have been received");
    JSDR_REQUIRE(variant == JSDR_VARIANT_EXACT || !h->do_fft, "jsdr_bpsk_set_variant: the fast variant covers the tune mode only");
    JSDR_REQUIRE(variant == JSDR_VARIANT_EXACT || !h->retuned, "jsdr_bpsk_set_variant: the fast variant has no live control, and this handle was retuned");
    h->variant = variant;
    return JSDR_OK;
}

int jsdr_bpsk_set_tuning(jsdr_bpsk *h, double tuning_hz)
{
    if (bpsk_live_check(h, -1, "jsdr_bpsk_set_tuning") != JSDR_OK) return JSDR_ERR;
    if (h->pst) {  // every stream
        if (pst_tuning_check(h, &tuning_hz, 1, 0, "jsdr_bpsk_set_tuning") != JSDR_OK) return JSDR_ERR;
        return pst_apply(h, 0, h->nstreams, nullptr, tuning_hz, true);
    }
    JSDR_REQUIRE(std::isfinite(tuning_hz), "jsdr_bpsk_set_tuning: tuning %g Hz is not finite", tuning_hz);
    if (h->nch > 0) return chan_apply(h, -1, &tuning_hz, nullptr, true, "jsdr_bpsk_set_tuning");
    return live_apply(h, tuning_hz, h->do_fft, h->do_up, true);
}

int jsdr_bpsk_set_mode(jsdr_bpsk *h, int do_fft, int do_up)
{
    if (bpsk_live_check(h, do_fft != 0, "jsdr_bpsk_set_mode") != JSDR_OK) return JSDR_ERR;
    if (h->nch > 0) {
        if (!h->live_chan && chan_mode_check(h, -1, do_fft, "jsdr_bpsk_set_mode") != JSDR_OK) return JSDR_ERR;
        const int up = do_up != 0, fft = do_fft != 0;
        return chan_apply(h, -1, nullptr, &up, true, "jsdr_bpsk_set_mode", h->live_chan ? &fft : nullptr);
    }
    if (do_fft && !h->do_fft && fft_mode_alloc(h, fft_front_kind(h->nsf, h->decim, false), true) != JSDR_OK) return JSDR_ERR;
    return live_apply(h, h->tuning, do_fft != 0, do_up != 0, true);
}

int jsdr_bpsk_reconfigure(jsdr_bpsk *h, double tuning_hz, int do_fft, int do_up)
{
    if (bpsk_live_check(h, do_fft != 0, "jsdr_bpsk_reconfigure") != JSDR_OK) return JSDR_ERR;
    if (h->pst) {  // setup() on every stream: the tuning, doUp stored, dmMaxCorr kept
        if (pst_tuning_check(h, &tuning_hz, 1, 0, "jsdr_bpsk_reconfigure") != JSDR_OK) return JSDR_ERR;
        if (pst_apply(h, 0, h->nstreams, nullptr, tuning_hz, false) != JSDR_OK) return JSDR_ERR;
        h->do_up = do_up != 0;
        return JSDR_OK;
    }
    JSDR_REQUIRE(std::isfinite(tuning_hz), "jsdr_bpsk_reconfigure: tuning %g Hz is not finite", tuning_hz);
    if (h->nch > 0) {
        if (!h->live_chan && chan_mode_check(h, -1, do_fft, "jsdr_bpsk_reconfigure") != JSDR_OK) return JSDR_ERR;
        const int up = do_up != 0, fft = do_fft != 0;
        return chan_apply(h, -1, &tuning_hz, &up, false, "jsdr_bpsk_reconfigure", h->live_chan ? &fft : nullptr);
    }
    if (do_fft && !h->do_fft && fft_mode_alloc(h, fft_front_kind(h->nsf, h->decim, false), true) != JSDR_OK) return JSDR_ERR;
    if (live_apply(h, tuning_hz, do_fft != 0, do_up != 0, false) != JSDR_OK) return JSDR_ERR;
    h->scope_origin = h->n_ds;  // setup() resets the debug rings' indices (:198-204): the scope counts its slots from here
    return JSDR_OK;
}

int jsdr_bpsk_get_control(jsdr_bpsk *h, double *tuning_hz, int *do_fft, int *do_up)
{
    JSDR_REQUIRE(h && tuning_hz && do_fft && do_up, "jsdr_bpsk_get_control: null argument");
    *tuning_hz = h->pst ? h->pst_tuning[0] : h->tuning;    // (a tuned handle reports stream 0)
    *do_fft = h->nch > 0 ? h->chan[0].do_fft : h->do_fft;  // (a channel handle reports channel 0)
    *do_up = h->do_up;
    return JSDR_OK;
}

int jsdr_bpsk_set_channel_tuning(jsdr_bpsk *h, int channel, double tuning_hz)
{
    JSDR_REQUIRE(h, "jsdr_bpsk_set_channel_tuning: null handle");
    JSDR_REQUIRE(h->pst_nch == 0, "jsdr_bpsk_set_channel_tuning: the channels of a tuned channel handle (jsdr_bpsk_create_tuned_channels) are "
                 "tuned as streams, input * nchannels + channel (jsdr_bpsk_set_stream_tuning); the handle is unchanged");
    JSDR_REQUIRE(!h->pst, "jsdr_bpsk_set_channel_tuning: a tuned handle has streams, not channels (jsdr_bpsk_set_stream_tuning); the handle is unchanged");
    if (h->nch == 0) {  // an ordinary handle is one channel
        JSDR_REQUIRE(channel == 0, "jsdr_bpsk_set_channel_tuning: channel %d out of range (the handle has 1)", channel);
        return jsdr_bpsk_set_tuning(h, tuning_hz);
    }
    JSDR_REQUIRE(channel >= 0, "jsdr_bpsk_set_channel_tuning: channel %d out of range (the handle has %d); the handle is unchanged",
                 channel, h->nch);
    return chan_apply(h, channel, &tuning_hz, nullptr, true, "jsdr_bpsk_set_channel_tuning");
}

int jsdr_bpsk_set_channel_mode(jsdr_bpsk *h, int channel, int do_fft, int do_up)
{
    JSDR_REQUIRE(h, "jsdr_bpsk_set_channel_mode: null handle");
    JSDR_REQUIRE(h->pst_nch == 0, "jsdr_bpsk_set_channel_mode: the channels of a tuned channel handle (jsdr_bpsk_create_tuned_channels) are "
                 "streams in the tune mode (jsdr_bpsk_set_mode sets doUp on all of them); the handle is unchanged");
    JSDR_REQUIRE(!h->pst, "jsdr_bpsk_set_channel_mode: a tuned handle has streams, not channels (jsdr_bpsk_set_mode); the handle is unchanged");
    if (h->nch == 0) {
        JSDR_REQUIRE(channel == 0, "jsdr_bpsk_set_channel_mode: channel %d out of range (the handle has 1)", channel);
        return jsdr_bpsk_set_mode(h, do_fft, do_up);
    }
    JSDR_REQUIRE(channel >= 0 && channel < h->nch, "jsdr_bpsk_set_channel_mode: channel %d out of range (the handle has %d); the handle "
                 "is unchanged", channel, h->nch);
    if (!h->live_chan && chan_mode_check(h, channel, do_fft, "jsdr_bpsk_set_channel_mode") != JSDR_OK) return JSDR_ERR;
    const int up = do_up != 0, fft = do_fft != 0;
    return chan_apply(h, channel, nullptr, &up, true, "jsdr_bpsk_set_channel_mode", h->live_chan ? &fft : nullptr);
}

int jsdr_bpsk_get_channel_control(jsdr_bpsk *h, int channel, double *tuning_hz, int *do_fft, int *do_up)
{
    JSDR_REQUIRE(h && tuning_hz && do_fft && do_up, "jsdr_bpsk_get_channel_control: null argument");
    JSDR_REQUIRE(h->pst_nch == 0, "jsdr_bpsk_get_channel_control: the channels of a tuned channel handle (jsdr_bpsk_create_tuned_channels) "
                 "are streams, input * nchannels + channel (jsdr_bpsk_get_stream_tuning)");
    JSDR_REQUIRE(!h->pst, "jsdr_bpsk_get_channel_control: a tuned handle has streams, not channels (jsdr_bpsk_get_stream_tuning)");
    if (h->nch == 0) {
        JSDR_REQUIRE(channel == 0, "jsdr_bpsk_get_channel_control: channel %d out of range (the handle has 1)", channel);
        return jsdr_bpsk_get_control(h, tuning_hz, do_fft, do_up);
    }
    JSDR_REQUIRE(channel >= 0 && channel < h->nch, "jsdr_bpsk_get_channel_control: channel %d out of range (the handle has %d)", channel,
                 h->nch);
    *tuning_hz = h->chan[channel].tuning;
    *do_fft = h->chan[channel].do_fft;
    *do_up = h->chan[channel].do_up;
    return JSDR_OK;
}

int jsdr_bpsk_set_stream_tunings(jsdr_bpsk *h, int first, int count, const double *tuning_hz)
{
    if (bpsk_live_check(h, -1, "jsdr_bpsk_set_stream_tunings") != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(h->pst, "jsdr_bpsk_set_stream_tunings: the handle was not made by jsdr_bpsk_create_tuned (its streams share one tuning: "
                 "jsdr_bpsk_set_tuning); the handle is unchanged");
    JSDR_REQUIRE(tuning_hz, "jsdr_bpsk_set_stream_tunings: null tuning array");
    JSDR_REQUIRE(first >= 0 && count >= 1 && first < h->nstreams && count <= h->nstreams - first, "jsdr_bpsk_set_stream_tunings: streams %d .. "
                 "%lld out of range (the handle has %d); the handle is unchanged", first, (long long)first + count - 1, h->nstreams);
    if (pst_tuning_check(h, tuning_hz, count, first, "jsdr_bpsk_set_stream_tunings") != JSDR_OK) return JSDR_ERR;  // every value before any is applied
    return pst_apply(h, first, count, tuning_hz, 0.0, true);
}

int jsdr_bpsk_set_stream_tuning(jsdr_bpsk *h, int stream, double tuning_hz)
{
    if (bpsk_live_check(h, -1, "jsdr_bpsk_set_stream_tuning") != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(h->pst, "jsdr_bpsk_set_stream_tuning: the handle was not made by jsdr_bpsk_create_tuned (its streams share one tuning: "
                 "jsdr_bpsk_set_tuning); the handle is unchanged");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_bpsk_set_stream_tuning: stream %d out of range (the handle has %d); the handle "
                 "is unchanged", stream, h->nstreams);
    if (pst_tuning_check(h, &tuning_hz, 1, stream, "jsdr_bpsk_set_stream_tuning") != JSDR_OK) return JSDR_ERR;
    return pst_apply(h, stream, 1, &tuning_hz, 0.0, true);
}

int jsdr_bpsk_get_stream_tuning(jsdr_bpsk *h, int stream, double *tuning_hz)
{
    JSDR_REQUIRE(h && tuning_hz, "jsdr_bpsk_get_stream_tuning: null argument");
    JSDR_REQUIRE(h->pst, "jsdr_bpsk_get_stream_tuning: the handle was not made by jsdr_bpsk_create_tuned (jsdr_bpsk_get_control reports its "
                 "one tuning)");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_bpsk_get_stream_tuning: stream %d out of range (the handle has %d)", stream,
                 h->nstreams);
    *tuning_hz = h->pst_tuning[(size_t)stream];
    return JSDR_OK;
}

// A tuning plan: entry i says "from sample at_sample[i] of the NEXT batch call on, stream stream[i] has tuning tuning_hz[i]" --
// setup()'s tuning change (:192-209, what jsdr_bpsk_reconfigure applies between calls) at a sample of the stream's own -- and,
// given with slopes (jsdr_bpsk_plan_stream_ramps), "... moving on by slope_hz_per_sample[i] a sample" (tuner_ramp_tuning).  Every
// check comes before any device work; then the handle's pending work is waited for (the call before may still read the plan it
// took) and the plan goes to the device in buffers of its own, which take the old ones' place only once all of it is there.
// slope: null for steps.  Slopes that are all zero are steps too, and go the steps' way.
static int pst_plan_give(jsdr_bpsk *h, const char *who, const int32_t *stream, const int64_t *at_sample, const double *tuning_hz,
                         const double *slope, bool with_slopes, int64_t n)
{
    JSDR_REQUIRE(h, "%s: null handle", who);
    JSDR_REQUIRE(h->pst, "%s: the handle was not made by jsdr_bpsk_create_tuned (its streams share one tuning: jsdr_bpsk_reconfigure between "
                 "calls); the handle is unchanged", who);
    JSDR_REQUIRE(n >= 0, "%s: %lld entries; the handle and its pending plan are unchanged", who, (long long)n);
    JSDR_REQUIRE(n == 0 || (stream && at_sample && tuning_hz && (slope || !with_slopes)), "%s: null array with %lld entries; the handle and its "
                 "pending plan are unchanged", who, (long long)n);
    const int S = h->nstreams;
    bool ramp = false;
    for (int64_t i = 0; i < n; i++) {
        JSDR_REQUIRE(stream[i] >= 0 && stream[i] < S, "%s: entry %lld: stream %d out of range (the handle has %d); the handle and its pending "
                     "plan are unchanged", who, (long long)i, (int)stream[i], S);
        JSDR_REQUIRE(at_sample[i] >= 0, "%s: entry %lld: at_sample %lld is negative; the handle and its pending plan are unchanged", who,
                     (long long)i, (long long)at_sample[i]);
        JSDR_REQUIRE(i == 0 || stream[i] > stream[i - 1] || (stream[i] == stream[i - 1] && at_sample[i] > at_sample[i - 1]),
                     "%s: entry %lld (stream %d, sample %lld) is out of order: entries go by stream, and within a stream by strictly ascending "
                     "at_sample; the handle and its pending plan are unchanged", who, (long long)i, (int)stream[i], (long long)at_sample[i]);
        JSDR_REQUIRE(std::isfinite(tuning_hz[i]) && tuning_hz[i] < (double)h->rate, "%s: entry %lld: tuning %g Hz of stream %d is not a finite "
                     "value below the rate (%d Hz); the handle and its pending plan are unchanged", who, (long long)i, tuning_hz[i],
                     (int)stream[i], h->rate);
        if (!with_slopes) continue;
        JSDR_REQUIRE(std::isfinite(slope[i]), "%s: entry %lld: slope %g Hz per sample of stream %d is not finite; the handle and its pending "
                     "plan are unchanged", who, (long long)i, slope[i], (int)stream[i]);
        ramp = ramp || slope[i] != 0.0;
        // the tunings of a ramp are monotone in the sample (rounding is), and its first is the entry's: the one in front of the
        // stream's next entry decides here; a ramp that runs to the call's end is checked at the call, which knows where that is
        if (i > 0 && stream[i] == stream[i - 1]) {
            const double t_end = tuner_ramp_tuning(tuning_hz[i - 1], slope[i - 1], (long long)(at_sample[i] - 1 - at_sample[i - 1]));
            JSDR_REQUIRE(std::isfinite(t_end) && t_end < (double)h->rate, "%s: entry %lld: the ramp of stream %d reaches %g Hz at sample %lld, in "
                         "front of its next entry, not a finite value below the rate (%d Hz); the handle and its pending plan are unchanged", who,
                         (long long)(i - 1), (int)stream[i], t_end, (long long)(at_sample[i] - 1), h->rate);
        }
    }
    std::vector<long long> off((size_t)S + 1, 0), pos((size_t)n);
    std::vector<double> inc((size_t)(ramp ? 0 : n));
    std::vector<PstPlanLast> last;
    long long max_at = -1;
    for (int64_t i = 0; i < n; i++) {
        off[(size_t)stream[i] + 1]++;
        pos[(size_t)i] = at_sample[i];
        if (!ramp) inc[(size_t)i] = tuner_inc(tuning_hz[i], h->rate);  // :196, the double pst_apply writes
        if (at_sample[i] > max_at) max_at = at_sample[i];
        const PstPlanLast pl = {(int)stream[i], (long long)i, (long long)at_sample[i], tuning_hz[i], ramp ? slope[i] : 0.0};
        if (!last.empty() && last.back().stream == stream[i])
            last.back() = pl;
        else
            last.push_back(pl);
    }
    for (int s = 0; s < S; s++) {
        JSDR_REQUIRE(off[(size_t)s + 1] <= 0x7fffffffLL, "%s: %lld entries for stream %d; the handle and its pending plan are unchanged", who,
                     off[(size_t)s + 1], s);
        off[(size_t)s + 1] += off[(size_t)s];
    }
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    DevBuf<long long> d_off, d_pos;
    DevBuf<double> d_inc, d_tun, d_slope, d_inc0;
    DevBuf<int> d_cke;
    const bool first = n > 0 && !h->pst_inc0.p;  // (what the planned walk leaves for the planned front end: with the first plan)
    if (n > 0) {  // (none: the next call is an ordinary one, and the old plan's buffers go)
        if (d_off.alloc(off.size()) != JSDR_OK || d_pos.alloc(pos.size()) != JSDR_OK) return JSDR_ERR;
        if (ramp ? d_tun.alloc((size_t)n) != JSDR_OK || d_slope.alloc((size_t)n) != JSDR_OK : d_inc.alloc(inc.size()) != JSDR_OK) return JSDR_ERR;
        if (first && (d_inc0.alloc((size_t)S) != JSDR_OK || d_cke.alloc((size_t)S * (size_t)h->pst_ckpt_stride) != JSDR_OK)) return JSDR_ERR;
        JSDR_HIP_TRY(hipMemcpy(d_off.p, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice));
        JSDR_HIP_TRY(hipMemcpy(d_pos.p, pos.data(), sizeof(long long) * pos.size(), hipMemcpyHostToDevice));
        if (ramp) {
            JSDR_HIP_TRY(hipMemcpy(d_tun.p, tuning_hz, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
            JSDR_HIP_TRY(hipMemcpy(d_slope.p, slope, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
        } else {
            JSDR_HIP_TRY(hipMemcpy(d_inc.p, inc.data(), sizeof(double) * inc.size(), hipMemcpyHostToDevice));
        }
    }
    std::swap(h->pst_plan_off, d_off);  // (the old plan's buffers go with the locals, those of the other kind for empty ones)
    std::swap(h->pst_plan_pos, d_pos);
    std::swap(h->pst_plan_inc, d_inc);
    std::swap(h->pst_plan_tun, d_tun);
    std::swap(h->pst_plan_slope, d_slope);
    if (first) {
        std::swap(h->pst_inc0, d_inc0);
        std::swap(h->pst_ckpt_e, d_cke);
    }
    pst_plan_clear(h);
    h->pst_plan_n = n;
    h->pst_plan_max_at = max_at;
    h->pst_plan_ramp = ramp;
    h->pst_plan_last.swap(last);
    return JSDR_OK;
}

int jsdr_bpsk_plan_stream_tunings(jsdr_bpsk *h, const int32_t *stream, const int64_t *at_sample, const double *tuning_hz, int64_t n)
{
    return pst_plan_give(h, "jsdr_bpsk_plan_stream_tunings", stream, at_sample, tuning_hz, nullptr, false, n);
}

int jsdr_bpsk_plan_stream_ramps(jsdr_bpsk *h, const int32_t *stream, const int64_t *at_sample, const double *tuning_hz,
                                const double *slope_hz_per_sample, int64_t n)
{
    return pst_plan_give(h, "jsdr_bpsk_plan_stream_ramps", stream, at_sample, tuning_hz, slope_hz_per_sample, true, n);
}

int jsdr_bpsk_planned_tunings(jsdr_bpsk *h, int64_t *n)
{
    JSDR_REQUIRE(h && n, "jsdr_bpsk_planned_tunings: null argument");
    JSDR_REQUIRE(h->pst, "jsdr_bpsk_planned_tunings: the handle was not made by jsdr_bpsk_create_tuned");
    *n = h->pst_plan_n;
    return JSDR_OK;
}

// host only, no device: jsdr_bpsk_tuner_walk_host with a plan for one stream -- from sample at_sample[e] on the increment is
// inc_at[e] (the advance of that sample is the first at it); entries at or behind sample n are not reached
int jsdr_bpsk_tuner_walk_plan_host(double tu0, double tu_inc, int64_t n, const int64_t *at_sample, const double *inc_at, int64_t nev,
                                   uint16_t *k9_out, double *tu_end)
{
    static const char *who = "jsdr_bpsk_tuner_walk_plan_host";
    JSDR_REQUIRE(n >= 0 && (k9_out || n == 0), "%s: %lld samples, index buffer %s", who, (long long)n, k9_out ? "given" : "null");
    JSDR_REQUIRE(nev >= 0 && (nev == 0 || (at_sample && inc_at)), "%s: %lld entries, arrays %s", who, (long long)nev,
                 at_sample && inc_at ? "given" : "null");
    for (int64_t e = 0; e < nev; e++)
        JSDR_REQUIRE(at_sample[e] >= 0 && (e == 0 || at_sample[e] > at_sample[e - 1]), "%s: entry %lld (sample %lld) is negative or out of order",
                     who, (long long)e, (long long)at_sample[e]);
    double tu = tu0, inc = tu_inc;
    int64_t e = 0;
    for (int64_t i = 0; i < n; i++) {
        if (e < nev && at_sample[e] == i) inc = inc_at[e++];
        k9_out[i] = (uint16_t)tuner_step(tu, inc);
    }
    if (tu_end) *tu_end = tu;
    return JSDR_OK;
}

// host only, no device: jsdr_bpsk_tuner_walk_plan_host with ramp entries -- from sample at_sample[e] on, sample i has the tuning
// tuner_ramp_tuning(tuning_at[e], slope_at[e], i - at_sample[e]) and advances by tuner_inc of it, as the ramp forms of the two
// kernels step it; tu_end / inc_end: tuPhase and tuPhaseInc after sample n - 1
int jsdr_bpsk_tuner_walk_ramp_host(double tu0, double tu_inc, int64_t n, int rate, const int64_t *at_sample, const double *tuning_at,
                                   const double *slope_at, int64_t nev, uint16_t *k9_out, double *tu_end, double *inc_end)
{
    static const char *who = "jsdr_bpsk_tuner_walk_ramp_host";
    JSDR_REQUIRE(n >= 0 && (k9_out || n == 0), "%s: %lld samples, index buffer %s", who, (long long)n, k9_out ? "given" : "null");
    JSDR_REQUIRE(rate >= 1, "%s: rate %d", who, rate);
    JSDR_REQUIRE(nev >= 0 && (nev == 0 || (at_sample && tuning_at && slope_at)), "%s: %lld entries, arrays %s", who, (long long)nev,
                 at_sample && tuning_at && slope_at ? "given" : "null");
    for (int64_t e = 0; e < nev; e++)
        JSDR_REQUIRE(at_sample[e] >= 0 && (e == 0 || at_sample[e] > at_sample[e - 1]), "%s: entry %lld (sample %lld) is negative or out of order",
                     who, (long long)e, (long long)at_sample[e]);
    double tu = tu0, inc = tu_inc;
    int64_t e = 0;
    bool on = false;  // an entry is in effect: e - 1
    for (int64_t i = 0; i < n; i++) {
        if (e < nev && at_sample[e] == i) on = true, e++;
        if (on) inc = tuner_ramp_inc(tuning_at[e - 1], slope_at[e - 1], (long long)(i - at_sample[e - 1]), (double)rate);
        k9_out[i] = (uint16_t)tuner_step(tu, inc);
    }
    if (tu_end) *tu_end = tu;
    if (inc_end) *inc_end = inc;
    return JSDR_OK;
}

// host only, no device: the tuner recurrence exactly as k_tuner_walk and k_front_pst walk it (bpsk_tuner.h) -- n samples from
// tuPhase tu0 at tuPhaseInc tu_inc: the 9-bit table index of every sample (256: passed through) and tuPhase at the end
int jsdr_bpsk_tuner_walk_host(double tu0, double tu_inc, int64_t n, uint16_t *k9_out, double *tu_end)
{
    JSDR_REQUIRE(n >= 0 && (k9_out || n == 0), "jsdr_bpsk_tuner_walk_host: %lld samples, index buffer %s", (long long)n, k9_out ? "given" : "null");
    double tu = tu0;
    for (int64_t i = 0; i < n; i++) k9_out[i] = (uint16_t)tuner_step(tu, tu_inc);
    if (tu_end) *tu_end = tu;
    return JSDR_OK;
}
