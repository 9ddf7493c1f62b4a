// demod_control.hip -- a demod handle (demod_handle.h) between calls: jsdr_demod_create / _create_channels and _destroy,
// configure and weights for every receiver or for one channel, the channel accessors, frame_stats and the profile entry
// points.  Host code only.
#include "demod_handle.h"

namespace jsdr {

// What both kinds of handle hold, allocated for a handle whose shape (rate, n, nin, nch, nstreams, max_batch, nco_pitch) is
// set: `tab` phases (nco_spare (cos, sin) pairs more) per carrier-table set; d_up_front: the [S][L] float rows now (an ordinary
// handle; a channel handle's dch grows with the calls); clear_events: the two events of channel_weights' asynchronous clear.
// *out on success, nothing left behind otherwise.
static int demod_create_body(jsdr_demod **out, jsdr_demod *h, size_t tab, size_t nco_spare, bool d_up_front, bool clear_events)
{
    h->ch.resize((size_t)h->nch);
    const size_t S = (size_t)h->nstreams, L = (size_t)h->max_batch, nf = S * (L / (size_t)h->n);
    bool ok = true;
    for (int k = 0; k < 2; k++)
        ok = ok && h->hist[k].alloc(S * DHALO) == JSDR_OK && h->lilq[k].alloc(S) == JSDR_OK && h->hist[k].zero() == JSDR_OK &&
             h->lilq[k].zero() == JSDR_OK;
    for (int k = 0; k < 2; k++)
        ok = ok && h->nco[k].alloc(tab + nco_spare) == JSDR_OK && h->nco[k].zero() == JSDR_OK && h->car_dev[k].alloc(tab) == JSDR_OK &&
             h->car_pinned[k].alloc(sizeof(float) * tab) && h->ev_table[k].create(hipEventDisableTiming) == JSDR_OK &&
             h->ev_used[k].create(hipEventDisableTiming) == JSDR_OK;
    ok = ok && h->copy_stream.create(hipStreamNonBlocking) == JSDR_OK;
    if (clear_events) ok = ok && h->ev_done.create(hipEventDisableTiming) == JSDR_OK && h->ev_clear.create(hipEventDisableTiming) == JSDR_OK;
    if (d_up_front) ok = ok && h->d.alloc(S * L) == JSDR_OK;
    ok = ok && h->favg.alloc(nf) == JSDR_OK && h->stats.alloc(2 * nf) == JSDR_OK && h->fmax.alloc(nf) == JSDR_OK &&
         h->stage_in.alloc(2 * (size_t)h->n) == JSDR_OK && h->stage_out.alloc((size_t)h->n * h->nch) == JSDR_OK &&
         h->favg.zero() == JSDR_OK && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        jsdr_demod_destroy(h);
        return JSDR_ERR;
    }
    *out = h;
    return JSDR_OK;
}

}  // namespace jsdr

extern "C" {

int jsdr_demod_create(jsdr_demod **out, int rate, int nsamples_per_frame, int nstreams, int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_demod_create: null handle pointer");
    *out = nullptr;
    JSDR_REQUIRE(rate > 0 && nsamples_per_frame > 0 && nstreams > 0, "jsdr_demod_create: rate, frame and nstreams must be positive");
    if (max_batch_samples <= 0) max_batch_samples = nsamples_per_frame;
    JSDR_REQUIRE(max_batch_samples % nsamples_per_frame == 0, "jsdr_demod_create: max_batch_samples must be whole frames");
    JSDR_REQUIRE(nstreams <= 65535 && max_batch_samples / nsamples_per_frame <= 65535,
                 "jsdr_demod_create: at most 65535 streams and 65535 frames per call");
    JSDR_REQUIRE((long long)nstreams * (max_batch_samples / nsamples_per_frame) < (1LL << 31) &&
                     (max_batch_samples / nsamples_per_frame) * ((nsamples_per_frame + DTILE - 1) / DTILE) < (1LL << 31),
                 "jsdr_demod_create: batch too large");
    jsdr_demod *h = new jsdr_demod();
    h->rate = rate;
    h->n = nsamples_per_frame;
    h->nstreams = h->nin = nstreams;  // one channel an input
    h->max_batch = max_batch_samples;
    return demod_create_body(out, h, (size_t)max_batch_samples, 8, true, false);  // one table a set, spare slots past it
}

int jsdr_demod_create_channels(jsdr_demod **out, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                               int64_t max_batch_samples)
{
    JSDR_REQUIRE(out, "jsdr_demod_create_channels: null handle pointer");
    *out = nullptr;
    JSDR_REQUIRE(rate > 0 && nsamples_per_frame > 0, "jsdr_demod_create_channels: rate and nsamples_per_frame must be positive");
    JSDR_REQUIRE(ninputs >= 1, "jsdr_demod_create_channels: ninputs = %d, at least 1", ninputs);
    JSDR_REQUIRE(nchannels >= 1 && nchannels <= DCHAN_MAX, "jsdr_demod_create_channels: nchannels = %d outside 1..%d", nchannels,
                 (int)DCHAN_MAX);
    if (max_batch_samples <= 0) max_batch_samples = nsamples_per_frame;
    JSDR_REQUIRE(max_batch_samples % nsamples_per_frame == 0, "jsdr_demod_create_channels: max_batch_samples must be whole frames");
    const long long S = (long long)ninputs * nchannels, nf = max_batch_samples / nsamples_per_frame;
    JSDR_REQUIRE(S <= 65535, "jsdr_demod_create_channels: ninputs * nchannels = %lld streams, at most 65535", S);
    JSDR_REQUIRE(nf <= 65535, "jsdr_demod_create_channels: max_batch_samples is %lld frames, at most 65535", nf);
    JSDR_REQUIRE(S * nf < (1LL << 31) && nf * ((nsamples_per_frame + DTILE - 1) / DTILE) < (1LL << 31),
                 "jsdr_demod_create_channels: batch too large");
    jsdr_demod *h = new jsdr_demod();
    h->chan = true;
    h->rate = rate;
    h->n = nsamples_per_frame;
    h->nin = ninputs;
    h->nch = nchannels;
    h->nstreams = (int)S;
    h->max_batch = max_batch_samples;
    h->nco_pitch = (max_batch_samples + 8 + 1) & ~1LL;  // even: every table 16-byte aligned; spare slots past each
    return demod_create_body(out, h, (size_t)nchannels * (size_t)h->nco_pitch, 0, false, true);
}

int jsdr_demod_destroy(jsdr_demod *h)
{
    if (!h) return JSDR_OK;
    (void)hipDeviceSynchronize();
    delete h;
    return JSDR_OK;
}

int jsdr_demod_profile_enable(jsdr_demod *h, int on)
{
    JSDR_REQUIRE(h, "jsdr_demod_profile_enable: null handle");
    h->prof_on = on != 0;
    return JSDR_OK;
}
int jsdr_demod_profile_count(void) { return DK_COUNT; }
const char *jsdr_demod_profile_name(int k) { return (k >= 0 && k < DK_COUNT) ? kDemodKernels[k] : ""; }
int jsdr_demod_profile_read(jsdr_demod *h, double *ms_total, int *launches)
{
    JSDR_REQUIRE(h && ms_total && launches, "jsdr_demod_profile_read: null argument");
    for (int k = 0; k < DK_COUNT; k++) {
        ms_total[k] = 0.0;
        launches[k] = 0;
    }
    for (auto &r : h->recs) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            ms_total[r.k] += ms;
            launches[r.k]++;
        }
        h->pool.push_back(std::move(r.a));
        h->pool.push_back(std::move(r.b));
    }
    h->recs.clear();
    return JSDR_OK;
}

#define DEMOD_CHANNEL_OK(fn)                                                                                                   \
    JSDR_REQUIRE(h, fn ": null handle");                                                                                       \
    JSDR_REQUIRE(channel >= 0 && channel < h->nch, fn ": channel %d outside 0..%d", channel, h->nch - 1)

static void demod_configure_one(DemodCtl &c, int mode, int dofir, int dodwn, int doagc)
{
    c.mode = mode;
    c.dofir = dofir != 0;
    c.dodwn = dodwn != 0;
    c.doagc = doagc != 0;
}

int jsdr_demod_configure(jsdr_demod *h, int mode, int dofir, int dodwn, int doagc)
{
    JSDR_REQUIRE(h, "jsdr_demod_configure: null handle");
    JSDR_REQUIRE(mode >= MODE_OFF && mode <= MODE_WFM, "jsdr_demod_configure: mode %d outside 0..4 (demod.java:39-43)", mode);
    for (auto &c : h->ch) demod_configure_one(c, mode, dofir, dodwn, doagc);  // a channel handle: every channel
    return JSDR_OK;
}

int jsdr_demod_configure_channel(jsdr_demod *h, int channel, int mode, int dofir, int dodwn, int doagc)
{
    DEMOD_CHANNEL_OK("jsdr_demod_configure_channel");
    JSDR_REQUIRE(mode >= MODE_OFF && mode <= MODE_WFM, "jsdr_demod_configure_channel: mode %d outside 0..4 (demod.java:39-43)", mode);
    demod_configure_one(h->ch[channel], mode, dofir, dodwn, doagc);
    return JSDR_OK;
}

// demod.weights() (:341-375) of one receiver for the band; a band-pass (not the all-pass impulse) sets phi and restarts car
static void demod_band_of(DemodCtl &c, int rate, int flo, int fhi)
{
    c.flo = flo;
    c.fhi = fhi;
    if (demod_weights_of(rate, flo, fhi, c.w, &c.phi)) c.car = 0.0f;
}

// weights() for every channel; clears the delay lines of every stream, between device syncs
int jsdr_demod_weights(jsdr_demod *h, int flo, int fhi, float w_out[21], float *phi_out)
{
    JSDR_REQUIRE(h, "jsdr_demod_weights: null handle");
    for (auto &c : h->ch) demod_band_of(c, h->rate, flo, fhi);
    JSDR_HIP_TRY(hipDeviceSynchronize());
    if (h->hist[0].zero() != JSDR_OK || h->hist[1].zero() != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipDeviceSynchronize());
    if (w_out) memcpy(w_out, h->ch[0].w, sizeof(h->ch[0].w));
    if (phi_out) *phi_out = h->ch[0].phi;
    return JSDR_OK;
}

// weights() for one channel.  Of a channel handle: its ring cleared on every input after the handle's pending calls (the next
// call waits for that, nothing else does), the other channels carry on.  Of an ordinary handle: jsdr_demod_weights.
int jsdr_demod_channel_weights(jsdr_demod *h, int channel, int flo, int fhi, float w_out[21], float *phi_out)
{
    DEMOD_CHANNEL_OK("jsdr_demod_channel_weights");
    if (!h->chan) return jsdr_demod_weights(h, flo, fhi, w_out, phi_out);
    DemodCtl c = h->ch[channel];  // (taken over once the clear is queued)
    demod_band_of(c, h->rate, flo, fhi);
    if (h->done_any) JSDR_HIP_TRY(hipStreamWaitEvent(h->copy_stream, h->ev_done, 0));
    JSDR_HIP_TRY(hipMemset2DAsync(h->hist[h->cur].p + (size_t)channel * DHALO, sizeof(float2) * DHALO * (size_t)h->nch, 0,
                                  sizeof(float2) * DHALO, (size_t)h->nin, h->copy_stream));
    JSDR_HIP_TRY(hipEventRecord(h->ev_clear, h->copy_stream));
    h->clear_pending = true;
    h->ch[channel] = c;
    if (w_out) memcpy(w_out, c.w, sizeof(c.w));
    if (phi_out) *phi_out = c.phi;
    return JSDR_OK;
}

int jsdr_demod_state(jsdr_demod *h, float *car_out, float *phi_out)
{
    JSDR_REQUIRE(h, "jsdr_demod_state: null handle");
    if (car_out) *car_out = h->ch[0].car;  // a channel handle: channel 0
    if (phi_out) *phi_out = h->ch[0].phi;
    return JSDR_OK;
}

int jsdr_demod_channel_info(jsdr_demod *h, int *ninputs, int *nchannels)
{
    JSDR_REQUIRE(h && ninputs && nchannels, "jsdr_demod_channel_info: null argument");
    *ninputs = h->nin;
    *nchannels = h->nch;
    return JSDR_OK;
}

int jsdr_demod_get_channel(jsdr_demod *h, int channel, int *mode, int *dofir, int *dodwn, int *doagc, int *flo, int *fhi)
{
    DEMOD_CHANNEL_OK("jsdr_demod_get_channel");
    JSDR_REQUIRE(mode && dofir && dodwn && doagc && flo && fhi, "jsdr_demod_get_channel: null argument");
    const DemodCtl &c = h->ch[channel];
    *mode = c.mode, *dofir = c.dofir, *dodwn = c.dodwn, *doagc = c.doagc, *flo = c.flo, *fhi = c.fhi;
    return JSDR_OK;
}

int jsdr_demod_channel_state(jsdr_demod *h, int channel, float *car_out, float *phi_out)
{
    DEMOD_CHANNEL_OK("jsdr_demod_channel_state");
    JSDR_REQUIRE(car_out && phi_out, "jsdr_demod_channel_state: null argument");
    *car_out = h->ch[channel].car;
    *phi_out = h->ch[channel].phi;
    return JSDR_OK;
}

// the reference's `max` and `avg` fields as the last frame of the last call left them (:465-467)
int jsdr_demod_frame_stats(jsdr_demod *h, int stream, float *max_out, float *avg_out)
{
    JSDR_REQUIRE(h && max_out && avg_out, "jsdr_demod_frame_stats: null argument");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_demod_frame_stats: stream %d outside 0..%d", stream, h->nstreams - 1);
    JSDR_REQUIRE(h->last_nfr > 0, "jsdr_demod_frame_stats: nothing processed yet");
    float v[2];
    JSDR_HIP_TRY(hipDeviceSynchronize());
    JSDR_HIP_TRY(hipMemcpy(v, h->stats.p + 2 * ((size_t)stream * h->last_nfr + (h->last_nfr - 1)), sizeof(v), hipMemcpyDeviceToHost));
    *max_out = v[0];
    *avg_out = v[1];
    return JSDR_OK;
}

}  // extern "C"
