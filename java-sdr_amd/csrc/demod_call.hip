// demod_call.hip -- a call of a demod handle (demod_handle.h): each stage stated once -- the shape check, the carrier
// hand-over, DemodArgs -- then the two runners that launch the call's kernels, and the entry points that get there:
// jsdr_demod_batch_i16 / _f32 and jsdr_demod_receive_f32.  Host code only.
#include "demod_handle.h"
#include <thread>

namespace jsdr {

// Every refusal of a batch call, before any device work.  `rows`: what stride_i16 lies between (streams; the inputs of a
// channel handle), `nrows_in` of them.
static int demod_call_check(const jsdr_demod *h, bool buffers, int64_t stride_i16, int64_t L, int64_t audio_stride_i16,
                            const char *rows, int nrows_in)
{
    JSDR_REQUIRE(h, "demod: null handle");
    JSDR_REQUIRE(buffers, "demod: null buffer");
    JSDR_REQUIRE(L > 0 && L <= h->max_batch && L % h->n == 0,
                 "demod: nsamples=%lld must be a positive multiple of the frame (%d) and at most max_batch_samples=%lld",
                 (long long)L, h->n, h->max_batch);
    JSDR_REQUIRE((stride_i16 & 1) == 0 && (nrows_in == 1 || stride_i16 >= 2 * L) && (audio_stride_i16 & 1) == 0 &&
                     (h->nstreams == 1 || audio_stride_i16 >= 2 * L),
                 "demod: %s stride too small for %lld samples", rows, (long long)L);
    return JSDR_OK;
}

// ---- the carrier hand-over.  `rows` tables of L phases, table r walked from (car[r], phi[r]) at r * nco_pitch of set `set`:
// waits until the call before last has let go of the set, steps the phases on the host (car[r]: left at the phase after the
// call), uploads them and turns them into (cos, sin) pairs on the copy stream; st waits for that.
static int carrier_begin(jsdr_demod *h, int set, float *car, const float *phi, int rows, int64_t L, hipStream_t st)
{
    if (h->used[set]) JSDR_HIP_TRY(hipEventSynchronize(h->ev_used[set]));
    float *tabs = h->car_pinned[set].p;
    auto walk = [&](int r) { car[r] = demod_carrier_walk(tabs + (size_t)r * h->nco_pitch, car[r], phi[r], L); };
    if (rows == 1 || L < 65536) {  // (a thread start costs more than a short table)
        for (int r = 0; r < rows; r++) walk(r);
    } else {  // one host thread per distinct table
        std::vector<std::thread> th;
        for (int r = 0; r < rows; r++) th.emplace_back(walk, r);
        for (auto &t : th) t.join();
    }
    const long long cnt = (long long)(rows - 1) * h->nco_pitch + L;
    JSDR_HIP_TRY(hipMemcpyAsync(h->car_dev[set].p, tabs, sizeof(float) * (size_t)cnt, hipMemcpyHostToDevice, h->copy_stream));
    DEMOD_TIMED(h, DK_NCO, h->copy_stream, launch_demod_nco(h->car_dev[set].p, cnt, h->nco[set].p, h->copy_stream));
    JSDR_HIP_TRY(hipEventRecord(h->ev_table[set], h->copy_stream));
    JSDR_HIP_TRY(hipStreamWaitEvent(st, h->ev_table[set], 0));
    return JSDR_OK;
}

int carrier_end(jsdr_demod *h, int set, hipStream_t st)
{
    JSDR_HIP_TRY(hipEventRecord(h->ev_used[set], st));
    h->used[set] = true;
    return JSDR_OK;
}

DemodArgs demod_args_of(const jsdr_demod *h, int set, const int16_t *raw_dev, const float *rawf_dev, int64_t stride_i16, int64_t L,
                        int ic, int qc)
{
    DemodArgs a;
    a.raw = reinterpret_cast<const int *>(raw_dev);
    a.rawf = reinterpret_cast<const float2 *>(rawf_dev);
    a.stride_pairs = stride_i16 / 2;
    a.L = L;
    a.n = h->n;
    a.nfr = (int)(L / h->n);
    a.ic = ic;
    a.qc = qc;
    a.hist = h->hist[h->cur].p;
    a.lilq = h->lilq[h->cur].p;
    a.nco = h->nco[set].p;
    a.d = h->d.p;
    a.fmax_bits = h->fmax.p;
    demod_const_of(h->ch[0], h->rate, a.c);
    return a;
}

int demod_run(jsdr_demod *h, bool f32in, const int16_t *raw_dev, const float *rawf_dev, int64_t stride_i16, int64_t L, int ic, int qc,
              int16_t *audio_dev, int64_t audio_stride_i16, hipStream_t st)
{
    if (demod_call_check(h, (raw_dev || rawf_dev) && audio_dev, stride_i16, L, audio_stride_i16, "stream", h ? h->nstreams : 0) != JSDR_OK)
        return JSDR_ERR;
    DemodCtl &ctl = h->ch[0];
    const int S = h->nstreams;
    const int set = carrier_set_take(h);
    const DemodArgs a = demod_args_of(h, set, raw_dev, rawf_dev, stride_i16, L, ic, qc);
    if (ctl.dodwn && carrier_begin(h, set, &ctl.car, &ctl.phi, 1, L, st) != JSDR_OK) return JSDR_ERR;
    int *out = reinterpret_cast<int *>(audio_dev);
    const long long osp = (long long)(audio_stride_i16 / 2);
    // every mode but AM, frames of up to 5 tiles (the reference's 9600-sample default included): one kernel from
    // raw samples to int16 audio; JSDR_DEMOD_FUSED=0 keeps the three-kernel path for A/B runs
    static const bool fused_ok = [] {
        const char *e = knob("JSDR_DEMOD_FUSED");
        return !(e && e[0] == '0');
    }();
    const bool fused = fused_ok && ctl.mode != MODE_AM && (h->n + DTILE - 1) / DTILE <= 5;
    if (!fused) JSDR_HIP_TRY(hipMemsetAsync(h->fmax.p, 0, sizeof(unsigned) * (size_t)S * a.nfr, st));
    DEMOD_TIMED(h, DK_FRONT, st, launch_demod_front(a, f32in, fused, S, out, osp, h->stats.p, st));
    DEMOD_TIMED(h, DK_STATE, st, launch_demod_state(a, f32in, h->hist[h->cur ^ 1].p, h->lilq[h->cur ^ 1].p, S, st));
    h->cur ^= 1;
    if (ctl.mode == MODE_AM)
        DEMOD_TIMED(h, DK_MEAN, st, launch_demod_mean(h->d.p, (long long)L, h->n, a.nfr, (long long)S * a.nfr, h->favg.p, st));
    if (!fused) DEMOD_TIMED(h, DK_OUT, st, launch_demod_out(a, S, h->favg.p, out, osp, h->stats.p, st));
    if (ctl.dodwn && carrier_end(h, set, st) != JSDR_OK) return JSDR_ERR;
    h->last_nfr = a.nfr;
    return JSDR_OK;
}

// one call of a channel handle: stride_i16 between INPUTS, audio_stride_i16 between the nin * nch output rows
static int demod_chan_run(jsdr_demod *h, bool f32in, const int16_t *raw_dev, const float *rawf_dev, int64_t stride_i16, int64_t L,
                          int ic, int qc, int16_t *audio_dev, int64_t audio_stride_i16, hipStream_t st)
{
    if (demod_call_check(h, (raw_dev || rawf_dev) && audio_dev, stride_i16, L, audio_stride_i16, "input or output row", h->nin) != JSDR_OK)
        return JSDR_ERR;
    const int K = h->nch;
    const int nfr = (int)(L / h->n);
    const bool fused = (h->n + DTILE - 1) / DTILE <= 5;
    const DemodChanPlan p = demod_chan_plan(h->ch.data(), K, fused);
    const int drows = p.nslots * h->nin;
    if ((size_t)drows * (size_t)L > h->dch.n) {
        JSDR_HIP_TRY(hipDeviceSynchronize());  // earlier calls may still use the smaller buffer
        if (h->dch.alloc((size_t)drows * (size_t)L) != JSDR_OK) return JSDR_ERR;
    }
    const int set = carrier_set_take(h);
    if (p.rows) {
        float car[DCHAN_MAX], phi[DCHAN_MAX];
        for (int r = 0; r < p.rows; r++) car[r] = h->ch[p.row_chan[r]].car, phi[r] = h->ch[p.row_chan[r]].phi;
        const int rc = carrier_begin(h, set, car, phi, p.rows, L, st);
        for (int c = 0; c < K; c++)  // (walked or not, as an ordinary handle's car: carrier_begin steps it in place)
            if (h->ch[c].dodwn) h->ch[c].car = car[p.nco_row[c]];
        if (rc != JSDR_OK) return JSDR_ERR;
    }
    if (h->clear_pending) {  // a channel's ring cleared since the last call
        JSDR_HIP_TRY(hipStreamWaitEvent(st, h->ev_clear, 0));
        h->clear_pending = false;
    }
    DemodChanArgs a = {};
    a.raw = reinterpret_cast<const int *>(raw_dev);
    a.rawf = reinterpret_cast<const float2 *>(rawf_dev);
    a.stride_pairs = stride_i16 / 2;
    a.L = L;
    a.n = h->n;
    a.nfr = nfr;
    a.ic = ic;
    a.qc = qc;
    a.ninputs = h->nin;
    a.K = K;
    a.hist = h->hist[h->cur].p;
    a.lilq = h->lilq[h->cur].p;
    a.nco = h->nco[set].p;
    a.nco_pitch = h->nco_pitch;
    a.d = h->dch.p;
    a.fmax_bits = h->fmax.p;
    a.out = reinterpret_cast<int *>(audio_dev);
    a.out_stride_pairs = audio_stride_i16 / 2;
    a.stats = h->stats.p;
    memcpy(a.slot_chan, p.slot_chan, sizeof(a.slot_chan));
    for (int c = 0; c < K; c++) {
        demod_const_of(h->ch[c], h->rate, a.c[c]);
        a.c[c].nco_row = p.nco_row[c];
        a.c[c].dslot = p.dslot[c];
    }
    if (!fused) JSDR_HIP_TRY(hipMemsetAsync(h->fmax.p, 0, sizeof(unsigned) * (size_t)drows * nfr, st));
    DEMOD_TIMED(h, DK_CHAN, st, launch_demod_chan(a, f32in, fused, st));
    DEMOD_TIMED(h, DK_CHAN, st, launch_demod_chan_state(a, f32in, h->hist[h->cur ^ 1].p, h->lilq[h->cur ^ 1].p, st));
    h->cur ^= 1;
    if (p.nam)  // the AM rows come first
        DEMOD_TIMED(h, DK_MEAN, st, launch_demod_mean(h->dch.p, (long long)L, h->n, nfr, (long long)p.nam * h->nin * nfr, h->favg.p, st));
    if (drows) DEMOD_TIMED(h, DK_CHAN, st, launch_demod_chan_out(a, drows, h->favg.p, st));
    if (p.rows && carrier_end(h, set, st) != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipEventRecord(h->ev_done, st));
    h->done_any = true;
    h->last_nfr = nfr;
    return JSDR_OK;
}

// the runner of the handle's kind
static int demod_call(jsdr_demod *h, bool f32in, const int16_t *raw_dev, const float *rawf_dev, int64_t stride_i16, int64_t L, int ic,
                      int qc, int16_t *audio_dev, int64_t audio_stride_i16, hipStream_t st)
{
    return (h && h->chan ? demod_chan_run : demod_run)(h, f32in, raw_dev, rawf_dev, stride_i16, L, ic, qc, audio_dev, audio_stride_i16, st);
}

}  // namespace jsdr

extern "C" {

int jsdr_demod_batch_i16(jsdr_demod *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc,
                         int16_t *audio_dev, int64_t audio_stride_i16, void *stream)
{
    return demod_call(h, false, raw_dev, nullptr, stream_stride_i16, nsamples, ic, qc, audio_dev, audio_stride_i16, as_stream(stream));
}

int jsdr_demod_batch_f32(jsdr_demod *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples, int16_t *audio_dev,
                         int64_t audio_stride_i16, void *stream)
{
    return demod_call(h, true, nullptr, iq_dev, stream_stride_f32, nsamples, 0, 0, audio_dev, audio_stride_i16, as_stream(stream));
}

// IAudioHandler.receive(float[]): one frame in, the frame's audio bytes out -- of a single-stream handle, or of a 1-input
// channel handle: nch frames of audio, channel c at c * 2n
int jsdr_demod_receive_f32(jsdr_demod *h, const float *buf_host, int16_t *audio_host)
{
    JSDR_REQUIRE(h && buf_host && audio_host, "jsdr_demod_receive_f32: null argument");
    JSDR_REQUIRE(h->nin == 1, h->chan ? "jsdr_demod_receive_f32: the frame-by-frame form needs a 1-input handle"
                                      : "jsdr_demod_receive_f32: the frame-by-frame form needs a 1-stream handle");
    const size_t in_bytes = sizeof(float) * 2 * (size_t)h->n, out_bytes = sizeof(int) * (size_t)h->n * h->nch;
    if (!h->pin_tried) {  // the first receive() of the handle (PinnedStage, common.h)
        h->pin.alloc(in_bytes + out_bytes);
        h->pin_tried = true;
    }
    auto run = [&] {
        return demod_call(h, true, nullptr, h->stage_in.p, 2 * (int64_t)h->n, h->n, 0, 0, reinterpret_cast<int16_t *>(h->stage_out.p),
                          2 * (int64_t)h->n, 0);
    };
    if (h->pin.p) {
        memcpy(h->pin.p, buf_host, in_bytes);
        SyncOnExit guard;  // (an error exit below must not leave the device reading or writing the stage)
        JSDR_HIP_TRY(hipMemcpyAsync(h->stage_in.p, h->pin.p, in_bytes, hipMemcpyHostToDevice, 0));
        if (run() != JSDR_OK) return JSDR_ERR;
        JSDR_HIP_TRY(hipMemcpyAsync(h->pin.p + in_bytes, h->stage_out.p, out_bytes, hipMemcpyDeviceToHost, 0));
        JSDR_HIP_TRY(hipStreamSynchronize(0));
        guard.armed = false;
        memcpy(audio_host, h->pin.p + in_bytes, out_bytes);
        return JSDR_OK;
    }
    JSDR_HIP_TRY(hipMemcpy(h->stage_in.p, buf_host, in_bytes, hipMemcpyHostToDevice));
    if (run() != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipMemcpy(audio_host, h->stage_out.p, out_bytes, hipMemcpyDeviceToHost));
    return JSDR_OK;
}

}  // extern "C"
