// bpsk_results.hip -- what a call left in a jsdr_bpsk handle: the getters, jsdr_bpsk_sync, receive()'s snapshot, profiling, the
// launch reports and the packed result slots.  Host code only (bpsk_handle.h).
#include "bpsk_handle.h"
#include <stddef.h>

// jsdr_bpsk_profile_name: the kernels behind the PK_* scopes, as rocprof shows them
static const char *const kProfNames[PK_COUNT] = {"k_front", "k_hist_in", "k_matched", "k_dm_history", "k_tail", "k_sync",
                                                 "k_sync_fin", "k_fec_bpsk", "k_fm", "k_sync_t", "k_fm_prep",
                                                 "k_acq_fwd", "k_acq_scan", "k_acq_inv", "k_acq_edges", "k_acqc_fwd", "k_tuner_walk"};

static void counters_from(const jsdr_bpsk *h, const TailState &t, const int last[2], int cdec, int centreBin, int32_t *out, int stream = 0)
{
    const bool fft = stream_fft(h, stream);
    out[0] = (int32_t)h->n_in;
    out[1] = (int32_t)h->n_ds;
    out[2] = t.cntBit;
    out[3] = t.cntFEC;
    out[4] = cdec;
    out[5] = last[0];
    out[6] = t.dmCorr;
    out[7] = t.dmMaxCorr;
    out[8] = last[1];
    out[9] = fft ? centreBin : 0;
}

static void state_from(const jsdr_bpsk *h, const TailState &t, double avePeakPower, double aveCentreBin, double *out, int stream = 0)
{
    const bool fft = stream_fft(h, stream);
    out[0] = h->tuPhase;
    out[1] = h->vcoPhase;
    // dmBitPhase (:501,:581-584): k steps of +1/9600 from 0.0 within the current bit, replayed exactly
    double ph = 0.0;
    for (int i = 0; i < (int)(h->n_ds & 7); i++) ph += 1.0 / (double)9600;
    out[2] = ph;
    out[3] = t.dmEnergyOut;
    out[4] = t.energy1;
    out[5] = t.energy2;
    out[6] = fft ? avePeakPower : 0.0;
    out[7] = fft ? aveCentreBin : 0.0;
    for (int i = 0; i < 8; i++) out[8 + i] = t.dmEnergy[i];
    out[16] = t.lastI;
    out[17] = t.lastQ;
}

int jsdr::publish_snapshot(jsdr_bpsk *h)
{
    // pack on the stream the call's last kernels ran on, fetch once
    hipStream_t ts = (h->overlap && h->tail_stream) ? h->tail_stream : h->last_stream;
    if (!h->snap_fused) {
        if (launch_snapshot_pack(h->snap_dev.p, h->tail.p, h->fec_last.p, h->cnt_dec.p, h->nbits.p,
                                 stream_fft(h, 0) ? h->fft_state.p : (const FftFrontState *)nullptr, h->decoded.p,
                                 h->bitlog[h->bitlog_cur].p + HIST_BITS, ts) != JSDR_OK)
            return JSDR_ERR;
    }
    SnapPack pk_stack;
    // (the arena's last slot: reserved at create, never handed out by h2d_call)
    SnapPack *pkp = h->pin.p ? reinterpret_cast<SnapPack *>(h->pin.p + h->pin_bytes) : &pk_stack;
    JSDR_HIP_TRY(hipMemcpyAsync(pkp, h->snap_dev.p, sizeof(SnapPack), hipMemcpyDeviceToHost, ts));
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipStreamSynchronize(ts));
    if (h->snap_fused) {  // what k_snapshot_pack does on the device: no FFT state in tune mode, no bytes beyond the call's bits
        if (!stream_fft(h, 0)) {
            pkp->centreBin = 0;
            pkp->avePeakPower = 0.0;
            pkp->aveCentreBin = 0.0;
        }
        for (int k = pkp->nbits < 0 ? 0 : pkp->nbits; k < 512; k++) pkp->bits[k] = 0;
    }
    const SnapPack &pk = *pkp;
    // what the getters refuse, the snapshot refuses (check_overflow)
    JSDR_REQUIRE(!pk.t.overflow, "receive: stream 0 exceeded its per-call capacity (%d bits / %d FEC calls per call of at most %lld samples)",
                 h->max_bits, h->trig_cap, h->max_batch);
    JSDR_REQUIRE(h->variant == 0 || !pk.t.uncertified, "receive: stream 0: the fast variant could not certify a slicer decision (inside "
                 "its error margin and not recomputable in exact order); run this stream with JSDR_VARIANT_EXACT");
    const int cur = h->snap_cur.load(std::memory_order_relaxed);
    const int w = cur == 0 ? 1 : 0;  // the copy no reader is directed to
    h->snap_seq[w].fetch_add(1, std::memory_order_acq_rel);  // odd: writing
    jsdr_bpsk_snapshot &sn = h->snap[w];
    counters_from(h, pk.t, pk.last, pk.cdec, pk.centreBin, sn.counters);
    state_from(h, pk.t, pk.avePeakPower, pk.aveCentreBin, sn.state);
    if (h->nch > 0) sn.state[0] = h->chan[0].tuPhase;
    memcpy(sn.decoded, pk.decoded, 256);
    static_assert(sizeof(sn.bits) == sizeof(pk.bits), "snapshot bit capacity");
    memcpy(sn.bits, pk.bits, sizeof(sn.bits));
    sn.nbits = pk.nbits;
    sn.frames = ++h->snap_count;
    h->snap_seq[w].fetch_add(1, std::memory_order_release);  // even: complete
    h->snap_cur.store(w, std::memory_order_release);
    return JSDR_OK;
}

int jsdr::sync_last(jsdr_bpsk *h)
{
    JSDR_HIP_TRY(hipStreamSynchronize(h->last_stream));
    if (h->tail_stream) JSDR_HIP_TRY(hipStreamSynchronize(h->tail_stream));
    if (h->shadow) return sync_last(h->shadow.get());
    return JSDR_OK;
}

// a stream jsdr_bpsk_recover_uncertified() has replayed is served by the exact shadow handle
#define JSDR_SHADOWED(h, stream) ((h)->shadow && (stream) >= 0 && (stream) < (h)->nstreams && (h)->shadow_map[(size_t)(stream)] >= 0)

// a stream that overflowed its per-call capacity has an incomplete result log: every getter says so
static int check_overflow(jsdr_bpsk *h, int stream, const char *who)
{
    int ov = 0;
    JSDR_HIP_TRY(hipMemcpy(&ov, reinterpret_cast<const char *>(h->tail.p + stream) + offsetof(TailState, overflow), sizeof(int),
                           hipMemcpyDeviceToHost));
    JSDR_REQUIRE(!ov, "%s: stream %d exceeded its per-call capacity (%d bits / %d FEC calls per call of at most %lld samples)", who,
                 stream, h->max_bits, h->trig_cap, h->max_batch);
    if (h->variant != 0) {
        int un = 0;
        JSDR_HIP_TRY(hipMemcpy(&un, reinterpret_cast<const char *>(h->tail.p + stream) + offsetof(TailState, uncertified), sizeof(int),
                               hipMemcpyDeviceToHost));
        JSDR_REQUIRE(!un, "%s: stream %d: the fast variant could not certify a slicer decision (inside its error margin and not "
                     "recomputable in exact order); run this stream with JSDR_VARIANT_EXACT", who, stream);
    }
    return JSDR_OK;
}

int jsdr_bpsk_get_counters(jsdr_bpsk *h, int stream, int32_t out[JSDR_BPSK_NCOUNTERS])
{
    JSDR_REQUIRE(h && out, "jsdr_bpsk_get_counters: null argument");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_bpsk_get_counters: stream %d out of range", stream);
    if (JSDR_SHADOWED(h, stream)) return jsdr_bpsk_get_counters(h->shadow.get(), h->shadow_map[(size_t)stream], out);
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    TailState t;
    int last[2], cdec;
    JSDR_HIP_TRY(hipMemcpy(&t, h->tail.p + stream, sizeof(t), hipMemcpyDeviceToHost));
    JSDR_HIP_TRY(hipMemcpy(last, h->fec_last.p + 2 * stream, sizeof(last), hipMemcpyDeviceToHost));
    JSDR_HIP_TRY(hipMemcpy(&cdec, h->cnt_dec.p + stream, sizeof(int), hipMemcpyDeviceToHost));
    if (check_overflow(h, stream, "jsdr_bpsk_get_counters") != JSDR_OK) return JSDR_ERR;
    int centreBin = 0;
    if (stream_fft(h, stream)) {
        FftFrontState fs;
        JSDR_HIP_TRY(hipMemcpy(&fs, h->fft_state.p + fft_state_at(h, stream), sizeof(fs), hipMemcpyDeviceToHost));
        centreBin = fs.centreBin;
    }
    counters_from(h, t, last, cdec, centreBin, out, stream);
    return JSDR_OK;
}

int jsdr_bpsk_get_bits(jsdr_bpsk *h, int stream, int8_t *bits_host, int cap, int *nbits)
{
    JSDR_REQUIRE(h && nbits, "jsdr_bpsk_get_bits: null argument");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_bpsk_get_bits: stream %d out of range", stream);
    if (JSDR_SHADOWED(h, stream)) return jsdr_bpsk_get_bits(h->shadow.get(), h->shadow_map[(size_t)stream], bits_host, cap, nbits);
    if (sync_last(h) != JSDR_OK || check_overflow(h, stream, "jsdr_bpsk_get_bits") != JSDR_OK) return JSDR_ERR;
    int nb = 0;
    JSDR_HIP_TRY(hipMemcpy(&nb, h->nbits.p + stream, sizeof(int), hipMemcpyDeviceToHost));
    *nbits = nb;
    int n = nb < cap ? nb : cap;
    if (n > 0 && bits_host)
        JSDR_HIP_TRY(hipMemcpy(bits_host, h->bitlog[h->bitlog_cur].p + (size_t)stream * h->bitlog_stride + HIST_BITS,
                               (size_t)n, hipMemcpyDeviceToHost));
    return JSDR_OK;
}

int jsdr_bpsk_get_fec_count(jsdr_bpsk *h, int stream, int *count)
{
    JSDR_REQUIRE(h && count, "jsdr_bpsk_get_fec_count: null argument");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_bpsk_get_fec_count: stream %d out of range", stream);
    if (JSDR_SHADOWED(h, stream)) return jsdr_bpsk_get_fec_count(h->shadow.get(), h->shadow_map[(size_t)stream], count);
    if (sync_last(h) != JSDR_OK || check_overflow(h, stream, "jsdr_bpsk_get_fec_count") != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipMemcpy(count, h->trig_count.p + stream, sizeof(int), hipMemcpyDeviceToHost));
    return JSDR_OK;
}

int jsdr_bpsk_get_fec(jsdr_bpsk *h, int stream, int idx, int32_t *rc, int32_t *bit_index, uint8_t out_host[256])
{
    JSDR_REQUIRE(h && rc && bit_index && out_host, "jsdr_bpsk_get_fec: null argument");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_bpsk_get_fec: stream %d out of range", stream);
    if (JSDR_SHADOWED(h, stream)) return jsdr_bpsk_get_fec(h->shadow.get(), h->shadow_map[(size_t)stream], idx, rc, bit_index, out_host);
    int cnt = 0;
    if (jsdr_bpsk_get_fec_count(h, stream, &cnt) != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(idx >= 0 && idx < cnt, "jsdr_bpsk_get_fec: index %d outside the %d calls of the last batch", idx, cnt);
    int b = 0;
    JSDR_HIP_TRY(hipMemcpy(rc, h->fec_rc.p + stream * h->trig_cap + idx, sizeof(int), hipMemcpyDeviceToHost));
    JSDR_HIP_TRY(hipMemcpy(&b, h->trig_bits.p + stream * h->trig_cap + idx, sizeof(int), hipMemcpyDeviceToHost));
    *bit_index = b + 1;
    JSDR_HIP_TRY(hipMemcpy(out_host, h->fec_data.p + ((size_t)stream * h->trig_cap + idx) * 256, 256, hipMemcpyDeviceToHost));
    return JSDR_OK;
}

int jsdr_bpsk_get_decoded(jsdr_bpsk *h, int stream, uint8_t out_host[256])
{
    JSDR_REQUIRE(h && out_host, "jsdr_bpsk_get_decoded: null argument");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_bpsk_get_decoded: stream %d out of range", stream);
    if (JSDR_SHADOWED(h, stream)) return jsdr_bpsk_get_decoded(h->shadow.get(), h->shadow_map[(size_t)stream], out_host);
    if (sync_last(h) != JSDR_OK || check_overflow(h, stream, "jsdr_bpsk_get_decoded") != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipMemcpy(out_host, h->decoded.p + (size_t)stream * 256, 256, hipMemcpyDeviceToHost));
    return JSDR_OK;
}

int jsdr_bpsk_get_trace(jsdr_bpsk *h, int stream, double *out_host, int64_t cap_pairs, int64_t *npairs)
{
    JSDR_REQUIRE(h && npairs, "jsdr_bpsk_get_trace: null argument");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_bpsk_get_trace: stream %d out of range", stream);
    if (JSDR_SHADOWED(h, stream)) return jsdr_bpsk_get_trace(h->shadow.get(), h->shadow_map[(size_t)stream], out_host, cap_pairs, npairs);
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    const long long have = (!h->trace_void.empty() && h->trace_void[(size_t)stream]) ? 0 : h->last_nds;  // (restored since: an empty call)
    *npairs = have;
    long long n = have < cap_pairs ? have : cap_pairs;
    if (n > 0 && out_host)
        JSDR_HIP_TRY(hipMemcpy(out_host, h->y[h->last_y].p + Y_PAD + (size_t)stream * h->y_stride, sizeof(double2) * (size_t)n,
                               hipMemcpyDeviceToHost));
    return JSDR_OK;
}

int jsdr_bpsk_get_state(jsdr_bpsk *h, int stream, double out[18])
{
    JSDR_REQUIRE(h && out, "jsdr_bpsk_get_state: null argument");
    JSDR_REQUIRE(stream >= 0 && stream < h->nstreams, "jsdr_bpsk_get_state: stream %d out of range", stream);
    if (JSDR_SHADOWED(h, stream)) return jsdr_bpsk_get_state(h->shadow.get(), h->shadow_map[(size_t)stream], out);
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    TailState t;
    JSDR_HIP_TRY(hipMemcpy(&t, h->tail.p + stream, sizeof(t), hipMemcpyDeviceToHost));
    double app = 0.0, acb = 0.0;
    if (stream_fft(h, stream)) {
        FftFrontState fs;
        JSDR_HIP_TRY(hipMemcpy(&fs, h->fft_state.p + fft_state_at(h, stream), sizeof(fs), hipMemcpyDeviceToHost));
        app = fs.avePeakPower;
        acb = fs.aveCentreBin;
    }
    state_from(h, t, app, acb, out, stream);
    if (h->nch > 0) out[0] = h->chan[stream % h->nch].tuPhase;
    if (h->pst) JSDR_HIP_TRY(hipMemcpy(&out[0], h->pst_tu.p + stream, sizeof(double), hipMemcpyDeviceToHost));
    return JSDR_OK;
}

int jsdr_bpsk_sync(jsdr_bpsk *h)
{
    JSDR_REQUIRE(h, "jsdr_bpsk_sync: null handle");
    return sync_last(h);
}

// any thread, no HIP call, no lock: the results of the last completed receive_*() of a 1-stream handle
int jsdr_bpsk_snapshot_read(jsdr_bpsk *h, jsdr_bpsk_snapshot *out)
{
    JSDR_REQUIRE(h && out, "jsdr_bpsk_snapshot_read: null argument");
    JSDR_REQUIRE(h->nch <= 1, "jsdr_bpsk_snapshot_read: a channel handle of %d channels has no snapshot (read the getters per stream)", h->nch);
    for (int attempt = 0; attempt < 1000; attempt++) {
        const int cur = h->snap_cur.load(std::memory_order_acquire);
        JSDR_REQUIRE(cur >= 0, "jsdr_bpsk_snapshot_read: nothing received yet");
        const unsigned s0 = h->snap_seq[cur].load(std::memory_order_acquire);
        if (s0 & 1u) continue;  // being rewritten: the writer has lapped us, take the newer copy
        memcpy(out, &h->snap[cur], sizeof(*out));
        std::atomic_thread_fence(std::memory_order_acquire);
        if (h->snap_seq[cur].load(std::memory_order_relaxed) == s0) return JSDR_OK;
    }
    set_error("jsdr_bpsk_snapshot_read: could not get a stable copy");
    return JSDR_ERR;
}

int jsdr_bpsk_profile_enable(jsdr_bpsk *h, int on)
{
    JSDR_REQUIRE(h, "jsdr_bpsk_profile_enable: null handle");
    h->prof_on = on != 0;
    return JSDR_OK;
}

int jsdr_bpsk_profile_count(void) { return PK_COUNT; }

const char *jsdr_bpsk_front_kernel(jsdr_bpsk *h) { return h ? h->front_name : ""; }

const char *jsdr_bpsk_tail_kernel(jsdr_bpsk *h) { return h ? h->tail_name : ""; }
const char *jsdr_bpsk_fec_kernel(jsdr_bpsk *h) { return h ? h->fec_name : ""; }

int jsdr_bpsk_side_stream(jsdr_bpsk *h, int *on)
{
    JSDR_REQUIRE(h && on, "jsdr_bpsk_side_stream: null argument");
    *on = h->overlap ? 1 : 0;
    return JSDR_OK;
}

// fast variant: decisions redone in exact order (all streams, since creation), streams that ended up uncertified, the
// error bound of (fi,fq) the margins are built on
int jsdr_bpsk_cert_stats(jsdr_bpsk *h, int64_t *redone, int64_t *uncertified_streams, double *ey)
{
    JSDR_REQUIRE(h, "jsdr_bpsk_cert_stats: null handle");
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    std::vector<TailState> ts((size_t)h->nstreams);
    JSDR_HIP_TRY(hipMemcpy(ts.data(), h->tail.p, sizeof(TailState) * ts.size(), hipMemcpyDeviceToHost));
    long long r = 0, u = 0;
    for (size_t s = 0; s < ts.size(); s++) {
        r += ts[s].redone;
        u += (ts[s].uncertified && !JSDR_SHADOWED(h, (int)s)) ? 1 : 0;  // (a recovered stream is served in exact order: not counted)
    }
    if (redone) *redone = r;
    if (uncertified_streams) *uncertified_streams = u;
    if (ey) *ey = h->fast_ey * h->margin_scale;
    return JSDR_OK;
}

// fast variant: WHICH streams are uncertified (ascending ids, at most cap of them; *count = how many there are in all).
// The flag is set by the call in which the uncertifiable decision fell and stays set: the results of that call and of
// every later one are withheld for that stream (its getters fail).  What a caller does with the list: run those streams
// -- from the first sample of the flagged call on an exact handle that has seen the same earlier input, or from the start
// of the stream -- with JSDR_VARIANT_EXACT, which decides the same near-tie by the reference's own arithmetic.
int jsdr_bpsk_uncertified_streams(jsdr_bpsk *h, int32_t *ids, int cap, int *count)
{
    JSDR_REQUIRE(h && count, "jsdr_bpsk_uncertified_streams: null argument");
    JSDR_REQUIRE(cap == 0 || ids, "jsdr_bpsk_uncertified_streams: null id buffer");
    *count = 0;
    if (h->variant == 0) return JSDR_OK;  // the exact variant certifies nothing and withholds nothing
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    std::vector<TailState> ts((size_t)h->nstreams);
    JSDR_HIP_TRY(hipMemcpy(ts.data(), h->tail.p, sizeof(TailState) * ts.size(), hipMemcpyDeviceToHost));
    int n = 0;
    for (int s = 0; s < h->nstreams; s++)
        if (ts[(size_t)s].uncertified && !JSDR_SHADOWED(h, s)) {
            if (n < cap) ids[n] = s;
            n++;
        }
    *count = n;
    return JSDR_OK;
}

int jsdr_bpsk_stream_recovered(jsdr_bpsk *h, int stream, int *recovered)
{
    JSDR_REQUIRE(h && recovered && stream >= 0 && stream < h->nstreams, "jsdr_bpsk_stream_recovered: bad argument");
    *recovered = JSDR_SHADOWED(h, stream) ? 1 : 0;
    return JSDR_OK;
}

int jsdr_bpsk_schedule_stats(jsdr_bpsk *h, int64_t *computed_inline, int64_t *prefetched)
{
    JSDR_REQUIRE(h, "jsdr_bpsk_schedule_stats: null handle");
    if (computed_inline) *computed_inline = h->sched_sync;
    if (prefetched) *prefetched = h->sched_prefetched;
    return JSDR_OK;
}

int jsdr_bpsk_last_launch(jsdr_bpsk *h, int64_t *work_items, int64_t *workgroups)
{
    JSDR_REQUIRE(h && work_items && workgroups, "jsdr_bpsk_last_launch: null argument");
    *work_items = h->last_fm_items;
    *workgroups = h->last_fm_grid;
    return JSDR_OK;
}

int jsdr_bpsk_fm_form(jsdr_bpsk *h, int *specialised, int *phase)
{
    JSDR_REQUIRE(h && specialised && phase, "jsdr_bpsk_fm_form: null argument");
    *specialised = h->last_fm_phase >= 0;
    *phase = h->last_fm_phase;
    return JSDR_OK;
}

int jsdr_bpsk_acq_last_launch(jsdr_bpsk *h, int64_t *fwd_frames, int64_t *inv_frames)
{
    JSDR_REQUIRE(h && fwd_frames && inv_frames, "jsdr_bpsk_acq_last_launch: null argument");
    *fwd_frames = h->acq_fwd_frames;
    *inv_frames = h->acq_inv_frames;
    return JSDR_OK;
}

const char *jsdr_bpsk_profile_name(int k) { return (k >= 0 && k < PK_COUNT) ? kProfNames[k] : ""; }

int jsdr_bpsk_profile_read(jsdr_bpsk *h, double *ms_total, int *launches)
{
    JSDR_REQUIRE(h && ms_total && launches, "jsdr_bpsk_profile_read: null argument");
    for (int k = 0; k < PK_COUNT; k++) {
        ms_total[k] = 0.0;
        launches[k] = 0;
    }
    for (auto &r : h->prof_recs) {
        float ms = 0.f;
        JSDR_HIP_TRY(hipEventSynchronize(r.b));
        JSDR_HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        ms_total[r.kernel] += (double)ms;
        launches[r.kernel] += 1;
        h->prof_pool.push_back(std::move(r.a));
        h->prof_pool.push_back(std::move(r.b));
    }
    h->prof_recs.clear();
    return JSDR_OK;
}

int jsdr_bpsk_slot_info(jsdr_bpsk *h, int64_t *slot_bytes, int64_t *bits_offset, int64_t *fec_offset, int *slot_bits,
                        int *nfec_max)
{
    JSDR_REQUIRE(h, "jsdr_bpsk_slot_info: null handle");
    int64_t bits = (h->max_bits + 15) & ~15;
    if (bits_offset) *bits_offset = 64;
    if (fec_offset) *fec_offset = 64 + bits;
    if (slot_bits) *slot_bits = (int)bits;
    if (nfec_max) *nfec_max = h->trig_cap;
    if (slot_bytes) *slot_bytes = 64 + bits + (int64_t)h->trig_cap * 264;
    return JSDR_OK;
}

int jsdr_bpsk_pack_slots(jsdr_bpsk *h, uint8_t *slots_dev, void *stream)
{
    JSDR_REQUIRE(h && slots_dev, "jsdr_bpsk_pack_slots: null argument");
    int64_t slot_bytes = 0;
    int slot_bits = 0;
    jsdr_bpsk_slot_info(h, &slot_bytes, nullptr, nullptr, &slot_bits, nullptr);
    if (h->overlap && h->tail_pending[h->last_y]) {  // results of the last call come from the side stream
        JSDR_HIP_TRY(hipStreamWaitEvent(as_stream(stream), h->ev_tail_done[h->last_y], 0));
    } else if (!h->overlap && as_stream(stream) != h->last_stream && h->ev_matched) {
        // no side stream (1-stream handles, JSDR_NO_OVERLAP): the results come from the stream of the last call; a pack on
        // ANOTHER stream waits for that one (the event is free in this mode)
        JSDR_HIP_TRY(hipEventRecord(h->ev_matched, h->last_stream));
        JSDR_HIP_TRY(hipStreamWaitEvent(as_stream(stream), h->ev_matched, 0));
    }
    if (launch_pack_slots(slots_dev, (long long)slot_bytes, slot_bits, h->trig_cap, h->tail.p, h->nbits.p, h->bitlog[h->bitlog_cur].p,
                          h->bitlog_stride, h->trig_count.p, h->trig_bits.p, h->fec_rc.p, h->fec_data.p, h->fec_last.p, h->cnt_dec.p,
                          (int)h->n_in, (int)h->n_ds, h->nstreams, as_stream(stream)) != JSDR_OK)
        return JSDR_ERR;
    // the per-call result arrays are single-buffered: the next call's tail / sync / FEC (side stream) must not
    // overwrite them while this kernel is still reading
    JSDR_HIP_TRY(hipEventRecord(h->ev_pack_done, as_stream(stream)));
    h->pack_pending = true;
    if (h->shadow) {
        // the recovered streams' slots are the exact shadow's (same slot layout: same max_batch), laid over the fast handle's
        if (jsdr_bpsk_pack_slots(h->shadow.get(), h->shadow_slots.p, stream) != JSDR_OK) return JSDR_ERR;
        for (size_t i = 0; i < h->shadow_ids.size(); i++)
            JSDR_HIP_TRY(hipMemcpyAsync(slots_dev + (size_t)h->shadow_ids[i] * (size_t)slot_bytes, h->shadow_slots.p + i * (size_t)slot_bytes,
                                        (size_t)slot_bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    }
    return JSDR_OK;
}
