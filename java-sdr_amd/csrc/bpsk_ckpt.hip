// bpsk_ckpt.hip -- checkpoints of a jsdr_bpsk handle: jsdr_bpsk_save / jsdr_bpsk_restore.  Host code only (bpsk_handle.h).
#include "bpsk_handle.h"
#include "bpsk_blob.h"
#include "bpsk_state.h"

// ------------------------------------------------------------------------------------------- checkpoints
// jsdr_bpsk_save / jsdr_bpsk_restore: the state of a range of streams out of a handle and into one, as a blob (bpsk_blob.h: the
// shared block and one canonical record per stream).  The handle's part is to say where each piece of a stream's state lives
// right now -- the current bit log, dm or dmh, the current input history and tuner-index buffer -- and to keep the host
// scheduler coherent; the records are gathered and scattered on the device (bpsk_state.hip), one copy each way.
// Every check comes before the first write: a REFUSED call leaves the handle exactly as it was.  A call that fails later, in a
// device allocation, copy or launch, may leave buffers behind it that it allocated (the staging image, the FFT-acquire buffers);
// they are harmless and reused.

// the handles a checkpoint covers
static int ckpt_check(jsdr_bpsk *h, const char *who)
{
    JSDR_REQUIRE(h, "%s: null handle", who);
    JSDR_REQUIRE(h->nch == 0, "%s: a channel handle (jsdr_bpsk_create_channels / _create_mode_channels / _create_live_channels) keeps "
                 "per-channel tuners and seams on the host, which the record does not carry; the handle is unchanged", who);
    JSDR_REQUIRE(h->pst_nch == 0, "%s: a tuned channel handle (jsdr_bpsk_create_tuned_channels) keeps one input history per input, and a "
                 "record carries a stream's own; the handle is unchanged", who);
    JSDR_REQUIRE(h->variant == JSDR_VARIANT_EXACT, "%s: a JSDR_VARIANT_FAST handle has no exact state to carry (its certification "
                 "bounds and its shadow are not part of the record); the handle is unchanged", who);
    return JSDR_OK;
}

static void ckpt_shared(const jsdr_bpsk *h, BlobShared &sh)
{
    sh.kind = h->pst ? BLOB_KIND_TUNED : BLOB_KIND_ORDINARY;
    sh.rate = (uint32_t)h->rate;
    sh.nsf = (uint32_t)h->nsf;
    sh.do_fft = h->do_fft ? 1u : 0u;
    sh.do_up = h->do_up ? 1u : 0u;
    sh.seam = (uint32_t)h->seam;
    sh.hist_float = h->hist_is_float ? 1u : 0u;
    sh.fft_state = h->fft_ready ? 1u : 0u;
    sh.ds_cnt = h->dsCnt;
    sh.n_in = h->n_in;
    sh.n_ds = h->n_ds;
    sh.tuning = h->tuning;
    sh.tu_phase = h->tuPhase;
    sh.tu_inc = h->tuPhaseInc;
    sh.vco_phase = h->vcoPhase;
    memcpy(sh.khist, h->h_khist, BLOB_HIST);
    memcpy(sh.mhist, h->h_mhist, BLOB_HIST);
}

// where the streams' state lives now
static StateArgs ckpt_args(jsdr_bpsk *h, int first, int count)
{
    StateArgs a;
    memset(&a, 0, sizeof(a));
    a.img = h->state_img.p;
    a.first = first;
    a.count = count;
    a.tail = h->tail.p;
    a.bitlog = h->bitlog[h->bitlog_cur].p;
    a.bitlog_stride = h->bitlog_stride;
    a.nbits = h->nbits.p;
    a.trig_count = h->trig_count.p;
    a.fec_last = h->fec_last.p;
    a.cnt_dec = h->cnt_dec.p;
    a.decoded = h->decoded.p;
    a.hist = h->hist_in[h->hist_cur].p;
    a.halo = h->halo_in_dmh ? h->dmh[h->dmh_cur].p : h->dm.p;
    a.halo_stride = h->halo_in_dmh ? 64 : h->dm_stride;
    a.fft = h->fft_ready ? h->fft_state.p : nullptr;
    if (h->pst) {
        a.pst_tu = h->pst_tu.p;
        a.pst_inc = h->pst_inc.p;
        a.pst_kh = h->pst_kh[h->pst_kh_cur].p;
    }
    return a;
}

static int ckpt_stage(jsdr_bpsk *h, int count)
{
    const size_t need = (size_t)count * BLOB_RECORD_BYTES;
    if (h->state_img.n >= need) return JSDR_OK;
    DevBuf<unsigned char> img;
    if (img.alloc(need) != JSDR_OK) return JSDR_ERR;
    h->state_img = std::move(img);  // (the smaller image goes)
    return JSDR_OK;
}

// the pair of events the pack / unpack launch is timed with (a diagnostic: a handle without them saves and restores all the same)
static bool ckpt_events(jsdr_bpsk *h)
{
    for (int i = 0; i < 2; i++)
        if (!h->ev_state[i] && h->ev_state[i].create() != JSDR_OK) {
            (void)hipGetLastError();
            return false;
        }
    return true;
}
static float ckpt_elapsed(jsdr_bpsk *h, bool timed)
{
    float ms = -1.f;
    if (timed && (hipEventSynchronize(h->ev_state[1]) != hipSuccess || hipEventElapsedTime(&ms, h->ev_state[0], h->ev_state[1]) != hipSuccess)) {
        (void)hipGetLastError();
        ms = -1.f;
    }
    return ms;
}

int jsdr_bpsk_state_kernel_ms(jsdr_bpsk *h, double *pack_ms, double *unpack_ms)
{
    JSDR_REQUIRE(h && pack_ms && unpack_ms, "jsdr_bpsk_state_kernel_ms: null argument");
    *pack_ms = (double)h->state_pack_ms;
    *unpack_ms = (double)h->state_unpack_ms;
    return JSDR_OK;
}

int jsdr_bpsk_state_bytes(jsdr_bpsk *h, int count, size_t *bytes)
{
    if (ckpt_check(h, "jsdr_bpsk_state_bytes") != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(bytes, "jsdr_bpsk_state_bytes: null size pointer");
    JSDR_REQUIRE(count >= 1 && count <= h->nstreams, "jsdr_bpsk_state_bytes: %d streams outside 1 .. %d", count, h->nstreams);
    *bytes = blob_bytes((uint32_t)count);
    return JSDR_OK;
}

int jsdr_bpsk_save(jsdr_bpsk *h, int first, int count, void *blob_host, size_t cap, size_t *bytes)
{
    if (ckpt_check(h, "jsdr_bpsk_save") != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(blob_host && bytes, "jsdr_bpsk_save: null pointer");
    JSDR_REQUIRE(first >= 0 && count >= 1 && first < h->nstreams && count <= h->nstreams - first, "jsdr_bpsk_save: streams %d .. %lld out of "
                 "range (the handle has %d)", first, (long long)first + count - 1, h->nstreams);
    const size_t need = blob_bytes((uint32_t)count);
    JSDR_REQUIRE(cap >= need, "jsdr_bpsk_save: the buffer holds %zu bytes, a blob of %d streams takes %zu", cap, count, need);
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    if (ckpt_stage(h, count) != JSDR_OK) return JSDR_ERR;
    const bool timed = ckpt_events(h);
    if (timed) (void)hipEventRecord(h->ev_state[0], 0);
    if (launch_state_pack(ckpt_args(h, first, count), 0) != JSDR_OK) return JSDR_ERR;
    if (timed) (void)hipEventRecord(h->ev_state[1], 0);
    BlobShared sh;
    ckpt_shared(h, sh);
    JSDR_REQUIRE(blob_begin(blob_host, cap, sh, (uint32_t)count), "jsdr_bpsk_save: internal: the blob's header could not be laid out");
    JSDR_HIP_TRY(hipMemcpy(blob_record(blob_host, 0), h->state_img.p, (size_t)count * BLOB_RECORD_BYTES, hipMemcpyDeviceToHost));
    if (h->pst)  // (a stream's tuning is a host value; its tuPhase and tuPhaseInc came from the device)
        for (int i = 0; i < count; i++) blob_put_f64(blob_record(blob_host, (uint32_t)i) + REC_PST_F64, h->pst_tuning[(size_t)(first + i)]);
    blob_seal(blob_host, need);
    h->state_pack_ms = ckpt_elapsed(h, timed);
    *bytes = need;
    return JSDR_OK;
}

int jsdr_bpsk_restore(jsdr_bpsk *h, int dst_first, const void *blob_host, size_t bytes)
{
    if (ckpt_check(h, "jsdr_bpsk_restore") != JSDR_OK) return JSDR_ERR;
    JSDR_REQUIRE(blob_host, "jsdr_bpsk_restore: null blob");
    BlobShared sh;
    uint32_t n = 0;
    char why[192];
    JSDR_REQUIRE(blob_parse(blob_host, bytes, &sh, &n, why, sizeof(why)), "jsdr_bpsk_restore: %s; the handle is unchanged", why);
    const int count = (int)n;
    JSDR_REQUIRE(sh.kind == (h->pst ? (uint32_t)BLOB_KIND_TUNED : (uint32_t)BLOB_KIND_ORDINARY), "jsdr_bpsk_restore: the blob is of %s handle, "
                 "this is %s; the handle is unchanged", sh.kind == BLOB_KIND_TUNED ? "a tuned" : "an ordinary", h->pst ? "a tuned one" : "an ordinary one");
    JSDR_REQUIRE(sh.rate == (uint32_t)h->rate && sh.nsf == (uint32_t)h->nsf, "jsdr_bpsk_restore: the blob is of rate %u Hz and frames of %u "
                 "samples, the handle of %d Hz and %d; the handle is unchanged", sh.rate, sh.nsf, h->rate, h->nsf);
    JSDR_REQUIRE(dst_first >= 0 && dst_first < h->nstreams && count <= h->nstreams - dst_first, "jsdr_bpsk_restore: streams %d .. %lld out of "
                 "range (the blob has %d, the handle %d); the handle is unchanged", dst_first, (long long)dst_first + count - 1, count, h->nstreams);
    // A checksum is easy to forge: what the host scheduler or a kernel would use as an index is range-checked too (blob_parse has
    // checked the shared block's flags, counters and phases), and tuPhaseInc must be the one its tuning gives (:189)
    {
        const double inc = tuner_inc(sh.tuning, h->rate);
        JSDR_REQUIRE(memcmp(&inc, &sh.tu_inc, sizeof(double)) == 0, "jsdr_bpsk_restore: the blob's tuPhaseInc (%.17g) is not the one its tuning "
                     "(%.17g Hz) gives; the handle is unchanged", sh.tu_inc, sh.tuning);
    }
    for (int i = 0; i < count; i++) {
        const unsigned char *rec = blob_record(blob_host, (uint32_t)i);
        JSDR_REQUIRE(blob_record_check(rec, sh, why, sizeof(why)), "jsdr_bpsk_restore: record %d: %s; the handle is unchanged", i, why);
        if (h->pst) {
            const double inc = tuner_inc(blob_get_f64(rec + REC_PST_F64), h->rate), got = blob_get_f64(rec + REC_PST_F64 + 16);
            JSDR_REQUIRE(memcmp(&inc, &got, sizeof(double)) == 0, "jsdr_bpsk_restore: record %d: tuPhaseInc (%.17g) is not the one the stream's "
                         "tuning gives; the handle is unchanged", i, got);
        }
    }
    const bool fresh = h->n_in == 0 && !h->restored;  // free to adopt the blob's shared block
    if (!fresh) {
        BlobShared mine;
        ckpt_shared(h, mine);
        JSDR_REQUIRE(blob_shared_equal(mine, sh), "jsdr_bpsk_restore: the blob's shared block (tuning, mode, phases, sample counts, input "
                     "history form, pending seam) is not this handle's (blob: %lld samples in, tuning %g, do_fft %u; handle: %lld, %g, %d), and "
                     "only a handle that has taken no sample and no blob adopts one; the handle is unchanged",
                     (long long)sh.n_in, sh.tuning, sh.do_fft, (long long)h->n_in, h->tuning, h->do_fft);
    }
    FftFront kind = FRONT_NONE;
    if (sh.fft_state) {
        kind = fft_front_kind(h->nsf, h->decim, false);
        JSDR_REQUIRE(kind != FRONT_NONE, "jsdr_bpsk_restore: the blob holds FFT-acquire state of a frame size (%d) FFT-acquire cannot take; the "
                     "handle is unchanged", h->nsf);
    }
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    if (h->worker.joinable()) h->worker.join();
    // what can fail for want of memory comes before anything of the handle moves: the staging image, and the FFT-acquire
    // buffers with the seam's scratch, as jsdr_bpsk_set_mode allocates them (zeroed: every other stream's state as at creation)
    if (ckpt_stage(h, count) != JSDR_OK) return JSDR_ERR;
    if (sh.fft_state && fft_mode_alloc(h, kind, true) != JSDR_OK) {
        set_error("jsdr_bpsk_restore: could not allocate the FFT-acquire buffers the blob's mode needs (%d streams of %d-sample frames); the "
                  "handle is unchanged", h->nstreams, h->nsf);
        return JSDR_ERR;
    }
    JSDR_HIP_TRY(hipMemcpy(h->state_img.p, blob_record(blob_host, 0), (size_t)count * BLOB_RECORD_BYTES, hipMemcpyHostToDevice));
    const bool timed = ckpt_events(h);
    if (timed) (void)hipEventRecord(h->ev_state[0], 0);
    if (launch_state_unpack(ckpt_args(h, dst_first, count), 0) != JSDR_OK) return JSDR_ERR;
    if (timed) (void)hipEventRecord(h->ev_state[1], 0);
    JSDR_HIP_TRY(hipStreamSynchronize(0));
    h->state_unpack_ms = ckpt_elapsed(h, timed);
    if (h->pst)
        for (int i = 0; i < count; i++) h->pst_tuning[(size_t)(dst_first + i)] = blob_get_f64(blob_record(blob_host, (uint32_t)i) + REC_PST_F64);
    if (fresh) {
        if (h->acq_scratch.p && ((sh.do_up != 0) != (h->do_up != 0) || (sh.do_fft != 0) != (h->do_fft != 0))) {
            h->acq_scratch.release();  // (cut for another band: allocated again by the next call that needs it)
            h->acq_chunk = 0;
        }
        h->tuning = sh.tuning;
        h->do_fft = (int)sh.do_fft;
        h->do_up = (int)sh.do_up;
        h->seam = (int)sh.seam;
        h->hist_is_float = sh.hist_float != 0;
        h->dsCnt = sh.ds_cnt;
        h->n_in = sh.n_in;
        h->n_ds = sh.n_ds;
        h->tuPhase = sh.tu_phase;
        h->tuPhaseInc = sh.tu_inc;
        h->vcoPhase = sh.vco_phase;
        memcpy(h->h_khist, sh.khist, BLOB_HIST);
        memcpy(h->h_mhist, sh.mhist, BLOB_HIST);
    }
    // the host scheduler starts over from the state as it stands: no schedule kept, no table on the device taken for current
    h->cur.valid = false;
    h->prefetch.valid = false;
    h->tables_on_device = false;
    h->ktu_uploaded = false;
    h->vco_cs_in_blob = false;
    h->retuned = true;  // (as after live control: the fast variant's replay from creation would not see this)
    h->restored = true;
    if (h->trace_void.empty()) h->trace_void.assign((size_t)h->nstreams, 0);
    for (int i = 0; i < count; i++) h->trace_void[(size_t)(dst_first + i)] = 1;
    return JSDR_OK;
}

int jsdr_bpsk_blob_info(const void *blob_host, size_t bytes, jsdr_bpsk_blob_info_t *out)
{
    JSDR_REQUIRE(blob_host && out, "jsdr_bpsk_blob_info: null pointer");
    BlobShared sh;
    uint32_t n = 0;
    char why[192];
    JSDR_REQUIRE(blob_parse(blob_host, bytes, &sh, &n, why, sizeof(why)), "jsdr_bpsk_blob_info: %s", why);
    memset(out, 0, sizeof(*out));
    out->version = BLOB_VERSION;
    out->kind = (int32_t)sh.kind;
    out->rate = (int32_t)sh.rate;
    out->nsamples_per_frame = (int32_t)sh.nsf;
    out->nstreams = (int32_t)n;
    out->do_fft = (int32_t)sh.do_fft;
    out->do_up = (int32_t)sh.do_up;
    out->seam = (int32_t)sh.seam;
    out->record_bytes = BLOB_RECORD_BYTES;
    out->header_bytes = BLOB_HEADER_BYTES;
    out->n_in = sh.n_in;
    out->n_ds = sh.n_ds;
    out->tuning_hz = sh.tuning;
    return JSDR_OK;
}
