// bpsk_call.hip -- an ordinary handle's call, end to end: the schedule glue, the stages of a call (shared with chan_run and
// pst_run), bpsk_run, and the batch / receive / recover entry points.  Host code only (bpsk_handle.h).
#include "bpsk_handle.h"
#include <stddef.h>
#include <stdlib.h>

static_assert((int)SCHED_TABLE_SLACK == (int)FM_TABLE_SLACK, "the scheduler's periodic table carries what k_fm reads past one period");

// the three-phase front end's per-phase timing hook (AcqProf::mark, ctx: an AcqProfCtx)
static void acq_prof_mark(void *ctx, int phase, bool begin, hipStream_t st)
{
    AcqProfCtx *c = static_cast<AcqProfCtx *>(ctx);
    if (!c->h->prof_on) return;
    if (begin) {
        c->a[phase] = prof_event(c->h);
        (void)hipEventRecord(c->a[phase], st);
    } else {
        Event b = prof_event(c->h);
        (void)hipEventRecord(b, st);
        c->h->prof_recs.push_back({PK_ACQ_FWD + phase, std::move(c->a[phase]), std::move(b)});
    }
}

// what a call of L samples from the handle's present state needs of its schedule
static ScheduleKey schedule_request(const jsdr_bpsk *h, long long L, bool first)
{
    ScheduleKey k;
    k.tu0 = h->tuPhase;
    k.inc = h->tuPhaseInc;
    k.vco0 = h->vcoPhase;
    k.ds0 = h->dsCnt;
    k.decim = h->decim;
    k.L = L;
    k.do_fft = h->do_fft != 0;
    k.first = first;
    memcpy(k.khist0, h->h_khist, sizeof(k.khist0));
    return k;
}

// the handle's state moves to the end of the call h->cur describes
static void schedule_advance(jsdr_bpsk *h)
{
    h->tuPhase = h->cur.tu1;
    h->vcoPhase = h->cur.vco1;
    h->dsCnt = h->cur.ds1;
    memcpy(h->h_khist, h->cur.ktu.data() + h->cur.key.L, 26);
}

// Returns the number of decimated outputs of a call of L samples and leaves its schedule in h->cur.
long long jsdr::build_schedule(jsdr_bpsk *h, long long L)
{
    const bool first = h->n_in == 0;
    const ScheduleKey want = schedule_request(h, L, first);
    // (a schedule computed for a stream's first call also serves a later call from the same state)
    if (h->tables_on_device && h->cur.valid && h->cur.key.same_call(want)) {
        schedule_advance(h);
        return h->cur.nds;
    }
    if (h->worker.joinable()) h->worker.join();
    Schedule &pf = h->prefetch;
    if (!schedule_matches(pf, want)) {
        schedule_key(pf, want);
        compute_schedule(pf, h->h_sincos.data());
        h->sched_sync++;
    } else {
        h->sched_prefetched++;
    }
    // adopt it (the structs change places: the outgoing vectors become the worker's scratch)
    std::swap(h->cur, pf);
    pf.valid = false;
    h->tables_on_device = false;  // refreshed by the caller
    const ScheduleKey from = h->cur.key;
    schedule_advance(h);
    // the next call, assuming the same length: nothing to do if the state has come back to where this call started (h->cur
    // will serve it), otherwise step it on the worker thread while the GPU runs this call
    const ScheduleKey next = schedule_request(h, L, false);
    if (!next.same_call(from) && h->prefetch_on && L >= 65536) {  // (a short call's schedule costs less than starting a thread)
        schedule_key(pf, next);
        const double *sincos = h->h_sincos.data();
        Schedule *dst = &pf;
        h->worker = std::thread([dst, sincos] { compute_schedule(*dst, sincos); });
    }
    return h->cur.nds;
}

// The side section of a call: the 9600 Hz tail, the sync correlation and the FEC of every hit, on the handle's side stream
// (the caller's when there is none), after the front end of THAT call.  Everything it needs from the call is in the job.
struct SideJob {
    int yb = 0;
    long long nds = 0, g_first = 0;
    int first_out = 0, ic = 0, qc = 0;
    const int *raw = nullptr;
    long long stride_pairs = 0;
    unsigned char *kvco_p = nullptr;
    double2 *tcs_p = nullptr;
    hipStream_t st = nullptr;
};

static int run_side(jsdr_bpsk *h, const SideJob &j)
{
    const int S = h->nstreams;
    const int yb = j.yb;
    hipStream_t ts = h->overlap ? h->tail_stream : j.st;
    if (h->overlap) JSDR_HIP_TRY(hipStreamWaitEvent(ts, h->ev_matched, 0));
    if (h->pack_pending) {  // a pack of the previous call's results may still be reading what the tail section rewrites
        JSDR_HIP_TRY(hipStreamWaitEvent(ts, h->ev_pack_done, 0));
        h->pack_pending = false;
    }
    {
        TailArgs ta;
        ta.y = h->y[yb].p + Y_PAD;
        ta.y_stride = h->y_stride;
        ta.nds = j.nds;
        ta.g_first = j.g_first;
        ta.st = h->tail.p;
        ta.bitlog_new = h->bitlog[h->bitlog_cur ^ 1].p;
        ta.bitlog_old = h->bitlog[h->bitlog_cur].p;
        ta.bitlog_stride = h->bitlog_stride;
        ta.nbits = h->nbits.p;
        ta.max_bits = h->max_bits;
        ta.nstreams = S;
        ta.ey = h->fast_ey;
        ta.amax = h->amax.p;
        ta.margin_scale = h->margin_scale;
        ta.argmax_scale = h->argmax_scale;
        ta.raw = j.raw;
        ta.stride_pairs = j.stride_pairs;
        ta.ic = j.ic;
        ta.qc = j.qc;
        ta.decim = h->decim;
        ta.first_out = j.first_out;
        ta.mix = h->cur.mix;
        ta.tper = (h->cur.mix == 1) ? h->cur.tper : 0;
        ta.tcs = j.tcs_p;
        ta.kvco = j.kvco_p;
        ta.sincos = h->sincos.p;
        ProfScope ps(h, PK_TAIL, ts);
        // (the fast variant's certified tail re-reads the call's raw input: tune mode, int16 input)
        const char *tail = launch_tail(ta, h->variant != 0 && !h->do_fft && j.raw, ts);
        if (!tail) return JSDR_ERR;
        h->tail_name = tail;
        h->bitlog_cur ^= 1;
    }
    {
        SyncArgs sa;
        sa.bitlog = h->bitlog[h->bitlog_cur].p;
        sa.bitlog_stride = h->bitlog_stride;
        sa.nbits = h->nbits.p;
        sa.corr = h->corr.p;
        sa.max_bits = h->max_bits;
        SyncFinArgs sf;
        sf.trig_count = h->trig_count.p;
        sf.trig_bits = h->trig_bits.p;
        sf.trig_cap = h->trig_cap;
        sf.st = h->tail.p;
        const bool transposed = sync_t_applies(h->max_bits);
        // (the hand-over inside the workgroup is a device-scope release / acquire pair: an L2 write-back per
        //  workgroup on this multi-XCD part -- nothing for one stream, a tax beside the PSD kernel for thousands)
        sf.fuse = (transposed && S == 1 && j.nds <= 16384) ? 1 : 0;  // at most ~2000 new bits: the scan is a few dozen iterations
        {
            ProfScope ps(h, transposed ? PK_SYNCT : PK_SYNC, ts);  // timed under the name rocprof shows
            if ((transposed ? launch_sync_t(sa, sf, S, ts) : launch_sync(sa, j.nds, S, ts)) != JSDR_OK) return JSDR_ERR;
            if (!sf.fuse) {
                ProfScope ps2(h, PK_SYNCFIN, ts);
                if (launch_sync_fin(sa, sf, S, ts) != JSDR_OK) return JSDR_ERR;
            }
        }
        BpskFecArgs fa2;
        fa2.bitlog = h->bitlog[h->bitlog_cur].p;
        fa2.bitlog_stride = h->bitlog_stride;
        fa2.trig_count = h->trig_count.p;
        fa2.trig_bits = h->trig_bits.p;
        fa2.max_trig = h->trig_cap;
        fa2.decoded = h->decoded.p;
        fa2.fec_rc = h->fec_rc.p;
        fa2.fec_data = h->fec_data.p;
        fa2.last = h->fec_last.p;
        fa2.cnt_dec = h->cnt_dec.p;
        fa2.nstreams = S;
        fa2.dec_scratch = h->fec_scratch.p;
        fa2.done = h->fec_done.p;
        fa2.fuse = (S == 1) ? 1 : 0;
        fa2.ncopy = 0;
        fa2.vit = h->fec_vit.p;  // (null below VIT64_MIN_STREAMS: one wave per block)
        fa2.work_count = h->fec_work.p;
        fa2.work_list = h->fec_work.p ? h->fec_work.p + 1 : nullptr;
        h->snap_fused = false;
        if (S == 1 && h->pin_call) {  // receive(): the snapshot is packed by the block that completes the FEC work
            SnapPack *sp = h->snap_dev.p;
            auto add = [&](const void *src, void *dst, size_t bytes) {
                fa2.csrc[fa2.ncopy] = static_cast<const unsigned char *>(src);
                fa2.cdst[fa2.ncopy] = static_cast<unsigned char *>(dst);
                fa2.cbytes[fa2.ncopy] = (int)bytes;
                fa2.ncopy++;
            };
            add(h->tail.p, &sp->t, sizeof(TailState));
            add(h->fec_last.p, sp->last, 2 * sizeof(int));
            add(h->cnt_dec.p, &sp->cdec, sizeof(int));
            add(h->nbits.p, &sp->nbits, sizeof(int));
            if (stream_fft(h, 0)) {
                add(&h->fft_state.p->centreBin, &sp->centreBin, sizeof(int));
                add(&h->fft_state.p->avePeakPower, &sp->avePeakPower, 2 * sizeof(double));  // avePeakPower, aveCentreBin
            }
            add(h->decoded.p, sp->decoded, 256);
            // the call's bits: what the log holds behind the history (the host clears the snapshot's bytes beyond nbits)
            const long long have = h->bitlog_stride - HIST_BITS;
            add(h->bitlog[h->bitlog_cur].p + HIST_BITS, sp->bits, (size_t)(have < 512 ? have : 512));
            h->snap_fused = true;
        }
        ProfScope ps(h, PK_FEC, ts);
        h->fec_name = (fa2.vit && !fa2.fuse) ? "k_fec_bits+k_vitq+k_fec_rs" : "k_fec_bpsk";
        if (launch_fec_bpsk(fa2, ts) != JSDR_OK) return JSDR_ERR;
    }
    if (h->overlap) {
        JSDR_HIP_TRY(hipEventRecord(h->ev_tail_done[yb], ts));
        h->tail_pending[yb] = true;
        h->y_cur ^= 1;
    }
    return JSDR_OK;
}

// ------------------------------------------------------------------------------------------- the stages of a call
// One function per stage; chan_run, pst_run and bpsk_run call them in the order their work goes onto the caller's stream.

// CUs of the device, asked once per handle (256 where the runtime does not say); 0: the query failed
int jsdr::device_cus(jsdr_bpsk *h)
{
    if (h->num_cu == 0) {
        int dev = 0, cus = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) {
            set_error("bpsk: the device's CU count could not be read: %s", hipGetErrorString(e));
            return 0;
        }
        h->num_cu = cus > 0 ? cus : 256;
    }
    return h->num_cu;
}

// The three-phase front end's scratch (what its phases hand each other), allocated at the first call that needs it:
// `rows` rows (streams, or inputs of a channel handle) of per_row_frame bytes a frame, for the largest call the handle takes,
// capped (JSDR_ACQ_SCRATCH_MB, default 6 GiB): longer calls go in several launches of acq_chunk frames per row
int jsdr::acq_scratch_ensure(jsdr_bpsk *h, size_t per_row_frame, size_t rows, size_t slack)
{
    if (h->acq_scratch.p) return JSDR_OK;
    long long cap_mb = 6144;
    if (const char *e = knob("JSDR_ACQ_SCRATCH_MB")) cap_mb = atoll(e) > 0 ? atoll(e) : cap_mb;
    long long fmax = h->max_batch / h->nsf;
    if (fmax < 1) fmax = 1;
    long long chunk = (cap_mb << 20) / (long long)(per_row_frame * rows);
    if (chunk < 1) chunk = 1;
    if (chunk > fmax) chunk = fmax;
    if (const char *e = knob("JSDR_ACQ_CHUNK")) chunk = atoll(e) > 0 && atoll(e) < chunk ? atoll(e) : chunk;
    if (h->acq_scratch.alloc(per_row_frame * rows * (size_t)chunk + slack) != JSDR_OK) return JSDR_ERR;
    h->acq_chunk = (int)chunk;
    return device_cus(h) ? JSDR_OK : JSDR_ERR;
}

// the FFT-acquire front ends' arguments for a call of L samples (whole frames) with nds outputs
FftFrontArgs jsdr::fft_front_args(jsdr_bpsk *h, const int *raw, const float2 *rawf, long long stride_pairs, long long L, int ic, int qc,
                                  int first_out, long long nds)
{
    FftFrontArgs xa;
    xa.raw = raw;
    xa.rawf = rawf;
    xa.stride_pairs = stride_pairs;
    xa.nframes = (int)(L / h->nsf);
    xa.n = h->nsf;
    xa.logn = h->logn;
    xa.ic = ic;
    xa.qc = qc;
    xa.do_up = h->do_up;
    xa.decim = h->decim;
    xa.first_out = first_out;
    // (receive() of a 1-stream handle may have sent the factors behind the frame)
    xa.vco_cs = h->vco_cs_in_blob ? reinterpret_cast<const double2 *>(reinterpret_cast<const unsigned char *>(h->stage_raw.p) + h->vco_cs_blob_off)
                                  : h->vco_cs.p;
    xa.tw = h->fft_tw.p;
    xa.st = h->fft_state.p;
    xa.dm = h->dm.p;
    xa.dm_stride = h->dm_stride;
    xa.nds = nds;
    xa.ds_taps = h->ds_taps_dev.p;
    xa.phase_clk = h->phase_clk.p;
    return xa;
}

void jsdr::acq_launch_ctx(jsdr_bpsk *h, AcqLaunchCtx &c)
{
    c.pc.h = h;
    c.prof.ctx = &c.pc;
    c.prof.mark = acq_prof_mark;
}

// the VCO factors of the call's outputs, the one table the FFT-acquire front ends read (:515-516)
static void fill_vco_cs(const jsdr_bpsk *h, double2 *dst, long long nds)
{
    const std::vector<unsigned char> &kvco = h->nch > 0 ? h->vco.kvco : h->cur.kvco;  // (a channel handle keeps the VCO's alone)
    for (long long j = 0; j < nds; j++) dst[j] = make_double2(h->h_sincos[kvco[(size_t)j]], h->h_sincos[256 + kvco[(size_t)j]]);
}

// ... through the handle's own table (the call's ordinary copy)
int jsdr::send_vco_cs(jsdr_bpsk *h, long long nds, hipStream_t st)
{
    h->h_vco_cs.resize((size_t)nds);
    fill_vco_cs(h, h->h_vco_cs.data(), nds);
    return h2d_call(h, h->vco_cs.p, h->h_vco_cs.data(), sizeof(double2) * (size_t)nds, st);
}

// k_front_split's and k_chan_front's table: cos[0..256], sin[0..256] with (1.0, 1.0) at 256 (the pass-through entry, :395)
int jsdr::sincos9_ensure(jsdr_bpsk *h)
{
    if (h->sincos9.p) return JSDR_OK;
    std::vector<double> t(514);
    for (int k = 0; k < 256; k++) {
        t[(size_t)k] = h->h_sincos[(size_t)k];
        t[(size_t)(257 + k)] = h->h_sincos[(size_t)(256 + k)];
    }
    t[256] = 1.0;
    t[513] = 1.0;
    if (h->sincos9.alloc(514) != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipMemcpy(h->sincos9.p, t.data(), sizeof(double) * 514, hipMemcpyHostToDevice));
    return JSDR_OK;
}

// the 64-sample halo of VCO-mixed samples lives where the previous call's path left it: dm[s][0..63] or dmh (k_fm's)
static int move_halo(jsdr_bpsk *h, bool to_dmh, hipStream_t st)
{
    double2 *dmh = h->dmh[h->dmh_cur].p;
    const size_t row = 64 * sizeof(double2), pitch = (size_t)h->dm_stride * sizeof(double2);
    JSDR_HIP_TRY(hipMemcpy2DAsync(to_dmh ? dmh : h->dm.p, to_dmh ? row : pitch, to_dmh ? h->dm.p : dmh, to_dmh ? pitch : row, row,
                                  (size_t)h->nstreams, hipMemcpyDeviceToDevice, st));
    h->halo_in_dmh = to_dmh;
    return JSDR_OK;
}

int jsdr::run_hist_in(jsdr_bpsk *h, const HistArgs &ha, hipStream_t st)
{
    ProfScope ps(h, PK_HIST, st);
    if (launch_hist_in(ha, st) != JSDR_OK) return JSDR_ERR;
    h->hist_cur ^= 1;
    return JSDR_OK;
}

// The 26-sample input history is kept in the form of the input that wrote it.  A call of the other form gets it converted
// (k_hist_convert): int16 -> float always exists; float -> int16 exists exactly when every float is some (float)s/32767f, and a
// call that finds another float is refused.  The conversion is made on a COPY in the idle history buffer, which becomes the
// current one only when it holds: a refused call leaves the handle as it was.  rows: streams, or inputs of a channel handle.
int jsdr::hist_form(jsdr_bpsk *h, bool want_float, int rows, hipStream_t st)
{
    if (h->n_in > 0 && want_float != h->hist_is_float) {
        int2 *cur = h->hist_in[h->hist_cur].p, *idle = h->hist_in[h->hist_cur ^ 1].p;
        JSDR_HIP_TRY(hipMemcpyAsync(idle, cur, sizeof(int2) * 32 * (size_t)rows, hipMemcpyDeviceToDevice, st));
        JSDR_HIP_TRY(hipMemsetAsync(h->hist_bad.p, 0, sizeof(int), st));
        if (launch_hist_convert(idle, rows, want_float ? 1 : 0, h->hist_bad.p, st) != JSDR_OK) return JSDR_ERR;
        if (!want_float) {
            int bad = 0;
            JSDR_HIP_TRY(hipMemcpyAsync(&bad, h->hist_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
            JSDR_HIP_TRY(hipStreamSynchronize(st));
            JSDR_REQUIRE(!bad, "bpsk: int16 input after float frames whose samples are not (float)s/32767f values: the input "
                         "history cannot be carried over");
        }
        h->hist_cur ^= 1;
    }
    h->hist_is_float = want_float;
    return JSDR_OK;
}

// first block boundary of the matched filter's tiling (slot 0 <=> g == 64 mod 65) at or before g_first; may be "negative" for g < 64
static long long first_block(long long g_first)
{
    return g_first - (((g_first - 64) % 65 + 65) % 65);
}

// the 65-tap matched filter over dm into y[yb], then the 64 samples the next call's filter reaches back into
int jsdr::run_matched(jsdr_bpsk *h, int yb, long long nds, long long g_first, hipStream_t st)
{
    const int S = h->nstreams;
    MatchedArgs ma;
    ma.dm = h->dm.p;
    ma.dm_stride = h->dm_stride;
    ma.y = h->y[yb].p + Y_PAD;
    ma.y_stride = h->y_stride;
    ma.nds = nds;
    ma.g_first = g_first;
    ma.tile0 = first_block(g_first);
    {
        ProfScope ps(h, PK_MATCHED, st);
        if (launch_matched(ma, S, st) != JSDR_OK) return JSDR_ERR;
    }
    ProfScope ps2(h, PK_DMHIST, st);
    return launch_dm_history(h->dm.p, h->dm_stride, nds, S, st);
}

// The end of every call: the side section (tail, sync, FEC) of the call goes out, and the handle's counters move on.
int jsdr::finish_call(jsdr_bpsk *h, int yb, long long L, long long nds, long long g_first, int first_out, int ic, int qc,
                      const int *raw, long long stride_pairs, unsigned char *kvco_p, double2 *tcs_p, hipStream_t st)
{
    SideJob job;
    job.yb = yb;
    job.nds = nds;
    job.g_first = g_first;
    job.first_out = first_out;
    job.ic = ic;
    job.qc = qc;
    job.raw = raw;
    job.stride_pairs = stride_pairs;
    job.kvco_p = kvco_p;
    job.tcs_p = tcs_p;
    job.st = st;
    if (h->overlap) JSDR_HIP_TRY(hipEventRecord(h->ev_matched, st));
    // (the side section goes out now.  In the pipeline it then waits behind the NEXT call's PSD kernel anyway -- k_fft holds
    //  every register of every SIMD, a tail wave finds no room until it ends -- and runs beside the first 5 ms of that call's
    //  k_fm: profiles/r04_b_timeline.txt.  Holding it back on the host until the next call's start measured slower.)
    if (run_side(h, job) != JSDR_OK) return JSDR_ERR;
    h->last_y = yb;
    h->trace_void.clear();
    h->n_in += L;
    h->n_ds += nds;
    h->last_nds = nds;
    h->last_stream = st;
    return JSDR_OK;
}

// ------------------------------------------------------------------------------------------- an ordinary handle's call
// The call's VCO / tuner tables to the device, when they changed (`fresh`).  receive(): the frame is at the arena's head and goes
// here too; when the call takes k_fm, the fresh tables ride behind the frame in the same copy and k_fm_prep scatters them from
// `sc` (three copies were ~10 us each of a 70 us call).
static int send_tables(jsdr_bpsk *h, bool fm_ok, bool fresh, long long nds, ScatterArgs &sc, hipStream_t st)
{
    unsigned char *kvco_p = kvco_cur(h);
    double2 *tcs_p = tcs_cur(h);
    memset(&sc, 0, sizeof(sc));
    bool tables_sent = false;
    if (h->rx_frame_bytes) {
        size_t total = h->rx_frame_bytes;
        const size_t o1 = (total + 63) & ~(size_t)63;
        const size_t tcs_bytes = h->cur.tper > 0 ? sizeof(double2) * h->cur.tcs.size() : 0;
        const size_t o2 = (o1 + (size_t)nds + 63) & ~(size_t)63;
        if (fm_ok && fresh && nds > 0 && o2 + tcs_bytes <= h->pin_bytes && o2 + tcs_bytes <= h->stage_raw.n * sizeof(int)) {
            unsigned char *dev = reinterpret_cast<unsigned char *>(h->stage_raw.p);
            memcpy(h->pin.p + o1, h->cur.kvco.data(), (size_t)nds);
            sc.src[0] = dev + o1;
            sc.dst[0] = kvco_p;
            sc.bytes[0] = (int)nds;
            if (tcs_bytes) {
                memcpy(h->pin.p + o2, h->cur.tcs.data(), tcs_bytes);
                sc.src[1] = dev + o2;
                sc.dst[1] = reinterpret_cast<unsigned char *>(tcs_p);
                sc.bytes[1] = (int)tcs_bytes;
            }
            total = o2 + tcs_bytes;
            h->pin_off = total;
            tables_sent = true;
        }
        else if (h->do_fft && fresh && nds > 0) {
            // FFT-acquire mode: the VCO factors of the call's outputs (the only table its front end reads) behind the frame
            // (at a FIXED offset behind the largest frame form -- a float frame: parked behind the int16 frame, the factors of
            //  a cached schedule were overwritten by the next float frame that failed the short-grid check, and read as they were)
            const size_t ov = (sizeof(float) * 2 * (size_t)h->nsf + 63) & ~(size_t)63, vb = sizeof(double2) * (size_t)nds;
            if (ov + vb <= h->pin_bytes && ov + vb <= h->stage_raw.n * sizeof(int)) {
                fill_vco_cs(h, reinterpret_cast<double2 *>(h->pin.p + ov), nds);
                total = ov + vb;
                h->pin_off = total;
                h->vco_cs_in_blob = true;
                h->vco_cs_blob_off = ov;
                tables_sent = true;
            }
        }
        JSDR_HIP_TRY(hipMemcpyAsync(h->stage_raw.p, h->pin.p, total, hipMemcpyHostToDevice, st));
        h->rx_frame_bytes = 0;
    }
    if (fresh && tables_sent) h->tables_on_device = true;
    if (fresh && !tables_sent) {
        if (nds > 0)
            if (h2d_call(h, kvco_p, h->cur.kvco.data(), (size_t)nds, st) != JSDR_OK) return JSDR_ERR;
        if (nds > 0 && h->do_fft) {
            h->vco_cs_in_blob = false;
            if (send_vco_cs(h, nds, st) != JSDR_OK) return JSDR_ERR;
        }
        if (h->cur.tper > 0)
            if (h2d_call(h, tcs_p, h->cur.tcs.data(), sizeof(double2) * h->cur.tcs.size(), st) != JSDR_OK) return JSDR_ERR;
        // the host vectors must stay untouched until the copies ran; pageable memcpyAsync stages
        // synchronously, so they are safe to reuse on return
        h->tables_on_device = true;
    }
    return JSDR_OK;
}

// the FFT-acquire front end over the frames of xa, a call of L samples a stream (the first call after a switch from the tune
// mode runs it twice)
static int fft_front(jsdr_bpsk *h, FftFrontArgs &xa, long long L, hipStream_t st)
{
    const int S = h->nstreams;
    // round 6: frames of 2^k samples, two or more per stream in the call: three phases over FRAMES (bpsk_acq.hip); a call of
    // one frame per stream (a live receive()) keeps the fused kernel -- one launch instead of four
    // The 2^k frames' three-phase kernels are the faster ones per frame as well (n = 2048, 1024 x 2^20: 8.65 against 9.1 ms);
    // the default mixed-radix frames' are the fused kernel's passes cut in two and cost 10-14 % more per frame at a full grid
    // (9600: 12.6 against 11.5 ms; the spectrum rows' round trip, a ticket a frame) -- they are taken where frames fill the
    // chip better than streams: ceil(S F / W) * 1.15 < ceil(S / W) * F, W = the workgroups the chip holds (one a CU).
    const FftFront kind = h->fft_plan.kind;
    bool three = kind != FRONT_FFT2X && acq3_supported(h->nsf) && h->acq_mode != 0 && (xa.nframes >= 2 || h->acq_mode == 1) &&
                 L < 0x7fffffffLL && (long long)S * ((xa.nframes + 1) / 2) < 0x7fffffffLL;  // (its kernels' 32-bit frame arithmetic)
    if (kind == FRONT_GEN) three = true;  // (no fused kernel exists for these frames)
    if (three && kind == FRONT_FFTM && h->acq_mode < 0) {
        if (!device_cus(h)) return JSDR_ERR;
        const long long W = h->num_cu, F = xa.nframes;
        // (4800 / 4410: the fused kernel takes two frames at once and is 1.38 / 1.27 x the three-phase kernels' pace at a full grid)
        const double pace = (h->nsf == 4800 && F >= 2) ? 1.4 : (h->nsf == 4410 && F >= 2) ? 1.3 : 1.15;
        three = (double)(((long long)S * F + W - 1) / W) * pace < (double)((((long long)S + W - 1) / W) * F);
    }
    if (three) {
        const size_t per = acq3_frame_bytes(h->nsf, h->do_up) + 64 + (kind == FRONT_GEN ? acqg_image_bytes(h->nsf) : 0);
        if (acq_scratch_ensure(h, per, (size_t)S, 512) != JSDR_OK) return JSDR_ERR;  // (per stream and frame)
        h->front_name = kind == FRONT_GEN ? "k_acqg_pass" : kind == FRONT_FFTM ? "k_acqm_fwd" : "k_acq_fwd";
        AcqLaunchCtx lc;
        acq_launch_ctx(h, lc);
        if (launch_acq3(xa, S, h->acq_scratch.p, h->acq_scratch.n, h->acq_chunk, h->num_cu, st, lc.prof, h->fft_plan) != JSDR_OK) return JSDR_ERR;
    } else {
        ProfScope ps(h, PK_FRONT, st);
        h->front_name = kind == FRONT_FFT2X ? "k_front_fft2x" : (kind == FRONT_FFTM ? (fftm_pairs(xa.n, xa.nframes) ? "k_front_fftm2" : "k_front_fftm") : "k_front_fft");
        const int frc = kind == FRONT_FFT2X ? launch_front_fft2x(xa, h->fft_plan, h->fft2x_ek.p, h->fft2x_r0.p, S, st)
                                         : (kind == FRONT_FFTM ? launch_front_fftm(xa, h->fft_plan, h->fft2x_ek.p, S, st) : launch_front_fft(xa, S, st));
        if (frc != JSDR_OK) return JSDR_ERR;
    }
    return JSDR_OK;
}

// An FFT-acquire call's front end, the tune -> FFT seam with it.  kh0 / mh0: the tuner indices / mix flags of the 26 samples
// before the call.
static int fft_acquire_front(jsdr_bpsk *h, FftFrontArgs xa, long long L, const unsigned char *kh0, const unsigned char *mh0, hipStream_t st)
{
    const int S = h->nstreams;
    if (h->seam == SEAM_TO_FFT) {
        // the first FFT-acquire call after jsdr_bpsk_set_mode switched from the tune mode.  dsBuf holds distinct I and Q
        // columns (tuner-mixed samples), the FFT front ends assume I == Q (:464 RxDownSample(re, re)); only the outputs
        // whose 27-tap windows reach back into that history differ.  The call runs with the I column as its history
        // (every output's fi is exact), then its first frame runs again from a copy of the FFT state with the Q column
        // into a scratch row (fq of those outputs is exact: the front end sums one rail, o = fi HOWARD, dm = (o cos, o sin)),
        // and k_seam_q takes the Q rail of those outputs from it.  Once per switch.
        SeamHist sh;
        memcpy(sh.khist, kh0, 26);
        memcpy(sh.mhist, mh0, 26);
        if (launch_seam_hist(h->hist_in[h->hist_cur].p, h->hist_is_float ? 1 : 0, h->sincos.p, sh, h->fft_state.p, h->fft_state2.p, S, st) != JSDR_OK)
            return JSDR_ERR;
    }
    if (fft_front(h, xa, L, st) != JSDR_OK) return JSDR_ERR;
    if (h->seam == SEAM_TO_FFT) {
        long long nds1 = 0;
        const long long J = seam_outputs((int)xa.first_out, h->nsf, h->decim, xa.nds, &nds1);
        if (J > 0) {
            const char *keep = h->front_name;
            FftFrontArgs x1 = xa;
            x1.nframes = 1;
            x1.st = h->fft_state2.p;
            x1.dm = h->dm2.p;
            x1.dm_stride = h->dm2_stride;
            x1.nds = nds1;
            x1.phase_clk = nullptr;
            if (fft_front(h, x1, L, st) != JSDR_OK) return JSDR_ERR;
            h->front_name = keep;
            if (launch_seam_q(h->dm.p, h->dm_stride, h->dm2.p, h->dm2_stride, (int)J, S, st) != JSDR_OK) return JSDR_ERR;
        }
        h->seam = SEAM_NONE;
    }
    return JSDR_OK;
}

// The fused front end + matched filter of a tune-mode call into y[y_cur]: k_fm_prep (the streams' edge images, the next call's
// 26-sample input history -- k_hist_in's work -- and, from `sc`, receive()'s tables) and k_fm; k_fm_prep_f32 and k_fm_f32 for
// a float batch.  fa: the call as the three-kernel front ends would take it.
static int fused_front(jsdr_bpsk *h, const FrontArgs &fa, const ScatterArgs &sc, long long g_first, hipStream_t st)
{
    const int S = h->nstreams, ic = fa.ic, qc = fa.qc;
    const long long L = fa.nsamples;
    if (wait_tail(h, h->y_cur, st) != JSDR_OK) return JSDR_ERR;
    FmArgs ma;
    ma.raw = fa.raw;
    ma.stride_pairs = fa.stride_pairs;
    ma.nsamples = (int)L;
    ma.ic = ic;
    ma.qc = qc;
    ma.edges = h->fm_edges.p;
    ma.tcs = tcs_cur(h);
    ma.tper = h->cur.mix ? h->cur.tper : 1;
    ma.kvco = kvco_cur(h);
    ma.sincos = h->sincos.p;
    ma.dmh_old = h->dmh[h->dmh_cur].p;
    ma.dmh_new = h->dmh[h->dmh_cur ^ 1].p;
    ma.y = h->y[h->y_cur].p + Y_PAD;
    ma.y_stride = h->y_stride;
    ma.nds = (int)fa.nds;
    ma.g_first = g_first;
    ma.tile0 = first_block(g_first);
    ma.first_out = fa.first_out;
    ma.amax = h->amax.p;
    ma.grid_limit = h->share_wgs_per_cu * h->num_cu;  // (jsdr_bpsk_set_cu_share has asked for the CU count)
    ma.tickets = h->fm_tickets.p;
    ma.trot = h->cur.mix == 1 ? h->cur.trot : -1;
    if (fa.rawf) {
        EdgeF32Args ea;
        ea.rawf = fa.rawf;
        ea.stride_pairs = fa.stride_pairs;
        ea.nsamples = (int)L;
        ea.hist = fa.hist;
        ea.edges = h->fm_edges_f32.p;
        ea.nstreams = S;
        const HistArgs ha = hist_args(h, nullptr, fa.rawf, fa.stride_pairs, L, 0, 0, S);
        ProfScope psh(h, PK_PREP, st);
        if (launch_fm_prep_f32(ea, ha, st) != JSDR_OK) return JSDR_ERR;
    } else {
        EdgeArgs ea;
        ea.raw = fa.raw;
        ea.stride_pairs = fa.stride_pairs;
        ea.nsamples = (int)L;
        ea.ic = ic;
        ea.qc = qc;
        ea.dc = (ic != 0) || (qc != 0);
        ea.hist = fa.hist;
        ea.edges = h->fm_edges.p;
        ea.nstreams = S;
        const HistArgs ha = hist_args(h, fa.raw, nullptr, fa.stride_pairs, L, ic, qc, S);
        ProfScope psh(h, PK_PREP, st);
        if (launch_fm_prep(ea, ha, sc, st) != JSDR_OK) return JSDR_ERR;
    }
    ProfScope ps(h, PK_FM, st);
    if (fa.rawf) {
        FmF32Args mf;
        mf.a = ma;
        mf.rawf = fa.rawf;
        mf.edges = h->fm_edges_f32.p;
        h->front_name = "k_fm_f32";
        if (launch_fm_f32(mf, h->decim, h->cur.mix != 0, S, st, &h->last_fm_items, &h->last_fm_grid) != JSDR_OK) return JSDR_ERR;
    } else {
        h->front_name = "k_fm";
        if (launch_fm(ma, h->decim, h->cur.mix != 0, (ic != 0) || (qc != 0), h->variant != 0, S, st, &h->last_fm_items, &h->last_fm_grid,
                      &h->last_fm_phase) != JSDR_OK)
            return JSDR_ERR;
    }
    h->dmh_cur ^= 1;
    return JSDR_OK;
}

static int bpsk_run(jsdr_bpsk *h, const int16_t *raw_dev, const float *rawf_dev, long long stride_i16, long long L,
                    int ic, int qc, hipStream_t st)
{
    JSDR_REQUIRE(h, "bpsk: null handle");
    if (h->nch > 0) return chan_run(h, raw_dev, rawf_dev, stride_i16, L, ic, qc, st);
    if (h->pst) return pst_run(h, raw_dev, rawf_dev, stride_i16, L, ic, qc, st);
    JSDR_REQUIRE(raw_dev || rawf_dev, "bpsk: null input");
    JSDR_REQUIRE(L > 0 && L <= h->max_batch, "bpsk: nsamples=%lld outside (0, max_batch_samples=%lld]", L, h->max_batch);
    JSDR_REQUIRE((stride_i16 & 1) == 0 && (h->nstreams == 1 || stride_i16 >= 2 * L),
                 "bpsk: stream stride %lld too small for %lld samples", stride_i16, L);
    JSDR_REQUIRE(!h->do_fft || (L % h->nsf) == 0, "bpsk: FFT-acquire mode needs whole frames (%lld %% %d != 0)", L, h->nsf);
    JSDR_REQUIRE(h->variant == 0 || raw_dev, "bpsk: the fast variant takes int16 input (its certification pass re-reads the raw samples)");
    JSDR_REQUIRE(h->seam != SEAM_TO_TUNE || L >= 26, "bpsk: the first tune-mode call after FFT-acquire frames needs at least 26 samples "
                 "(the input history is rebuilt from them)");
    // the fused float kernel's edge images (4 KB a stream), at the first float batch: what can fail for want of memory fails
    // before anything of the handle has moved on
    if (rawf_dev && h->f32_batch && h->use_fm && !h->fm_edges_f32.p && (h->decim == 4 || h->decim == 5 || h->decim == 10 || h->decim == 20))
        if (h->fm_edges_f32.alloc((size_t)h->nstreams * 4 * FM_EDGE) != JSDR_OK) return JSDR_ERR;
    // the previous call may have come through the other input form (before the schedule moves on: the conversion can refuse)
    if (!h->do_fft && h->seam != SEAM_TO_TUNE && hist_form(h, rawf_dev != nullptr, h->nstreams, st) != JSDR_OK) return JSDR_ERR;
    const int first_out = h->decim - 1 - h->dsCnt;
    const long long g_first = h->n_ds;
    unsigned char kh0[26], mh0[26];  // the tuner indices / mix flags of the 26 samples before the call (build_schedule moves them on)
    memcpy(kh0, h->h_khist, 26);
    memcpy(mh0, h->h_mhist, 26);
    h->last_fm_phase = -1;  // (until this call's k_fm says otherwise)
    const long long nds = build_schedule(h, L);
    JSDR_REQUIRE(nds <= h->max_ds, "bpsk: internal: %lld decimated samples exceed capacity %lld", nds, h->max_ds);
    // after a retune the call's samples, or the 26 history samples its first windows reach into, may lie on both sides of
    // the tuner's sign test (:388): those calls take k_front_split (in the steady state every flag is the call's own)
    const int f0 = h->cur.f0;
    const long long n0 = h->cur.n0;
    if (h->n_in == 0) memset(h->h_mhist, f0, 26);  // (the history of a stream's first call is zeros: either side is exact)
    bool split = false;
    if (!h->do_fft) {
        split = h->cur.mix < 0 || h->seam == SEAM_TO_TUNE;
        for (int i = 0; i < 26 && !split; i++) split = h->h_mhist[i] != (unsigned char)f0;
    }
    // fused path (k_fm; k_fm_f32 for the float batches of jsdr_bpsk_batch_f32): a tuner schedule that is periodic with a
    // period dividing the lane span (or no tuner at all), 32-bit sample indices
    const bool std_decim = h->decim == 4 || h->decim == 5 || h->decim == 10 || h->decim == 20;  // the specialised front ends
    const int fm_rd = h->decim == 4 ? 20 : h->decim * 4;  // D * R of the k_fm instantiation
    const bool per_ok = !h->do_fft && !split && h->cur.mix == 1 && h->cur.tper > 0 && fm_rd % h->cur.tper == 0;
    const bool fm_ok = h->use_fm && std_decim && !h->do_fft && !split && nds > 0 && L <= 0x3fffffffLL &&
                       ((raw_dev && !rawf_dev) || (rawf_dev && h->f32_batch && h->variant == 0 && h->fm_edges_f32.p)) && (h->cur.mix == 0 || per_ok);
    const bool fresh = !h->tables_on_device;
    if (fresh) {
        h->ktu_uploaded = false;
        // The VCO / tuner tables are double-buffered: the fast variant's tail (side stream) may still re-read those of
        // the previous call.  The half written now was last used two schedules ago; the tail that read it is the one
        // that also frees y[y_cur], so waiting for that one (not for the previous call's) keeps the overlap.
        h->tab_cur ^= 1;
        if (h->variant != 0 && wait_tail(h, h->y_cur, st) != JSDR_OK) return JSDR_ERR;
    }
    // the 1 B/sample index table is only read by the kernels without the periodic table (k_front, k_front_reg<PER = false>)
    const bool reg_will_run = front_reg_enabled() && std_decim && raw_dev && !rawf_dev && L <= 0x3fffffffLL && L >= 64;
    const bool need_ktu = !h->do_fft && !split && !fm_ok && !(per_ok && reg_will_run) && h->cur.mix != 0;
    if (need_ktu && !h->ktu_uploaded) {
        if (h2d_call(h, h->ktu.p, h->cur.ktu.data(), (size_t)L + 26, st) != JSDR_OK) return JSDR_ERR;
        h->ktu_uploaded = true;
    }
    ScatterArgs sc;
    if (send_tables(h, fm_ok, fresh, nds, sc, st) != JSDR_OK) return JSDR_ERR;
    if (split && nds > 0) {
        // k_front_split's index table: the schedule's index where the sample was mixed, 256 (pass-through) where not
        if (!h->ktu9.p && h->ktu9.alloc((size_t)h->max_batch + 26) != JSDR_OK) return JSDR_ERR;
        if (sincos9_ensure(h) != JSDR_OK) return JSDR_ERR;
        // (the history of the first tune call after FFT-acquire frames is the FFT path's unmixed doubles)
        expand_k9(h->h_ktu9, h->cur.ktu.data(), 0, L, h->seam != SEAM_TO_TUNE ? h->h_mhist : nullptr, f0, n0);
        if (h2d_call(h, h->ktu9.p, h->h_ktu9.data(), sizeof(unsigned short) * ((size_t)L + 26), st) != JSDR_OK) return JSDR_ERR;
    }
    // the 64-sample halo of VCO-mixed samples lives where the previous call's path left it
    if (nds > 0 && !h->do_fft && fm_ok != h->halo_in_dmh)
        if (move_halo(h, fm_ok, st) != JSDR_OK) return JSDR_ERR;
    const int S = h->nstreams;
    FrontArgs fa;
    fa.raw = reinterpret_cast<const int *>(raw_dev);
    fa.rawf = reinterpret_cast<const float2 *>(rawf_dev);
    fa.stride_pairs = stride_i16 / 2;
    fa.nsamples = L;
    fa.ic = ic;
    fa.qc = qc;
    fa.mix = h->cur.mix;
    fa.ktu = h->ktu.p;
    fa.kvco = kvco_cur(h);
    fa.sincos = h->sincos.p;
    fa.hist = h->hist_in[h->hist_cur].p;
    fa.dm = h->dm.p;
    fa.dm_stride = h->dm_stride;
    fa.ds_dbg = nullptr;
    fa.nds = nds;
    fa.first_out = first_out;
    fa.tcs = per_ok ? tcs_cur(h) : nullptr;
    fa.tper = h->cur.tper;
    bool hist_done = false;  // the next call's input history has been written (k_fm_prep does it in the k_fm path)
    if (h->do_fft && nds > 0 && h->halo_in_dmh)  // (the last tune call left the matched filter's halo in dmh)
        if (move_halo(h, false, st) != JSDR_OK) return JSDR_ERR;
    if (h->do_fft) {
        if (fft_acquire_front(h, fft_front_args(h, fa.raw, fa.rawf, fa.stride_pairs, L, ic, qc, first_out, nds), L, kh0, mh0, st) != JSDR_OK)
            return JSDR_ERR;
    } else if (nds > 0 && split) {
        ProfScope ps(h, PK_FRONT, st);
        h->front_name = "k_front_split";
        const FftFrontState *dh = h->seam == SEAM_TO_TUNE ? h->fft_state.p : nullptr;  // FFT -> tune: the history is doubles
        if (launch_front_split(fa, h->ktu9.p, h->sincos9.p, h->decim, dh, S, st) != JSDR_OK) return JSDR_ERR;
    } else if (nds > 0 && fm_ok) {
        if (fused_front(h, fa, sc, g_first, st) != JSDR_OK) return JSDR_ERR;
        hist_done = true;
    } else if (nds > 0) {
        ProfScope ps(h, PK_FRONT, st);
        // (not the fast form: a fast handle whose call cannot take k_fm runs it in exact order -- the amplitude the fast variant's
        //  bound scales with is tracked by k_fm only)
        const char *front = launch_front(fa, h->decim, S, false, st);
        if (!front) return JSDR_ERR;
        h->front_name = front;
    }
    if (!h->do_fft && hist_done) h->hist_cur ^= 1;
    if (!h->do_fft && !hist_done)
        if (run_hist_in(h, hist_args(h, fa.raw, fa.rawf, fa.stride_pairs, L, ic, qc, S), st) != JSDR_OK) return JSDR_ERR;
    const int yb = h->y_cur;
    if (wait_tail(h, yb, st) != JSDR_OK) return JSDR_ERR;
    if (nds > 0 && !(fm_ok && !h->do_fft) && run_matched(h, yb, nds, g_first, st) != JSDR_OK) return JSDR_ERR;
    if (finish_call(h, yb, L, nds, g_first, first_out, ic, qc, fa.raw, fa.stride_pairs, kvco_cur(h), tcs_cur(h), st) != JSDR_OK) return JSDR_ERR;
    if (!h->do_fft && h->seam == SEAM_TO_TUNE) {
        h->seam = SEAM_NONE;
        h->hist_is_float = rawf_dev != nullptr;
    }
    if (!h->do_fft) {
        mhist_advance(h->h_mhist, L, f0, n0);  // the mix flags of the 26 samples before the next call
    }
    return JSDR_OK;
}

// ------------------------------------------------------------------------------------------- the entry points
// the shadow's rows of a call's input, gathered into its own stream-major buffer
static int shadow_stage(const jsdr_bpsk *h, const std::vector<int> &ids, int16_t *in, const int16_t *raw_dev, int64_t stride,
                        int64_t nsamples, hipStream_t st)
{
    for (size_t i = 0; i < ids.size(); i++)
        JSDR_HIP_TRY(hipMemcpyAsync(in + i * (size_t)(2 * h->max_batch), raw_dev + (int64_t)ids[i] * stride,
                                    (size_t)nsamples * 4, hipMemcpyDeviceToDevice, st));
    return JSDR_OK;
}

int jsdr_bpsk_batch_i16(jsdr_bpsk *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic,
                        int qc, void *stream)
{
    if (bpsk_run(h, raw_dev, nullptr, stream_stride_i16, nsamples, ic, qc, as_stream(stream)) != JSDR_OK) return JSDR_ERR;
    h->batch_calls++;
    if (h->shadow) {  // the recovered streams, in exact order, in lock-step
        if (shadow_stage(h, h->shadow_ids, h->shadow_in.p, raw_dev, stream_stride_i16, nsamples, as_stream(stream)) != JSDR_OK) return JSDR_ERR;
        if (bpsk_run(h->shadow.get(), h->shadow_in.p, nullptr, 2 * h->max_batch, nsamples, ic, qc, as_stream(stream)) != JSDR_OK) return JSDR_ERR;
    }
    return JSDR_OK;
}

// batched IAudioHandler.receive(float[]): bpsk_run with the float input; its refusals are bpsk_run's / chan_run's checks, which come
// before any device work.
int jsdr_bpsk_batch_f32(jsdr_bpsk *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples, void *stream)
{
    JSDR_REQUIRE(h && iq_dev, "jsdr_bpsk_batch_f32: null argument");
    h->f32_batch = true;
    const int rc = bpsk_run(h, nullptr, iq_dev, stream_stride_f32, nsamples, 0, 0, as_stream(stream));
    h->f32_batch = false;
    return rc;
}

// Fast variant: the streams the calls so far left uncertified are REPLAYED from the handle's first call on an internal exact
// handle (every uncertified stream at once, in lock-step), which serves them from then on: their getters and their packed slots
// come from it, the sticky flag no longer withholds them, and every later batch call advances it beside the fast kernels.
// raw_dev_calls[k] / nsamples_calls[k]: what jsdr_bpsk_batch_i16 was given at call k -- ALL calls since creation, with the
// buffers still holding those samples (a batch over recordings has them; a live source does not and uses the exact variant).
// Why from the first call: the decision that could not be certified depends on the exact energy history, and after a fast call
// no exact state exists to restart from.  Cost: one small exact handle's call per call replayed (latency bound,
// about a millisecond each), whatever the number of streams recovered.
int jsdr_bpsk_recover_uncertified(jsdr_bpsk *h, const int16_t *const *raw_dev_calls, const int64_t *nsamples_calls, int ncalls,
                                  int64_t stream_stride_i16, int ic, int qc, int *recovered, void *stream)
{
    JSDR_REQUIRE(h && (ncalls == 0 || (raw_dev_calls && nsamples_calls)), "jsdr_bpsk_recover_uncertified: null argument");
    if (recovered) *recovered = 0;
    if (h->variant == 0) return JSDR_OK;
    JSDR_REQUIRE((long long)ncalls == h->batch_calls, "jsdr_bpsk_recover_uncertified: %d calls given, the handle has seen %lld (all of "
                 "them are replayed)", ncalls, h->batch_calls);
    long long total = 0;
    for (int k = 0; k < ncalls; k++) {
        JSDR_REQUIRE(raw_dev_calls[k] && nsamples_calls[k] >= 0 && nsamples_calls[k] <= h->max_batch, "jsdr_bpsk_recover_uncertified: call %d", k);
        total += nsamples_calls[k];
    }
    JSDR_REQUIRE(total == h->n_in, "jsdr_bpsk_recover_uncertified: the calls given hold %lld samples per stream, the handle has taken %lld",
                 total, h->n_in);
    if (sync_last(h) != JSDR_OK) return JSDR_ERR;
    std::vector<TailState> ts((size_t)h->nstreams);
    JSDR_HIP_TRY(hipMemcpy(ts.data(), h->tail.p, sizeof(TailState) * ts.size(), hipMemcpyDeviceToHost));
    std::vector<int> ids;
    int fresh = 0;
    for (int s = 0; s < h->nstreams; s++)
        if (ts[(size_t)s].uncertified) {
            ids.push_back(s);
            if (h->shadow_map.empty() || h->shadow_map[(size_t)s] < 0) fresh++;
        }
    if (fresh == 0) return JSDR_OK;  // nothing new to recover (the shadow, if any, is up to date)
    // the new shadow is built and replayed in locals and takes the old one's place only once every call has replayed: a failure
    // leaves the handle as it was, the old shadow still serving.  (The staging buffers are declared before the shadow: it goes
    // first, and its destroy waits for the replay that reads them.)
    DevBuf<int16_t> in;
    DevBuf<unsigned char> slots;
    jsdr_bpsk *made = nullptr;
    if (jsdr_bpsk_create(&made, h->rate, h->nsf, (int)h->tuning, 0, h->do_up, (int)ids.size(), h->max_batch) != JSDR_OK) return JSDR_ERR;
    decltype(h->shadow) sh(made);
    std::vector<int> map((size_t)h->nstreams, -1);
    for (size_t i = 0; i < ids.size(); i++) map[(size_t)ids[i]] = (int)i;
    int64_t sb = 0;
    (void)jsdr_bpsk_slot_info(h, &sb, nullptr, nullptr, nullptr, nullptr);
    if (in.alloc(ids.size() * (size_t)(2 * h->max_batch)) != JSDR_OK || slots.alloc(ids.size() * (size_t)sb) != JSDR_OK) return JSDR_ERR;
    for (int k = 0; k < ncalls; k++) {
        if (shadow_stage(h, ids, in.p, raw_dev_calls[k], stream_stride_i16, nsamples_calls[k], as_stream(stream)) != JSDR_OK ||
            bpsk_run(sh.get(), in.p, nullptr, 2 * h->max_batch, nsamples_calls[k], ic, qc, as_stream(stream)) != JSDR_OK)
            return JSDR_ERR;
    }
    std::swap(h->shadow, sh);  // (the old shadow and its buffers go with the locals)
    std::swap(h->shadow_in, in);
    std::swap(h->shadow_slots, slots);
    h->shadow_ids = ids;
    h->shadow_map.swap(map);
    h->recovered_events++;
    if (recovered) *recovered = (int)ids.size();
    return JSDR_OK;
}

int jsdr_bpsk_receive_i16(jsdr_bpsk *h, const int16_t *raw_host, int ic, int qc)
{
    JSDR_REQUIRE(h && raw_host, "jsdr_bpsk_receive_i16: null argument");
    JSDR_REQUIRE(h->pst_nch == 0, "jsdr_bpsk_receive_i16: a tuned channel handle (jsdr_bpsk_create_tuned_channels) takes batches only "
                 "(jsdr_bpsk_batch_i16); the handle is unchanged");
    JSDR_REQUIRE(!h->pst, "jsdr_bpsk_receive_i16: a tuned handle (jsdr_bpsk_create_tuned) takes batches only; receive() is the 1-stream "
                 "form of jsdr_bpsk_create");
    JSDR_REQUIRE(h->nstreams == 1 || (h->nch > 0 && h->nin == 1),
                 "jsdr_bpsk_receive_i16: handle has %d streams; receive() is the 1-stream form (or a 1-input channel handle)",
                 h->nstreams);
    h->pin_call = true;
    h->pin_off = 0;
    int rc = JSDR_OK;
    const size_t fb = sizeof(int16_t) * 2 * (size_t)h->nsf;
    if (h->pin.p && fb <= h->pin_bytes) {  // the frame waits at the arena's head: bpsk_run sends it (with the tables, if new)
        memcpy(h->pin.p, raw_host, fb);
        h->pin_off = fb;
        h->rx_frame_bytes = fb;
    } else {
        rc = h2d_call(h, h->stage_raw.p, raw_host, fb, 0);
    }
    if (rc == JSDR_OK)
        rc = bpsk_run(h, reinterpret_cast<const int16_t *>(h->stage_raw.p), nullptr, 2LL * h->nsf, h->nsf, ic, qc, 0);
    h->rx_frame_bytes = 0;
    if (rc == JSDR_OK) rc = h->nstreams == 1 ? publish_snapshot(h) : sync_last(h);  // synchronises: the arena is free again
    if (rc != JSDR_OK) (void)hipDeviceSynchronize();  // (a failed call, wherever it failed: nothing may still be reading the arena)
    h->pin_call = false;
    return rc;
}

int jsdr_bpsk_receive_f32(jsdr_bpsk *h, const float *iq_host)
{
    JSDR_REQUIRE(h && iq_host, "jsdr_bpsk_receive_f32: null argument");
    JSDR_REQUIRE(h->pst_nch == 0, "jsdr_bpsk_receive_f32: a tuned channel handle (jsdr_bpsk_create_tuned_channels) takes batches only "
                 "(jsdr_bpsk_batch_f32); the handle is unchanged");
    JSDR_REQUIRE(!h->pst, "jsdr_bpsk_receive_f32: a tuned handle (jsdr_bpsk_create_tuned) takes batches only; receive() is the 1-stream "
                 "form of jsdr_bpsk_create");
    if (h->nch > 0) {
        // a channel handle takes what IAudioHandler delivers, (float)s / 32767f values (JavaAudio.java:281-288), through the
        // int16 kernels; any other float frame is refused
        JSDR_REQUIRE(h->nin == 1, "jsdr_bpsk_receive_f32: the channel handle has %d inputs; receive() takes a 1-input handle", h->nin);
        std::vector<int16_t> q(2 * (size_t)h->nsf);
        for (size_t i = 0; i < q.size(); i++) {
            const float f = iq_host[i];
            float v = f * 32767.0f;
            if (!(v == v)) v = 1e9f;  // NaN: refused below
            v = v > 32767.0f ? 32767.0f : (v < -32768.0f ? -32768.0f : v);
            const int sv = (int)__builtin_rintf(v);
            const float back = (float)sv / 32767.0f;
            JSDR_REQUIRE(memcmp(&back, &f, 4) == 0, "jsdr_bpsk_receive_f32: sample %zu (%g) is not a (float)s/32767f value; a channel "
                         "handle takes the frames JavaAudio produces (the int16 kernels) and refuses other floats", i, (double)f);
            q[i] = (int16_t)sv;
        }
        return jsdr_bpsk_receive_i16(h, q.data(), 0, 0);
    }
    JSDR_REQUIRE(h->nstreams == 1, "jsdr_bpsk_receive_f32: handle has %d streams; receive() is the 1-stream form",
                 h->nstreams);
    h->pin_call = true;
    h->pin_off = 0;
    // What IAudioHandler delivers are (float)s / 32767f values of DC-corrected shorts (JavaAudio.java:281-288).  When every
    // sample of the frame IS such a value -- checked here, on the host, with the same float division -- the frame goes
    // through the int16 kernels (k_fm: two launches instead of four, half the bytes up): same doubles, the two input
    // forms are bit-identical by construction (test_bpsk_one_stream_fed_through_both_input_forms_alternately).  Any other
    // float takes the float kernels as before.
    const size_t nfl = 2 * (size_t)h->nsf;
    static const bool route = [] {
        const char *e = knob("JSDR_F32_AS_I16");  // JSDR_F32_AS_I16=0: float frames always take the float kernels (tests)
        return !e || atoi(e) != 0;
    }();
    bool as_i16 = route && h->variant == 0 && h->pin.p && (h->n_in == 0 || !h->hist_is_float) && nfl * sizeof(int16_t) <= h->pin_bytes;
    if (as_i16) {
        int16_t *q = reinterpret_cast<int16_t *>(h->pin.p);  // the arena's head: the frame's slot
        unsigned bad = 0;
        for (size_t i = 0; i < nfl; i++) {
            const float f = iq_host[i];
            float v = f * 32767.0f;
            if (!(v == v)) {  // NaN: not the conversion of any short (and the casts below are undefined for it)
                bad = 1;
                v = 0.0f;
            }
            v = v > 32767.0f ? 32767.0f : (v < -32768.0f ? -32768.0f : v);
            const int sv = (int)__builtin_rintf(v);
            const float back = (float)sv / 32767.0f;
            unsigned bf, bb;  // compared as bit patterns: -0.0f is NOT the conversion of any short, and stays a float
            memcpy(&bf, &f, 4);
            memcpy(&bb, &back, 4);
            bad |= bf ^ bb;
            q[i] = (int16_t)sv;
        }
        as_i16 = bad == 0;
    }
    int rc;
    if (as_i16) {
        h->pin_off = nfl * sizeof(int16_t);
        h->rx_frame_bytes = nfl * sizeof(int16_t);  // sent by bpsk_run
        rc = bpsk_run(h, reinterpret_cast<const int16_t *>(h->stage_raw.p), nullptr, 2LL * h->nsf, h->nsf, 0, 0, 0);
        h->rx_frame_bytes = 0;
    } else {
        rc = h2d_call(h, h->stage_raw.p, iq_host, sizeof(float) * 2 * (size_t)h->nsf, 0);
        if (rc == JSDR_OK) rc = bpsk_run(h, nullptr, reinterpret_cast<const float *>(h->stage_raw.p), 2LL * h->nsf, h->nsf, 0, 0, 0);
    }
    if (rc == JSDR_OK) rc = publish_snapshot(h);
    if (rc != JSDR_OK) (void)hipDeviceSynchronize();
    h->pin_call = false;
    return rc;
}
