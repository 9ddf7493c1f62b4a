// bpsk_handle.hip -- the jsdr_bpsk handle: the stages of a call and the C ABI (include/jsdr_hip.h).
//
// Host code only: no kernel is defined or launched here.  The tune-mode kernels are in bpsk_front.hip, bpsk_front_reg.hip,
// bpsk_fm.hip and bpsk_tail.hip and are started through the launch_* functions of bpsk_kernels.h; the other kernel families
// come in through bpsk_fft.h, bpsk_chan.h and bpsk_fec.h.  The handle fills their argument structs and calls the launchers,
// each stage of a call in ONE function that every kind of handle (ordinary, channel, FFT-acquire channel) calls.
//
// The input-independent schedule of a call (tuPhase, vcoPhase, dsCnt stepped in host doubles; the period search; the keys that
// say which call a schedule serves) is bpsk_sched.hip's.  The handle holds schedules, decides when one is computed -- on the
// calling thread, or a call ahead on a worker -- and keeps their device copies.
//
// Compiled with -ffp-contract=off like the kernels and the scheduler: tuPhaseInc (bpsk_tuner.h) and the sin / cos tables are
// computed here in host doubles, and every product and sum must round separately, as Java's do.
#include "bpsk_kernels.h"
#include "bpsk_fec.h"
#include "bpsk_fft.h"
#include "bpsk_chan.h"
#include "bpsk_pst.h"
#include "bpsk_sched.h"
#include "bpsk_blob.h"
#include "bpsk_state.h"
#include <math.h>
#include <cmath>
#include <atomic>
#include <memory>
#include <thread>
#include <stddef.h>
#include <stdlib.h>
#include <vector>

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

using namespace jsdr;

// =============================================================================================== host
static_assert((int)SCHED_TABLE_SLACK == (int)FM_TABLE_SLACK, "the scheduler's periodic table carries what k_fm reads past one period");

// one channel of a channel handle (jsdr_bpsk_create_channels): its tuner (FUNcubeBPSKDemod.java:381-390, :196) and the
// cache of its last schedule.  The table is of 9-bit indices (256: the sample passed through unmixed, :395).
struct BpskChan {
    double tuning = 0.0, tuPhase = 0.0, tuPhaseInc = 0.0;
    int do_up = 0;
    int do_fft = 0;                  // jsdr_bpsk_create_mode_channels: the channel runs FFT-acquire (fixed at creation; a live
                                     // channel handle's "FFT/Tune" action changes it)
    int seam = 0;                    // live channel handle: the channel's first call after a switch is still to come (SEAM_*)
    int cb_band = -1;                // ... the band (doUp) its FFT state's centreBin was last settled in, -1: no FFT-acquire frame yet
    std::vector<unsigned short> k9x; // ... its FFT -> tune call's table for k_front_split: [26 + L], the history passed through
    unsigned short khist[26] = {0};  // indices of the 26 samples before the next call
    ChanSchedule sched;              // the schedule last computed for this channel, keyed by the state it started from
    DevBuf<unsigned short> dev;      // the device copy of sched.tab
};

// the last entry a pending tuning plan has for a stream: what the stream's tuning is after the call (a ramp: at its last sample)
struct PstPlanLast {
    int stream;
    long long entry, at;  // its number in the plan, its at_sample
    double tuning, slope;
};

struct SideJob;
struct jsdr_bpsk {
    double tuning = 0.0;  // FUNcubeBPSKDemod.tuning (a double: freqDialog may give what +-10 never reaches)
    int rate = 0, nsf = 0, do_fft = 0, do_up = 0, nstreams = 0, decim = 0;
    long long max_batch = 0, max_ds = 0;
    int max_bits = 0;
    int trig_cap = MIN_TRIG;  // FECDecode calls (sync hits) one stream can log per call; sized from max_bits at create
    // input-independent scheduler state, exact doubles (FUNcubeBPSKDemod.java:381,:494,:501,:468)
    double tuPhase = 0.0, tuPhaseInc = 0.0, vcoPhase = 0.0;
    int dsCnt = 0;
    long long n_in = 0, n_ds = 0;  // samples consumed / demodulated since creation (cntRaw, cntDS)
    // the schedule of the current call (a one-entry cache: a call from the same state takes it as it is) and the next call's,
    // stepped on `worker` while the GPU runs the current one
    Schedule cur, prefetch;
    bool tables_on_device = false;     // the device copy of cur's tables (kvco, tcs; vco_cs) is the current one
    unsigned char h_khist[26] = {0};   // tuner indices of the 26 samples before the next call
    bool retuned = false;              // a live-control call has run (the fast variant's replay from creation would not see it)
    // live mode switches (jsdr_bpsk_set_mode): the FFT-acquire buffers exist (at create, or from the first switch on), the
    // first call after a switch still to come, and the second run's scratch of a tune -> FFT switch
    bool fft_ready = false;
    int seam = 0;
    DevBuf<FftFrontState> fft_state2;
    DevBuf<double2> dm2;
    long long dm2_stride = 0;
    unsigned char h_mhist[26] = {0};   // 1: the 26 samples before the next call were mixed, 0: passed through
    DevBuf<unsigned short> ktu9;       // k_front_split: [26 + L] 9-bit tuner index (256: pass-through)
    DevBuf<double> sincos9;            // cos[0..256], sin[0..256] with (1.0, 1.0) at 256
    std::vector<unsigned short> h_ktu9;
    int c_kshift = -1;
    // device
    DevBuf<double> sincos;
    DevBuf<unsigned char> ktu;
    DevBuf<unsigned char> kvco;
    DevBuf<int2> hist_in[2];
    int hist_cur = 0;
    bool hist_is_float = false;    // form of the samples in hist_in[hist_cur] (the input form of the call that wrote them)
    DevBuf<int> hist_bad;          // k_hist_convert's "not an int16 sample" flag
    DevBuf<int> amax;              // fast variant: [S] running maximum of |int16 sample| (float bits)
    DevBuf<SnapPack> snap_dev;     // receive(): the packed results of the call, fetched in one copy (k_snapshot_pack)
    DevBuf<unsigned> fm_tickets;   // [1] k_fm / k_fm_f32 held to a CU share: the launch's tile counter (zeroed on the stream by the launcher)
    DevBuf<int> fm_edges;          // k_fm: [S][4 * FM_EDGE] the stream around sample 0 and around the last sample (k_fm_edges)
    DevBuf<float2> fm_edges_f32;   // k_fm_f32: the same images as float pairs (k_fm_prep_f32); allocated by the first jsdr_bpsk_batch_f32
    bool f32_batch = false;        // the call in progress is a jsdr_bpsk_batch_f32: float input may take the fused kernel (receive_f32's
                                   // frames keep the three-kernel path)
    DevBuf<double2> dm, y[2];  // y is double-buffered: the tail of call k overlaps the front end of call k+1
    int y_cur = 0;
    // fused front end + matched filter (k_fm): the 64-sample halo lives in its own double buffer, the tuner table is
    // an unwrapped periodic (cos, sin) table
    DevBuf<double2> dmh[2], tcs;
    int dmh_cur = 0;
    int tab_cur = 0;               // which half of kvco / tcs holds the current schedule's tables
    bool halo_in_dmh = false;      // where the last call left the 64 VCO-mixed history samples (dm[s][0..63] or dmh)
    bool use_fm = true;            // JSDR_FM=0: always the three-kernel path
    long long last_fm_items = 0, last_fm_grid = 0;  // jsdr_bpsk_last_launch
    int last_fm_phase = -1;                         // jsdr_bpsk_fm_form: the last call's k_fm form (-1: generic, or another kernel)
    int share_wgs_per_cu = 0;      // jsdr_bpsk_set_cu_share: workgroups per CU k_fm is held to (0: one per tile, all the chip takes)
    int num_cu = 0;                // CUs of the device (device_cus: asked at the first use, 0 until then)
    int variant = 0;               // 0 exact-order FP64, 1 fast (FMA-contracted FP64, margin-certified decisions)
    double fast_ey = 0.0;          // bound on the error of (fi,fq) in the fast variant (set at create from the taps)
    double margin_scale = 1.0;     // JSDR_FAST_MARGIN_SCALE: widens the detector margins (tests force the exact redo path with it)
    double argmax_scale = 1.0;     // JSDR_FAST_ARGMAX_SCALE: widens the argmax margin (tests provoke an uncertifiable stream)
    const char *front_name = "k_front";  // the front-end kernel the last call launched
    const char *tail_name = "k_tail";    // ... the tail kernel (k_tail / k_tail8) ...
    const char *fec_name = "k_fec_bpsk"; // ... and the FEC form (one wave per block, or the batch form's kernels)
    bool ktu_uploaded = false;     // the device copy of the per-sample tuner index table matches cur's
    std::thread worker;
    bool prefetch_on = true;       // JSDR_SCHED_PREFETCH=0: always on the calling thread
    long long sched_sync = 0, sched_prefetched = 0;  // schedules computed on the calling thread / taken from the worker
    Stream tail_stream;                  // non-blocking side stream for the latency-bound 9600 Hz tail + FEC
    Event ev_matched;                    // caller stream -> tail stream: (fi,fq) of this call are complete
    Event ev_tail_done[2];               // tail stream -> caller stream: y[i] may be overwritten
    bool tail_pending[2] = {false, false};
    // results of the last receive_*() of a 1-stream handle, double-buffered for a reader on another thread (the Swing
    // EDT paints while the audio thread receives): the writer fills the idle copy, then publishes it
    jsdr_bpsk_snapshot snap[2];
    std::atomic<unsigned> snap_seq[2];   // odd while that copy is being written
    std::atomic<int> snap_cur{-1};       // -1: nothing received yet
    long long snap_count = 0;
    Event ev_pack_done;                  // pack stream -> tail stream: the result arrays of the previous call have been read
    bool pack_pending = false;
    bool overlap = true;
    long long dm_stride = 0, y_stride = 0;
    DevBuf<TailState> tail;
    DevBuf<signed char> bitlog[2];
    int bitlog_cur = 0;
    long long bitlog_stride = 0;
    DevBuf<int> nbits, trig_count, trig_bits, fec_rc, fec_last, cnt_dec;
    DevBuf<signed char> corr;
    DevBuf<unsigned char> fec_data, decoded;
    DevBuf<unsigned long long> fec_scratch;  // Viterbi decision words of every (stream, hit) block
    DevBuf<unsigned char> fec_vit;           // batch form (k_vitq): the Viterbi output bytes of every (stream, hit) block
    DevBuf<int> fec_work;                    // ... its work list, [0] = count
    DevBuf<int> fec_done;                    // [S] k_fec_bpsk's per-stream count of finished blocks (zero between launches)
    // receive_*() of a 1-stream handle: every host<->device copy of the call goes through ONE pinned arena (the frame in,
    // the schedule's tables when they change, the packed results out).  A copy from / to pageable memory is staged by the
    // runtime and costs a multiple of the transfer; the arena is reused every call, which is safe because receive()
    // synchronises before it returns.  Batch calls (asynchronous, caller-owned streams) keep the pageable path.
    PinnedStage pin;               // (the SnapPack slot sits behind pin_bytes)
    size_t pin_bytes = 0, pin_off = 0;
    bool pin_call = false;
    bool vco_cs_in_blob = false;  // FFT-acquire mode: the current schedule's VCO factors sit behind the frame in stage_raw
    size_t vco_cs_blob_off = 0;
    size_t rx_frame_bytes = 0;  // receive(): the frame sits at the arena's head and has not been sent yet (bpsk_run sends it,
                                // with the schedule's tables behind it in the SAME copy when they changed)
    bool snap_fused = false;  // the last call's k_fec_bpsk packed the snapshot itself (receive() of a 1-stream handle)
    DevBuf<int> stage_raw;  // one frame for receive_*()
    DevBuf<FftFrontState> fft_state;  // FFT-acquire mode only
    DevBuf<double2> fft_tw;
    DevBuf<double> ds_taps_dev;
    DevBuf<double2> vco_cs;       // FFT-acquire mode: (cos, sin) of the VCO table entry of every decimated sample of the call
    std::vector<double> h_sincos;
    std::vector<double2> h_vco_cs;
    DevBuf<long long> phase_clk;  // JSDR_FFT_PHASECLK=1: k_front_fft's per-phase cycle counts, printed at destroy
    int logn = 0;
    bool fft_mixed = false;  // FFT-acquire frame is not a power of two (bpsk_fftm.hip)
    bool fft_2x = false;     // ... and is 2 m with m an LDS-sized frame (n = 19200): two m-point halves per transform
    AcqgPlan gen_plan;       // gen_plan.on: none of the LDS front ends takes the frame (or its decimation): bpsk_acqg.hip, always in three phases
    int fm_np = 0, fm_rad[12] = {0}, fm_off[12] = {0}, fm_off1[12] = {0};
    DevBuf<double2> fft2x_ek;  // per-stream scratch of the 2 m front end
    DevBuf<double> fft2x_r0;
    // round 6: the three-phase front end (bpsk_acq.hip) for calls of two or more frames per stream -- what its phases hand each
    // other, for nstreams x acq_chunk frames; allocated at the first such call
    DevBuf<unsigned char> acq_scratch;
    int acq_chunk = 0;
    // round 6, fast variant: the streams jsdr_bpsk_recover_uncertified() has replayed live on in an EXACT shadow handle (lock-step
    // with this one from then on); their getters and their packed slots come from it
    struct Destroy {
        void operator()(jsdr_bpsk *h) const { (void)jsdr_bpsk_destroy(h); }
    };
    std::unique_ptr<jsdr_bpsk, Destroy> shadow;
    std::vector<int> shadow_ids;   // ascending stream ids, index = the shadow's stream
    std::vector<int> shadow_map;   // [nstreams] index into the shadow, or -1
    DevBuf<int16_t> shadow_in;     // [U][2 max_batch] the shadow's rows of a call's input
    DevBuf<unsigned char> shadow_slots;
    long long batch_calls = 0;     // jsdr_bpsk_batch_i16 calls since creation (a recovery must be given all of them)
    long long recovered_events = 0;
    int acq_mode = -1;  // JSDR_ACQ3 (tests, A/B): 0 never, 1 whenever the frame size allows (also for one frame a call); -1: from two frames a call
    long long last_nds = 0;
    int last_y = 0;
    hipStream_t last_stream = 0;
    // optional per-kernel HIP-event timing (bench.py's roofline leg)
    bool prof_on = false;
    struct ProfRec {
        int kernel;
        Event a, b;
    };
    std::vector<ProfRec> prof_recs;
    std::vector<Event> prof_pool;
    // channel handle (jsdr_bpsk_create_channels): nch > 0 channels per input, stream = input * nch + channel
    int nch = 0, nin = 0;
    std::vector<BpskChan> chan;
    VcoSchedule vco;                 // the VCO schedule of the last call, shared by every channel and input
    // jsdr_bpsk_create_mode_channels: every channel in the tune mode or in FFT-acquire, fixed at creation.  nfftch of them run
    // FFT-acquire (bpsk_acq_chan.hip); fft_state is then CHANNEL-major, [nch][nin]
    bool mode_chan = false;
    int nfftch = 0;
    long long acq_fwd_frames = 0, acq_inv_frames = 0;  // jsdr_bpsk_acq_last_launch
    // jsdr_bpsk_create_live_channels: a channel's mode changes live.  fft_state has every channel's rows from creation on, seam_q
    // the Q columns of the tune -> FFT seam ([nch][nin][26], beside fft_state's I columns); acq_mask: the bands acq_scratch is cut for
    bool live_chan = false;
    DevBuf<double> seam_q;
    int acq_mask = 0;
    // tuned handle (jsdr_bpsk_create_tuned): every stream its own tuner, walked on the device once a call (bpsk_pst.hip).  The
    // handle's own tuPhase / tuPhaseInc stay 0: build_schedule's shared parts (decimation counter, VCO schedule) are all the
    // call takes from it
    bool pst = false;
    std::vector<double> pst_tuning;    // [S] each stream's tuning (the device holds its tuPhaseInc)
    DevBuf<double> pst_tu, pst_inc;    // [S] tuPhase, tuPhaseInc
    DevBuf<double> pst_ckpt;           // [S][pst_ckpt_stride] k_tuner_walk's checkpoints of the call
    long long pst_ckpt_stride = 0;
    DevBuf<unsigned short> pst_kh[2];  // [S][32] the 9-bit indices of the 26 samples before the next call, double-buffered like hist_in
    int pst_kh_cur = 0;
    DevBuf<int> pst_ids;               // [S] the streams an action zeroes dmMaxCorr in (k_reset_maxcorr_list)
    // tuned channel handle (jsdr_bpsk_create_tuned_channels): a tuned handle of pst_nin x pst_nch streams whose pst_nch channels of
    // an input read ONE input row (k_chan_front_pst, bpsk_chan_pst.hip) -- the input, its stride and its 26-sample history are per
    // input, everything else per stream as above.  0: a tuned handle of jsdr_bpsk_create_tuned (nch stays 0 on both)
    int pst_nin = 0, pst_nch = 0;
    // a tuning plan (jsdr_bpsk_plan_stream_tunings, jsdr_bpsk_plan_stream_ramps): retunes inside the next call, copied to the device
    // when it is given.  The call that takes it clears pst_plan_n; the device copy stays until the next plan replaces it, a plan of 0
    // entries or destroy.
    long long pst_plan_n = 0;                            // entries pending
    long long pst_plan_max_at = -1;                      // the largest at_sample among them
    std::vector<PstPlanLast> pst_plan_last;              // every planned stream's last entry: pst_tuning after the call
    bool pst_plan_ramp = false;                          // given by jsdr_bpsk_plan_stream_ramps with a slope that is not zero
    DevBuf<long long> pst_plan_off, pst_plan_pos;        // [S + 1], [n]  (PstPlanArgs)
    DevBuf<double> pst_plan_inc;                         // [n], a step plan's
    DevBuf<double> pst_plan_tun, pst_plan_slope;         // [n], [n], a ramp plan's  (PstRampArgs)
    DevBuf<double> pst_inc0;                             // [S], with the first plan
    DevBuf<int> pst_ckpt_e;                              // [S][pst_ckpt_stride], with the first plan
    // checkpoints (jsdr_bpsk_save / jsdr_bpsk_restore): the records' staging image, allocated at the first use
    DevBuf<unsigned char> state_img;
    bool restored = false;                   // a blob has been restored: the handle is no longer free to adopt a shared block
    std::vector<unsigned char> trace_void;   // [S] 1: restored since the last call -- the stream's last call is an empty one
    Event ev_state[2];                       // around the last k_state_pack / k_state_unpack launch (created at the first use)
    float state_pack_ms = -1.f, state_unpack_ms = -1.f;  // jsdr_bpsk_state_kernel_ms; -1: none yet
};

// whether a stream runs FFT-acquire (state doubles 6 / 7 and counter centreBin are live), and where its FftFrontState sits
static bool stream_fft(const jsdr_bpsk *h, int stream)
{
    return h->nch > 0 ? (h->nfftch > 0 && h->chan[stream % h->nch].do_fft != 0) : h->do_fft != 0;
}
static size_t fft_state_at(const jsdr_bpsk *h, int stream)
{
    return h->nch > 0 ? (size_t)(stream % h->nch) * (size_t)h->nin + (size_t)(stream / h->nch) : (size_t)stream;
}

// the input rows of a tuned handle's call: its streams, or the inputs of a tuned channel handle
static int pst_rows_in(const jsdr_bpsk *h)
{
    return h->pst_nch > 0 ? h->pst_nin : h->nstreams;
}

static void pst_plan_clear(jsdr_bpsk *h)  // no plan pends (the device copy stays until a plan replaces it)
{
    h->pst_plan_n = 0;
    h->pst_plan_max_at = -1;
    h->pst_plan_ramp = false;
    h->pst_plan_last.clear();
}

enum { PK_FRONT = 0, PK_HIST, PK_MATCHED, PK_DMHIST, PK_TAIL, PK_SYNC, PK_SYNCFIN, PK_FEC, PK_FM, PK_SYNCT, PK_PREP,
       PK_ACQ_FWD, PK_ACQ_SCAN, PK_ACQ_INV, PK_ACQ_EDGES, PK_ACQC_FWD, PK_TWALK, PK_COUNT };
static const char *const kProfNames[PK_COUNT] = {"k_front", "k_hist_in", "k_matched", "k_dm_history", "k_tail", "k_sync",
                                                 "k_sync_fin", "k_fec_bpsk", "k_fm", "k_sync_t", "k_fm_prep",
                                                 "k_acq_fwd", "k_acq_scan", "k_acq_inv", "k_acq_edges", "k_acqc_fwd", "k_tuner_walk"};

static Event prof_event(jsdr_bpsk *h)
{
    Event e;
    if (h->prof_pool.empty()) {
        (void)e.create();  // (none: the scope records nothing)
    } else {
        e = std::move(h->prof_pool.back());
        h->prof_pool.pop_back();
    }
    return e;
}
struct ProfScope {
    jsdr_bpsk *h;
    hipStream_t st;
    Event a, b;
    int k;
    ProfScope(jsdr_bpsk *h_, int k_, hipStream_t st_) : h(h_), st(st_), k(k_)
    {
        if (h->prof_on) {
            a = prof_event(h);
            b = prof_event(h);
            (void)hipEventRecord(a, st);
        }
    }
    ~ProfScope()
    {
        if (h->prof_on && a && b) {
            (void)hipEventRecord(b, st);
            h->prof_recs.push_back({k, std::move(a), std::move(b)});
        }
    }
};

// the three-phase front end's launches (bpsk_acq.hip) under the same timing scopes
struct AcqProfCtx {
    jsdr_bpsk *h;
    Event a[5];  // (phase 4: the channel handle's both-band forward kernel)
};
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

enum { SEAM_NONE = 0, SEAM_TO_FFT = 1, SEAM_TO_TUNE = 2 };

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
static long long build_schedule(jsdr_bpsk *h, long long L)
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

static int sync_last(jsdr_bpsk *h);
static int publish_snapshot(jsdr_bpsk *h);

// host -> device copy of a call's input or tables: through the pinned arena inside receive_*(), pageable otherwise
static int h2d_call(jsdr_bpsk *h, void *dst_dev, const void *src_host, size_t bytes, hipStream_t st)
{
    if (h->pin_call && h->pin.p) {
        const size_t off = (h->pin_off + 63) & ~(size_t)63;
        if (off + bytes <= h->pin_bytes) {
            memcpy(h->pin.p + off, src_host, bytes);
            h->pin_off = off + bytes;
            JSDR_HIP_TRY(hipMemcpyAsync(dst_dev, h->pin.p + off, bytes, hipMemcpyHostToDevice, st));
            return JSDR_OK;
        }
    }
    JSDR_HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, st));
    return JSDR_OK;
}

// The side section of a call: the 9600 Hz tail, the sync correlation and the FEC of every hit, on the handle's side stream
// (the caller's when there is none), after the front end of THAT call.  Everything it needs from the call is in the job.
struct SideJob {
    bool valid = false;
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
// One function per stage; chan_run and bpsk_run call them in the order their work goes onto the caller's stream.

// CUs of the device, asked once per handle (256 where the runtime does not say); 0: the query failed
static int device_cus(jsdr_bpsk *h)
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
static int acq_scratch_ensure(jsdr_bpsk *h, size_t per_row_frame, size_t rows, size_t slack)
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
static FftFrontArgs fft_front_args(jsdr_bpsk *h, const int *raw, const float2 *rawf, long long stride_pairs, long long L, int ic, int qc,
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

// what launch_acq3 / launch_acq3_chan take beside the arguments: the handle's mixed-radix plan and the per-phase timing hook
struct AcqLaunchCtx {
    AcqmPlan plan;
    AcqProfCtx pc;
    AcqProf prof;
};
static void acq_launch_ctx(jsdr_bpsk *h, AcqLaunchCtx &c)
{
    c.plan.np = h->fm_np;
    c.plan.rad = h->fm_rad;
    c.plan.tw_off = h->fm_off;
    c.plan.wr_off = h->fm_off1;
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
static int send_vco_cs(jsdr_bpsk *h, long long nds, hipStream_t st)
{
    h->h_vco_cs.resize((size_t)nds);
    fill_vco_cs(h, h->h_vco_cs.data(), nds);
    return h2d_call(h, h->vco_cs.p, h->h_vco_cs.data(), sizeof(double2) * (size_t)nds, st);
}

// k_front_split's and k_chan_front's table: cos[0..256], sin[0..256] with (1.0, 1.0) at 256 (the pass-through entry, :395)
static int sincos9_ensure(jsdr_bpsk *h)
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

// the tail that last read y[yb] (two calls ago) must be done before the matched filter (or k_fm) overwrites it
static int wait_tail(jsdr_bpsk *h, int yb, hipStream_t st)
{
    if (h->overlap && h->tail_pending[yb]) {
        JSDR_HIP_TRY(hipStreamWaitEvent(st, h->ev_tail_done[yb], 0));
        h->tail_pending[yb] = false;
    }
    return JSDR_OK;
}

// the next call's 26-sample input history of `rows` rows (streams, or inputs of a channel handle): k_hist_in's work
static HistArgs hist_args(const jsdr_bpsk *h, const int *raw, const float2 *rawf, long long stride_pairs, long long L, int ic, int qc,
                          int rows)
{
    HistArgs ha;
    ha.raw = raw;
    ha.rawf = rawf;
    ha.stride_pairs = stride_pairs;
    ha.nsamples = L;
    ha.ic = ic;
    ha.qc = qc;
    ha.hist_old = h->hist_in[h->hist_cur].p;
    ha.hist_new = h->hist_in[h->hist_cur ^ 1].p;
    ha.nstreams = rows;
    return ha;
}

static int run_hist_in(jsdr_bpsk *h, const HistArgs &ha, hipStream_t st)
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
static int hist_form(jsdr_bpsk *h, bool want_float, int rows, hipStream_t st)
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
static int run_matched(jsdr_bpsk *h, int yb, long long nds, long long g_first, hipStream_t st)
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
static int finish_call(jsdr_bpsk *h, int yb, long long L, long long nds, long long g_first, int first_out, int ic, int qc,
                       const int *raw, long long stride_pairs, unsigned char *kvco_p, double2 *tcs_p, hipStream_t st)
{
    SideJob job;
    job.valid = true;
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
enum FftFront { FRONT_POW2, FRONT_FFTM, FRONT_FFT2X, FRONT_GEN, FRONT_NONE };
static FftFront fft_front_kind(int n, int decim, bool chan_form, int force_gen);

static bool chan_cb_foreign(const jsdr_bpsk *h, int c)
{
    return h->live_chan && h->chan[c].cb_band >= 0 && h->chan[c].cb_band != (h->chan[c].do_up ? 1 : 0);
}

static bool chan_fused_ok(const jsdr_bpsk *h)
{
    return !h->gen_plan.on && fft_front_kind(h->nsf, h->decim, false, -1) == fft_front_kind(h->nsf, h->decim, true, -1);
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
    auto front = [&](const FftFrontArgs &x) {
        return h->fft_2x ? launch_front_fft2x(x, h->fm_np, h->fm_rad, h->fm_off, h->fm_off1, h->fft2x_ek.p, h->fft2x_r0.p, S, st)
                         : (h->fft_mixed ? launch_front_fftm(x, h->fm_np, h->fm_rad, h->fm_off, h->fm_off1, h->fft2x_ek.p, S, st)
                                         : launch_front_fft(x, S, st));
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
        const char *name = h->fft_2x ? "k_front_fft2x" : (h->fft_mixed ? (fftm_pairs(x1.n, x1.nframes) ? "k_front_fftm2" : "k_front_fftm") : "k_front_fft");
        if (names_call) h->front_name = name;  // (no three-phase launch ran in the call)
        if (front(x1) != JSDR_OK) return JSDR_ERR;
        if (seam) {
            const int D = h->decim, fo = (int)x1.first_out;
            const long long nds1 = fo < n ? (long long)((n - 1 - fo) / D + 1) : 0;  // outputs of frame 0
            long long J = fo <= 25 ? (long long)((25 - fo) / D + 1) : 0;          // outputs whose windows reach back
            if (J > nds1) J = nds1;
            if (J > x1.nds) J = x1.nds;
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
static int chan_run(jsdr_bpsk *h, const int16_t *raw_dev, const float *rawf_dev, long long stride_i16, long long L, int ic,
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
        if (acq_scratch_ensure(h, acq3c_frame_bytes(h->nsf, mask, h->gen_plan.on), (size_t)h->nin, 4096) != JSDR_OK) return JSDR_ERR;
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
                const int D = h->decim;
                const long long nds1 = first_out < h->nsf ? (long long)((h->nsf - 1 - first_out) / D + 1) : 0;  // outputs of frame 0
                long long J = first_out <= 25 ? (long long)((25 - first_out) / D + 1) : 0;  // outputs whose windows reach back
                if (J > nds1) J = nds1;
                if (J > nds) J = nds;
                ca.seam_q[ca.nfft] = qcol;
                ca.seam_J = (int)J;
            }
            ca.nfft++;
        }
        ca.st = h->fft_state.p;
        FftFrontArgs xa = fft_front_args(h, raw, rawf, stride_pairs, L, ic, qc, first_out, nds);
        xa.do_up = 0;  // (each channel's band is in ca.up)
        AcqLaunchCtx lc;
        acq_launch_ctx(h, lc);
        if (ca.nfft > 0 &&
            launch_acq3_chan(xa, ca, h->acq_scratch.p, h->acq_scratch.n, h->acq_chunk, device_cus(h), st, lc.prof, lc.plan, &h->gen_plan) != JSDR_OK)
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

// ------------------------------------------------------------------------------------------- tuned handles
// A call of a tuned handle (jsdr_bpsk_create_tuned): every stream's tuner walked on the device (k_tuner_walk), the front end fed
// from the walk's checkpoints (k_front_pst), then the three-kernel path's k_hist_in, k_matched, k_dm_history and the side
// section, as bpsk_run launches them.  build_schedule provides the parts every stream shares -- the decimation counter, the VCO
// schedule, the outputs of the call; the handle's own tuner stands at 0 and its tables are not sent.
static int pst_run(jsdr_bpsk *h, const int16_t *raw_dev, const float *rawf_dev, long long stride_i16, long long L, int ic, int qc,
                   hipStream_t st)
{
    JSDR_REQUIRE(raw_dev || rawf_dev, "bpsk: null input");
    JSDR_REQUIRE(L > 0 && L <= h->max_batch, "bpsk: nsamples=%lld outside (0, max_batch_samples=%lld]", L, h->max_batch);
    const int rows_in = pst_rows_in(h);  // (a tuned channel handle: the stride is between inputs)
    JSDR_REQUIRE((stride_i16 & 1) == 0 && (rows_in == 1 || stride_i16 >= 2 * L),
                 "bpsk: %s stride %lld too small for %lld samples", h->pst_nch > 0 ? "input" : "stream", stride_i16, L);
    // the previous call may have come through the other input form (before anything moves on: the conversion can refuse)
    const bool planned = h->pst_plan_n > 0;
    JSDR_REQUIRE(!planned || L > h->pst_plan_max_at, "bpsk: the pending tuning plan has an entry at sample %lld, the call has %lld samples; the "
                 "handle is unchanged and the plan stays pending", h->pst_plan_max_at, L);
    const bool ramp = planned && h->pst_plan_ramp;
    if (ramp)  // a ramp that runs to the call's end: its last sample's tuning (the other end was checked with the plan)
        for (const PstPlanLast &pl : h->pst_plan_last) {
            const double t_end = tuner_ramp_tuning(pl.tuning, pl.slope, L - 1 - pl.at);
            JSDR_REQUIRE(std::isfinite(t_end) && t_end < (double)h->rate, "bpsk: entry %lld of the pending ramp plan (stream %d, from sample %lld) "
                         "reaches %g Hz at the call's last sample (%lld), not a finite value below the rate (%d Hz); the handle is unchanged and "
                         "the plan stays pending", pl.entry, pl.stream, pl.at, t_end, L - 1, h->rate);
        }
    if (hist_form(h, rawf_dev != nullptr, rows_in, st) != JSDR_OK) return JSDR_ERR;
    const int S = h->nstreams;
    const int first_out = h->decim - 1 - h->dsCnt;
    const long long g_first = h->n_ds;
    const long long nds = build_schedule(h, L);
    JSDR_REQUIRE(nds <= h->max_ds, "bpsk: internal: %lld decimated samples exceed capacity %lld", nds, h->max_ds);
    if (!h->tables_on_device) {
        h->tab_cur ^= 1;  // (double-buffered as bpsk_run's)
        if (nds > 0)
            if (h2d_call(h, h->kvco.p + (size_t)h->tab_cur * (size_t)h->max_ds, h->cur.kvco.data(), (size_t)nds, st) != JSDR_OK) return JSDR_ERR;
        h->tables_on_device = true;
    }
    unsigned char *kvco_p = h->kvco.p + (size_t)h->tab_cur * (size_t)h->max_ds;
    double2 *tcs_p = h->tcs.p + (size_t)h->tab_cur * (256 + FM_TABLE_SLACK);
    const int *raw = reinterpret_cast<const int *>(raw_dev);
    const float2 *rawf = reinterpret_cast<const float2 *>(rawf_dev);
    const long long stride_pairs = stride_i16 / 2;
    // the plan was copied when it was given: the planned forms of the two kernels read it where it lies
    const PstPlanArgs pa = {h->pst_plan_off.p, h->pst_plan_pos.p, h->pst_plan_inc.p, h->pst_inc0.p, h->pst_ckpt_e.p, h->pst_inc.p};
    const PstPlanArgs *plan = planned ? &pa : nullptr;
    const PstRampArgs ra = {h->pst_plan_tun.p, h->pst_plan_slope.p, (double)h->rate};
    const PstRampArgs *rplan = ramp ? &ra : nullptr;
    {
        TunerWalkArgs wa;
        wa.tu = h->pst_tu.p;
        wa.inc = h->pst_inc.p;
        wa.ckpt = h->pst_ckpt.p;
        wa.ckpt_stride = h->pst_ckpt_stride;
        wa.nsamples = L;
        wa.kh_old = h->pst_kh[h->pst_kh_cur].p;
        wa.kh_new = h->pst_kh[h->pst_kh_cur ^ 1].p;
        wa.nstreams = S;
        ProfScope ps(h, PK_TWALK, st);
        if (launch_tuner_walk(wa, plan, rplan, st) != JSDR_OK) return JSDR_ERR;
    }
    if (nds > 0 && h->pst_nch > 0) {  // every input read once, its channels' rows fed from the walk's checkpoints
        PstChanFrontArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.raw = rawf ? reinterpret_cast<const int *>(rawf) : raw;
        fa.stride_pairs = stride_pairs;
        fa.ic = ic;
        fa.qc = qc;
        fa.hist = h->hist_in[h->hist_cur].p;
        fa.inc = h->pst_inc.p;
        fa.ckpt = h->pst_ckpt.p;
        fa.ckpt_stride = h->pst_ckpt_stride;
        fa.kh_old = h->pst_kh[h->pst_kh_cur].p;
        fa.kvco = kvco_p;
        fa.sc9 = h->sincos9.p;
        fa.ds_taps = h->ds_taps_dev.p;
        fa.dm = h->dm.p;
        fa.dm_stride = h->dm_stride;
        fa.nds = nds;
        fa.first_out = first_out;
        fa.decim = h->decim;
        fa.nch = h->pst_nch;
        ProfScope ps(h, PK_FRONT, st);
        h->front_name = ramp ? "k_chan_front_pst_ramp" : planned ? "k_chan_front_pst_plan" : "k_chan_front_pst";
        if (launch_chan_front_pst(fa, h->pst_nin, rawf != nullptr, plan, rplan, st) != JSDR_OK) return JSDR_ERR;
    } else if (nds > 0) {
        PstFrontArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.raw = rawf ? reinterpret_cast<const int *>(rawf) : raw;
        fa.stride_pairs = stride_pairs;
        fa.ic = ic;
        fa.qc = qc;
        fa.hist = h->hist_in[h->hist_cur].p;
        fa.inc = h->pst_inc.p;
        fa.ckpt = h->pst_ckpt.p;
        fa.ckpt_stride = h->pst_ckpt_stride;
        fa.kh_old = h->pst_kh[h->pst_kh_cur].p;
        fa.kvco = kvco_p;
        fa.sc9 = h->sincos9.p;
        fa.ds_taps = h->ds_taps_dev.p;
        fa.dm = h->dm.p;
        fa.dm_stride = h->dm_stride;
        fa.nds = nds;
        fa.first_out = first_out;
        fa.decim = h->decim;
        ProfScope ps(h, PK_FRONT, st);
        h->front_name = ramp ? "k_front_pst_ramp" : planned ? "k_front_pst_plan" : "k_front_pst";
        if (launch_front_pst(fa, S, rawf != nullptr, plan, rplan, st) != JSDR_OK) return JSDR_ERR;
    }
    h->pst_kh_cur ^= 1;
    if (run_hist_in(h, hist_args(h, raw, rawf, stride_pairs, L, ic, qc, rows_in), st) != JSDR_OK) return JSDR_ERR;
    const int yb = h->y_cur;
    if (wait_tail(h, yb, st) != JSDR_OK) return JSDR_ERR;
    if (nds > 0 && run_matched(h, yb, nds, g_first, st) != JSDR_OK) return JSDR_ERR;
    if (finish_call(h, yb, L, nds, g_first, first_out, ic, qc, raw, stride_pairs, kvco_p, tcs_p, st) != JSDR_OK) return JSDR_ERR;
    if (planned) {  // one-shot: the streams it named stand at their last entries, a ramp at the call's last sample (the walk left
                    // their tuPhaseInc on the device: tuner_inc of these)
        for (const PstPlanLast &pl : h->pst_plan_last) h->pst_tuning[(size_t)pl.stream] = tuner_ramp_tuning(pl.tuning, pl.slope, L - 1 - pl.at);
        pst_plan_clear(h);
    }
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
    const int kshift = 0;
    const bool fresh = !h->tables_on_device;
    if (fresh) h->ktu_uploaded = false;
    if (fresh) {
        // The VCO / tuner tables are double-buffered: the fast variant's tail (side stream) may still re-read those of
        // the previous call.  The half written now was last used two schedules ago; the tail that read it is the one
        // that also frees y[y_cur], so waiting for that one (not for the previous call's) keeps the overlap.
        h->tab_cur ^= 1;
        if (h->variant != 0 && wait_tail(h, h->y_cur, st) != JSDR_OK) return JSDR_ERR;
    }
    unsigned char *kvco_p = h->kvco.p + (size_t)h->tab_cur * (size_t)h->max_ds;
    double2 *tcs_p = h->tcs.p + (size_t)h->tab_cur * (256 + FM_TABLE_SLACK);
    // the 1 B/sample index table is only read by the kernels without the periodic table (k_front, k_front_reg<PER = false>)
    const bool reg_will_run = front_reg_enabled() && std_decim && raw_dev && !rawf_dev && L <= 0x3fffffffLL && L >= 64;
    const bool need_ktu = !h->do_fft && !split && !fm_ok && !(per_ok && reg_will_run) && h->cur.mix != 0;
    if (need_ktu && (!h->ktu_uploaded || kshift != h->c_kshift)) {
        h->c_kshift = kshift;
        if (h2d_call(h, h->ktu.p + kshift, h->cur.ktu.data(), (size_t)L + 26, st) != JSDR_OK) return JSDR_ERR;
        h->ktu_uploaded = true;
    }
    ScatterArgs sc;
    memset(&sc, 0, sizeof(sc));
    bool tables_sent = false;
    if (h->rx_frame_bytes) {
        // receive(): the frame is at the arena's head.  When the call takes k_fm and its tables changed, they ride behind
        // the frame in the same copy and k_fm_prep scatters them (three copies were ~10 us each of a 70 us call)
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
    fa.ktu = h->ktu.p + kshift;
    fa.kvco = kvco_p;
    fa.sincos = h->sincos.p;
    fa.hist = h->hist_in[h->hist_cur].p;
    fa.dm = h->dm.p;
    fa.dm_stride = h->dm_stride;
    fa.ds_dbg = nullptr;
    fa.nds = nds;
    fa.first_out = first_out;
    fa.tcs = per_ok ? tcs_p : nullptr;
    fa.tper = h->cur.tper;
    bool hist_done = false;  // the next call's input history has been written (k_fm_prep does it in the k_fm path)
    if (h->do_fft && nds > 0 && h->halo_in_dmh)  // (the last tune call left the matched filter's halo in dmh)
        if (move_halo(h, false, st) != JSDR_OK) return JSDR_ERR;
    if (h->do_fft) {
        FftFrontArgs xa = fft_front_args(h, fa.raw, fa.rawf, fa.stride_pairs, L, ic, qc, first_out, nds);
        // the front end over the frames of xa (a lambda: the first call after a switch from the tune mode runs it twice)
        auto fft_front = [&](FftFrontArgs &xa) -> int {
            // round 6: frames of 2^k samples, two or more per stream in the call: three phases over FRAMES (bpsk_acq.hip); a call of
            // one frame per stream (a live receive()) keeps the fused kernel -- one launch instead of four
            // The 2^k frames' three-phase kernels are the faster ones per frame as well (n = 2048, 1024 x 2^20: 8.65 against 9.1 ms);
            // the default mixed-radix frames' are the fused kernel's passes cut in two and cost 10-14 % more per frame at a full grid
            // (9600: 12.6 against 11.5 ms; the spectrum rows' round trip, a ticket a frame) -- they are taken where frames fill the
            // chip better than streams: ceil(S F / W) * 1.15 < ceil(S / W) * F, W = the workgroups the chip holds (one a CU).
            bool three = !h->fft_2x && acq3_supported(h->nsf) && h->acq_mode != 0 && (xa.nframes >= 2 || h->acq_mode == 1) &&
                         L < 0x7fffffffLL && (long long)S * ((xa.nframes + 1) / 2) < 0x7fffffffLL;  // (its kernels' 32-bit frame arithmetic)
            if (h->gen_plan.on) three = true;  // (no fused kernel exists for these frames)
            if (three && h->fft_mixed && h->acq_mode < 0) {
                if (!device_cus(h)) return JSDR_ERR;
                const long long W = h->num_cu, F = xa.nframes;
                // (4800 / 4410: the fused kernel takes two frames at once and is 1.38 / 1.27 x the three-phase kernels' pace at a full grid)
                const double pace = (h->nsf == 4800 && F >= 2) ? 1.4 : (h->nsf == 4410 && F >= 2) ? 1.3 : 1.15;
                three = (double)(((long long)S * F + W - 1) / W) * pace < (double)((((long long)S + W - 1) / W) * F);
            }
            if (three) {
                const size_t per = acq3_frame_bytes(h->nsf, h->do_up) + 64 + (h->gen_plan.on ? acqg_image_bytes(h->nsf) : 0);
                if (acq_scratch_ensure(h, per, (size_t)S, 512) != JSDR_OK) return JSDR_ERR;  // (per stream and frame)
                h->front_name = h->gen_plan.on ? "k_acqg_pass" : h->fft_mixed ? "k_acqm_fwd" : "k_acq_fwd";
                AcqLaunchCtx lc;
                acq_launch_ctx(h, lc);
                if (launch_acq3(xa, S, h->acq_scratch.p, h->acq_scratch.n, h->acq_chunk, h->num_cu, st, lc.prof, lc.plan, &h->gen_plan) != JSDR_OK) return JSDR_ERR;
            } else {
                ProfScope ps(h, PK_FRONT, st);
                h->front_name = h->fft_2x ? "k_front_fft2x" : (h->fft_mixed ? (fftm_pairs(xa.n, xa.nframes) ? "k_front_fftm2" : "k_front_fftm") : "k_front_fft");
                const int frc = h->fft_2x ? launch_front_fft2x(xa, h->fm_np, h->fm_rad, h->fm_off, h->fm_off1, h->fft2x_ek.p, h->fft2x_r0.p, S, st)
                                          : (h->fft_mixed ? launch_front_fftm(xa, h->fm_np, h->fm_rad, h->fm_off, h->fm_off1, h->fft2x_ek.p, S, st) : launch_front_fft(xa, S, st));
                if (frc != JSDR_OK) return JSDR_ERR;
            }
            return JSDR_OK;
        };
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
        if (fft_front(xa) != JSDR_OK) return JSDR_ERR;
        if (h->seam == SEAM_TO_FFT) {
            const int D = h->decim;
            const long long nds1 = first_out < h->nsf ? (long long)((h->nsf - 1 - first_out) / D + 1) : 0;  // outputs of frame 0
            long long J = first_out <= 25 ? (long long)((25 - first_out) / D + 1) : 0;  // outputs whose windows reach back
            if (J > nds1) J = nds1;
            if (J > nds) J = nds;
            if (J > 0) {
                const char *keep = h->front_name;
                FftFrontArgs x1 = xa;
                x1.nframes = 1;
                x1.st = h->fft_state2.p;
                x1.dm = h->dm2.p;
                x1.dm_stride = h->dm2_stride;
                x1.nds = nds1;
                x1.phase_clk = nullptr;
                if (fft_front(x1) != JSDR_OK) return JSDR_ERR;
                h->front_name = keep;
                if (launch_seam_q(h->dm.p, h->dm_stride, h->dm2.p, h->dm2_stride, (int)J, S, st) != JSDR_OK) return JSDR_ERR;
            }
            h->seam = SEAM_NONE;
        }
    } else if (nds > 0 && split) {
        ProfScope ps(h, PK_FRONT, st);
        h->front_name = "k_front_split";
        const FftFrontState *dh = h->seam == SEAM_TO_TUNE ? h->fft_state.p : nullptr;  // FFT -> tune: the history is doubles
        if (launch_front_split(fa, h->ktu9.p, h->sincos9.p, h->decim, dh, S, st) != JSDR_OK) return JSDR_ERR;
    } else if (nds > 0 && fm_ok) {
        if (wait_tail(h, h->y_cur, st) != JSDR_OK) return JSDR_ERR;
        FmArgs ma;
        ma.raw = fa.raw;
        ma.stride_pairs = fa.stride_pairs;
        ma.nsamples = (int)L;
        ma.ic = ic;
        ma.qc = qc;
        ma.edges = h->fm_edges.p;
        ma.tcs = tcs_p;
        ma.tper = h->cur.mix ? h->cur.tper : 1;
        ma.kvco = kvco_p;
        ma.sincos = h->sincos.p;
        ma.dmh_old = h->dmh[h->dmh_cur].p;
        ma.dmh_new = h->dmh[h->dmh_cur ^ 1].p;
        ma.y = h->y[h->y_cur].p + Y_PAD;
        ma.y_stride = h->y_stride;
        ma.nds = (int)nds;
        ma.g_first = g_first;
        ma.tile0 = first_block(g_first);
        ma.first_out = first_out;
        ma.amax = h->amax.p;
        ma.grid_limit = h->share_wgs_per_cu * h->num_cu;  // (jsdr_bpsk_set_cu_share has asked for the CU count)
        ma.tickets = h->fm_tickets.p;
        ma.trot = h->cur.mix == 1 ? h->cur.trot : -1;
        if (rawf_dev) {
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
            hist_done = true;
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
            // the next call's 26-sample input history, in the same launch (k_hist_in's work)
            const HistArgs ha = hist_args(h, fa.raw, nullptr, fa.stride_pairs, L, ic, qc, S);
            ProfScope psh(h, PK_PREP, st);
            if (launch_fm_prep(ea, ha, sc, st) != JSDR_OK) return JSDR_ERR;
            hist_done = true;
        }
        ProfScope ps(h, PK_FM, st);
        if (rawf_dev) {
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
    } else if (nds > 0) {
        ProfScope ps(h, PK_FRONT, st);
        const bool fast = false;  // (a fast handle whose call cannot take k_fm runs it in exact order: the amplitude the
                                  //  fast variant's bound scales with is tracked by k_fm only)
        const char *front = launch_front(fa, h->decim, S, fast, st);
        if (!front) return JSDR_ERR;
        h->front_name = front;
    }
    if (!h->do_fft && hist_done) h->hist_cur ^= 1;
    if (!h->do_fft && !hist_done)
        if (run_hist_in(h, hist_args(h, fa.raw, fa.rawf, fa.stride_pairs, L, ic, qc, S), st) != JSDR_OK) return JSDR_ERR;
    const int yb = h->y_cur;
    if (wait_tail(h, yb, st) != JSDR_OK) return JSDR_ERR;
    if (nds > 0 && !(fm_ok && !h->do_fft) && run_matched(h, yb, nds, g_first, st) != JSDR_OK) return JSDR_ERR;
    if (finish_call(h, yb, L, nds, g_first, first_out, ic, qc, fa.raw, fa.stride_pairs, kvco_p, tcs_p, st) != JSDR_OK) return JSDR_ERR;
    if (!h->do_fft && h->seam == SEAM_TO_TUNE) {
        h->seam = SEAM_NONE;
        h->hist_is_float = rawf_dev != nullptr;
    }
    if (!h->do_fft) {
        mhist_advance(h->h_mhist, L, f0, n0);  // the mix flags of the 26 samples before the next call
    }
    return JSDR_OK;
}

// ------------------------------------------------------------------------------------------- FFT-acquire set-up
// Which FFT-acquire front end serves a frame of n samples at a decimation of decim.  The power-of-two (1024 .. 8192) and the
// 2 m front ends size their per-thread output lists for a decimation of at least 4; the mixed-radix one (any other frame up
// to 9600 samples) loops and takes any.  Whatever those refuse -- and any other frame the oracle defines -- goes through the
// any-frame passes (bpsk_acqg.hip); FRONT_NONE: no front end takes the frame.
// chan_form (jsdr_bpsk_create_mode_channels): a channel handle has the three-phase front ends only, so every frame that is
// not one of theirs (2^k of 1024 .. 8192 at a decimation of 4 and more, 9600 / 4800 / 4410) takes the any-frame passes' plan.
// force_gen (jsdr_bpsk_create under JSDR_ACQG, tests): 1 the any-frame passes for a frame the LDS kernels take, 0 never them.
static FftFront fft_front_kind(int n, int decim, bool chan_form, int force_gen = -1)
{
    const bool pow2 = n >= 1024 && n <= 8192 && (n & (n - 1)) == 0;
    const bool lds = chan_form ? ((pow2 && decim >= 4) || acqm_supported(n)) : (fftm_supported(n) || (decim >= 4 && (pow2 || fft2x_supported(n))));
    if (force_gen >= 0 ? force_gen != 0 : !lds) return acqg_supported(n) ? FRONT_GEN : FRONT_NONE;
    return pow2 ? FRONT_POW2 : fft2x_supported(n) ? FRONT_FFT2X : FRONT_FFTM;
}

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
static int fft_mode_alloc(jsdr_bpsk *h, FftFront kind, bool seam)
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
    AcqgPlan plan;
    int np = 0, rad[12] = {0}, off[12] = {0}, off1[12] = {0};
    bool ok = !want_seam || (st2.alloc(S) == JSDR_OK && dm2.alloc(S * (size_t)stride2) == JSDR_OK && st2.zero() == JSDR_OK && dm2.zero() == JSDR_OK);
    if (ok && !h->fft_ready) {
        ok = st.alloc(S) == JSDR_OK && vcs.alloc((size_t)h->max_ds) == JSDR_OK &&
             tw.alloc(gen ? 3 * (size_t)n + 64 : pow2 ? (size_t)n : (size_t)65536) == JSDR_OK &&
             (!f2x || (ek.alloc(S * fft2x_scratch_ek(n)) == JSDR_OK && r0.alloc(S * fft2x_scratch_r0(n)) == JSDR_OK)) &&
             // (a mixed-radix frame with a prime factor above 7: the out-of-place pass's scratch, in the 2 m front end's slot)
             (!(kind == FRONT_FFTM && fftm_scratch(n) > 0) || ek.alloc(S * fftm_scratch(n)) == JSDR_OK);
        if (ok) {
            if (gen) acqg_twiddles(w, n, &plan);
            else if (pow2) fft_twiddles_f64(w, n);
            else if (f2x) fft2x_twiddles(w, n, &np, rad, off, off1);
            else fftm_twiddles(w, n, &np, rad, off, off1);  // (off1: the prime radices' r-point tables)
            ok = w.size() <= tw.n && hipMemcpy(tw.p, w.data(), sizeof(double2) * w.size(), hipMemcpyHostToDevice) == hipSuccess &&
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
        h->fft_mixed = !pow2 && !gen;
        h->fft_2x = f2x;
        h->gen_plan = plan;
        h->fm_np = np;
        memcpy(h->fm_rad, rad, sizeof(rad));
        memcpy(h->fm_off, off, sizeof(off));
        memcpy(h->fm_off1, off1, sizeof(off1));
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
    const char *const *names = h->fft_mixed ? names_mx : names_p2;
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

extern "C" {

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

static int publish_snapshot(jsdr_bpsk *h)
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

static int sync_last(jsdr_bpsk *h)
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

// ------------------------------------------------------------------------------------------- live control
// FUNcubeBPSKDemod.actionPerformed (:177-190) between two calls.  Every check comes first: a refused call leaves the handle
// exactly as it was.  Then the handle's own work is waited for (the previous call's tail and FEC on the side stream finish
// with the settings they were launched with), the schedule prefetch is joined, and dmMaxCorr is zeroed in every stream.
// tuPhase, the down-sampler and matched-filter histories, vcoPhase, the tail state, the FEC register and the counters carry on.
// The schedules need no word from here: their keys hold tuPhaseInc and the mode, so one computed for the old settings does
// not match the next call.  The device copy of the tables is marked stale, which makes that call send its own.
}  // extern "C"

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
        const size_t per = acq3_frame_bytes(h->nsf, do_up) + 64 + (h->gen_plan.on ? acqg_image_bytes(h->nsf) : 0);
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
                if (acq_scratch_ensure(h, acq3c_frame_bytes(h->nsf, mask, h->gen_plan.on), (size_t)h->nin, 4096) != JSDR_OK) {
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

extern "C" {

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
    return live_apply(h, tuning_hz, do_fft != 0, do_up != 0, false);
}

int jsdr_bpsk_get_control(jsdr_bpsk *h, double *tuning_hz, int *do_fft, int *do_up)
{
    JSDR_REQUIRE(h && tuning_hz && do_fft && do_up, "jsdr_bpsk_get_control: null argument");
    *tuning_hz = h->pst ? h->pst_tuning[0] : h->tuning;    // (a tuned handle reports stream 0)
    *do_fft = h->nch > 0 ? h->chan[0].do_fft : h->do_fft;  // (a channel handle reports channel 0)
    *do_up = h->do_up;
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

int jsdr_bpsk_acq_last_launch(jsdr_bpsk *h, int64_t *fwd_frames, int64_t *inv_frames)
{
    JSDR_REQUIRE(h && fwd_frames && inv_frames, "jsdr_bpsk_acq_last_launch: null argument");
    *fwd_frames = h->acq_fwd_frames;
    *inv_frames = h->acq_inv_frames;
    return JSDR_OK;
}

int jsdr_bpsk_channel_info(jsdr_bpsk *h, int *ninputs, int *nchannels)
{
    JSDR_REQUIRE(h && ninputs && nchannels, "jsdr_bpsk_channel_info: null argument");
    *ninputs = h->nch > 0 ? h->nin : h->pst_nch > 0 ? h->pst_nin : h->nstreams;
    *nchannels = h->nch > 0 ? h->nch : h->pst_nch > 0 ? h->pst_nch : 1;
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

}  // extern "C"

extern "C" int jsdr_bpsk_pack_slots(jsdr_bpsk *h, uint8_t *slots_dev, void *stream)
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

extern "C" {

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

}  // extern "C"
