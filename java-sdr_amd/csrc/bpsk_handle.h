// bpsk_handle.h -- struct jsdr_bpsk and what the host units that work on it share (internal, not installed).
//
// The handle's host code is cut by what it does to the handle, one unit each, host code only, no kernel defined or launched:
//   bpsk_handle.hip     lifecycle: the tap tables, FFT-acquire set-up, jsdr_bpsk_create*, jsdr_bpsk_destroy, the knobs
//   bpsk_call.hip       an ordinary handle's call: the schedule glue, the stages of a call, bpsk_run, batch / receive / recover
//   bpsk_call_chan.hip  a channel handle's call: chan_run
//   bpsk_call_pst.hip   a tuned handle's call: pst_run
//   bpsk_results.hip    what a call left: the getters, the snapshot, profiling, the packed slots
//   bpsk_control.hip    live control between calls: tuning, mode, per-stream tunings and tuning plans
//   bpsk_ckpt.hip       checkpoints: jsdr_bpsk_save / jsdr_bpsk_restore
// (bpsk_scope.hip, the painter's scope passes behind a batch call, holds its own kernels beside its host code.)
// The kernels come in through the launch_* functions of bpsk_kernels.h, bpsk_fft.h, bpsk_chan.h, bpsk_pst.h and bpsk_fec.h.  The
// handle fills their argument structs and calls the launchers, each stage of a call in ONE function that every kind of handle
// (ordinary, channel, tuned) calls.
//
// The input-independent schedule of a call (tuPhase, vcoPhase, dsCnt stepped in host doubles; the period search; the keys that
// say which call a schedule serves) is bpsk_sched.hip's.  The handle holds schedules, decides when one is computed -- on the
// calling thread, or a call ahead on a worker -- and keeps their device copies.
//
// Every unit is compiled with -ffp-contract=off like the kernels and the scheduler: tuPhaseInc and the ramps' tunings
// (bpsk_tuner.h) and the sin / cos tables are computed in host doubles, and every product and sum must round separately, as
// Java's do.
//
// One call of receive() on a one-stream handle is ~70 us, its host code on the critical path: everything it runs between
// jsdr_bpsk_receive_* and the launch_* functions is in bpsk_call.hip or inline here.
#pragma once
#include "bpsk_kernels.h"
#include "bpsk_fec.h"
#include "bpsk_fftplan.h"
#include "bpsk_chan.h"
#include "bpsk_pst.h"
#include "bpsk_sched.h"
#include <atomic>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace jsdr {
// (internal to the library: nothing here is part of what libjsdr_hip.so exports)
#pragma GCC visibility push(hidden)

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

enum { PK_FRONT = 0, PK_HIST, PK_MATCHED, PK_DMHIST, PK_TAIL, PK_SYNC, PK_SYNCFIN, PK_FEC, PK_FM, PK_SYNCT, PK_PREP,
       PK_ACQ_FWD, PK_ACQ_SCAN, PK_ACQ_INV, PK_ACQ_EDGES, PK_ACQC_FWD, PK_TWALK, PK_COUNT };

enum { SEAM_NONE = 0, SEAM_TO_FFT = 1, SEAM_TO_TUNE = 2 };

#pragma GCC visibility pop
}  // namespace jsdr

using namespace jsdr;  // (every unit that includes this header is the library's own host code)

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
    // the FFT-acquire plan of the handle's frame (bpsk_fftplan.h), fixed when the FFT-acquire buffers are made; its kind: FRONT_FFTM
    // the frame is not a power of two (bpsk_fftm.hip), FRONT_FFT2X it is 2 m with m such a frame (n = 19200), FRONT_GEN none of the
    // LDS front ends takes the frame (or its decimation): bpsk_acqg.hip, always in three phases
    FftPlan fft_plan;
    DevBuf<double2> fft2x_ek;  // per-stream scratch of the 2 m front end (a mixed-radix frame with a prime radix above 7: of its out-of-place pass)
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
    // the scope (jsdr_bpsk_scope_*, bpsk_scope.hip).  scope_origin: the decimated samples before the reference's ring indices were
    // last reset (setup, :198-204: jsdr_bpsk_reconfigure); the rest is the scope passes' scratch, allocated at the first scope call
    long long scope_origin = 0;
    DevBuf<TailState> scope_tail0;               // [S] the tail state of before the call (the walk starts from it)
    DevBuf<unsigned short> scope_k9;             // [26 + max_batch] the call's 9-bit tuner indices (expand_k9)
    std::vector<unsigned short> scope_h_k9;
    Event scope_ev_copy, scope_ev_walk;          // side stream -> caller's: the copy is made; caller's -> side: the walk has read it
    bool scope_walk_pending = false;
    std::string scope_name;                      // jsdr_bpsk_scope_kernel
    // the scope's spectra (jsdr_bpsk_scope_spectra_*): the plans of the rows of n and of L points with their tables, built at the
    // first spectra call; the handle's own `tuned` / `ds` rows of one pass of frames, for a spectrum whose rows the caller did not
    // ask for, and the 26 inputs in front of a pass that does not start the call; all allocated at the first call that needs them
    FftPlan scope_spec_plan[2];
    DevBuf<double2> scope_spec_w[2];
    DevBuf<double2> scope_spec_tuned;            // [S][c][n]
    DevBuf<double> scope_spec_ds;                // [S][c][L][2]
    DevBuf<int2> scope_spec_hist;                // [S][32]
    int scope_spec_chunk = 0;                    // jsdr_bpsk_scope_chunk: frames of a pass at most (0: what 64 MiB of rows hold)
};

namespace jsdr {
#pragma GCC visibility push(hidden)

// whether a stream runs FFT-acquire (state doubles 6 / 7 and counter centreBin are live), and where its FftFrontState sits
inline bool stream_fft(const jsdr_bpsk *h, int stream)
{
    return h->nch > 0 ? (h->nfftch > 0 && h->chan[stream % h->nch].do_fft != 0) : h->do_fft != 0;
}
inline size_t fft_state_at(const jsdr_bpsk *h, int stream)
{
    return h->nch > 0 ? (size_t)(stream % h->nch) * (size_t)h->nin + (size_t)(stream / h->nch) : (size_t)stream;
}

// the input rows of a tuned handle's call: its streams, or the inputs of a tuned channel handle
inline int pst_rows_in(const jsdr_bpsk *h)
{
    return h->pst_nch > 0 ? h->pst_nin : h->nstreams;
}

inline void pst_plan_clear(jsdr_bpsk *h)  // no plan pends (the device copy stays until a plan replaces it)
{
    h->pst_plan_n = 0;
    h->pst_plan_max_at = -1;
    h->pst_plan_ramp = false;
    h->pst_plan_last.clear();
}

// where the current schedule's tables sit in kvco / tcs (both double-buffered, tab_cur)
inline unsigned char *kvco_cur(const jsdr_bpsk *h) { return h->kvco.p + (size_t)h->tab_cur * (size_t)h->max_ds; }
inline double2 *tcs_cur(const jsdr_bpsk *h) { return h->tcs.p + (size_t)h->tab_cur * (256 + FM_TABLE_SLACK); }

// The tune -> FFT seam of a call whose first output comes of sample first_out: frame 0 (n samples) yields *nds1 of the call's nds
// outputs, and the windows of the first J of them -- returned -- reach back into the 26 samples before the call.
inline long long seam_outputs(int first_out, int n, int decim, long long nds, long long *nds1 = nullptr)
{
    const long long n1 = first_out < n ? (long long)((n - 1 - first_out) / decim + 1) : 0;  // outputs of frame 0
    long long J = first_out <= 25 ? (long long)((25 - first_out) / decim + 1) : 0;         // outputs whose windows reach back
    if (J > n1) J = n1;
    if (J > nds) J = nds;
    if (nds1) *nds1 = n1;
    return J;
}

// optional per-kernel HIP-event timing (jsdr_bpsk_profile_enable): a scope around a launch, its events taken from the handle's pool
inline Event prof_event(jsdr_bpsk *h)
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
// what launch_acq3 / launch_acq3_chan take beside the arguments and the handle's plan: the per-phase timing hook
struct AcqLaunchCtx {
    AcqProfCtx pc;
    AcqProf prof;
};

// host -> device copy of a call's input or tables: through the pinned arena inside receive_*(), pageable otherwise
inline int h2d_call(jsdr_bpsk *h, void *dst_dev, const void *src_host, size_t bytes, hipStream_t st)
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

// the tail that last read y[yb] (two calls ago) must be done before the matched filter (or k_fm) overwrites it
inline int wait_tail(jsdr_bpsk *h, int yb, hipStream_t st)
{
    if (h->overlap && h->tail_pending[yb]) {
        JSDR_HIP_TRY(hipStreamWaitEvent(st, h->ev_tail_done[yb], 0));
        h->tail_pending[yb] = false;
    }
    return JSDR_OK;
}

// the next call's 26-sample input history of `rows` rows (streams, or inputs of a channel handle): k_hist_in's work
inline HistArgs hist_args(const jsdr_bpsk *h, const int *raw, const float2 *rawf, long long stride_pairs, long long L, int ic, int qc,
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

// ------------------------------------------------------------------------------------------- what crosses a unit boundary
// bpsk_handle.hip.  fft_mode_alloc: the FFT-acquire buffers of a handle and its plan for the front end `kind` (fft_front_kind,
// bpsk_fftplan.h), all or nothing
int fft_mode_alloc(jsdr_bpsk *h, FftFront kind, bool seam);

// bpsk_call.hip: the stages of a call, in the order chan_run, pst_run and bpsk_run put their work onto the caller's stream
long long build_schedule(jsdr_bpsk *h, long long L);
int device_cus(jsdr_bpsk *h);
int acq_scratch_ensure(jsdr_bpsk *h, size_t per_row_frame, size_t rows, size_t slack);
FftFrontArgs fft_front_args(jsdr_bpsk *h, const int *raw, const float2 *rawf, long long stride_pairs, long long L, int ic, int qc,
                            int first_out, long long nds);
void acq_launch_ctx(jsdr_bpsk *h, AcqLaunchCtx &c);
int send_vco_cs(jsdr_bpsk *h, long long nds, hipStream_t st);
int sincos9_ensure(jsdr_bpsk *h);
int run_hist_in(jsdr_bpsk *h, const HistArgs &ha, hipStream_t st);
int hist_form(jsdr_bpsk *h, bool want_float, int rows, hipStream_t st);
int run_matched(jsdr_bpsk *h, int yb, long long nds, long long g_first, hipStream_t st);
int finish_call(jsdr_bpsk *h, int yb, long long L, long long nds, long long g_first, int first_out, int ic, int qc, const int *raw,
                long long stride_pairs, unsigned char *kvco_p, double2 *tcs_p, hipStream_t st);

// bpsk_call_chan.hip, bpsk_call_pst.hip: a call of a channel handle, of a tuned handle (bpsk_run hands them theirs)
int chan_run(jsdr_bpsk *h, const int16_t *raw_dev, const float *rawf_dev, long long stride_i16, long long L, int ic, int qc,
             hipStream_t st);
int pst_run(jsdr_bpsk *h, const int16_t *raw_dev, const float *rawf_dev, long long stride_i16, long long L, int ic, int qc,
            hipStream_t st);

// bpsk_results.hip.  sync_last: waits for the handle's last call (and its shadow's); publish_snapshot: receive()'s results,
// fetched in one copy and published to the reader
int sync_last(jsdr_bpsk *h);
int publish_snapshot(jsdr_bpsk *h);

#pragma GCC visibility pop
}  // namespace jsdr

// bpsk_control.hip: the checks of jsdr_bpsk_set_tuning / _set_mode, which jsdr_group_* (group.hip) makes on every rank's handle
// before any of them acts
int bpsk_live_check(jsdr_bpsk *h, int do_fft, const char *who);
