// demod_handle.h -- struct jsdr_demod and what the host units that work on it share (internal, not installed).
//
// The handle's host code is cut by what it does to the handle, host code only, no kernel defined in any of them:
//   demod_control.hip     between calls: create / create_channels, destroy, configure, weights, the channel accessors, profiling
//   demod_call.hip        a call: the shape check, the carrier hand-over, DemodArgs, the two runners, batch_* and receive
//   demod_scope_host.hip  the scope behind a batch call: demod_scope_layout, demod_scope_run, the scope_* entry points
//   demod_host.hip        what needs no device (demod_host.h): the weights, the carrier walk, a channel call's plan
// The kernels come in through the launch_* functions of demod.h.  Every unit is compiled with -ffp-contract=off like the
// kernels: the weights, the carrier phases and the scope's column schedules are host floats that must round as Java's do.
// One receive() of a one-stream handle is ~50 us, nearly all of it host path: demod_call.hip and what is inline here.
#pragma once
#include "demod_dev.h"
#include "demod_host.h"
#include <string>
#include <vector>

namespace jsdr {
// (internal to the library: nothing here is part of what libjsdr_hip.so exports)
#pragma GCC visibility push(hidden)

// the scope's jsdr_fft, owned like a stream or an event (counted by jsdr_live_resources among them)
inline hipError_t demod_scope_fft_release(jsdr_fft *f)
{
    (void)jsdr_fft_destroy(f);
    return hipSuccess;
}
using DemodScopeFft = Owned<jsdr_fft *, demod_scope_fft_release>;

#pragma GCC visibility pop
}  // namespace jsdr

using namespace jsdr;  // (every unit that includes this header is the library's own host code)

struct jsdr_demod {
    int rate = 0, n = 0, nstreams = 0;
    long long max_batch = 0;
    // the receivers: nstreams = nin * nch, channel c of input i is stream i * nch + c, every channel with its own controls and
    // carrier phase.  An ordinary handle (jsdr_demod_create) is nstreams inputs of ONE channel: ch[0] is the handle's controls.
    // chan (jsdr_demod_create_channels) says which runner a call takes, and little else.
    bool chan = false;
    int nin = 0, nch = 1;
    std::vector<DemodCtl> ch;
    DevBuf<float2> hist[2], lilq[2];
    PinnedStage pin;        // receive(): [frame in | audio out]
    bool pin_tried = false;
    int cur = 0;
    // carrier tables, double-buffered: call k fills set k&1 on the copy stream while call k-1's kernels still read
    // the other one (no bubble between calls for the host's phase recurrence and its upload)
    DevBuf<float2> nco[2];
    DevBuf<float> car_dev[2];
    Pinned<float> car_pinned[2];
    long long nco_pitch = 0;   // entries between two carrier tables of a set (a channel handle)
    Stream copy_stream;
    Event ev_table[2], ev_used[2];
    bool used[2] = {false, false};
    unsigned calls = 0;
    DevBuf<float> d, favg, stats;  // (d: an ordinary handle's [S][L] float rows)
    DevBuf<unsigned> fmax;
    DevBuf<float> stage_in;  // one frame, receive_f32
    DevBuf<int> stage_out;
    int last_nfr = 0;
    // optional per-kernel HIP-event timing (bench.py's roofline leg), same contract as jsdr_bpsk_profile_*
    bool prof_on = false;
    struct Rec {
        int k;
        Event a, b;
    };
    std::vector<Rec> recs;
    std::vector<Event> pool;
    // a channel handle's own
    DevBuf<float> dch;         // [dslots * nin][L] float rows (AM channels; every channel of a frame above 5 tiles)
    Event ev_done, ev_clear;   // end of the last call; a channel ring cleared after it
    bool done_any = false, clear_pending = false;
    // the demod scope (jsdr_demod_scope_*): all of it empty until the first scope call
    struct Scope {
        DevBuf<float2> dbg;    // [frames of a pass][n] mixed IQ, when the caller takes no dbg rows
        DevBuf<float> fin;     // [frames of a pass][n] final floats (trace)
        DevBuf<float> psd;     // [frames of a pass][n + 2] (spectrum)
        DevBuf<int> tab;       // int[4][width]: the column schedules of tab_width
        int tab_width = 0;
        DemodScopeFft fft;     // jsdr_fft of n samples (spectrum)
        int chunk = 0;         // jsdr_demod_scope_chunk; 0: the default
        std::string kernel;
    } scope;
};

namespace jsdr {
#pragma GCC visibility push(hidden)

enum { DK_NCO = 0, DK_FRONT, DK_STATE, DK_MEAN, DK_OUT, DK_CHAN, DK_COUNT };
// (DK_CHAN: every launch of a channel handle but the shared k_demod_nco / k_demod_mean)
inline const char *const kDemodKernels[DK_COUNT] = {"k_demod_nco", "k_demod_front", "k_demod_state", "k_demod_mean",
                                                    "k_demod_out", "k_demod_chan"};
struct DemodProf {
    jsdr_demod *h;
    hipStream_t st;
    Event a, b;
    int k;
    static Event get(jsdr_demod *h)
    {
        Event e;
        if (h->pool.empty()) {
            (void)e.create();  // (none: the scope records nothing)
        } else {
            e = std::move(h->pool.back());
            h->pool.pop_back();
        }
        return e;
    }
    DemodProf(jsdr_demod *h_, int k_, hipStream_t st_) : h(h_), st(st_), k(k_)
    {
        if (h->prof_on) {
            a = get(h);
            b = get(h);
            (void)hipEventRecord(a, st);
        }
    }
    ~DemodProf()
    {
        if (h->prof_on && a && b) {
            (void)hipEventRecord(b, st);
            h->recs.push_back({k, std::move(a), std::move(b)});
        }
    }
};

// one launch under its profile key; a failure leaves the calling function with JSDR_ERR
#define DEMOD_TIMED(h, k, st, launch)                 \
    do {                                              \
        DemodProf ps_(h, k, st);                      \
        if ((launch) != JSDR_OK) return JSDR_ERR;     \
    } while (0)

// ---- demod_call.hip, for the scope behind it
// Which carrier-table set a call uses: call k takes set k & 1.  A runner takes it (and counts the call) with
// carrier_set_take, first thing after its refusals; demod_scope_run reads the set of the call it is about to make with
// carrier_set_next BEFORE demod_run takes it, and its passes then read the table that call filled.
inline int carrier_set_next(const jsdr_demod *h) { return (int)(h->calls & 1); }
inline int carrier_set_take(jsdr_demod *h) { return (int)(h->calls++ & 1); }
// the call's readers of table set `set` are queued on st: the call after next may fill the set again
int carrier_end(jsdr_demod *h, int set, hipStream_t st);
// the arguments of an ordinary handle's kernels for the call, from the handle as it is BEFORE the call
DemodArgs demod_args_of(const jsdr_demod *h, int set, const int16_t *raw_dev, const float *rawf_dev, int64_t stride_i16, int64_t L,
                        int ic, int qc);
// one batch call of an ordinary handle
int demod_run(jsdr_demod *h, bool f32in, const int16_t *raw_dev, const float *rawf_dev, int64_t stride_i16, int64_t L, int ic, int qc,
              int16_t *audio_dev, int64_t audio_stride_i16, hipStream_t st);

#pragma GCC visibility pop
}  // namespace jsdr
