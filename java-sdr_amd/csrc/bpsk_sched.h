// bpsk_sched.h -- the host scheduler of the BPSK demodulator: the input-independent part of a call.
//
// FUNcubeBPSKDemod steps tuPhase once a sample (:384-390), and dsCnt and vcoPhase once a decimated sample (:468, :511-516),
// whatever the samples are.  Which table entry every sample is mixed with is therefore a function of the state at the start
// of a call, the call's length and the configuration: a SCHEDULE, computed here on the host in exact doubles and sent to the
// device as index tables.  The recurrences themselves are stated in bpsk_tuner.h; this unit walks them, looks for a period,
// and keeps each schedule with the complete key it was computed from, so that "is this schedule the one the call needs" is
// one comparison.  No device, no HIP runtime call and no handle in here: everything works on plain values and these structs,
// and tests/test_bpsk_sched_host.py drives it without a GPU.
#pragma once
#include "bpsk_tuner.h"
#include <vector>

namespace jsdr {
// (internal to the library: nothing here is part of what libjsdr_hip.so exports)
#pragma GCC visibility push(hidden)

enum { SCHED_HIST = 26 };  // samples before a call that its first down-sampler windows reach into (27 taps)

// ------------------------------------------------------------------------------------------- the VCO and the decimation counter
// L input samples from (vco, ds): the table index of every decimated sample of the call is left in kvco, vco and ds move to
// their values at the call's end.  Returns the number of decimated samples.  0 <= ds < decim.
long long vco_walk(double &vco, int &ds, int decim, long long L, std::vector<unsigned char> &kvco);

// the VCO schedule of a call for the handles whose tuner schedules are kept elsewhere (channel handles: one VCO for all channels)
struct VcoSchedule {
    bool valid = false;
    double vco0 = 0.0;  // the key: state at the start of the call, its length, the decimation
    int ds0 = 0, decim = 0;
    long long L = -1;
    double vco1 = 0.0;  // state at its end
    int ds1 = 0;
    std::vector<unsigned char> kvco;  // one index per decimated sample
};
// leaves the schedule of that call in v; true: it was computed (false: v held it already)
bool vco_schedule(VcoSchedule &v, double vco, int ds, int decim, long long L);

// ------------------------------------------------------------------------------------------- the ordinary handle's schedule
// Everything compute_schedule reads.  `first`: the call is the first of its stream, its 26 history samples are zeros whose
// table entry does not matter -- the period search leaves them out.
struct ScheduleKey {
    double tu0 = 0.0, inc = 0.0, vco0 = 0.0;
    int ds0 = 0, decim = 0;
    long long L = -1;
    bool do_fft = false, first = false;
    unsigned char khist0[SCHED_HIST] = {0};  // tuner indices of the 26 samples before the call
    // the same state, mode and length: the tables and end states of the two schedules are the same (`first` only decides what
    // the period search looks at)
    bool same_call(const ScheduleKey &o) const;
    bool operator==(const ScheduleKey &o) const { return same_call(o) && first == o.first; }
};

struct Schedule {
    bool valid = false;
    ScheduleKey key;
    double tu1 = 0.0, vco1 = 0.0;  // state at the call's end
    int ds1 = 0;
    int mix = 1;       // 1: every sample is mixed (tuPhase > 0, :388), 0: none, -1: tuPhase crossed 0 inside the call (after a retune)
    int f0 = 1;        // sample 0 of the call is mixed ...
    long long n0 = 0;  // ... and so is every sample before n0, none from it on (f0 == 0: the other way round; n0 = L: no crossing)
    int tper = 0;      // > 0: the tuner index is periodic in the sample number with this period; 0: no period <= 256
    int trot = -1;     // tper == 8 and the factors of tcs[0 .. 8) have the 8-phase tuner's exact classes (bpsk_tuner.h): entry e is
                       // phase e + trot; -1: any other table
    long long nds = 0;
    std::vector<unsigned char> ktu;  // [26 history + L] tuner index (0 where the sample is passed through)
    std::vector<unsigned char> kvco; // [nds]
    std::vector<double2> tcs;        // tper > 0: the unwrapped (cos, sin) table, tper + SCHED_TABLE_SLACK entries, entry e for the
                                     // samples n with (n + 26) mod tper == e mod tper
};
enum { SCHED_TABLE_SLACK = 128 };  // (== FM_TABLE_SLACK, bpsk_kernels.h: what k_fm reads past one period)

inline void schedule_key(Schedule &sc, const ScheduleKey &key)
{
    sc.valid = false;
    sc.key = key;
}
inline bool schedule_matches(const Schedule &sc, const ScheduleKey &key) { return sc.valid && sc.key == key; }
// sc.key -> the rest of sc.  sincos: cos[0..255], sin[0..255] of the reference's tables
void compute_schedule(Schedule &sc, const double *sincos);

// ------------------------------------------------------------------------------------------- a channel's tuner schedule
// The table is of 9-bit indices (256: the sample is passed through unmixed, :395).
struct ChanKey {
    double tu0 = 0.0, inc = 0.0;
    long long L = -1;
    bool first = false;
    unsigned short hist0[SCHED_HIST] = {0};  // indices of the 26 samples before the call
    bool operator==(const ChanKey &o) const;
};
struct ChanSchedule {
    bool valid = false;
    ChanKey key;
    double tu1 = 0.0;                        // tuPhase at the call's end
    unsigned short khist1[SCHED_HIST] = {0}; // the indices of its last 26 samples
    int per = 0;                             // > 0: tab holds one period (entry (n + 26) mod per); 0: tab holds 26 + L entries
    std::vector<unsigned short> tab;
};
void chan_compute(ChanSchedule &c);  // c.key -> the rest of c
// The schedules of n channels for one call.  sched[c] (null: the channel does not run the tuner in this call) is left holding
// the schedule of want[c]; fresh[c]: it was not there already.  Returns how many were computed: channels with equal keys share
// one computation.
int chan_schedules(ChanSchedule *const *sched, const ChanKey *want, int n, bool *fresh);

// ------------------------------------------------------------------------------------------- pieces both kinds share
// does the period p hold over k[0 .. len)?
template <class K>
inline bool period_holds(const K *k, long long len, int p)
{
    return p >= len || memcmp(k, k + p, sizeof(K) * (size_t)(len - p)) == 0;
}

// The 9-bit table of a call for the front end that takes a table entry or passes through sample by sample (k_front_split):
// 26 history entries, then L.  tab / per: the schedule's table, entry i for the sample n = i - 26 (per > 0: entry i mod per).
// mhist: which of the history samples were mixed (null: none -- they are the FFT path's unmixed doubles); f0 / n0 as in
// Schedule.  A sample that was not mixed gets 256, the others their table entry (which, in a 9-bit table, may be 256 itself).
template <class K>
void expand_k9(std::vector<unsigned short> &out, const K *tab, int per, long long L, const unsigned char *mhist, int f0, long long n0)
{
    out.resize((size_t)L + SCHED_HIST);
    for (long long i = 0; i < L + SCHED_HIST; i++) {
        const long long n = i - SCHED_HIST;
        const bool mixed = n < 0 ? (mhist && mhist[i]) : ((n < n0) ? f0 != 0 : f0 == 0);
        out[(size_t)i] = mixed ? (unsigned short)tab[(size_t)(per > 0 ? i % per : i)] : (unsigned short)256;
    }
}

// the mix flags of the 26 samples before the NEXT call, from those before this one and this call's f0 / n0
void mhist_advance(unsigned char mhist[SCHED_HIST], long long L, int f0, long long n0);

#pragma GCC visibility pop
}  // namespace jsdr
