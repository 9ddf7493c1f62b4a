// bpsk_sched.hip -- the host scheduler (bpsk_sched.h): schedules of a call, their keys, the period search, the channel sharing.
//
// Host code only, no HIP runtime call.  Compiled with -ffp-contract=off like the kernels: the recurrences of bpsk_tuner.h are
// stepped in host doubles (FUNcubeBPSKDemod.java:384-390, :511-516), and every product and sum must round separately, as
// Java's do.
//
// Why on the host: the recurrences round state-dependently (tuPhase += inc; wrap at 2 pi; truncate tuPhase*256/(2 pi)), so they
// are stepped one sample at a time in double, mul THEN div.  A single GPU lane needs ~35 cycles per link of this dependent FP64
// chain (17 ms per 2^20 samples, against ~4 ms on a host core), and the links cannot be spread over lanes.  What keeps it off
// the critical path instead: the state repeats exactly for periodic configurations (the handle's cached schedule matches,
// nothing is computed), and for the others the handle computes the schedule of the NEXT call on a worker thread while the GPU
// works on this one.
#include "bpsk_sched.h"
#include <thread>

namespace jsdr {

// ONE walk over the L samples of a call.  Every sample: the tuner (TUNER; bpsk_tuner.h's tuner_step) and the decimation counter
// (:468); every decimated sample: the VCO (vco_step).  The two phase chains are independent and each is bound by the latency
// of its own add - compare - multiply - divide, so walking them in one loop costs what the tuner's alone does.
struct TunerWalk {
    double tu, inc;      // tuPhase (moves to the call's end), tuPhaseInc
    unsigned char *kt;   // [L] the byte table: k9 & 255, 0 where the sample is passed through
    long long nmix = 0;  // samples that were mixed (tuPhase > 0, :388)
};
template <bool TUNER>
static long long walk(TunerWalk *t, double &vco_io, int &ds_io, int decim, long long L, std::vector<unsigned char> &kvco)
{
    kvco.clear();
    kvco.reserve((size_t)(L / decim + 2));
    double tu = TUNER ? t->tu : 0.0, vco = vco_io;
    const double inc = TUNER ? t->inc : 0.0;
    int cnt = ds_io;
    long long nmix = 0;
    for (long long n = 0; n < L; n++) {
        if (TUNER) {
            // tuner_step, its two halves around a BRANCH on the sign test: the index of a passed-through sample is never
            // computed, and the predicted branch measured 10 % faster over 2^20 samples than tuner_k9's select
            tuner_advance(tu, inc);
            int k = 0;
            if (tu > 0.0) {
                k = tuner_k9(tu);
                nmix++;
            }
            t->kt[n] = (unsigned char)k;
        }
        if (++cnt >= decim) {
            cnt = 0;
            kvco.push_back((unsigned char)vco_step(vco));
        }
    }
    if (TUNER) {
        t->tu = tu;
        t->nmix = nmix;
    }
    vco_io = vco;
    ds_io = cnt;
    return (long long)kvco.size();
}

long long vco_walk(double &vco, int &ds, int decim, long long L, std::vector<unsigned char> &kvco)
{
    return walk<false>(nullptr, vco, ds, decim, L, kvco);
}

bool vco_schedule(VcoSchedule &v, double vco, int ds, int decim, long long L)
{
    if (v.valid && v.L == L && v.vco0 == vco && v.ds0 == ds && v.decim == decim) return false;
    v.vco0 = v.vco1 = vco;
    v.ds0 = v.ds1 = ds;
    v.decim = decim;
    v.L = L;
    vco_walk(v.vco1, v.ds1, decim, L, v.kvco);
    v.valid = true;
    return true;
}

bool ScheduleKey::same_call(const ScheduleKey &o) const
{
    return L == o.L && tu0 == o.tu0 && inc == o.inc && vco0 == o.vco0 && ds0 == o.ds0 && decim == o.decim && do_fft == o.do_fft &&
           memcmp(khist0, o.khist0, sizeof(khist0)) == 0;
}

void compute_schedule(Schedule &sc, const double *sincos)
{
    const ScheduleKey &key = sc.key;
    const long long L = key.L;
    sc.ktu.resize((size_t)L + SCHED_HIST);
    memcpy(sc.ktu.data(), key.khist0, SCHED_HIST);
    TunerWalk t;
    t.tu = key.tu0;
    t.inc = key.inc;
    t.kt = sc.ktu.data() + SCHED_HIST;
    sc.vco1 = key.vco0;
    sc.ds1 = key.ds0;
    if (key.do_fft) {  // doBufferFFT never runs the tuner (:406-464): tuPhase stands still, no sample is mixed
        memset(t.kt, 0, (size_t)L);
        sc.nds = walk<false>(nullptr, sc.vco1, sc.ds1, key.decim, L, sc.kvco);
    } else {
        sc.nds = walk<true>(&t, sc.vco1, sc.ds1, key.decim, L, sc.kvco);
    }
    // tuPhase > 0 holds for every sample (tuning > 0) or for none (tuning <= 0): one flag per call
    sc.mix = (t.nmix == L) ? 1 : (t.nmix == 0 ? 0 : -1);
    sc.f0 = sc.mix == 0 ? 0 : 1;
    sc.n0 = L;
    if (sc.mix < 0) {
        // tuPhase crossed 0 inside the call (a retune, jsdr_bpsk_set_tuning).  It crosses once: at or below 0 it moves one way
        // only, and above 0 it stays there (the wrap at 2 pi leaves it above 0).  So the mixed samples are the call's first
        // nmix or its last nmix, and sample 0 tells which -- no second walk
        double tu = key.tu0;
        sc.f0 = tuner_step(tu, key.inc) != 256;
        sc.n0 = sc.f0 ? t.nmix : L - t.nmix;
    }
    sc.tu1 = t.tu;
    // Is the tuner index periodic in the sample number?  (An exact 8-cycle at 12 kHz / 96 kHz.)  The first p that the head of
    // the table repeats with is the one candidate; it counts if it holds over EVERY sample of the call, history included -- at
    // the start of a stream the 26 history samples are zeros, whose table entry does not matter.
    sc.tper = 0;
    sc.trot = -1;
    if (!key.do_fft && sc.mix == 1) {
        const long long off = key.first ? SCHED_HIST : 0;  // k[i] is the index of sample n = i + off - 26
        const unsigned char *k = sc.ktu.data() + off;
        const long long len = L + SCHED_HIST - off;
        const long long head = len < 1024 ? len : 1024;
        for (int p = 1; p <= 256 && p < len; p++) {
            if (!period_holds(k, head, p)) continue;
            if (period_holds(k, len, p)) {
                sc.tper = p;
                // unwrapped table: entry e <-> samples n with (n + 26) mod p == e mod p
                sc.tcs.resize((size_t)p + SCHED_TABLE_SLACK);
                for (int e = 0; e < p + SCHED_TABLE_SLACK; e++) {
                    const int i = (int)(((e - off) % p + p) % p);  // smallest i >= 0 with (i + off) mod p == e mod p
                    const int kk = k[i];
                    sc.tcs[(size_t)e] = make_double2(sincos[kk], sincos[256 + kk]);
                }
                if (p == 8) sc.trot = tuner8_rotation(sc.tcs.data());  // (every entry beyond the first period repeats it)
            }
            break;
        }
    }
    sc.valid = true;
}

bool ChanKey::operator==(const ChanKey &o) const
{
    return tu0 == o.tu0 && inc == o.inc && L == o.L && first == o.first && memcmp(hist0, o.hist0, sizeof(hist0)) == 0;
}

// The tuner walk with the sign test (:388) folded into the index (256: pass-through).  Then the shortest period p <= 256 that
// holds over every sample of the call (and the 26 history samples, except at the stream's start, where they are zeros and
// their factor does not matter) -- one period is all the device needs.
void chan_compute(ChanSchedule &c)
{
    const long long L = c.key.L;
    std::vector<unsigned short> full((size_t)L + SCHED_HIST);
    memcpy(full.data(), c.key.hist0, sizeof(c.key.hist0));
    double tu = c.key.tu0;
    const double inc = c.key.inc;
    unsigned short *kt = full.data() + SCHED_HIST;
    for (long long n = 0; n < L; n++) kt[n] = (unsigned short)tuner_step(tu, inc);
    c.tu1 = tu;
    memcpy(c.khist1, full.data() + L, sizeof(c.khist1));
    const long long off = c.key.first ? SCHED_HIST : 0;
    const long long len = L + SCHED_HIST - off;
    const unsigned short *k = full.data() + off;
    c.per = 0;
    for (int p = 1; p <= 256 && p < len; p++) {
        if (!period_holds(k, len, p)) continue;
        c.per = p;
        c.tab.resize((size_t)p);
        for (int e = 0; e < p; e++) c.tab[(size_t)e] = k[(((e - off) % p) + p) % p];  // the entry of the samples n + 26 == e mod p
        break;
    }
    if (c.per == 0) c.tab.swap(full);
    c.valid = true;
}

// A channel whose state has come back to where its schedule started keeps that one (a periodic tuning with a call length of
// whole periods: nothing to build after its first calls); of the others, those with equal keys share one computation, and the
// computations run in parallel, one thread each (at most 16, the most channels a handle has), for calls long enough to pay
// for the threads.
int chan_schedules(ChanSchedule *const *sched, const ChanKey *want, int n, bool *fresh)
{
    std::vector<int> lead;
    std::vector<int> follow((size_t)n, -1);
    long long L = 0;
    for (int c = 0; c < n; c++) {
        fresh[c] = false;
        if (!sched[c]) continue;
        ChanSchedule &s = *sched[c];
        if (s.valid && s.key == want[c]) continue;
        s.key = want[c];
        fresh[c] = true;
        L = want[c].L;
        for (int l : lead)
            if (sched[l]->key == s.key) follow[(size_t)c] = l;
        if (follow[(size_t)c] < 0) lead.push_back(c);
    }
    if (lead.size() >= 2 && L >= 65536) {
        std::vector<std::thread> pool;
        for (int l : lead) pool.emplace_back([sched, l] { chan_compute(*sched[l]); });
        for (auto &t : pool) t.join();
    } else {
        for (int l : lead) chan_compute(*sched[l]);
    }
    for (int c = 0; c < n; c++) {
        if (follow[(size_t)c] < 0) continue;
        const ChanSchedule &src = *sched[follow[(size_t)c]];
        ChanSchedule &s = *sched[c];
        s.tu1 = src.tu1;
        memcpy(s.khist1, src.khist1, sizeof(s.khist1));
        s.per = src.per;
        s.tab = src.tab;
        s.valid = true;
    }
    return (int)lead.size();
}

void mhist_advance(unsigned char mhist[SCHED_HIST], long long L, int f0, long long n0)
{
    unsigned char nh[SCHED_HIST];
    for (int i = 0; i < SCHED_HIST; i++) {
        const long long n = L - SCHED_HIST + i;
        nh[i] = n < 0 ? mhist[L + i] : (unsigned char)((n < n0) ? f0 : !f0);
    }
    memcpy(mhist, nh, SCHED_HIST);
}

}  // namespace jsdr
