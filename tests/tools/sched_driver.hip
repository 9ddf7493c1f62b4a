// sched_driver.hip -- a stand-alone driver of the host scheduler (java-sdr_amd/csrc/bpsk_sched.hip) for
// tests/test_bpsk_sched_host.py: no device, no library.  Reads one command a line from stdin and answers each on stdout.
// Doubles travel as C99 hex floats, tables as hex strings (two digits an entry for bytes, four for 9-bit entries).
//
//   inc TUNING RATE                                          -> inc
//   sched TU0 INC VCO0 DS0 DECIM L DO_FFT FIRST KHIST        -> mix f0 n0 tper nds tu1 vco1 ds1 / ktu / kvco / tcs  (kept: "the schedule")
//   match TU0 INC VCO0 DS0 DECIM L DO_FFT FIRST KHIST        -> does the schedule match this key: 0 / 1
//   expand8 MHIST|-                                          -> the 9-bit expansion of the schedule (- : history passed through)
//   mhist MHIST L F0 N0                                      -> the mix flags before the next call
//   vco VCO0 DS0 DECIM L                                     -> computed nds vco1 ds1 / kvco                (one VcoSchedule is kept)
//   chans N, then N lines  TU0 INC L FIRST HIST | -          -> computed / per channel: fresh per tu1 / khist1 / tab  (N kept)
//   expand9 C                                                -> the seam expansion of channel C's schedule
//
// The sin / cos table given to compute_schedule holds cos[k] = k and sin[k] = 1000 + k, so the periodic table shows its indices.
#include "../../java-sdr_amd/csrc/bpsk_sched.h"
#include <iostream>
#include <sstream>
#include <string>

using namespace jsdr;

static double rd(std::istream &in)
{
    std::string s;
    in >> s;
    return strtod(s.c_str(), nullptr);
}
template <class K>
static void rd_tab(std::istream &in, K *dst, int n)
{
    std::string s;
    in >> s;
    const int w = 2 * (int)sizeof(K);
    for (int i = 0; i < n; i++) dst[i] = (K)strtoul(s.substr((size_t)(i * w), (size_t)w).c_str(), nullptr, 16);
}
template <class K>
static void wr_tab(const char *name, const K *k, size_t n)
{
    printf("%s ", name);
    for (size_t i = 0; i < n; i++) printf(sizeof(K) == 1 ? "%02x" : "%04x", (unsigned)k[i]);
    printf("\n");
}
static ScheduleKey rd_key(std::istream &in)
{
    ScheduleKey k;
    k.tu0 = rd(in);
    k.inc = rd(in);
    k.vco0 = rd(in);
    int do_fft, first;
    in >> k.ds0 >> k.decim >> k.L >> do_fft >> first;
    k.do_fft = do_fft != 0;
    k.first = first != 0;
    rd_tab(in, k.khist0, SCHED_HIST);
    return k;
}

int main()
{
    std::vector<double> sincos(512);
    for (int k = 0; k < 256; k++) {
        sincos[(size_t)k] = (double)k;
        sincos[(size_t)(256 + k)] = (double)(1000 + k);
    }
    Schedule sc;
    VcoSchedule vs;
    ChanSchedule ch[16];
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "inc") {
            const double tuning = rd(in);
            int rate;
            in >> rate;
            printf("%a\n", tuner_inc(tuning, rate));
        } else if (cmd == "sched") {
            schedule_key(sc, rd_key(in));
            compute_schedule(sc, sincos.data());
            printf("%d %d %lld %d %lld %a %a %d\n", sc.mix, sc.f0, sc.n0, sc.tper, sc.nds, sc.tu1, sc.vco1, sc.ds1);
            wr_tab("ktu", sc.ktu.data(), sc.ktu.size());
            wr_tab("kvco", sc.kvco.data(), sc.kvco.size());
            printf("tcs");
            for (size_t e = 0; sc.tper > 0 && e < sc.tcs.size(); e++) printf(" %d:%d", (int)sc.tcs[e].x, (int)sc.tcs[e].y);
            printf("\n");
        } else if (cmd == "match") {
            printf("%d\n", schedule_matches(sc, rd_key(in)) ? 1 : 0);
        } else if (cmd == "expand8") {
            std::string m;
            in >> m;
            unsigned char mh[SCHED_HIST];
            if (m != "-") {
                std::istringstream ms(m);
                rd_tab(ms, mh, SCHED_HIST);
            }
            std::vector<unsigned short> out;
            expand_k9(out, sc.ktu.data(), 0, sc.key.L, m != "-" ? mh : nullptr, sc.f0, sc.n0);
            wr_tab("k9", out.data(), out.size());
        } else if (cmd == "mhist") {
            unsigned char mh[SCHED_HIST];
            rd_tab(in, mh, SCHED_HIST);
            long long L, n0;
            int f0;
            in >> L >> f0 >> n0;
            mhist_advance(mh, L, f0, n0);
            wr_tab("mhist", mh, SCHED_HIST);
        } else if (cmd == "vco") {
            const double vco0 = rd(in);
            int ds0, decim;
            long long L;
            in >> ds0 >> decim >> L;
            const bool computed = vco_schedule(vs, vco0, ds0, decim, L);
            printf("%d %zu %a %d\n", computed ? 1 : 0, vs.kvco.size(), vs.vco1, vs.ds1);
            wr_tab("kvco", vs.kvco.data(), vs.kvco.size());
        } else if (cmd == "chans") {
            int n;
            in >> n;
            ChanSchedule *sched[16];
            ChanKey want[16];
            bool fresh[16];
            for (int c = 0; c < n; c++) {
                std::getline(std::cin, line);
                std::istringstream cin2(line);
                sched[c] = &ch[c];
                if (line == "-") {
                    sched[c] = nullptr;
                    continue;
                }
                want[c].tu0 = rd(cin2);
                want[c].inc = rd(cin2);
                int first;
                cin2 >> want[c].L >> first;
                want[c].first = first != 0;
                rd_tab(cin2, want[c].hist0, SCHED_HIST);
            }
            printf("%d\n", chan_schedules(sched, want, n, fresh));
            for (int c = 0; c < n; c++) {
                printf("%d %d %a\n", fresh[c] ? 1 : 0, ch[c].per, ch[c].tu1);
                wr_tab("khist1", ch[c].khist1, (size_t)SCHED_HIST);
                wr_tab("tab", ch[c].tab.data(), ch[c].tab.size());
            }
        } else if (cmd == "expand9") {
            int c;
            in >> c;
            std::vector<unsigned short> out;
            expand_k9(out, ch[c].tab.data(), ch[c].per, ch[c].key.L, nullptr, 1, ch[c].key.L);
            wr_tab("k9", out.data(), out.size());
        } else {
            fprintf(stderr, "sched_driver: unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
