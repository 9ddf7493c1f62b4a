// demod_host_driver.hip -- a stand-alone driver of the demod handle's pure host unit (java-sdr_amd/csrc/demod_host.hip) for
// tests/test_demod_host.py: no device, no library.  Reads one command a line from stdin and answers each on stdout.
// Floats travel as C99 hex floats (exact), in both directions.
//
//   weights RATE FLO FHI                        -> bandpass phi / w[0..21)      (phi starts as the float 7: untouched by the all-pass)
//   walk CAR PHI L                              -> end / tab[0..L)
//   const RATE MODE DOFIR DODWN DOAGC W0        -> fmgain mode dofir dodwn doagc w[0] w[20], of DemodConst and of DemodChanConst
//   plan FUSED K, then K lines MODE DODWN CAR PHI
//                                               -> nam nslots rows / dslot[0..K) / slot_chan[0..nslots) / nco_row[0..K) / row_chan[0..rows)
#include "../../java-sdr_amd/csrc/demod_dev.h"
#include "../../java-sdr_amd/csrc/demod_host.h"
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace jsdr;

static float rdf(std::istream &in)
{
    std::string s;
    in >> s;
    return strtof(s.c_str(), nullptr);
}
static void wr_ints(const int *v, int n)
{
    for (int i = 0; i < n; i++) printf(i ? " %d" : "%d", v[i]);
    printf("\n");
}
template <class C>
static void wr_const(const C &c)
{
    printf("%a %d %d %d %d %a %a\n", (double)c.fmgain, c.mode, c.dofir, c.dodwn, c.doagc, (double)c.w[0], (double)c.w[20]);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "weights") {
            int rate, flo, fhi;
            in >> rate >> flo >> fhi;
            float w[21], phi = 7.0f;
            const bool bandpass = demod_weights_of(rate, flo, fhi, w, &phi);
            printf("%d %a\n", bandpass ? 1 : 0, (double)phi);
            for (int i = 0; i < 21; i++) printf(i ? " %a" : "%a", (double)w[i]);
            printf("\n");
        } else if (cmd == "walk") {
            const float car = rdf(in), phi = rdf(in);
            long long L;
            in >> L;
            std::vector<float> tab((size_t)L + 1, -1.0f);  // (one guard entry behind the table)
            const float end = demod_carrier_walk(tab.data(), car, phi, L);
            printf("%a %a\n", (double)end, (double)tab[(size_t)L]);
            for (long long g = 0; g < L; g++) printf(g ? " %a" : "%a", (double)tab[(size_t)g]);
            printf("\n");
        } else if (cmd == "const") {
            DemodCtl ctl;
            int rate;
            in >> rate >> ctl.mode >> ctl.dofir >> ctl.dodwn >> ctl.doagc;
            ctl.w[0] = rdf(in);
            ctl.w[20] = -ctl.w[0];
            DemodConst a;
            DemodChanConst b;
            demod_const_of(ctl, rate, a);
            demod_const_of(ctl, rate, b);
            wr_const(a);
            wr_const(b);
        } else if (cmd == "plan") {
            int fused, K;
            in >> fused >> K;
            if (K < 1 || K > DCHAN_MAX) return 3;
            DemodCtl ch[DCHAN_MAX];
            for (int c = 0; c < K; c++) {
                std::getline(std::cin, line);
                std::istringstream cl(line);
                cl >> ch[c].mode >> ch[c].dodwn;
                ch[c].car = rdf(cl);
                ch[c].phi = rdf(cl);
            }
            const DemodChanPlan p = demod_chan_plan(ch, K, fused != 0);
            printf("%d %d %d\n", p.nam, p.nslots, p.rows);
            wr_ints(p.dslot, K);
            wr_ints(p.slot_chan, p.nslots);
            wr_ints(p.nco_row, K);
            wr_ints(p.row_chan, p.rows);
        } else {
            fprintf(stderr, "demod_host_driver: unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
