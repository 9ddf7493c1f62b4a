// acq_rule_driver.hip -- a stand-alone driver of the FFT-acquire scalar rules (java-sdr_amd/csrc/bpsk_acq_rule.h) for
// tests/test_bpsk_acq_rule_host.py: no device, no library.  Reads one command a line from stdin and answers each on stdout.
// Doubles travel as C99 hex floats.
//
//   consts                                -> CFREQ_INV CFREQ_AVG PSD_INV PSD_AVG HOWARD
//   band N DO_UP                          -> beg end
//   rule N DO_UP APP ACB CB K, K lines  AVEPSD MAXBIN BINPOS
//                                         -> K lines  avePeakPower aveCentreBin centreBin  (the state after every frame; AVEPSD is
//                                            what avePsd holds at the clamped centre bin IF the frame's loop filled it)
//   max K V0 .. VK-1                      -> maxBin binPos of the ascending search over V
//   merge K V0 I0 .. VK-1 IK-1            -> maxBin binPos of the candidates merged in this order
//   first T0 FIRST_OUT D                  -> the first RxDownSample output of the frame that starts at T0
#include "../../java-sdr_amd/csrc/bpsk_acq_rule.h"
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

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "consts") {
            printf("%a %a %a %a %a\n", ACQ_CFREQ_INV, ACQ_CFREQ_AVG, ACQ_PSD_INV, ACQ_PSD_AVG, ACQ_HOWARD);
        } else if (cmd == "band") {
            int n, up;
            in >> n >> up;
            printf("%d %d\n", acq_band_beg(n, up), acq_band_end(n, up));
        } else if (cmd == "rule") {
            int n, up, k;
            in >> n >> up;
            double app = rd(in), acb = rd(in);
            int cb;
            in >> cb >> k;
            const int beg = acq_band_beg(n, up), end = acq_band_end(n, up);
            for (int f = 0; f < k; f++) {
                std::getline(std::cin, line);
                std::istringstream fr(line);
                const double psd = rd(fr), mb = rd(fr);
                int bp;
                fr >> bp;
                cb = centre_bin_clamp(cb, end);
                const double atc = acq_band_filled(cb, beg, end) ? psd : 0.0;
                centre_bin_step(app, acb, cb, atc, mb, bp);
                printf("%a %a %d\n", app, acb, cb);
            }
        } else if (cmd == "max") {
            int k;
            in >> k;
            double bv = 0.0;
            int bi = -1;
            for (int i = 0; i < k; i++) first_max_update(bv, bi, rd(in), i);
            printf("%a %d\n", bv, bi);
        } else if (cmd == "merge") {
            int k;
            in >> k;
            double bv = 0.0;
            int bi = -1;
            for (int i = 0; i < k; i++) {
                const double v = rd(in);
                int idx;
                in >> idx;
                first_max_merge(bv, bi, v, idx);
            }
            printf("%a %d\n", bv, bi);
        } else if (cmd == "first") {
            long long t0, fo;
            int d;
            in >> t0 >> fo >> d;
            printf("%lld\n", ds_first_output(t0, fo, d));
        } else if (!cmd.empty()) {
            fprintf(stderr, "acq_rule_driver: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
