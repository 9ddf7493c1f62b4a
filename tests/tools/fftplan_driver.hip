// fftplan_driver.hip -- a stand-alone driver of the FFT-acquire plan unit (java-sdr_amd/csrc/bpsk_fftplan.hip) for
// tests/test_bpsk_fftplan_host.py: no device, no library.  Reads one command a line from stdin and answers each on stdout.
// Table entries travel as the bit patterns of their two doubles, 32 hex digits an entry.  KIND: 0 pow2, 1 fftm, 2 fft2x, 3 gen.
//
//   radices N                    -> np r0 r1 ..
//   table LEN                    -> the LEN entries of fft_table
//   plan N KIND                  -> ok kind logn np wsize lds_tw lds_tw_pair / rad .. / tw_off .. / wr_off .. / tw1_off .. / pmagic ..
//   w N KIND                     -> the entries of the plan's tables, one line
//   args N KIND ROOM PAIR SHIFT FROM -> fft_pass_args on a copy of the plan with the table offsets of the passes FROM .. np - 1
//                                   moved by SHIFT entries, against ROOM bytes of LDS (-1: the single-frame form's own, -2: the
//                                   pair form's): ok lds_tw (the prefix found, also where refused)
//   sweep LO HI                  -> per n: n fftm fft2x acqm acqg fftm_scratch, then fft_front_kind for decim 1, 2, 4, 10 x
//                                   chan_form 0, 1 x force_gen -1, 0, 1 (decim outermost), one digit each (4: none)
//   scratch N                    -> fftm_scratch fft2x_scratch_ek fft2x_scratch_r0 acqg_image_bytes
#include "../../java-sdr_amd/csrc/bpsk_fftplan.h"
#include <iostream>
#include <sstream>
#include <string>

using namespace jsdr;

static void wr_entries(const double2 *t, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        unsigned long long b[2];
        memcpy(b, &t[i], sizeof(b));
        printf("%016llx%016llx", b[0], b[1]);
    }
    printf("\n");
}
static void wr_ints(const char *name, const int *v, int n)
{
    printf("%s", name);
    for (int i = 0; i < n; i++) printf(" %d", v[i]);
    printf("\n");
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "radices") {
            int n, rad[FFT_MAXPASS];
            in >> n;
            const int np = fft_radices(n, rad);
            printf("%d", np);
            for (int p = 0; p < np; p++) printf(" %d", rad[p]);
            printf("\n");
        } else if (cmd == "table") {
            int len;
            in >> len;
            std::vector<double2> t((size_t)len);
            fft_table(t.data(), len);
            wr_entries(t.data(), t.size());
        } else if (cmd == "plan" || cmd == "w" || cmd == "args") {
            int n, kind;
            in >> n >> kind;
            FftPlan pl;
            std::vector<double2> w;
            const bool ok = fft_plan_build(pl, w, n, (FftFront)kind);
            if (cmd == "w") {
                wr_entries(w.data(), w.size());
            } else if (cmd == "plan") {
                printf("%d %d %d %d %zu %d %d\n", ok ? 1 : 0, (int)pl.kind, pl.logn, pl.np, w.size(), pl.args.lds_tw, pl.lds_tw_pair);
                wr_ints("rad", pl.rad, pl.np);
                wr_ints("tw_off", pl.tw_off, pl.np);
                wr_ints("wr_off", pl.wr_off, pl.np);
                wr_ints("tw1_off", pl.tw1_off, pl.np);
                printf("pmagic");
                for (int p = 0; p < pl.np && p < FM_MAXPASS; p++) printf(" %u", pl.args.pmagic[p]);
                printf("\n");
            } else {
                long long room;
                int pair, shift, from;
                in >> room >> pair >> shift >> from;
                if (room == -1) room = (long long)(FM_LDS_BYTES - fm_lds_fixed(n));
                if (room == -2) room = (long long)(FM_LDS_BYTES - fm2_lds_fixed(n));
                FftPlan moved = pl;
                for (int p = from; p < moved.np; p++) moved.tw_off[p] += shift;
                FftmArgs aa = {};
                const bool fits = ok && fft_pass_args(aa, moved, (size_t)room, pair != 0);
                printf("%d %d\n", fits ? 1 : 0, aa.lds_tw);  // (the prefix the tables gave, also where the plan is refused)
            }
        } else if (cmd == "sweep") {
            int lo, hi;
            in >> lo >> hi;
            static const int decims[4] = {1, 2, 4, 10};
            for (int n = lo; n <= hi; n++) {
                printf("%d %d %d %d %d %zu ", n, fftm_supported(n) ? 1 : 0, fft2x_supported(n) ? 1 : 0, acqm_supported(n) ? 1 : 0,
                       acqg_supported(n) ? 1 : 0, fftm_scratch(n));
                for (int d = 0; d < 4; d++)
                    for (int chan = 0; chan < 2; chan++)
                        for (int force = -1; force <= 1; force++) printf("%d", (int)fft_front_kind(n, decims[d], chan != 0, force));
                printf("\n");
            }
        } else if (cmd == "scratch") {
            int n;
            in >> n;
            printf("%zu %zu %zu %zu\n", fftm_scratch(n), fft2x_scratch_ek(n), fft2x_scratch_r0(n), acqg_image_bytes(n));
        } else {
            fprintf(stderr, "fftplan_driver: unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
