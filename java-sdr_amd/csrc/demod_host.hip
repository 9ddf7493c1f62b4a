// demod_host.hip -- demod_host.h's functions: host code only, no HIP runtime call.  Compiled with -ffp-contract=off: the
// weights are float products of double sines that must round one by one, as Java's do.
#include "demod_host.h"
#include <math.h>

namespace jsdr {

static double dsinl(double x) { return (double)sinl((long double)x); }
static double dcosl(double x) { return (double)cosl((long double)x); }

bool demod_weights_of(int rate, int flo, int fhi, float w[21], float *phi)
{
    const int len = 21;
    if ((-2147483647 - 1) == flo) {
        for (int i = 0; i < len; i++) w[i] = 0;
        w[(len - 1) / 2] = 1;
        return false;
    }
    const float frate = (float)rate;
    const float nlo = (float)flo / frate;
    const float nhi = (float)fhi / frate;
    const int ord = len - 1;
    const double PI = 3.14159265358979323846;
    for (int n = 0; n < len; n++) {
        if (n == ord / 2) {
            w[n] = 2.0f * (nhi - nlo);
        } else {
            w[n] = (float)((dsinl(2 * PI * nhi * (double)(n - ord / 2)) / (PI * (double)(n - ord / 2))) -
                           (dsinl(2 * PI * nlo * (double)(n - ord / 2)) / (PI * (double)(n - ord / 2))));
        }
        w[n] *= (float)(0.54 - 0.46 * dcosl(2 * PI * (double)n / (double)ord));
    }
    *phi = (float)(2 * PI * nlo);
    return true;
}

DemodChanPlan demod_chan_plan(const DemodCtl *ch, int K, bool fused)
{
    DemodChanPlan p;
    for (int c = 0; c < K; c++) {
        p.dslot[c] = -1;
        if (ch[c].mode == MODE_AM) {
            p.dslot[c] = p.nslots;
            p.slot_chan[p.nslots++] = c;
        }
    }
    p.nam = p.nslots;
    if (!fused)
        for (int c = 0; c < K; c++)
            if (ch[c].mode != MODE_AM) {
                p.dslot[c] = p.nslots;
                p.slot_chan[p.nslots++] = c;
            }
    for (int c = 0; c < K; c++) {
        p.nco_row[c] = 0;
        if (!ch[c].dodwn) continue;
        int r = 0;
        while (r < p.rows && (memcmp(&ch[p.row_chan[r]].car, &ch[c].car, 4) != 0 || memcmp(&ch[p.row_chan[r]].phi, &ch[c].phi, 4) != 0)) r++;
        if (r == p.rows) p.row_chan[p.rows++] = c;
        p.nco_row[c] = r;
    }
    return p;
}

}  // namespace jsdr
