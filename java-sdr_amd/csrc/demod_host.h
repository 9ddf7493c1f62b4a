// demod_host.h -- the part of a demod handle's host side that needs no device: one receiver's controls, demod.weights(),
// the carrier walk, and which carrier tables and float rows a channel call needs.  These decide whether the audio stays
// bit-identical to the reference.  No HIP runtime call and no handle in here: plain values and these structs, and
// tests/test_demod_host.py drives the unit without a GPU.  Compiled with -ffp-contract=off.
#pragma once
#include "demod.h"

namespace jsdr {
// (internal to the library: nothing here is part of what libjsdr_hip.so exports)
#pragma GCC visibility push(hidden)

// the controls of one receiver (demod.java's mode / dofir / dodwn / doagc, flo / fhi, wfir, phi, car): an ordinary handle has
// one for all its streams, a channel handle one a channel
struct DemodCtl {
    int mode = MODE_OFF, dofir = 0, dodwn = 0, doagc = 0;
    int flo = (-2147483647 - 1), fhi = 2147483647;
    float w[21] = {0};
    float phi = 0.0f, car = 0.0f;
};

// demod.weights() (:341-375) for the band [flo, fhi] at `rate` into w; a band-pass (false for flo = INT_MIN, the all-pass
// impulse) also sets phi
bool demod_weights_of(int rate, int flo, int fhi, float w[21], float *phi);

// the fields DemodConst and DemodChanConst share, from one receiver's controls
template <class C>
inline void demod_const_of(const DemodCtl &ctl, int rate, C &c)
{
    memcpy(c.w, ctl.w, sizeof(c.w));
    c.fmgain = (float)rate / (MODE_NFM == ctl.mode ? 5000.0f : 75000.0f);  // :410
    c.mode = ctl.mode;
    c.dofir = ctl.dofir;
    c.dodwn = ctl.dodwn;
    c.doagc = ctl.doagc;
}

// :427-429 in float, exactly as the reference steps it: tab[g] = the phase at sample g, returns the phase after L samples.
// A serial float recurrence, on the host; kept as a (well predicted) branch so that the dependent chain per sample is the
// one subtraction -- as a select it is subtract + add + blend, four times slower, and longer than the GPU takes for the
// whole batch
inline float demod_carrier_walk(float *tab, float car, float phi, int64_t L)
{
    const float two_pi = (float)(2 * 3.14159265358979323846);
    for (int64_t g = 0; g < L; g++) {
        tab[g] = car;
        car -= phi;
        if (__builtin_expect(car < 0.0f, 0)) {
            asm volatile("" : "+x"(car));
            car += two_pi;
        }
    }
    return car;
}

// What a call of K channels needs, from their controls alone.
struct DemodChanPlan {
    // float rows in d: the AM channels (their mean needs the whole frame), then, when not fused (frames above 5 tiles), every other one
    int dslot[DCHAN_MAX] = {0};      // a channel's slot, -1: none
    int slot_chan[DCHAN_MAX] = {0};  // the channel of a slot
    int nam = 0, nslots = 0;         // AM slots (they come first), all slots
    // distinct carrier tables: one per (car, phi) BIT PATTERN among the down-converting channels
    int nco_row[DCHAN_MAX] = {0};    // a channel's table (0 where it does not down-convert)
    int row_chan[DCHAN_MAX] = {0};   // the first channel of a table: its car and phi are the table's
    int rows = 0;
};
DemodChanPlan demod_chan_plan(const DemodCtl *ch, int K, bool fused);

#pragma GCC visibility pop
}  // namespace jsdr
