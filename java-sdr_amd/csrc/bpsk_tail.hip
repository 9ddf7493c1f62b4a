// bpsk_tail.hip -- FUNcubeBPSKDemod.receive() chain for batches of independent streams, exact-order FP64: the 9600 Hz tail,
// and the overview of the device code.
//
// Reference: FUNcubeBPSKDemod.java:357-595 (receive -> doBufferTune -> RxMixTuner -> RxDownSample ->
// RxDemodulate), constants :26-96, tables :159-162.  This translation unit is compiled with
// -ffp-contract=off: every double product and sum is rounded separately, in the reference's order, so
// the slicer bits are bit-identical to the Java arithmetic by construction (tests compare with the
// oracle's restatement).
//
// This is the last of the four units of the tune-mode pipeline, which is cut by kernel family so that an edit to one
// family recompiles that family only (the two heavy ones, k_front_reg and k_fm, are 43 % of the instructions each):
//   bpsk_front.hip     : k_front, k_front_any, k_front_split, k_hist_*, k_seam_*
//   bpsk_front_reg.hip : k_front_reg
//   bpsk_fm.hip        : k_matched, k_dm_history, k_fm, k_fm_prep
//   bpsk_tail.hip      : k_tail, k_tail8, k_sync*, k_reset_maxcorr*, k_pack_slots, k_snapshot_pack (this file)
// Each unit that reads the tables has its own copy of them (bpsk_units.h); this one reads all three (ds_taps and dm_taps in
// tail_exact_sample, sync in k_sync / k_sync_t), and bpsk_upload_constants() at its end fills every unit's.
//
// Pipeline per batch of L input samples x S streams (all on one HIP stream):
//   host        : input-independent schedules (tuner / VCO table indices per sample) in exact double,
//                 cached while the phase state repeats (it is an exact 8-cycle at 12 kHz / 96 kHz) -- bpsk_handle.hip
//   k_front*    : int16 -> float -> double, tuner mix, 27-tap low-pass at the decimated instants
//                 (newest-first order, :479-483), x HOWARD_FUDGE_FACTOR, VCO mix  -> dm[s][64+j]
//                 (k_fm: fused with the matched filter, the default for int16 input with a periodic tuner schedule;
//                 k_front_reg: register-staged lane windows; k_front: generic, float input; bpsk_fft.hip /
//                 bpsk_fftm.hip: FFT-acquire mode)
//   k_matched   : 65-tap matched filter in RING-SLOT order with rotated taps (:519-523) -> y[s][j]=(fi,fq)
//   k_tail      : bit-energy IIRs, peak tracking, differential slicer (:534-593) -> bits
//   k_sync      : 65-symbol sync correlation at stride 80 over the 5200-bit window (:556-560)
//   k_sync_fin  : trigger ordering, dmCorr / dmMaxCorr bookkeeping (:567-572)
//   k_fec_bpsk  : FECDecode of every triggered window (fec.hip)
// DESIGN.md has the lane/LDS mapping of each kernel and its roofline.
//
// The handle and the C ABI are in the host units of bpsk_handle.h, which see the four units through bpsk_kernels.h: the
// argument structs and the launch_* functions at the end of each unit.
#include "bpsk_units.h"
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

namespace jsdr {

namespace tail { __constant__ BpskConst c_bpsk; }  // this unit's copy of the tables, under this unit's name (bpsk_units.h)
using tail::c_bpsk;

// ------------------------------------------------------------------------------------------- k_tail
// One wave per stream, the 9600 Hz tail (:534-593) in chunks of 64 bit periods (512 samples).
// The bit clock is input independent and exactly periodic (bitPos == g mod 8, a new peak is measured
// after every g == 7 mod 8; verified on the host at create time).  The only truly serial arithmetic is
// the nine first-order IIRs (eight dmEnergy channels :535, dmEnergyOut :538); everything else is taken
// out of their loop:
//   parallel : coalesced load of the chunk (prefetched one chunk ahead), energy1 = fi*fi+fq*fq     (:534)
//   serial   : 64 steps; lanes 0..7 advance dmEnergy[lane], lane 8 advances dmEnergyOut SPECULATING that
//              the peak position stays where it is (decision point = bitPos v in every period)
//   parallel : lane = period: first-maximum argmax of the eight energies after that period (:586-592)
//   check    : if every new peak equals v the speculation held (the steady state of a locked demodulator):
//              decision points are (period, v).  Otherwise (rare: acquisition, fades) the chunk is replayed
//              by the scalar state machine of :537,:577-579 and dmEnergyOut is recomputed from its saved value
//   parallel : lane = decision: differential detector, sqrt, threshold, bit (:539-545), ordered compaction

// (fi,fq) of the 9600 Hz sample g in EXACT order, by the whole wave, from the call's raw input: the 65 VCO-mixed samples
// g-64..g (27-tap low-pass each, :479-483, one per lane) through LDS, then the 65 products in ring-slot order (:519-523).
// The cold path of the fast variant: only samples whose 65-sample window lies inside this call (j0 >= 7, checked by the
// caller, keeps every input index >= 0).
__device__ __forceinline__ double2 tail_exact_sample(const TailArgs &a, int s, long long g, double2 *dmL, int lane)
{
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const double HOWARD = 0.9 * 32768.0;
    const bool dc = (a.ic != 0) || (a.qc != 0);
    for (int i = lane; i < 65; i += 64) {
        const long long j = g - 64 + i - a.g_first;  // call-relative index of the decimated sample
        double fi = 0.0, fq = 0.0;
        for (int age = 0; age < 27; age++) {
            const long long n = (long long)a.first_out + (long long)a.decim * j - age;
            double di, dq;
            fm_convert(raw[n], a.ic, a.qc, dc, di, dq);
            if (a.mix) {
                const double2 cs = a.tcs[(int)((n + 26) % a.tper)];
                di = di * cs.x;
                dq = dq * cs.y;
            }
            const double tp = c_bpsk.ds_taps[age];
            fi += di * tp;
            fq += dq * tp;
        }
        const double oi = fi * HOWARD, oq = fq * HOWARD;
        const int kv = a.kvco[j];
        dmL[i] = make_double2(oi * a.sincos[kv], oq * a.sincos[256 + kv]);
    }
    JSDR_WAVE_SYNC();
    const int u = (int)(((g - 64) % 65 + 65) % 65);  // g = s0 + u, s0 the sample in ring slot 0
    const double *f = c_bpsk.dm_taps;
    double yi = 0.0, yq = 0.0;
    for (int i = 0; i <= 64 - u; i++) {  // s0, s0-1, .., g-64: ages u .. 64
        const double2 x = dmL[64 - u - i];
        yi += x.x * f[u + i];
        yq += x.y * f[u + i];
    }
    for (int m = 0; m < u; m++) {        // g, g-1, .., s0+1: ages 0 .. u-1
        const double2 x = dmL[64 - m];
        yi += x.x * f[m];
        yq += x.y * f[m];
    }
    JSDR_WAVE_SYNC();
    return make_double2(yi, yq);
}

#ifdef JSDR_X_T8CLK  // timing experiment: s_memtime ticks per phase, summed over every wave of every launch
__device__ unsigned long long g_t8_clk[8];
#define T8_CLK(i)                                                     \
    do {                                                              \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        t8acc_[i] += now_ - t8last_;                                  \
        t8last_ = now_;                                               \
    } while (0)
#else
#define T8_CLK(i) do {} while (0)
#endif
// CERT = the fast variant's tail: the same arithmetic on (fi,fq) that carry a bounded error |d| <= ey, plus, for every
// data-dependent decision, a margin that covers the worst case of that error (DESIGN.md "fast variant"):
//   argmax of the eight smoothed energies (:586-592): certified when the winner leads by more than twice the bound on
//     an energy's error; otherwise the stream is marked uncertified (the IIR state cannot be redone locally)
//   energy2 > 100 (:544) and di < 0 (:545): when inside the margin, the two (fi,fq) samples of the detector are
//     recomputed from the raw input in exact order and the decision is taken on those
template <bool CERT>
__global__ __launch_bounds__(64) void k_tail(TailArgs a)
{
    // (fi,fq) of the chunk's 64 samples at the bit position the peak tracker holds when the chunk starts -- the
    // differential detector's inputs while the demodulator is locked; a decision anywhere else (acquisition, a moving
    // peak) reads its sample from y.  The whole chunk (8 KB) used to sit here: with 10 KB instead of 17 KB a CU holds
    // sixteen of these one-wave workgroups instead of nine, and the kernel is occupancy x latency bound.
    __shared__ double2 ydL[64];        // [period]
    // The exact kernel serves handles of fewer than 2048 streams since round 4 (k_tail8 takes the others): a wave per SIMD at
    // most, so LDS no longer decides how many of these workgroups a CU holds -- the whole chunk's (fi,fq) stay here for the
    // decisions that fall on another bit position (acquisition, fades, the FFT-acquire mode's frame seams) instead of being
    // read again from y (two dependent L2 round trips per chunk: with the serial state machine below, 27 us a chunk unlocked
    // against 3 us locked).  The fast variant's tail (CERT) runs at 8192 streams and keeps the small footprint.
    constexpr bool ALLY = !CERT;
    __shared__ double2 yAll[ALLY ? 512 : 1];
    // The chains' work area, in place and ROW PER CHAIN: before the chain, row c < 8 holds the inputs of dmEnergy[c] --
    // energy1 x 1/200 of the sample at bit position c of every period (the products are taken lane-parallel when the chunk
    // is staged, not by the nine chain lanes one at a time) -- and row 8 energy1 x 1/800 of the sample at position v, for
    // dmEnergyOut; afterwards dmEnergy[c] after every period (a chain has the inputs of its next eight links in registers
    // before it overwrites them).  A chain lane reads and writes ITS row two periods per LDS instruction: the kernel is
    // bound by the number of LDS instructions its twenty waves per CU issue (SQ counters: half of a wave's life spent
    // waiting on lgkmcnt), and one 8-byte access per link in each direction was most of them.  6 KB a workgroup.
    __shared__ __align__(16) double eT[9][72];  // [chain][period]; 72: rows 16-byte aligned, two-way conflicts at worst
    __shared__ unsigned char maskL[64];
    __shared__ short declist[136];
    __shared__ double2 dmL[CERT ? 66 : 1];
    const int lane = threadIdx.x;
    const int s = blockIdx.x;
    if (s >= a.nstreams) return;
#ifdef JSDR_X_T8CLK
    unsigned long long t8acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t8last_ = __builtin_amdgcn_s_memtime();
#endif
    TailState *sp = &a.st[s];
    double emax = CERT ? sp->emax : 0.0;
    long long last_g = CERT ? sp->last_g : -1;
    int uncert = 0;
    long long redone = 0;
    const double2 *y = a.y + (long long)s * a.y_stride;
    signed char *blog = a.bitlog_new + (long long)s * a.bitlog_stride;
    const int nbits_prev = sp->nbits_prev;
    const int cntBit0 = sp->cntBit;
    // carry the 5200-bit shift register (dmFECCorr, :503) over from the previous call's log
    {
        // (the source is byte aligned only; 82 byte loads per lane, in two batches kept in flight together -- a
        // load / wait / store loop would pay the memory latency 82 times before the first chunk starts)
        const signed char *old = a.bitlog_old + (long long)s * a.bitlog_stride + nbits_prev;
        constexpr int NQ = (HIST_BITS + 63) / 64, HALF = (NQ + 1) / 2;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            signed char t[HALF];
#pragma unroll
            for (int q = 0; q < HALF; q++) {
                const int i = lane + 64 * (h * HALF + q);
                t[q] = old[i < HIST_BITS ? i : HIST_BITS - 1];
            }
#pragma unroll
            for (int q = 0; q < HALF; q++) {
                const int i = lane + 64 * (h * HALF + q);
                if (i < HIST_BITS) blog[i] = t[q];
            }
        }
    }
    const double K1 = 1.0 - 1.0 / 200.0, S1 = 1.0 / 200.0;  // BIT_SMOOTH1 (:89)
    const double K2 = 1.0 - 1.0 / 800.0, S2 = 1.0 / 800.0;  // BIT_SMOOTH2 (:90)
    // lanes 0..7 carry dmEnergy[lane], lane 8 carries dmEnergyOut
    double e = (lane < 8) ? sp->dmEnergy[lane] : sp->dmEnergyOut;
    const double Kc = (lane < 8) ? K1 : K2;
    int peakPos = __builtin_amdgcn_readfirstlane(sp->peakPos);
    int newPeak = __builtin_amdgcn_readfirstlane(sp->newPeak);
    double lastI = sp->lastI, lastQ = sp->lastQ, energy1 = sp->energy1, energy2 = sp->energy2;
    int nbits = 0;
    const long long g_first = a.g_first, g_end = a.g_first + a.nds;
    const long long M_first = g_first >> 3, M_last = (g_end - 1) >> 3;

    double2 pre[8];
    auto fetch = [&](long long MB) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            long long g = 8 * MB + k * 64 + lane;
            pre[k] = (g >= g_first && g < g_end) ? y[g - g_first] : make_double2(0.0, 0.0);
        }
    };
    if (a.nds > 0) fetch(M_first);

    for (long long MB = M_first; MB <= M_last && a.nds > 0; MB += 64) {
        // ---------------- stage the prefetched chunk, start fetching the next one
        const int v = peakPos;
#pragma unroll
        for (int k = 0; k < 8; k++) {  // sample k*64 + lane = period k*8 + lane/8, position lane%8
            const double en = pre[k].x * pre[k].x + pre[k].y * pre[k].y;  // :534
            if constexpr (ALLY) yAll[k * 64 + lane] = pre[k];
            eT[lane & 7][k * 8 + (lane >> 3)] = en * S1;
            if ((lane & 7) == v) {
                ydL[k * 8 + (lane >> 3)] = pre[k];
                eT[8][k * 8 + (lane >> 3)] = en * S2;
            }
        }
        JSDR_WAVE_SYNC();
        const double2 *ychunk = y + (8 * MB - g_first);  // sample i of the chunk (only in-range samples are ever decisions)
        auto ysample = [&](int pos) {
            if constexpr (ALLY) return yAll[pos];
            else return (pos & 7) == v ? ydL[pos >> 3] : ychunk[pos];
        };
        double m_en = 0.0, m_d = 0.0, m_e2 = 0.0;  // this chunk's margins
        if constexpr (CERT) {
            double em = 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const double en = pre[k].x * pre[k].x + pre[k].y * pre[k].y;
                em = en > em ? en : em;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double o = __shfl_xor(em, off, 64);
                em = o > em ? o : em;
            }
            emax = em > emax ? em : emax;
            // |fi|,|fq| <= sqrt(emax); u = 2^-53.  energy1: 2 sqrt2 sqrt(emax) ey + 7 u emax; through the IIR (gain 1, 3
            // roundings a link, 1/(1-K) = 200 links deep): + 1200 u emax.  di, dq: 4 sqrt(emax) ey + 7 u emax.
            // (all linear in the input: the full-scale bound ey shrinks with the stream's largest sample so far)
            const double sq = sqrt(emax), U = 1.1102230246251565e-16;
            const double eys = a.ey * ((double)__int_as_float(a.amax[s]) * (1.0000001 / 32767.0));
            m_en = a.argmax_scale * 2.0 * (2.83 * sq * eys + 2.0 * eys * eys + 1207.0 * U * emax);
            m_d = a.margin_scale * (4.1 * sq * eys + 2.0 * eys * eys + 7.0 * U * emax);
            m_e2 = 1.5 * m_d + (m_d > 0.0 ? 4.0e-14 : 0.0);
        }
        if (MB + 64 <= M_last) fetch(MB + 64);
        const int nper = (int)((M_last - MB + 1) < 64 ? (M_last - MB + 1) : 64);
        const bool interior = (8 * MB >= g_first) && (8 * (MB + 64) <= g_end);  // every sample of all 64 periods is in range (uniform)
        T8_CLK(0);  // staging
        // ---------------- serial IIRs, speculating that the peak position stays at v
        const bool spec = (newPeak == peakPos);
        const double e_in = e;
        {
            const int idx = (lane < 8) ? lane : v;
            const int col = (lane < 8) ? lane : 8;
            const long long glane = 8 * MB + idx;
            const bool lane_iir = lane < 8, lane_out = (lane == 8) && spec;
            const bool lane_on = lane_iir || lane_out;
            // the 64 energies this lane will fold in, fetched up front: the serial chain below then touches
            // registers only (an LDS read per step would put ~100 cycles of latency on every link of the chain)
#ifndef JSDR_TAIL_XS
#define JSDR_TAIL_XS 8
#endif
            // (a few at a time: the preload is 16 VGPRs instead of 128 -- at 8192 streams the tail is occupancy x latency
            //  bound, and what counts is how many of these one-wave workgroups a CU holds)
            constexpr int XS = JSDR_TAIL_XS;
            const int pfirst = (glane < g_first) ? 1 : 0;  // period 0 of the chunk lacks this lane's sample
#pragma unroll
            for (int p0 = 0; p0 < 64; p0 += XS) {
                double xs[XS];
#pragma unroll
                for (int p = 0; p < XS; p += 2) {  // (the x S products were taken at staging)
                    const double2 x2 = *reinterpret_cast<const double2 *>(&eT[col][p0 + p]);
                    xs[p] = x2.x;
                    xs[p + 1] = x2.y;
                }
                // (pinned: left to itself the compiler sinks the reads back into the chain, one LDS wait per two steps)
#pragma unroll
                for (int p = 0; p < XS; p++) asm volatile("" : "+v"(xs[p]));
                // only the first and the last period of a call can be partial; everywhere else, with the peak position
                // settled (the locked demodulator), a link of the chain is one multiply and one add.  The energies go to
                // LDS as they fall out (stores are not on the chain; a register copy of all 64 would double the kernel's
                // footprint beside the kernels it overlaps with).
                if (interior && spec) {
                    // lanes 0..8 only, under ONE exec mask for the whole chain (a mask per store costs an exec write and
                    // its hazard on every link); lane 8 (dmEnergyOut) stores into the rows' pad column, which nobody reads
                    if (lane <= 8) {
#pragma unroll
                        for (int p = 0; p < XS; p += 2) {
                            const double e0 = (e * Kc) + xs[p];  // :535 / :538
                            e = (e0 * Kc) + xs[p + 1];
                            *reinterpret_cast<double2 *>(&eT[lane][p0 + p]) = make_double2(e0, e);
                        }
                    }
                } else {
#pragma unroll
                    for (int p = 0; p < XS; p++) {
                        const double ne = (e * Kc) + xs[p];
                        const bool ok = lane_on && (p0 + p >= pfirst) && (glane + 8 * (p0 + p) < g_end);
                        if (ok) e = ne;
                        if (lane_iir) eT[lane][p0 + p] = e;
                    }
                }
            }
        }
        JSDR_WAVE_SYNC();
        T8_CLK(1);  // chains
        // ---------------- new peak after every period whose last sample (bitPos 7) is in range (:582-593)
        int np = -1;
        if (lane < nper) {
            const long long g7 = 8 * (MB + lane) + 7;
            if (g7 >= g_first && g7 < g_end) {
                // eMax starts at -1.0e10F and only a slot ABOVE it takes dmNewPeak (:586-592): a NaN slot is passed over, and with
                // all eight NaN no slot is taken -- np = -2, dmNewPeak keeps its value.  (Energies are never below 0: on finite
                // input slot 0 always takes the first step, and the runner-up sv is a real energy from slot 1 on.)
                double bv = (double)-1.0e10F, sv = -1.0e300;
                np = -2;
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    double ov = eT[c][lane];
                    if (ov > bv) {  // strict: the first maximum wins
                        sv = bv;
                        bv = ov;
                        np = c;
                    } else if (CERT && ov > sv) {
                        sv = ov;
                    }
                }
                if constexpr (CERT) {
                    // (m_en == 0: nothing but zeros has gone through the fast kernels, both variants hold the same numbers)
                    if (!(bv - sv > m_en) && m_en > 0.0) uncert = 1;  // the order of the two largest is not certain
                }
            }
        }
        // A period that took no slot keeps the dmNewPeak it entered with: the peak of the nearest measured period below it that took
        // one, or the carried newPeak where there is none.  One ballot finds whether any lane has such a period (none on finite
        // input); a second one, taken only then, gives every lane the lanes that did take a slot, whatever the pattern.  From here
        // on np is what dmNewPeak holds after the period, as everything below reads it.
        {
            const unsigned long long kept = __ballot(np == -2);
            if (kept) {
                const unsigned long long below = __ballot(np >= 0) & ((1ull << lane) - 1ull);
                const int src = below ? 63 - __clzll((long long)below) : 0;
                const int from = __shfl(np, src, 64);
                if (np == -2) np = below ? from : newPeak;
            }
        }
        T8_CLK(2);  // argmax
        bool replay = false;
        const bool bad = (np >= 0) && (np != v);
        const bool held = spec && (__ballot(bad) == 0ull);
        // A locked stream away from the call's edges: every period has its one decision at bit position v, in period
        // order -- the decision list is known without the mask / prefix-sum / list round trips through LDS.
        const bool fastd = held && interior;
        int nd = 64;
        if (!fastd) {
            if (held) {
                if (lane < nper) {
                    const long long g = 8 * (MB + lane) + v;
                    maskL[lane] = (g >= g_first && g < g_end) ? (unsigned char)(1 << v) : (unsigned char)0;
                }
                // peakPos stays v; every measured peak was v, so newPeak stays v as well
            } else {
                // The peak moved (acquisition, fades, frame seams of the FFT-acquire mode).  The peakPos/newPeak
                // machine of :537,:577-579,:592 is integer only -- its inputs are the per-period argmax values np,
                // which do not depend on dmEnergyOut -- so it runs as scalar code over the periods, one mask per
                // period; dmEnergyOut is then redone from its saved value along the decision list further down.
                // Walking the bit positions cfirst..clast of a period: a decision where c == peakPos (:537); at c ==
                // (peakPos+4)&7 peakPos = newPeak (dmHalfTable, :500,:577-578), after which a second decision can fall at the NEW
                // peakPos if that position is still to come.  In closed form (k_tail8's; branch-free, scalar).
                // Away from the call's edges every period is whole and measured, and then the machine is not serial at all:
                // whenever peakPos != newPeak the switch position (peakPos+4)&7 lies inside the period, so peakPos leaves every
                // period equal to the newPeak it entered with, which is the peak measured one period earlier --
                //     newPeak(p) = np[p-1],  peakPos(p) = np[p-2]   (the chunk's first two periods take the carried state)
                // and each lane writes down its own period's decisions (the scalar walk over 64 periods was most of the 27 us an
                // unlocked chunk took, against 3 us for a locked one).
                int mymask_r = 0;
                if (interior) {
                    const int up1 = __shfl_up(np, 1, 64), up2 = __shfl_up(np, 2, 64);
                    const int nwv = lane == 0 ? newPeak : up1;
                    const int pkv = lane == 0 ? peakPos : (lane == 1 ? newPeak : up2);
                    const int h = (pkv + 4) & 7;
                    const bool diff = pkv != nwv;
                    const bool d1 = !(diff && h < pkv);
                    const bool d2 = diff && nwv > h;
                    mymask_r = (d1 ? 1 << pkv : 0) | (d2 ? 1 << nwv : 0);
                    peakPos = __builtin_amdgcn_readlane(np, 62);
                    newPeak = __builtin_amdgcn_readlane(np, 63);
                } else
                for (int p = 0; p < nper; p++) {
                    const long long gbase = 8 * (MB + p);
                    const int cfirst = (gbase < g_first) ? (int)(g_first - gbase) : 0;
                    const int clast = (gbase + 7 >= g_end) ? (int)(g_end - 1 - gbase) : 7;
                    const int h = (peakPos + 4) & 7;
                    const bool pin = peakPos >= cfirst && peakPos <= clast;
                    const bool hin = h >= cfirst && h <= clast && peakPos != newPeak;
                    const bool d1 = pin && !(hin && h < peakPos);  // the old peakPos decides unless the switch came first
                    const bool d2 = hin && newPeak > h && newPeak <= clast;
                    const int mask = (d1 ? 1 << peakPos : 0) | (d2 ? 1 << newPeak : 0);
                    peakPos = hin ? newPeak : peakPos;
                    if (lane == p) mymask_r = mask;
                    if (clast == 7) newPeak = __builtin_amdgcn_readlane(np, p);
                }
                if (lane < 64) maskL[lane] = (unsigned char)mymask_r;
                replay = true;
            }
            JSDR_WAVE_SYNC();
            // ---------------- decision list of the chunk, in time order
            const int mymask = (lane < nper) ? (int)maskL[lane] : 0;
            const int mycnt = __popc(mymask);
            // inclusive prefix sum over lanes: a period holds at most two decisions, so two ballots count them (six dependent
            // cross-lane adds before)
            const unsigned long long b1 = __ballot(mycnt >= 1), b2 = __ballot(mycnt >= 2);
            const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
            const int pre_sum = __popcll(b1 & upto) + __popcll(b2 & upto);
            nd = __popcll(b1) + __popcll(b2);
            {
                int pos = pre_sum - mycnt;
                int m = mymask;
                while (m) {
                    int c = __ffs(m) - 1;
                    m &= m - 1;
                    declist[pos++] = (short)(lane * 8 + c);
                }
            }
            JSDR_WAVE_SYNC();
            if (replay) {
                // dmEnergyOut (:538) over the decisions in time order: the products x*S2 lane-parallel, the chain
                // e = e*K2 + (x*S2) on broadcast values, in the reference's operation order
                double xa = 0.0, xb = 0.0;
                auto en_of = [&](int pos) {  // energy1 of the chunk's sample pos, as :534 forms it
                    const double2 q = ysample(pos);
                    return q.x * q.x + q.y * q.y;
                };
                if (lane < nd) xa = en_of(declist[lane]) * S2;
                if (lane + 64 < nd) xb = en_of(declist[lane + 64]) * S2;
                double eo = __shfl(e_in, 8, 64);
                // (lane indices as constants, sixteen links per uniform test: as a counted loop every link paid the hazards
                //  of a lane select in an SGPR and a branch)
                auto chain = [&](double xs, int cnt) {
#pragma unroll 1
                    for (int d0 = 0; d0 < 64; d0 += 16) {
                        if (d0 >= cnt) break;
#pragma unroll
                        for (int u = 0; u < 16; u++) {
                            const int lo = __builtin_amdgcn_readlane(__double2loint(xs), u);
                            const int hi = __builtin_amdgcn_readlane(__double2hiint(xs), u);
                            const double ne = (eo * K2) + __hiloint2double(hi, lo);
                            eo = (d0 + u < cnt) ? ne : eo;
                        }
                        // the next sixteen inputs move down to lanes 0..15
                        xs = __hiloint2double(__shfl_down(__double2hiint(xs), 16, 64), __shfl_down(__double2loint(xs), 16, 64));
                    }
                };
                chain(xa, nd < 64 ? nd : 64);
                if (nd > 64) chain(xb, nd - 64);
                if (lane == 8) e = eo;
            }
        }
        T8_CLK(3);  // machine, list, replay
        // ---------------- parallel: differential detector per decision (:539-545)
        for (int d0 = 0; d0 < nd; d0 += 64) {
            const int d = d0 + lane;
            const bool have = d < nd;
            double2 cur = make_double2(0.0, 0.0), prv = make_double2(lastI, lastQ);
            if (have) {
                cur = fastd ? ydL[d] : ysample((int)declist[d]);
                if (d > 0) prv = fastd ? ydL[d - 1] : ysample((int)declist[d - 1]);
            }
            double di = -((prv.x * cur.x) + (prv.y * cur.y));
            double dq = (prv.x * cur.y) - (prv.y * cur.x);
            double e2 = sqrt((di * di) + (dq * dq));
            if constexpr (CERT) {
                const bool unsure = have && (fabs(e2 - 100.0) <= m_e2 || (e2 > 100.0 && fabs(di) <= m_d));
                unsigned long long um = __ballot(unsure);
                if (um) {  // cold: redo those decisions on (fi,fq) recomputed from the raw input in exact order
                    const int ci = have ? (fastd ? 8 * d + v : (int)declist[d]) : 0;
                    const int pi = (have && d > 0) ? (fastd ? 8 * (d - 1) + v : (int)declist[d - 1]) : -1;
                    while (um) {
                        const int L = __ffsll((long long)um) - 1;
                        um &= um - 1ull;
                        const long long gc = 8 * MB + __shfl(ci, L, 64);
                        const int pl = __shfl(pi, L, 64);
                        const long long gp = pl >= 0 ? 8 * MB + pl : last_g;
                        // both windows (65 VCO-mixed samples of 27 inputs each) must lie inside this call
                        const bool can = gp >= 0 && gp - 64 - a.g_first >= 7 && gc - 64 - a.g_first >= 7 && gc < a.g_first + a.nds &&
                                         (a.mix == 0 || a.tper > 0);
                        if (!can) {
                            // (the first samples of a call reach back into the previous one) not recomputable: the decision
                            // stands if it clears the margin proper -- margin_scale only widens what is sent to the redo
                            const double e2L = __shfl(e2, L, 64), diL = __shfl(di, L, 64);
                            if (fabs(e2L - 100.0) <= m_e2 / a.margin_scale || (e2L > 100.0 && fabs(diL) <= m_d / a.margin_scale)) uncert = 1;
                            continue;
                        }
                        // (one inlined instance in a two-trip loop: a call would put the kernel on the function-call ABI --
                        //  256 VGPRs, a stack, one wave per SIMD)
                        double2 ec = make_double2(0.0, 0.0), ep = make_double2(0.0, 0.0);
#pragma unroll 1
                        for (int which = 0; which < 2; which++) {
                            const double2 r = tail_exact_sample(a, s, which ? gp : gc, dmL, lane);
                            if (which) ep = r; else ec = r;
                        }
                        if (lane == L) {
                            di = -((ep.x * ec.x) + (ep.y * ec.y));
                            dq = (ep.x * ec.y) - (ep.y * ec.x);
                            e2 = sqrt((di * di) + (dq * dq));
                        }
                        redone++;
                    }
                }
            }
            const bool valid = have && (e2 > 100.0);
            const unsigned long long vm = __ballot(valid);
            if (valid) {
                int rank = __popcll(vm & ((1ull << lane) - 1ull));
                int pos = nbits + rank;
                if (pos < a.max_bits) blog[HIST_BITS + pos] = (di < 0.0) ? (signed char)1 : (signed char)-1;
            }
            nbits += __popcll(vm);
            // the last decision of the chunk defines dmLastIQ / energy2 for what follows
            const int lastd = nd - 1 - d0;
            if (lastd >= 0 && lastd < 64) {
                energy2 = __shfl(e2, lastd, 64);
                lastI = __shfl(cur.x, lastd, 64);
                lastQ = __shfl(cur.y, lastd, 64);
                if constexpr (CERT) {
                    const int li = have ? (fastd ? 8 * d + v : (int)declist[d]) : 0;
                    last_g = 8 * MB + __shfl(li, lastd, 64);
                }
            }
        }
        JSDR_WAVE_SYNC();
    }
#ifdef JSDR_X_T8CLK
    T8_CLK(4);  // detector (of the last chunk; the others' land on "staging")
    if (lane == 0)
        for (int i = 0; i < 6; i++) atomicAdd(&g_t8_clk[i], t8acc_[i]);
#endif
    // energy1 = that of the last sample processed (:534)
    if (a.nds > 0) {
        const double2 q = y[a.nds - 1];
        energy1 = q.x * q.x + q.y * q.y;
    }
    // ---------------- write back
    const bool any_uncert = CERT && (__ballot(uncert != 0) != 0ull);
    const double e8 = __shfl(e, 8, 64);
    if (lane < 8) sp->dmEnergy[lane] = e;
    if (lane == 0) {
        sp->dmEnergyOut = e8;
        sp->lastI = lastI;
        sp->lastQ = lastQ;
        sp->energy1 = energy1;
        sp->energy2 = energy2;
        sp->peakPos = peakPos;
        sp->newPeak = newPeak;
        const int nb = nbits < a.max_bits ? nbits : a.max_bits;
        sp->cntBit = cntBit0 + nb;
        sp->nbits_prev = nb;
        if (nbits > a.max_bits) sp->overflow = 1;
        a.nbits[s] = nb;
        if constexpr (CERT) {
            sp->emax = emax;
            sp->last_g = last_g;
            sp->redone += redone;
            if (any_uncert) sp->uncertified = 1;
        }
    }
}

// ------------------------------------------------------------------------------------------- k_tail8
// The exact-order tail (:534-593) with EIGHT STREAMS PER WAVE: lane = 8 x (stream of the wave) + bit position.  k_tail
// (one wave per stream) keeps nine of its 64 lanes busy while the nine IIR chains run and moves every energy through
// LDS twice to get it to a chain lane and back; here the eight dmEnergy chains of eight streams ARE the 64 lanes, and a
// lane reads the samples of its own bit position straight from y (the eight lanes of a stream read 128 contiguous
// bytes per period) -- no transposition on the way in.  Per chunk of CH bit periods:
//   A  every lane: energy1 (:534), its dmEnergy link (:535) and -- speculating that its position is the peak -- a
//      dmEnergyOut link (:538); the chain values go to an LDS image for the argmax, the (fi,fq) of the lanes that sit on
//      the peak position to a small LDS list; the next chunk's samples are requested as this chunk's are consumed
//   B  lane = (stream, period): first-maximum argmax of the eight energies after the period (:586-592)
//   fast path (every stream of the wave locked: peakPos == newPeak == every measured peak): the decisions are (period,
//      peakPos); lane = (stream, decision): differential detector, threshold, bit (:539-545), ordered compaction
//   general path (acquisition, fades, the frame seams of the FFT-acquire mode): the peakPos / newPeak machine (:537,
//      :577-579,:592) in closed form per period (at most two decisions fall into one period), lane-replicated per stream;
//      the decision samples re-read from y (L2), dmEnergyOut re-run over them in time order, the detector lane-parallel
//      over the 2 CH decision slots -- no per-stream scalar loop, the eight streams of the wave go through it together
// energy2 = sqrt(di^2+dq^2) > 100 (:543-544) is decided as di^2+dq^2 > 10000: sqrt is correctly rounded and monotone,
// sqrt(10000) = 100 exactly and sqrt(nextafter(10000)) = 100 + 9.1e-15 rounds to the double above 100
// (tests/test_host_logic.py checks the neighbourhood); the square root itself is taken once, for the state the call leaves.
template <int CH, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_tail8(TailArgs a)
{
#ifdef JSDR_X_T8CLK
    unsigned long long t8acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t8last_ = __builtin_amdgcn_s_memtime();
#endif
    static_assert(CH == 16, "two decision slots per period in one 64-bit mask, one nibble per period in another");
    constexpr int ROW = 82;  // doubles per period of the energy image: 8 streams x 10 (8 used) + 2 -> conflict-free b128 reads
    __shared__ __align__(16) double EoL_[WPB][CH * ROW];
    __shared__ __align__(16) double2 FQL_[WPB][8][CH];
    __shared__ __align__(16) unsigned char NPL_[WPB][8][CH];
    // (WPB waves per workgroup, each on its own: a workgroup of four puts one wave on every SIMD of a CU, so that the four
    //  take the registers ONE workgroup of the kernel they run beside leaves free -- four one-wave workgroups land on four CUs)
    const int wv = WPB > 1 ? (int)(threadIdx.x >> 6) : 0, wblk = (int)blockIdx.x * WPB + wv;
    double *EoL = EoL_[wv];
    double2 (*FQL)[CH] = FQL_[wv];
    unsigned char (*NPL)[CH] = NPL_[wv];
    double *X2L = EoL;                                               // general path, once the argmax has read the image:
    double2 *CURL = reinterpret_cast<double2 *>(EoL + 8 * 2 * CH);   // [8][2 CH] each
    static_assert(8 * 2 * CH * 3 <= CH * ROW, "work areas fit the dead energy image");
    const int lane = threadIdx.x & 63, s8 = lane >> 3, c = lane & 7;
    const int S = a.nstreams;
    const int sraw = wblk * 8 + s8;
    const bool live = sraw < S;
    const int s = live ? sraw : S - 1;  // (surplus lanes of the last wave shadow its last stream and store nothing)
    TailState *sp = &a.st[s];
    const int nds = (int)a.nds;
    const long long g_first = a.g_first;
    // ---- carry the 5200-bit shift register (dmFECCorr, :503) over from the previous call's log: the whole wave per stream,
    // dwords (the rows are 16-byte aligned, the source starts at any byte)
    for (int t = 0; t < 8; t++) {
        const int st = wblk * 8 + t;
        if (st >= S) break;
        const int nprev = __builtin_amdgcn_readfirstlane(a.st[st].nbits_prev);
        const signed char *old = a.bitlog_old + (long long)st * a.bitlog_stride + nprev;
        const int sh = (int)(reinterpret_cast<unsigned long long>(old) & 3ull);
        const unsigned *ow = reinterpret_cast<const unsigned *>(old - sh);
        unsigned *nw32 = reinterpret_cast<unsigned *>(a.bitlog_new + (long long)st * a.bitlog_stride);
        constexpr int NW = HIST_BITS / 4, NIT = (NW + 63) / 64;
        unsigned lo[NIT], hi[NIT];
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            const int i = lane + 64 * q;
            const int ic = i < NW ? i : NW - 1;
            lo[q] = ow[ic];
            hi[q] = ow[ic + 1];
        }
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            const int i = lane + 64 * q;
            if (i < NW) nw32[i] = __builtin_amdgcn_alignbyte(hi[q], lo[q], (unsigned)sh);
        }
    }
    const double K1 = 1.0 - 1.0 / 200.0, S1 = 1.0 / 200.0;  // BIT_SMOOTH1 (:89)
    const double K2 = 1.0 - 1.0 / 800.0, S2 = 1.0 / 800.0;  // BIT_SMOOTH2 (:90)
    double e = sp->dmEnergy[c];
    double eo = sp->dmEnergyOut;
    int pk = sp->peakPos, nw = sp->newPeak;
    double lastI = sp->lastI, lastQ = sp->lastQ;
    const int cntBit0 = sp->cntBit;
    int nbits = 0;
    int ord_last = -1;    // this lane's latest decision (ordinal within the call) and its di^2 + dq^2: the stream's last one
    double x_last = 0.0;  // gives energy2 (:543)
    const long long M_first = g_first >> 3, M_last = (g_first + nds - 1) >> 3;
    const double2 *ys = a.y + (long long)s * a.y_stride;
    signed char *blog = a.bitlog_new + (long long)s * a.bitlog_stride;
    int rel0 = (int)(8 * M_first - g_first);  // call-relative index of the chunk's sample 0 (-7 .. 0 for the first chunk)
    // (reads before sample 0 and past the last one stay inside the buffers' slack, Y_PAD; what they return is never used)
    // The call's first period may start and its last may end anywhere (range masks, uniform over the streams).  One code path:
    // with the masks under a branch -- or two sample buffers picked by a branch -- the compiler reconciles the register
    // assignment of the requests in flight where the paths meet, with copies behind an s_waitcnt vmcnt(0): the whole memory
    // latency per chunk (3.0 ms at 8192 streams where the reads alone take 2.2).
    // (the state is due HERE, before the first requests go out: a loop-carried value that is still on its way at the loop's
    //  entry makes the compiler wait for it -- and for everything requested before it -- in EVERY iteration)
    asm volatile("" : "+v"(e), "+v"(eo), "+v"(lastI), "+v"(lastQ), "+v"(pk), "+v"(nw));
    double2 F[CH];
    if (nds > 0) {
        const double2 *p0 = ys + (rel0 + c);
#pragma unroll
        for (int p = 0; p < CH; p++) F[p] = p0[8 * p];
    }
    T8_CLK(0);  // shift register, state, first requests
    for (long long MB = M_first; MB <= M_last && nds > 0; MB += CH, rel0 += 8 * CH) {
        const int v = pk;
        const bool mine = c == v;
        double eo_l = eo;
        const double2 *pn = ys + (rel0 + 8 * CH + c);
        // ---------------- A: the chains; a sample's register is asked for the next chunk's as soon as it has been read
#pragma unroll
        for (int p = 0; p < CH; p++) {
            const double2 f = F[p];
            const double en = (f.x * f.x) + (f.y * f.y);  // :534
            if (mine) FQL[s8][p] = f;
            double x1 = en * S1, x2 = en * S2;
            asm volatile("" : "+v"(x1), "+v"(x2));  // (due HERE: nothing of the sample may be needed below the request)
            // (the sample's last use lies ABOVE the request that overwrites it: scheduled the other way round -- the scheduler's
            //  preference -- the new sample needs registers of its own and comes home through copies behind an s_waitcnt
            //  vmcnt(0) at the loop's back edge: the whole memory latency per chunk)
            __builtin_amdgcn_sched_barrier(0);
#ifndef JSDR_X_T8_NOLOAD  // (timing probe: the first chunk's samples over and over -- the kernel without its HBM reads)
            F[p] = pn[8 * p];
#endif
            __builtin_amdgcn_sched_barrier(0);
            const double ne = (e * K1) + x1;       // :535
            const double no = (eo_l * K2) + x2;    // :538, were this lane's position the peak
            const bool inr = (unsigned)(rel0 + 8 * p + c) < (unsigned)nds;
            e = inr ? ne : e;
            eo_l = inr ? no : eo_l;
            EoL[p * ROW + s8 * 10 + c] = e;
        }
        JSDR_WAVE_SYNC();
        T8_CLK(1);  // A
#ifdef JSDR_X_T8_LOADONLY  // (timing probe: the reads and the chains only)
        if (nds > 0) continue;
#endif
        // ---------------- B: new peak after every period whose last sample is in range (:582-593); lane = (stream, period)
        bool fail = pk != nw;
#pragma unroll
        for (int i = 0; i < CH / 8; i++) {
            const int p = 8 * i + c;
            const double2 *row = reinterpret_cast<const double2 *>(&EoL[p * ROW + s8 * 10]);
            const double2 q0 = row[0], q1 = row[1], q2 = row[2], q3 = row[3];
            // eMax starts at -1.0e10F and only a slot ABOVE it takes dmNewPeak (:586): a NaN slot is passed over, and with all
            // eight NaN none is taken -- np stays 8, which the machine below already reads as "dmNewPeak keeps its value"
            double bv = (double)-1.0e10F;
            int np = 8;
            if (q0.x > bv) { bv = q0.x; np = 0; }
            if (q0.y > bv) { bv = q0.y; np = 1; }  // strict: the first maximum wins
            if (q1.x > bv) { bv = q1.x; np = 2; }
            if (q1.y > bv) { bv = q1.y; np = 3; }
            if (q2.x > bv) { bv = q2.x; np = 4; }
            if (q2.y > bv) { bv = q2.y; np = 5; }
            if (q3.x > bv) { bv = q3.x; np = 6; }
            if (q3.y > bv) { bv = q3.y; np = 7; }
            const bool meas = rel0 + 8 * p + 7 < nds;
            np = meas ? np : 8;
            NPL[s8][p] = (unsigned char)np;
            fail = fail || (np < 8 && np != v);  // (a period that took no slot leaves a locked stream locked: newPeak == v stays)
        }
        const bool general = __ballot(fail) != 0ull;
        JSDR_WAVE_SYNC();
        T8_CLK(2);  // B
        const int ord0 = 2 * (int)(MB - M_first) * 1;  // ordinal of the chunk's slot 0 (two slots per period)
        if (!general) {
            // ---------------- locked: one decision per period, at bit position v
            eo = __shfl(eo_l, 8 * s8 + v, 64);
#pragma unroll
            for (int i = 0; i < CH / 8; i++) {
                const int p = 8 * i + c;
                const int drel = rel0 + 8 * p + v;
                const bool inr = drel >= 0 && drel < nds;
                const double2 cur = FQL[s8][p];
                const double2 pv = FQL[s8][p > 0 ? p - 1 : 0];
                const bool from_state = p == 0 || drel < 8;  // the decision before this one fell into an earlier chunk or call
                const double pI = from_state ? lastI : pv.x, pQ = from_state ? lastQ : pv.y;
                const double di = -((pI * cur.x) + (pQ * cur.y));  // :539
                const double dq = (pI * cur.y) - (pQ * cur.x);     // :540
                const double x = (di * di) + (dq * dq);
                const bool valid = inr && x > 10000.0;             // energy2 > 100 (:544)
                const unsigned vm = (unsigned)(__ballot(valid) >> (8 * s8)) & 0xffu;
                if (valid && live) {
                    const int pos = nbits + __popc(vm & ((1u << c) - 1u));
                    if (pos < a.max_bits) blog[HIST_BITS + pos] = (di < 0.0) ? (signed char)1 : (signed char)-1;  // :545
                }
                nbits += __popc(vm);
                if (inr) {
                    ord_last = ord0 + 2 * p;
                    x_last = x;
                }
            }
            {   // dmLastIQ (:541-542) = the chunk's last decision sample
                int plast = (nds - 1 - rel0 - v) >> 3;  // (arithmetic shift: floor)
                plast = plast < CH - 1 ? plast : CH - 1;
                const int pfirst = rel0 + v >= 0 ? 0 : 1;
                const double2 l = FQL[s8][plast > 0 ? plast : 0];
                if (plast >= pfirst) {
                    lastI = l.x;
                    lastQ = l.y;
                }
            }
            T8_CLK(3);  // locked
        } else {
            // ---------------- general: the peakPos / newPeak machine per period, in closed form.  Walking the bit positions
            // cf..cl of a period (:537,:577-579): a decision where c == peakPos; at c == (peakPos+4)&7 peakPos = newPeak, after
            // which a second decision can fall at the NEW peakPos if that position is still to come.
            unsigned long long smask = 0ull;  // bit 2p+k: decision slot k of period p is taken
            unsigned long long pos1 = 0ull, pos2 = 0ull;  // nibble p: the bit position of slot 0 / slot 1
            {
                const uint4 n4 = *reinterpret_cast<const uint4 *>(&NPL[s8][0]);
#pragma unroll
                for (int p = 0; p < CH; p++) {
                    const unsigned w = p < 4 ? n4.x : (p < 8 ? n4.y : (p < 12 ? n4.z : n4.w));
                    const int np = (int)((w >> (8 * (p & 3))) & 0xffu);
                    int cf = -(rel0 + 8 * p), cl = nds - 1 - (rel0 + 8 * p);
                    cf = cf < 0 ? 0 : cf;    // first / last bit position of the period that belongs to the call
                    cl = cl > 7 ? 7 : cl;    // (cl < cf: none of it does)
                    const int h = (pk + 4) & 7;
                    const bool pin = pk >= cf && pk <= cl;
                    const bool hin = h >= cf && h <= cl && pk != nw;
                    // the old peakPos decides unless the switch came first (h < peakPos and h inside the period)
                    const bool d1 = pin && !(hin && h < pk);
                    const bool d2 = hin && nw > h && nw <= cl;
                    if (d1) {
                        smask |= 1ull << (2 * p);
                        pos1 |= (unsigned long long)pk << (4 * p);
                    }
                    if (d2) {
                        smask |= 1ull << (2 * p + 1);
                        pos2 |= (unsigned long long)nw << (4 * p);
                    }
                    pk = hin ? nw : pk;
                    nw = np < 8 ? np : nw;  // :592
                }
            }
            // the decision samples, lane = (stream, slot); dmEnergyOut's inputs and the samples themselves go to LDS
            double2 cur[2 * CH / 8];
            bool has[2 * CH / 8];
#pragma unroll
            for (int r = 0; r < 2 * CH / 8; r++) {
                const int slot = 8 * r + c, p = slot >> 1;
                has[r] = ((smask >> slot) & 1ull) != 0ull;
                const int cpos = (int)((((slot & 1) ? pos2 : pos1) >> (4 * p)) & 15ull);
                const int rel = has[r] ? rel0 + 8 * p + cpos : 0;
                cur[r] = ys[rel];
            }
#pragma unroll
            for (int r = 0; r < 2 * CH / 8; r++) {
                const int slot = 8 * r + c;
                const double en = (cur[r].x * cur[r].x) + (cur[r].y * cur[r].y);
                X2L[s8 * 2 * CH + slot] = en * S2;
                CURL[s8 * 2 * CH + slot] = cur[r];
            }
            JSDR_WAVE_SYNC();
            // dmEnergyOut (:538) over the decisions in time order (lane-replicated per stream)
            {
                const double2 *x2 = reinterpret_cast<const double2 *>(&X2L[s8 * 2 * CH]);
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const double2 xx = x2[q];
                    const double n0 = (eo * K2) + xx.x;
                    eo = ((smask >> (2 * q)) & 1ull) ? n0 : eo;
                    const double n1 = (eo * K2) + xx.y;
                    eo = ((smask >> (2 * q + 1)) & 1ull) ? n1 : eo;
                }
            }
            // detector per slot; the previous decision is the nearest taken slot below (or the state)
#pragma unroll
            for (int r = 0; r < 2 * CH / 8; r++) {
                const int slot = 8 * r + c;
                const unsigned long long below = smask & ((1ull << slot) - 1ull);
                const int prev = below ? 63 - __clzll((long long)below) : 0;
                const double2 pv = CURL[s8 * 2 * CH + prev];
                const double pI = below ? pv.x : lastI, pQ = below ? pv.y : lastQ;
                const double di = -((pI * cur[r].x) + (pQ * cur[r].y));
                const double dq = (pI * cur[r].y) - (pQ * cur[r].x);
                const double x = (di * di) + (dq * dq);
                const bool valid = has[r] && x > 10000.0;
                const unsigned vm = (unsigned)(__ballot(valid) >> (8 * s8)) & 0xffu;
                if (valid && live) {
                    const int pos = nbits + __popc(vm & ((1u << c) - 1u));
                    if (pos < a.max_bits) blog[HIST_BITS + pos] = (di < 0.0) ? (signed char)1 : (signed char)-1;
                }
                nbits += __popc(vm);
                if (has[r]) {
                    ord_last = ord0 + slot;
                    x_last = x;
                }
            }
            if (smask) {
                const double2 l = CURL[s8 * 2 * CH + (63 - __clzll((long long)smask))];
                lastI = l.x;
                lastQ = l.y;
            }
            T8_CLK(4);  // general
        }
        JSDR_WAVE_SYNC();
    }
    // ---------------- what the call leaves
    double energy1 = sp->energy1, energy2 = sp->energy2;
    if (nds > 0) {
        const double2 q = ys[nds - 1];
        energy1 = (q.x * q.x) + (q.y * q.y);  // that of the last sample processed (:534)
    }
    {   // energy2 (:543) of the stream's last decision: the lane of the stream that holds the highest ordinal
        int o = ord_last;
        double x = x_last;
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            const int oo = __shfl_xor(o, off, 64);
            const double xo = __shfl_xor(x, off, 64);
            if (oo > o) {
                o = oo;
                x = xo;
            }
        }
        if (o >= 0) energy2 = sqrt(x);
    }
    if (live) {
        sp->dmEnergy[c] = e;
        if (c == 0) {
            sp->dmEnergyOut = eo;
            sp->lastI = lastI;
            sp->lastQ = lastQ;
            sp->energy1 = energy1;
            sp->energy2 = energy2;
            sp->peakPos = pk;
            sp->newPeak = nw;
            const int nb = nbits < a.max_bits ? nbits : a.max_bits;
            sp->cntBit = cntBit0 + nb;
            sp->nbits_prev = nb;
            if (nbits > a.max_bits) sp->overflow = 1;
            a.nbits[s] = nb;
        }
    }
#ifdef JSDR_X_T8CLK
    T8_CLK(5);  // write-back
    if (lane == 0)
        for (int i = 0; i < 6; i++) atomicAdd(&g_t8_clk[i], t8acc_[i]);
#endif
}

// ------------------------------------------------------------------------------------------- k_sync
// sync-vector correlation for every new bit (:556-559): window = the 5200 most recent bits, 65 taps at
// stride 80.  corr[b] kept (int8) for the dmMaxCorr bookkeeping; hits (>=45, :560) go to a per-stream list.
__global__ void k_sync(SyncArgs a)
{
    const int s = blockIdx.y;
    const int nb = a.nbits[s];
    const signed char *bl = a.bitlog + (long long)s * a.bitlog_stride;
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += gridDim.x * blockDim.x) {
        const signed char *w = bl + b + 1;  // dmFECCorr after shifting bit b in
        int c = 0;
#pragma unroll 5
        for (int n = 0; n < SYNC_N; n++) c += (int)w[n * 80] * (int)c_bpsk.sync[n];
        a.corr[(long long)s * a.max_bits + b] = (signed char)c;
    }
}

// k_sync_t: the same correlations from a TRANSPOSED image of the stream's bit log in LDS.  Window p of output b is
// W[b + 80 n], W[p] = bitlog[1 + p]: with T[p mod 80][p div 80] = W[p] the 65 bytes of an output are CONTIGUOUS in row
// b mod 80 from column b div 80 -- eighteen aligned dword reads, a byte alignment and seventeen v_dot4_i32_i8 against
// the packed sync vector instead of 65 strided byte loads and 65 multiply-adds (integer arithmetic: same sums).  One
// workgroup per stream; the row stride is 4 * odd so that the rows of 32 consecutive outputs fall on 32 different banks.
// Its first wave then orders the hits and leaves dmCorr / dmMaxCorr (sync_fin_wave below; a kernel of its own until
// round 3: one dependent launch less per call): the workgroup's correlations are read back from global memory behind a
// device-scope release / acquire pair around the barrier.
__device__ __forceinline__ void sync_fin_wave(int s, int lane, int nb, const signed char *c, int *trig_count, int *trig_bits,
                                              int trig_cap, TailState *st);
__global__ __launch_bounds__(256) void k_sync_t(SyncArgs a, int row_stride, SyncFinArgs f)
{
    extern __shared__ __align__(16) unsigned char smem[];
    signed char *T = reinterpret_cast<signed char *>(smem);  // [80][row_stride]
    const int s = blockIdx.x;
    const int nb = a.nbits[s];
    if (nb <= 0) {  // no new bit: no hit, dmCorr / dmMaxCorr stay (what sync_fin_wave does with nb = 0)
        if (f.fuse && threadIdx.x == 0) f.trig_count[s] = 0;
        return;
    }
    const int np = HIST_BITS - 1 + nb;  // W[0 .. np), W = the stream's log from byte 1: the last window ends at W[nb-1 + 80*64]
    {
        // the log comes in as 16-byte loads, eight per thread in flight (the rows are 16-byte aligned; W[p] is byte p + 1 of
        // the row): as a byte-at-a-time loop every one of its 120 iterations waited for its own load
        const uint4 *row16 = reinterpret_cast<const uint4 *>(a.bitlog + (long long)s * a.bitlog_stride);
        const int n16 = (np + 1 + 15) / 16;
        for (int i0 = 0; i0 < n16; i0 += 256 * 8) {
            uint4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int i = i0 + 256 * u + (int)threadIdx.x;
                v[u] = row16[i < n16 ? i : n16 - 1];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int i = i0 + 256 * u + (int)threadIdx.x;
                if (i < n16) {
                    const int p0 = 16 * i - 1;  // W index of the quad's first byte
                    int r = (p0 + 80) % 80, q = (p0 + 80) / 80 - 1;
                    const unsigned w4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                    for (int b = 0; b < 16; b++) {
                        const int p = p0 + b;
                        if (p >= 0 && p < np) T[r * row_stride + q] = (signed char)((w4[b >> 2] >> (8 * (b & 3))) & 0xffu);
                        r += 1;
                        if (r >= 80) {
                            r = 0;
                            q += 1;
                        }
                    }
                }
            }
        }
    }
    // packed sync vector: bytes 4i .. 4i+3 (zero beyond 64)
    int S4[17];
#pragma unroll
    for (int i = 0; i < 17; i++) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (4 * i + k < SYNC_N) v |= ((int)c_bpsk.sync[4 * i + k] & 0xff) << (8 * k);
        S4[i] = v;
    }
    __syncthreads();
    {
        int b = threadIdx.x, r = b % 80, q0 = b / 80;
        for (; b < nb; b += 256) {
            const int *row = reinterpret_cast<const int *>(T + r * row_stride + (q0 & ~3));
            const int sh = q0 & 3;
            int d[18];
#pragma unroll
            for (int i = 0; i < 18; i++) d[i] = row[i];
            int c = 0;
#pragma unroll
            for (int i = 0; i < 17; i++) {
                const int w = (int)__builtin_amdgcn_alignbyte((unsigned)d[i + 1], (unsigned)d[i], (unsigned)sh);
                c = __builtin_amdgcn_sdot4(w, S4[i], c, false);
            }
            a.corr[(long long)s * a.max_bits + b] = (signed char)c;
            r += 256 % 80;
            q0 += 256 / 80;
            if (r >= 80) {
                r -= 80;
                q0 += 1;
            }
        }
    }
    if (!f.fuse) return;  // (uniform)
    __threadfence();  // release: every wave's correlations are visible device-wide ...
    __syncthreads();
    if (threadIdx.x < 64) {
        __threadfence();  // ... acquire: and read from there, not from a stale L1 line
        sync_fin_wave(s, (int)threadIdx.x, nb, a.corr + (long long)s * a.max_bits, f.trig_count, f.trig_bits, f.trig_cap, f.st);
    }
}

// the hits (correlation >= 45, :560) in bit order -- one wave per stream walks the correlations 64 at a time, a ballot
// and a prefix count give every hit its slot: deterministic, and when a call holds more hits than the handle has room
// for it is the FIRST trig_cap that are kept (the stream is flagged; the getters then fail instead of returning a
// truncated result).  Then dmCorr / dmMaxCorr exactly as the serial loop leaves them (:556-572): after a hit dmMaxCorr
// restarts from 0 (:567) and immediately takes that bit's correlation (:571-572).
__device__ __forceinline__ void sync_fin_wave(int s, int lane, int nb, const signed char *c, int *trig_count, int *trig_bits,
                                              int trig_cap, TailState *st)
{
    int nt = 0, last_hit = -1;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + lane;
        const bool hit = b < nb && (int)c[b] >= 45;
        const unsigned long long m = __ballot(hit);
        if (hit) {
            const int slot = nt + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < trig_cap) trig_bits[s * trig_cap + slot] = b;
        }
        if (m) last_hit = b0 + 63 - __clzll(m);
        nt += __popcll(m);
    }
    int from = 0, best = st[s].dmMaxCorr;
    if (nt > 0) {
        from = last_hit;
        best = 0;
    }
    for (int b = from + lane; b < nb; b += 64) best = best > (int)c[b] ? best : (int)c[b];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        int o = __shfl_xor(best, off, 64);
        best = best > o ? best : o;
    }
    if (lane == 0) {
        if (nb > 0) st[s].dmCorr = c[nb - 1];
        st[s].dmMaxCorr = best;
        st[s].cntFEC += nt;  // the reference counts every hit (:566), decoded or not
        if (nt > trig_cap) {
            st[s].overflow = 1;
            nt = trig_cap;
        }
        trig_count[s] = nt;
    }
}

// after the strided k_sync (the fallback for calls whose bit log does not fit a workgroup's LDS); k_sync_t does this itself
__global__ __launch_bounds__(64) void k_sync_fin(const int *nbits, const signed char *corr, int max_bits, int *trig_count,
                                                 int *trig_bits, int trig_cap, TailState *st, int nstreams)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= nstreams) return;
    sync_fin_wave(s, lane, nbits[s], corr + (long long)s * max_bits, trig_count, trig_bits, trig_cap, st);
}


// slot = int32 header[16] | int8 bits[slot_bits] | trig_cap x {int32 rc, int32 bit_index, uint8 data[256]}
// header: nbits, nfec, cntRaw, cntDS, cntBit, cntFEC, cntDec, dmErrBits, dmCorr, dmMaxCorr, decodeOK, overflow (a stream
// that overflowed its per-call bit / FEC capacity: its slot is incomplete), uncertified (fast variant: a decision of this
// stream could not be certified), 0...
__global__ void k_pack_slots(unsigned char *slots, long long slot_bytes, int slot_bits, int trig_cap, const TailState *st,
                             const int *nbits, const signed char *bitlog, long long bitlog_stride, const int *trig_count,
                             const int *trig_bits, const int *fec_rc, const unsigned char *fec_data, const int *fec_last,
                             const int *cnt_dec, int n_in, int n_ds)
{
    const int s = blockIdx.x;
    unsigned char *slot = slots + (long long)s * slot_bytes;
    int *hdr = reinterpret_cast<int *>(slot);
    const int nb = nbits[s], nt = trig_count[s];
    if (threadIdx.x < 16) {
        int v = 0;
        switch (threadIdx.x) {
            case 0: v = nb; break;
            case 1: v = nt; break;
            case 2: v = n_in; break;
            case 3: v = n_ds; break;
            case 4: v = st[s].cntBit; break;
            case 5: v = st[s].cntFEC; break;
            case 6: v = cnt_dec[s]; break;
            case 7: v = fec_last[2 * s]; break;
            case 8: v = st[s].dmCorr; break;
            case 9: v = st[s].dmMaxCorr; break;
            case 10: v = fec_last[2 * s + 1]; break;
            case 11: v = st[s].overflow; break;
            case 12: v = st[s].uncertified; break;
            default: v = 0;
        }
        hdr[threadIdx.x] = v;
    }
    const signed char *bl = bitlog + (long long)s * bitlog_stride + HIST_BITS;
    for (int i = threadIdx.x; i < slot_bits; i += blockDim.x) slot[64 + i] = (i < nb) ? (unsigned char)bl[i] : 0;
    unsigned char *f = slot + 64 + slot_bits;
    for (int t = 0; t < trig_cap; t++) {
        int *fh = reinterpret_cast<int *>(f + t * 264);
        if (threadIdx.x == 0) {
            fh[0] = (t < nt) ? fec_rc[s * trig_cap + t] : 0;
            fh[1] = (t < nt) ? trig_bits[s * trig_cap + t] + 1 : 0;
        }
        for (int i = threadIdx.x; i < 256; i += blockDim.x)
            f[t * 264 + 8 + i] = (t < nt) ? fec_data[((long long)s * trig_cap + t) * 256 + i] : 0;
    }
}

// jsdr_bpsk_set_tuning / _set_mode: dmMaxCorr = 0 (:189) in every stream
__global__ void k_reset_maxcorr(TailState *st, int nstreams)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nstreams) st[s].dmMaxCorr = 0;
}
}  // namespace jsdr

using namespace jsdr;

// ---- the 1-stream receive() forms publish their results for a concurrent reader (jsdr_bpsk_snapshot_read).  What the
// four getters behind the snapshot fetch with eleven small blocking copies (each a round trip to the device: ~130 us of
// a 290 us receive) is packed by ONE tiny kernel at the end of the side stream's work and comes back in ONE copy.
// (C linkage: the symbol profiles and traces have always shown)
extern "C" __global__ void k_snapshot_pack(SnapPack *out, const TailState *st, const int *fec_last, const int *cnt_dec, const int *nbits,
                                const FftFrontState *fs, const unsigned char *decoded, const signed char *bits_new)
{
    const int i = threadIdx.x;
    if (i == 0) {
        out->t = st[0];
        out->last[0] = fec_last[0];
        out->last[1] = fec_last[1];
        out->cdec = cnt_dec[0];
        out->nbits = nbits[0];
        out->centreBin = fs ? fs[0].centreBin : 0;
        out->pad = 0;
        out->avePeakPower = fs ? fs[0].avePeakPower : 0.0;
        out->aveCentreBin = fs ? fs[0].aveCentreBin : 0.0;
    }
    if (i < 256) out->decoded[i] = decoded[i];
    const int nb = nbits[0];
    for (int k = i; k < 512; k += blockDim.x) out->bits[k] = k < nb ? bits_new[k] : (signed char)0;
}

// actionPerformed on channel `ch` (-1: every channel) of a channel handle, after the handle's pending work: tuning (and
// tuPhaseInc, :189) and / or doUp, and dmMaxCorr = 0 (:190) in the streams of those channels on every input.  tuPhase and
// every other piece of state carry on; the other channels are not touched.  The one step that can fail comes first.
__global__ void k_reset_maxcorr_chan(TailState *st, int nin, int nch, int ch)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nin * nch && (ch < 0 || s % nch == ch)) st[s].dmMaxCorr = 0;
}

// =============================================================================================== launchers
// What the handle's call (bpsk_call.hip) starts (bpsk_kernels.h): the grid, the LDS and the template choice of each kernel.
namespace jsdr {

// every unit's copy of the tables (bpsk_units.h)
int bpsk_upload_constants(const BpskConst &bc)
{
    if (bpsk_front_upload_constants(bc) != JSDR_OK || bpsk_fm_upload_constants(bc) != JSDR_OK || bpsk_fm_f32_upload_constants(bc) != JSDR_OK) return JSDR_ERR;
    JSDR_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_bpsk), &bc, sizeof(bc)));
    return JSDR_OK;
}

// cert: the fast variant's margin-certified tail (k_tail<true>); otherwise k_tail8 from 2048 streams, k_tail below
const char *launch_tail(const TailArgs &ta, bool cert, hipStream_t ts)
{
    const int S = ta.nstreams;
    static const bool use_tail8 = [] {
        const char *e = knob("JSDR_TAIL8");  // JSDR_TAIL8=0: the one-wave-per-stream tail (A/B timing)
        return !e || atoi(e) != 0;
    }();
    static const bool force_tail8 = [] {
        const char *e = knob("JSDR_TAIL8");  // JSDR_TAIL8=2: k_tail8 whatever the number of streams (the tests' small handles)
        return e && atoi(e) == 2;
    }();
    const char *name = "k_tail";
    if (cert)
        hipLaunchKernelGGL(k_tail<true>, dim3((unsigned)S), dim3(64), 0, ts, ta);
    else if (use_tail8 && (S >= 2048 || force_tail8))
        // (below ~2000 streams there are too few waves of eight streams to fill the chip and a wave's own latency per chunk
        //  decides: 1024 streams, FFT-acquire lines of round 4: locked 0.64 ms (k_tail) against 1.6, unlocked 5.6 against 3.5)
    {
        static const int wpb = [] {
            const char *e = knob("JSDR_TAIL8_WPB");  // JSDR_TAIL8_WPB=1: one-wave workgroups (A/B timing)
            return e ? atoi(e) : 4;
        }();
        const unsigned waves = (unsigned)((S + 7) / 8);
        if (wpb == 1)
            hipLaunchKernelGGL((k_tail8<16, 1>), dim3(waves), dim3(64), 0, ts, ta);
        else
            hipLaunchKernelGGL((k_tail8<16, 4>), dim3((waves + 3) / 4), dim3(256), 0, ts, ta);
        name = "k_tail8";
    }
    else
        hipLaunchKernelGGL(k_tail<false>, dim3((unsigned)S), dim3(64), 0, ts, ta);
    JSDR_LAUNCH_CHECK_NAMED();
    return name;
}

// k_sync_t's row stride (bytes, 4 * odd) and LDS for a handle whose calls slice at most max_bits bits
static size_t sync_t_lds(int max_bits, int *row_stride)
{
    int cols = (HIST_BITS + max_bits + 79) / 80 + 72;  // + the 18 dwords an output reads past its first column
    int rs = (cols + 3) & ~3;
    if (((rs / 4) & 1) == 0) rs += 4;  // 4 * odd
    *row_stride = rs;
    return (size_t)80 * rs + 16;
}

// transposed-image kernel when the stream's log fits a workgroup's LDS (always, up to ~8M samples a call)
bool sync_t_applies(int max_bits)
{
    static const bool use_t = [] {
        const char *e = knob("JSDR_SYNC_T");  // JSDR_SYNC_T=0: the strided kernel
        return !e || atoi(e) != 0;
    }();
    int rs = 0;
    return use_t && sync_t_lds(max_bits, &rs) <= 150 * 1024;
}

int launch_sync_t(const SyncArgs &sa, const SyncFinArgs &sf, int nstreams, hipStream_t st)
{
    int rs = 0;
    const size_t lds = sync_t_lds(sa.max_bits, &rs);
    JSDR_LDS_ATTR(k_sync_t, lds);
    hipLaunchKernelGGL(k_sync_t, dim3((unsigned)nstreams), dim3(256), lds, st, sa, rs, sf);
    return launched();
}

int launch_sync(const SyncArgs &sa, long long nds, int nstreams, hipStream_t st)
{
    int gx = (sa.max_bits + 255) / 256;
    long long maxnew = nds / 4 + 8;
    if ((long long)gx * 256 > maxnew + 255) gx = (int)((maxnew + 255) / 256);
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_sync, dim3((unsigned)gx, (unsigned)nstreams), dim3(256), 0, st, sa);
    return launched();
}

int launch_sync_fin(const SyncArgs &sa, const SyncFinArgs &sf, int nstreams, hipStream_t st)
{
    hipLaunchKernelGGL(k_sync_fin, dim3((unsigned)nstreams), dim3(64), 0, st, sa.nbits, sa.corr, sa.max_bits, sf.trig_count, sf.trig_bits,
                       sf.trig_cap, sf.st, nstreams);
    return launched();
}

int launch_reset_maxcorr(TailState *st, int nstreams, hipStream_t stream)
{
    hipLaunchKernelGGL(k_reset_maxcorr, dim3((unsigned)((nstreams + 255) / 256)), dim3(256), 0, stream, st, nstreams);  // :190
    return launched();
}

int launch_reset_maxcorr_chan(TailState *st, int nin, int nch, int ch, hipStream_t stream)
{
    hipLaunchKernelGGL(k_reset_maxcorr_chan, dim3((unsigned)((nin * nch + 255) / 256)), dim3(256), 0, stream, st, nin, nch, ch);
    return launched();
}

int launch_snapshot_pack(SnapPack *out, const TailState *st, const int *fec_last, const int *cnt_dec, const int *nbits,
                         const FftFrontState *fs, const unsigned char *decoded, const signed char *bits_new, hipStream_t stream)
{
    hipLaunchKernelGGL(k_snapshot_pack, dim3(1), dim3(256), 0, stream, out, st, fec_last, cnt_dec, nbits, fs, decoded, bits_new);
    return launched();
}

int launch_pack_slots(unsigned char *slots, long long slot_bytes, int slot_bits, int trig_cap, const TailState *st, const int *nbits,
                      const signed char *bitlog, long long bitlog_stride, const int *trig_count, const int *trig_bits, const int *fec_rc,
                      const unsigned char *fec_data, const int *fec_last, const int *cnt_dec, int n_in, int n_ds, int nstreams, hipStream_t stream)
{
    hipLaunchKernelGGL(k_pack_slots, dim3((unsigned)nstreams), dim3(256), 0, stream, slots, slot_bytes, slot_bits, trig_cap, st, nbits, bitlog,
                       bitlog_stride, trig_count, trig_bits, fec_rc, fec_data, fec_last, cnt_dec, n_in, n_ds);
    return launched();
}

void bpsk_debug_clocks_report()
{
#ifdef JSDR_X_T8CLK
    {
        unsigned long long cc[8] = {0};
        if (hipMemcpyFromSymbol(cc, HIP_SYMBOL(g_t8_clk), sizeof(cc)) == hipSuccess) {
            static const char *nm[6] = {"prologue", "A chains", "B argmax", "locked", "general", "write-back"};
            unsigned long long tot = 0;
            for (int i = 0; i < 6; i++) tot += cc[i];
            for (int i = 0; i < 6; i++) fprintf(stderr, "k_tail8 clk %-12s %14llu ticks %5.1f%%\n", nm[i], cc[i], 100.0 * cc[i] / (tot ? tot : 1));
            memset(cc, 0, sizeof(cc));
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_t8_clk), cc, sizeof(cc));
        }
    }
#endif
    bpsk_fm_clocks_report();
}

}  // namespace jsdr
