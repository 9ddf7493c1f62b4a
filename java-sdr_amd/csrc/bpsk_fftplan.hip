// bpsk_fftplan.hip -- the FFT-acquire plan (bpsk_fftplan.h): front-end selection, radices, twiddle tables, pass arguments.
// Host code only, no HIP runtime call.  Compiled with -ffp-contract=off like its neighbours.
#include "bpsk_fftplan.h"
#include <math.h>
#include <stdlib.h>

namespace jsdr {

// ------------------------------------------------------------------------------------------- radices and tables
int fft_radices(int n, int *rad)
{
    int c = 0;
    if (n < 2) return 0;
    // (the oracle's choice for frames above 9600 samples: the transform splits into two independent halves, bpsk_fft2x.hip)
    if (n > FM_NMAX && n % 2 == 0) {
        rad[c++] = 2;
        n /= 2;
    }
    while (n % 4 == 0 && c < FFT_MAXPASS) {
        rad[c++] = 4;
        n /= 4;
    }
    if (n % 2 == 0 && c < FFT_MAXPASS) {
        rad[c++] = 2;
        n /= 2;
    }
    for (int p = 3; p <= 7; p += 2)
        while (n % p == 0 && c < FFT_MAXPASS) {
            rad[c++] = p;
            n /= p;
        }
    for (int p = 11; n > 1 && c < FFT_MAXPASS; p += 2) {
        if (p * p > n) p = n;
        while (n % p == 0 && c < FFT_MAXPASS) {
            rad[c++] = p;
            n /= p;
        }
    }
    return n == 1 ? c : 0;
}

void fft_table(double2 *t, int len)
{
    for (int m = 0; m < len; m++) {
        const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)len;
        t[m] = make_double2((double)cosl(ang), (double)(-sinl(ang)));
    }
    t[0] = make_double2(1.0, -0.0);
    if (len % 4 == 0) {
        t[len / 4] = make_double2(0.0, -1.0);
        t[3 * len / 4] = make_double2(-0.0, 1.0);
    }
    if (len % 2 == 0) t[len / 2] = make_double2(-1.0, -0.0);
}

// Ts[half-1+j] = W_n^(j*n/(2*half)), j < half, half = 1,2,..,n/2 (n-1 entries), every value taken from the SAME table as
// oracle/o_fft.c jo_fft_twiddles_f64 builds (long double + one rounding, exact on the axes)
void fft_twiddles_f64(std::vector<double2> &w, int n)
{
    std::vector<double2> base((size_t)n / 2);
    for (int k = 0; k < n / 2; k++) {
        long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
        base[k] = make_double2((double)cosl(ang), (double)(-sinl(ang)));
    }
    base[0] = make_double2(1.0, -0.0);
    if (n >= 4) base[n / 4] = make_double2(0.0, -1.0);
    w.assign((size_t)n, make_double2(0.0, 0.0));
    for (int half = 1; half < n; half <<= 1) {
        const int step = n / (2 * half);
        for (int j = 0; j < half; j++) w[(size_t)half - 1 + j] = base[(size_t)j * step];
    }
}

// ------------------------------------------------------------------------------------------- which front end
static bool has_prime_radix(int n)
{
    int rad[FFT_MAXPASS];
    const int np = fft_radices(n, rad);
    return np > 0 && rad[np - 1] > 7;  // (they come last)
}

size_t fftm_scratch(int n) { return has_prime_radix(n) ? (size_t)n : 0; }

bool fftm_supported(int n)
{
    int rad[FFT_MAXPASS];
    // the band arithmetic (:429-443: beg = n/4 or 0, end = n/2 or n/4 in Java's integer division, a 100-wide window and 75
    // bins of margin either side) needs n/4 > 150; the image must fit the LDS.  Round 4: any such n = 2^a 3^b 5^c 7^d -- n need
    // not be a multiple of 16 (the 16-byte boxcar reads are aligned relative to the band's own start), so the 4410-sample
    // frame of a 44.1 kHz sound card is in
    // Round 5: any prime factor (a pass of that radix as the DFT's definition: 11.025 kHz gives n = 1102 = 2 19 29), and frames
    // down to 416 samples (8 kHz gives 800): below n = 604 the boxcar range [beg+75, end-75) is empty -- as in the reference,
    // whose loop (:433) then never runs -- and the 204 gathered bins (centreBin <= n/2 - 1) still end inside the frame.
    if (n < 416 || n > FM_NMAX || (n & (n - 1)) == 0) return false;
    const int np = fft_radices(n, rad);
    return np > 0 && np <= FM_MAXPASS;
}

// frames of n = 2 m samples with m an LDS-sized mixed-radix frame (n = 19200: m = 9600)
// (the halves' passes are the blocked ones of the 2^a 3^b 5^c frames: m a multiple of 16 without a factor 7)
bool fft2x_supported(int n)
{
    const int m = n / 2;
    return n > FM_NMAX && (n % 2) == 0 && (m % 16) == 0 && (m % 7) != 0 && fftm_supported(m);
}

bool acqm_supported(int n) { return n == 9600 || n == 4800 || n == 4410; }

bool acqg_supported(int n)
{
    // below 416 samples the 204 gathered bins do not end inside the frame (the reference's own arraycopy would throw); the image
    // index arithmetic of the kernels is 32-bit within a frame
    if (n < 416 || n > (1 << 22)) return false;
    if ((n & (n - 1)) == 0) return true;
    int rad[FFT_MAXPASS];
    const int np = fft_radices(n, rad);
    if (np <= 0) return false;
    // a prime radix r above 7 is a pass of n r complex multiply-adds (one thread per output, r terms each): bounded, so that a frame
    // with a huge prime factor is refused at create instead of occupying the GPU for minutes per call
    for (int p = 0; p < np; p++)
        if (rad[p] > 7 && (long long)n * rad[p] > (1LL << 31)) return false;
    return true;
}

// round 6: a call of two or more 4800- or 4410-sample frames a stream takes them in pairs (k_front_fftm2); JSDR_FFTM_PAIR=0: never
bool fftm_pairs(int n, int nframes)
{
    bool pair = (n == 4800 || n == 4410) && nframes >= 2;
    if (const char *e = knob("JSDR_FFTM_PAIR")) pair = pair && atoi(e) != 0;
    return pair;
}

size_t fft2x_scratch_ek(int n) { return (size_t)(n / 4 + 52); }
// (+16: the aligned 16-byte reads of a window run may end two slots past the last sample)
size_t fft2x_scratch_r0(int n) { return (size_t)(n / 2) + 16; }
// images of a frame in the launch's scratch: a power of two is transformed in place, the Stockham passes go between two
size_t acqg_image_bytes(int n) { return sizeof(double2) * (size_t)n * (((n & (n - 1)) == 0) ? 1 : 2); }

// Which FFT-acquire front end serves a frame of n samples at a decimation of decim.  The power-of-two (1024 .. 8192) and the
// 2 m front ends size their per-thread output lists for a decimation of at least 4; the mixed-radix one (any other frame up
// to 9600 samples) loops and takes any.  Whatever those refuse -- and any other frame the oracle defines -- goes through the
// any-frame passes (bpsk_acqg.hip); FRONT_NONE: no front end takes the frame.
// chan_form (jsdr_bpsk_create_mode_channels): a channel handle has the three-phase front ends only, so every frame that is
// not one of theirs (2^k of 1024 .. 8192 at a decimation of 4 and more, 9600 / 4800 / 4410) takes the any-frame passes' plan.
// force_gen (jsdr_bpsk_create under JSDR_ACQG, tests): 1 the any-frame passes for a frame the LDS kernels take, 0 never them
// -- a frame that no LDS front end takes is then refused, FRONT_NONE (it used to be handed to an LDS front end whose plan it lacks).
FftFront fft_front_kind(int n, int decim, bool chan_form, int force_gen)
{
    const bool pow2 = n >= 1024 && n <= 8192 && (n & (n - 1)) == 0;
    const bool lds = chan_form ? ((pow2 && decim >= 4) || acqm_supported(n)) : (fftm_supported(n) || (decim >= 4 && (pow2 || fft2x_supported(n))));
    if (force_gen >= 0 ? force_gen != 0 : !lds) return acqg_supported(n) ? FRONT_GEN : FRONT_NONE;
    if (!lds) return FRONT_NONE;  // (force_gen == 0 on a frame that only the any-frame passes take)
    return pow2 ? FRONT_POW2 : fft2x_supported(n) ? FRONT_FFT2X : FRONT_FFTM;
}

// ------------------------------------------------------------------------------------------- the plan
// the Stockham passes of an m-point transform: radices, the pass tables back to back, the r-point tables of the prime radices
// above 7 behind every pass table (so the default frames' offsets stay put)
static bool plan_pass_tables(FftPlan &pl, std::vector<double2> &w, int m)
{
    pl.np = fft_radices(m, pl.rad);
    if (pl.np <= 0) return false;
    auto table = [&](int len) {
        const size_t o = w.size();
        w.resize(o + (size_t)len);
        fft_table(w.data() + o, len);
        return (int)o;
    };
    int P = 1;
    for (int p = 0; p < pl.np; p++) {
        pl.tw_off[p] = table(P * pl.rad[p]);
        P *= pl.rad[p];
    }
    for (int p = 0; p < pl.np; p++) pl.wr_off[p] = pl.rad[p] > 7 ? table(pl.rad[p]) : 0;
    return true;
}

bool fft_plan_build_row(FftPlan &pl, std::vector<double2> &w, int n)
{
    pl = FftPlan();
    pl.n = n;
    pl.kind = FRONT_ROW;
    w.clear();
    if (n < 2 || n > FM_NMAX) return false;
    if ((n & (n - 1)) == 0) {
        while ((1 << pl.logn) < n) pl.logn++;
        fft_twiddles_f64(w, n);
        return true;
    }
    if (!plan_pass_tables(pl, w, n)) return false;
    return fft_pass_args(pl.args, pl, 0);  // (every table from L2; more than FM_MAXPASS passes: no plan)
}

bool fft_plan_build(FftPlan &pl, std::vector<double2> &w, int n, FftFront kind)
{
    pl = FftPlan();
    pl.n = n;
    pl.kind = kind;
    w.clear();
    if (kind == FRONT_NONE || (kind == FRONT_FFTM && !fftm_supported(n)) || (kind == FRONT_FFT2X && !fft2x_supported(n)) ||
        (kind == FRONT_GEN && !acqg_supported(n)))
        return false;
    if ((n & (n - 1)) == 0) {
        while ((1 << pl.logn) < n) pl.logn++;
        fft_twiddles_f64(w, n);
        return true;
    }
    const int m = kind == FRONT_FFT2X ? n / 2 : n;  // (the 2 m front end runs the m-point passes on each half)
    if (kind == FRONT_POW2 || !plan_pass_tables(pl, w, m)) return false;
    if (kind == FRONT_GEN) return true;
    if (kind == FRONT_FFT2X) {
        // the c = 1 tables U_p[(j-1) P' + k'] = T_{2 P' r}[(2 k' + 1) j]
        std::vector<double2> t;
        int P = 1;
        for (int p = 0; p < pl.np; p++) {
            const int r = pl.rad[p];
            t.resize((size_t)2 * P * r);
            fft_table(t.data(), 2 * P * r);
            pl.tw1_off[p] = (int)w.size();
            for (int j = 1; j < r; j++)
                for (int k = 0; k < P; k++) w.push_back(t[(size_t)(2 * k + 1) * j]);
            P *= r;
        }
        return fft_pass_args(pl.args, pl, 0);  // (every table from L2)
    }
    if (n == 4800 || n == 4410) {  // (fftm_pairs)
        FftmArgs pair;
        if (!fft_pass_args(pair, pl, FM_LDS_BYTES - fm2_lds_fixed(n), true)) return false;
        pl.lds_tw_pair = pair.lds_tw;
    }
    return fft_pass_args(pl.args, pl, FM_LDS_BYTES - fm_lds_fixed(n));
}

bool fft_pass_args(FftmArgs &aa, const FftPlan &pl, size_t lds_room, bool pair)
{
    if (pl.np < 1 || pl.np > FM_MAXPASS) return false;
    aa = FftmArgs();
    aa.np = pl.np;
    int P = 1;
    for (int p = 0; p < FM_MAXPASS; p++) {
        aa.rad[p] = p < pl.np ? pl.rad[p] : 1;
        aa.tw_off[p] = p < pl.np ? pl.tw_off[p] : 0;
        aa.wr_off[p] = p < pl.np ? pl.wr_off[p] : 0;
        aa.pmagic[p] = (unsigned)(((1ull << 32) + (unsigned)P - 1) / (unsigned)P);  // exact for b < 2^16, P <= 9600
        if (p < pl.np) {
            const size_t len = (size_t)P * aa.rad[p], end = (size_t)aa.tw_off[p] + len;
            if (end == (size_t)aa.lds_tw + len && end * sizeof(double2) <= lds_room) aa.lds_tw = (int)end;  // a prefix
            P *= aa.rad[p];
        }
    }
    // the default frames' kernels address their tables by compile-time offsets (fm_forward, k_front_fftm2); the 2 m front end
    // reads every table from L2 and has no split to agree on
    static const struct {
        int n, np, off[7], lds_tw, lds_tw_pair;
    } dflt[3] = {{9600, 7, {0, 4, 20, 84, 212, 596, 2516}, 596, 0},
                 {4800, 6, {0, 4, 20, 84, 276, 1236}, 1236, 276},
                 {4410, 6, {0, 2, 8, 26, 116, 746}, 5156, 746}};
    const int m = pl.kind == FRONT_FFT2X ? pl.n / 2 : pl.n;
    for (const auto &d : dflt) {
        if (m != d.n) continue;
        if (pl.np != d.np) return false;
        for (int p = 0; p < d.np; p++)
            if (pl.tw_off[p] != d.off[p]) return false;
        if (pl.kind != FRONT_FFT2X && pl.kind != FRONT_ROW && aa.lds_tw != (pair ? d.lds_tw_pair : d.lds_tw)) return false;
    }
    return true;
}

}  // namespace jsdr
