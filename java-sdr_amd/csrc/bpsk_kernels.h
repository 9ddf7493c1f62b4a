// bpsk_kernels.h -- the tune-mode pipeline's kernels (bpsk_front.hip, bpsk_front_reg.hip, bpsk_fm.hip, bpsk_tail.hip) as the
// handle (bpsk_handle.hip) sees them: the argument structs that cross the seam, the geometry constants the handle sizes its
// buffers with, and one launcher per kernel it starts.  The launchers hold each kernel's grid, LDS and template choice (and
// the knobs that pick between kernels).
#pragma once
#include "common.h"
#include "bpsk_fft.h"

namespace jsdr {

enum { DS_N = 27, DM_N = 65, HIST_BITS = 5200, MIN_TRIG = 8, SYNC_N = 65 };
// slack (elements) in front of and behind the (fi,fq) buffers: k_tail8 prefetches whole chunks without range checks
enum { Y_PAD = 1024 };
#ifndef JSDR_FM_NB
#define JSDR_FM_NB 62
#endif
enum { FM_NB = JSDR_FM_NB, FM_NT = 64 + 65 * FM_NB, FM_THREADS = 512, FM_TABLE_SLACK = 128, FM_EDGE = 128 };

struct BpskConst {
    double ds_taps[32];   // [27] used
    double dm_taps[96];   // [65] used, zero beyond (edge steps of the register-blocked loops read past 64)
    signed char sync[72]; // [65] used, +1/-1
};
int bpsk_upload_constants(const BpskConst &bc);  // -> every unit's __constant__ c_bpsk, read by the front, matched, fm, tail and sync kernels

// per-stream demodulator state that depends on the data (FUNcubeBPSKDemod.java:497-503)
struct TailState {
    double dmEnergy[8];
    double dmEnergyOut;
    double lastI, lastQ;
    double energy1, energy2;
    int peakPos, newPeak;
    int dmCorr, dmMaxCorr;
    int cntBit, cntFEC, cntDec, dmErrBits, decodeOK;
    int nbits_prev;  // bits sliced in the previous call (locates the 5200-bit history in the other bitlog)
    int overflow;    // sticky: more sync hits in one call than the handle's capacity (trig_cap), or more bits than max_bits
    int uncertified; // fast variant, sticky: a slicer decision fell inside the error margin and could not be redone exactly
    // fast variant only (k_tail<CERT>)
    double emax;        // running maximum of fi*fi+fq*fq over the life of the stream: scales the error bounds
    long long last_g;   // 9600 Hz index of the sample of the last decision (whose (fi,fq) are lastI, lastQ); -1: none yet
    long long redone;   // decisions recomputed in exact order because they fell inside the margin
};

struct FrontArgs {
    const int *raw;            // int16 pairs as dwords, [S][stride] (null when rawf is used)
    const float2 *rawf;        // alternative input: the float frame of IAudioHandler.receive, [S][stride]
    long long stride_pairs;
    long long nsamples;        // L
    int ic, qc;
    int mix;                   // 0: tuPhase never exceeds 0 (tuning <= 0): samples pass unmixed (:388,:395)
    const unsigned char *ktu;  // [26 + L] tuner table index per sample, 26 history entries first
    const unsigned char *kvco; // [nds]
    const double *sincos;      // cos[256], sin[256]
    const int2 *hist;          // [S][32]: the 26 inputs before this call: DC-corrected int16 pair (.x) or float2 bits
    double2 *dm;               // [S][dm_stride]: 64 history + nds VCO-mixed samples
    long long dm_stride;
    double2 *ds_dbg;           // optional [S][nds] down-sampler outputs (after HOWARD), may be null
    long long nds;
    int first_out;             // input index whose arrival completes output 0 (= D-1-dsCnt0)
    const double2 *tcs;        // k_front_reg<PER>: unwrapped periodic tuner table (see FmArgs), else null
    int tper;
};

// jsdr_bpsk_set_mode, tune -> FFT-acquire (k_seam_hist): the schedule of the 26 samples before the call
struct SeamHist {
    unsigned char khist[26];  // tuner table index of the 26 samples before the call
    unsigned char mhist[26];  // 1: mixed, 0: passed through
};

// jsdr_bpsk_create_live_channels, tune -> FFT-acquire on one channel (k_chan_seam_hist): that channel's 9-bit tuner indices of the
// 26 samples before the call (256: passed through)
struct ChanSeamHist {
    unsigned short k9[26];
};

// k_hist_in: keep the 26 most recent inputs (DC-corrected int16 pair, or the float pair) for the next call
struct HistArgs {
    const int *raw;
    const float2 *rawf;
    long long stride_pairs, nsamples;
    int ic, qc;
    const int2 *hist_old;
    int2 *hist_new;
    int nstreams;
};

struct MatchedArgs {
    const double2 *dm;   // [S][dm_stride], index 64 + (g - g_first)
    long long dm_stride;
    double2 *y;          // [S][y_stride]
    long long y_stride;
    long long nds;
    long long g_first;   // global 9600 Hz index of dm[64] (= samples demodulated before this call)
    long long tile0;     // global index of the first block of tile 0 (== 64 mod 65, <= g_first)
};

struct FmArgs {
    const int *raw;             // int16 pairs as dwords, [S][stride]
    long long stride_pairs;
    int nsamples;               // L
    int ic, qc;
    const int *edges;           // [S][4 * FM_EDGE]: k_fm_edges' images of the stream around sample 0 and around the last sample
    const double2 *tcs;         // unwrapped tuner table: entry e = (cos, sin) for samples n with (n + 26) mod P == e mod P
    int tper;                   // P (1 when the tuner is off)
    const unsigned char *kvco;  // [nds] VCO table index per decimated sample
    const double *sincos;       // cos[256], sin[256]
    const double2 *dmh_old;     // [S][64] the 64 VCO-mixed samples before this call
    double2 *dmh_new;           // [S][64] the last 64 of this call
    double2 *y;                 // [S][y_stride]
    long long y_stride;
    int nds;
    long long g_first;          // global 9600 Hz index of this call's output 0
    long long tile0;            // global index of tile 0's first block (== 64 mod 65, <= g_first)
    int first_out;              // input index whose arrival completes output 0
    int *amax;                  // FAST: [S] running maximum of |int16 sample| per stream, float bits (never reset)
    int ntiles, nstreams;       // work items = ntiles x nstreams, stream-major; the grid strides over them
    int grid_limit;             // > 0: at most that many workgroups, striding over the work items (jsdr_bpsk_set_cu_share)
    unsigned *tickets;          // the handle's tile counter for such a launch, which hands the items out by ticket (k_fm, k_fm_f32; the
                                // launcher zeroes it on the stream, and drops it where every tile has a workgroup); nullptr: none
#ifdef JSDR_X_WGCLK
    int wgclk_slot;             // timing probe: the launch's row of the per-workgroup start / end ticks
#endif
    int trot;                   // >= 0: tper == 8 and entry e of tcs is phase e + trot of the 8-phase tuner, whose exact factors k_fm
                                // has a form for (Schedule::trot, bpsk_tuner.h); -1: any other table, the generic form
};

// k_fm_prep: the stream's edge images for k_fm ...
struct EdgeArgs {
    const int *raw;
    long long stride_pairs;
    int nsamples, ic, qc, dc;
    const int2 *hist;
    int *edges;
    int nstreams;
};
// ... and, in the receive() form, the schedule's tables from behind the frame to where the kernels read them
struct ScatterArgs {
    const unsigned char *src[2];
    unsigned char *dst[2];
    int bytes[2];
};

// k_fm_f32 (bpsk_fm_f32.hip): k_fm's arguments with the float input and the float edge images (a.raw, a.edges, a.ic, a.qc and
// a.amax are unused)
struct FmF32Args {
    FmArgs a;
    const float2 *rawf;         // the float frames of IAudioHandler.receive, [S][stride]
    const float2 *edges;        // [S][4 * FM_EDGE]: k_fm_prep_f32's images
};
struct EdgeF32Args {
    const float2 *rawf;
    long long stride_pairs;
    int nsamples;
    const int2 *hist;           // [S][32]: the 26 inputs before this call, float pairs' bits
    float2 *edges;
    int nstreams;
};

struct TailArgs {
    const double2 *y;
    long long y_stride;
    long long nds;
    long long g_first;
    TailState *st;
    signed char *bitlog_new;        // [S][stride]: 5200 history + new bits
    const signed char *bitlog_old;
    long long bitlog_stride;
    int *nbits;                     // [S] bits sliced in this call
    int max_bits;
    int nstreams;
    // ---- fast variant (k_tail<true>): what it takes to bound the error of (fi,fq) and to redo a sample in exact order
    double ey;                      // bound on |fi' - fi|, |fq' - fq| of the FMA-contracted front end + matched filter at FULL SCALE
    const int *amax;                // [S] largest |int16 sample| the fast kernels have converted so far (float bits): the bound scales with it
    double margin_scale;            // safety factor on the detector margins (>= 1; tests raise it to force the exact path)
    double argmax_scale;            // ... on the argmax margin (tests raise it to provoke an uncertifiable decision)
    const int *raw;                 // the call's input, as FmArgs
    long long stride_pairs;
    int ic, qc, decim, first_out, mix, tper;
    const double2 *tcs;
    const unsigned char *kvco;
    const double *sincos;
};

struct SyncArgs {
    const signed char *bitlog;
    long long bitlog_stride;
    const int *nbits;
    signed char *corr;      // [S][max_bits]
    int max_bits;
};
struct SyncFinArgs {
    int *trig_count, *trig_bits;
    int trig_cap;
    TailState *st;
    int fuse;  // 1: this kernel orders the hits itself (short calls: one dependent launch less); 0: k_sync_fin follows --
               // for a long call the scan is a chain of L2 round trips that one wave walks while the workgroup's LDS
               // image and its other three waves' registers stay allocated (measured at 8192 x 2^20: the step +4 ms)
};

// ---- launchers.  int: JSDR_OK / JSDR_ERR; const char *: the name of the kernel launched (the handle records it), null on error
bool front_reg_enabled();  // JSDR_FRONT_REG=0: never the register-staged front end
const char *launch_front(const FrontArgs &fa, int decim, int nstreams, bool fast, hipStream_t st);
int launch_front_split(const FrontArgs &fa, const unsigned short *ktu9, const double *sc9, int decim, const FftFrontState *dhist,
                       int nstreams, hipStream_t st);
int launch_seam_hist(const int2 *hist, int is_float, const double *sincos, const SeamHist &sh, FftFrontState *st, FftFrontState *st2,
                     int nstreams, hipStream_t stream);
int launch_seam_q(double2 *dm, long long dm_stride, const double2 *dm2, long long dm2_stride, int J, int nstreams, hipStream_t st);
// st, qcol: the channel's first row of the channel-major FFT state, and of the Q columns' copy ([ninputs][26])
int launch_chan_seam_hist(const int2 *hist, int is_float, const double *sc9, const ChanSeamHist &sh, FftFrontState *st, double *qcol,
                          int ninputs, hipStream_t stream);
int launch_hist_in(const HistArgs &ha, hipStream_t st);
int launch_hist_convert(int2 *hist, int nstreams, int to_float, int *bad, hipStream_t st);
int launch_matched(const MatchedArgs &ma, int nstreams, hipStream_t st);
int launch_dm_history(double2 *dm, long long dm_stride, long long nds, int nstreams, hipStream_t st);
int launch_fm_prep(const EdgeArgs &ea, const HistArgs &ha, const ScatterArgs &sc, hipStream_t st);
// *items, *grid: the work items (tiles x streams) of the launch and the workgroups that stride over them; *phase: the tuner phase
// (0 .. 7) of tile 0's window sample 0 where the launch took the 8-phase tuner's form, -1 where it took the generic one
int launch_fm(const FmArgs &a, int decim, bool mix, bool dc, bool fast, int nstreams, hipStream_t st, long long *items, long long *grid,
              int *phase);
int launch_fm_prep_f32(const EdgeF32Args &ea, const HistArgs &ha, hipStream_t st);
int launch_fm_f32(const FmF32Args &a, int decim, bool mix, int nstreams, hipStream_t st, long long *items, long long *grid);
const char *launch_tail(const TailArgs &ta, bool cert, hipStream_t st);
bool sync_t_applies(int max_bits);  // the transposed-image sync kernel takes a log of that many new bits (JSDR_SYNC_T=0: never)
int launch_sync_t(const SyncArgs &sa, const SyncFinArgs &sf, int nstreams, hipStream_t st);
int launch_sync(const SyncArgs &sa, long long nds, int nstreams, hipStream_t st);
int launch_sync_fin(const SyncArgs &sa, const SyncFinArgs &sf, int nstreams, hipStream_t st);
int launch_reset_maxcorr(TailState *st, int nstreams, hipStream_t stream);
int launch_reset_maxcorr_chan(TailState *st, int nin, int nch, int ch, hipStream_t stream);
// slot = int32 header[16] | int8 bits[slot_bits] | trig_cap x {int32 rc, int32 bit_index, uint8 data[256]} (k_pack_slots)
int launch_pack_slots(unsigned char *slots, long long slot_bytes, int slot_bits, int trig_cap, const TailState *st, const int *nbits,
                      const signed char *bitlog, long long bitlog_stride, const int *trig_count, const int *trig_bits, const int *fec_rc,
                      const unsigned char *fec_data, const int *fec_last, const int *cnt_dec, int n_in, int n_ds, int nstreams, hipStream_t stream);
void bpsk_debug_clocks_report();  // the compile-time timing probes' counters (JSDR_X_T8CLK / JSDR_X_CLK builds), printed and cleared

}  // namespace jsdr

// receive(): the packed results of a 1-stream call, fetched in one copy (k_snapshot_pack, or the FEC kernel's fused copies)
struct SnapPack {
    jsdr::TailState t;
    int last[2];
    int cdec, nbits, centreBin, pad;
    double avePeakPower, aveCentreBin;
    unsigned char decoded[256];
    signed char bits[512];
};
namespace jsdr {
int launch_snapshot_pack(SnapPack *out, const TailState *st, const int *fec_last, const int *cnt_dec, const int *nbits,
                         const FftFrontState *fs, const unsigned char *decoded, const signed char *bits_new, hipStream_t stream);
}
