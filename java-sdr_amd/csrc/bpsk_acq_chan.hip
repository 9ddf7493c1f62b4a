// bpsk_acq_chan.hip -- the FFT-acquire front end of a channel handle (jsdr_bpsk_create_mode_channels): several FUNcubeBPSKDemod
// tabs in FFT-acquire on ONE input (jsdr.java:479-483), each searching its own half of the band ("Track high",
// FUNcubeBPSKDemod.java:183-189).  Of doBufferFFT (:406-464) the input conversion, the forward transform and |X| (:416-427) depend on
// the frame alone, the boxcar and its first maximum (:428-443) on the frame and the band; only the three-number rule (:444-453), the
// gather, the inverse transform and RxDownSample (:458-463) belong to a tab.  bpsk_acq.hip's three phases cut the loop exactly there:
//   phase A          once per (INPUT, frame).  Frames of 1024 .. 8192 samples (2^k) with both bands in use: k_acqc_fwd below, ONE
//                    transform that leaves one spectrum row [0, n/2 + 28) and, per band, the boxcar sums and (maxBin, binPos).
//                    One band in use on the whole handle: k_acq_fwd itself over the inputs -- nothing of the other band is paid.
//                    9600 / 4800 / 4410 and every other frame: k_acqm_fwd / the any-frame passes, once per input and band IN USE.
//   scan, inverse,   once per FFT channel over that channel's streams (one per input), by k_acq_scan / k_acq_inv (k_acqm_inv, the
//   edges            any-frame passes) / k_acq_edges THEMSELVES: the streams of channel c are i * nch + c, so with dm = dm + c *
//                    dm_stride, a row stride of nch * dm_stride and the FFT state kept channel-major, stream index s of such a launch
//                    IS input s -- the kernels read their input's rows under their channel's band and write their stream's dm row,
//                    centre bins, edges and state.  Per-stream work is the ordinary handle's, instruction for instruction.
//   the seam        a live channel handle (jsdr_bpsk_create_live_channels), a channel's first call after tune -> FFT-acquire:
//                    k_acq_edges_seam below, behind that channel's k_acq_edges in the call's first launch, forms the Q rail of the
//                    outputs whose windows reach into the tune path's history from its Q column.
// A both-band row holds the bins in natural order, so every channel gathers from it as a lower-band stream does (offset c - 102):
// the upper band's centre bins end at n/2 - 75, inside the row.
//
// Compiled with -ffp-contract=off.  k_acqc_fwd is k_acq_fwd's transform -- the same butterflies on the same table in the same order,
// 16 points a thread, LDS-only barriers, in-order requests, tickets -- with the last stage formed for bins [0, n/2 + 28) and the
// boxcar run once per band over the one |X| image.
#include "bpsk_acq_dev.h"
#include "bpsk_fftplan.h"

namespace jsdr {

struct AcqcFwdArgs {
    AcqArgs a;        // S = inputs; spec rows of nsb = n/2 + 28 bins; aband / peak: the LOWER band's
    double *aband1;   // [S F][na] the UPPER band's boxcar sums over [n/4 + 75, n/2 - 75)
    AcqPeak *peak1;   // [S F]
};

template <int LOGN>
__global__ __launch_bounds__((1 << LOGN) / 16, 2) void k_acqc_fwd(AcqcFwdArgs ca)
{
    const AcqArgs &a = ca.a;
    constexpr int N = 1 << LOGN, T = N / 16;
    using Plan = AcqPlan<LOGN>;
    constexpr int GL = Plan::GL, ML = 1 << GL, NGL = 16 >> GL, HL = N >> GL;  // the last pass: wings HL .. N/2
    constexpr int NA = N / 4 - 150;                                           // boxcar outputs per band (:433)
    constexpr int RB = (NA + T - 1) / T + (((NA + T - 1) / T) % 2 == 0 ? 1 : 0);  // per thread, odd (see k_acq_fwd)
    constexpr int PB = 24;                                                    // |X| is kept from bin 24 on (:425-427)
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *X = reinterpret_cast<double2 *>(smem);            // [N] the image
    double2 *TsL = X + N;                                      // [ACQ_TWL]
    double *redv = reinterpret_cast<double *>(TsL + ACQ_TWL);  // [2][8] per-band, per-wave best value
    int *redi = reinterpret_cast<int *>(redv + 16);            // [2][8] ... and index
    int *tkL = redi + 16;                                      // [2]
    double *P = reinterpret_cast<double *>(smem);              // |X| over [24, n/2 - 24): over the image, dead by then
    const double2 *__restrict__ tsg = a.tw;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < ACQ_TWL - 1; i += T) TsL[i] = tsg[i];
    double2 w1[8];
    {
        constexpr int idx[8] = {4, 6, 8, 9, 10, 12, 13, 14};
#pragma unroll
        for (int i = 0; i < 8; i++) w1[i] = acq_tw_s(tsg, idx[i]);
    }
    int pre[16];
    auto fetch = [&](int s, int f) {
        const long long off = (long long)s * a.stride_pairs + (long long)(a.f0 + f) * N + tid;
#pragma unroll
        for (int m = 0; m < 16; m++) pre[m] = a.raw[off + acq_brev<4>(m) * (N / 16)];
    };
    // frames in runs of a.run, a ticket each; a run lies inside one input (k_acq_fwd has the reasons)
    const int K = a.run;
    const int nruns = a.S * a.rps;
    if (tid == 0) tkL[0] = (int)atomicAdd(a.tickets + 0, 1u);
    acq_barrier<T>();
    int r_next = tkL[0];
    int s = 0, f = 0, fe = 0;
    int sn = 0, fn = 0, fen = 0;
    bool have = r_next < nruns;
    bool first = true;
    auto run_of = [&](int r, int &s_, int &f_, int &fe_) {
        s_ = (int)((unsigned)r / (unsigned)a.rps);
        f_ = (r - s_ * a.rps) * K;
        fe_ = f_ + K < a.F ? f_ + K : a.F;
    };
    if (have) {
        run_of(r_next, s, f, fe);
        fetch(s, f);
    }
    while (have) {
        const long long g = (long long)s * a.F + f;  // the frame's row in what the phases hand each other
        unsigned tk = 0;
        if (first && tid == 0) tk = atomicAdd(a.tickets + 0, 1u);
        int tf = tid;  // opaque per frame: nothing derived from the thread index is loop invariant (see k_acq_fwd)
        asm volatile("" : "+v"(tf));
        // ---- forward transform (:416-423): the first four stages from the load registers
        {
            double2 v[16];
#pragma unroll
            for (int m = 0; m < 16; m++) {
                double di, dq;
                fm_convert(pre[m], a.ic, a.qc, true, di, dq);
                v[m] = make_double2(di, dq);
            }
            acq_first4_i16(v, w1);
            const int q1f = acq_brev<LOGN - 4>(tf);
            const int key = acq_key(q1f);
#pragma unroll
            for (int m = 0; m < 16; m++) X[16 * q1f + (m ^ key)] = v[m];
        }
        acq_barrier<T>();
        // the last pass's twiddles, a whole pass ahead of their use and ahead of the next frame's samples (in-order returns)
        double2 twl[NGL][ML - 1];
#pragma unroll
        for (int it = 0; it < NGL; it++) acq_load_tw<GL, HL>(twl[it], tf + T * it, tsg);
        __builtin_amdgcn_sched_barrier(0);
        acq_mid_pass<4, 16, false, LOGN>(X, TsL, tsg, tf);
        {
            int zlate = 0;  // (pinned behind the pass: see k_acq_fwd)
            asm volatile("" : "+v"(zlate));
            if (first && tid == 0) tkL[1] = (int)tk + zlate;
        }
        acq_barrier<T>();
        r_next = tkL[1];
        bool more = true;
        if (f + 1 < fe) {
            sn = s;
            fn = f + 1;
            fen = fe;
        } else if (r_next < nruns) {
            run_of(r_next, sn, fn, fen);
        } else {
            sn = s;
            fn = f;
            fen = fe;
            more = false;
        }
        if constexpr (Plan::G4 != 0) {
            acq_mid_pass<Plan::G3, 256, false, LOGN>(X, TsL, tsg, tf);
            acq_barrier<T>();
        }
        // ---- last pass: wings HL .. N/2; of its last stage only the bins [0, n/2 + 28) are formed (both bands' gathers and |X|)
        double2 o[NGL][ML];
#pragma unroll
        for (int it = 0; it < NGL; it++) {
            const int j = tf + T * it;
#pragma unroll
            for (int m = 0; m < ML; m++) o[it][m] = X[acq_slot_hm(j, HL * m)];
        }
        fetch(sn, fn);  // (unconditional: the workgroup's last frame requests itself once more)
        __builtin_amdgcn_sched_barrier(0);
        acq_barrier<T>();  // the image is dead: |X| goes over it
        double2 *specg = a.spec + g * a.nsb;
#pragma unroll
        for (int it = 0; it < NGL; it++) {
            const int j = tf + T * it;
            acq_stages_w<GL, 0, GL - 1, false>(o[it], twl[it]);  // all but the last stage in full
            // last stage, wing N/2: bins ba = j + HL m (below n/2: all of them) and bb = ba + N/2 (its first 28)
#pragma unroll
            for (int m = 0; m < ML / 2; m++) {
                const int ba = j + HL * m, bb = ba + N / 2;
                const double2 wv = twl[it][ML / 2 - 1 + m];
                const double2 aq = o[it][m], bq = o[it][m + ML / 2];
                const double p1 = wv.x * bq.x, p2 = wv.y * bq.y, p3 = wv.x * bq.y, p4 = wv.y * bq.x;
                const double tr = p1 - p2;
                const double ti = p3 + p4;
                {
                    const double2 r = make_double2(aq.x + tr, aq.y + ti);
                    specg[ba] = r;
                    // |X| where a boxcar of either band reads it (:425-427): [24, n/4 - 24) and [n/4 + 24, n/2 - 24)
                    if ((ba >= PB && ba < N / 4 - 24) || (ba >= N / 4 + 24 && ba < N / 2 - 24)) P[ba - PB] = sqrt(r.x * r.x + r.y * r.y);
                }
                if (bb < N / 2 + 28) specg[bb] = make_double2(aq.x - tr, aq.y - ti);
            }
        }
        acq_barrier<T>();
        // ---- per band: the 100-wide boxcar, summed j ascending for every i (:433-437), and its first maximum (:439-442)
        double bestv[2];
        int besti[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int beg = u ? N / 4 : 0, end = u ? N / 2 : N / 4;
            bestv[u] = 0.0;  // maxBin starts at 0.0, binPos at -1
            besti[u] = -1;
            const int i0 = beg + 75 + RB * tf;
            if (i0 < end - 75) {
                const double *w = P + (i0 - 50 - PB);
                double acc[RB];
                constexpr int NV = 99 + RB, CH = 8, NCH = (NV + CH - 1) / CH;
                double cur[CH], nxt[CH];
#pragma unroll
                for (int c = 0; c < CH; c++) cur[c] = w[c];
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    if (c + 1 < NCH) {
#pragma unroll
                        for (int q = 0; q < CH; q++)
                            if ((c + 1) * CH + q < NV) nxt[q] = w[(c + 1) * CH + q];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = 0; q < CH; q++) {
                        const int k = c * CH + q;
                        if (k < NV) {
#pragma unroll
                            for (int r = 0; r < RB; r++) {
                                if (k == r) acc[r] = cur[q];  // 0.0 + x == x for the |X| values (never -0.0)
                                if (k > r && k < r + 100) acc[r] += cur[q];
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = 0; q < CH; q++) cur[q] = nxt[q];
                }
                double *ab = (u ? ca.aband1 : a.aband) + g * a.na + (i0 - (beg + 75));
#pragma unroll
                for (int r = 0; r < RB; r++) {
                    if (i0 + r < end - 75) {
                        ab[r] = acc[r];
                        if (bestv[u] < acc[r]) {  // i ascends within a thread: strict '<' keeps the first maximum
                            bestv[u] = acc[r];
                            besti[u] = i0 + r;
                        }
                    }
                }
            }
            // the wave's first maximum: the largest value, and of the lanes that hold it the lowest (outputs ascend with the lane)
            const double mv = acq_wave_max(bestv[u]);
            int mi = -1;
            if (mv > 0.0) {
                const unsigned long long bal = __ballot(bestv[u] == mv && besti[u] >= 0);
                mi = __builtin_amdgcn_readlane(besti[u], (int)__builtin_ctzll(bal));
            }
            bestv[u] = mv;
            besti[u] = mi;
        }
        if constexpr (T > 64) {
            if (lane == 0) {
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    redv[8 * u + wave] = bestv[u];
                    redi[8 * u + wave] = besti[u];
                }
            }
            acq_barrier<T>();
            if (tid < 2) {
                const int u = tid;
                double mv = 0.0;
                int mi = -1;
#pragma unroll
                for (int w = 0; w < T / 64; w++) first_max_merge(mv, mi, redv[8 * u + w], redi[8 * u + w]);
                AcqPeak pk;
                pk.maxBin = mv;
                pk.binPos = mi;
                pk.pad = 0;
                (u ? ca.peak1 : a.peak)[g] = pk;
            }
        } else {
            if (tid < 2) {
                const int u = tid;
                const double bv = u ? bestv[1] : bestv[0];
                const int bi = u ? besti[1] : besti[0];
                AcqPeak pk;
                pk.maxBin = bi >= 0 ? bv : 0.0;
                pk.binPos = bi;
                pk.pad = 0;
                (u ? ca.peak1 : a.peak)[g] = pk;
            }
            acq_barrier<T>();  // P is read before the next frame's first pass stores over it
        }
        first = fn != f + 1 || sn != s;
        have = more;
        s = sn;
        f = fn;
        fe = fen;
    }
}

// ============================================================================================================= the seam's edges
// jsdr_bpsk_create_live_channels, the first call of a channel after it switched tune -> FFT-acquire.  dsBuf then holds the tune
// path's last 26 samples, distinct I and Q columns, and the first outputs of the call's first frame -- those whose 27-tap windows
// reach back into it, at most 26 / D + 1 -- are RxDownSample(re, re) over (I column | frame) on the I rail and (Q column | frame) on
// the Q rail (:461-463, :479-492).  The channel's launches have run with the I column in FftFrontState::hist (k_chan_seam_hist),
// so every fi is right and k_acq_edges has formed those outputs' Q rail from the I column too; this kernel forms it again from the
// Q column: k_acq_edges' window loop over the same 26 head samples of frame 0 (still in the launch's scratch: it runs behind the
// channel's k_acq_edges of the call's FIRST launch) and qcol in the history's place, written to .y alone.  One block per stream
// of the channel (= input), one thread per output.
__global__ __launch_bounds__(64) void k_acq_edges_seam(AcqArgs a, const double *qcol, int J)
{
    const int s = blockIdx.x, j = threadIdx.x;
    const int e = (int)a.first_out + a.decim * j;  // the sample of frame 0 whose arrival completes output j
    if (j >= J || e >= 26 || e >= a.n || j >= (int)a.nds) return;
    const double *head = a.edges + (long long)s * a.F * 52;  // frame 0 of the launch is frame 0 of the call (a.f0 == 0)
    const double *prev = qcol + (long long)s * 26;
    double fq = 0.0;
#pragma unroll
    for (int k = 0; k < 27; k++) {  // newest first (:479-483)
        const int i = e - k;
        const double x = i >= 0 ? head[i] : prev[26 + i];
        fq += x * ds_tap(k);
    }
    const double ov = fq * ACQ_HOWARD;
    a.dm[(long long)s * a.dm_stride + 64 + j].y = ov * a.vco_cs[j].y;
}

// ============================================================================================================= host
size_t acq3c_frame_bytes(int n, int band_mask, bool generic)
{
    size_t b = 64;
    for (int u = 0; u < 2; u++)
        if (band_mask & (1 << u)) b += acq3_frame_bytes(n, u) + 64;  // (each with room for a centre bin and the edges: one set is used)
    // (a both-band row [0, n/2 + 28) is shorter than the two bands' own rows together)
    if (generic) b += acqg_image_bytes(n);
    return b;
}

template <int LOGN>
static int launch_acqc_fwd_t(AcqcFwdArgs &ca, int num_cu, hipStream_t st)
{
    constexpr int N = 1 << LOGN, T = N / 16;
    constexpr size_t lds = sizeof(double2) * ((size_t)N + ACQ_TWL) + 16 * sizeof(double) + 16 * sizeof(int) + 2 * sizeof(int) + 8;
    const long long nfr = (long long)ca.a.S * ca.a.F;
    int per_cu = 1;
    JSDR_LDS_ATTR((k_acqc_fwd<LOGN>), lds);
    JSDR_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_acqc_fwd<LOGN>, T, lds));
    if (per_cu < 1) per_cu = 1;
    long long grid = (long long)per_cu * num_cu;
    if (grid > nfr) grid = nfr;
    hipLaunchKernelGGL((k_acqc_fwd<LOGN>), dim3((unsigned)grid), dim3(T), lds, st, ca);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_acq3_chan(const FftFrontArgs &fa, AcqChanArgs &ca, unsigned char *scratch, size_t scratch_bytes, int chunk_frames, int num_cu,
                     hipStream_t st, const AcqProf &prof, const FftPlan &plan)
{
    const bool generic = plan.kind == FRONT_GEN;
    const int n = fa.n;
    JSDR_REQUIRE(generic || acq3_supported(n), "bpsk channels: no FFT-acquire front end for frames of %d samples", n);
    JSDR_REQUIRE(ca.nfft >= 1 && ca.nfft <= 16 && ca.nin >= 1 && (fa.raw != nullptr) != (fa.rawf != nullptr), "bpsk channels: internal: bad FFT-acquire channel set");
    int mask = 0;
    for (int k = 0; k < ca.nfft; k++) mask |= ca.up[k] ? 2 : 1;
    const bool pow2 = !generic && !acqm_supported(n);
    // one transform serves both bands -- of int16 input: k_acqc_fwd has no float form, float input (jsdr_bpsk_batch_f32) takes
    // k_acq_fwd's once per band in use
    const bool both = mask == 3 && pow2 && !fa.rawf;
    if (chunk_frames < 1) chunk_frames = 1;
    const size_t nf = (size_t)ca.nin * (size_t)chunk_frames;
    JSDR_REQUIRE(nf * acq3c_frame_bytes(n, mask, generic) + 4096 <= scratch_bytes, "bpsk channels: FFT-acquire scratch too small (%zu frames)", nf);
    // the launch's scratch: per band in use the spectrum rows, boxcar sums and peaks of every (input, frame) -- a both-band forward
    // kernel leaves ONE set of rows -- then one set of centre bins and edges (the channels' launches follow each other on the stream)
    int nsb[2] = {0, 0}, na[2] = {0, 0};
    double2 *spec[2] = {nullptr, nullptr};
    double *aband[2] = {nullptr, nullptr};
    AcqPeak *peak[2] = {nullptr, nullptr};
    unsigned char *p = scratch;
    auto take = [&](size_t bytes) {
        unsigned char *q = p;
        p += (bytes + 255) & ~(size_t)255;
        return q;
    };
    for (int u = 0; u < 2; u++) acq3_row_layout(n, u, &nsb[u], &na[u]);
    if (both) {
        nsb[0] = nsb[1] = n / 2 + 28;
        spec[0] = spec[1] = reinterpret_cast<double2 *>(take(sizeof(double2) * nf * (size_t)nsb[0]));
    }
    for (int u = 0; u < 2; u++) {
        if (!(mask & (1 << u))) continue;
        if (!both) spec[u] = reinterpret_cast<double2 *>(take(sizeof(double2) * nf * (size_t)nsb[u]));
        aband[u] = reinterpret_cast<double *>(take(sizeof(double) * nf * (size_t)na[u]));
        peak[u] = reinterpret_cast<AcqPeak *>(take(sizeof(AcqPeak) * nf));
    }
    AcqArgs a;
    a.raw = fa.raw;
    a.rawf = fa.rawf;
    a.stride_pairs = fa.stride_pairs;
    a.ic = fa.ic;
    a.qc = fa.qc;
    a.S = ca.nin;
    a.n = n;
    a.decim = fa.decim;
    a.first_out = fa.first_out;
    a.nds = fa.nds;
    a.vco_cs = fa.vco_cs;
    a.tw = fa.tw;
    a.edges = reinterpret_cast<double *>(take(sizeof(double) * 52 * nf));
    a.cbin = reinterpret_cast<int *>(take(sizeof(int) * nf));
    a.tickets = reinterpret_cast<unsigned *>(take(64));
    double2 *img = reinterpret_cast<double2 *>(p);  // (any-frame passes only)
    JSDR_REQUIRE((size_t)(p - scratch) + (generic ? nf * acqg_image_bytes(n) : 0) <= scratch_bytes, "bpsk channels: internal: FFT-acquire scratch layout");
    a.run = 4;
    if (const char *e = knob("JSDR_ACQ_RUN")) a.run = atoi(e) >= 2 ? atoi(e) : 4;
    a.nwg = 0;
    a.clk = nullptr;
    ca.fwd_frames = ca.inv_frames = 0;
    ca.fwd_name = both ? "k_acqc_fwd" : generic ? "k_acqg_pass" : pow2 ? "k_acq_fwd" : "k_acqm_fwd";
    auto band = [&](int u) {
        a.do_up = u;
        a.spec = spec[u];
        a.nsb = nsb[u];
        a.aband = aband[u];
        a.na = na[u];
        a.peak = peak[u];
    };
    for (int f0 = 0; f0 < fa.nframes; f0 += chunk_frames) {
        a.f0 = f0;
        a.F = fa.nframes - f0 < chunk_frames ? fa.nframes - f0 : chunk_frames;
        a.rps = (a.F + a.run - 1) / a.run;
        JSDR_REQUIRE((long long)a.S * a.rps < 0x7fffffffLL && (long long)(a.f0 + a.F) * n < 0x7fffffffLL,
                     "bpsk channels: an FFT-acquire launch of %d inputs x %d frames is beyond its 32-bit frame arithmetic", a.S, a.F);
        // ---- phase A over the inputs
        a.st = ca.st;
        a.dm = fa.dm;
        a.dm_stride = fa.dm_stride;
        if (both) {
            AcqcFwdArgs fw;
            band(0);
            fw.a = a;
            fw.aband1 = aband[1];
            fw.peak1 = peak[1];
            JSDR_HIP_TRY(hipMemsetAsync(a.tickets, 0, 2 * sizeof(unsigned), st));
            if (prof.mark) prof.mark(prof.ctx, 4, true, st);
            int rc;
            switch (fa.logn) {
                case 10: rc = launch_acqc_fwd_t<10>(fw, num_cu, st); break;
                case 11: rc = launch_acqc_fwd_t<11>(fw, num_cu, st); break;
                case 12: rc = launch_acqc_fwd_t<12>(fw, num_cu, st); break;
                default: rc = launch_acqc_fwd_t<13>(fw, num_cu, st); break;
            }
            if (rc != JSDR_OK) return rc;
            if (prof.mark) prof.mark(prof.ctx, 4, false, st);
            ca.fwd_frames += (long long)a.S * a.F;
        } else {
            for (int u = 0; u < 2; u++) {
                if (!(mask & (1 << u))) continue;
                band(u);
                if (launch_acq3_parts(a, fa, ACQ_PART_FWD, num_cu, st, prof, plan, img) != JSDR_OK) return JSDR_ERR;
                ca.fwd_frames += (long long)a.S * a.F;
            }
        }
        // ---- scan, inverse, edges: per FFT channel over its streams (input i of channel c is stream i * nch + c)
        for (int k = 0; k < ca.nfft; k++) {
            band(ca.up[k] ? 1 : 0);
            if (both) a.do_up = 0;  // a both-band row is in natural order: every gather is a lower-band stream's ...
            const int up = ca.up[k] ? 1 : 0;
            a.st = ca.st + (size_t)ca.chan[k] * (size_t)ca.nin;
            a.dm = fa.dm + (long long)ca.chan[k] * fa.dm_stride;
            a.dm_stride = fa.dm_stride * ca.nch;
            if (both && up) {
                // ... but the SCAN's band is the channel's own
                AcqArgs sc = a;
                sc.do_up = 1;
                if (launch_acq3_parts(sc, fa, ACQ_PART_SCAN, num_cu, st, prof, plan, img) != JSDR_OK) return JSDR_ERR;
                if (launch_acq3_parts(a, fa, ACQ_PART_INV | ACQ_PART_EDGES, num_cu, st, prof, plan, img) != JSDR_OK) return JSDR_ERR;
            } else {
                if (launch_acq3_parts(a, fa, ACQ_PART_SCAN | ACQ_PART_INV | ACQ_PART_EDGES, num_cu, st, prof, plan, img) != JSDR_OK)
                    return JSDR_ERR;
            }
            ca.inv_frames += (long long)a.S * a.F;
            if (f0 == 0 && ca.seam_q[k] != nullptr && ca.seam_J > 0) {
                // the channel's first call after tune -> FFT-acquire: the Q rail of the outputs that reach into the tune path's history
                hipLaunchKernelGGL(k_acq_edges_seam, dim3((unsigned)a.S), dim3(64), 0, st, a, ca.seam_q[k], ca.seam_J);
                JSDR_LAUNCH_CHECK();
            }
        }
    }
    return JSDR_OK;
}

}  // namespace jsdr
