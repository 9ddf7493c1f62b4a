// bpsk_pst_front_body.h -- the body of k_front_pst<F32IN>, k_front_pst_plan<F32IN> and k_front_pst_ramp<F32IN> (bpsk_pst.hip),
// included between their braces.  In scope: PstFrontArgs a, PstPlanArgs p, PstRampArgs r, constexpr bool F32IN, PLAN (phase 1
// switches tuPhaseInc at the plan's entries), RAMP (PLAN, and the entries are ramps: under a slope tuPhaseInc is the sample's own).
    extern __shared__ __align__(16) unsigned char smem[];
    double *sc = reinterpret_cast<double *>(smem);            // [514] cos[0..256], sin[0..256]
    double *taps = sc + 514;                                  // [27]
    double2 *x = reinterpret_cast<double2 *>(taps + 28);      // [cap] the tile's samples, mixed
    double *tus = reinterpret_cast<double *>(x);              // ... before that, their phases (pst_slot)
    const int D = a.decim;
    const int cap = (a.nout - 1) * D + 27;
    unsigned short *k9 = reinterpret_cast<unsigned short *>(x + cap);  // [cap] their table indices
    for (int i = threadIdx.x; i < 514; i += blockDim.x) sc[i] = a.sc9[i];
    if (threadIdx.x < 27) taps[threadIdx.x] = a.ds_taps[threadIdx.x];
    const int s = blockIdx.y;
    const long long j0 = (long long)blockIdx.x * a.nout;
    const long long jend = (j0 + a.nout < a.nds) ? j0 + a.nout : a.nds;
    const long long n_lo = (long long)a.first_out + (long long)D * j0 - 26;  // input index of x[0] (>= -26)
    const int cnt = (int)((jend - 1 - j0) * D + 27);                         // <= cap
#include "bpsk_pst_phase1.h"
    // ---- the samples, read once, converted and mixed (:372-373, :388-390 / :395)
    const int *raw = a.raw + (long long)s * a.stride_pairs;
    const int2 *hist = a.hist + (long long)s * 32;
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
        const long long n = n_lo + e;
        float2 f;
        if constexpr (F32IN) {
            if (n >= 0) {
                f = reinterpret_cast<const float2 *>(a.raw)[(long long)s * a.stride_pairs + n];
            } else {
                const int2 h = hist[26 + n];  // the float pair's bits (k_hist_in)
                f = make_float2(__int_as_float(h.x), __int_as_float(h.y));
            }
        } else {
            int w;
            if (n >= 0) {
                w = raw[n];
                const int si = java_short_add((int)(short)(w & 0xffff), a.ic);
                const int sq = java_short_add(w >> 16, a.qc);
                w = (si & 0xffff) | (sq << 16);
            } else {
                w = hist[26 + n].x;  // kept DC-corrected by k_hist_in
            }
            f = make_float2(i16_to_float_java((int)(short)(w & 0xffff)), i16_to_float_java(w >> 16));
        }
        const int k = k9[e];
        double di = (double)f.x, dq = (double)f.y;
        di = di * sc[k];
        dq = dq * sc[257 + k];
        x[e] = make_double2(di, dq);
    }
    __syncthreads();
    // ---- phase 2: one output a lane
    const long long j = j0 + threadIdx.x;
    if (j >= jend) return;
    const double HOWARD = 0.9 * 32768.0;                         // :469
    const double2 *xw = x + (long long)D * threadIdx.x + 26;     // xw[-age] = the sample `age` before the one that completes output j
    double fi = 0.0, fq = 0.0;
    for (int age = 0; age < 27; age++) {
        const double2 v = xw[-age];
        const double tp = taps[age];
        fi += v.x * tp;
        fq += v.y * tp;
    }
    const double oi = fi * HOWARD, oq = fq * HOWARD;  // :486
    const int kv = a.kvco[j];
    a.dm[(long long)s * a.dm_stride + 64 + j] = make_double2(oi * sc[kv], oq * sc[257 + kv]);  // :515-516
