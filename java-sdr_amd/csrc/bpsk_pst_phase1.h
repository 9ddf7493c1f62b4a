// bpsk_pst_phase1.h -- phase 1 of a tuned front end, stated once: the 9-bit tuner table indices of one tile of one row (a stream of
// a tuned handle, a channel of an input of a tuned channel handle), expanded from the row's checkpoints of k_tuner_walk.  Included
// between the braces of k_front_pst* (bpsk_pst_front_body.h) and, once per channel in flight, of k_chan_front_pst* (bpsk_chan_pst.hip):
// text, not a function, for the reason bpsk_pst.hip gives for the bodies -- the plain forms' code stays as it was.
// In scope: a (its inc, ckpt, ckpt_stride and kh_old), PstPlanArgs p, PstRampArgs r, constexpr bool PLAN and RAMP; int s, the row;
// long long n_lo, the input index of the tile's first sample (>= -26), and int cnt, the tile's samples; double *tus, the workgroup's
// phase scratch (pst_slot(cnt - 1) + 1 doubles); unsigned short *k9, where the cnt indices go.  Every thread of the workgroup comes
// through; the text ends behind the barrier after which k9[0 .. cnt - 1] may be read and tus written again.
    // ---- phase 1: the phases of the tile's samples of this call, PST_C of them a lane from the checkpoint before them
    const long long n_first = n_lo < 0 ? 0 : n_lo;
    const long long n_last = n_lo + cnt - 1;  // the newest sample of the tile's last output: 0 <= n_last < L
    const double inc = a.inc[s];
    const double *ck = a.ckpt + (long long)s * a.ckpt_stride;
    for (long long c = n_first / PST_C + threadIdx.x; c <= n_last / PST_C; c += blockDim.x) {
        double tu = ck[c];
        const long long nb = c * PST_C;
        double inc_c = inc;  // the increment at the block's first sample
        if constexpr (PLAN) {  // ... with a plan: of the entry in effect there; then through the entries inside the block
            const long long e0 = p.off[s], e_end = p.off[s + 1];
            long long e = e0 + p.ckpt_e[(long long)s * a.ckpt_stride + c];
            double rt = 0.0, rs = 0.0;  // RAMP: the tuning and the slope of the entry in effect (no slope: inc_c stands), at sample rat
            long long rat = 0;
            if constexpr (RAMP) {
                inc_c = p.inc0[s];
                if (e > e0) {
                    rt = r.tuning[e - 1];
                    rs = r.slope[e - 1];
                    rat = p.pos[e - 1];
                    if (rs == 0.0) inc_c = tuner_ramp_inc(rt, rs, 0, r.rate);
                }
            } else {
                inc_c = e > e0 ? p.inc[e - 1] : p.inc0[s];
            }
            long long next = e < e_end ? p.pos[e] : PST_NO_ENTRY;
            bool slow = next < nb + PST_C;
            if constexpr (RAMP) slow = slow || rs != 0.0;
            if (slow) {
                for (int i = 0; i < PST_C; i++) {
                    const long long n = nb + i;
                    if (n == next) {
                        if constexpr (RAMP) {
                            rt = r.tuning[e];
                            rs = r.slope[e];
                            rat = n;
                            if (rs == 0.0) inc_c = tuner_ramp_inc(rt, rs, 0, r.rate);
                        } else {
                            inc_c = p.inc[e];
                        }
                        e++;
                        next = e < e_end ? p.pos[e] : PST_NO_ENTRY;
                    }
                    if constexpr (RAMP)
                        if (rs != 0.0) inc_c = tuner_ramp_inc(rt, rs, n - rat, r.rate);
                    tuner_advance(tu, inc_c);
                    if (n >= n_first && n <= n_last) tus[pst_slot((int)(n - n_lo))] = tu;
                }
                continue;
            }
        }
        for (int i = 0; i < PST_C; i++) {  // (a block without an entry and under no slope: the plain loop)
            tuner_advance(tu, inc_c);
            const long long n = nb + i;
            if (n >= n_first && n <= n_last) tus[pst_slot((int)(n - n_lo))] = tu;
        }
    }
    __syncthreads();
    const unsigned short *ko = a.kh_old + (long long)s * 32;
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
        const long long n = n_lo + e;
        k9[e] = n < 0 ? ko[26 + n] : (unsigned short)tuner_k9(tus[pst_slot(e)]);
    }
    __syncthreads();
