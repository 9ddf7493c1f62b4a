// bpsk_pst_walk_body.h -- the body of k_tuner_walk, k_tuner_walk_plan and k_tuner_walk_ramp (bpsk_pst.hip), included between their
// braces: the walk of one stream.  In scope: TunerWalkArgs a, PstPlanArgs p, PstRampArgs r, PstRampAt ra, constexpr bool PLAN (with the stream's
// entries of the call's plan), RAMP (PLAN, and the entries are ramps: under a slope tuPhaseInc is the sample's own).
    const int s = blockIdx.x * PST_WALK_THREADS + threadIdx.x;
    if (s >= a.nstreams) return;
    const long long L = a.nsamples;
    double tu = a.tu[s];
    double inc = a.inc[s];
    double *ck = a.ckpt + (long long)s * a.ckpt_stride;
    const unsigned short *ko = a.kh_old + (long long)s * 32;
    unsigned short *kn = a.kh_new + (long long)s * 32;
    const long long keep = L < 26 ? L : 26;  // samples of this call among the 26 before the next one
    for (int i = 0; i < 26 - (int)keep; i++) kn[i] = ko[i + L];  // (a call shorter than the history: the rest moves up)
    const long long nmain = L - keep;
    long long e0 = 0, e = 0, e_end = 0, next = PST_NO_ENTRY;  // the stream's entries: first, next, end; the next one's position
    int *cke = nullptr;
    if constexpr (PLAN) {
        e0 = e = p.off[s];
        e_end = p.off[s + 1];
        if (e < e_end) next = p.pos[e];
        p.inc0[s] = inc;
        cke = p.ckpt_e + (long long)s * a.ckpt_stride;
    }
    for (long long c = 0; c * PST_C < L; c++) {
        ck[c] = tu;  // c < ckpt_stride: L <= max_batch_samples
        const long long n1 = (c + 1) * PST_C < L ? (c + 1) * PST_C : L;
        if constexpr (PLAN) {
            cke[c] = (int)(e - e0);
            // an entry in this block, in some lane of the wave; RAMP: or the block lies under a slope in one
            if (__any(RAMP ? (next < n1 || ra.s != 0.0) : (next < n1))) {
                for (long long n = c * PST_C; n < n1; n++) {
                    if (n == next) {  // the advance of sample `next` is the first at the new increment
                        if constexpr (RAMP) {
                            ra.t = r.tuning[e];
                            ra.s = r.slope[e];
                            ra.at = n;
                            if (ra.s == 0.0) inc = tuner_ramp_inc(ra.t, ra.s, 0, r.rate);
                        } else {
                            inc = p.inc[e];
                        }
                        e++;
                        next = e < e_end ? p.pos[e] : PST_NO_ENTRY;
                    }
                    if constexpr (RAMP)
                        if (ra.s != 0.0) inc = tuner_ramp_inc(ra.t, ra.s, n - ra.at, r.rate);  // (a lane under no slope keeps its increment)
                    tuner_advance(tu, inc);
                    if (n >= nmain) kn[26 - (L - n)] = (unsigned short)tuner_k9(tu);
                }
                continue;
            }
        }
        for (long long n = c * PST_C; n < n1; n++) {
            tuner_advance(tu, inc);
            if (n >= nmain) kn[26 - (L - n)] = (unsigned short)tuner_k9(tu);  // (uniform: the division runs 26 times a call)
        }
    }
    a.tu[s] = tu;
    if constexpr (PLAN) p.inc_out[s] = inc;  // (every entry lies inside the call: the last one's, a ramp's of the last sample)
