// bpsk_call_pst.hip -- a tuned handle's call (jsdr_bpsk_create_tuned, jsdr_bpsk_create_tuned_channels): pst_run.  Host code only
// (bpsk_handle.h); the stages it shares with the other kinds of handle are bpsk_call.hip's.
#include "bpsk_handle.h"
#include <cmath>

// ------------------------------------------------------------------------------------------- tuned handles
// what k_front_pst and k_chan_front_pst both take (PstFrontArgs, PstChanFrontArgs): the input rows, the walk's checkpoints, the
// VCO schedule and the outputs of the call
template <class A>
static void pst_front_fill(A &fa, const jsdr_bpsk *h, const int *raw, const float2 *rawf, long long stride_pairs, int ic, int qc,
                           long long nds, int first_out)
{
    memset(&fa, 0, sizeof(fa));
    fa.raw = rawf ? reinterpret_cast<const int *>(rawf) : raw;
    fa.stride_pairs = stride_pairs;
    fa.ic = ic;
    fa.qc = qc;
    fa.hist = h->hist_in[h->hist_cur].p;
    fa.inc = h->pst_inc.p;
    fa.ckpt = h->pst_ckpt.p;
    fa.ckpt_stride = h->pst_ckpt_stride;
    fa.kh_old = h->pst_kh[h->pst_kh_cur].p;
    fa.kvco = kvco_cur(h);
    fa.sc9 = h->sincos9.p;
    fa.ds_taps = h->ds_taps_dev.p;
    fa.dm = h->dm.p;
    fa.dm_stride = h->dm_stride;
    fa.nds = nds;
    fa.first_out = first_out;
    fa.decim = h->decim;
}

// A call of a tuned handle (jsdr_bpsk_create_tuned): every stream's tuner walked on the device (k_tuner_walk), the front end fed
// from the walk's checkpoints (k_front_pst), then the three-kernel path's k_hist_in, k_matched, k_dm_history and the side
// section, as bpsk_run launches them.  build_schedule provides the parts every stream shares -- the decimation counter, the VCO
// schedule, the outputs of the call; the handle's own tuner stands at 0 and its tables are not sent.
int jsdr::pst_run(jsdr_bpsk *h, const int16_t *raw_dev, const float *rawf_dev, long long stride_i16, long long L, int ic, int qc,
                  hipStream_t st)
{
    JSDR_REQUIRE(raw_dev || rawf_dev, "bpsk: null input");
    JSDR_REQUIRE(L > 0 && L <= h->max_batch, "bpsk: nsamples=%lld outside (0, max_batch_samples=%lld]", L, h->max_batch);
    const int rows_in = pst_rows_in(h);  // (a tuned channel handle: the stride is between inputs)
    JSDR_REQUIRE((stride_i16 & 1) == 0 && (rows_in == 1 || stride_i16 >= 2 * L),
                 "bpsk: %s stride %lld too small for %lld samples", h->pst_nch > 0 ? "input" : "stream", stride_i16, L);
    // the previous call may have come through the other input form (before anything moves on: the conversion can refuse)
    const bool planned = h->pst_plan_n > 0;
    JSDR_REQUIRE(!planned || L > h->pst_plan_max_at, "bpsk: the pending tuning plan has an entry at sample %lld, the call has %lld samples; the "
                 "handle is unchanged and the plan stays pending", h->pst_plan_max_at, L);
    const bool ramp = planned && h->pst_plan_ramp;
    if (ramp)  // a ramp that runs to the call's end: its last sample's tuning (the other end was checked with the plan)
        for (const PstPlanLast &pl : h->pst_plan_last) {
            const double t_end = tuner_ramp_tuning(pl.tuning, pl.slope, L - 1 - pl.at);
            JSDR_REQUIRE(std::isfinite(t_end) && t_end < (double)h->rate, "bpsk: entry %lld of the pending ramp plan (stream %d, from sample %lld) "
                         "reaches %g Hz at the call's last sample (%lld), not a finite value below the rate (%d Hz); the handle is unchanged and "
                         "the plan stays pending", pl.entry, pl.stream, pl.at, t_end, L - 1, h->rate);
        }
    if (hist_form(h, rawf_dev != nullptr, rows_in, st) != JSDR_OK) return JSDR_ERR;
    const int S = h->nstreams;
    const int first_out = h->decim - 1 - h->dsCnt;
    const long long g_first = h->n_ds;
    const long long nds = build_schedule(h, L);
    JSDR_REQUIRE(nds <= h->max_ds, "bpsk: internal: %lld decimated samples exceed capacity %lld", nds, h->max_ds);
    if (!h->tables_on_device) {
        h->tab_cur ^= 1;  // (double-buffered as bpsk_run's)
        if (nds > 0)
            if (h2d_call(h, kvco_cur(h), h->cur.kvco.data(), (size_t)nds, st) != JSDR_OK) return JSDR_ERR;
        h->tables_on_device = true;
    }
    const int *raw = reinterpret_cast<const int *>(raw_dev);
    const float2 *rawf = reinterpret_cast<const float2 *>(rawf_dev);
    const long long stride_pairs = stride_i16 / 2;
    // the plan was copied when it was given: the planned forms of the two kernels read it where it lies
    const PstPlanArgs pa = {h->pst_plan_off.p, h->pst_plan_pos.p, h->pst_plan_inc.p, h->pst_inc0.p, h->pst_ckpt_e.p, h->pst_inc.p};
    const PstPlanArgs *plan = planned ? &pa : nullptr;
    const PstRampArgs ra = {h->pst_plan_tun.p, h->pst_plan_slope.p, (double)h->rate};
    const PstRampArgs *rplan = ramp ? &ra : nullptr;
    {
        TunerWalkArgs wa;
        wa.tu = h->pst_tu.p;
        wa.inc = h->pst_inc.p;
        wa.ckpt = h->pst_ckpt.p;
        wa.ckpt_stride = h->pst_ckpt_stride;
        wa.nsamples = L;
        wa.kh_old = h->pst_kh[h->pst_kh_cur].p;
        wa.kh_new = h->pst_kh[h->pst_kh_cur ^ 1].p;
        wa.nstreams = S;
        ProfScope ps(h, PK_TWALK, st);
        if (launch_tuner_walk(wa, plan, rplan, st) != JSDR_OK) return JSDR_ERR;
    }
    if (nds > 0 && h->pst_nch > 0) {  // every input read once, its channels' rows fed from the walk's checkpoints
        PstChanFrontArgs fa;
        pst_front_fill(fa, h, raw, rawf, stride_pairs, ic, qc, nds, first_out);
        fa.nch = h->pst_nch;
        ProfScope ps(h, PK_FRONT, st);
        h->front_name = ramp ? "k_chan_front_pst_ramp" : planned ? "k_chan_front_pst_plan" : "k_chan_front_pst";
        if (launch_chan_front_pst(fa, h->pst_nin, rawf != nullptr, plan, rplan, st) != JSDR_OK) return JSDR_ERR;
    } else if (nds > 0) {
        PstFrontArgs fa;
        pst_front_fill(fa, h, raw, rawf, stride_pairs, ic, qc, nds, first_out);
        ProfScope ps(h, PK_FRONT, st);
        h->front_name = ramp ? "k_front_pst_ramp" : planned ? "k_front_pst_plan" : "k_front_pst";
        if (launch_front_pst(fa, S, rawf != nullptr, plan, rplan, st) != JSDR_OK) return JSDR_ERR;
    }
    h->pst_kh_cur ^= 1;
    if (run_hist_in(h, hist_args(h, raw, rawf, stride_pairs, L, ic, qc, rows_in), st) != JSDR_OK) return JSDR_ERR;
    const int yb = h->y_cur;
    if (wait_tail(h, yb, st) != JSDR_OK) return JSDR_ERR;
    if (nds > 0 && run_matched(h, yb, nds, g_first, st) != JSDR_OK) return JSDR_ERR;
    if (finish_call(h, yb, L, nds, g_first, first_out, ic, qc, raw, stride_pairs, kvco_cur(h), tcs_cur(h), st) != JSDR_OK) return JSDR_ERR;
    if (planned) {  // one-shot: the streams it named stand at their last entries, a ramp at the call's last sample (the walk left
                    // their tuPhaseInc on the device: tuner_inc of these)
        for (const PstPlanLast &pl : h->pst_plan_last) h->pst_tuning[(size_t)pl.stream] = tuner_ramp_tuning(pl.tuning, pl.slope, L - 1 - pl.at);
        pst_plan_clear(h);
    }
    return JSDR_OK;
}
