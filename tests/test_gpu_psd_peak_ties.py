"""GPU: the first-maximum search of every PSD kernel family on rows whose maximum is held many times over (tests/peak_ties.py).

Every row of every entry point is checked against the reference's serial rule (fft.java:201-224) applied to the row's OWN bins:
the two trailing floats must be, bit for bit, the Hz of the first bin that holds the maximum and the maximum.  That is exact,
needs no oracle and no tolerance, and holds whatever the transform's rounding: a reduction that finds the right value and the
wrong bin among equals fails it.  The frames: combs of period r (the maximum held by n / r bins), among them the impulse at
sample 0 (all n bins one number: every thread, lane and wave of a reduction holds a copy of the maximum), a silent frame (no
maximum), noise (no tie), a real-valued tone (mirror bins) and, in the float forms, a frame with a +Inf (the first +Inf bin wins,
NaN bins never).  The impulse stands first, last and either side of a workgroup's frame count."""
import numpy as np
import pytest

import java_sdr_amd as J
import nonfinite as NF
import oracle_lib as O
import peak_ties as PT

pytestmark = pytest.mark.gpu

FPB = {64: 32, 128: 32, 256: 16, 512: 4, 1024: 4, 2048: 2, 4096: 1, 8192: 1}  # frames per workgroup of k_fft (pick_launcher); 1 elsewhere
IC, QC = 1234, -4321


def build_batch(n):
    """(int16 frames [nf][2n], kinds [nf]): kind is the comb's period r, or "zero" / "noise" / "real tone" """
    combs, periods = PT.comb_frames(n, n)
    rng = np.random.default_rng(n + 1)
    rest = [(combs[i], periods[i]) for i in range(1, len(periods))]
    rest += [(np.zeros(2 * n, np.int16), "zero"), (rng.integers(-20000, 20001, 2 * n).astype(np.int16), "noise"),
             (PT.real_tone_frame(n), "real tone")]
    fpb = FPB.get(n, 1)
    while len(rest) < fpb + 2:  # (the small frames: enough rows to reach into a second workgroup)
        rest = rest + rest
    imp = (combs[0], 1)
    assert periods[0] == 1
    seq = [imp] + rest[:max(fpb - 2, 0)] + [imp, imp] + rest[max(fpb - 2, 0):] + [imp]
    if fpb == 1:
        seq = seq[1:]
    kinds = [k for _, k in seq]
    assert kinds[0] == 1 and kinds[-1] == 1 and kinds[fpb - 1] == 1 and kinds[fpb] == 1
    return np.stack([x for x, _ in seq]), kinds


def to_f32(raw):
    return (O.convert_i16(raw.ravel()) * np.float32(0.93)).astype(np.float32).reshape(raw.shape)


def inf_frame(n):
    """the +Inf frame of the non-finite tests (tests/test_gpu_psd_demod_phase_nonfinite.py): noise with one +Inf sample"""
    x = (np.random.default_rng(n).standard_normal(2 * n) * 0.3).astype(np.float32)
    x[2 * (n // 3)] = NF.PINF
    return x


class Tally:
    def __init__(self):
        self.combs = self.tied = self.impulses = 0

    def row(self, row, n, rate, kind, where):
        PT.assert_row_peak(row, n, rate, where)
        if isinstance(kind, int):
            self.combs += 1
            self.tied += PT.multiplicity(row, n) >= 2
        if kind == 1:
            # exact butterflies: zeros added, the unit twiddle multiplied -- all n bins are one number
            assert np.all(PT.u32(row[:n]) == PT.u32(row[0])), (where, "impulse: %d distinct bins" % np.unique(PT.u32(row[:n])).size)
            assert row[n] == 0.0 and PT.u32(row[n + 1]) == PT.u32(row[0]), (where, row[n], row[n + 1], row[0])
            assert PT.multiplicity(row, n) == n
            self.impulses += 1
        if kind == "zero":
            assert np.all(np.isneginf(row[:n])) and row[n + 1] == -PT.FLT_MAX, where
        if kind == "inf":
            NF.check_psd_inf_frame(row, n, rate, where)

    def rows(self, rows, n, rate, kinds, where):
        assert rows.shape == (len(kinds), n + 2), (where, rows.shape)
        for k, (row, kind) in enumerate(zip(rows, kinds)):
            self.row(row, n, rate, kind, (where, "frame %d" % k, kind))


def batch(f, form, d_in, nf, ic=0, qc=0):
    d_psd = J.DeviceBuffer(4 * nf * (f.n + 2))
    if form == "i16":
        f.batch_i16(d_in, nf, d_psd, ic, qc)
    else:
        f.batch_f32(d_in, nf, d_psd)
    J.binding.stream_sync()
    return d_psd.to_host(np.float32).reshape(nf, f.n + 2)


def fused_rows(f, form, d_in, nf):
    """the fused waterfall call at width = n: the pooled maxima are the row's bins, the peak pair its two trailing floats"""
    n = f.n
    d_pix, d_max, d_peak = J.DeviceBuffer(4 * nf * n), J.DeviceBuffer(4 * nf * n), J.DeviceBuffer(4 * nf * 2)
    if form == "i16":
        f.waterfall_i16(d_in, nf, n, d_pix, max_dev=d_max, peak_dev=d_peak)
    else:
        f.waterfall_f32(d_in, nf, n, d_pix, max_dev=d_max, peak_dev=d_peak)
    J.binding.stream_sync()
    return np.concatenate([d_max.to_host(np.float32).reshape(nf, n), d_peak.to_host(np.float32).reshape(nf, 2)], axis=1)


@pytest.mark.parametrize("n,family", PT.PSD_SIZES)
def test_psd_first_maximum_on_tied_rows(n, family):
    rate = PT.psd_rate(n)
    f = J.Fft(n, rate)
    assert f.kernel_name() == family, f.kernel_name()
    raw, kinds = build_batch(n)
    nf = len(kinds)
    flt = np.concatenate([to_f32(raw), inf_frame(n)[None, :]])
    fkinds = kinds + ["inf"]
    t = Tally()
    d_raw, d_flt = J.DeviceBuffer.from_host(raw), J.DeviceBuffer.from_host(flt)
    # the batch forms
    a = batch(f, "i16", d_raw, nf)
    t.rows(a, n, rate, kinds, (n, "batch_i16"))
    # ... the same samples made by the DC correction: before it, the impulse frame's silent samples are (-IC, -QC)
    shifted = raw.astype(np.int32).reshape(nf, n, 2) - np.array([IC, QC])
    assert np.abs(shifted).max() < 32768
    b = batch(f, "i16", J.DeviceBuffer.from_host(shifted.astype(np.int16)), nf, IC, QC)
    t.rows(b, n, rate, kinds, (n, "batch_i16 ic qc"))
    assert np.array_equal(PT.u32(a), PT.u32(b)), (n, "the DC correction made the same samples, the rows differ")
    c = batch(f, "f32", d_flt, nf + 1)
    t.rows(c, n, rate, fkinds, (n, "batch_f32"))
    # one frame a call, spread over the chip: every distinct frame once
    seen = set()
    for k, kind in enumerate(fkinds):
        key = (kind, flt[k].tobytes())
        if key in seen:
            continue
        seen.add(key)
        t.row(f.receive(flt[k]), n, rate, kind, (n, "receive", k, kind))
        if k < nf:
            t.row(f.receive_raw(raw[k]), n, rate, kind, (n, "receive_raw", k, kind))
    # the fused PSD-to-waterfall forms
    w = fused_rows(f, "i16", d_raw, nf)
    assert f.waterfall_kernel() == ("k_fft_pix" if family == "k_fft" else family + "+k_waterfall"), f.waterfall_kernel()
    t.rows(w, n, rate, kinds, (n, "waterfall_i16"))
    w = fused_rows(f, "f32", d_flt, nf + 1)
    t.rows(w, n, rate, fkinds, (n, "waterfall_f32"))
    print("%s n = %d: %d of %d comb rows held their maximum in two bins or more on the device (%d impulse rows, all bins equal)"
          % (family, n, t.tied, t.combs, t.impulses))
    assert t.impulses >= 5 * 3 + 2 and t.tied >= t.impulses  # three impulse rows or more in five batch calls, two single frames


def test_psd_first_maximum_on_tied_rows_under_a_cu_share():
    """n = 2048 held to two workgroups a CU: the persistent stride takes the frames, a workgroup meets the impulse in either of its
    two frame slots"""
    n, rate = 2048, 96000
    f = J.Fft(n, rate)
    raw, kinds = build_batch(n)
    reps = 1400 // len(kinds) + 1
    raw, kinds = np.concatenate([raw] * reps + [raw[:1]]), kinds * reps + kinds[:1]  # an odd count: the last workgroup holds one frame
    nf = len(kinds)
    assert nf % 2 == 1
    d_raw = J.DeviceBuffer.from_host(raw)
    free = batch(f, "i16", d_raw, nf)
    f.set_cu_share(2)
    t = Tally()
    held = batch(f, "i16", d_raw, nf)
    items, wgs = f.last_launch()
    assert items == (nf + 1) // 2 and wgs < items, (items, wgs)  # fewer workgroups than pairs of frames: the stride ran
    t.rows(held, n, rate, kinds, (n, "batch_i16 under a share"))
    assert np.array_equal(PT.u32(held), PT.u32(free))
    w = fused_rows(f, "i16", d_raw, nf)
    items, wgs = f.last_launch()
    assert f.waterfall_kernel() == "k_fft_pix" and wgs < items, (items, wgs)
    t.rows(w, n, rate, kinds, (n, "waterfall_i16 under a share"))
    assert t.tied >= t.impulses > 0
