"""GPU: checkpoints of BPSK handles (jsdr_bpsk_save / jsdr_bpsk_restore / jsdr_bpsk_state_bytes / jsdr_bpsk_blob_info).  A handle is
fed part of an input, saved and destroyed; another handle -- of another max_batch_samples, often of another stream count -- is
restored from the blob and fed the rest.  The references are the oracle fed the whole input, or an uninterrupted GPU handle
given the same calls and actions (other tests pin that handle to the oracle).  Bits, (fi, fq) trace, FECDecode rc / bit index /
bytes, the ten counters, the 18 state doubles and decoded[] must be the same, bit for bit: there is no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bpsk_checkpoint_v1.bin")
STATE = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)  # (6, 7: FFT-acquire only)
CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK", "centreBin")
HEADER, RECORD = 192, 7184


def same_counters(g, o):
    for k in CKEYS:
        assert g[k] == o[k], (k, g[k], o[k])


def same_state(g, o, fft=False):
    for i in STATE + ((6, 7) if fft else ()):
        assert g[i] == o[i], (i, g[i], o[i])


def ragged(total, cap):
    """calls that cover `total` samples: odd lengths, one sample, the 2560-sample tile, never above cap"""
    pat = [77, 1, 16384, 4099, 26, 2560, 40000, 2561]
    out, i = [], 0
    while total > 0:
        L = min(pat[i % len(pat)], cap, total)
        out.append(L)
        total -= L
        i += 1
    return out


class Run:
    """what a handle's streams gave, call by call"""

    def __init__(self, nstreams):
        self.bits = [[] for _ in range(nstreams)]
        self.trace = [[] for _ in range(nstreams)]
        self.fec = [[] for _ in range(nstreams)]

    def take(self, d, streams=None, offset=0):
        for s in (range(d.nstreams) if streams is None else streams):
            self.bits[s + offset].append(d.bits(s).copy())
            self.trace[s + offset].append(d.trace(s).copy())
            self.fec[s + offset].extend(d.fec_results(s))


def oracle_of(x, rate=96000, tuning=12000, do_fft=0, do_up=0, nsf=2):
    n = len(x) // 2
    o = O.Bpsk(rate=rate, blen=(4 * nsf if do_fft else 4), tuning=tuning, do_fft=do_fft, do_up=do_up, trace=n // max(1, rate // 9600) + 8)
    o.receive_i16(x)
    return o


def check_run_against_oracle(d, s, run, rs, o, fft=False):
    assert np.array_equal(np.concatenate(run.bits[rs]), o.bits()), "bits differ"
    assert np.array_equal(np.concatenate(run.trace[rs]), o.trace()), "(fi,fq) differ"
    fo = o.fec_results()
    assert len(run.fec[rs]) == len(fo), (len(run.fec[rs]), len(fo))
    for (rc, _, data), (orc, _, odata) in zip(run.fec[rs], fo):
        assert rc == orc and np.array_equal(data, odata)
    same_counters(d.counters(s), o.counters())
    same_state(d.state(s), o.state(), fft)
    assert np.array_equal(d.decoded(s), o.decoded())


def same_as_handle(d, s, r, rs, what):
    """stream s of d against stream rs of r, after a call both were given"""
    assert np.array_equal(d.bits(s), r.bits(rs)), what
    assert np.array_equal(d.trace(s), r.trace(rs)), what
    same_counters(d.counters(s), r.counters(rs))
    gs, ro = d.state(s), r.state(rs)
    assert np.array_equal(gs, ro), (what, gs, ro)  # all 18, 6 and 7 included
    fg, fr = d.fec_results(s), r.fec_results(rs)
    assert [(a, b) for a, b, _ in fg] == [(a, b) for a, b, _ in fr], what
    assert all(np.array_equal(x[2], y[2]) for x, y in zip(fg, fr)), what
    assert np.array_equal(d.decoded(s), r.decoded(rs)), what


def empty_last_call(d, s):
    """per-call results are not state: a restored stream reports an empty call"""
    assert len(d.bits(s)) == 0 and len(d.fec_results(s)) == 0 and len(d.trace(s)) == 0


def destroy(d):
    J.lib().jsdr_bpsk_destroy(d.h)
    d.borrowed = True  # (its __del__ must not destroy it again)


# ------------------------------------------------------------------ 1: cut points
N1 = 65536
_cache = {}


def input1():
    if "x1" not in _cache:
        _cache["x1"] = O.make_dbpsk_stream(501, 0, N1, noise_sigma=900.0)[0]
        _cache["o1"] = oracle_of(_cache["x1"])
    return _cache["x1"], _cache["o1"]


@pytest.mark.parametrize("c", [1, 25, 26, 27, 639, 640, 641, 2559, 2560, 2561, 4099, 40000])
def test_cut_points(c):
    """history not yet full (c < 26), halo not yet full (c < 640), dsCnt != 0, the 2560-sample tile edge"""
    x, o = input1()
    d_iq = J.DeviceBuffer.from_host(x)
    run = Run(1)
    a = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=1, max_batch_samples=65536)
    a.batch_i16(d_iq.ptr, 2 * N1, c)
    run.take(a)
    blob = a.save()
    assert len(blob) == a.state_bytes(1) == HEADER + RECORD
    destroy(a)
    info = J.blob_info(blob)
    assert (info["n_in"], info["n_ds"], info["nstreams"], info["kind"], info["rate"]) == (c, c // 10, 1, 0, 96000)
    b = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=1, max_batch_samples=20000)
    b.restore(blob)
    empty_last_call(b, 0)
    assert b.counters()["cntRaw"] == c
    pos = c
    for L in ragged(N1 - c, 20000):
        b.batch_i16(d_iq.ptr + 4 * pos, 2 * N1, L)
        run.take(b)
        pos += L
    check_run_against_oracle(b, 0, run, 0, o)


# ------------------------------------------------------------------ 2: both front-end paths, both input forms
def one_stream(t, max_batch, rate=96000):
    r = J.Bpsk(rate=rate, blen=8, tuning=int(t), nstreams=1, max_batch_samples=max_batch)
    if float(t) != int(t):
        r.set_tuning(float(t))
    return r


@pytest.mark.parametrize("forms", [("i16", "i16"), ("f32", "f32"), ("f32", "i16")])
def test_both_front_end_paths_and_both_input_forms(forms):
    x, _ = input1()
    xf = (x.astype(np.float32) / np.float32(32767.0)).astype(np.float32)  # (float)s / 32767f
    d_i = J.DeviceBuffer.from_host(x)
    d_f = J.DeviceBuffer.from_host(xf)

    def call(d, form, pos, L):
        if form == "i16":
            d.batch_i16(d_i.ptr + 4 * pos, 2 * N1, L)
        else:
            d.batch_f32(d_f.ptr + 8 * pos, 2 * N1, L)

    c = 4099
    names = {}
    for t in (12000, 12345.678):
        ref = one_stream(t, 40000)
        a = one_stream(t, 40000)
        call(ref, forms[0], 0, c)
        call(a, forms[0], 0, c)
        same_as_handle(a, 0, ref, 0, "before the cut")
        blob = a.save()
        destroy(a)
        b = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=1, max_batch_samples=20000)  # (adopts the blob's tuning)
        b.restore(blob)
        assert b.control()[0] == float(t)
        pos = c
        for L in ragged(N1 - c, 20000):
            call(ref, forms[1], pos, L)
            call(b, forms[1], pos, L)
            same_as_handle(b, 0, ref, 0, (t, pos, L))
            if L == 16384:
                names[t] = (ref.front_kernel_name(), b.front_kernel_name())
            pos += L
    # the fused kernel keeps the matched filter's 64 samples in its own buffer, the three-kernel path in the dm rows: one tuning
    # took the one, one the other, before and after the cut
    fused = {"i16": "k_fm", "f32": "k_fm_f32"}[forms[1]]
    assert names[12000] == (fused, fused), names
    assert fused not in names[12345.678] and names[12345.678][0] == names[12345.678][1], names


# ------------------------------------------------------------------ 3: other decimations
@pytest.mark.parametrize("rate", [192000, 44100])
def test_other_decimations(rate):
    n, c = 32768, 4099
    assert c % (rate // 9600) != 0
    x = O.make_dbpsk_stream(503, 0, n, rate=rate, noise_sigma=900.0)[0]
    o = oracle_of(x, rate=rate)
    d_iq = J.DeviceBuffer.from_host(x)
    run = Run(1)
    a = J.Bpsk(rate=rate, blen=8, tuning=12000, nstreams=1, max_batch_samples=8192)
    a.batch_i16(d_iq.ptr, 2 * n, c)
    run.take(a)
    blob = a.save()
    destroy(a)
    b = J.Bpsk(rate=rate, blen=8, tuning=12000, nstreams=1, max_batch_samples=20000)
    b.restore(blob)
    pos = c
    for L in ragged(n - c, 20000):
        b.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        run.take(b)
        pos += L
    check_run_against_oracle(b, 0, run, 0, o)


# ------------------------------------------------------------------ 4: the register and a frame across the cut
def test_the_register_and_a_frame_across_the_cut():
    n = 1 << 20
    x = O.make_dbpsk_stream(20020109, 0, n)[0]
    o = oracle_of(x)
    hit = next(f for f in o.fec_results() if f[0] >= 0)  # (rc, 1-based index of the bit that triggered, bytes)
    B = hit[1]
    c1 = (B - 2600) * 80 + 37  # about 2600 bits before the hit
    o1 = O.Bpsk(rate=96000, blen=4, tuning=12000)
    o1.receive_i16(x[:2 * c1])
    nb1 = o1.counters()["cntBit"]
    # on the oracle alone: the hit's 5200-bit window starts before the cut and ends after it, so it cannot be decoded from bits
    # that all arrive after the restore
    assert B - 5200 < nb1 < B, (B, nb1)
    L1 = 262144
    c2 = c1 + L1
    assert nb1 + 1 <= B <= nb1 + L1 // 80 - 8  # the hit falls into the restored handle's first call
    o2 = O.Bpsk(rate=96000, blen=4, tuning=12000)
    o2.receive_i16(x[:2 * c2])
    assert o2.counters()["cntBit"] > 5200  # the second cut: more than a register's worth of bits into the stream
    d_iq = J.DeviceBuffer.from_host(x)
    run = Run(1)
    a = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=1, max_batch_samples=c1)
    a.batch_i16(d_iq.ptr, 2 * n, c1)
    run.take(a)
    blob = a.save()
    destroy(a)
    b = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=1, max_batch_samples=L1)
    b.restore(blob)
    b.batch_i16(d_iq.ptr + 4 * c1, 2 * n, L1)
    run.take(b)
    got = [f for f in b.fec_results() if f[0] >= 0]
    assert got and got[0][0] == hit[0] and got[0][1] == B - nb1 and np.array_equal(got[0][2], hit[2])
    blob2 = b.save()
    destroy(b)
    d = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=1, max_batch_samples=300000)
    d.restore(blob2)
    pos = c2
    for L in [min(300000, n - c2)] + ragged(max(0, n - c2 - 300000), 300000):
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        run.take(d)
        pos += L
    assert pos == n
    check_run_against_oracle(d, 0, run, 0, o)


# ------------------------------------------------------------------ 5: FFT-acquire
@pytest.mark.parametrize("nsf,do_up", [(2048, 0), (2048, 1), (4800, 0), (4800, 1)])
def test_fft_acquire(nsf, do_up):
    n = 16 * nsf
    x = O.make_dbpsk_stream(505, 0, n, carrier_hz=30000.0 if do_up else 13200.0, noise_sigma=700.0)[0]
    o = oracle_of(x, do_fft=1, do_up=do_up, nsf=nsf)
    d_iq = J.DeviceBuffer.from_host(x)
    run = Run(1)
    cuts = [0, nsf, 3 * nsf, n]  # after frame 1 and after frame 3
    d = None
    for k in range(3):
        # the first handle is created in FFT-acquire; the others in the tune mode, and adopt the mode with the blob
        h = J.Bpsk(rate=96000, blen=4 * nsf, tuning=12000, do_fft=1 if k == 0 else 0, do_up=do_up if k == 0 else 0, nstreams=1,
                   max_batch_samples=(2 + 3 * k) * nsf)
        if d is not None:
            blob = d.save()
            info = J.blob_info(blob)
            assert (info["do_fft"], info["do_up"], info["nsamples_per_frame"], info["n_in"]) == (1, do_up, nsf, cuts[k])
            destroy(d)
            h.restore(blob)
            assert h.control() == (12000.0, 1, do_up)
        d = h
        pos = cuts[k]
        while pos < cuts[k + 1]:
            L = min(d.max_batch, cuts[k + 1] - pos)
            d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
            run.take(d)
            pos += L
    check_run_against_oracle(d, 0, run, 0, o, fft=True)
    assert d.counters()["centreBin"] == o.counters()["centreBin"]


# ------------------------------------------------------------------ 6: a seam in the blob
def _to_fft(d):
    d.set_mode(1, 0)


def _to_tune(d):
    d.set_mode(0, 0)


@pytest.mark.parametrize("start_fft,action", [
    (0, _to_fft), (1, _to_tune), (0, lambda d: d.set_tuning(12345.678)), (0, lambda d: d.set_tuning(12010.0)),
    (0, lambda d: d.set_tuning(11990.0)), (1, lambda d: d.reconfigure(12010.0, 0, 1)),
], ids=["tune-to-fft", "fft-to-tune", "set_tuning", "plus10", "minus10", "reconfigure"])
def test_a_seam_in_the_blob(start_fft, action):
    """the action is given after call 1, the save comes BEFORE call 2, the restore goes into a fresh handle"""
    nsf = 2048
    chunks = [2 * nsf, nsf, 3 * nsf, nsf, 2 * nsf]
    n = sum(chunks)
    x = O.make_dbpsk_stream(506, 0, n, noise_sigma=700.0)[0]
    d_iq = J.DeviceBuffer.from_host(x)
    ref = J.Bpsk(rate=96000, blen=4 * nsf, tuning=12000, do_fft=start_fft, nstreams=1, max_batch_samples=3 * nsf)
    a = J.Bpsk(rate=96000, blen=4 * nsf, tuning=12000, do_fft=start_fft, nstreams=1, max_batch_samples=3 * nsf)
    for d in (ref, a):
        d.batch_i16(d_iq.ptr, 2 * n, chunks[0])
        action(d)
    blob = a.save()
    destroy(a)
    b = J.Bpsk(rate=96000, blen=4 * nsf, tuning=12000, do_fft=0, nstreams=1, max_batch_samples=5 * nsf)
    b.restore(blob)
    assert b.control() == ref.control()
    assert b.save() == blob  # the seam is still pending, and is carried again
    pos = chunks[0]
    for L in chunks[1:]:
        ref.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        b.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        same_as_handle(b, 0, ref, 0, pos)
        pos += L


# ------------------------------------------------------------------ 7: split, merge, refusal
def test_split_merge_and_refusal():
    S = 8
    chunks = [4099, 16384, 2561, 8192, 77, 4096, 2560]
    n = sum(chunks)
    xs = [O.make_dbpsk_stream(507, s, n, carrier_hz=13200.0 + 40.0 * s, noise_sigma=600.0 + 150 * s)[0] for s in range(S)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    row = 4 * n  # bytes between streams
    ref = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=S, max_batch_samples=16384)
    pos = 0
    for L in chunks[:2]:
        ref.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        pos += L
    early = ref.save(0, 3), ref.save(3, 5)
    assert ref.save() == ref.save()  # and saving changes nothing: ref goes on as the uninterrupted handle
    assert [len(b) for b in early] == [HEADER + 3 * RECORD, HEADER + 5 * RECORD]
    h3 = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=3, max_batch_samples=20000)
    h5 = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=5, max_batch_samples=9000)
    h3.restore(early[0])
    h5.restore(early[1])
    for L in chunks[2:4]:
        ref.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        h3.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        h5.batch_i16(d_iq.ptr + 3 * row + 4 * pos, 2 * n, L)
        for s in range(S):
            same_as_handle(h3 if s < 3 else h5, s if s < 3 else s - 3, ref, s, ("split", pos, s))
        pos += L
    m = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=S, max_batch_samples=17000)
    m.restore(h3.save(), 0)
    m.restore(h5.save(), 3)  # (the first restore adopted the block this one must match)
    assert m.save() == ref.save()
    for L in chunks[4:6]:
        ref.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        m.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        for s in range(S):
            same_as_handle(m, s, ref, s, ("merged", pos, s))
        pos += L
    # a blob taken at another sample count does not go into a handle that is under way, and the handle is as it was
    before = m.save()
    with pytest.raises(J.JsdrError, match="jsdr_bpsk_restore.*shared block"):
        m.restore(early[0], 0)
    assert m.save() == before
    ref.batch_i16(d_iq.ptr + 4 * pos, 2 * n, chunks[6])
    m.batch_i16(d_iq.ptr + 4 * pos, 2 * n, chunks[6])
    for s in range(S):
        same_as_handle(m, s, ref, s, ("after the refusal", s))


# ------------------------------------------------------------------ 8: tuned handles
def test_tuned_handles_split_and_merge():
    tunings = [12000, 12345.678, -500, 0, 13337.25]
    S = len(tunings)
    chunks = [4099, 16384, 2561, 8192, 77, 4096]
    n = sum(chunks)
    xs = [O.make_dbpsk_stream(508, s, n, carrier_hz=13200.0 + 300.0 * s, noise_sigma=700.0)[0] for s in range(S)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    row = 4 * n
    ref = J.BpskTuned(96000, 8, tunings, max_batch_samples=16384)
    pos = 0
    for k, L in enumerate(chunks[:2]):
        ref.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        pos += L
        if k == 0:
            ref.set_stream_tuning(2, 11990.5)  # a retune before the save: the last 26 samples keep their old factors
    ref.set_stream_tuning(4, 13347.25)  # ... and one whose first call is still to come
    blobs = ref.save(0, 2), ref.save(2, 3)
    assert J.blob_info(blobs[0])["kind"] == 1
    h2 = J.BpskTuned(96000, 8, [0.0, 0.0], max_batch_samples=20000)
    h3 = J.BpskTuned(96000, 8, [1.0, 2.0, 3.0], max_batch_samples=9000)
    h2.restore(blobs[0])
    h3.restore(blobs[1])
    assert [h2.stream_tuning(0), h2.stream_tuning(1), h3.stream_tuning(0), h3.stream_tuning(1), h3.stream_tuning(2)] == \
        [12000.0, 12345.678, 11990.5, 0.0, 13347.25]
    for L in chunks[2:4]:
        ref.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        h2.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        h3.batch_i16(d_iq.ptr + 2 * row + 4 * pos, 2 * n, L)
        for s in range(S):
            same_as_handle(h2 if s < 2 else h3, s if s < 2 else s - 2, ref, s, ("split", pos, s))
        pos += L
    ref.set_stream_tuning(1, 12355.678)
    h2.set_stream_tuning(1, 12355.678)
    m = J.BpskTuned(96000, 8, [0.0] * S, max_batch_samples=17000)
    m.restore(h2.save(), 0)
    m.restore(h3.save(), 2)
    assert m.save() == ref.save()
    for L in chunks[4:6]:
        ref.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        m.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        for s in range(S):
            same_as_handle(m, s, ref, s, ("merged", pos, s))
        pos += L
    # an ordinary handle's blob is of another kind, either way round
    o = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=4096)
    with pytest.raises(J.JsdrError, match="jsdr_bpsk_restore"):
        m.restore(o.save(), 0)
    with pytest.raises(J.JsdrError, match="jsdr_bpsk_restore"):
        o.restore(blobs[0], 0)


# ------------------------------------------------------------------ 9: the wide forms
def test_the_wide_forms():
    """2048 streams: k_tail8 carries the register over in dwords, the batch FEC form reads the log it writes"""
    S, L = 2048, 8192
    n = 2 * L
    base = [O.make_dbpsk_stream(509, s, n, carrier_hz=13200.0 + 25.0 * s, noise_sigma=500.0 + 200 * s)[0] for s in range(8)]
    rows = np.stack([base[s % 8] for s in range(S)])
    rows[S - 3:] = np.stack([base[(5 * s + 1) % 8] for s in range(3)])  # (the last three: not what their neighbours have)
    d_iq = J.DeviceBuffer.from_host(rows)
    ref = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=S, max_batch_samples=L)
    ref.batch_i16(d_iq.ptr, 2 * n, L)
    assert ref.tail_kernel_name() == "k_tail8" and ref.fec_kernel_name() == "k_fec_bits+k_vitq+k_fec_rs"
    blob = ref.save()
    assert len(blob) == HEADER + S * RECORD
    last3 = ref.save(S - 3, 3)
    assert last3[HEADER:] == blob[HEADER + (S - 3) * RECORD:]  # a range's records are the whole handle's
    b = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=S, max_batch_samples=L)
    b.restore(blob)
    c = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=3, max_batch_samples=L)
    c.restore(last3)
    for d, off in ((ref, 0), (b, 0), (c, S - 3)):
        d.batch_i16(d_iq.ptr + 4 * n * off + 4 * L, 2 * n, L)
    assert b.tail_kernel_name() == "k_tail8" and c.tail_kernel_name() == "k_tail"
    info = ref.slot_info()
    assert b.slot_info() == info
    slots = []
    for d in (ref, b):
        dev = J.DeviceBuffer(S * info["slot_bytes"])
        dev.zero()
        d.pack_slots(dev)
        d.sync()
        slots.append(dev.to_host(np.uint8))
    assert np.array_equal(slots[0], slots[1])
    assert int(np.frombuffer(slots[0][:4].tobytes(), np.int32)[0]) > 0  # (bits were sliced: the slots are not empty)
    for s in (0, 7, 1000, S - 3, S - 1):
        same_as_handle(b, s, ref, s, s)
    for s in range(3):
        same_as_handle(c, s, ref, S - 3 + s, s)
    assert b.save() == ref.save()


# ------------------------------------------------------------------ 10: format
GOLDEN_SEED, GOLDEN_N, GOLDEN_CUT = 777, 65536, 40000  # tools/make_checkpoint_golden.py


def test_format_is_canonical():
    """save -> restore into a fresh handle -> save gives the same bytes, and so do handles of different max_batch_samples"""
    n, c = 16384, 4099
    xs = [O.make_dbpsk_stream(510, s, n, noise_sigma=800.0)[0] for s in range(2)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    blobs = []
    for mb in (4099, 60000):
        d = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=mb)
        d.batch_i16(d_iq.ptr, 2 * n, c)
        blobs.append(d.save())
    assert blobs[0] == blobs[1]
    f = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=8000)
    f.restore(blobs[0])
    assert f.save() == blobs[0]
    # the calls in pieces, through the other front end's buffers (k_fm against the three-kernel path of a short call): same bytes
    d = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=4099)
    for pos, L in ((0, 4000), (4000, 99)):
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
    assert d.save() == blobs[0]


def test_golden_blob_pins_format_version_1():
    blob = open(GOLDEN, "rb").read()
    info = J.blob_info(blob)
    assert (info["version"], info["nstreams"], info["n_in"], info["record_bytes"]) == (1, 2, GOLDEN_CUT, RECORD)
    n, c = GOLDEN_N, GOLDEN_CUT
    xs = [O.make_dbpsk_stream(GOLDEN_SEED, s, n)[0] for s in range(2)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    d = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=n)
    d.restore(blob)
    assert d.save() == blob
    d.batch_i16(d_iq.ptr + 4 * c, 2 * n, n - c)
    for s in range(2):
        o = oracle_of(xs[s])
        bits, trace = d.bits(s), d.trace(s)
        assert len(bits) > 0 and np.array_equal(bits, o.bits()[len(o.bits()) - len(bits):])
        assert len(trace) == (n - c) // 10 and np.array_equal(trace, o.trace()[c // 10:])
        same_counters(d.counters(s), o.counters())
        same_state(d.state(s), o.state())
        assert np.array_equal(d.decoded(s), o.decoded())


# ------------------------------------------------------------------ 11: refusals leave the handle unchanged
def _raw_save(d, first, count, buf, cap, nbytes):
    return J.lib().jsdr_bpsk_save(d.h, first, count, buf, C.c_size_t(cap), nbytes)


def test_refusals_leave_the_handle_unchanged():
    n = 16384
    xs = [O.make_dbpsk_stream(511, s, n, noise_sigma=800.0)[0] for s in range(2)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    ref = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=8192)
    d = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=8192)
    pos = [0]

    def step(L=77):
        for h in (ref, d):
            h.batch_i16(d_iq.ptr + 4 * pos[0], 2 * n, L)
        for s in range(2):
            same_as_handle(d, s, ref, s, pos[0])
        pos[0] += L

    step(4099)
    early = d.save()
    step(2561)
    good = d.save()
    lib = J.lib()

    def refused(rc_or_call, who):
        nonlocal good
        if callable(rc_or_call):
            with pytest.raises(J.JsdrError, match=who):
                rc_or_call()
        else:
            assert rc_or_call != 0
            assert who in lib.jsdr_last_error().decode(), lib.jsdr_last_error()
        assert d.save() == good  # exactly as it was ...
        step()                   # ... and the next call is the reference's
        good = d.save()

    other_rate = J.Bpsk(rate=48000, blen=8, tuning=12000, nstreams=2, max_batch_samples=4096).save()
    other_frame = J.Bpsk(rate=96000, blen=8192, tuning=12000, nstreams=2, max_batch_samples=4096).save()
    tuned = J.BpskTuned(96000, 8, [12000.0, 12010.0], max_batch_samples=4096).save()
    refused(lambda: d.restore(other_rate), "jsdr_bpsk_restore.*rate")
    refused(lambda: d.restore(other_frame), "jsdr_bpsk_restore.*frames")
    refused(lambda: d.restore(tuned), "jsdr_bpsk_restore.*tuned")
    # ranges
    refused(lambda: d.save(1, 2), "jsdr_bpsk_save.*out of range")
    refused(lambda: d.save(-1, 1), "jsdr_bpsk_save.*out of range")
    refused(_raw_save(d, 0, 0, np.zeros(8, np.uint8).ctypes.data_as(C.c_void_p), 8, C.byref(C.c_size_t())), "jsdr_bpsk_save")
    refused(lambda: d.restore(good, 1), "jsdr_bpsk_restore.*out of range")
    refused(lambda: d.restore(good, -1), "jsdr_bpsk_restore.*out of range")
    refused(lambda: d.state_bytes(3), "jsdr_bpsk_state_bytes")
    # cap too small, null pointers
    buf = np.zeros(len(good), np.uint8)
    nb = C.c_size_t()
    refused(_raw_save(d, 0, 2, buf.ctypes.data_as(C.c_void_p), len(good) - 1, C.byref(nb)), "jsdr_bpsk_save")
    assert not buf.any()  # nothing was written
    refused(_raw_save(d, 0, 2, None, len(good), C.byref(nb)), "jsdr_bpsk_save")
    refused(_raw_save(d, 0, 2, buf.ctypes.data_as(C.c_void_p), len(good), None), "jsdr_bpsk_save")
    refused(lib.jsdr_bpsk_restore(d.h, 0, None, C.c_size_t(len(good))), "jsdr_bpsk_restore")
    refused(lib.jsdr_bpsk_state_bytes(d.h, 1, None), "jsdr_bpsk_state_bytes")
    for fn, args in (("jsdr_bpsk_save", (None, 0, 1, buf.ctypes.data_as(C.c_void_p), C.c_size_t(len(good)), C.byref(nb))),
                     ("jsdr_bpsk_restore", (None, 0, buf.ctypes.data_as(C.c_void_p), C.c_size_t(len(good)))),
                     ("jsdr_bpsk_state_bytes", (None, 1, C.byref(nb)))):
        assert getattr(lib, fn)(*args) != 0 and fn in lib.jsdr_last_error().decode()
    # damaged blobs: short, wrong magic / version / record size, a failed checksum
    def patched(off, val):
        b = bytearray(good)
        b[off] = val
        return bytes(b)
    refused(lambda: d.restore(good[:-1]), "jsdr_bpsk_restore")
    refused(lambda: d.restore(good[:7]), "jsdr_bpsk_restore")
    refused(lambda: d.restore(good[:HEADER]), "jsdr_bpsk_restore")
    refused(lambda: d.restore(good + b"\0"), "jsdr_bpsk_restore")
    refused(lambda: d.restore(patched(0, ord("X"))), "jsdr_bpsk_restore.*magic")
    refused(lambda: d.restore(patched(8, 2)), "jsdr_bpsk_restore.*version")
    refused(lambda: d.restore(patched(16, 17)), "jsdr_bpsk_restore.*record size")
    refused(lambda: d.restore(patched(HEADER + 5000, good[HEADER + 5000] ^ 1)), "jsdr_bpsk_restore.*checksum")
    refused(lambda: d.restore(patched(104, good[104] ^ 1)), "jsdr_bpsk_restore.*checksum")
    # a shared block that is not the handle's
    refused(lambda: d.restore(early), "jsdr_bpsk_restore.*shared block")
    # ... while its own goes in, and changes nothing
    d.restore(good)
    assert d.save() == good
    step()


def _fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def _forged(blob, off, fmt, val):
    """the blob with one field changed and the checksum made to fit"""
    import struct
    b = bytearray(blob)
    struct.pack_into(fmt, b, off, val)
    struct.pack_into("<Q", b, 24, _fnv1a(bytes(b[32:])))
    return bytes(b)


def test_a_forged_checksum_does_not_get_an_index_out_of_range_into_a_handle():
    """what the scheduler or a kernel would index with is range-checked behind the checksum; the handle stays as it was"""
    n = 8192
    xs = [O.make_dbpsk_stream(515, s, n, noise_sigma=800.0)[0] for s in range(2)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    ref = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=4096)
    d = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=4096)
    tref = J.BpskTuned(96000, 8, [12000.0, 12010.5], max_batch_samples=4096)
    t = J.BpskTuned(96000, 8, [12000.0, 12010.5], max_batch_samples=4096)
    for h in (ref, d, tref, t):
        h.batch_i16(d_iq.ptr, 2 * n, 4099 - 3)
    good, tgood = d.save(), t.save()
    assert d.save() == _forged(good, 104, "<d", 12000.0)  # (the forging itself is sound)
    r1 = HEADER + RECORD  # record 1
    for blob, what in ((_forged(good, r1 + 104, "<i", 8), "bit-clock"), (_forged(good, r1 + 108, "<i", -1), "bit-clock"),
                       (_forged(good, HEADER + 176, "<i", 5000), "centre bin"), (_forged(good, r1 + 140, "<i", 7), "overflow"),
                       (_forged(good, 104, "<d", 12010.0), "tuPhaseInc"), (_forged(good, 120, "<d", 0.5), "tuPhaseInc"),
                       (_forged(good, 112, "<d", float("nan")), "tuPhase"), (_forged(good, 128, "<d", 9.0), "vcoPhase")):
        with pytest.raises(J.JsdrError, match="jsdr_bpsk_restore.*" + what):
            d.restore(blob)
        assert d.save() == good
    for blob, what in ((_forged(tgood, r1 + 432 + 2 * 7, "<H", 300), "tuner index"), (_forged(tgood, r1 + 400, "<d", float("inf")), "tuned stream"),
                       (_forged(tgood, r1 + 408, "<d", 1e30), "tuned stream"), (_forged(tgood, r1 + 416, "<d", 0.25), "tuPhaseInc")):
        with pytest.raises(J.JsdrError, match="jsdr_bpsk_restore.*" + what):
            t.restore(blob)
        assert t.save() == tgood
    for h in (ref, d, tref, t):
        h.batch_i16(d_iq.ptr + 4 * 4096, 2 * n, 4096)
    for s in range(2):
        same_as_handle(d, s, ref, s, s)
        same_as_handle(t, s, tref, s, s)
    # the kernels' own time is there to be read after a save and a restore
    d.restore(d.save())
    pack_ms, unpack_ms = d.state_kernel_ms()
    assert 0.0 < pack_ms < 100.0 and 0.0 < unpack_ms < 100.0


@pytest.mark.parametrize("kind", ["channels", "mode", "live"])
def test_channel_handles_are_refused(kind):
    kw = dict(channels={}, mode=dict(do_fft=[0, 1]), live=dict(live=True))[kind]
    n = 4096
    x = O.make_dbpsk_stream(512, 0, n, noise_sigma=800.0)[0]
    d_iq = J.DeviceBuffer.from_host(x)
    pair = [J.BpskChannels(96000, 8192, [12000.0, 12010.0], max_batch_samples=2048, **kw) for _ in range(2)]
    for d in pair:
        d.batch_i16(d_iq.ptr, 2 * n, 2048)
    d = pair[0]
    blob = J.Bpsk(rate=96000, blen=8192, tuning=12000, nstreams=2, max_batch_samples=2048).save()
    with pytest.raises(J.JsdrError, match="channel handle"):  # (the binding asks jsdr_bpsk_state_bytes first: refused there)
        d.save()
    buf, nb = np.zeros(HEADER + 2 * RECORD, np.uint8), C.c_size_t()
    assert _raw_save(d, 0, 2, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(nb)) != 0 and not buf.any()
    msg = J.lib().jsdr_last_error().decode()
    assert "jsdr_bpsk_save" in msg and "channel handle" in msg, msg
    with pytest.raises(J.JsdrError, match="jsdr_bpsk_restore.*channel handle"):
        d.restore(blob)
    with pytest.raises(J.JsdrError, match="jsdr_bpsk_state_bytes.*channel handle"):
        d.state_bytes(1)
    for h in pair:
        h.batch_i16(d_iq.ptr + 4 * 2048, 2 * n, 2048)
    for ch in range(2):
        assert np.array_equal(pair[0].bits(0, ch), pair[1].bits(0, ch)) and np.array_equal(pair[0].trace(0, ch), pair[1].trace(0, ch))
        same_counters(pair[0].counters(0, ch), pair[1].counters(0, ch))
        assert np.array_equal(pair[0].state(0, ch), pair[1].state(0, ch))


def test_the_fast_variant_is_refused_both_ways():
    n = 8192
    x = O.make_dbpsk_stream(513, 0, n, noise_sigma=800.0)[0]
    d_iq = J.DeviceBuffer.from_host(x)
    pair = [J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=1, max_batch_samples=4096, variant="fast") for _ in range(2)]
    for d in pair:
        d.batch_i16(d_iq.ptr, 2 * n, 4096)
    exact = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=1, max_batch_samples=4096)
    exact.batch_i16(d_iq.ptr, 2 * n, 4096)
    blob = exact.save()
    with pytest.raises(J.JsdrError, match="FAST"):  # (the binding asks jsdr_bpsk_state_bytes first: refused there)
        pair[0].save()
    buf, nb = np.zeros(HEADER + RECORD, np.uint8), C.c_size_t()
    assert _raw_save(pair[0], 0, 1, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(nb)) != 0 and not buf.any()
    msg = J.lib().jsdr_last_error().decode()
    assert "jsdr_bpsk_save" in msg and "FAST" in msg, msg
    with pytest.raises(J.JsdrError, match="jsdr_bpsk_restore.*FAST"):
        pair[0].restore(blob)
    for d in pair:
        d.batch_i16(d_iq.ptr + 4 * 4096, 2 * n, 4096)
    assert np.array_equal(pair[0].bits(), pair[1].bits()) and np.array_equal(pair[0].trace(), pair[1].trace())
    same_counters(pair[0].counters(), pair[1].counters())
    # and a restored handle cannot become FAST, as a retuned one cannot
    f = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=1, max_batch_samples=4096)
    f.restore(exact.save())
    assert J.lib().jsdr_bpsk_set_variant(f.h, 1) != 0


# ------------------------------------------------------------------ 12: the one-stream drop-in
def test_one_stream_drop_in_through_receive():
    nsf, frames, cut = 2048, 24, 9
    n = nsf * frames
    x = O.make_dbpsk_stream(514, 0, n, noise_sigma=800.0)[0]
    o = oracle_of(x)
    run = Run(1)
    a = J.Bpsk(rate=96000, blen=4 * nsf, tuning=12000, nstreams=1)
    for k in range(cut):
        a.receive_raw(x[2 * nsf * k:2 * nsf * (k + 1)])
        run.take(a)
    blob = a.save()
    destroy(a)
    b = J.Bpsk(rate=96000, blen=4 * nsf, tuning=12000, nstreams=1)
    b.restore(blob)
    with pytest.raises(J.JsdrError, match="nothing received"):  # the snapshot is the receive calls' own: none yet on this handle
        b.snapshot()
    for k in range(cut, frames):
        b.receive_raw(x[2 * nsf * k:2 * nsf * (k + 1)])
        run.take(b)
        sn = b.snapshot()
        assert sn.frames == k - cut + 1 and list(sn.counters) == [b.counters()[key] for key in CKEYS]
    check_run_against_oracle(b, 0, run, 0, o)
