"""GPU: the BPSK scope's spectra (jsdr_bpsk_scope_spectra_i16 / _f32) -- the painter's green and cyan spectra
(FUNcubeBPSKDemod.java:270-327) for every frame of a batch call.  tests/bpsk_scope_spectra.py has the contract (spectra_of), the
Java text (literal_of) and the cases; tests/test_bpsk_scope_spectra_oracle.py holds the two to each other.

No tolerance anywhere: doubles are compared as bit patterns (any NaN equal to any NaN), integers as integers.  Every call writes
into one arena whose gaps hold a canary that must survive; the six outputs of the scope are held to a twin handle's plain scope
call, and bits, counters, state, trace and FEC results to a second twin's batch call."""
import gc

import numpy as np
import pytest

import bpsk_scope as B
import bpsk_scope_spectra as SP
import java_sdr_amd as J
import test_gpu_bpsk_scope as G

pytestmark = pytest.mark.gpu

F64 = np.float64
OLD, NEW = B.OUTPUTS, SP.NEW
ALL = OLD + NEW


def form_of(length):
    """the kernel that takes a row of `length` points"""
    if length & (length - 1) == 0:
        return "k_bpsk_spec_pow2"
    return "k_bpsk_spec_mixed64" if length <= 512 else "k_bpsk_spec_mixed256" if length <= 2048 else "k_bpsk_spec_mixed768"


def kernels_of(outs, n, ring):
    t, d = bool({"tspec", "tpeak", "tpsd"} & set(outs)), bool({"dspec", "dpeak", "dpsd"} & set(outs))
    front = bool({"tuned", "ds"} & set(outs)) or (t and "tuned" not in outs) or (d and "ds" not in outs)
    own_only = front and not ({"tuned", "ds"} & set(outs))
    return "+".join(["k_bpsk_scope_front"] * (front and not own_only) + ["k_bpsk_scope_walk"] * bool({"pts", "bits"} & set(outs)) +
                    ["k_bpsk_scope_pts"] * bool({"iq", "max", "pts"} & set(outs)) + ["k_bpsk_scope_front"] * own_only +
                    [form_of(n)] * t + [form_of(ring)] * d)


def spectra_call(h, form, data, L, outs=ALL, Wp=749, ic=0, qc=0, what=None):
    """one spectra call over data [S][2L]: name -> rows, for the outputs asked for"""
    S, n = h.nstreams, h.samples
    rows = S * (L // n)
    ring = h.scope_layout(L)[0]
    d_in, stride = G.upload(form, data, L)
    size = dict(tuned=16 * rows * n, ds=16 * rows * ring, iq=16 * rows * ring, max=16 * rows, pts=16 * rows * ring, bits=rows * ring,
                tspec=4 * rows * Wp, tpeak=16 * rows, tpsd=8 * rows * n, dspec=4 * rows * Wp, dpeak=16 * rows, dpsd=8 * rows * ring)
    ar = G.Arena({k: size[k] * (k in outs) for k in ALL})
    kw = {k: ar.ptr(k) for k in ALL}
    if form == "i16":
        h.scope_spectra_i16(d_in, stride, L, ic, qc, plot_width=Wp, **kw)
    else:
        h.scope_spectra_f32(d_in, stride, L, plot_width=Wp, **kw)
    h.sync()
    raw = ar.read((what, form, outs))
    shape = dict(tuned=(F64, (rows, n, 2)), ds=(F64, (rows, ring, 2)), iq=(F64, (rows, ring, 2)), max=(F64, (rows, 2)),
                 pts=(np.int32, (rows, ring, 4)), bits=(np.int8, (rows, ring)), tspec=(np.int32, (rows, Wp)), tpeak=(F64, (rows, 2)),
                 tpsd=(F64, (rows, n)), dspec=(np.int32, (rows, Wp)), dpeak=(F64, (rows, 2)), dpsd=(F64, (rows, ring)))
    got = {k: raw[k].view(shape[k][0]).reshape(shape[k][1]) for k in outs}
    assert h.scope_kernel() == kernels_of(outs, n, ring), (what, h.scope_kernel(), outs)
    return got


def want_of(tuned, ds, Wp):
    """spectra_of over rows [rows][len][2]: name -> rows of the six new outputs"""
    t = [SP.spectra_of(r, Wp) for r in tuned]
    d = [SP.spectra_of(r, Wp) for r in ds]
    return dict(tspec=np.stack([x["spec"] for x in t]), tpeak=np.stack([x["peak"] for x in t]), tpsd=np.stack([x["psd"] for x in t]),
                dspec=np.stack([x["spec"] for x in d]), dpeak=np.stack([x["peak"] for x in d]), dpsd=np.stack([x["psd"] for x in d]))


def differ(got, want, outs):
    bad = []
    for k in outs:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        ok = B.same(a, b) if a.dtype == F64 else np.array_equal(a, b)
        if not ok:
            neq = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b)) if a.dtype == F64 else (a != b)
            bad.append((k, int(neq.sum()), np.argwhere(neq)[:3].tolist()))
    return bad


def make(case, S, nf, **kw):
    c = SP.CASES[case]
    return J.Bpsk(rate=c["rate"], blen=4 * c["n"], size=4, tuning=c["tuning"], nstreams=S, max_batch_samples=nf * c["n"], **kw)


def inputs(case, S):
    ins = [SP.case_input(case, s) for s in range(S)]
    return ins[0][0], np.stack([d for _, d in ins])


# ---------------------------------------------------------------------------------------------------------------- 1. every case
@pytest.mark.parametrize("case,Wp", [(c, w) for c in SP.CASES for w in SP.widths(c)])
def test_every_row_of_every_case(case, Wp):
    """3 streams, two consecutive calls of half the case's frames each, all twelve outputs: the new rows are spectra_of the call's
    own tuned / ds rows, which are the oracle's rows; the old rows are a twin's scope call; the demodulator is a twin's batch call"""
    c = SP.CASES[case]
    n, S, total = c["n"], 3, SP.frames_of(case)
    nf = max(total // 2, 1)
    form, data = inputs(case, S)
    h, scoped, plain = make(case, S, nf), make(case, S, nf), make(case, S, nf)
    oracle = [SP.run_case(case, s) for s in range(S)]
    ring = B.ring_len(c["rate"], n)
    for k in range(total // nf):
        chunk = np.ascontiguousarray(data[:, 2 * k * nf * n:2 * (k + 1) * nf * n])
        tag = (case, Wp, "call", k)
        got = spectra_call(h, form, chunk, nf * n, ALL, Wp, what=tag)
        old = G.scope_call(scoped, form, chunk, nf * n, what=tag)
        assert not G.differ(got, old), (tag, G.differ(got, old))
        G.batch_call(plain, form, chunk, nf * n)
        G.twins_agree(h, plain, tag)
        orows = {name: np.concatenate([o[name][k * nf:(k + 1) * nf] for o in oracle]) for name in ("tuned", "ds")}
        assert B.same(got["tuned"], orows["tuned"]) and B.same(got["ds"], orows["ds"]), tag  # (the oracle's rows ARE the call's)
        bad = differ(got, want_of(got["tuned"], got["ds"], Wp), NEW)
        assert not bad, (tag, bad)
    assert h.scope_kernel().endswith(form_of(n) + "+" + form_of(ring)), (case, h.scope_kernel())
    census = SP.load_census()[case]
    if case == "impulse":
        assert census["t"]["frames_with_tied_max"] >= 1
    if case == "silence":
        assert not got["tpeak"].any() and not got["dspec"].any()


def test_the_kernel_forms_by_case():
    want = {"96k": ("k_bpsk_spec_pow2", "k_bpsk_spec_mixed64"), "48k": ("k_bpsk_spec_mixed768", "k_bpsk_spec_mixed256"),
            "44k1": ("k_bpsk_spec_mixed768", "k_bpsk_spec_mixed256"), "r192k": ("k_bpsk_spec_pow2", "k_bpsk_spec_mixed64"),
            "r48k_2048": ("k_bpsk_spec_pow2", "k_bpsk_spec_mixed64"), "p1024": ("k_bpsk_spec_pow2", "k_bpsk_spec_mixed64"),
            "p8192": ("k_bpsk_spec_pow2", "k_bpsk_spec_mixed256")}
    for case, forms in want.items():
        c = SP.CASES[case]
        assert (form_of(c["n"]), form_of(B.ring_len(c["rate"], c["n"]))) == forms, case


# ---------------------------------------------------------------------------------------------------------------- 2. live control
def test_two_calls_then_set_tuning_then_reconfigure():
    """the rows of the scope are pinned to the Java text through both actions by test_gpu_bpsk_scope.py: here the spectra are held
    to the rows of the same call, and the old outputs and the demodulator to the twins, through the same actions"""
    case, S, nf, Wp = "96k", 2, 2, 749
    n = SP.CASES[case]["n"]
    data = np.stack([B.case_input(case, s)[1] for s in range(S)])
    h, scoped, plain = make(case, S, nf), make(case, S, nf), make(case, S, nf)
    for k, act in enumerate(("first", "second", "set_tuning", "after", "reconfigure")):
        for hh in (h, scoped, plain):
            if act == "set_tuning":
                hh.set_tuning(11990.0)
            if act == "reconfigure":
                hh.reconfigure(12003.0, 0, 0)
        chunk = np.ascontiguousarray(data[:, 2 * k * nf * n:2 * (k + 1) * nf * n])
        outs = ALL if k % 2 == 0 else OLD[2:] + ("tspec", "tpeak", "dspec", "dpeak")  # (odd calls: the handle's own rows)
        got = spectra_call(h, "i16", chunk, nf * n, outs, Wp, what=act)
        old = G.scope_call(scoped, "i16", chunk, nf * n, what=act)
        assert not G.differ(got, old, [o for o in outs if o in OLD]), act
        G.batch_call(plain, "i16", chunk, nf * n)
        G.twins_agree(h, plain, act)
        bad = differ(got, want_of(old["tuned"], old["ds"], Wp), [o for o in outs if o in NEW])
        assert not bad, (act, bad)


# ---------------------------------------------------------------------------------------------------------------- 3. many streams
def test_2048_streams_under_k_tail8():
    """2048 streams x 2 frames, the handle's own rows (512 MiB of tuned rows would be the caller's otherwise): two passes of one
    frame at the default bound; three distinct signals go round the streams"""
    S, nf, n, Wp = 2048, 2, 2048, 749
    base = [B.case_input("96k", s)[1][:2 * nf * n] for s in range(3)]
    which = np.arange(S) % 3
    h = J.Bpsk(rate=96000, blen=4 * n, size=4, tuning=12000, nstreams=S, max_batch_samples=nf * n)
    outs = ("tspec", "tpeak", "dspec", "dpeak", "dpsd")
    got = spectra_call(h, "i16", np.stack(base)[which], nf * n, outs, Wp, what="2048 streams")
    assert h.tail_kernel_name() == "k_tail8"
    for j in range(3):
        o = SP.run_case("96k", j)
        want = want_of(o["tuned"][:nf], o["ds"][:nf], Wp)
        rows = (np.flatnonzero(which == j)[:, None] * nf + np.arange(nf)[None, :]).ravel()
        tiled = {k: np.tile(want[k], (len(rows) // nf,) + (1,) * (want[k].ndim - 1)) for k in outs}
        bad = differ({k: got[k][rows] for k in outs}, tiled, outs)
        assert not bad, (j, bad)


# ---------------------------------------------------------------------------------------------------------------- 4. NULL outputs, both row paths
def test_each_new_output_alone_with_and_without_the_rows():
    case, S, nf, Wp = "96k", 2, 2, 100
    n = SP.CASES[case]["n"]
    data = np.stack([B.case_input(case, s)[1][:2 * 2 * nf * n] for s in range(S)])
    ref = None
    sets = [ALL, ()] + [(k,) for k in NEW] + [("tuned", "ds", k) for k in NEW] + [("ds", "tspec", "dpeak"), ("tuned", "tpsd", "dspec")]
    for outs in sets:
        h = make(case, S, nf)
        G.batch_call(h, "i16", data[:, :2 * nf * n], nf * n)  # (the spectra call is the second: it starts from carried state)
        before = J.live_resources()
        got = spectra_call(h, "i16", data[:, 2 * nf * n:], nf * n, outs, Wp, what=("outputs", outs))
        if ref is None:
            ref = got
            ref_bits = [h.bits(s).copy() for s in range(S)]
        assert not differ(got, ref, outs), outs
        assert all(np.array_equal(h.bits(s), ref_bits[s]) for s in range(S)), outs
        if not outs:  # the batch call: nothing launched, nothing allocated
            assert h.scope_kernel() == "" and J.live_resources() == before


def test_with_the_new_outputs_null_it_is_the_scope_call_launch_for_launch():
    case, S, nf = "96k", 2, 2
    n = SP.CASES[case]["n"]
    data = np.stack([B.case_input(case, s)[1][:2 * nf * n] for s in range(S)])
    a, b = make(case, S, nf), make(case, S, nf)
    start = J.live_resources()
    got = spectra_call(a, "i16", data, nf * n, OLD, 749, what="old outputs alone")
    held = J.live_resources()
    old = G.scope_call(b, "i16", data, nf * n, what="the scope call")
    assert not G.differ(got, old) and a.scope_kernel() == b.scope_kernel()
    assert tuple(y - x for x, y in zip(start, held)) == tuple(y - x for x, y in zip(held, J.live_resources()))


# ---------------------------------------------------------------------------------------------------------------- 5. passes of frames
def test_scope_chunk_of_one_and_of_three_frames_against_the_default():
    case, S, nf, Wp = "96k", 3, 5, 749
    n = SP.CASES[case]["n"]
    data = np.stack([B.case_input(case, s)[1][:2 * 2 * nf * n] for s in range(S)])
    outs = ("tspec", "tpeak", "tpsd", "dspec", "dpeak", "dpsd")
    ref = None
    for chunk in (0, 1, 3):
        h = make(case, S, nf)
        h.scope_chunk(chunk)
        first = spectra_call(h, "i16", data[:, :2 * nf * n], nf * n, outs, Wp, what=("chunk", chunk, 0))
        second = spectra_call(h, "i16", data[:, 2 * nf * n:], nf * n, outs, Wp, what=("chunk", chunk, 1))
        if ref is None:
            ref = (first, second)
            full = spectra_call(make(case, S, nf), "i16", data[:, :2 * nf * n], nf * n, ALL, Wp, what="caller rows")
            assert not differ(first, full, outs)
        assert not differ(first, ref[0], outs) and not differ(second, ref[1], outs), chunk
    with pytest.raises(J.JsdrError):
        h.scope_chunk(-1)


# ---------------------------------------------------------------------------------------------------------------- 6. resources
def test_resources_allocated_once_and_gone_with_the_handle():
    case, S, nf = "96k", 1, 2
    n = SP.CASES[case]["n"]
    data = np.stack([B.case_input(case, 0)[1][:2 * nf * n]])
    gc.collect()
    start = J.live_resources()
    h = make(case, S, nf)
    G.scope_call(h, "i16", data, nf * n, what="the scope call")
    scoped = J.live_resources()
    outs = ("tspec", "dpeak")
    spectra_call(h, "i16", data, nf * n, outs, 749, what="spectra")
    held = J.live_resources()
    assert held[0] >= scoped[0] + 4 and held[1] > scoped[1], (scoped, held)  # two tables, two row buffers
    spectra_call(h, "i16", data, nf * n, outs, 749, what="spectra again")
    assert J.live_resources() == held  # allocated once
    del h
    gc.collect()
    assert J.live_resources() == start


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def _refused(fn, word):
    with pytest.raises(J.JsdrError) as e:
        fn()
    assert word in str(e.value), (word, str(e.value))


def test_refusals_leave_the_handle_as_it_was():
    case, S, nf = "96k", 2, 2
    n = SP.CASES[case]["n"]
    L = nf * n
    data = np.stack([B.case_input(case, s)[1][:2 * 2 * L] for s in range(S)])
    h, twin = make(case, S, nf), make(case, S, nf)
    G.batch_call(h, "i16", data[:, :2 * L], L)
    G.batch_call(twin, "i16", data[:, :2 * L], L)
    d_in, stride = G.upload("i16", data[:, 2 * L:], L)
    out = J.DeviceBuffer(16 * S * nf * n + 64)
    p = out.ptr
    assert p % 16 == 0
    for kw, word in ((dict(tspec=p, plot_width=0), "plot_width=0 outside 1 .. 32768"),
                     (dict(dspec=p, plot_width=32769), "plot_width=32769 outside 1 .. 32768"),
                     (dict(tspec=p + 2, plot_width=749), "tspec_dev is not aligned to 4"),
                     (dict(dspec=p + 2, plot_width=749), "dspec_dev is not aligned to 4"),
                     (dict(tpeak=p + 8), "tpeak_dev or tpsd_dev is not aligned to 16"),
                     (dict(tpsd=p + 8), "tpeak_dev or tpsd_dev is not aligned to 16"),
                     (dict(dpeak=p + 8), "dpeak_dev or dpsd_dev is not aligned to 16"),
                     (dict(dpsd=p + 8), "dpeak_dev or dpsd_dev is not aligned to 16"),
                     (dict(ds=p + 8, dpeak=p), "ds_dev is not aligned to 16"),
                     (dict(tuned=p + 8, tpeak=p), "tuned_dev is not aligned to 16")):
        _refused(lambda: h.scope_spectra_i16(d_in, stride, L, **kw), word)
        _refused(lambda: h.scope_spectra_f32(d_in, stride, L, **kw), word)
    _refused(lambda: h.scope_spectra_i16(d_in, stride, L - 1, tpeak=p), "not whole frames")
    _refused(lambda: h.scope_spectra_i16(None, stride, L, tpeak=p), "null input")
    h.scope_spectra_i16(d_in, stride, L, plot_width=0, tpeak=p)  # (the width is the columns' alone)
    G.batch_call(twin, "i16", data[:, 2 * L:], L)
    G.twins_agree(h, twin, "after the refusals and a call")
    # a row length that no kernel serves: n = 16384 (above the LDS image), L = 1638 is served
    big = J.Bpsk(rate=96000, blen=4 * 16384, size=4, tuning=12000, nstreams=1, max_batch_samples=16384)
    src = J.DeviceBuffer.from_host(np.zeros(2 * 16384, np.int16))
    untouched = big.counters(0)
    _refused(lambda: big.scope_spectra_i16(src, 2 * 16384, 16384, tpeak=p), "no spectrum kernel serves the tuned rows of 16384 points")
    assert big.scope_kernel() == "" and big.counters(0) == untouched
    big.scope_spectra_i16(src, 2 * 16384, 16384, dpeak=p)
    assert big.scope_kernel() == "k_bpsk_scope_front+k_bpsk_spec_mixed256"
    # the kinds of handle that have no scope have no spectra
    _refused(lambda: make(case, S, nf, variant="fast").scope_spectra_i16(d_in, stride, L, tpeak=p), "fast variant")
    fft = J.Bpsk(rate=96000, blen=4 * n, size=4, tuning=12000, do_fft=1, nstreams=S, max_batch_samples=L)
    _refused(lambda: fft.scope_spectra_i16(d_in, stride, L, tpeak=p), "do_fft is set or a mode switch is pending")
    _refused(lambda: J.BpskTuned(96000, 4 * n, [12000.0, 12010.0], L).scope_spectra_i16(d_in, stride, L, tpeak=p), "tuned handle")
    _refused(lambda: J.BpskChannels(96000, 4 * n, [12000.0, 12010.0], max_batch_samples=L).scope_spectra_i16(d_in, stride, L, tpeak=p),
             "channel handle")
