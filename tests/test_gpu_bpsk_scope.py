"""GPU: the BPSK scope (jsdr_bpsk_scope_i16 / _f32) -- the five debug rings of FUNcubeBPSKDemod and the painter's first panel for
every frame of a batch call.  tests/bpsk_scope.py has the restatement, the literal Java text and the cases;
tests/test_bpsk_scope_oracle.py holds the two to each other and counts what the cases contain.

No tolerance anywhere: doubles are compared as bit patterns (any NaN equal to any NaN), integers as integers.  Every call writes
into one arena whose gaps -- before, between and after the six outputs -- hold a canary that must survive, reads its input from
rows padded with poison, and is followed on a twin handle by the plain batch call, which must leave the same bits, counters,
state, trace and FEC results."""
import gc

import numpy as np
import pytest

import bpsk_scope as B
import java_sdr_amd as J
import oracle_lib as O

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
PAD = 6
GAP = 64
CANARY = 0xA5
ALL = B.OUTPUTS


class Arena:
    """one device buffer: canary, region, canary, region, .. canary; a region of 0 bytes is a NULL pointer"""

    def __init__(self, sizes):
        self.off, at = {}, GAP
        for name, nbytes in sizes.items():
            self.off[name] = (at, nbytes)
            at += (nbytes + GAP - 1) // GAP * GAP + GAP
        self.total = at
        self.buf = J.DeviceBuffer.from_host(np.full(at, CANARY, np.uint8))

    def ptr(self, name):
        at, nbytes = self.off[name]
        return self.buf.ptr + at if nbytes else None

    def read(self, what):
        host = self.buf.to_host(np.uint8)
        keep = np.ones(self.total, bool)
        out = {}
        for name, (at, nbytes) in self.off.items():
            keep[at:at + nbytes] = False
            out[name] = host[at:at + nbytes].copy()
        assert (host[keep] == CANARY).all(), (what, "a canary outside the outputs was written", np.flatnonzero(keep & (host != CANARY))[:8])
        return out


def upload(form, data, L):
    """data [S][2L] into rows padded by PAD elements of poison: (device buffer, stride)"""
    S = data.shape[0]
    stride = 2 * L + PAD
    src = np.full((S, stride), 32767, np.int16) if form == "i16" else np.full((S, stride), np.nan, F32)
    src[:, :2 * L] = data
    return J.DeviceBuffer.from_host(src), stride


def scope_call(h, form, data, L, outs=ALL, ic=0, qc=0, what=None):
    """one scope call over data [S][2L] (int16 for "i16", float32 for "f32"): name -> rows, for the outputs asked for"""
    S, n = h.nstreams, h.samples
    rows = S * (L // n)
    ring = h.scope_layout(L)[0]
    d_in, stride = upload(form, data, L)
    size = dict(tuned=16 * rows * n, ds=16 * rows * ring, iq=16 * rows * ring, max=16 * rows, pts=16 * rows * ring, bits=rows * ring)
    ar = Arena({k: size[k] * (k in outs) for k in ALL})
    kw = {k: ar.ptr(k) for k in ALL}
    if form == "i16":
        h.scope_i16(d_in, stride, L, ic, qc, **kw)
    else:
        h.scope_f32(d_in, stride, L, **kw)
    h.sync()
    raw = ar.read((what, form, outs))
    shape = dict(tuned=(F64, (rows, n, 2)), ds=(F64, (rows, ring, 2)), iq=(F64, (rows, ring, 2)), max=(F64, (rows, 2)),
                 pts=(np.int32, (rows, ring, 4)), bits=(np.int8, (rows, ring)))
    got = {k: raw[k].view(shape[k][0]).reshape(shape[k][1]) for k in outs}
    want = "+".join(["k_bpsk_scope_front"] * bool({"tuned", "ds"} & set(outs)) + ["k_bpsk_scope_walk"] * bool({"pts", "bits"} & set(outs)) +
                    ["k_bpsk_scope_pts"] * bool({"iq", "max", "pts"} & set(outs)))
    assert h.scope_kernel() == want, (what, h.scope_kernel(), outs)
    return got


def batch_call(h, form, data, L, ic=0, qc=0):
    d_in, stride = upload(form, data, L)
    if form == "i16":
        h.batch_i16(d_in, stride, L, ic, qc)
    else:
        h.batch_f32(d_in, stride, L)
    h.sync()


def differ(got, want, outs=ALL):
    bad = []
    for k in outs:
        ok = B.same(got[k], want[k]) if k in ("tuned", "ds", "iq", "max") else np.array_equal(got[k], want[k])
        if not ok:
            a, b = np.asarray(got[k]), np.asarray(want[k])
            neq = (a.view(np.uint64) != b.view(np.uint64)) if a.dtype == F64 else (a != b)
            if a.dtype == F64:
                neq &= ~(np.isnan(a) & np.isnan(b))
            bad.append((k, int(neq.sum()), np.argwhere(neq)[:3].tolist()))
    return bad


def twins_agree(h, twin, what):
    for s in range(h.nstreams):
        assert h.counters(s) == twin.counters(s), (what, s, "counters", h.counters(s), twin.counters(s))
        assert np.array_equal(h.bits(s), twin.bits(s)), (what, s, "bits")
        assert B.same(h.state(s), twin.state(s)), (what, s, "state")
        assert B.same(h.trace(s), twin.trace(s)), (what, s, "trace")
        a, b = h.fec_results(s), twin.fec_results(s)
        assert len(a) == len(b) and all(x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) for x, y in zip(a, b)), (what, s, "fec")


class Rig:
    """a scoped handle, its twin that only takes batch calls, and the restatement of every stream"""

    def __init__(self, case, S, frames_per_call, form=None, ic=0, qc=0):
        c = B.CASES[case]
        self.case, self.c, self.S, self.n, self.rate = case, c, S, c["n"], c["rate"]
        ins = [B.case_input(case, s) for s in range(S)]
        self.form = form or ins[0][0]
        self.ic, self.qc = ic, qc
        if self.form == "f32":
            self.data = np.stack([B.as_float(f, d) for f, d in ins])
            self.floats = self.data
        else:
            self.data = np.stack([d for _, d in ins])
            self.floats = np.stack([O.convert_i16(d, ic=ic, qc=qc) for d in self.data])
        mk = lambda: J.Bpsk(rate=self.rate, blen=4 * self.n, size=4, tuning=c["tuning"], nstreams=S,  # noqa: E731
                            max_batch_samples=frames_per_call * self.n)
        self.h, self.twin = mk(), mk()
        self.r = [B.Restated(self.rate, self.n, c["tuning"], c["frames"]) for _ in range(S)]
        self.t = B.Tuner(c["tuning"], self.rate)
        self.frame = 0
        self.origin = 0

    def call(self, nf, outs=ALL, what=None):
        n, L, f0 = self.n, nf * self.n, self.frame
        chunk = np.ascontiguousarray(self.data[:, 2 * f0 * n:2 * (f0 + nf) * n])
        for f in range(f0, f0 + nf):
            idx = self.t.step(n)
            for s in range(self.S):
                self.r[s].receive(self.floats[s, 2 * f * n:2 * (f + 1) * n], idx)
        self.frame += nf
        tag = (what, self.case, self.form, "frames", f0, f0 + nf)
        ring, origin, G = self.h.scope_layout(L)
        assert ring == self.r[0].L and origin == self.origin and np.array_equal(G, B.g_first(self.rate, n, f0 * n, nf, self.origin)), tag
        got = scope_call(self.h, self.form, chunk, L, outs, self.ic, self.qc, tag)
        per = [r.rows(f0, nf, self.origin) for r in self.r]
        want = {k: np.concatenate([p[k] for p in per]) for k in ALL}
        bad = differ(got, want, outs)
        assert not bad, (tag, bad)
        batch_call(self.twin, self.form, chunk, L, self.ic, self.qc)
        twins_agree(self.h, self.twin, tag)
        for s in range(self.S):
            assert self.h.counters(s)["cntBit"] == self.r[s].o.counters()["cntBit"], (tag, s)
        return got, G


def marks_of(bits, g, G, ring):
    """the demodBits rows of a call's frames from the call's get_bits and the g of every bit (relative to the origin, ascending):
    zero, then slot (g + 1) mod L of the bit's frame takes the bit, a later one over an earlier one"""
    rows = np.zeros((len(G) - 1, ring), np.int8)
    f = np.searchsorted(G, g, side="right") - 1
    for k in range(len(g)):
        rows[f[k], (g[k] + 1) % ring] = bits[k]
    return rows


# ---------------------------------------------------------------------------------------------------------------- 1. the rows
@pytest.mark.parametrize("form,ic,qc", [("i16", 0, 0), ("i16", 300, -200), ("f32", 0, 0)])
def test_every_row_at_96k_over_consecutive_calls(form, ic, qc):
    """3 streams x 4 frames, three calls: G_f leaves the origin and the 204 / 205 pattern turns"""
    rig = Rig("96k", 3, 4, form, ic, qc)
    seen = set()
    for k in range(3):
        got, G = rig.call(4, what="96k")
        seen |= set(np.diff(G).tolist())
        for s in range(3):  # the bits rows are get_bits of the call, placed by the g of every bit
            dec_g, dec = rig.r[s].o.declog_pos()
            g = dec_g[dec[:, 1] > 100.0]
            g = g[(g >= G[0]) & (g < G[-1])]
            bits = rig.h.bits(s)
            assert len(g) == len(bits) > 0, (k, s)
            assert np.array_equal(got["bits"][4 * s:4 * s + 4], marks_of(bits, g, G, 204)), (k, s, "bits rows against get_bits")
    assert seen == {204, 205}
    assert rig.h.tail_kernel_name() == "k_tail"


@pytest.mark.parametrize("form", ["i16", "f32"])
@pytest.mark.parametrize("case", ["44k1", "48k"])
def test_every_row_at_the_other_rates(case, form):
    """2 streams x 2 frames, two calls: L = 960 against 1102 / 1103 outputs (slots marked twice) and against 960"""
    rig = Rig(case, 2, 2, form)
    for k in range(2):
        rig.call(2, what=case)


@pytest.mark.parametrize("case", ["silence", "untuned", "tiny_i", "nan"])
def test_the_edge_cases(case):
    """silence (mi == 0: Infinity and NaN in the painter), no tuner at all, (int)(Q * xs) saturating, a NaN inside a frame"""
    rig = Rig(case, 2, 2)
    for k in range(B.CASES[case]["frames"] // 2):
        got, _ = rig.call(2, what=case)
    c = B.load_census()[case]
    if case == "silence":
        assert not got["max"].any() and not got["pts"].any() and not got["bits"].any() and c["frames_with_mi_zero"] == 3
    if case == "tiny_i":
        assert (np.abs(got["pts"][:, :, 2].astype(np.int64)) >= B.INT_MAX).any() and c["pts_saturated"] >= 1
    if case == "nan":
        assert c["nan_slots"] >= 1


def test_a_fec_block_decoded_inside_a_scoped_call():
    rig = Rig("fec", 1, 6)
    decoded, hits = [], []
    for k in range(8):
        rig.call(6, what="fec")
        decoded.append(rig.h.counters(0)["cntDec"])
        hits.append(len(rig.h.fec_results(0)))
    assert decoded[-1] >= 1 and decoded[0] == 0 and B.load_census()["fec"]["fec_decoded"] == decoded[-1]
    assert sum(hits) >= 1 and hits[0] == 0  # the block was decoded inside one of the scoped calls


def test_scope_calls_of_the_two_input_forms_alternate_on_one_handle():
    """the 26 samples before a call come from the half of the input history the call did not write -- behind a call of the other
    form that is the half the conversion has just filled.  The floats are (float)s / 32767f values: the int16 form takes over from them"""
    rig = Rig("96k", 2, 2, "i16")
    raw, flt = rig.data, rig.floats
    for form in ("i16", "f32", "f32", "i16", "f32"):
        rig.form, rig.data = form, (raw if form == "i16" else flt)
        rig.call(2, what="alternating forms")


# ---------------------------------------------------------------------------------------------------------------- 2. live control
def test_after_set_tuning_after_reconfigure_and_on_a_restored_handle():
    """the Java text takes the same actions: a retune (tuPhaseInc alone), setup (the rings' indices: the origin moves), and a
    handle restored from a blob, whose origin is 0 again"""
    rate, n, nf = 96000, 2048, 2
    D, ring = rate // 9600, B.ring_len(rate, n)
    form, data = B.case_input("96k", 2)
    x = B.as_float(form, data)
    h = J.Bpsk(rate=rate, blen=4 * n, size=4, tuning=12000, nstreams=1, max_batch_samples=nf * n)
    twin = J.Bpsk(rate=rate, blen=4 * n, size=4, tuning=12000, nstreams=1, max_batch_samples=nf * n)
    lit = B.Literal(rate, n, 12000)
    origin, frame = 0, 0

    def call(hh, what, org):
        nonlocal frame
        want = []
        for f in range(frame, frame + nf):
            lit.receive(x[2 * f * n:2 * (f + 1) * n])
            rows = lit.rows()
            placed = B.rows_of(ring, (f * n) // D, ((f + 1) * n) // D, org, *lit.logs(), rows["tuned"])
            if org == origin:
                assert not B.rows_equal(placed, rows), (what, f, "the restatement over the Java text's instruments")
            want.append(placed)
        chunk = data[None, 2 * frame * n:2 * (frame + nf) * n]
        assert hh.scope_layout(nf * n)[1] == org, what
        got = scope_call(hh, "i16", chunk, nf * n, what=what)
        bad = differ(got, {k: np.stack([w[k] for w in want]) for k in ALL})
        assert not bad, (what, bad)
        if hh is h:
            batch_call(twin, "i16", chunk, nf * n)
            twins_agree(h, twin, what)
        frame += nf

    call(h, "before", 0)
    for hh in (h, twin):
        hh.set_tuning(11990.0)
    lit.action(11990.0)
    call(h, "after set_tuning", 0)
    call(h, "the call after that", 0)
    for hh in (h, twin):
        hh.reconfigure(12003.0, 0, 0)
    lit.setup(12003)
    origin = (frame * n) // D
    assert origin % ring != 0
    call(h, "after reconfigure", origin)
    blob = h.save()
    fresh = J.Bpsk(rate=rate, blen=4 * n, size=4, tuning=12000, nstreams=1, max_batch_samples=nf * n)
    fresh.restore(blob)
    call(fresh, "restored", 0)  # (the blob does not carry the origin)


# ---------------------------------------------------------------------------------------------------------------- 3. many streams
def test_2048_streams_take_the_k_tail8_side():
    """2048 streams x 2 frames, two calls (the second starts from a clock state that is not the initial one); three distinct
    signals go round the streams; tuned is left out"""
    S, nf, n, ring = 2048, 2, 2048, 204
    base = [B.case_input("96k", s)[1] for s in range(3)]
    h = J.Bpsk(rate=96000, blen=4 * n, size=4, tuning=12000, nstreams=S, max_batch_samples=nf * n)
    r = [B.Restated(96000, n, 12000, 4) for _ in range(3)]
    t = B.Tuner(12000, 96000)
    outs = ("ds", "iq", "max", "pts", "bits")
    which = np.arange(S) % 3
    for k in range(2):
        for f in range(k * nf, (k + 1) * nf):
            idx = t.step(n)
            for j in range(3):
                r[j].receive(O.convert_i16(base[j][2 * f * n:2 * (f + 1) * n]), idx)
        chunk = np.stack([b[2 * k * nf * n:2 * (k + 1) * nf * n] for b in base])[which]
        got = scope_call(h, "i16", chunk, nf * n, outs, what=("2048 streams", k))
        assert h.tail_kernel_name() == "k_tail8"
        per = [x.rows(k * nf, nf) for x in r]
        for j in range(3):
            rows = (np.flatnonzero(which == j)[:, None] * nf + np.arange(nf)[None, :]).ravel()
            want = {name: np.tile(per[j][name], (len(rows) // nf,) + (1,) * (per[j][name].ndim - 1)) for name in outs}
            bad = differ({name: got[name][rows] for name in outs}, want, outs)
            assert not bad, (k, j, bad)
    assert h.counters(5)["cntBit"] == r[2].o.counters()["cntBit"]


# ---------------------------------------------------------------------------------------------------------------- 4. NULL outputs
def test_each_output_alone_and_none_at_all():
    n, nf = 2048, 2
    data = np.stack([B.case_input("96k", s)[1][:2 * 2 * nf * n] for s in range(2)])
    ref = None
    for outs in (ALL, ()) + tuple((k,) for k in ALL) + (("max", "bits"), ("tuned", "pts")):
        h = J.Bpsk(rate=96000, blen=4 * n, size=4, tuning=12000, nstreams=2, max_batch_samples=nf * n)
        batch_call(h, "i16", data[:, :2 * nf * n], nf * n)  # (the scoped call is the second: it starts from carried state)
        before = J.live_resources()
        got = scope_call(h, "i16", data[:, 2 * nf * n:], nf * n, outs, what=("outputs", outs))
        if ref is None:
            ref = got
            ref_bits = [h.bits(s).copy() for s in range(2)]
        assert not differ(got, ref, outs), outs
        assert all(np.array_equal(h.bits(s), ref_bits[s]) for s in range(2)), outs
        if not outs:  # the batch call: nothing launched, nothing allocated
            assert h.scope_kernel() == "" and J.live_resources() == before


# ---------------------------------------------------------------------------------------------------------------- 5. resources
def test_resources_of_a_handle_that_never_scopes_and_after_destroy():
    n, nf = 2048, 2
    data = np.stack([B.case_input("96k", 0)[1][:2 * nf * n]])
    gc.collect()
    start = J.live_resources()
    a = J.Bpsk(rate=96000, blen=4 * n, size=4, tuning=12000, nstreams=1, max_batch_samples=nf * n)
    batch_call(a, "i16", data, nf * n)
    plain = J.live_resources()
    b = J.Bpsk(rate=96000, blen=4 * n, size=4, tuning=12000, nstreams=1, max_batch_samples=nf * n)
    scope_call(b, "i16", data, nf * n, (), what="no output")
    both = J.live_resources()
    assert tuple(y - x for x, y in zip(plain, both)) == tuple(y - x for x, y in zip(start, plain))  # b holds what a holds
    scope_call(b, "i16", data, nf * n, ALL, what="all outputs")
    held = J.live_resources()
    assert held[0] > both[0] and held[1] > both[1] and held[3] >= both[3] + 2, (both, held)  # the clock copy, the index table, two events
    again = J.live_resources()
    scope_call(b, "i16", data, nf * n, ALL, what="all outputs again")
    assert J.live_resources() == again  # allocated once
    del a, b
    gc.collect()
    assert J.live_resources() == start


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def _refused(fn, word):
    with pytest.raises(J.JsdrError) as e:
        fn()
    assert word in str(e.value), (word, str(e.value))


def test_refusals_leave_the_handle_as_it_was():
    n, nf = 2048, 2
    L = nf * n
    data = np.stack([B.case_input("96k", s)[1][:2 * 2 * L] for s in range(2)])
    mk = lambda **kw: J.Bpsk(rate=96000, blen=4 * n, size=4, tuning=12000, nstreams=2, max_batch_samples=L, **kw)  # noqa: E731
    h, twin = mk(), mk()
    batch_call(h, "i16", data[:, :2 * L], L)
    batch_call(twin, "i16", data[:, :2 * L], L)
    d_in, stride = upload("i16", data[:, 2 * L:], L)
    out = J.DeviceBuffer(16 * 2 * nf * n + 64)
    p = out.ptr
    assert p % 16 == 0
    for kw, nsamples, st, word in ((dict(tuned=p), L - 1, stride, "not whole frames"),
                                   (dict(tuned=p), L + n, stride + 2 * n, "outside (0, max_batch_samples"),
                                   (dict(tuned=p), 0, stride, "outside (0, max_batch_samples"),
                                   (dict(tuned=p), L, stride - 1, "stride"),
                                   (dict(tuned=p), L, 2 * L - 2, "stride"),
                                   (dict(tuned=p + 8), L, stride, "tuned_dev is not aligned to 16"),
                                   (dict(ds=p + 4), L, stride, "ds_dev is not aligned to 8"),
                                   (dict(iq=p + 4), L, stride, "iq_dev is not aligned to 8"),
                                   (dict(max=p + 2), L, stride, "max_dev is not aligned to 8"),
                                   (dict(pts=p + 2), L, stride, "pts_dev is not aligned to 4")):
        _refused(lambda: h.scope_i16(d_in, st, nsamples, **kw), word)
        _refused(lambda: h.scope_f32(d_in, st, nsamples, **kw), word)
    _refused(lambda: h.scope_i16(None, stride, L, tuned=p), "null input")
    assert h.scope_kernel() == ""
    twins_agree(h, twin, "after the refusals")
    got = scope_call(h, "i16", data[:, 2 * L:], L, what="after the refusals")
    batch_call(twin, "i16", data[:, 2 * L:], L)
    twins_agree(h, twin, "a call after the refusals")
    assert got["bits"].any()
    # the handle's history is not whole frames
    k = mk()
    batch_call(k, "i16", data[:, :n], n // 2)
    _refused(lambda: k.scope_i16(d_in, stride, L, tuned=p), "is not whole frames")
    _refused(lambda: k.scope_layout(L), "is not whole frames")
    # the kinds of handle that have no scope
    _refused(lambda: mk(variant="fast").scope_i16(d_in, stride, L, tuned=p), "fast variant")
    fft = J.Bpsk(rate=96000, blen=4 * n, size=4, tuning=12000, do_fft=1, nstreams=2, max_batch_samples=L)
    _refused(lambda: fft.scope_i16(d_in, stride, L, tuned=p), "do_fft is set or a mode switch is pending")
    batch_call(fft, "i16", data[:, :2 * L], L)
    fft.set_mode(0, 0)  # (tune mode from the next call on: the seam pends)
    _refused(lambda: fft.scope_i16(d_in, stride, L, tuned=p), "do_fft is set or a mode switch is pending")
    # a frame too short for the rings (n * 9600 / rate == 0), and a rate at which a frame does not refill them
    for short, word, ns in ((J.Bpsk(rate=96000, blen=32, size=4, tuning=12000, nstreams=2, max_batch_samples=8), "ring length L=0", 8),
                            (J.Bpsk(rate=8000, blen=4 * n, size=4, tuning=1000, nstreams=2, max_batch_samples=L), "below 9600", L)):
        untouched = short.counters(0)
        _refused(lambda: short.scope_i16(d_in, stride, ns, tuned=p), word)
        _refused(lambda: short.scope_f32(d_in, stride, ns, tuned=p), word)
        _refused(lambda: short.scope_i16(d_in, stride, ns), word)  # (with no output as well: the checks come first)
        _refused(lambda: short.scope_layout(ns), word)
        assert short.scope_kernel() == "" and short.counters(0) == untouched
    _refused(lambda: J.BpskTuned(96000, 4 * n, [12000.0, 12010.0], L).scope_i16(d_in, stride, L, tuned=p), "tuned handle")
    _refused(lambda: J.BpskChannels(96000, 4 * n, [12000.0, 12010.0], max_batch_samples=L).scope_i16(d_in, stride, L, tuned=p),
             "channel handle")
