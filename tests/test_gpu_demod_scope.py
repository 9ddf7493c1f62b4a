"""GPU: the demod scope (jsdr_demod_scope_i16 / _f32) -- demod.paintComponent's trace and spectrum for every frame of a batch call.
tests/demod_scope.py has the restatement of the painters, the oracle pair and the case lists; tests/test_demod_scope_abi.py
holds the restatement to the Java loops and counts, on the oracle alone, what the trace cases contain.

No tolerance anywhere.  The trace and the dbg rows are compared bit for bit with the oracle (oracle_lib.Demod's sam[] after
receive(), and the sam[] of its MODE_RAW twin) through the restatement; the spectrum with its composition: the PSD rows a fresh
Fft(n).batch_f32 writes for the RETURNED dbg rows, pooled by the restatement.  The audio of every scope call is compared with
the oracle's as well.  Every call writes into one arena whose gaps -- before, between and after the audio rows and the three
outputs, and the padding of every audio row -- hold a canary that must survive."""
import gc

import numpy as np
import pytest

import demod_scope as DS
import java_sdr_amd as J
import oracle_lib as O
from test_gpu_demod import same

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
PAD = 6          # elements between a row's last sample and the next row, input and audio
GAP = 64         # canary bytes around every region of the arena
CANARY = 0xA5


def same_bits(a, b):
    """float32 arrays equal bit for bit, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))).all())


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


_ffts = {}


def composition(dbg_rows, n, W, H):
    """spec rows from dbg rows: a Fft(n) of this test's own, its batch_f32, the restatement's pooling"""
    if n not in _ffts:
        _ffts[n] = J.Fft(n, DS.RATE)
    rows = dbg_rows.shape[0]
    d_in = J.DeviceBuffer.from_host(np.ascontiguousarray(dbg_rows, F32))
    d_out = J.DeviceBuffer(4 * rows * (n + 2))
    _ffts[n].batch_f32(d_in, rows, d_out)
    psd = d_out.to_host(F32).reshape(rows, n + 2)
    return np.stack([DS.spec(psd[r, :n], W, H) for r in range(rows)])


def scope_call(h, form, data, L, W, H, outs=("trace", "spec", "dbg"), ic=0, qc=0, what=None):
    """one scope call over data [S][2L] (int16 for "i16", float32 for "f32") in rows padded by PAD: dict of audio int16 [S][2L]
    and the outputs asked for, trace / spec int32 [rows][W], dbg float32 [rows][2n]"""
    S, n = h.S, h.n
    rows = S * (L // n)
    stride = 2 * L + PAD
    if form == "i16":
        src = np.full((S, stride), 12345, np.int16)
    else:
        src = np.full((S, stride), np.nan, F32)  # whatever is read from beyond a row poisons what it reaches
    src[:, :2 * L] = data
    d_in = J.DeviceBuffer.from_host(src)
    ar = Arena(dict(audio=2 * S * stride, trace=4 * rows * W * ("trace" in outs), spec=4 * rows * W * ("spec" in outs),
                    dbg=8 * rows * n * ("dbg" in outs)))
    kw = dict(trace_dev=ar.ptr("trace"), spec_dev=ar.ptr("spec"), dbg_dev=ar.ptr("dbg"))
    if form == "i16":
        h.scope_i16(d_in, stride, L, ar.ptr("audio"), stride, W, H, ic=ic, qc=qc, **kw)
    else:
        h.scope_f32(d_in, stride, L, ar.ptr("audio"), stride, W, H, **kw)
    raw = ar.read((what, form, W, H, outs))
    audio = raw["audio"].view(np.int16).reshape(S, stride)
    assert (audio[:, 2 * L:].view(np.uint8) == CANARY).all(), (what, "audio row padding written")
    got = dict(audio=audio[:, :2 * L].copy())
    if "trace" in outs:
        got["trace"] = raw["trace"].view(np.int32).reshape(rows, W)
    if "spec" in outs:
        got["spec"] = raw["spec"].view(np.int32).reshape(rows, W)
    if "dbg" in outs:
        got["dbg"] = raw["dbg"].view(F32).reshape(rows, 2 * n)
    want_kernel = "+".join(["k_demod_scope_front"] * bool(outs) + ["k_demod_trace"] * ("trace" in outs))
    k = h.scope_kernel()
    assert k.startswith(want_kernel) and k.endswith("+k_demod_spec") == ("spec" in outs), (what, k, outs)
    return got


class Rig:
    """handles (one a form) and one oracle pair a stream, given the same controls and calls"""

    def __init__(self, n, mode, sw, band, forms=("i16", "f32"), streams=DS.S, max_frames=max(DS.CALLS)):
        self.n, self.S, self.mode = n, streams, mode
        self.h = {f: J.Demod(DS.RATE, n, streams, max_frames * n) for f in forms}
        self.p = [DS.Painter(mode, *sw, band) for _ in range(streams)]
        for h in self.h.values():
            h.configure(mode, *sw)
            h.weights(*band)
        self.pos = 0

    def expect(self, bufs, nf):
        """the oracle over float frames bufs [S][2L]: audio [S][2L], sam and dbg [rows][2n]"""
        n = self.n
        audio, sams, dbgs = [], [], []
        for s in range(self.S):
            a = []
            for f in range(nf):
                au, sam, dbg = self.p[s].receive(bufs[s][2 * f * n:2 * (f + 1) * n])
                a.append(au)
                sams.append(sam)
                dbgs.append(dbg)
            audio.append(np.concatenate(a))
        return np.stack(audio), np.stack(sams), np.stack(dbgs)

    def call(self, raws, nf, W, H, ic=DS.IC, qc=DS.QC, what=None, floats=None):
        """the next nf frames of raws (int16 [S][..]), or of floats (float32 [S][..], the float form alone)"""
        n, L = self.n, nf * self.n
        if floats is None:
            chunk = raws[:, 2 * self.pos:2 * (self.pos + L)]
            bufs = np.stack([O.convert_i16(chunk[s], ic=ic, qc=qc) for s in range(self.S)])
        else:
            chunk, bufs = None, np.ascontiguousarray(floats[:, 2 * self.pos:2 * (self.pos + L)], F32)
        self.pos += L
        audio, sams, dbgs = self.expect(bufs, nf)
        trace = np.stack([DS.trace(sam, W, H) for sam in sams])
        for form, h in self.h.items():
            tag = (what, form, "n", n, "mode", self.mode, "W", W, "H", H)
            got = scope_call(h, form, chunk if form == "i16" else bufs, L, W, H, ic=ic, qc=qc, what=tag)
            assert np.array_equal(got["audio"], audio), (tag, "audio")
            assert same_bits(got["dbg"], dbgs), (tag, "dbg", np.argwhere(got["dbg"].view(U32) != dbgs.view(U32))[:4])
            bad = np.argwhere(got["trace"] != trace)
            assert bad.size == 0, (tag, "trace", len(bad), "entries differ; first (row, entry)", bad[:4].tolist(),
                                   got["trace"][tuple(bad[0])], trace[tuple(bad[0])])
            if n >= 2:
                want = composition(got["dbg"], n, W, H)
                bad = np.argwhere(got["spec"] != want)
                assert bad.size == 0, (tag, "spectrum", len(bad), "entries differ; first (row, entry)", bad[:4].tolist())
            for s in range(self.S):
                mx, av = h.frame_stats(s)
                assert same(mx, self.p[s].o.max) and same(av, self.p[s].o.avg), (tag, "frame_stats", s)
            assert h.state()[0] == self.p[0].o.car, (tag, "car")


# ---------------------------------------------------------------------------------------------------------------- 1. the grid
@pytest.mark.parametrize("mode", DS.MODES)
@pytest.mark.parametrize("n", DS.GPU_N)
def test_trace_dbg_and_spectrum_on_the_grid(n, mode):
    """every switch set on a band-pass or the all-pass, int16 and float input, three calls each of 2, 3, 2 frames; the grid's
    widths and the heights go round the twelve calls"""
    ws = DS.widths(n)
    raws = DS.signal(n)
    k = 0
    for j, sw in enumerate(DS.SWITCHES):
        band = DS.BAND if (j + mode) % 2 == 0 else DS.ALLPASS
        rig = Rig(n, mode, sw, band)
        for nf in DS.CALLS:
            rig.call(raws, nf, ws[(k + 2 * mode) % len(ws)], DS.HEIGHTS[(k + mode) % len(DS.HEIGHTS)], what=("grid", sw, band))
            k += 1


def test_the_grid_reaches_what_it_is_meant_to():
    """(no device work) widths both sides of the frame and of its half, 1000 at 9600, columns that straddle tile edges"""
    assert 1000 in DS.widths(9600) and 9600 // 1000 == 9
    for n in DS.GPU_N:
        ws = DS.widths(n)
        assert len(ws) <= 12 and any(w > n for w in ws) and 1 in ws and any(n // w >= 2 for w in ws)
    tf, tc, _, _ = DS.layout(9600, 1000)
    straddle = [(int(i), int(i) + 9 // 2) for i in tf[:999] if int(i) // 2048 != (int(i) + 9 // 2 - 1) // 2048]
    assert straddle, "no trace column of (9600, 1000) reads Qs on both sides of a tile edge"
    # (a width that does not divide the tile: columns start at every residue of the 8 samples a thread owns)
    assert len({int(i) % 8 for i in tf[:999]}) == 8


# ---------------------------------------------------------------------------------------------------------------- 2. the spectrum
@pytest.mark.parametrize("n,kernel", [(2048, "k_fft"), (9600, "k_fft_mixed"), (4410, "k_fft_rt"), (10241, "k_dft_any")])
def test_spectrum_is_the_composition_in_every_fft_family(n, kernel):
    assert J.Fft(n, DS.RATE).kernel_name() == kernel
    raws = DS.signal(n)
    for mode, sw, band, W, H in ((DS.NFM, (1, 1, 1), DS.BAND, 1000, 400), (DS.OFF, (0, 1, 0), DS.BAND, n, 1001),
                                 (DS.AM, (1, 0, 1), DS.ALLPASS, n // 2 + 1, 3)):
        rig = Rig(n, mode, sw, band, forms=("i16",))
        rig.call(raws, 2, W, H, what=("families", kernel))
        assert rig.h["i16"].scope_kernel() == "k_demod_scope_front+k_demod_trace+%s+k_demod_spec" % kernel


# ---------------------------------------------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("mode", [DS.RAW, DS.AM, DS.NFM])
def test_silence_with_agc(mode):
    """max = 0: the finals are 0 * inf = NaN, the PSD is -inf, the casts saturate and the sums wrap"""
    n = 2049
    raws = np.zeros((DS.S, 2 * sum(DS.CALLS) * n), np.int16)
    rig = Rig(n, mode, (1, 1, 1), DS.BAND)
    for nf, (W, H) in zip(DS.CALLS, ((1000, 400), (n, 0), (512, 1001))):
        rig.call(raws, nf, W, H, ic=0, qc=0, what="silence")
    assert np.isnan(rig.p[0].o.d.sam[0]) and rig.p[0].o.max == 0
    assert (DS.spec(np.full(n, -np.inf, F32), 8, 400) == DS.wrap32(200 + DS.INT_MAX)).all()  # H/2 + (int)(+inf) wraps


@pytest.mark.parametrize("mode", [DS.RAW, DS.WFM])
def test_full_scale_int16_with_a_dc_correction_that_wraps(mode):
    n = 4410
    rng = np.random.default_rng(77)
    raws = rng.choice(np.array([-32768, -32767, 32766, 32767], np.int16), (DS.S, 2 * sum(DS.CALLS) * n))
    rig = Rig(n, mode, (1, 1, 0), DS.BAND)
    for nf, (W, H) in zip(DS.CALLS, ((1000, 400), (2205, 1001), (4411, 3))):
        rig.call(raws, nf, W, H, ic=1000, qc=-1000, what="full scale")
    assert O.convert_i16(np.array([32767, -32768], np.int16), ic=1000, qc=-1000)[0] < 0  # the correction wrapped


@pytest.mark.parametrize("sw", [(0, 0, 0), (0, 1, 1), (1, 1, 1)])
@pytest.mark.parametrize("mode", [DS.RAW, DS.AM, DS.NFM])
def test_nan_and_inf_in_float_input(mode, sw):
    """at a tile edge, and in a trace column's first and later Q (W = 512 at n = 2049: four samples a column, two Qs looked at)"""
    n, W = 2049, 512
    frames = sum(DS.CALLS)
    x = np.stack([O.convert_i16(r) for r in DS.signal(n)]).copy()
    assert n // W == 4
    for s in range(DS.S):
        for f in range(frames):
            fr = x[s, 2 * f * n:2 * (f + 1) * n]
            which = (s + f) % 4
            if which == 0:    # the tile's last and the next tile's only sample
                fr[2 * 2047] = np.nan
                fr[2 * 2048 + 1] = -np.inf
            elif which == 1:  # first Q of column 10, later Q of column 20, the final's I of column 30
                fr[2 * 40 + 1] = np.nan
                fr[2 * 81 + 1] = np.inf
                fr[2 * 120] = -np.inf
            elif which == 2:  # the frame's first and last sample
                fr[0] = np.inf
                fr[2 * n - 1] = np.nan
            # (which == 3: a clean frame between poisoned ones)
    rig = Rig(n, mode, sw, DS.BAND, forms=("f32",))
    for nf, H in zip(DS.CALLS, (400, 1001, 3)):
        rig.call(None, nf, W, H, what=("nonfinite", sw), floats=x)


@pytest.mark.parametrize("mode", [DS.NFM, DS.WFM])
def test_the_first_sample_of_a_call_in_fm_takes_the_carried_detector_state(mode):
    """W = n: one sample a column, no Q looked at -- entry x + 1 is (int)(final float of sample x * h).  The scope passes run
    AFTER the call has stored its last sample as the next call's li / lq: sample 0 must still be detected against the state
    from BEFORE the call"""
    n, H = 64, 4 * 10 ** 6
    raws = DS.signal(n)
    rig = Rig(n, mode, (1, 1, 0), DS.BAND)
    before = []
    for nf in DS.CALLS:
        before.append((rig.p[0].o.d.li, rig.p[0].o.d.lq))
        rig.call(raws, nf, n, H, what="carried")
    assert before[0] == (0.0, 0.0) and before[1] != before[2] and before[1] != (0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------- 4. the batch call
@pytest.mark.parametrize("mode,n", [(DS.NFM, 2049), (DS.AM, 2049), (DS.WFM, 10241)])
def test_a_scope_call_is_the_batch_call(mode, n):
    """three handles -- scope calls, batch calls, alternating -- agree in audio, frame_stats, state and launch counts"""
    raws = DS.signal(n)
    hs = [J.Demod(DS.RATE, n, DS.S, max(DS.CALLS) * n) for _ in range(3)]
    for h in hs:
        h.configure(mode, 1, 1, 1)
        h.weights(*DS.BAND)
        h.profile_enable(True)
    pos = 0
    for k, nf in enumerate(DS.CALLS + DS.CALLS):
        L = nf * n
        if pos + L > raws.shape[1] // 2:
            pos = 0
        chunk = np.ascontiguousarray(raws[:, 2 * pos:2 * (pos + L)])
        pos += L
        audio = []
        for j, h in enumerate(hs):
            if j == 0 or (j == 2 and k % 2 == 0):
                audio.append(scope_call(h, "i16", chunk, L, 1000, 400, ic=DS.IC, qc=DS.QC, what="scope beside batch")["audio"])
            else:
                d_in = J.DeviceBuffer.from_host(chunk)
                d_out = J.DeviceBuffer(chunk.nbytes)
                h.batch_i16(d_in, 2 * L, L, d_out, 2 * L, DS.IC, DS.QC)
                audio.append(d_out.to_host(np.int16).reshape(DS.S, 2 * L))
        assert np.array_equal(audio[0], audio[1]) and np.array_equal(audio[0], audio[2]), (k, "audio")
        for s in range(DS.S):
            st = [h.frame_stats(s) for h in hs]
            assert all(same(a[0], st[0][0]) and same(a[1], st[0][1]) for a in st), (k, s, st)
        assert hs[0].state() == hs[1].state() == hs[2].state(), k
    counts = [{name: v[1] for name, v in h.profile_read().items()} for h in hs]
    assert counts[0] == counts[1] == counts[2] and counts[0]["k_demod_front"] == 6, counts


# ---------------------------------------------------------------------------------------------------------------- 5. chunks
def test_chunked_passes_give_the_same_rows():
    n, nf, W, H = 2049, 3, 1000, 400
    raws = np.ascontiguousarray(DS.signal(n)[:, :2 * nf * n])
    ref = None
    for chunk in (0, 1, 2, 4, 9, 1000):  # nine rows: 4 leaves a ragged last pass, 2 a pass that spans two streams
        h = J.Demod(DS.RATE, n, DS.S, nf * n)
        h.configure(DS.AM, 1, 1, 1)
        h.weights(*DS.BAND)
        h.scope_chunk(chunk)
        got = scope_call(h, "i16", raws, nf * n, W, H, ic=DS.IC, qc=DS.QC, what=("chunk", chunk))
        if ref is None:
            ref = got
            assert got["trace"].shape == (9, W) and len({r.tobytes() for r in got["trace"]}) == 9
        for name in ("audio", "trace", "spec"):
            assert np.array_equal(got[name], ref[name]), (chunk, name)
        assert same_bits(got["dbg"], ref["dbg"]), chunk


# ---------------------------------------------------------------------------------------------------------------- 6. NULL outputs
def test_every_combination_of_outputs_and_nothing_beside_them():
    n, nf, W, H = 100, 2, 33, 400
    raws = np.ascontiguousarray(DS.signal(n)[:, :2 * nf * n])
    ref = None
    for bits in (7, 0, 1, 2, 3, 4, 5, 6):
        outs = tuple(name for b, name in ((1, "trace"), (2, "spec"), (4, "dbg")) if bits & b)
        h = J.Demod(DS.RATE, n, DS.S, nf * n)
        h.configure(DS.NFM, 1, 1, 1)
        h.weights(*DS.BAND)
        before = J.live_resources()
        got = scope_call(h, "i16", raws, nf * n, W, H, outs=outs, ic=DS.IC, qc=DS.QC, what=("outputs", outs))
        if ref is None:
            ref = got
        for name in ("audio",) + outs:
            assert same_bits(got[name], ref[name]) if name == "dbg" else np.array_equal(got[name], ref[name]), (outs, name)
        if not outs:  # the batch call: nothing launched, nothing allocated
            assert h.scope_kernel() == "" and J.live_resources() == before


# ---------------------------------------------------------------------------------------------------------------- 7. resources
def test_resources_return_and_a_width_change_is_followed_by_correct_rows():
    n = 2049
    raws = DS.signal(n)
    composition(np.zeros((1, 2 * n), F32), n, 4, 4)  # (this file's own Fft(n) exists before the count)
    gc.collect()
    before = J.live_resources()
    rig = Rig(n, DS.NFM, (1, 1, 1), DS.BAND, forms=("i16",))
    created = J.live_resources()
    for nf, W in zip(DS.CALLS, (50, 77, 50)):
        rig.call(raws, nf, W, 400, what=("width change", W))
    held = J.live_resources()
    assert held[0] >= created[0] + 4 and held[1] > created[1] and held[3] >= created[3] + 1, (created, held)  # rows, table, the Fft
    with pytest.raises(J.JsdrError, match="channel handle"):
        ch = J.DemodChannels(DS.RATE, n, 1, 2, n)
        d = J.DeviceBuffer(16 * n)
        ch.scope_i16(d, 2 * n, n, d, 2 * n, 8, 8, trace_dev=d)
    del rig, ch
    gc.collect()
    assert J.live_resources() == before
