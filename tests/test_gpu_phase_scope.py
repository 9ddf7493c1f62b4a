"""GPU: the batched phase scope (jsdr_phase_scope_i16 / _f32) against phase_scope.py's restatement of phase.paintComponent's
arithmetic, every row of every output bit for bit (floats by nonfinite.same_f32: the same bits, or both NaN).

Every call reads its frames from a padded layout (tests/layouts.py): a lead of one IQ pair -- frame starts that are 4 bytes
(int16) or 8 bytes (float) off a 16-byte boundary -- a stride above a stream's frames, and poison in every gap (+-32767 / -32768,
NaN and 3e38) that would move a maximum or a mean if it were read.  Every output lies between guard bytes that are checked after
the call.  Shapes are the smallest that can still go wrong; a case takes a second or two."""
import gc

import numpy as np
import pytest

import java_sdr_amd as J
import layouts as L
import nonfinite as NF
import phase_scope as PS

pytestmark = pytest.mark.gpu

IC, QC = 321, -123
HALF, QUARTER = 300, 137  # size/2 and getHeight()/4 of a 600 x 550 panel
LEAD, TAIL = 16, 48  # guard bytes in front of and behind every output


def in_dtype(form):
    return np.int16 if form == "i16" else np.float32


class Guarded:
    """nbytes of output between guard bytes"""

    def __init__(self, nbytes, what):
        self.nbytes, self.what = nbytes, what
        self.lay = L.Layout(1, nbytes, lead=LEAD, tail=TAIL)
        self.d = J.DeviceBuffer.from_host(L.guard_fill(self.lay.nbytes))
        self.ptr = self.d.ptr + LEAD

    def read(self, dtype):
        got = self.d.to_host(np.uint8)
        L.check_guards(got, self.lay, self.what)
        self.d.free()
        return got[LEAD:LEAD + self.nbytes].copy().view(dtype)


class Input:
    """frames [nstreams * fps][2n] on the device at stream stride `stride`, one IQ pair behind the allocation's start"""

    def __init__(self, form, frames, nstreams, fps, stride, seed=0):
        frames = np.ascontiguousarray(frames, in_dtype(form))
        rows = [frames[s * fps:(s + 1) * fps].ravel() for s in range(nstreams)]
        host, starts = L.build_input(rows, stride=stride if nstreams > 1 else None, lead=2, tail=8, unit=2, seed=seed)
        assert starts[0] == 2
        self.d = J.DeviceBuffer.from_host(host)
        self.ptr = self.d.ptr + 2 * host.itemsize


def launch(P, form, src, nstreams, stride, fps, bx, ic=0, qc=0, avg=True, pts=True, stream=None):
    """the call into fresh guarded outputs; nothing is waited for"""
    rows, ncol = nstreams * fps, PS.layout(P.n, bx)[0].size
    outs = (Guarded(4 * rows, "max_dev"), Guarded(8 * rows * ncol, "avg_dev") if avg else None,
            Guarded(16 * rows * ncol, "pts_dev") if pts else None)
    ptrs = [o.ptr if o is not None else None for o in outs]
    if form == "i16":
        P.scope_i16(src, nstreams, stride, fps, ic, qc, bx, HALF, QUARTER, *ptrs, stream=stream)
    else:
        P.scope_f32(src, nstreams, stride, fps, bx, HALF, QUARTER, *ptrs, stream=stream)
    return outs


def collect(outs):
    """(max, avg, pts) of a finished call, guards checked"""
    return tuple(o.read(dt) if o is not None else None for o, dt in zip(outs, (np.float32, np.float32, np.int32)))


def run(P, form, frames, nstreams, fps, stride, bx, ic=0, qc=0, avg=True, pts=True, seed=0):
    src = Input(form, frames, nstreams, fps, stride, seed)
    outs = launch(P, form, src.ptr, nstreams, stride, fps, bx, ic, qc, avg, pts)
    J.binding.stream_sync()
    got = collect(outs)
    src.d.free()
    return got


def check(P, form, frames, nstreams, fps, stride, bx, ic=0, qc=0, where=None, **kw):
    got = run(P, form, frames, nstreams, fps, stride, bx, ic, qc, **kw)
    want = PS.expected_rows(PS.as_floats(form, frames, ic, qc), bx, HALF, QUARTER)
    PS.assert_rows(got, want, (where, form, P.n, bx))
    return got, want


# ------------------------------------------------------------------ the schedule grid
@pytest.mark.parametrize("form", ["i16", "f32"])
@pytest.mark.parametrize("n", PS.GRID_N)
def test_every_schedule_of_the_grid(n, form):
    """3 streams x 3 frames, every row's maximum somewhere else: first sample, last sample, a sample no column holds, ..."""
    S, F = 3, 3
    stride = F * 2 * n + 2 * 7
    ic, qc = (IC, QC) if form == "i16" else (0, 0)
    P = J.Phase(n)
    for bx in PS.grid_bx(n):
        frames = PS.grid_frames(form, n, bx, S * F)
        (mx, _, _), _ = check(P, form, frames, S, F, stride, bx, ic, qc, "grid", seed=bx)
        assert np.unique(mx).size == S * F  # (the rows differ)
        assert P.scope_kernel() == "k_phase_scope"


# ------------------------------------------------------------------ both kernel forms
@pytest.mark.parametrize("form", ["i16", "f32"])
@pytest.mark.parametrize("n,kernel", [(PS.LDS_MAX_N, "k_phase_scope"), (PS.LDS_MAX_N + 2, "k_phase_scope_g"), (9600, "k_phase_scope_g")])
def test_both_kernel_forms_on_either_side_of_the_lds_limit(n, kernel, form):
    S, F = 2, 2
    stride = F * 2 * n + 2 * 3
    ic, qc = (IC, QC) if form == "i16" else (0, 0)
    P = J.Phase(n)
    for bx in (700, 1024):
        check(P, form, PS.grid_frames(form, n, bx, S * F), S, F, stride, bx, ic, qc, "forms", seed=bx)
        assert P.scope_kernel() == kernel


def test_the_global_form_on_schedules_with_short_long_and_no_columns():
    """k_phase_scope_g's own sample fetch: one-sample columns, long columns with a dropped tail, no column at all"""
    n, S, F = PS.LDS_MAX_N + 2, 2, 2
    stride = F * 2 * n + 2 * 5
    for form in ("i16", "f32"):
        P = J.Phase(n)
        for bx in (0, 1, 7, n + 1):
            check(P, form, PS.grid_frames(form, n, bx, S * F), S, F, stride, bx, where="g", seed=bx)
        assert P.scope_kernel() == "k_phase_scope_g"


# ------------------------------------------------------------------ more rows than workgroups; offsets past 2^31
def repeated(form, n, bx, rows, ic=0, qc=0, distinct=9):
    """rows frames drawn from `distinct` (no two neighbours alike), and what their rows must hold"""
    base = PS.grid_frames(form, n, bx, distinct)
    idx = np.arange(rows) * 7 % distinct
    want = PS.expected_rows(PS.as_floats(form, base, ic, qc), bx, HALF, QUARTER)
    return base[idx], tuple(w[idx] for w in want)


@pytest.mark.parametrize("form,n,S,F", [("i16", 64, 5, 1700), ("f32", 64, 5, 1700), ("i16", PS.LDS_MAX_N + 2, 3, 700)])
def test_rows_beyond_the_grid_are_walked_across_stream_ends(form, n, S, F):
    """more rows than the launch has workgroups (at most 8 a CU: 2048 on this chip), so every workgroup walks on from its first
    row by additions -- across stream ends, F being no divisor of the grid; in both kernel forms"""
    bx = 21 if n == 64 else 7
    ic, qc = (IC, QC) if form == "i16" else (0, 0)
    frames, want = repeated(form, n, bx, S * F, ic, qc)
    P = J.Phase(n)
    got = run(P, form, frames, S, F, F * 2 * n + 2 * 7, bx, ic, qc)
    PS.assert_rows(got, want, ("walk", form, n))
    assert P.scope_kernel() == ("k_phase_scope" if n <= PS.LDS_MAX_N else "k_phase_scope_g")


def test_stream_offsets_past_2_to_31_elements():
    """2 streams x 2 frames at n = 2048 with stream_stride_i16 = 2^31 + 2 * 4096: one input allocation above 4 GiB of which four
    frames are touched"""
    import ctypes as C
    n, S, F, bx = 2048, 2, 2, 512
    stride = 2 ** 31 + F * 2 * n
    frames = PS.grid_frames("i16", n, bx, S * F)
    d_in = J.DeviceBuffer(2 * (stride + F * 2 * n))
    assert d_in.nbytes > 2 ** 32
    try:
        for s in range(S):
            rows = np.ascontiguousarray(frames[s * F:(s + 1) * F])
            J.binding._check(J.lib().jsdr_memcpy_h2d(J.binding._addr(d_in.ptr + 2 * s * stride), J.binding._addr(rows),
                                                     C.c_size_t(rows.nbytes)), "h2d")
        P = J.Phase(n)
        outs = launch(P, "i16", d_in.ptr, S, stride, F, bx, IC, QC)
        J.binding.stream_sync()
        PS.assert_rows(collect(outs), PS.expected_rows(PS.as_floats("i16", frames, IC, QC), bx, HALF, QUARTER), "past 2^31")
    finally:
        d_in.free()


# ------------------------------------------------------------------ bx changes on one handle, one stream, no sync between
def test_bx_changes_back_to_back_rebuild_the_table_behind_its_readers():
    n, S, F = 2048, 2, 2
    stride = F * 2 * n + 2 * 7
    seq = (512, 7, 512, 0, 1001)
    frames = PS.grid_frames("i16", n, 512, S * F)
    want = {bx: PS.expected_rows(PS.as_floats("i16", frames, IC, QC), bx, HALF, QUARTER) for bx in set(seq)}
    src = Input("i16", frames, S, F, stride)
    st = J.Stream()
    P = J.Phase(n)
    calls = [launch(P, "i16", src.ptr, S, stride, F, bx, IC, QC, stream=st.ptr) for bx in seq]
    st.sync()
    for k, (bx, outs) in enumerate(zip(seq, calls)):
        PS.assert_rows(collect(outs), want[bx], ("call", k, bx))
    src.d.free()


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("form", ["i16", "f32"])
def test_one_stream_no_frames_and_null_outputs(form):
    n, bx = 600, 21
    ic, qc = (IC, QC) if form == "i16" else (0, 0)
    P = J.Phase(n)
    frames = PS.grid_frames(form, n, bx, 6)
    # one stream: its stride says nothing
    check(P, form, frames[:3], 1, 3, 7, bx, ic, qc, "one stream")
    # avg_dev and pts_dev NULL in turn, and both
    for avg, pts in ((False, True), (True, False), (False, False)):
        check(P, form, frames, 2, 3, 3 * 2 * n + 2 * 11, bx, ic, qc, ("null", avg, pts), avg=avg, pts=pts)
    # no frames: nothing is written (the guards around three empty outputs)
    src = Input(form, frames, 2, 3, 3 * 2 * n + 2)
    outs = launch(P, form, src.ptr, 2, 3 * 2 * n + 2, 0, bx, ic, qc)
    J.binding.stream_sync()
    assert all(o.size == 0 for o in collect(outs))
    src.d.free()


# ------------------------------------------------------------------ int16 edges
def test_int16_edges():
    n, bx, S, F = 600, 63, 1, 3
    base = np.array(PS.raw_frames(n, 3, seed=1))
    # -32768: |x| = 32768/32767 is the maximum; an all-zero frame: max 0, the scales are +Inf, every 0 * Inf is NaN -> 0
    fr = base.copy()
    fr[0, 2 * 10] = -32768
    fr[1] = 0
    P = J.Phase(n)
    (mx, avg, pts), _ = check(P, "i16", fr, S, F, 0, bx, 0, 0, "min / zero")
    assert mx[0] == np.float32(32768) / np.float32(32767) and mx[1] == 0
    ncol = PS.layout(n, bx)[0].size
    assert not pts.reshape(F, ncol, 4)[1].any() and not avg.reshape(F, ncol, 2)[1].any()
    # corrections that wrap: 32767 + 1 -> -32768, -32768 - 1 -> 32767, and (short)70000 = 4464
    fr = base.copy()
    fr[0, 2 * 20], fr[0, 2 * 20 + 1] = 32767, -32768
    fr[2, 2 * 599], fr[2, 2 * 599 + 1] = 32767, -32768
    assert PS.as_floats("i16", fr, 1, -1)[0, 40] == -np.float32(32768) / np.float32(32767)
    for ic, qc in ((1, -1), (70000, -70000), (-32768, 32767)):
        check(P, "i16", fr, S, F, 0, bx, ic, qc, ("wrap", ic, qc))


# ------------------------------------------------------------------ float edges
def test_float_edges_between_clean_frames():
    n, bx, S, F = 600, 63, 5, 3
    _, first, count = PS.layout(n, bx)
    assert count.min() >= 2
    clean = PS.grid_frames("f32", n, bx, S * F)
    fr = clean.copy()
    fr[1] = NF.poison(clean[1], [(int(first[5]), NF.I, NF.NAN)])                              # a NaN inside a column
    fr[3] = NF.poison(clean[3], [(int(first[7] + count[7] - 1), NF.Q, NF.NAN)])               # ... at a column's closing sample
    fr[5] = np.full(2 * n, NF.NAN)                                                            # max -1: negative scales
    fr[7] = NF.poison(clean[7], [(100, NF.I, NF.PINF)])                                       # max Inf: scales 0, Inf * 0 -> 0
    fr[9] = NF.poison(clean[9], [(n - 1, NF.Q, NF.NINF)])
    fr[11] = NF.poison(clean[11], [(300, NF.I, NF.HUGE), (301, NF.Q, -NF.HUGE)])
    fr[13] = PS.denormal_frame(n)
    PS.check_denormal_row(fr[13], bx, HALF, QUARTER)
    P = J.Phase(n)
    (mx, avg, pts), _ = check(P, "f32", fr, S, F, F * 2 * n + 2 * 9, bx, where="edges")
    ncol = first.size
    pts = pts.reshape(S * F, ncol, 4)
    assert mx[5] == -1 and np.isposinf(mx[7]) and np.isposinf(mx[9]) and mx[11] == NF.HUGE and mx[13] == np.float32(1e-40)
    assert not pts[5].any() and not pts[7].any() and not pts[9].any()
    assert (pts[13] == PS.INT_MAX).any() and (pts[13] == PS.INT_MIN).any()
    # the same frames through the form that reads its columns from memory
    n2 = PS.LDS_MAX_N + 2
    big = np.tile(fr[:, :2 * n], (1, n2 // n + 1))[:, :2 * n2].copy()
    P2 = J.Phase(n2)
    check(P2, "f32", big[4:10], 2, 3, 3 * 2 * n2 + 2, 700, where="edges, g form")
    assert P2.scope_kernel() == "k_phase_scope_g"


# ------------------------------------------------------------------ composition with the calls that were there before
def test_scope_equals_phase_columns_and_phase_maxabs():
    n, bx, rows = 2048, 512, 4
    for form, ic, qc in (("f32", 0, 0), ("i16", IC, QC)):
        frames = PS.grid_frames(form, n, bx, rows)
        mx, avg, _ = run(J.Phase(n), form, frames, 2, 2, 2 * 2 * n + 2 * 7, bx, ic, qc)
        fl = frames if form == "f32" else J.convert_i16(frames.ravel(), ic=ic, qc=qc).reshape(rows, 2 * n)
        assert np.array_equal(mx.view(np.uint32), J.phase_maxabs(fl, n).view(np.uint32))
        avg = avg.reshape(rows, -1, 2)
        for r in range(rows):
            pix, ai, aq = J.phase_columns(fl[r], bx)
            assert np.array_equal(pix, PS.layout(n, bx)[0])
            assert np.array_equal(avg[r, :, 0].view(np.uint32), ai.view(np.uint32)) and np.array_equal(avg[r, :, 1].view(np.uint32), aq.view(np.uint32))


# ------------------------------------------------------------------ resources
def test_the_handle_gives_back_what_the_scope_allocated():
    n = 2048
    gc.collect()
    before = J.live_resources()
    P = J.Phase(n)
    created = J.live_resources()
    frames = PS.grid_frames("i16", n, 512, 2)
    run(P, "i16", frames, 1, 2, 0, 0)
    first = J.live_resources()
    assert first[0] == created[0] + 1 and first[1] == created[1] + 8 * n  # the schedule table, at the first scope call
    for bx in (512, 7, 2048):
        run(P, "i16", frames, 1, 2, 0, bx)
    assert J.live_resources() == first  # no later call allocates
    del P
    gc.collect()
    assert J.live_resources() == before
