"""GPU: the tuned channel handle (jsdr_bpsk_create_tuned_channels) -- ninputs x nchannels lock-step demodulators in the tune mode,
every channel of every input with its own tuning, retunes and plans, the channels of an input reading ONE input row
(k_chan_front_pst).  Two references, and no tolerance anywhere:
  (A) a BpskTuned handle of ninputs x nchannels streams on a buffer in which every input is repeated nchannels times, given the
      same calls, the same set_stream_tuning(s) and the same plans -- every stream, after every call;
  (B) one-stream ordinary handles (one_stream_ref / Ref of the tuned handle's tests: set_tuning between calls, the samples in
      pieces with reconfigure at a plan's entries), which pass through none of the tuned handle's kernels.
Compared bit for bit: the bits of every call, FECDecode rc / bit index / bytes, the ten counters, the state doubles of STATE,
decoded[] and the (fi, fq) trace."""
import ctypes as C
import gc

import numpy as np
import pytest

import java_sdr_amd as J
import layouts as LY
import oracle_lib as O
from test_gpu_bpsk_stream_tuning import RAGGED, _outputs, _rc, mixed_input, noise_input
from test_gpu_bpsk_tuning_plan import Ref, plan_of, same_call
from test_gpu_bpsk_tuning_ramp import expand, ramps_of, same_as_twin

pytestmark = pytest.mark.gpu

# a tile of 256 outputs at a decimation of 10 is 2560 samples, and 26 is the history (the positions of
# test_entries_at_the_history_checkpoint_and_tile_positions; k_chan_front_pst's tile there is 200 outputs, 2000 samples)
P_OF = lambda L: [0, 1, 25, 26, 27, 63, 64, 65, 2559, 2560, 2561, 2586, L - 27, L - 26, L - 1]  # noqa: E731


class Pair:
    """a tuned channel handle d on the inputs [ninputs][2n] and reference A: a tuned handle a of ninputs x nchannels streams on a
    buffer in which every input is repeated nchannels times"""

    def __init__(self, rate, nin, nch, tunings, max_batch, inputs, finputs=None):
        assert len(inputs) == nin and len(tunings) == nin * nch
        self.n = len(inputs[0]) // 2
        self.nin, self.nch, self.S = nin, nch, nin * nch
        self.d = J.BpskTunedChannels(rate, 8192, nin, nch, tunings, max_batch_samples=max_batch)
        self.a = J.BpskTuned(rate, 8192, tunings, max_batch_samples=max_batch)
        self.buf = J.DeviceBuffer.from_host(np.concatenate(inputs))
        self.dup = J.DeviceBuffer.from_host(np.concatenate([x for x in inputs for _ in range(nch)]))
        if finputs is not None:
            self.buf32 = J.DeviceBuffer.from_host(np.concatenate(finputs))
            self.dup32 = J.DeviceBuffer.from_host(np.concatenate([x for x in finputs for _ in range(nch)]))

    def run(self, pos, L, f32=False, ic=0, qc=0):
        """the call on both handles, not compared"""
        if f32:
            self.d.batch_f32(self.buf32.ptr + 8 * pos, 2 * self.n, L)
            self.a.batch_f32(self.dup32.ptr + 8 * pos, 2 * self.n, L)
        else:
            self.d.batch_i16(self.buf.ptr + 4 * pos, 2 * self.n, L, ic, qc)
            self.a.batch_i16(self.dup.ptr + 4 * pos, 2 * self.n, L, ic, qc)

    def call(self, pos, L, f32=False, ic=0, qc=0, what=""):
        self.run(pos, L, f32, ic, qc)
        same_as_twin(self.d, self.a, self.S, (what, pos, L))

    def refs(self, rate, tunings, max_batch, streams):
        """reference B for these streams: each reads the row of its INPUT"""
        return {s: Ref(rate, tunings[s], max_batch, self.buf, s // self.nch, self.n) for s in streams}


def same_stream(d, e, s, what):
    """stream s of two handles that were given the same calls"""
    for get in (J.Bpsk.counters, J.Bpsk.state, J.Bpsk.bits, J.Bpsk.trace):
        g, w = get(d, s), get(e, s)
        assert g == w if isinstance(g, dict) else g.tobytes() == w.tobytes(), (what, get.__name__)
    fg, fe = d.fec_results(s), e.fec_results(s)
    assert [(a, b) for a, b, _ in fg] == [(a, b) for a, b, _ in fe], what
    assert all(np.array_equal(x[2], y[2]) for x, y in zip(fg, fe)), what
    assert np.array_equal(d.decoded(s), e.decoded(s)), what
    assert d.stream_tuning(s) == e.stream_tuning(s), what


# ---- 1
def test_unplanned_ragged_calls_on_three_inputs_of_five_channels():
    """fractional tunings, one <= 0, 0 itself, an equal pair on one input; the calls move the tile edges by odd counts"""
    nin, nch = 3, 5
    chunks = RAGGED
    n = sum(chunks)
    inputs = [mixed_input(500 + i, n, [13200.0, 25200.0])[0] for i in range(2)] + [noise_input(502, n)]
    tunings = [12000.5, 24000.25, 11987.25, -700.5, 12000.5,
               12010.5, 300.75, 0.0, 23999.0, 12000.0,
               47999.5, 12000.5, 95999.0, 1.25, 9000.75]
    p = Pair(96000, nin, nch, tunings, max(chunks), inputs)
    refs = p.refs(96000, tunings, max(chunks), (0, 3, 4, 7, 8, 12, 14))
    assert p.d.channel_info() == (nin, nch) and p.d.nstreams == nin * nch
    assert [p.d.stream_tuning(s) for s in range(p.S)] == tunings and p.d.control() == (12000.5, 0, 0)
    pos = 0
    for L in chunks:
        p.call(pos, L, what="ragged")
        for s, r in refs.items():
            same_call(p.d, s, r, r.call(pos, L), ("one-stream reference", pos, L, s))
        pos += L
    assert p.d.front_kernel_name() == "k_chan_front_pst" and p.a.front_kernel_name() == "k_front_pst"
    assert p.d.state(3)[0] <= 0.0  # the channel below 0 Hz passes its samples through unmixed
    prof = p.d
    prof.profile_enable(True)
    p.run(0, 4099)
    assert prof.profile_read()["k_tuner_walk"][1] == 1  # the walk appears as it does on a tuned handle


# ---- 2
@pytest.mark.parametrize("nch", [1, 16])
def test_one_channel_and_sixteen_channels(nch):
    nin = 2
    chunks = [4099, 20000, 77, 2586]
    n = sum(chunks)
    inputs = [mixed_input(510 + i, n, [13200.0])[0] for i in range(nin)]
    tunings = [11000.0 + 37.25 * s for s in range(nin * nch)]
    p = Pair(96000, nin, nch, tunings, max(chunks), inputs)
    pos = 0
    for L in chunks:
        p.call(pos, L, what=("channels", nch))
        pos += L
    assert p.d.channel_info() == (nin, nch) and p.d.front_kernel_name() == "k_chan_front_pst"


# ---- 3
@pytest.mark.parametrize("rate,base", [(192000, 12000.0), (48000, 9000.0), (44100, 8000.0)])
def test_other_rates(rate, base):
    """the tile is what fits the workgroup's LDS: 100 outputs at 192 kHz (200 at 96 kHz), and the 256 its lanes allow at 48 and 44.1 kHz"""
    nin, nch = 2, 3
    n = 60000 * (rate // 9600) // 10
    inputs = [mixed_input(rate, n, [base + 1200.0], rate=rate, noise=500.0)[0], noise_input(rate + 1, n)]
    tunings = [base, base + 10.5, -3000.0, base + 0.25, base, base / 2.0 + 0.125]
    chunks = [n // 3, 5, n - n // 3 - 5]
    p = Pair(rate, nin, nch, tunings, max(chunks), inputs)
    refs = p.refs(rate, tunings, max(chunks), range(p.S))
    pos = 0
    for L in chunks:
        p.call(pos, L, what=("rate", rate))
        for s, r in refs.items():
            same_call(p.d, s, r, r.call(pos, L), ("one-stream reference", rate, pos, s))
        pos += L
    assert p.d.front_kernel_name() == "k_chan_front_pst"


# ---- 4
def test_retunes_between_calls_touch_the_streams_named_only():
    nin, nch = 2, 3
    chunks = [4099, 16384, 77, 20000, 8192]
    n = sum(chunks)
    tunings = [12000.5, 11987.25, 12000.0, 12000.0, 300.75, -0.5]
    inputs = [mixed_input(520 + i, n, [13200.0])[0] for i in range(nin)]
    # before call k: (first stream, [new tunings]) -- one value: set_stream_tuning, more: the bulk form
    acts = {1: [(1, [12010.0])], 2: [(4, [310.25, 5.5])], 3: [(0, [12000.5])],  # (3: the current value -- still an action)
            4: [(2, [0.0]), (3, [-3000.0])]}
    p = Pair(96000, nin, nch, tunings, max(chunks), inputs)
    still = J.BpskTunedChannels(96000, 8192, nin, nch, tunings, max_batch_samples=max(chunks))  # undisturbed
    refs = p.refs(96000, tunings, max(chunks), range(p.S))
    now, touched = list(tunings), set()
    pos = 0
    for k, L in enumerate(chunks):
        for first, vals in acts.get(k, []):
            mc = [p.d.counters(s)["dmMaxCorr"] for s in range(p.S)]
            if k == 3:
                assert mc[0] > 0 and mc[3] > 0  # (there is something to zero, and something to keep)
            for h in (p.d, p.a):
                if len(vals) == 1:
                    h.set_stream_tuning(first, vals[0])
                else:
                    h.set_stream_tunings(first, vals)
            for i, v in enumerate(vals):
                refs[first + i].r.set_tuning(v)
                now[first + i] = v
                touched.add(first + i)
            assert [p.d.stream_tuning(s) for s in range(p.S)] == now
            for s in range(p.S):  # dmMaxCorr zeroed exactly where the action says
                hit = first <= s < first + len(vals)
                assert p.d.counters(s)["dmMaxCorr"] == (0 if hit else mc[s]), (k, s)
        p.call(pos, L, what=("retuned", k))
        still.batch_i16(p.buf.ptr + 4 * pos, 2 * n, L)
        for s, r in refs.items():
            same_call(p.d, s, r, r.call(pos, L), ("one-stream reference", k, s))
            if s not in touched:
                same_stream(p.d, still, s, ("untouched", k, s))
        pos += L
    assert touched == set(range(p.S)) and p.d.control()[0] == 12000.5


# ---- 5
def test_step_plans_at_the_history_checkpoint_and_tile_positions():
    """the entries sit on different channels of one input, beside a channel without any; every stream against one-stream handles
    fed the samples in pieces with reconfigure between them"""
    first, L, after = 4099, 20000, 5000
    n = first + L + after
    P = P_OF(L)
    nin, nch = 2, 4
    tunings = [12000.0, 12010.5, 11987.25, 12000.0, 300.75, 12000.5, 11999.0, 12000.0]
    entries = {
        0: [(a, 12000.0 + 7.25 * (i + 1) * (-1) ** i) for i, a in enumerate(P)],  # every position
        # (1: none, on the same input)
        2: [(0, 11990.0)],
        3: [(2560, 12010.0), (2561, 12020.5)],                                   # a sample apart
        4: [(25, 310.25), (26, 5.5), (27, 320.0)],                               # three in one checkpoint block
        5: [(64, 12000.5), (2559, 0.0), (2586, -500.0), (L - 27, 11990.0)],      # down through 0 and, in the next call, back up
        6: [(1999, 11990.5), (2000, 12004.0), (2001, 11999.0), (2026, 12001.25)],  # k_chan_front_pst's own tile: 200 outputs
        7: [(L - 1, 12003.5)],
    }
    inputs = [mixed_input(530 + i, n, [13200.0])[0] for i in range(nin)]
    p = Pair(96000, nin, nch, tunings, L, inputs)
    refs = p.refs(96000, tunings, L, range(p.S))

    def call(pos, length, ent, what):
        if ent:
            for h in (p.d, p.a):
                h.plan_tunings(*plan_of(ent))
        assert p.d.planned() == sum(len(v) for v in ent.values())
        p.call(pos, length, what=what)
        assert p.d.planned() == 0
        assert p.d.front_kernel_name() == ("k_chan_front_pst_plan" if ent else "k_chan_front_pst"), what
        for s, r in refs.items():
            same_call(p.d, s, r, r.call(pos, length, ent.get(s, ())), (what, "one-stream reference", s))
            if ent.get(s):
                assert p.d.stream_tuning(s) == float(ent[s][-1][1]), (what, s)

    call(0, first, {}, "before")
    call(first, L, entries, "planned")
    assert p.d.stream_tuning(1) == 12010.5 and p.d.control()[0] == entries[0][-1][1]
    assert p.d.state(5)[0] <= 0.0  # stream 5 is below 0: its last 26 samples passed through unmixed
    call(first + L, after, {}, "after")  # one-shot: the plain kernel again, from the kept indices of the last 26 samples
    assert p.d.state(5)[0] > 0.0


# ---- 6
def test_ramp_plans_of_both_signs_through_zero_and_as_steps():
    first, L, after = 4099, 20000, 3000
    n = first + L + after
    P = P_OF(L)
    nin, nch = 2, 3
    tunings = [12000.0, 12010.5, 30.0, 11987.25, 12000.5, 11999.0]
    ramps = {
        0: [(a, 12000.0 + 7.25 * (i + 1) * (-1) ** i, 0.01 * (i + 1) * (-1) ** (i // 2)) for i, a in enumerate(P)],  # every position
        # (1: none)
        2: [(100, 30.0, -0.05)],                                # down through 0 Hz at k = 600, on to the call's end
        3: [(64, 11990.0, 0.003), (2586, 12030.0, 0.0)],        # a ramp, then a zero slope: a hold
        4: [(63, 12005.0, 0.04), (63 + 140, 12010.75, 0.0)],    # a short ramp: also as one step entry per sample
        5: [(1999, 11999.0, 0.02), (2001, 12001.0, -0.01)],     # across the edge of k_chan_front_pst's tile of 200 outputs
    }
    inputs = [mixed_input(540 + i, n, [13200.0])[0] for i in range(nin)]
    p = Pair(96000, nin, nch, tunings, L, inputs)
    steps = J.BpskTunedChannels(96000, 8192, nin, nch, tunings, max_batch_samples=L)  # stream 4's ramp as a step plan
    ref4 = p.refs(96000, tunings, L, [4])[4]
    st4 = expand({4: ramps[4]}, L)

    def call(pos, length, planned, what):
        if planned:
            for h in (p.d, p.a):
                h.plan_ramps(*ramps_of(ramps))
            steps.plan_tunings(*plan_of(st4))
        p.call(pos, length, what=what)
        steps.batch_i16(p.buf.ptr + 4 * pos, 2 * n, length)
        assert p.d.planned() == 0 and steps.planned() == 0
        assert p.d.front_kernel_name() == ("k_chan_front_pst_ramp" if planned else "k_chan_front_pst"), what
        assert steps.front_kernel_name() == ("k_chan_front_pst_plan" if planned else "k_chan_front_pst"), what
        same_stream(p.d, steps, 4, (what, "as steps"))
        same_call(p.d, 4, ref4, ref4.call(pos, length, st4[4] if planned else ()), (what, "one-stream reference"))

    call(0, first, False, "before")
    call(first, L, True, "ramps")
    assert p.a.front_kernel_name() == "k_front_pst_ramp"
    assert p.d.stream_tuning(2) == 30.0 + float(L - 1 - 100) * -0.05 and p.d.state(2)[0] <= 0.0
    assert p.d.stream_tuning(3) == 12030.0 and p.d.stream_tuning(1) == 12010.5
    assert p.d.control()[0] == p.d.stream_tuning(0) == ramps[0][-1][1]  # (an entry at L - 1: k = 0)
    call(first + L, after, False, "after")  # the streams stand where their ramps ended


# ---- 7
def test_float_input_alternating_forms_and_a_refused_call_that_keeps_the_plan():
    """int16 and float calls alternate as a channel handle allows; the int16 call after arbitrary floats is refused and changes
    nothing, a pending plan included, which the next call then takes"""
    frame = 2048
    nin, nch = 2, 3
    tunings = [12000.5, -700.25, 23999.0, 12010.0, 12000.5, 300.75]
    forms = [("i16", 3), ("java", 2), ("i16", 1), ("any", 3), ("refused", 1), ("any", 1), ("java", 1)]
    N = frame * sum(f for form, f in forms if form != "refused")
    xs = [mixed_input(550 + i, N, [13200.0])[0] for i in range(nin)]
    rng = np.random.default_rng(62)
    fls = []
    for i in range(nin):
        fl = O.convert_i16(xs[i]).astype(np.float32)  # JavaAudio's (float)s/32767f
        pos = 0
        for form, f in forms:
            if form == "any":  # not (float)s/32767f values
                seg = slice(2 * pos * frame, 2 * (pos + f) * frame)
                fl[seg] = (fl[seg] * np.float32(0.7) + rng.normal(0.0, 0.01, 2 * f * frame).astype(np.float32)) * np.float32(1.0001)
            if form != "refused":
                pos += f
        fls.append(fl)
    p = Pair(96000, nin, nch, tunings, 3 * frame, xs, fls)
    refs = p.refs(96000, tunings, 3 * frame, (1, 5))
    entries = {1: [(0, -690.5), (26, -700.25)], 3: [(2047, 12020.25)], 5: [(25, 310.0)]}
    pos, pending = 0, {}
    for form, f in forms:
        L = f * frame
        if form == "refused":
            for h in (p.d, p.a):
                h.plan_tunings(*plan_of(entries))
            pending = entries
            before = _outputs(p.d, p.S), [p.d.stream_tuning(s) for s in range(p.S)]
            for h, b in ((p.d, p.buf), (p.a, p.dup)):
                with pytest.raises(J.JsdrError, match="32767"):
                    h.batch_i16(b.ptr + 4 * pos * frame, 2 * N, L)
            assert (_outputs(p.d, p.S), [p.d.stream_tuning(s) for s in range(p.S)]) == before
            assert p.d.planned() == sum(len(v) for v in entries.values())  # the plan survives the refused call
            continue
        p.call(pos * frame, L, f32=form != "i16", what=(form, pos))
        assert p.d.planned() == 0
        assert p.d.front_kernel_name() == ("k_chan_front_pst_plan" if pending else "k_chan_front_pst"), (form, pos)
        for s, r in refs.items():
            r.buf = p.buf if form == "i16" else p.buf32
            same_call(p.d, s, r, r.call(pos * frame, L, pending.get(s, ()), f32=form != "i16"), (form, pos, "one-stream reference", s))
        pending = {}
        pos += f


def test_dc_correction_with_wrapping_samples():
    """ic, qc as JavaAudio adds them: (short)(s + ic) wraps at 32767 + ic"""
    nin, nch = 2, 3
    chunks = [4099, 6000]
    n = sum(chunks)
    inputs = [mixed_input(560 + i, n, [13200.0])[0].copy() for i in range(nin)]
    for x in inputs:
        x[7::97] = 32767
        x[8::101] = -32768
        x[50:52] = 32767  # inside the first call's first window, and kept in the history of the next
        x[2 * chunks[0] - 4:2 * chunks[0]] = [32767, -32768, 32766, -32767]
    tunings = [12000.5, 11987.25, -5.5, 12000.0, 12010.5, 12000.5]
    p = Pair(96000, nin, nch, tunings, max(chunks), inputs)
    refs = p.refs(96000, tunings, max(chunks), (1, 2, 5))
    pos = 0
    for (ic, qc), L in zip([(5, -7), (-3, 2)], chunks):
        p.call(pos, L, ic=ic, qc=qc, what=("dc", ic, qc))
        for s, r in refs.items():
            r.r.batch_i16(p.buf.ptr + 4 * ((s // nch) * n + pos), 2 * n, L, ic, qc)
            same_call(p.d, s, r, (r.r.bits(), r.r.trace(), r.r.fec_results()), ("one-stream reference", ic, qc, s))
        pos += L


# ---- 8
@pytest.mark.parametrize("f32", [False, True], ids=["i16", "f32"])
def test_padded_input_stride_base_offset_and_guarded_slots(f32):
    """two inputs 33 pairs apart behind a one-pair base offset, poison in the lead, the gap and the tail: a read past an input's row,
    or at stream * stride where input * stride is meant, changes a result.  The handle's dm rows are its own and cannot be read
    through the ABI: a store outside the row of its stream lands in another stream's row or its 64-sample halo, and every stream is
    compared with reference A after every call.  pack_slots writes 16 bytes into a guarded buffer."""
    nin, nch = 2, 5
    chunks = [77, 4099, 26, 20000]
    n = sum(chunks)
    x16 = [mixed_input(570 + i, n, [13200.0, 25200.0])[0] for i in range(nin)]
    rows = [(x.astype(np.float32) / np.float32(32767.0) * np.float32(0.9)).astype(np.float32) for x in x16] if f32 else x16
    tunings = [12000.5 + 3.25 * s for s in range(nin * nch)]
    stride = 2 * n + 66
    buf, starts = LY.build_input(rows, stride, lead=2, tail=2 * 33, unit=2, seed=9)
    assert starts == [2, 2 + stride]
    d_in = J.DeviceBuffer.from_host(buf)
    d_dup = J.DeviceBuffer.from_host(np.concatenate([r for r in rows for _ in range(nch)]))
    d = J.BpskTunedChannels(96000, 8192, nin, nch, tunings, max_batch_samples=max(chunks))
    a = J.BpskTuned(96000, 8192, tunings, max_batch_samples=max(chunks))
    b = buf.itemsize
    pos = 0
    for L in chunks:
        if f32:
            d.batch_f32(d_in.ptr + b * (2 + 2 * pos), stride, L)
            a.batch_f32(d_dup.ptr + b * 2 * pos, 2 * n, L)
        else:
            d.batch_i16(d_in.ptr + b * (2 + 2 * pos), stride, L)
            a.batch_i16(d_dup.ptr + b * 2 * pos, 2 * n, L)
        same_as_twin(d, a, nin * nch, ("padded", f32, pos))
        pos += L
    assert np.array_equal(d_in.to_host(buf.dtype).view(np.uint8), buf.view(np.uint8))  # the input and its poison: read only
    info = d.slot_info()
    assert info == a.slot_info()
    lay = LY.Layout(nin * nch, info["slot_bytes"], lead=16, tail=64)
    got = []
    for h in (d, a):
        out = J.DeviceBuffer.from_host(LY.guard_fill(lay.nbytes))
        h.sync()
        h.pack_slots(out.ptr + 16)
        J.binding.stream_sync()
        raw = out.to_host(np.uint8)
        LY.check_guards(raw, lay, "slots")
        got.append(lay.rows_of(raw))
    assert np.array_equal(got[0], got[1])
    with pytest.raises(J.JsdrError, match="input stride"):  # the stride is between inputs, and too small for the call
        d.batch_i16(d_in.ptr, 2 * 4099 - 2, 4099)


# ---- 9
def test_refusals_name_the_creator_and_leave_the_handle_untouched():
    gc.collect()
    L = 2600
    nin, nch = 2, 3
    tunings = [12000.0, 12010.5, -5000.0, 12000.5, 300.75, 12000.0]
    S = nin * nch
    lib = J.lib()
    t_, f_, u_ = C.c_double(), C.c_int(), C.c_int()
    nbytes = C.c_size_t()
    blob = np.zeros(4096, np.uint8)
    frame_i16 = np.zeros(2 * 2048, np.int16)
    frame_f32 = np.zeros(2 * 2048, np.float32)
    base = J.live_resources()
    for bad_nin, bad_nch in ((4096, 16), (2, 17)):  # a create refused for its geometry holds nothing
        with pytest.raises(J.JsdrError, match="jsdr_bpsk_create_tuned_channels"):
            J.BpskTunedChannels(96000, 8192, bad_nin, bad_nch, [12000.0] * max(bad_nin * bad_nch, 1), max_batch_samples=L)
    hp = C.c_void_p()
    assert lib.jsdr_bpsk_create_tuned_channels(C.byref(hp), 96000, 2048, 2, 0, (C.c_double * 1)(12000.0), C.c_int64(L)) != 0 and not hp.value
    assert "nchannels 0" in lib.jsdr_last_error().decode()
    with pytest.raises(J.JsdrError, match="below the rate"):
        J.BpskTunedChannels(96000, 8192, nin, nch, tunings[:-1] + [96000.0], max_batch_samples=L)
    gc.collect()
    assert J.live_resources() == base

    def held():  # (its locals, the exceptions' frames among them, go when it returns)
        a = J.BpskTunedChannels(96000, 8192, nin, nch, tunings, max_batch_samples=L)
        b = J.BpskTunedChannels(96000, 8192, nin, nch, tunings, max_batch_samples=L)
        assert J.live_resources()[0] > base[0]
        CR = "jsdr_bpsk_create_tuned_channels"
        refusals = [
            (CR, lambda: a.set_mode(1, 0)),
            (CR, lambda: a.reconfigure(12000.0, 1, 0)),
            (CR, _rc(lambda: lib.jsdr_bpsk_set_variant(a.h, 1))),
            (CR, lambda: a.receive_raw(frame_i16)),
            (CR, lambda: a.receive(frame_f32)),
            ("jsdr_bpsk_set_stream_tuning", _rc(lambda: lib.jsdr_bpsk_set_channel_tuning(a.h, 0, C.c_double(100.0)))),
            (CR, _rc(lambda: lib.jsdr_bpsk_set_channel_mode(a.h, 0, 0, 1))),
            ("jsdr_bpsk_get_stream_tuning", _rc(lambda: lib.jsdr_bpsk_get_channel_control(a.h, 0, C.byref(t_), C.byref(f_), C.byref(u_)))),
            ("one input history per input", _rc(lambda: lib.jsdr_bpsk_state_bytes(a.h, 1, C.byref(nbytes)))),
            ("one input history per input", _rc(lambda: lib.jsdr_bpsk_save(a.h, 0, 1, blob.ctypes.data_as(C.c_void_p), C.c_size_t(blob.size),
                                                                          C.byref(nbytes)))),
            ("one input history per input", _rc(lambda: lib.jsdr_bpsk_restore(a.h, 0, blob.ctypes.data_as(C.c_void_p), C.c_size_t(blob.size)))),
            ("below the rate", lambda: a.set_stream_tuning(0, 96000.0)),
            ("out of range", lambda: a.set_stream_tuning(S, 100.0)),
            ("input stride", lambda: a.batch_i16(d_iq.ptr, 2 * L - 2, L)),
            ("outside", lambda: a.batch_i16(d_iq.ptr, 2 * L + 2, L + 1)),
        ]
        n = L * (len(refusals) + 1)
        inputs = [mixed_input(580 + i, n, [13200.0])[0] for i in range(nin)]
        d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
        for h in (a, b):
            h.batch_i16(d_iq.ptr, 2 * n, L)
        for k, (what, bad) in enumerate(refusals):
            with pytest.raises(J.JsdrError, match=what) as err:
                bad()
            if "history" in what:
                assert CR in str(err.value)
            assert [a.stream_tuning(s) for s in range(S)] == tunings and a.control() == (12000.0, 0, 0), what
            for h in (a, b):
                h.batch_i16(d_iq.ptr + 4 * L * (k + 1), 2 * n, L)
            assert _outputs(a, S) == _outputs(b, S), (k, what)
        # the whole-handle controls it does take, as a tuned handle does
        a.set_mode(0, 1)
        assert a.control() == (12000.0, 0, 1) and a.counters(0)["dmMaxCorr"] == 0
        a.reconfigure(11000.0, 0, 0)
        assert [a.stream_tuning(s) for s in range(S)] == [11000.0] * S and a.control() == (11000.0, 0, 0)
        a.set_tuning(-12.5)
        assert [a.stream_tuning(s) for s in range(S)] == [-12.5] * S

    held()
    gc.collect()
    assert J.live_resources() == base


# ---- 10
def test_pack_slots_equal_the_tuned_handles():
    nin, nch = 2, 5
    L = 50000
    inputs = [mixed_input(590 + i, L, [13200.0, 25200.0])[0] for i in range(nin)]
    tunings = [12000.0, 24000.0, 12010.5, -5000.0, 11999.25, 24000.5, 12000.0, 0.0, 23990.0, 12001.0]
    p = Pair(96000, nin, nch, tunings, L, inputs)
    p.call(0, L, what="one call")
    info = p.d.slot_info()
    assert info == p.a.slot_info()
    got = []
    for h in (p.d, p.a):
        slots = J.DeviceBuffer(info["slot_bytes"] * p.S)
        h.pack_slots(slots.ptr)
        J.binding.stream_sync()
        got.append(slots.to_host(np.uint8).reshape(p.S, -1))
    assert np.array_equal(got[0], got[1])
