"""GPU: jsdr_bpsk_batch_f32 -- float IQ batches through the BPSK demodulator (IAudioHandler.receive(float[]) batched: the floats
are taken as the reference takes buf[], x = (double)f).  Everything is bit for bit: against the C oracle fed the same floats,
against one-stream handles fed receive(), against the int16 form on floats of the short grid, on ordinary handles in the tune
mode (the fused float kernel k_fm_f32 and the three-kernel path) and in FFT-acquire, and on channel handles.

Sizes sit around k_fm_f32's seams: a tile is 62 x 65 = 4030 outputs (40 300 samples at /10), its short-call form takes calls
of at most 512 outputs, a window reaches 26 samples back into the previous call."""
import os
import subprocess
import sys

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O
import test_gpu_bpsk_live_control as LC  # act / actions / check and the fixtures (scenarios as there, a new input form here)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 62 * 65
CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK", "centreBin")
# JSDR_KNOBS=1 JSDR_FM=0 (test 1's child process): every tune-mode call takes the three-kernel path
FUSED = not (os.environ.get("JSDR_KNOBS") == "1" and os.environ.get("JSDR_FM") == "0")


def offgrid(raw):
    """floats off the int16 grid, as the float tests of test_gpu_bpsk.py make them"""
    return (O.convert_i16(raw) * np.float32(0.93)).astype(np.float32)


def awkward(x):
    """values above 1.0, some -0.0, subnormals and a silent stretch (no NaN, no Inf) in a copy of x"""
    x = x.copy()
    n = x.size
    x[100:140] *= np.float32(40.0)
    assert np.abs(x[100:140]).max() > 1.0
    x[n // 3:n // 3 + 6000] = 0.0
    x[n // 3 + 11:n // 3 + 300:7] = np.float32(-0.0)
    x[n // 2:n // 2 + 64] = np.float32(1e-41) * np.arange(1, 65, dtype=np.float32)  # subnormal
    x[n // 2 + 64:n // 2 + 96:2] = np.float32(-3e-42)
    x[-50:] *= np.float32(-7.5)
    return x


class Acc:
    """what S streams of a handle produced, accumulated over its calls"""

    def __init__(self, S, get=None):
        self.S = S
        self.bits = [[] for _ in range(S)]
        self.trace = [[] for _ in range(S)]
        self.fec = [[] for _ in range(S)]
        self.get = get or (lambda s: (s,))

    def take(self, d):
        for s in range(self.S):
            a = self.get(s)
            self.bits[s].append(d.bits(*a).copy())
            self.trace[s].append(d.trace(*a).copy())
            self.fec[s].extend(d.fec_results(*a))

    def of(self, d, s):
        """everything of stream s, in comparable form"""
        a = self.get(s)
        c = d.counters(*a)
        return dict(trace=np.concatenate(self.trace[s]).tobytes(), bits=np.concatenate(self.bits[s]).tobytes(),
                    counters=[c[k] for k in CKEYS], state=d.state(*a).tobytes(),
                    fec=[(rc, bi, data.tobytes()) for rc, bi, data in self.fec[s]], decoded=d.decoded(*a).tobytes())


def same(a, b, where):
    for k in a:
        assert a[k] == b[k], (where, k)


def against_oracle(acc, d, s, o, fft, where):
    got = acc.of(d, s)
    assert got["trace"] == o.trace().tobytes(), (where, "(fi,fq)")
    assert got["bits"] == o.bits().tobytes(), (where, "bits")
    oc = o.counters()
    for k, v in zip(CKEYS, got["counters"]):
        if k != "centreBin" or fft:
            assert v == oc[k], (where, k, v, oc[k])
    gs, os_ = np.frombuffer(got["state"]), o.state()
    for i in range(18):
        if i not in (6, 7) or fft:  # (avePeakPower, aveCentreBin: live in FFT-acquire)
            assert gs[i] == os_[i], (where, "state", i, gs[i], os_[i])
    fo = o.fec_results()
    assert len(got["fec"]) == len(fo), (where, len(got["fec"]), len(fo))
    for (rc, _, data), (orc, _, odata) in zip(got["fec"], fo):
        assert rc == orc and data == odata.tobytes(), where
    assert got["decoded"] == o.decoded().tobytes(), where


def padded(xs, pos, L, pad=6):
    """the call's samples of every stream in a [S][2 L + pad] device buffer whose padding is NaN: a read outside a stream's
    samples of THIS call poisons its trace.  -> (buffer, stride in floats)"""
    h = np.full((len(xs), 2 * L + pad), np.nan, np.float32)
    for s, x in enumerate(xs):
        h[s, :2 * L] = x[2 * pos:2 * (pos + L)]
    return J.DeviceBuffer.from_host(h), 2 * L + pad


def feed_f32(d, xs, calls, acc, names=None, between=None):
    pos = 0
    for c, L in enumerate(calls):
        if between:
            between(c)
        buf, stride = padded(xs, pos, L)
        d.batch_f32(buf.ptr, stride, L)
        acc.take(d)
        if names is not None:
            names.append(d.front_kernel_name())
        pos += L
    return pos


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("tuning", [12000, 0, -3000, 12010])
@pytest.mark.parametrize("rate", [96000, 48000, 192000, 44100])
def test_tune_mode_against_the_oracle(rate, tuning):
    D = rate // 9600
    # 2 tiles and a remainder; at most 512 outputs (the short-call form); shorter than the 26-sample history; 2 tiles again.
    # None is a multiple of the decimation: dsCnt and first_out move.
    calls = [2 * TILE * D + 1237, 500 * D - 3, 19, 2 * TILE * D + 7]
    assert all(L % D for L in calls) and (calls[1] + D) // D <= 512
    N = sum(calls)
    raws = [O.make_dbpsk_stream(5100 + s, s, N, rate=rate, carrier_hz=abs(tuning) + 1200.0, noise_sigma=500.0 + 400 * s)[0] for s in range(3)]
    xs = [offgrid(r) for r in raws]
    xs[2] = awkward(xs[2])
    d = J.Bpsk(rate=rate, tuning=tuning, nstreams=3, max_batch_samples=max(calls))
    acc, names = Acc(3), []
    assert feed_f32(d, xs, calls, acc, names) == N
    for s in range(3):
        o = O.Bpsk(rate=rate, blen=4 * N, tuning=tuning, trace=N // D + 8)  # (sample-sequential: one frame of N samples)
        o.receive(xs[s])
        against_oracle(acc, d, s, o, False, (rate, tuning, s))
    # the kernel: the fused float kernel exactly where an int16 call of this schedule takes k_fm, k_front everywhere else
    z = J.DeviceBuffer.from_host(np.zeros(2 * max(calls), np.int16))
    d16 = J.Bpsk(rate=rate, tuning=tuning, nstreams=1, max_batch_samples=max(calls))
    for c, L in enumerate(calls):
        d16.batch_i16(z.ptr, 2 * L, L)
        if c != 2:  # (the 19-sample call may have no output at all: no front end runs)
            want = "k_fm_f32" if (FUSED and d16.front_kernel_name() == "k_fm") else "k_front"
            assert names[c] == want, (rate, tuning, c, names, d16.front_kernel_name())
    if FUSED and (tuning <= 0 or (rate, tuning) == (96000, 12000)):  # no tuner; the exact 8-cycle
        assert [names[c] for c in (0, 1, 3)] == ["k_fm_f32"] * 3, names
    if (rate, tuning) == (96000, 12010):  # not periodic
        assert [names[c] for c in (0, 1, 3)] == ["k_front"] * 3, names


def test_tune_mode_once_more_on_the_three_kernel_path():
    """JSDR_FM=0 (behind JSDR_KNOBS=1) forces the three-kernel path for float batches too: test 1 again in a child process"""
    if not FUSED:
        return
    env = dict(os.environ, JSDR_KNOBS="1", JSDR_FM="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__),
                        "-k", "test_tune_mode_against_the_oracle"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "16 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------- 2
def slots_of(d, nstreams):
    info = d.slot_info()
    buf = J.DeviceBuffer(info["slot_bytes"] * nstreams)
    d.pack_slots(buf.ptr)
    J.binding.stream_sync()
    return buf.to_host(np.uint8).reshape(nstreams, -1).copy()


def test_floats_of_the_short_grid_equal_the_int16_form():
    S = 40
    calls = [7 * TILE * 10 + 11, TILE * 10 - 5]  # (7 tiles and a bit: 8 work items a stream, 320 in all)
    N = sum(calls)
    raws = [O.make_dbpsk_stream(6200 + s, s, N, noise_sigma=400.0 + 60 * s)[0] for s in range(S)]
    xs = [O.convert_i16(r) for r in raws]  # exactly (float)s / 32767f
    d_raw = J.DeviceBuffer.from_host(np.concatenate(raws))
    d_x = J.DeviceBuffer.from_host(np.concatenate(xs))
    res = {}
    for form in ("i16", "f32", "f32_share"):
        d = J.Bpsk(nstreams=S, max_batch_samples=max(calls))
        if form == "f32_share":
            d.set_cu_share(1)
        acc, slots, pos = Acc(S), [], 0
        for c, L in enumerate(calls):
            if form == "i16":
                d.batch_i16(d_raw.ptr + 4 * pos, 2 * N, L)
            else:
                d.batch_f32(d_x.ptr + 8 * pos, 2 * N, L)
            acc.take(d)
            slots.append(slots_of(d, S))
            assert d.front_kernel_name() == ("k_fm" if form == "i16" else "k_fm_f32")
            if c == 0:
                items, wgs = d.last_launch()
                assert items == 8 * S
                assert (wgs < items) if form == "f32_share" else (wgs == items), (form, items, wgs)
            pos += L
        res[form] = ([acc.of(d, s) for s in range(S)], slots)
        if form == "f32":
            for s in (0, 17, 39):
                o = O.Bpsk(blen=4, trace=N // 10 + 8)
                o.receive_i16(raws[s])
                against_oracle(acc, d, s, o, False, s)
    for form in ("f32", "f32_share"):
        for s in range(S):
            same(res[form][0][s], res["i16"][0][s], (form, s))
        for a, b in zip(res[form][1], res["i16"][1]):
            assert a.tobytes() == b.tobytes(), form


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("do_fft", [0, 1])
def test_a_batch_equals_receive_frame_by_frame(do_fft):
    n, frames = 2048, [5, 1, 7, 11]
    N = n * sum(frames)
    xs = [offgrid(O.make_dbpsk_stream(7300 + s, s, N, noise_sigma=700.0)[0]) for s in range(3)]
    d = J.Bpsk(do_fft=do_fft, nstreams=3, max_batch_samples=n * max(frames))
    acc = Acc(3)
    feed_f32(d, xs, [n * f for f in frames], acc)
    for s in range(3):
        d1 = J.Bpsk(do_fft=do_fft, nstreams=1)
        a1 = Acc(1)
        for k in range(N // n):
            d1.receive(xs[s][2 * n * k:2 * n * (k + 1)])
            a1.take(d1)
        same(acc.of(d, s), a1.of(d1, 0), (do_fft, s))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("rate,n,per_call", [(96000, 2048, 4), (96000, 2048, 1), (96000, 9600, 2), (44100, 4410, 2), (96000, 512, 4)])
@pytest.mark.parametrize("do_up", [0, 1])
def test_fft_acquire_against_the_oracle(rate, n, per_call, do_up):
    N = 2 * per_call * n
    carrier = 30000.0 if do_up else 13200.0
    if rate == 44100:
        carrier = 14000.0 if do_up else 6000.0
    xs = [offgrid(O.make_dbpsk_stream(8400 + s, s, N, rate=rate, carrier_hz=carrier, noise_sigma=600.0 + 200 * s)[0]) for s in range(3)]
    d = J.Bpsk(rate=rate, blen=4 * n, do_fft=1, do_up=do_up, nstreams=3, max_batch_samples=per_call * n)
    acc = Acc(3)
    feed_f32(d, xs, [per_call * n] * 2, acc)
    for s in range(3):
        o = O.Bpsk(rate=rate, blen=4 * n, do_fft=1, do_up=do_up, trace=N // (rate // 9600) + 8)
        for k in range(N // n):
            o.receive(xs[s][2 * n * k:2 * n * (k + 1)])
        against_oracle(acc, d, s, o, True, (rate, n, per_call, do_up, s))  # (centreBin, avePeakPower, aveCentreBin with it)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", list(LC.M.SCENARIOS))
def test_live_control_between_float_batches(name):
    """every scenario of the live-control fixtures as test_gpu_bpsk_live_control.run feeds it, through batch_f32 with 5 streams
    (k_front_split<F32IN> and the float k_seam_hist with more than one stream)"""
    S = 5
    p = LC.M.SCENARIOS[name]
    buf = O.convert_i16(LC.M.scenario_input(name))
    n, calls, N = p["frame"], p["calls"], sum(p["calls"])
    d = J.Bpsk(rate=p["rate"], blen=4 * n, tuning=p["tuning"], do_fft=p["do_fft"], do_up=p["do_up"], nstreams=S, max_batch_samples=max(calls))
    d_x = J.DeviceBuffer.from_host(np.tile(buf, S))
    acts = LC.actions(name)
    rec = [[] for _ in range(S)]
    pos = 0
    for c, L in enumerate(calls):
        for cmd, v in acts.get(c, []):
            LC.act(d, cmd, v)
        d.batch_f32(d_x.ptr + 8 * pos, 2 * N, L)
        pos += L
        for s in range(S):
            rec[s].append((list(d.counters(s).values()), d.state(s).copy(), d.bits(s).copy(), d.fec_results(s), [d.front_kernel_name()]))
    for s in (0, 4):
        LC.check(name, rec[s])
    for s in (1, 2, 3):
        for a, b in zip(rec[s], rec[0]):
            assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), (name, s)
            assert [(r[0], r[2].tobytes()) for r in a[3]] == [(r[0], r[2].tobytes()) for r in b[3]], (name, s)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_the_two_input_forms_alternate_on_one_handle():
    S = 3
    calls = [TILE * 10 + 333, 2048, TILE * 10 * 2 - 17, 4999, 17, TILE * 10 + 5]
    forms = ["f32", "i16", "f32", "f32", "i16", "i16"]  # both hand-overs, also behind a short call and a 17-sample one
    N = sum(calls)
    raws = [O.make_dbpsk_stream(9500 + s, s, N, noise_sigma=500.0)[0] for s in range(S)]
    d_raw = J.DeviceBuffer.from_host(np.concatenate(raws))
    d_x = J.DeviceBuffer.from_host(np.concatenate([O.convert_i16(r) for r in raws]))
    a = J.Bpsk(nstreams=S, max_batch_samples=max(calls))
    b = J.Bpsk(nstreams=S, max_batch_samples=max(calls))
    acc_a, acc_b, pos = Acc(S), Acc(S), 0
    for L, form in zip(calls, forms):
        if form == "f32":
            a.batch_f32(d_x.ptr + 8 * pos, 2 * N, L)
        else:
            a.batch_i16(d_raw.ptr + 4 * pos, 2 * N, L)
        b.batch_i16(d_raw.ptr + 4 * pos, 2 * N, L)
        acc_a.take(a)
        acc_b.take(b)
        assert a.front_kernel_name() == ("k_fm_f32" if form == "f32" else "k_fm"), (L, form)
        pos += L
    for s in range(S):
        same(acc_a.of(a, s), acc_b.of(b, s), s)


def test_int16_after_other_floats_is_refused_and_the_handle_unchanged():
    S = 3
    calls = [TILE * 10 + 99, 3001, TILE * 10]
    N = sum(calls)
    raws = [O.make_dbpsk_stream(9600 + s, s, N, noise_sigma=500.0)[0] for s in range(S)]
    xs = [offgrid(r) for r in raws]
    d_raw = J.DeviceBuffer.from_host(np.concatenate(raws))
    d_x = J.DeviceBuffer.from_host(np.concatenate(xs))
    a = J.Bpsk(nstreams=S, max_batch_samples=max(calls))
    b = J.Bpsk(nstreams=S, max_batch_samples=max(calls))
    acc_a, acc_b, pos = Acc(S), Acc(S), 0
    for c, L in enumerate(calls):
        if c > 0:
            with pytest.raises(J.JsdrError, match="cannot be carried over"):
                a.batch_i16(d_raw.ptr + 4 * pos, 2 * N, L)
        for h, acc in ((a, acc_a), (b, acc_b)):
            h.batch_f32(d_x.ptr + 8 * pos, 2 * N, L)
            acc.take(h)
        pos += L
    for s in range(S):
        same(acc_a.of(a, s), acc_b.of(b, s), s)
        o = O.Bpsk(blen=4 * N, trace=N // 10 + 8)
        o.receive(xs[s])
        against_oracle(acc_a, a, s, o, False, s)


# ---------------------------------------------------------------------------------------------------------------- 7
def channel_inputs(seed, n, nin):
    out = []
    for i in range(nin):
        acc = np.zeros(2 * n, np.int64)
        for k, f in enumerate((13200.0, 31200.0)):
            acc += O.make_dbpsk_stream(seed + i, k, n, carrier_hz=f, noise_sigma=900.0)[0].astype(np.int64)
        out.append(offgrid(np.clip(acc, -32768, 32767).astype(np.int16)))
    return out


def run_channels(d, chans, xs, calls, retune, frame=2048):
    """the channel handle d and one ordinary one-stream handle per (input, channel) through the same float calls, `retune` =
    (channel, tuning) applied before the second call -> (acc of d, [[(handle, acc)]])"""
    nin, K = len(xs), len(chans)
    acc = Acc(nin * K, get=lambda s: (s // K, s % K))
    singles = [[(J.Bpsk(blen=4 * frame, tuning=t, do_fft=f, do_up=u, nstreams=1, max_batch_samples=max(calls)), Acc(1)) for t, f, u in chans]
               for _ in range(nin)]
    pos = 0
    for c, L in enumerate(calls):
        if c == 1:
            d.set_channel_tuning(*retune)
            for i in range(nin):
                singles[i][retune[0]][0].set_tuning(retune[1])
        buf, stride = padded(xs, pos, L)
        d.batch_f32(buf.ptr, stride, L)
        acc.take(d)
        for i in range(nin):
            for h, a1 in singles[i]:
                h.batch_f32(buf.ptr + 4 * stride * i, stride, L)
                a1.take(h)
        pos += L
    for i in range(nin):
        for k in range(K):
            h, a1 = singles[i][k]
            same(acc.of(d, i * K + k), a1.of(h, 0), (i, k))
    return acc


def test_channel_handle_in_the_tune_mode():
    chans = [(12000, 0, 0), (12010, 0, 0), (-3000, 0, 0)]
    calls = [256 * 10 * 3 + 77, 256 * 10 + 1230]  # (k_chan_front: 256 outputs a workgroup; more than one, the last one partial)
    N = sum(calls)
    xs = channel_inputs(1100, N, 2)
    d = J.BpskChannels(96000, 8192, [t for t, _, _ in chans], ninputs=2, max_batch_samples=max(calls))
    acc = run_channels(d, chans, xs, calls, (1, 11990.0))
    assert d.front_kernel_name() == "k_chan_front"
    for i, k in ((0, 0), (1, 2)):  # (channels that were not retuned)
        o = O.Bpsk(blen=4 * N, tuning=chans[k][0], trace=N // 10 + 8)
        o.receive(xs[i])
        against_oracle(acc, d, i * 3 + k, o, False, (i, k))
    # receive() keeps its rule on a channel handle: JavaAudio's values only
    d1 = J.BpskChannels(96000, 8192, [12000, 12010], ninputs=1)
    with pytest.raises(J.JsdrError, match="32767f"):
        d1.receive(xs[0][:4096])


@pytest.mark.parametrize("frame", [2048, 9600])
def test_channel_handle_with_fft_acquire_channels(frame):
    chans = [(12000, 0, 0), (12000, 1, 0), (12000, 1, 1), (30000, 0, 0)]
    calls = [3 * frame, 2 * frame]
    N = sum(calls)
    xs = channel_inputs(1200, N, 2)
    d = J.BpskChannels(96000, 4 * frame, [t for t, _, _ in chans], do_up=[u for _, _, u in chans], ninputs=2,
                       max_batch_samples=max(calls), do_fft=[f for _, f, _ in chans])
    acc = run_channels(d, chans, xs, calls, (3, 30010.0), frame)
    # float input: the forward phase once per band in use (no both-band float transform), inverses per channel
    assert d.front_kernel_name() == ("k_acq_fwd" if frame == 2048 else "k_acqm_fwd")
    assert d.acq_last_launch() == (2 * 2 * 2, 2 * 2 * 2)  # inputs x bands x frames; inputs x FFT channels x frames
    for i, k in ((0, 1), (1, 2)):
        o = O.Bpsk(blen=4 * frame, tuning=12000, do_fft=1, do_up=chans[k][2], trace=N // 10 + 8)
        for f in range(N // frame):
            o.receive(xs[i][2 * frame * f:2 * frame * (f + 1)])
        against_oracle(acc, d, i * 4 + k, o, True, (frame, i, k))


# ---------------------------------------------------------------------------------------------------------------- 8
def _outputs(d, S):
    return [(list(d.counters(s).values()), d.state(s).tobytes(), d.bits(s).tobytes(), d.trace(s).tobytes()) for s in range(S)]


def test_refusals_leave_the_handle_as_it_was():
    S, L = 3, 2048 * 4
    raws = [O.make_dbpsk_stream(1300 + s, s, 2 * L, noise_sigma=500.0)[0] for s in range(S)]
    d_raw = J.DeviceBuffer.from_host(np.concatenate(raws))
    d_x = J.DeviceBuffer.from_host(np.concatenate([offgrid(r) for r in raws]))
    stride = 4 * L

    def twins(**kw):
        return J.Bpsk(nstreams=S, max_batch_samples=L, **kw), J.Bpsk(nstreams=S, max_batch_samples=L, **kw)

    # a FAST handle: its certification re-reads int16
    a, b = twins(variant="fast")
    for h in (a, b):
        h.batch_i16(d_raw.ptr, stride, L)
    with pytest.raises(J.JsdrError, match="fast variant"):
        a.batch_f32(d_x.ptr, stride, L)
    for h in (a, b):
        h.batch_i16(d_raw.ptr + 4 * L, stride, L)
    assert _outputs(a, S) == _outputs(b, S)
    # an exact handle in the tune mode: stride, call length, null pointer
    a, b = twins()
    for h in (a, b):
        h.batch_f32(d_x.ptr, stride, L)
    for args, what in (((d_x.ptr, 2 * L - 2, L), "stride"), ((d_x.ptr, 2 * L + 1, L), "stride"), ((d_x.ptr, stride, L + 1), "max_batch"),
                       ((d_x.ptr, stride, 0), "max_batch"), ((None, stride, L), "null")):
        with pytest.raises(J.JsdrError, match=what):
            a.batch_f32(*args)
    for h in (a, b):
        h.batch_f32(d_x.ptr + 8 * L, stride, L)
    assert _outputs(a, S) == _outputs(b, S)
    assert a.front_kernel_name() == ("k_fm_f32" if FUSED else "k_front")
    # FFT-acquire: whole frames
    a, b = twins(do_fft=1)
    for h in (a, b):
        h.batch_f32(d_x.ptr, stride, L)
    with pytest.raises(J.JsdrError, match="whole frames"):
        a.batch_f32(d_x.ptr + 8 * L, stride, 2048 + 100)
    for h in (a, b):
        h.batch_f32(d_x.ptr + 8 * L, stride, L)
    assert _outputs(a, S) == _outputs(b, S)
    # a channel handle with FFT-acquire channels: whole frames, stride between inputs
    mk = lambda: J.BpskChannels(96000, 8192, [12000, 12000], do_up=[0, 1], ninputs=2, max_batch_samples=L, do_fft=[0, 1])  # noqa: E731
    a, b = mk(), mk()
    for h in (a, b):
        h.batch_f32(d_x.ptr, stride, L)
    with pytest.raises(J.JsdrError, match="whole frames"):
        a.batch_f32(d_x.ptr + 8 * L, stride, 2048 + 100)
    with pytest.raises(J.JsdrError, match="stride"):
        a.batch_f32(d_x.ptr + 8 * L, 2 * L - 2, L)
    for h in (a, b):
        h.batch_f32(d_x.ptr + 8 * L, stride, L)
    for i in range(2):
        for k in range(2):
            assert a.state(i, k).tobytes() == b.state(i, k).tobytes() and a.trace(i, k).tobytes() == b.trace(i, k).tobytes(), (i, k)
