"""GPU: demod channel handles (jsdr_demod_create_channels): ninputs x nchannels demod.receive channels, each with its own band,
NCO, mode and switches, on one IQ input each.  Every stream (i, c) is compared bit for bit with an O.Demod fed input i and
given channel c's controls and actions: the int16 audio of every frame, frame_stats after each call and channel_state."""
import ctypes as C

import numpy as np
import pytest

import big_offsets as BO
import java_sdr_amd as J
import layouts as LY
import oracle_lib as O

from test_gpu_demod import fm_am_signal, same
from test_gpu_layouts import Guarded

pytestmark = pytest.mark.gpu
ALLPASS = (-2 ** 31, 2 ** 31 - 1)
# (mode, dofir, dodwn, doagc, band): one channel per mode, each with its own band and switches
FIVE = [
    (0, 1, 1, 1, (2000, 9000)),
    (1, 1, 0, 1, (-12000, -3000)),
    (2, 1, 1, 1, (2000, 9000)),
    (3, 1, 1, 1, (15000, 30000)),
    (4, 0, 1, 0, ALLPASS),
]


class Bank:
    """a channel handle and one oracle per (input, channel), given the same controls and actions"""

    def __init__(self, rate, n, nin, chans, max_frames):
        self.rate, self.n, self.nin, self.K = rate, n, nin, len(chans)
        self.h = J.DemodChannels(rate, n, nin, self.K, max_frames * n)
        assert self.h.channel_info() == (nin, self.K)
        self.o = [[O.Demod(rate) for _ in range(self.K)] for _ in range(nin)]
        for c in range(self.K):  # a new channel starts as a new ordinary handle does
            assert self.h.channel_control(c) == (0, 0, 0, 0) + ALLPASS and self.h.channel_state(c) == (0.0, 0.0)
        for c, (mode, fir, dwn, agc, band) in enumerate(chans):
            self.configure(c, mode, fir, dwn, agc)
            self.weights(c, *band)

    def configure(self, c, mode, fir=0, dwn=0, agc=0):
        self.h.configure_channel(c, mode, fir, dwn, agc)
        for row in self.o:
            row[c].configure(mode, fir, dwn, agc)

    def weights(self, c, flo, fhi):
        w, phi = self.h.channel_weights(c, flo, fhi)
        for row in self.o:
            ow, ophi = row[c].weights(flo, fhi)
        assert np.array_equal(w, ow) and phi == ophi, c

    def controls_match(self):
        for c in range(self.K):
            d = self.o[0][c].d
            assert self.h.channel_control(c) == (d.mode, d.dofir, d.dodwn, d.doagc, d.flo, d.fhi), c

    def check(self, got, bufs, nf, what=""):
        """got: audio [nin][K][2L]; bufs: the float samples each oracle of input i receives, [nin][2L]"""
        n = self.n
        for i in range(self.nin):
            for c in range(self.K):
                o = self.o[i][c]
                for f in range(nf):
                    want = o.receive(bufs[i][2 * f * n:2 * (f + 1) * n])
                    assert np.array_equal(got[i][c][2 * f * n:2 * (f + 1) * n], want), (what, i, c, f)
                mx, av = self.h.frame_stats(self.h.stream(i, c))
                assert same(mx, o.max) and same(av, o.avg), (what, i, c)
        for c in range(self.K):
            car, phi = self.h.channel_state(c)
            assert car == self.o[0][c].car and phi == np.float32(self.o[0][c].d.phi), (what, c)


def signals(seed, nin, total, rate):
    rng = np.random.default_rng(seed)
    return [fm_am_signal(rng, total, rate, fc=4000.0 + 2100.0 * i, seed_shift=17.0 * i) for i in range(nin)]


def run_calls(bank, raws, frames, ic=0, qc=0, what="", between=None):
    pos = 0
    for k, nf in enumerate(frames):
        if between:
            between(k)
        L = nf * bank.n
        chunk = np.stack([r[2 * pos:2 * (pos + L)] for r in raws])
        got = bank.h.batch_host_i16(chunk, L, ic, qc)
        bank.check(got, [O.convert_i16(x, ic=ic, qc=qc) for x in chunk], nf, (what, k))
        pos += L


def test_three_inputs_five_channels_one_per_mode():
    """AM channels (k_demod_mean + k_demod_chan_out) and FM / RAW / OFF channels (k_demod_chan alone) in the same calls"""
    rate, n, frames = 96000, 2048, [1, 3, 2]
    bank = Bank(rate, n, 3, FIVE, max(frames))
    bank.controls_match()
    run_calls(bank, signals(1, 3, sum(frames) * n, rate), frames)


def test_one_channel_handle_equals_an_ordinary_handle():
    rate, n, S, frames = 96000, 2048, 3, [1, 3, 2]
    raws = signals(2, S, sum(frames) * n, rate)
    lib = J.lib()
    for mode in range(5):
        ch = J.DemodChannels(rate, n, S, 1, max(frames) * n)
        od = J.Demod(rate, n, S, max(frames) * n)
        for h in (ch, od):
            h.configure(mode, 1, 1, 1)
            h.weights(3000, 11000)
            h.profile_enable(True)
        pos = 0
        for nf in frames:
            L = nf * n
            chunk = np.stack([r[2 * pos:2 * (pos + L)] for r in raws])
            a = ch.batch_host_i16(chunk, L)
            b = od.batch_host_i16(chunk, L)
            assert np.array_equal(a[:, 0], b), (mode, nf)
            for s in range(S):
                assert all(same(x, y) for x, y in zip(ch.frame_stats(s), od.frame_stats(s))), (mode, s)
            assert ch.state() == od.state() == ch.channel_state(0)
            pos += L
        pc, po = ch.profile_read(), od.profile_read()
        assert pc["k_demod_chan"][1] > 0 and po["k_demod_chan"][1] == 0, (pc, po)
        assert pc["k_demod_front"][1] == 0 and po["k_demod_front"][1] > 0, (pc, po)
        # an ordinary handle is nstreams x 1 and takes channel 0 in the per-channel calls
        a_, b_ = C.c_int(), C.c_int()
        assert lib.jsdr_demod_channel_info(od.h, C.byref(a_), C.byref(b_)) == 0 and (a_.value, b_.value) == (S, 1)
        v = [C.c_int() for _ in range(6)]
        assert lib.jsdr_demod_get_channel(od.h, 0, *[C.byref(x) for x in v]) == 0
        assert [x.value for x in v] == [mode, 1, 1, 1, 3000, 11000]
        assert lib.jsdr_demod_get_channel(od.h, 1, *[C.byref(x) for x in v]) != 0
        assert lib.jsdr_demod_configure_channel(od.h, 1, 1, 0, 0, 0) != 0


def test_an_ordinary_handle_through_the_channel_form_calls():
    """configure_channel(0) / channel_weights(0) on an ordinary handle are configure / weights: the same audio, byte for byte, the
    same controls and state through either form of getter; channel 1 is refused and nothing of the handle moves"""
    rate, n, S, nf = 96000, 64, 2, 2
    CH = J.DemodChannels  # (its per-channel methods take any demod handle)
    raws = signals(9, S, 2 * nf * n, rate)
    a, b = J.Demod(rate, n, S, nf * n), J.Demod(rate, n, S, nf * n)
    a.configure(3, 1, 1, 0)
    CH.configure_channel(b, 0, 3, 1, 1, 0)
    (wa, pa), (wb, pb) = a.weights(3000, 11000), CH.channel_weights(b, 0, 3000, 11000)
    assert wa.tobytes() == wb.tobytes() and pa == pb and pa != 0
    for k in range(2):
        chunk = np.stack([r[2 * k * nf * n:2 * (k + 1) * nf * n] for r in raws])
        got_a, got_b = a.batch_host_i16(chunk, nf * n), b.batch_host_i16(chunk, nf * n)
        assert got_a.tobytes() == got_b.tobytes() and got_a.any(), k
        assert CH.channel_control(b, 0) == CH.channel_control(a, 0) == (3, 1, 1, 0, 3000, 11000)
        assert CH.channel_state(b, 0) == b.state() == a.state() == CH.channel_state(a, 0), k
        assert b.state()[0] != 0  # (the carrier has moved: the state compared is not the initial one)
    before = (CH.channel_control(b, 0), b.state())
    for refused in (lambda: CH.configure_channel(b, 1, 1, 0, 0, 0), lambda: CH.channel_weights(b, 1, 0, 5000),
                    lambda: CH.channel_control(b, 1), lambda: CH.channel_state(b, 1), lambda: CH.configure_channel(b, -1, 1, 0, 0, 0)):
        with pytest.raises(J.JsdrError, match="channel -?1 outside 0..0"):
            refused()
    assert (CH.channel_control(b, 0), b.state()) == before and CH.channel_info(b) == (S, 1)


def test_live_per_channel_control_between_calls():
    """configure_channel on one channel, filterMove steps applied with channel_weights, the all-pass impulse on one channel,
    then a handle-wide configure / weights; the channels no action touched stay equal to their own oracles"""
    rate, n = 96000, 2048
    chans = [(3, 1, 1, 1, (2000, 9000)), (2, 1, 1, 1, (-9000, -1000)), (1, 1, 1, 0, (10000, 20000)), (4, 1, 1, 1, (3000, 12000))]
    frames = [2, 1, 2, 1, 2, 1, 2]
    bank = Bank(rate, n, 2, chans, 2)

    def move(c, lo, hi):
        oks = [row[c].filter_move(lo, hi) for row in bank.o]
        assert len(set(oks)) == 1
        if oks[0]:
            d = bank.o[0][c].d
            w, phi = bank.h.channel_weights(c, d.flo, d.fhi)
            assert np.array_equal(w, np.array(d.wfir[:], np.float32)) and phi == np.float32(d.phi)
        return oks[0]

    def act(k):
        if k == 1:
            bank.configure(1, 3, 1, 1, 1)  # AM -> NFM on channel 1: fields only, its state carries on
        elif k == 2:
            bank.configure(2, 2, 0, 1, 1)  # RAW -> AM without the filter
        elif k == 3:
            assert move(0, 500, 500)       # up 500 Hz
            assert move(0, -250, 250)      # wider
            assert not move(3, -60000, 0)  # out of range: nothing happens
        elif k == 4:
            bank.weights(2, *ALLPASS)      # the all-pass impulse on one channel: car and phi carry on
        elif k == 5:
            bank.h.configure(3, 1, 1, 1)
            for row in bank.o:
                for o in row:
                    o.configure(3, 1, 1, 1)
        elif k == 6:
            w, phi = bank.h.weights(1000, 8000)
            for row in bank.o:
                for o in row:
                    ow, ophi = o.weights(1000, 8000)
            assert np.array_equal(w, ow) and phi == ophi
        bank.controls_match()

    run_calls(bank, signals(3, 2, sum(frames) * n, rate), frames, what="live", between=act)


@pytest.mark.parametrize("rate,n,frames", [
    (96000, 9600, [2, 1]),    # the reference's default frame: 5 tiles, k_demod_chan<5>
    (48000, 4800, [2, 1]),
    (44100, 256, [4, 4]),
    (96000, 12288, [1, 2]),   # 6 tiles: k_demod_chan_front, every channel through k_demod_chan_out
    (96000, 2051, [2, 2]),    # odd frame: the scalar carrier loads, a ragged last tile
    (96000, 16, [3, 5, 2]),   # frames shorter than the 21-sample history: frames 0 and 1 of a call both reach into it
    (48000, 7, [4, 3, 5]),    # frames 0, 1 and 2 of a call reach into the history
])
def test_other_frames_rates_and_dc_correction(rate, n, frames):
    bank = Bank(rate, n, 2, FIVE, max(frames))
    run_calls(bank, signals(n, 2, sum(frames) * n, rate), frames, ic=37, qc=-1200, what=(rate, n))


def test_float_input_batch_and_receive():
    rate, n = 96000, 2048
    chans = [(3, 1, 1, 1, (2000, 9000)), (2, 1, 1, 1, (-12000, -3000)), (1, 0, 1, 1, ALLPASS)]
    rng = np.random.default_rng(5)
    raws = signals(6, 2, 8 * n, rate)
    # batch_f32: JavaAudio's (float)s/32767f values in one call, arbitrary floats in the next
    bank = Bank(rate, n, 2, chans, 2)
    L = 2 * n
    for k in range(2):
        if k == 0:
            bufs = [O.convert_i16(r[:2 * L]) for r in raws]
        else:
            bufs = [(rng.standard_normal(2 * L) * 0.4).astype(np.float32) for _ in range(2)]
        d_in = J.DeviceBuffer.from_host(np.stack(bufs))
        d_out = J.DeviceBuffer(2 * 3 * 2 * L * 2)
        bank.h.batch_f32(d_in, 2 * L, L, d_out, 2 * L)
        bank.check(d_out.to_host(np.int16).reshape(2, 3, 2 * L), bufs, 2, ("f32", k))
    # receive_f32 on a 1-input, 3-channel handle: 3 frames a call, equal to the batch form and to the oracles
    rx = Bank(rate, n, 1, chans, 1)
    bt = J.DemodChannels(rate, n, 1, 3, n)
    for c, (mode, fir, dwn, agc, band) in enumerate(chans):
        bt.configure_channel(c, mode, fir, dwn, agc)
        bt.channel_weights(c, *band)
    for k in range(4):
        buf = O.convert_i16(raws[0][2 * k * n:2 * (k + 1) * n]) if k % 2 == 0 else (rng.standard_normal(2 * n) * 0.4).astype(np.float32)
        got = rx.h.receive(buf)
        assert got.shape == (3, 2 * n)
        d_in = J.DeviceBuffer.from_host(buf)
        d_out = J.DeviceBuffer(3 * 2 * n * 2)
        bt.batch_f32(d_in, 2 * n, n, d_out, 2 * n)
        assert np.array_equal(got, d_out.to_host(np.int16).reshape(3, 2 * n)), k
        rx.check(got[None], [buf], 1, ("receive", k))


@pytest.mark.parametrize("n", [2048, 12288])
def test_padded_input_rows_and_audio_strides(n):
    """an input stride above 2L, audio strides of 2L + 2 and 2L + 6 (the scalar store paths), every guard byte unchanged"""
    rate, nin, frames = 96000, 2, [1, 2]
    chans = FIVE[1:]
    for xin, xout, olead in ((6, 2, 2), (2, 6, 0)):
        bank = Bank(rate, n, nin, chans, max(frames))
        raws = signals(n + xin, nin, sum(frames) * n, rate)
        pos = 0
        for call, nf in enumerate(frames):
            L = nf * n
            chunk = [r[2 * pos:2 * (pos + L)] for r in raws]
            si = 2 * L + xin
            buf, _ = LY.build_input(chunk, si, lead=2, tail=2 * 17, unit=2, seed=call)
            d_in = J.DeviceBuffer.from_host(buf)
            out = Guarded(LY.Layout(nin * bank.K, 2 * L, 2 * L + xout, lead=olead, tail=2 * 9, itemsize=2, unit=2),
                          f"demod channel audio (+{xin}/+{xout}, lead {olead})")
            bank.h.batch_i16(d_in.ptr + 2 * 2, si, L, out.ptr, 2 * L + xout)
            got = out.rows(np.int16).reshape(nin, bank.K, 2 * L)
            bank.check(got, [O.convert_i16(x) for x in chunk], nf, (n, xin, xout, call))
            pos += L


def test_output_rows_past_2_to_31_elements():
    """256 inputs x 8 channels x 2^20 samples in one call: stream (i, c)'s audio row starts at (8 i + c) 2^21 int16 elements,
    past 2^31 elements from stream 1024 on.  Input i is class row i mod 97 (tests/big_offsets.py), so a row written or read
    2^k bytes off lands on different data.  Sampled streams against the oracle over all 512 frames; channel 7 has channel
    0's controls, so its rows equal channel 0's."""
    rate, n, L, nin, K = 96000, 2048, 1 << 20, 256, 8
    chans = [(3, 1, 1, 1, (2000, 9000)), (2, 1, 1, 1, (-12000, -3000)), (1, 1, 0, 1, (10000, 20000)), (4, 1, 1, 1, (3000, 30000)),
             (3, 0, 1, 1, ALLPASS), (0, 1, 1, 1, (2000, 9000)), (3, 1, 1, 0, (-20000, -2000)), (3, 1, 1, 1, (2000, 9000))]
    h = J.DemodChannels(rate, n, nin, K, L)
    for c, (mode, fir, dwn, agc, band) in enumerate(chans):
        h.configure_channel(c, mode, fir, dwn, agc)
        h.channel_weights(c, *band)
    base = fm_am_signal(np.random.default_rng(7), L, rate, fc=6500.0)
    cls = lambda i: np.roll(base, 2 * 997 * BO.twin(i))  # noqa: E731  (I/Q kept paired)
    d_in = J.DeviceBuffer(nin * 4 * L)
    for i in range(nin):
        row = cls(i)
        J.binding._check(lib_h2d(d_in.ptr + i * 4 * L, row), "h2d")
    d_out = J.DeviceBuffer(nin * K * 4 * L)
    h.batch_i16(d_in, 2 * L, L, d_out, 2 * L)
    J.binding.stream_sync()
    rows = BO.boundary_rows(nin * K, 4 * L, 2, extra=4)
    assert any(r * 2 * L >= 2 ** 31 for r in rows)
    for s in rows:
        i, c = divmod(s, K)
        got = d_out.to_host(np.int16, count=2 * L, offset_bytes=s * 4 * L)
        mode, fir, dwn, agc, band = chans[c]
        o = O.Demod(rate)
        o.configure(mode, fir, dwn, agc)
        o.weights(*band)
        buf = O.convert_i16(cls(i))
        for f in range(L // n):
            assert np.array_equal(got[2 * f * n:2 * (f + 1) * n], o.receive(buf[2 * f * n:2 * (f + 1) * n])), (s, f)
        mx, av = h.frame_stats(s)
        assert same(mx, o.max) and same(av, o.avg), s
        twin = d_out.to_host(np.int16, count=2 * L, offset_bytes=(i * K + (7 if c == 0 else 0)) * 4 * L)
        if c in (0, 7):
            assert np.array_equal(got, twin), s
    assert h.channel_state(0) == h.channel_state(7)


def lib_h2d(dst, arr):
    arr = np.ascontiguousarray(arr)
    return J.lib().jsdr_memcpy_h2d(C.c_void_p(dst), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes))


def test_refused_calls_change_nothing():
    rate, n, nin = 96000, 2048, 2
    bank = Bank(rate, n, nin, FIVE[1:4], 2)
    raws = signals(8, nin, 6 * n, rate)
    lib = J.lib()
    buf = J.DeviceBuffer(nin * bank.K * 2 * 8192 * 2)
    h = bank.h

    def checked(rc):
        J.binding._check(rc, "refused")

    refused = [
        lambda: h.configure_channel(3, 1),
        lambda: h.configure_channel(-1, 1),
        lambda: h.configure_channel(0, 5),
        lambda: h.configure_channel(1, -1),
        lambda: h.configure(7, 1, 1, 1),
        lambda: h.channel_weights(3, 1000, 2000),
        lambda: h.channel_weights(-1, 1000, 2000),
        lambda: h.channel_control(3),
        lambda: h.channel_state(5),
        lambda: checked(lib.jsdr_demod_channel_state(h.h, 0, None, None)),
        lambda: checked(lib.jsdr_demod_get_channel(h.h, 0, None, None, None, None, None, None)),
        lambda: checked(lib.jsdr_demod_channel_info(h.h, None, None)),
        lambda: h.batch_i16(buf, 2 * 3000, 3000, buf, 2 * 3000),          # not whole frames
        lambda: h.batch_i16(buf, 2 * 6144, 6144, buf, 2 * 6144),          # above max_batch
        lambda: h.batch_i16(buf, 2 * 2048 - 2, 2048, buf, 2 * 2048),      # input stride too small
        lambda: h.batch_i16(buf, 2 * 2048, 2048, buf, 2 * 2048 - 2),      # audio stride too small
        lambda: h.batch_f32(buf, 2 * 2048 - 2, 2048, buf, 2 * 2048),
        lambda: h.batch_i16(None, 2 * 2048, 2048, buf, 2 * 2048),         # null buffer
        lambda: h.receive(np.zeros(2 * n, np.float32)),                   # receive_f32 with ninputs > 1
    ]
    for round_ in range(2):
        before = [h.channel_control(c) for c in range(bank.K)]
        states = [h.channel_state(c) for c in range(bank.K)]
        for k, fn in enumerate(refused):
            with pytest.raises(J.JsdrError):
                fn()
            assert [h.channel_control(c) for c in range(bank.K)] == before, (round_, k)
            assert [h.channel_state(c) for c in range(bank.K)] == states, (round_, k)
        # the next calls equal the oracles, which saw none of it
        run_calls(bank, [r[2 * 3 * n * round_:] for r in raws], [1, 2], what=("after refusals", round_))
