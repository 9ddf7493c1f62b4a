"""GPU: NaN, +Inf and 3e38 through the float entry points of the PSD (fft.java:190-228), the AM/FM chain (demod.java:341-483) and
phase.java's max |x|, in the style of test_gpu_bpsk_nonfinite.py (comparison rule and poisons: nonfinite.py).

PSD: a NaN anywhere in a frame makes every bin NaN whatever the transform's order, `m < psd[i]` (:214) is then never true, so the
frame's slots n / n+1 are the p = -1 branch of :214-216 and -FLT_MAX; the frames beside it are untouched.  In the spectrum every
bin of that frame is NaN in its real or its imaginary part.  For a +Inf frame only
what the reference's text fixes is checked (which bins are Inf and which NaN depends on the transform's order).
demod: audio bit-exact against O.Demod; what FOLLOWS the poisoned frame is the point -- filter history, FM detector, NCO.
phase: `max < a` passes over a NaN (phase.java:123-128)."""
import numpy as np
import pytest

import java_sdr_amd as J
import nonfinite as NF
import oracle_lib as O

pytestmark = pytest.mark.gpu


def psd_batch(f, frames):
    n = f.n
    d_in = J.DeviceBuffer.from_host(np.ascontiguousarray(frames, np.float32))
    d_out = J.DeviceBuffer(4 * frames.shape[0] * (n + 2))
    f.batch_f32(d_in, frames.shape[0], d_out)
    return d_out.to_host(np.float32).reshape(frames.shape[0], n + 2)


# one size for each kernel family: 2^k, the mixed-radix 9600 and 19200, 4410, and the any-size plan (101 is prime)
@pytest.mark.parametrize("n,rate", [(2048, 96000), (9600, 96000), (19200, 192000), (4410, 44100), (101, 96000)])
def test_psd_of_a_batch_with_a_nan_frame_and_an_inf_frame(n, rate):
    rng = np.random.default_rng(n)
    clean = (rng.standard_normal((5, 2 * n)) * 0.3).astype(np.float32)
    f = J.Fft(n, rate)
    want = psd_batch(f, clean)
    assert np.isfinite(want).all()
    want_spec = f.spectrum(clean)
    for where in (0, 2 * (n // 2) + 1, 2 * n - 1):  # the first float, a Q in the middle, the last float
        x = clean.copy()
        x[2, where] = NF.NAN
        got = psd_batch(f, x)
        for k in (0, 1, 3, 4):
            assert got[k].tobytes() == want[k].tobytes(), (n, where, k)
        one = f.receive(x[2])
        for g, what in ((got[2], "batch"), (one, "receive")):
            NF.check_psd_nan_frame(g, n, rate, (n, where, what))
        # (every BIN is NaN -- its real or its imaginary part, so that |X|^2 is; which of the two depends on the twiddles a transform
        #  treats as 1 or i: sample 0 is never multiplied at all, and a NaN on its I leaves every imaginary part finite, in the
        #  oracle's transform as here)
        spec = f.spectrum(x).reshape(5, n, 2)
        assert np.isnan(spec[2]).any(axis=1).all(), (n, where, int(np.isnan(spec[2]).any(axis=1).sum()))
        spec = spec.reshape(5, 2 * n)
        for k in (0, 1, 3, 4):
            assert spec[k].tobytes() == want_spec[k].tobytes(), (n, where, k)
    x = clean.copy()
    x[2, 2 * (n // 3)] = NF.PINF
    got = psd_batch(f, x)
    for k in (0, 1, 3, 4):
        assert got[k].tobytes() == want[k].tobytes(), (n, "inf", k)
    for g, what in ((got[2], "batch"), (f.receive(x[2]), "receive")):
        NF.check_psd_inf_frame(g, n, rate, (n, what))


# ---------------------------------------------------------------------------------------------------------------- demod
def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def demod_inputs(S, N, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(N)
    xs = []
    for s in range(S):
        msg = np.sin(2 * np.pi * (440.0 + 31.0 * s) * t / rate)
        ph = 2 * np.pi * (5000.0 + 900.0 * s) * t / rate + np.cumsum(msg) * (2 * np.pi * 2500.0 / rate)
        amp = 0.35 * (1.0 + 0.6 * np.sin(2 * np.pi * 300.0 * t / rate))
        x = np.empty(2 * N)
        x[0::2], x[1::2] = amp * np.cos(ph), amp * np.sin(ph)
        xs.append((x + rng.standard_normal(2 * N) * 0.01).astype(np.float32))
    return xs


def demod_poison(x, n):
    """frame 1 holds a NaN, a +Inf and a 3e38"""
    return NF.poison(x, [(n + 7, NF.I, NF.NAN), (n + n // 2, NF.Q, NF.PINF), (2 * n - 3, NF.I, NF.HUGE)])


# 10240 = 5 tiles of 2048: the largest frame the fused kernel takes; 10241: the three-kernel path (AM takes it at every size)
@pytest.mark.parametrize("n", [10240, 10241])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_demod_batch_f32_after_a_poisoned_frame(mode, n):
    rate, S = 96000, 3
    xs = demod_inputs(S, 4 * n, rate, 100 * mode + n)
    xs[1] = demod_poison(xs[1], n)
    for dofir, dodwn, doagc in ((1, 1, 1), (1, 1, 0)):
        d = J.Demod(rate=rate, n=n, nstreams=S, max_batch_samples=2 * n)
        d.configure(mode, dofir, dodwn, doagc)
        d.weights(3000, 11000)
        os_ = [O.Demod(rate) for _ in range(S)]
        for o in os_:
            o.configure(mode, dofir, dodwn, doagc)
            o.weights(3000, 11000)
        for call in range(2):  # two frames a call: the first call ends in the poisoned frame
            L = 2 * n
            chunk = np.stack([x[2 * call * L:2 * (call + 1) * L] for x in xs])
            d_in, d_out = J.DeviceBuffer.from_host(chunk), J.DeviceBuffer(chunk.shape[0] * 2 * L * 2)
            d.batch_f32(d_in, 2 * L, L, d_out, 2 * L)
            got = d_out.to_host(np.int16).reshape(S, 2 * L)
            for s in range(S):
                for fr in range(2):
                    want = os_[s].receive(chunk[s, 2 * fr * n:2 * (fr + 1) * n])
                    assert np.array_equal(got[s, 2 * fr * n:2 * (fr + 1) * n], want), (mode, dofir, dodwn, doagc, n, s, 2 * call + fr)
                mx, av = d.frame_stats(s)
                assert same(mx, os_[s].max) and same(av, os_[s].avg), (mode, doagc, n, s, call, mx, os_[s].max, av, os_[s].avg)
            if dodwn:  # (one NCO a handle, advanced by the sample count alone: the poisoned stream's oracle holds it too)
                assert same(d.state()[0], os_[0].car) and same(d.state()[0], os_[1].car)


@pytest.mark.parametrize("n", [10240, 10241])
@pytest.mark.parametrize("switches", [(1, 1, 1), (1, 1, 0)])
def test_demod_channel_handle_after_a_poisoned_frame(switches, n):
    """two inputs x five channels, one per mode; input 1's frame 1 is poisoned"""
    rate = 96000
    xs = demod_inputs(2, 4 * n, rate, 7 + n)
    xs[1] = demod_poison(xs[1], n)
    bands = [(3000, 11000), (-9000, -1000), (2000, 9000), (10000, 20000), (3000, 12000)]
    h = J.DemodChannels(rate, n, 2, 5, 2 * n)
    os_ = [[O.Demod(rate) for _ in range(5)] for _ in range(2)]
    for c in range(5):
        h.configure_channel(c, c, *switches)
        h.channel_weights(c, *bands[c])
        for i in range(2):
            os_[i][c].configure(c, *switches)
            os_[i][c].weights(*bands[c])
    for call in range(2):
        L = 2 * n
        chunk = np.stack([x[2 * call * L:2 * (call + 1) * L] for x in xs])
        d_in, d_out = J.DeviceBuffer.from_host(chunk), J.DeviceBuffer(2 * 5 * 2 * L * 2)
        h.batch_f32(d_in, 2 * L, L, d_out, 2 * L)
        got = d_out.to_host(np.int16).reshape(2, 5, 2 * L)
        for i in range(2):
            for c in range(5):
                o = os_[i][c]
                for fr in range(2):
                    want = o.receive(chunk[i, 2 * fr * n:2 * (fr + 1) * n])
                    assert np.array_equal(got[i, c, 2 * fr * n:2 * (fr + 1) * n], want), (switches, n, i, c, 2 * call + fr)
                mx, av = h.frame_stats(h.stream(i, c))
                assert same(mx, o.max) and same(av, o.avg), (switches, n, i, c, call)
        for c in range(5):  # (one NCO a channel, advanced by the sample count alone: the poisoned input's oracle holds it too)
            if switches[1]:
                assert same(h.channel_state(c)[0], os_[1][c].car), (switches, n, c, call)


# ---------------------------------------------------------------------------------------------------------------- phase
@pytest.mark.parametrize("n", [2048, 1002])  # (frames are whole pairs of samples)
def test_phase_maxabs_passes_over_nan_and_takes_inf(n):
    rng = np.random.default_rng(n)
    base = (rng.standard_normal(2 * n) * 0.3).astype(np.float32)
    rows = [base]
    for at in (0, n + 1, 2 * n - 1):
        x = base.copy()
        x[at] = NF.NAN
        rows.append(x)
    big = int(np.argmax(np.abs(base)))
    x = base.copy()
    x[big] = NF.NAN  # the largest sample itself: the runner-up is the answer
    rows.append(x)
    for v in (NF.PINF, NF.NINF):
        x = base.copy()
        x[n // 3], x[n // 3 + 1] = v, NF.NAN
        rows.append(x)
    rows.append(np.full(2 * n, NF.NAN, np.float32))  # nothing is ever above -1
    rows = np.stack(rows)
    got = J.phase_maxabs(rows, n)
    want = np.array([O.phase_maxabs(r) for r in rows], np.float32)
    assert want[-1] == -1.0 and want[5] == np.inf and want[6] == np.inf and want[4] < want[0] == want[1] == want[2] == want[3]
    NF.assert_same(got, want, n)
