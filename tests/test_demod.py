"""CPU: the oracle's demod.java chain (demod.java:341-483) against an independent numpy float32 restatement, plus
its corner semantics (filterMove's range check, AGC on silence, NaN handling of Math.max)."""
import numpy as np

import oracle_lib as O

from demod_numpy import NumpyDemod, f32


def test_demod_oracle_matches_numpy_restatement():
    rng = np.random.default_rng(4)
    n = 256
    for mode in (0, 1, 2, 3, 4):
        for dofir, dodwn, doagc in ((0, 0, 0), (1, 0, 1), (1, 1, 1), (0, 1, 0)):
            o = O.Demod(96000)
            p = NumpyDemod(96000)
            o.configure(mode, dofir, dodwn, doagc)
            p.mode, p.dofir, p.dodwn, p.doagc = mode, dofir, dodwn, doagc
            w, phi = o.weights(3000, 9000)
            p.weights(3000, 9000)
            assert np.array_equal(w, p.wfir) and phi == p.phi
            for k in range(3):
                t = np.arange(k * n, (k + 1) * n)
                buf = np.empty(2 * n, f32)
                buf[0::2] = (0.4 * np.cos(2 * np.pi * 6000 * t / 96000 + 2.0 * np.sin(2 * np.pi * 400 * t / 96000))).astype(f32)
                buf[1::2] = (0.4 * np.sin(2 * np.pi * 6000 * t / 96000 + 2.0 * np.sin(2 * np.pi * 400 * t / 96000))).astype(f32)
                buf += (rng.standard_normal(2 * n) * 0.01).astype(f32)
                got = o.receive(buf)
                want, mx, avg = p.receive(buf)
                assert np.array_equal(got, want), (mode, dofir, dodwn, doagc, k)
                assert (o.max == mx or (np.isnan(o.max) and np.isnan(mx))) and o.avg == avg
                assert o.car == p.car


def test_demod_filter_move_range_check_and_defaults():
    o = O.Demod(96000)
    # demod.java:300-312 with the default filter points (Integer.MIN_VALUE / MAX_VALUE, :85-86): the range check
    # fails, weights() never runs and the weights stay all zero -- with the filter enabled the output is silence
    assert not o.filter_move(0, 0)
    o.configure(1, 1, 0, 0)
    buf = np.full(64, 0.5, f32)
    assert np.all(o.receive(buf) == 0)
    o2 = O.Demod(96000)
    o2.d.flo, o2.d.fhi = 1000, 5000
    assert o2.filter_move(500, 500) and (o2.d.flo, o2.d.fhi) == (1500, 5500)
    assert not o2.filter_move(0, 60000) and (o2.d.flo, o2.d.fhi) == (1500, 5500)  # hi >= rate/2
    assert not o2.filter_move(5000, 0)  # lo >= hi


def test_demod_agc_on_silence_and_nan():
    o = O.Demod(48000)
    o.configure(1, 0, 0, 1)  # RAW + AGC
    out = o.receive(np.zeros(32, f32))
    assert np.all(out == 0)  # 0 * (1/0 = inf) = NaN -> (short)NaN = 0
    buf = np.zeros(32, f32)
    buf[6] = np.nan
    buf[8] = 0.25
    out = o.receive(buf)
    assert np.isnan(o.max) and np.all(out == 0)  # Math.max propagates NaN; x * (1/NaN) = NaN -> 0
    o.configure(1, 0, 0, 0)
    out = o.receive(np.array([2.0, 0, -2.0, 0, 0.5, 0, 70000.0, 0], f32))
    # (short)(int)(2.0*32767) = 65534 -> -2 ; -65534 -> 2 ; 0.5 -> 16383 ; 70000*32767 saturates to INT_MAX -> (short) = -1
    assert list(out[0::2]) == [-2, 2, 16383, -1]
