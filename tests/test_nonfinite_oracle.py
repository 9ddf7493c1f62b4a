"""CPU: what the reference does with NaN, +-Inf and huge floats, pinned before any kernel is asked.

1. The C oracle against the pure-Python restatement of the Java text (tests/golden/java_restatement.py: Demod and DemodFFT) on
   30 frames of 2048 with a NaN on I, a +Inf on I and a +Inf on Q: bits, counters, the integer state and the (fi, fq) trace equal,
   the state doubles equal by nonfinite.same_f64.  Two independent statements of :357-595 agree on the non-finite cases, the peak
   search's `dmEnergy[n] > eMax` from eMax = -1.0e10F (:586-592) among them.
2. The inputs of the GPU tests (nonfinite.py) meet, in the oracle alone, the conditions that make those tests bite: the peak
   position the NaN freezes is not 0 (a search that starts from a NaN slot 0 answers 0), bits go on being sliced after the poison,
   the NaN-at-6149 stream still decodes a FEC frame, the Inf-at-204877 stream ends with +Inf and NaN energy slots side by side.
   A generator change that breaks one of these calls for another position, not for a weaker condition."""
import os
import sys

import numpy as np
import pytest

import nonfinite as NF
import oracle_lib as O

N, FRAMES = 2048, 30
POISONS = {"nan_i": [(NF.NAN_HI, NF.I, NF.NAN)], "inf_i": [(20011, NF.I, NF.PINF)], "inf_q": [(20012, NF.Q, NF.PINF)]}


def restatement():
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    ref = os.environ.get("JSDR_REFERENCE", "/root/reference")  # (where java_restatement looks for the reference's text)
    if not all(os.path.isfile(os.path.join(ref, f)) for f in ("FECDecoder.java", "FUNcubeBPSKDemod.java")):
        pytest.skip("java_restatement parses its tables out of the reference's text, which is not present here")
    import java_restatement as R
    return R


@pytest.mark.parametrize("do_fft", [0, 1])
@pytest.mark.parametrize("name", list(POISONS))
def test_the_restatement_and_the_oracle_agree_on_non_finite_input(name, do_fft):
    R = restatement()
    x = NF.poison(NF.base_stream(NF.STREAM, 0.93, nsamp=N * FRAMES), POISONS[name])
    cap = N * FRAMES // 10 + 8
    o = O.Bpsk(blen=4 * N, do_fft=do_fft, trace=cap)
    r = R.DemodFFT(N, [float(v) for v in O.fft_twiddles_f64(N)], trace_cap=cap) if do_fft else R.Demod(trace_cap=cap)
    xl = x.astype(np.float64).tolist()  # (double)buf[n]: the float's value
    for k in range(FRAMES):
        o.receive(x[2 * N * k:2 * N * (k + 1)])
        r.receive(xl[2 * N * k:2 * N * (k + 1)])
    assert np.array_equal(o.bits(), np.array(r.bits, np.int8)), name
    assert list(o.istate()) == r.istate(), (name, o.istate(), r.istate())
    oc = o.counters()
    assert [oc[k] for k in NF.CKEYS[:9]] == r.counters()[:9], (name, oc, r.counters())
    st = r.state()
    if do_fft:
        st[6], st[7] = r.avePeakPower, r.aveCentreBin
        assert oc["centreBin"] == r.centre_log[-1], name
    NF.assert_same(o.state(), np.array(st, np.float64), (name, do_fft, "state"))
    NF.assert_same(o.trace().reshape(-1, 2), np.array(r.trace, np.float64).reshape(-1, 2), (name, do_fft, "(fi,fq)"))
    # the case is a non-finite one to its end, and it went on slicing bits
    assert not np.isfinite(o.state()[8:16]).any(), (name, o.state()[8:16])
    assert oc["cntBit"] > 600, oc


def test_same_f64_and_same_f32_are_the_stated_rule():
    qnan, neg_nan = np.float64(np.nan), np.frombuffer(np.uint64(0xFFF8000000000001).tobytes(), np.float64)[0]
    a = np.array([0.0, 1.5, qnan, np.inf, qnan, 1.0])
    b = np.array([-0.0, 1.5, neg_nan, np.inf, 1.0, qnan])
    assert list(NF.same_f64(a, b)) == [False, True, True, True, False, False]  # (-0.0 is another bit pattern than 0.0)
    assert list(NF.same_f32(a.astype(np.float32), b.astype(np.float32))) == [False, True, True, True, False, False]
    with pytest.raises(AssertionError):
        NF.assert_same(a, b, "x")
    NF.assert_same(a[1:4], b[1:4], "x")
    x = NF.poison(np.zeros(8, np.float32), [(1, NF.I, NF.NAN), (2, NF.Q, NF.NINF), (3, NF.I, NF.NZERO), (3, NF.Q, NF.SUBN)])
    assert np.isnan(x[2]) and x[5] == -np.inf and np.signbit(x[6]) and 0 < x[7] < np.finfo(np.float32).tiny and not x[[0, 1, 3, 4]].any()


def bits_after(x, first, **kw):
    """cntBit 2000 samples after the poison (its windows have passed) and at the end"""
    n = x.size // 2
    frame = kw.get("frame")
    cut = first + 2000 if frame is None else -(-(first + 2000) // frame) * frame
    assert cut < n
    mid = NF.run_oracle(x[:2 * cut], **kw).counters()["cntBit"]
    return mid, cut


def check_goes_on(o, x, first, where, **kw):
    rate = kw.get("rate", 96000)
    mid, cut = bits_after(x, first, **kw)
    left = (x.size // 2 - cut) // (rate // 9600) // 8  # bit periods still to come
    grown = o.counters()["cntBit"] - mid
    assert left >= 50 and grown >= 0.9 * left, (where, mid, o.counters()["cntBit"], left)


@pytest.mark.parametrize("cases", [NF.TUNE_CASES, NF.PHASE_CASES], ids=["batch", "phases"])
def test_tune_mode_inputs_meet_their_conditions(cases):
    xs = NF.tune_inputs(cases)
    assert len(NF.TUNE_CASES) == 12 and sum(not spec for _, _, _, spec in NF.TUNE_CASES) >= 3
    assert sorted((NF.INF_Q_FIRST + k) % 8 for k in range(8)) == list(range(8))  # each phase of the 8-cycle once
    assert NF.TUNE_CALLS[1] < 26 and sum(NF.TUNE_CALLS) == NF.NSAMP and min(NF.TUNE_CALLS) > 0
    for (name, _, _, spec), x in zip(cases, xs):
        o = NF.run_oracle(x)
        en = o.state()[8:16]
        if not spec or np.isfinite(x).all():
            assert np.isfinite(en).all(), name
            if spec and name == "huge_pair":
                assert en.max() > 1e60 and np.isfinite(o.trace()).all(), (name, en)  # huge, and finite in double all the way
            continue
        assert np.isnan(en).any(), (name, en)
        assert o.istate()[5] != 0 and o.istate()[4] == o.istate()[5], (name, o.istate())
        check_goes_on(o, x, NF.first_poison(spec), name)
        if name == "nan_i_hi":
            assert np.isnan(en).all() and np.isnan(o.state()[3]), en
            fec = o.fec_results()
            assert len(fec) == 1 and fec[0][0] >= 0, [f[:2] for f in fec]  # a whole FEC frame decoded at the frozen peak
        if name == "inf_i_mid":
            assert (en == np.inf).any() and np.isnan(en).any(), en
            assert en[o.istate()[5]] == np.inf, (en, o.istate())  # the search passed over the NaN slots
        if name == "nan_call_end":
            p = NF.first_poison(spec)
            assert NF.TUNE_CALLS[0] - 26 <= p < NF.TUNE_CALLS[0], p
        if name == "nan_call_first":
            assert NF.first_poison(spec) == sum(NF.TUNE_CALLS[:3])


def test_odd_rate_inputs_meet_their_conditions():
    for (name, spec), x in zip(NF.ODD_CASES, NF.odd_inputs()):
        o = NF.run_oracle(x, rate=NF.ODD_RATE, tuning=NF.ODD_TUNING)
        if not spec:
            assert np.isfinite(o.state()).all()
            continue
        assert np.isnan(o.state()[8:16]).all(), name
        check_goes_on(o, x, NF.first_poison(spec), name, rate=NF.ODD_RATE, tuning=NF.ODD_TUNING)
    # (the peak the NaN freezes may be 0 here: the case is about the generic front end, the argmax has its cases above)


@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("n,rate", NF.FFT_SIZES)
def test_fft_acquire_inputs_meet_their_conditions(n, rate, do_up):
    xs = NF.fft_inputs(n, rate, do_up)
    kw = dict(rate=rate, frame=n, do_fft=1, do_up=do_up)
    o = [NF.run_oracle(x, **kw) for x in xs]
    # the NaN: the peak frozen away from 0, avePeakPower NaN for ever and the centre bin frozen with it, bits go on
    assert o[0].istate()[5] != 0 and np.isnan(o[0].state()[8:16]).all(), (o[0].istate(), o[0].state()[8:16])
    check_goes_on(o[0], xs[0], NF.FFT_POISON_FRAME * n, (n, do_up), **kw)
    if n >= 604:  # (below, the searched band is empty: centreBin is the clamp value and avePeakPower stays 0)
        assert np.isnan(o[0].state()[6])
        before = NF.run_oracle(xs[0], upto=(NF.FFT_POISON_FRAME + 1) * n, **kw).counters()["centreBin"]
        assert o[0].counters()["centreBin"] == before > 102
    # +-3e38: finite in double all the way
    assert np.isfinite(o[1].state()).all() and np.isfinite(o[1].trace()).all() and o[1].state()[8:16].max() > 1e60
    assert np.isfinite(o[2].state()).all()


# (a 2^k frame and one through the oracle's exact DFT, which is O(n^2))
@pytest.mark.parametrize("n,rate", [(2048, 96000), (101, 96000)])
def test_the_psd_rule_on_a_nan_frame_and_an_inf_frame(n, rate):
    """what test_gpu_psd_demod_phase_nonfinite.py expects of the kernels, on the oracle: fft.java:205-218 with NaN and +Inf bins"""
    x = (np.random.default_rng(n).standard_normal(2 * n) * 0.3).astype(np.float32)
    c = O.fft_receive(x, rate)
    pk = int(np.argmax(c[:n]))
    assert c[n] == NF.hz_rule(2 * pk, n, rate) and c[n + 1] == c[pk]  # (the rule as restated in nonfinite.py, on a finite frame)
    for where in (0, 2 * (n // 2) + 1, 2 * n - 1):
        NF.check_psd_nan_frame(O.fft_receive(NF.poison(x, [(where // 2, where % 2, NF.NAN)]), rate), n, rate, (n, where))
    NF.check_psd_inf_frame(O.fft_receive(NF.poison(x, [(n // 3, NF.I, NF.PINF)]), rate), n, rate, n)
