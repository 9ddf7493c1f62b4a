"""The C oracle held against fixtures produced by an INDEPENDENT restatement of the Java text.

tests/golden/reference_fixtures.npz comes from tests/golden/java_restatement.py (pure Python, written from
FUNcubeBPSKDemod.java / FECDecoder.java, tables parsed from the reference's source as data; generated in the
build container by make_reference_fixtures.py).  The C oracle (oracle/*.c) must reproduce every bit, counter,
state double and decoded byte: two restatements written separately from the same text agreeing bit for bit is
what pins the oracle where the reference itself cannot run (no JVM).
"""
import hashlib
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fixture_cases import FEC_CASES, STREAMS, stream_input  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "reference_fixtures.npz"))


def test_sincos_tables_are_the_correctly_rounded_ones(fx):
    """oracle: cosl/sinl rounded once; fixture: exact rational Taylor series rounded once"""
    s, c = O.bpsk_sincos()
    assert np.array_equal(s, fx["sin_tab"]) and np.array_equal(c, fx["cos_tab"])


@pytest.mark.parametrize("name", list(STREAMS))
def test_oracle_demodulator_equals_python_restatement(fx, name):
    p = STREAMS[name]
    raw = stream_input(name)
    k = "s_" + name + "_"
    assert hashlib.sha256(raw.tobytes()).digest() == fx[k + "sha256"].tobytes(), "input generator changed"
    d = O.Bpsk(rate=p["rate"], blen=8192, size=4, tuning=p["tuning"], trace=2048)
    d.receive_i16(raw, p["ic"], p["qc"])
    c = d.counters()
    got = [c[n] for n in ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK")]
    assert got == [int(v) for v in fx[k + "counters"][:9]]
    assert np.array_equal(d.bits(), fx[k + "bits"])
    st = d.state()
    # doubles compared as bit patterns (avePeakPower / aveCentreBin are FFT-mode only)
    keep = [0, 1, 2, 3, 4, 5] + list(range(8, 18))
    assert st[keep].tobytes() == fx[k + "state"][keep].tobytes()
    assert np.array_equal(d.istate(), fx[k + "istate"])
    assert d.trace()[:2048].tobytes() == fx[k + "trace"].tobytes()
    assert np.array_equal(d.decoded(), fx[k + "decoded"])
    fr = d.fec_results()
    assert [r[0] for r in fr] == [int(v) for v in fx[k + "fec_rc"]]
    assert [r[1] for r in fr] == [int(v) for v in fx[k + "fec_bitidx"]]
    for r, want in zip(fr, fx[k + "fec_data"]):
        assert np.array_equal(r[2], want)


def test_oracle_encoder_equals_python_restatement(fx):
    assert np.array_equal(O.fec_encode(fx["f_payload"]), fx["f_symbols"])


@pytest.mark.parametrize("name", FEC_CASES)
def test_oracle_fecdecode_equals_python_restatement(fx, name):
    blk = fx["f_" + name + "_in"]
    out = np.full(256, 0xEE, np.uint8)
    rc = O.lib().jo_fec_decode(O.ptr(blk), O.ptr(out))
    assert rc == int(fx["f_" + name + "_rc"][0])
    assert np.array_equal(out, fx["f_" + name + "_out"])  # untouched (0xEE) when RS fails


def test_fixture_corpus_covers_the_interesting_outcomes(fx):
    rcs = {n: int(fx["f_" + n + "_rc"][0]) for n in FEC_CASES}
    assert rcs["clean"] == 0 and rcs["flips200"] == 200 and rcs["burst400"] == 400 and rcs["soft"] > 0
    assert rcs["flips700"] == -1 and rcs["garbage"] == -1
    # RS stage exercised with known error counts: 8+8 and 16+16 (the limit) byte errors decode, 17 in one word does not
    assert rcs["rs8"] > 0 and rcs["rs16"] > 0 and rcs["rs16_0"] > 0 and rcs["rs17"] == -1
    assert int(fx["s_clean_fec_rc"][0]) >= 0 and int(fx["s_noisy_fec_rc"][0]) > 100 and int(fx["s_fail_fec_rc"][0]) == -1


def test_fft_acquire_at_2048_sample_frames_never_finds_sync():
    """DESIGN.md section 3 claims that the reference's FFT-acquire mode (doBufferFFT, :406-464) cannot synchronise
    at BASELINE's 2048-sample frames (blen = 8192): 204 bins of 46.9 Hz moved to bin 0 are not the 2 kHz signal
    band the 10 Hz-bin design assumes.  Shown here instead of asserted in prose: a CLEAN synthetic stream that the
    tune mode decodes (and that the same mode decodes at the default 9600-sample frame) yields no sync hit."""
    iq, _, _ = O.make_dbpsk_stream(20020109, 5, 458752, noise_sigma=300.0)
    d = O.Bpsk(rate=96000, blen=8192, size=4, tuning=12000, do_fft=1)
    d.receive_i16(iq)
    c = d.counters()
    assert c["cntRaw"] == 458752 and c["cntFEC"] == 0 and c["cntDec"] == 0
    t = O.Bpsk(rate=96000, blen=8192, size=4, tuning=12000, do_fft=0)
    t.receive_i16(iq)
    assert t.counters()["cntDec"] == 1
    n = (458752 // 9600) * 9600
    f = O.Bpsk(rate=96000, blen=38400, size=4, tuning=12000, do_fft=1)
    f.receive_i16(iq[:2 * n])
    assert f.counters()["cntDec"] == 1


# ------------------------------------------------------------------ FFT-acquire mode (bpsk-dofft), :399-464
from fixture_cases import FFT_STREAMS, fft_stream_input  # noqa: E402


@pytest.fixture(scope="module")
def fxf():
    return np.load(os.path.join(HERE, "golden", "fftmode_fixtures.npz"))


@pytest.mark.parametrize("name", list(FFT_STREAMS))
def test_oracle_fft_acquire_equals_python_restatement(fxf, name):
    """doBufferFFT restated from the Java text (java_restatement.DemodFFT) around the transform this project defines in
    JTransforms' place: the C oracle must give the same centre bin after every frame, the same bits, counters and state
    doubles (avePeakPower and aveCentreBin included), bit for bit"""
    p = FFT_STREAMS[name]
    raw = fft_stream_input(name)
    k = "x_" + name + "_"
    assert hashlib.sha256(raw.tobytes()).digest() == fxf[k + "sha256"].tobytes(), "input generator changed"
    n = p["frame"]
    d = O.Bpsk(rate=p["rate"], blen=4 * n, size=4, tuning=12000, do_fft=1, do_up=p["do_up"], trace=1024)
    centre = []
    for f in range(p["n"] // n):
        d.receive_i16(raw[2 * n * f:2 * n * (f + 1)], 0, 0)
        centre.append(d.counters()["centreBin"])
    assert centre == [int(v) for v in fxf[k + "centre"]]
    c = d.counters()
    got = [c[m] for m in ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK")]
    assert got == [int(v) for v in fxf[k + "counters"][:9]]
    assert np.array_equal(d.bits(), fxf[k + "bits"])
    st = d.state()
    keep = [1, 2, 3, 4, 5, 6, 7] + list(range(8, 18))  # (tuPhase is not advanced in this mode)
    assert st[keep].tobytes() == fxf[k + "state"][keep].tobytes()
    assert np.array_equal(d.istate(), fxf[k + "istate"])
    assert d.trace()[:1024].tobytes() == fxf[k + "trace"].tobytes()


def test_fft_twiddle_table_is_cos_sin_to_the_last_bit_or_one(fxf):
    """the table of the defined transform (cosl / sinl of the long-double angle, rounded once; exact on the axes) against
    the correctly rounded cos / sin of the exact angle 2 pi k / n: equal, or one unit in the last place apart"""
    from fractions import Fraction

    from exact_trig import _sincos_exact

    pi = Fraction(314159265358979323846264338327950288419716939937510582097494459230781640628620899, 10 ** 80)
    for n in (1024, 2048, 4096):
        w = O.fft_twiddles_f64(n)
        assert np.array_equal(w, fxf[f"twiddles_{n}"])
        off = 0
        for kk in range(0, n // 2, 7):  # a seventh of the table keeps the exact arithmetic short
            ang = 2 * pi * kk / n
            s, c = _sincos_exact(ang)
            for got, want in ((w[2 * kk], c), (w[2 * kk + 1], -s)):
                if got != want:
                    off += 1
                    assert abs(got - want) <= np.spacing(abs(want)), (n, kk, got, want)
        assert off <= 4, (n, off)
