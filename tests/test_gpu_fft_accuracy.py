"""GPU: the float spectrum kernels at float32 round-off (tests/fft_accuracy.py has the cases, the expectations and the bars).

tests/test_gpu_fft.py holds the contract, 1e-5 of the frame's peak; these are the regression guard inside it, 8 to 20 times
tighter: every family and every instantiation the product runs (IN_F32 / OUT_SPEC, IN_F32 / OUT_PSD, IN_I16 / OUT_PSD with the
2^15-scaled plan), one launch shape a frame (receive) and batches, against the exact DFT and four times a float32 CPU FFT's
own error; every twiddle on its own through impulses; the dB rule alone over 109 binades of level.  Any change to twiddles,
accumulation width or psd_db has to keep them green.  Each test prints its figures (pytest -s) before it asserts: DESIGN.md's
table of measured ratios is made of them."""
import math

import numpy as np
import pytest

import fft_accuracy as A
import java_sdr_amd as J

pytestmark = pytest.mark.gpu

EPS = A.EPS


def make(n):
    f = J.Fft(n, 10 * n)
    assert f.kernel_name() == A.kernel_for(n), (n, f.kernel_name())  # the family named is the family that ran
    return f


def batch_f32(f, bufs):
    bufs = np.ascontiguousarray(bufs, np.float32).reshape(-1, 2 * f.n)
    d_in, d_out = J.DeviceBuffer.from_host(bufs), J.DeviceBuffer(4 * bufs.shape[0] * (f.n + 2))
    f.batch_f32(d_in, bufs.shape[0], d_out)
    return d_out.to_host(np.float32).reshape(bufs.shape[0], f.n + 2)


def report(part, n, **figs):
    print("FFTACC %s n=%d %s " % (part, n, A.kernel_for(n)) + " ".join("%s=%.3f" % kv for kv in figs.items()))


@pytest.mark.parametrize("n", A.SIZES)
def test_spectrum_within_four_times_a_float32_fft(n):
    """A, spectrum form: E2 and Emax of every frame within four times the yardstick's worst frame of the size; the noise frame's
    Emax within four times the yardstick's on that frame"""
    f = make(n)
    x, want = A.frames(n), A.want(n)
    got = A.as_complex(f.spectrum(x))
    bar2, barm = A.bars(n)
    m = [A.measures(got[k], want[k], x[k]) for k in range(5)]
    ym = A.yardstick_measures(n)
    report("A-spec", n, E2_eps=max(e for e, _ in m) / EPS, E2_ratio=max(e for e, _ in m) / max(e for e, _ in ym),
           Emax_eps=max(e for _, e in m) / EPS, Emax_ratio=max(e for _, e in m) / max(e for _, e in ym),
           noise_Emax_eps=m[A.NOISE][1] / EPS, noise_Emax_ratio=m[A.NOISE][1] / ym[A.NOISE][1])
    for k in range(5):
        assert m[k][0] <= bar2, (n, A.FRAME_NAMES[k], m[k][0] / EPS, bar2 / EPS)
        assert m[k][1] <= barm, (n, A.FRAME_NAMES[k], m[k][1] / EPS, barm / EPS)
    assert m[A.NOISE][1] <= A.noise_emax_bar(n), (n, m[A.NOISE][1] / EPS, A.noise_emax_bar(n) / EPS)


@pytest.mark.parametrize("n", A.SIZES)
def test_psd_forms_within_the_spectrum_bar(n):
    """A, PSD forms: lin(dB) of every bin of receive and batch_f32 (every frame), batch_i16 and receive_raw (the square wave)
    against |want_k| 2/n, within the spectrum's Emax bar carried through the modulus plus the dB value's own rounding"""
    f = make(n)
    x, want = A.frames(n), A.want(n)
    _, barm = A.bars(n)
    rows = {"batch_f32": batch_f32(f, x), "receive": np.stack([f.receive(x[k]) for k in range(5)])}
    raw = A.square_i16(n)
    i16 = {"batch_i16": f.batch_host_i16(raw)[0], "receive_raw": f.receive_raw(raw)}
    worst = 0.0
    for name, psd in rows.items():
        assert psd.shape == (5, n + 2)
        for k in range(5):
            err = np.abs(A.lin(psd[k, :n]) - A.psd_target(n, want[k]))
            bound = A.psd_bound(n, want[k], x[k], barm)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (n, name, A.FRAME_NAMES[k], float((err / bound).max()))
    # the int16 entry points see the same samples as the float ones saw converted: one frame at a time and batched
    worst16 = 0.0
    for name, psd in i16.items():
        err = np.abs(A.lin(psd[:n]) - A.psd_target(n, want[A.SQUARE]))
        bound = A.psd_bound(n, want[A.SQUARE], x[A.SQUARE], barm)
        worst16 = max(worst16, float((err / bound).max()))
        assert np.all(err <= bound), (n, name, float((err / bound).max()))
    report("A-psd", n, f32_of_bound=worst, i16_of_bound=worst16)


@pytest.mark.parametrize("n", A.K_ANY + A.K_RT)
def test_dft_any_is_the_correctly_rounded_exact_dft(n):
    """fft_any.hip's header: the correctly rounded float of the exact DFT.  Every real and imaginary component within half a
    float32 ulp of the exact value plus the a-priori double round-off, (n + 256) 2^-52 |x|_1.  k_fft_rt's sizes run along for
    the figure alone: how close float passes with double-summed prime radices come to that bar."""
    f = make(n)
    x, want = A.frames(n), A.want(n)
    got = A.as_complex(f.spectrum(x))
    worst, of_noise = 0.0, 0.0
    for k in range(5):
        br, bi = A.correctly_rounded_bound(n, want[k], x[k])
        r = max(float((np.abs(got[k].real - want[k].real) / br).max()), float((np.abs(got[k].imag - want[k].imag) / bi).max()))
        worst = max(worst, r)
        of_noise = r if k == A.NOISE else of_noise
        if A.kernel_for(n) == "k_dft_any":
            assert r <= 1.0, (n, A.FRAME_NAMES[k], r)
    # (of_bound: over all frames, the bins that are exactly zero included, where the bound is the double round-off alone;
    #  noise_of_bound: the flat spectrum, where the bound is half a float32 ulp of every component)
    report("A-rounded", n, of_bound=worst, noise_of_bound=of_noise)


@pytest.mark.parametrize("n", A.SIZES)
def test_impulses_every_bin_within_four_times_a_float32_fft(n):
    """B: the impulse at t0 gives exp(-2 pi i (k t0 mod n) / n) in bin k -- every bin of every position within four times the
    yardstick's worst bin, and the PSD row flat at 20 log10(2/n) within that bar in dB plus the dB rule's own rounding"""
    f = make(n)
    x, want = A.impulse_frames(n), A.impulse_want(n)
    got = A.as_complex(f.spectrum(x))
    err = np.abs(got - want)
    bar = A.impulse_bar(n)
    psd = batch_f32(f, x)
    t = 20.0 * math.log10(2.0 / n)
    dberr = np.abs(psd[:, :n].astype(np.float64) - t)
    report("B", n, err_eps=float(err.max()) / EPS, ratio=float(err.max()) / A.impulse_yardstick_error(n),
           db_of_bar=float(dberr.max()) / A.impulse_db_bar(n))
    i, k = np.unravel_index(int(np.argmax(err)), err.shape)
    assert err.max() <= bar, (n, "t0", A.impulse_positions(n)[i], "bin", int(k), float(err.max()) / EPS, bar / EPS)
    i, k = np.unravel_index(int(np.argmax(dberr)), dberr.shape)
    assert dberr.max() <= A.impulse_db_bar(n), (n, "t0", A.impulse_positions(n)[i], "bin", int(k), float(dberr.max()), A.impulse_db_bar(n))
    assert np.all(psd[:, n + 1] == psd[:, :n].max(axis=1))


def check_level_rows(n, psd, a, what):
    """every bin of row i is T(a_i) within 4 ulp32(M); the pair behind the row is the first of n equal maxima"""
    t, bound = A.level_target(n, a), A.level_bound(n, a)
    err = np.abs(psd[:, :n].astype(np.float64) - t[:, None])
    ulps = err / (bound[:, None] / 4.0)
    i, k = np.unravel_index(int(np.argmax(ulps)), ulps.shape)
    assert ulps.max() <= 4.0, (n, what, "a", float(a[i]), "bin", int(k), "T", float(t[i]), "got", float(psd[i, k]), float(ulps.max()))
    assert np.all(psd[:, :n] == psd[:, :1]), (n, what, "bins of one row differ")
    assert np.all(psd[:, n] == 0), (n, what)
    assert np.array_equal(psd[:, n + 1], psd[:, 0]), (n, what)
    return float(ulps.max())


@pytest.mark.parametrize("n", A.SIZES)
def test_db_rule_over_the_float_range(n):
    """C: a at sample 0 is (a, +-0) in every bin of every family, bit for bit; the PSD row is then 10 log10(fl(a a) 4 / n^2)
    within 4 ulp32(|T| + 20 log10(n/2)) from 2^-48 to 2^60 (batch_f32, the whole sweep in one call) and at the int16 levels
    down to one count (batch_i16)"""
    f = make(n)
    a = A.levels_f32(n)
    x = A.level_frames_f32(n)
    spec = f.spectrum(x)
    assert np.array_equal(spec[:, 0::2], np.repeat(a[:, None], n, axis=1)), (n, "re != a")
    assert np.all(spec[:, 1::2] == 0), (n, "im != 0")
    del spec
    u32 = check_level_rows(n, batch_f32(f, x), a, "batch_f32")
    u16 = check_level_rows(n, f.batch_host_i16(A.level_frames_i16(n)), A.levels_i16_as_float(), "batch_i16")
    report("C", n, f32_ulp=u32, i16_ulp=u16)
