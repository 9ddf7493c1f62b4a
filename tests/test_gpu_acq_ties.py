"""GPU: the first-maximum search of every FFT-acquire front end on boxcar sums that tie exactly (tests/peak_ties.py).

doBufferFFT (FUNcubeBPSKDemod.java:433-443) keeps the FIRST position of the largest 100-bin boxcar sum, and that position goes
straight into aveCentreBin: another index among equals is another centre bin, other 204 gathered bins, other bits.  tie_stream's
comb frames make the sums tie across the whole searched band -- every lane, wave and chunk of a search holds a copy of the
maximum -- and its growing amplitude keeps the centre-bin rule firing, so that binPos reaches the state (the census is asserted
on the oracle in tests/test_peak_ties_oracle.py).  Every front end is fed that stream and compared with the oracle: bits, the
(fi, fq) trace, the ten counters, all 18 state doubles, FEC results and decoded[].  front_kernel_name() is asserted for every
form, so that the form named is the form that ran."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import java_sdr_amd as J
import nonfinite as NF
import oracle_lib as O
import peak_ties as PT

pytestmark = pytest.mark.gpu

NFR = PT.ACQ_FRAMES
STATE_NAMES = {6: "avePeakPower", 7: "aveCentreBin"}
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------------------------------------------- inputs, oracle
@functools.lru_cache(maxsize=None)
def stream_i16(nsf, which):
    """"tie": the tie stream; "noise": uniform noise of the same length (no ties: the stream beside it)"""
    if which == "tie":
        x = PT.tie_stream(nsf, NFR)
    else:
        x = np.random.default_rng(nsf + 1).integers(-12000, 12001, 2 * nsf * NFR).astype(np.int16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def stream_f32(nsf, which):
    x = NF.offgrid(stream_i16(nsf, which))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle_result(nsf, rate, do_up, which, form):
    """the oracle over one stream, computed once and left unchanged"""
    o = O.Bpsk(rate=rate, blen=4 * nsf, do_fft=1, do_up=do_up, trace=nsf * NFR // max(1, rate // 9600) + 8)
    if form == "i16":
        o.receive_i16(stream_i16(nsf, which))
    else:
        x = stream_f32(nsf, which)
        for f in range(NFR):
            o.receive(x[2 * nsf * f:2 * nsf * (f + 1)])
    return NF.of_oracle(o)


def assert_equal(got, want, where):
    """every part of two results (NF.Acc.of / NF.of_oracle); the state doubles one by one, those that a wrong binPos reaches first"""
    gs, ws = got["state"], want["state"]
    acq = "state double 7 (aveCentreBin) %r / %r, state double 6 (avePeakPower) %r / %r, centreBin %d / %d" % (
        gs[7], ws[7], gs[6], ws[6], got["counters"][-1], want["counters"][-1])
    for i in [7, 6] + [i for i in range(18) if i not in STATE_NAMES]:
        name = " (%s)" % STATE_NAMES[i] if i in STATE_NAMES else ""
        assert NF.same_f64(gs[i], ws[i]), (where, "state double %d%s differs: %r / %r" % (i, name, gs[i], ws[i]), acq)
    NF.assert_results(got, want, where)


WHICH = ("tie", "noise")


def run_handle(nsf, rate, do_up, calls, form="i16", expect=None, S=2, check=None, via="batch"):
    """an ordinary handle of S streams (tie, noise, tie, ...) through calls of the given frame counts; expect: the front kernel of
    every call (one name, or one a call); the streams of `check` against the oracle"""
    assert sum(calls) == NFR
    d = J.Bpsk(rate=rate, blen=4 * nsf, do_fft=1, do_up=do_up, nstreams=S, max_batch_samples=max(calls) * nsf)
    src = stream_i16 if form == "i16" else stream_f32
    host = np.concatenate([src(nsf, WHICH[s % 2]) for s in range(S)])
    buf = J.DeviceBuffer.from_host(host) if via == "batch" else None
    check = list(range(min(S, 2))) if check is None else check
    acc = NF.Acc(S)
    names = []
    pos = 0
    for nf in calls:
        L = nf * nsf
        if via == "receive":
            assert S == 1 and nf == 1
            fr = host[2 * pos:2 * (pos + L)]
            d.receive(fr) if form == "f32" else d.receive_raw(fr)
        elif form == "i16":
            d.batch_i16(buf.ptr + 4 * pos, 2 * nsf * NFR, L)
        else:
            d.batch_f32(buf.ptr + 8 * pos, 2 * nsf * NFR, L)
        names.append(d.front_kernel_name())
        acc.take(d, only=check)
        pos += L
    if expect is not None:
        assert names == ([expect] * len(calls) if isinstance(expect, str) else list(expect)), names
    for s in check:
        assert_equal(acc.of(d, s), oracle_result(nsf, rate, do_up, WHICH[s % 2], form), (nsf, rate, do_up, form, calls, names[-1], "stream %d" % s))
    return d, acc


# ---------------------------------------------------------------------------------------------------------------- 2^k frames
@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("nsf", [1024, 2048, 4096, 8192])
def test_fused_kernel_one_frame_a_call(nsf, do_up):
    run_handle(nsf, 96000, do_up, [1] * NFR, expect="k_front_fft")


@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("nsf", [1024, 2048, 4096, 8192])
def test_three_phase_front_end(nsf, do_up, monkeypatch):
    run_handle(nsf, 96000, do_up, [2, 5, 7], expect="k_acq_fwd")
    # ... the call cut into launches of three frames a stream, tickets of two frames: a tie meets every seam of the scan
    monkeypatch.setenv("JSDR_ACQ_CHUNK", "3")
    monkeypatch.setenv("JSDR_ACQ_RUN", "2")
    run_handle(nsf, 96000, do_up, [2, 5, 7], expect="k_acq_fwd")


@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("nsf", [1024, 2048, 4096, 8192])
def test_fused_kernel_multi_frame_calls(nsf, do_up, monkeypatch):
    monkeypatch.setenv("JSDR_ACQ3", "0")
    run_handle(nsf, 96000, do_up, [2, 5, 7], expect="k_front_fft")


# ---------------------------------------------------------------------------------------------------------------- mixed radix
@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("nsf", [9600, 4800])
def test_mixed_radix_front_ends(nsf, do_up):
    rate = PT.ACQ_RATE[nsf]
    run_handle(nsf, rate, do_up, [1] * NFR, expect="k_front_fftm")
    run_handle(nsf, rate, do_up, [2, 5, 7], expect="k_acqm_fwd")  # few streams, several frames: frames fill the chip


@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("nsf", [4800, 4410])
def test_two_frames_at_once_at_a_full_grid_of_streams(nsf, do_up):
    """k_front_fftm2 (frames f and f + 1 of a stream together, the centre-bin rule for f then f + 1) keeps the call at a full grid
    of streams: 256 streams that repeat the tie stream and a noise stream; the first two and the last two against the oracle"""
    run_handle(nsf, PT.ACQ_RATE[nsf], do_up, [1, 2, 3, 8], expect=["k_front_fftm"] + ["k_front_fftm2"] * 3, S=256, check=[0, 1, 254, 255])


@pytest.mark.parametrize("do_up", [0, 1])
def test_the_19200_frames_fused_kernel(do_up):
    run_handle(19200, 192000, do_up, [1, 2, 5, 6], expect="k_front_fft2x")


# ---------------------------------------------------------------------------------------------------------------- any frame
@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("nsf", [16384, 17640])
def test_any_frame_passes(nsf, do_up):
    run_handle(nsf, PT.ACQ_RATE[nsf], do_up, [1, 2, 4, 7], expect="k_acqg_pass")


@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("nsf", [2048, 9600])
def test_any_frame_passes_forced_on_lds_frames(nsf, do_up, monkeypatch):
    monkeypatch.setenv("JSDR_ACQG", "1")
    run_handle(nsf, 96000, do_up, [1, 2, 4, 7], expect="k_acqg_pass")


# ---------------------------------------------------------------------------------------------------------------- float input
@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("nsf,expect", [(2048, "k_acq_fwd"), (9600, "k_acqm_fwd"), (17640, "k_acqg_pass")])
def test_float_batches(nsf, expect, do_up):
    run_handle(nsf, PT.ACQ_RATE[nsf], do_up, [2, 5, 7], form="f32", expect=expect)


@pytest.mark.parametrize("do_up", [0, 1])
def test_float_frames_through_receive(do_up):
    run_handle(2048, 96000, do_up, [1] * NFR, form="f32", expect="k_front_fft", S=1, via="receive")


# ---------------------------------------------------------------------------------------------------------------- channel handles
CHANNELS = [(12000, 1, 0), (12000, 1, 1), (12000, 0, 0)]  # (tuning, do_fft, do_up): both bands in FFT-acquire, a hand-tuned tab beside them


def channel_run(nsf, form, chans, calls, expect, launches):
    """a mode-channel handle over two inputs (tie, noise); returns (handle, Acc over stream = input * K + channel)"""
    K = len(chans)
    d = J.BpskChannels(96000, 4 * nsf, [t for t, _, _ in chans], do_up=[u for _, _, u in chans], ninputs=2, max_batch_samples=max(calls) * nsf,
                       do_fft=[f for _, f, _ in chans] if any(f for _, f, _ in chans) else None)
    src = stream_i16 if form == "i16" else stream_f32
    buf = J.DeviceBuffer.from_host(np.concatenate([src(nsf, w) for w in WHICH]))
    acc = NF.Acc(2 * K, get=lambda s: divmod(s, K))
    pos = 0
    for nf in calls:
        L = nf * nsf
        if form == "i16":
            d.batch_i16(buf.ptr + 4 * pos, 2 * nsf * NFR, L)
        else:
            d.batch_f32(buf.ptr + 8 * pos, 2 * nsf * NFR, L)
        if expect is not None:
            assert d.front_kernel_name() == expect, d.front_kernel_name()
            assert d.acq_last_launch() == tuple(v * nf for v in launches), (d.acq_last_launch(), nf)
        acc.take(d)
        pos += L
    return d, acc


@pytest.mark.parametrize("nsf,form", [(2048, "i16"), (8192, "i16"), (2048, "f32")])
def test_mode_channels_on_both_bands(nsf, form):
    """int16: both bands of an input from ONE forward transform (k_acqc_fwd, two searches over one spectrum); float: the per-band
    forward phase.  Each FFT-acquire channel equals the oracle and the ordinary handle of its band on the same stream; the tune
    channel beside them is what it is without them."""
    calls = [2, 5, 7]
    K = len(CHANNELS)
    expect, launches = ("k_acqc_fwd", (2, 4)) if form == "i16" else ("k_acq_fwd", (4, 4))  # (inputs x bands forward, inputs x channels inverted) a frame
    d, acc = channel_run(nsf, form, CHANNELS, calls, expect, launches)
    for c, (_, _, up) in enumerate(CHANNELS[:2]):
        o, oacc = run_handle(nsf, 96000, up, calls, form=form, expect="k_acq_fwd")
        for i in range(2):
            where = (nsf, form, "input %d" % i, "channel %d" % c)
            assert_equal(acc.of(d, i * K + c), oracle_result(nsf, 96000, up, WHICH[i], form), where)
            assert_equal(acc.of(d, i * K + c), oacc.of(o, i), where + ("against the ordinary handle",))
    alone, aacc = channel_run(nsf, form, [CHANNELS[2]], calls, None, None)
    for i in range(2):
        assert_equal(acc.of(d, i * K + 2), aacc.of(alone, i), (nsf, form, "input %d" % i, "the tune channel"))


# ---------------------------------------------------------------------------------------------------------------- the tail
def test_a_changed_centre_bin_meets_the_eight_streams_per_wave_tail():
    """k_tail8 serves handles of 2048 streams and more; JSDR_TAIL8=2 gives it every handle, and is read once a process: the case
    runs in a child process, as the tail's other tests do"""
    if os.environ.get("JSDR_TAIL8") == "2":
        for do_up in (0, 1):
            d, _ = run_handle(2048, 96000, do_up, [2, 5, 7], expect="k_acq_fwd", S=3, check=[0, 1, 2])
            assert d.tail_kernel_name() == "k_tail8", d.tail_kernel_name()
        return
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        os.path.join(HERE, "test_gpu_acq_ties.py"), "-k", "eight_streams_per_wave_tail"],
                       env=dict(os.environ, JSDR_TAIL8="2"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
