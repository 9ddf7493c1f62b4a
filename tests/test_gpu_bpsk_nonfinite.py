"""GPU: NaN, +-Inf and +-3e38 through every float entry point of the BPSK demodulator, against one O.Bpsk per stream fed the same
floats frame by frame.  The reference takes any float, and Java defines what follows (nonfinite.py); above all, one NaN makes all
eight dmEnergy slots NaN for the rest of the stream, the peak search (:586-592: eMax = -1.0e10F, `dmEnergy[n] > eMax`) then takes
no slot, dmNewPeak keeps its value, and the slicer goes on at the frozen peak -- bits, FEC frames and all.

The inputs and what the oracle alone makes of them are pinned on the CPU by test_nonfinite_oracle.py.  Doubles are compared by
nonfinite.same_f64 (identical bits, or both NaN); bits, counters, FEC rc / bit index / bytes and decoded[] exactly.

Without a knob these small handles take k_tail (one wave a stream); a child process with JSDR_TAIL8=2 takes them through k_tail8
(eight streams a wave), another with JSDR_FM=0 through the three-kernel front end: both argmax sites, both front ends.  Every test
asserts the tail kernel (and the front kernel where the shape fixes it) that served its handle.

+-Inf in FFT-acquire is left out: which bins of a frame turn to Inf and which to NaN depends on the order of the transform's
additions; JTransforms' order is unknown, so no expectation could be pinned to the reference.  NaN (every bin NaN, whatever the
order) and +-3e38 (finite in double all the way) are in."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import java_sdr_amd as J
import nonfinite as NF
import oracle_lib as O

pytestmark = pytest.mark.gpu

PAD = 6
# which kernels the handles of this process take: k_tail (one wave a stream) unless JSDR_TAIL8=2 forces k_tail8; the fused float front
# end in the standard tune mode unless JSDR_FM=0 forces the three-kernel path
TAIL = "k_tail8" if os.environ.get("JSDR_TAIL8") == "2" else "k_tail"
FRONT = "k_front" if os.environ.get("JSDR_FM") == "0" else "k_fm_f32"


def feed(d, xs, calls, acc, start=0, only=None):
    """the calls' samples of every row from a [rows][2 L + PAD] device buffer whose padding is NaN (a read outside a row's samples of
    THIS call poisons its trace) -> the position after the last call"""
    pos = start
    for L in calls:
        h = np.full((len(xs), 2 * L + PAD), np.nan, np.float32)
        for s, x in enumerate(xs):
            h[s, :2 * L] = x[2 * pos:2 * (pos + L)]
        buf = J.DeviceBuffer.from_host(h)
        d.batch_f32(buf.ptr, 2 * L + PAD, L)
        acc.take(d, only)
        pos += L
    return pos


@functools.lru_cache(maxsize=None)
def tune_set(which):
    """(cases, inputs, the oracle's results) -- computed once, shared, left unchanged"""
    cases = NF.TUNE_CASES if which == "batch" else NF.PHASE_CASES
    xs = NF.tune_inputs(cases)
    for x in xs:
        x.setflags(write=False)
    return cases, xs, [NF.of_oracle(NF.run_oracle(x)) for x in xs]


# ---------------------------------------------------------------------------------------------------------------- tune mode
def test_tune_mode_batch_of_twelve_streams():
    cases, xs, want = tune_set("batch")
    S = len(xs)
    d = J.Bpsk(nstreams=S, max_batch_samples=max(NF.TUNE_CALLS))
    acc = NF.Acc(S)
    assert feed(d, xs, NF.TUNE_CALLS, acc) == NF.NSAMP
    assert (d.front_kernel_name(), d.tail_kernel_name()) == (FRONT, TAIL)
    got = [acc.of(d, s) for s in range(S)]
    clean = [s for s, c in enumerate(cases) if not c[3]]
    # the clean streams first: a poisoned neighbour in the wave must not reach them
    c = J.Bpsk(nstreams=len(clean), max_batch_samples=max(NF.TUNE_CALLS))
    acc_c = NF.Acc(len(clean))
    feed(c, [xs[s] for s in clean], NF.TUNE_CALLS, acc_c)
    for k, s in enumerate(clean):
        assert np.isfinite(got[s]["trace"]).all() and np.isfinite(got[s]["state"]).all(), cases[s][0]
        NF.assert_results(got[s], acc_c.of(c, k), (cases[s][0], "beside poisoned streams / among clean ones"), fft=False)
    for s in range(S):
        NF.assert_results(got[s], want[s], cases[s][0], fft=False)


def test_tune_mode_inf_on_q_at_each_phase_of_the_tuner():
    cases, xs, want = tune_set("phases")
    d = J.Bpsk(nstreams=8, max_batch_samples=max(NF.TUNE_CALLS))
    acc = NF.Acc(8)
    feed(d, xs, NF.TUNE_CALLS, acc)
    assert (d.front_kernel_name(), d.tail_kernel_name()) == (FRONT, TAIL)
    for s in range(8):
        NF.assert_results(acc.of(d, s), want[s], cases[s][0], fft=False)


@pytest.mark.parametrize("name", ["nan_i_hi", "inf_i_mid"])
def test_one_stream_handles_batch_and_receive(name):
    cases, xs, want = tune_set("batch")
    s = [c[0] for c in cases].index(name)
    d = J.Bpsk(nstreams=1, max_batch_samples=max(NF.TUNE_CALLS))
    acc = NF.Acc(1)
    feed(d, [xs[s]], NF.TUNE_CALLS, acc)
    assert (d.front_kernel_name(), d.tail_kernel_name()) == (FRONT, TAIL)
    NF.assert_results(acc.of(d, 0), want[s], (name, "one-stream batch_f32"), fft=False)
    n = 2048
    r = J.Bpsk(nstreams=1)
    acc_r = NF.Acc(1)
    for k in range(NF.NSAMP // n):
        r.receive(xs[s][2 * n * k:2 * n * (k + 1)])
        acc_r.take(r)
    assert r.tail_kernel_name() == TAIL
    NF.assert_results(acc_r.of(r, 0), want[s], (name, "receive_f32 frame by frame"), fft=False)


def child(env, select, least):
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__), "-k", select],
                       env=dict(os.environ, JSDR_KNOBS="1", **env), capture_output=True, text=True, timeout=300)
    m = re.search(r"(\d+) passed", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) >= least and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_tune_mode_once_more_on_the_three_kernel_path_in_a_child_process():
    child(dict(JSDR_FM="0"), "(tune_mode or one_stream) and not child_process", 4)


def test_once_more_through_the_eight_streams_per_wave_tail_in_a_child_process():
    """JSDR_TAIL8=2: every handle takes k_tail8 -- its argmax, its locked path beside NaN streams, its general path"""
    child(dict(JSDR_TAIL8="2"), "(tune_mode or one_stream or odd_rate or fft_acquire_2048 or channel_handle or checkpoint or hand_over) and not child_process", 13)


def test_odd_rate_through_the_generic_front_end():
    """44.1 kHz / 8 kHz: no exact tuner cycle, decimation 4"""
    xs = NF.odd_inputs()
    d = J.Bpsk(rate=NF.ODD_RATE, tuning=NF.ODD_TUNING, nstreams=3, max_batch_samples=max(NF.ODD_CALLS))
    acc = NF.Acc(3)
    assert feed(d, xs, NF.ODD_CALLS, acc) == NF.ODD_NSAMP
    assert d.front_kernel_name() in ("k_front", "k_front_any") and d.tail_kernel_name() == TAIL
    for s, (name, _) in enumerate(NF.ODD_CASES):
        o = NF.run_oracle(xs[s], rate=NF.ODD_RATE, tuning=NF.ODD_TUNING)
        NF.assert_results(acc.of(d, s), NF.of_oracle(o), name, fft=False)


# ---------------------------------------------------------------------------------------------------------------- FFT-acquire
def fft_acquire(n, rate, do_up, expect=None):
    xs = NF.fft_inputs(n, rate, do_up)
    frames = [1, 4, 2, 5]  # the poisoned frame 3 inside a call; a one-frame call (the fused kernel), calls of several frames
    assert sum(frames) == NF.FFT_FRAMES
    d = J.Bpsk(rate=rate, blen=4 * n, do_fft=1, do_up=do_up, nstreams=3, max_batch_samples=max(frames) * n)
    acc = NF.Acc(3)
    feed(d, xs, [f * n for f in frames], acc)
    if expect:
        assert d.front_kernel_name() in expect, (d.front_kernel_name(), expect)
    assert d.tail_kernel_name() == TAIL
    for s, what in enumerate(("a NaN in frame 3", "+-3e38 in frame 3", "clean")):
        o = NF.run_oracle(xs[s], rate=rate, frame=n, do_fft=1, do_up=do_up)
        # (bits, the trace, centreBin, avePeakPower and aveCentreBin among the rest: the frames after the poisoned one are the point)
        NF.assert_results(acc.of(d, s), NF.of_oracle(o), (n, rate, do_up, what), fft=True)


@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("acq3", [None, "0"])
def test_fft_acquire_2048_with_either_front_end(acq3, do_up, monkeypatch):
    forced = os.environ.get("JSDR_ACQ3") is not None or os.environ.get("JSDR_ACQG") is not None
    if acq3 is not None and not forced:
        monkeypatch.setenv("JSDR_ACQ3", acq3)  # the fused kernel for calls of several frames too
    fft_acquire(2048, 96000, do_up, None if forced else (("k_acq_fwd",) if acq3 is None else ("k_front_fft",)))


@pytest.mark.parametrize("do_up", [0, 1])
@pytest.mark.parametrize("n,rate", [s for s in NF.FFT_SIZES if s[0] != 2048])
def test_fft_acquire_other_front_end_families(n, rate, do_up):
    forced = os.environ.get("JSDR_ACQ3") is not None or os.environ.get("JSDR_ACQG") is not None
    # the mixed-radix LDS front ends (fused or three-phase, as the call's shape has it), the two-halves kernel of the 19200 frame,
    # the any-frame passes for 512
    family = {512: ("k_acqg_pass",), 19200: ("k_front_fft2x",)}.get(n, ("k_acqm_fwd", "k_front_fftm", "k_front_fftm2"))
    fft_acquire(n, rate, do_up, None if forced else family)


# ---------------------------------------------------------------------------------------------------------------- channels
def channel_inputs(n):
    out = []
    for i in range(2):
        acc = np.zeros(2 * n, np.int64)
        for k, f in enumerate((13200.0, 31200.0)):
            acc += O.make_dbpsk_stream(1100 + i, k, n, carrier_hz=f, noise_sigma=900.0)[0].astype(np.int64)
        out.append(NF.offgrid(np.clip(acc, -32768, 32767).astype(np.int16)))
    return out


def test_channel_handle_with_one_poisoned_input():
    tunings = [12000, 12010, 30000]
    calls = [256 * 10 * 3 + 77, 256 * 10 + 1230, 4000]
    N = sum(calls)
    clean = channel_inputs(N)
    xs = [NF.poison(clean[0], [(3001, NF.I, NF.NAN)]), clean[1]]
    K = len(tunings)

    def run(inputs):
        d = J.BpskChannels(96000, 8192, tunings, ninputs=2, max_batch_samples=max(calls))
        acc = NF.Acc(2 * K, get=lambda s: (s // K, s % K))
        feed(d, inputs, calls, acc)
        assert (d.front_kernel_name(), d.tail_kernel_name()) == ("k_chan_front", TAIL)
        return [acc.of(d, s) for s in range(2 * K)]

    got, ref = run(xs), run(clean)
    for i in range(2):
        for k, t in enumerate(tunings):
            h = J.Bpsk(tuning=t, nstreams=1, max_batch_samples=max(calls))
            a1 = NF.Acc(1)
            feed(h, [xs[i]], calls, a1)
            NF.assert_results(got[i * K + k], a1.of(h, 0), ("one-stream handle", i, k), fft=False)
            NF.assert_results(got[i * K + k], NF.of_oracle(NF.run_oracle(xs[i], tuning=t)), ("oracle", i, k), fft=False)
            if i == 0:
                assert np.isnan(got[k]["state"][8:16]).all(), k
            else:  # untouched by the other input's NaN
                assert np.isfinite(got[K + k]["trace"]).all() and np.isfinite(got[K + k]["state"]).all(), k
                NF.assert_results(got[K + k], ref[K + k], ("input 1 beside a clean input 0", k), fft=False)


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_after_the_nan_has_gone_through():
    cases, xs, _ = tune_set("batch")
    names = [c[0] for c in cases]
    N, cut = 90000, [20000 + 7, 15000]  # the NaN at 6149 is well behind the cut
    rows = [xs[names.index(k)][:2 * N] for k in ("nan_i_hi", "clean_b", "clean_c")]
    rest = [N - sum(cut) - 30011, 30011]
    a = J.Bpsk(nstreams=3, max_batch_samples=40000)
    acc_a = NF.Acc(3)
    pos = feed(a, rows, cut, acc_a)
    assert np.isnan(a.state(0)[8:16]).all() and a.tail_kernel_name() == TAIL
    blob = a.save(0, 1)  # NaN energies are data, not indices: the blob is taken, and accepted below
    b = J.Bpsk(nstreams=4, max_batch_samples=65000)
    b.restore(blob, 1)
    acc_b = NF.Acc(4)
    acc_b.bits[1], acc_b.trace[1], acc_b.fec[1], acc_b.nbits[1] = list(acc_a.bits[0]), list(acc_a.trace[0]), list(acc_a.fec[0]), acc_a.nbits[0]
    feed(a, rows, rest, acc_a, start=pos)
    feed(b, [rows[1], rows[0], rows[2], rows[1]], rest, acc_b, start=pos, only=[1])
    want = NF.of_oracle(NF.run_oracle(rows[0]))
    assert np.isnan(want["state"][8:16]).all() and want["counters"][2] > 1000
    NF.assert_results(acc_a.of(a, 0), want, "the handle that was saved", fft=False)
    NF.assert_results(acc_b.of(b, 1), want, "the handle that was restored", fft=False)
    for s in (1, 2):
        NF.assert_results(acc_a.of(a, s), NF.of_oracle(NF.run_oracle(rows[s])), ("clean neighbour", s), fft=False)


# ---------------------------------------------------------------------------------------------------------------- hand-over
@pytest.mark.parametrize("value", [NF.NAN, NF.PINF], ids=["nan", "inf"])
def test_hand_over_to_int16_with_a_non_finite_float_in_the_history(value):
    """the 26-sample input history goes from float to int16 only if every float is a (float)s/32767f value.  Call A ends in 40
    samples of the short grid in both streams, so that one NaN (one Infinity) among the last 26 floats of stream 0 is the ONLY
    offender: the int16 call is refused and the handle is as it was; the control handle, fed the same floats without it, takes the
    int16 call.  Once 26 values of the short grid have followed, the int16 call is taken, and the stream goes on with its NaN state"""
    S, TAILG = 2, 40
    A, B, Cc, D = 9000 + 3, 5000, 4030 + 7, 8000
    N = A + B + Cc + D
    raws = [O.make_dbpsk_stream(9700 + s, s, N, noise_sigma=600.0)[0] for s in range(S)]
    grid = [O.convert_i16(r) for r in raws]
    clean = []
    for s, r in enumerate(raws):
        x = NF.offgrid(r)
        x[2 * (A - TAILG):2 * A] = grid[s][2 * (A - TAILG):2 * A]  # the end of call A on the short grid
        x[2 * (A + B):] = grid[s][2 * (A + B):]                    # calls C and D on the short grid
        clean.append(x)
    xs = [NF.poison(clean[0], [(A - 5, NF.Q, value)]), clean[1]]
    assert np.array_equal(xs[1][2 * (A - 26):2 * A], grid[1][2 * (A - 26):2 * A])  # stream 1's history is on the grid
    assert int((xs[0][2 * (A - 26):2 * A] != grid[0][2 * (A - 26):2 * A]).sum()) == 1  # one float of the history is off the grid
    d_raw = J.DeviceBuffer.from_host(np.concatenate(raws))
    # the control: the same grid tail, nothing non-finite -- the int16 call is taken
    c = J.Bpsk(nstreams=S, max_batch_samples=max(A, D))
    acc_c = NF.Acc(S)
    feed(c, clean, [A], acc_c)
    c.batch_i16(d_raw.ptr + 4 * A, 2 * N, B)
    acc_c.take(c)
    for s in range(S):
        o = NF.run_oracle(np.concatenate([clean[s][:2 * A], grid[s][2 * A:2 * (A + B)]]))
        NF.assert_results(acc_c.of(c, s), NF.of_oracle(o), ("control: float, int16", s), fft=False)
    a = J.Bpsk(nstreams=S, max_batch_samples=max(A, D))
    b = J.Bpsk(nstreams=S, max_batch_samples=max(A, D))  # the twin that is never asked
    acc_a, acc_b = NF.Acc(S), NF.Acc(S)
    feed(a, xs, [A], acc_a)
    feed(b, xs, [A], acc_b)
    before = a.save()
    with pytest.raises(J.JsdrError, match="cannot be carried over"):
        a.batch_i16(d_raw.ptr + 4 * A, 2 * N, B)
    assert a.save() == before
    feed(a, xs, [B], acc_a, start=A)
    feed(b, xs, [B], acc_b, start=A)
    for s in range(S):
        NF.assert_results(acc_a.of(a, s), acc_b.of(b, s), ("after the refused call", s), fft=False)
    # C ends in more than 26 values of the short grid: the int16 call D is taken
    feed(a, xs, [Cc], acc_a, start=A + B)
    a.batch_i16(d_raw.ptr + 4 * (A + B + Cc), 2 * N, D)
    acc_a.take(a)
    assert a.front_kernel_name() in ("k_fm", "k_front") and a.tail_kernel_name() == TAIL
    for s in range(S):
        o = NF.run_oracle(xs[s])
        if s == 0:
            assert np.isnan(o.state()[8:16]).any() and not np.isfinite(o.state()[8:16]).any()
        NF.assert_results(acc_a.of(a, s), NF.of_oracle(o), ("float, float, grid floats, int16", s), fft=False)
