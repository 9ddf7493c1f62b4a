"""GPU: the sync stage on engineered hits through every handle kind that test_gpu_sync_cases.py does not feed -- channel handles
(rows input * nchannels + channel), mode and live channel handles, tuned and tuned channel handles, ordinary FFT-acquire handles
-- and at the edge of a row's hit log (sync_handles.py has the inputs and the why; test_sync_handles_oracle.py counts, on the
oracle alone, what they contain).

After EVERY call and for EVERY row: one O.Bpsk per row, created with the row's (tuning, do_fft, do_up) and fed the same samples,
against the call's bits, all ten counters, the state doubles bit for bit (all 18 on handles with FFT-acquire rows) and the FEC
results (count, rc, trigger bit, 256 bytes).  Every comparison is an equality.  Every test asserts, from the handle's launch
counts, which sync kernels served its calls (rows > 1 are never fused: k_sync_t + k_sync_fin, or k_sync + k_sync_fin on the
handle created too large for the transposed image), and from front_kernel_name() the front end's family after every call.

  cap     rows in the order 7 hits, 9 (or 8 + 4), 8, a threshold stream on handles that log 8 hits a call: the overflowing row
          counts every hit, keeps the first eight in order, is flagged in its slot and refused by every getter from then on; the
          full row directly behind it and every other row equal the oracle in everything, in that call and all later ones

Child processes run the file again with JSDR_SYNC_T=0 (the strided k_sync everywhere), JSDR_TAIL8=2 (k_tail8 carries the register)
and JSDR_VITQ=1 (k_fec_bits + k_vitq, whose scratch is sized from trig_cap: the cap tests matter most there).

Checked by hand (scratch builds, not committed), one run of this file each: `slot < trig_cap` as `slot <= trig_cap` in
sync_fin_wave fails the cap tests on the row of 8 hits (its first logged hit becomes the overflowing row's ninth) -- both
ordinary-handle tests in both runs made, and one or none of the four channel-handle tests: the stray write and the row's own write
of that slot come from two workgroups of one launch, and which one lasts is the hardware's choice; without `nt = trig_cap` every
cap test fails (the slot of the overflowing row claims nine or twelve entries); `>= 45` as `> 45` fails every test of the file.
(The one-channel layout of the channel-handle cap test was added after these runs and met the first mutation only.)"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O
import sync_cases as Y
import sync_handles as H
from java_sdr_amd import sharding as SH

pytestmark = pytest.mark.gpu

SYNC_T = os.environ.get("JSDR_SYNC_T") != "0"
TAIL = "k_tail8" if os.environ.get("JSDR_TAIL8") == "2" else "k_tail"
VITQ = os.environ.get("JSDR_VITQ") == "1"
STATE = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)  # (6, 7 belong to the FFT-acquire mode)
COUNTERS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK", "centreBin")
GETTERS = ("bits", "fec_results", "decoded", "counters")
TUNE_12000 = (12000, 0, 0, 1)          # a row's configuration: (tuning, do_fft, do_up, samples a frame)
NO_SIGNAL = 30000                      # a tuning that sees none of the 13 200 Hz stream: garbage bits, which still equal the oracle
FFT_FRONTS = {9600: {"k_front_fftm", "k_front_fftm2", "k_acqm_fwd"}, 8192: {"k_front_fft", "k_acq_fwd"}}


@functools.lru_cache(maxsize=None)
def expected(case, carrier, nsamp, config, calls):
    """what the oracle of a row holds after each call: (bits of the call, counters, state, FEC results so far, decoded[]) -- computed once per
    (stream, configuration, schedule), shared, left unchanged"""
    iq = Y.stream_of(case, carrier)[:2 * nsamp]
    o = H.new_oracle(config)
    out, pos, nb = [], 0, 0
    for L in calls:
        o.receive_i16(iq[2 * pos:2 * (pos + L)])
        pos += L
        bits = o.bits()
        out.append((bits[nb:].copy(), o.counters(), o.state().copy(), [(rc, bi, dat.tobytes()) for rc, bi, dat in o.fec_results()],
                    o.decoded().tobytes()))
        nb = bits.size
    assert pos == nsamp
    return out


def run(d, inputs, rows, calls, form, fronts, nsamp=Y.N, all_state=False, flagged=(), slots=False):
    """d: the handle; inputs: (case, carrier) per input row of the device buffer; rows: (input, configuration) per row of the handle,
    in the handle's order; compared with the oracle after every call.  form: the sync kernels that must have served every call,
    "t" (k_sync_t + k_sync_fin) or "strided" (k_sync + k_sync_fin); fronts: the names front_kernel_name() may give.  flagged: the
    rows that must overflow their hit log (all others must not); slots: pack_slots is held to the oracle as well.
    -> per call and row what the getters gave"""
    calls = tuple(int(L) for L in calls)
    assert sum(calls) == nsamp and d.nstreams == len(rows)
    R = len(rows)
    want = [expected(inputs[i][0], inputs[i][1], nsamp, cfg, calls) for i, cfg in rows]
    cap = d.slot_info()["nfec_max"]
    d.profile_enable(True)
    d_iq = J.DeviceBuffer.from_host(np.concatenate([Y.stream_of(c, car)[:2 * nsamp] for c, car in inputs]))
    over, record = set(), []
    try:
        pos = 0
        nbits, nfec = [0] * R, [0] * R
        for k, L in enumerate(calls):
            d.batch_i16(d_iq.ptr + 4 * pos, 2 * nsamp, L)
            assert d.front_kernel_name() in fronts, (k, L, d.front_kernel_name(), fronts)
            if slots:
                info = d.slot_info()
                buf = J.DeviceBuffer(info["slot_bytes"] * R)
                d.pack_slots(buf)
                d.sync()
                packed = buf.to_host(np.uint8).reshape(R, -1).copy()
                buf.free()
            for r in range(R):
                where = (Y.name_of(inputs[rows[r][0]][0]), "row", r, rows[r][1], "call", k, "input samples", pos, L)
                bits, counters, state, fec, decoded = want[r][k]
                new = fec[nfec[r]:]
                if len(new) > cap:
                    over.add(r)
                if slots:
                    u = SH.unpack_slot(packed[r], info)
                    hdr = [int(v) for v in u["header"]]
                    assert hdr[11] == int(r in over), (where, "overflow flag", hdr[11])
                    assert hdr[2:11] == [counters[n] for n in COUNTERS[:9]] or r in over, (where, "slot counters", hdr)
                    assert hdr[5] == counters["cntFEC"] and hdr[4] == counters["cntBit"], (where, "cntFEC, cntBit", hdr, counters)
                    sf = [(rc, nbits[r] + bi, dat.tobytes()) for rc, bi, dat in u["fec"]]
                    assert sf == new[:cap], (where, "slot fec: the first hits, in order", [f[:2] for f in sf], [f[:2] for f in new[:cap]])
                    assert u["bits"].tobytes() == bits.tobytes(), (where, "slot bits")
                if r in over:  # sticky: refused in this call and in every later one
                    for g in GETTERS:
                        with pytest.raises(J.JsdrError):
                            getattr(J.Bpsk, g)(d, r)
                    record.append(None)
                else:
                    got = J.Bpsk.bits(d, r)
                    assert got.tobytes() == bits.tobytes(), (where, "bits", got.size, bits.size)
                    gc = J.Bpsk.counters(d, r)
                    assert [gc[n] for n in COUNTERS] == [counters[n] for n in COUNTERS], (where, COUNTERS, gc, counters)
                    gs = J.Bpsk.state(d, r)
                    idx = list(range(18)) if all_state else list(STATE)
                    assert gs[idx].tobytes() == state[idx].tobytes(), (where, "state", gs, state)
                    # (the library counts the trigger bit within the call, the oracle within the stream)
                    gf = [(rc, nbits[r] + bi, dat.tobytes()) for rc, bi, dat in J.Bpsk.fec_results(d, r)]
                    assert gf == new, (where, "fec", [f[:2] for f in gf], [f[:2] for f in new])
                    assert J.Bpsk.decoded(d, r).tobytes() == decoded, (where, "decoded")
                    record.append((got.tobytes(), tuple(gc[n] for n in COUNTERS), gs.tobytes(), gf))
                nbits[r] += bits.size
                nfec[r] = len(fec)
            pos += L
        assert pos == nsamp and d.tail_kernel_name() == TAIL
        assert over == set(flagged), (over, flagged)
        if R > 1:
            assert ("k_vitq" in d.fec_kernel_name()) == VITQ, d.fec_kernel_name()
        prof = d.profile_read()
        launches = {n: prof[n][1] for n in ("k_sync_t", "k_sync", "k_sync_fin")}
        if not SYNC_T:
            form = "strided"
        n = len(calls)
        assert R > 1 and launches == {"t": dict(k_sync_t=n, k_sync=0, k_sync_fin=n),
                                      "strided": dict(k_sync_t=0, k_sync=n, k_sync_fin=n)}[form], (form, n, launches)
    finally:
        d_iq.free()
    return record


def at_13200(names):
    return [(H.case_of(n), 13200.0) for n in names]


# ---------------------------------------------------------------------------------------------------------------- channel handles
def channels(ninputs, tunings, max_batch=Y.N):
    return J.BpskChannels(Y.RATE, 8, tunings, ninputs=ninputs, max_batch_samples=max_batch, size=4)


@pytest.mark.parametrize("schedule", ["one_call", "seams", "lengths"])
def test_channel_rows_with_hits_alternate_with_rows_without(schedule):
    """2 inputs x 3 channels: channels 0 and 2 at 12000 Hz, channel 1 where there is no signal; two cases with 4 and 11 hits"""
    tunings = [12000, NO_SIGNAL, 12000]
    rows = [(i, (t, 0, 0, 1)) for i in range(2) for t in tunings]
    d = channels(2, tunings)
    assert d.channel_info() == (2, 3)
    run(d, at_13200(["order", "neighbours_a"]), rows, Y.schedule(schedule), "t", {"k_chan_front"})


def test_all_thirteen_cases_as_inputs_of_one_channel_handle():
    tunings = [12000, NO_SIGNAL]
    rows = [(i, (t, 0, 0, 1)) for i in range(len(Y.CASES)) for t in tunings]
    run(channels(len(Y.CASES), tunings), [(c, 13200.0) for c in Y.CASES], rows, Y.schedule("seams"), "t", {"k_chan_front"})


def test_a_channel_handle_too_large_for_the_transposed_image_takes_the_strided_kernel():
    tunings = [12000, NO_SIGNAL, 12000]
    rows = [(i, (t, 0, 0, 1)) for i in range(2) for t in tunings]
    d = channels(2, tunings, max_batch=Y.fallback_batch_samples())
    run(d, at_13200(["threshold_last", "neighbours_b"]), rows, Y.schedule("seams"), "strided", {"k_chan_front"})


# ---------------------------------------------------------------------------------------------------------------- mode and live channels
MODE_INPUTS = ("threshold_spread", "placed_9600", "order")


def mode_channels(live):
    """one tune channel and one FFT-acquire (do_up = 0) channel per input, frames of 9600 samples, the whole-frame schedule"""
    frame = 9600
    v = H.FFT(frame)
    d = J.BpskChannels(Y.RATE, 4 * frame, [12000, 12000], do_up=[0, 0], ninputs=len(MODE_INPUTS), max_batch_samples=H.samples_of(v),
                       do_fft=[0, 1], live=live)
    rows = [(i, cfg) for i in range(len(MODE_INPUTS)) for cfg in ((12000, 0, 0, 1), H.oracle_config(v))]
    return run(d, at_13200(MODE_INPUTS), rows, H.fft_calls(frame), "t", {"k_acqm_fwd"}, nsamp=H.samples_of(v), all_state=True)


@functools.lru_cache(maxsize=None)
def mode_channel_record():
    return mode_channels(False)


def test_mode_channels_each_row_against_the_oracle_of_its_own_mode():
    mode_channel_record()


def test_live_channels_in_steady_state_equal_the_mode_channels():
    assert mode_channels(True) == mode_channel_record()


# ---------------------------------------------------------------------------------------------------------------- tuned handles
def test_tuned_handle_one_stream_per_tuned_variant():
    variants = H.TUNED + [H.PASS_THROUGH]
    inputs = [(Y.BY_NAME[n], H.carrier_of(H.TUNE(t))) for n, t in variants]
    rows = [(i, (t, 0, 0, 1)) for i, (_, t) in enumerate(variants)]
    d = J.BpskTuned(Y.RATE, 8, [t for _, t in variants], max_batch_samples=Y.N, size=4)
    run(d, inputs, rows, H.tuned_calls(), "t", {"k_front_pst"})


def test_tuned_channel_handle_one_channel_per_tuned_variant():
    """every input carries one variant's stream; channel 0 is tuned to it, channel 1 is passed through or tuned to a neighbour's
    carrier, so rows with hits alternate with rows of garbage"""
    inputs = [(Y.BY_NAME[n], H.carrier_of(H.TUNE(t))) for n, t in H.TUNED]
    others = [0 if i % 2 == 0 else H.TUNED[i][1] - 3000 for i in range(len(H.TUNED))]
    tunings = [t for (_, v), o in zip(H.TUNED, others) for t in (v, o)]
    rows = [(i, (t, 0, 0, 1)) for i in range(len(H.TUNED)) for t in tunings[2 * i:2 * i + 2]]
    d = J.BpskTunedChannels(Y.RATE, 8, len(H.TUNED), 2, tunings, max_batch_samples=Y.N, size=4)
    assert d.channel_info() == (len(H.TUNED), 2)
    run(d, inputs, rows, H.tuned_calls(), "t", {"k_chan_front_pst"})


# ---------------------------------------------------------------------------------------------------------------- FFT-acquire
@pytest.mark.parametrize("frame", H.FRAMES)
def test_fft_acquire_handle_on_whole_frame_calls(frame):
    v = H.FFT(frame)
    names = H.FFT_CASES[frame]
    d = J.Bpsk(rate=Y.RATE, blen=4 * frame, do_fft=1, do_up=0, nstreams=len(names), max_batch_samples=H.samples_of(v))
    rows = [(i, H.oracle_config(v)) for i in range(len(names))]
    run(d, at_13200(names), rows, H.fft_calls(frame), "t", FFT_FRONTS[frame], nsamp=H.samples_of(v), all_state=True)


# ---------------------------------------------------------------------------------------------------------------- the cap edge
def cap_rows(over, copies):
    names = H.CAP_ROWS[over]
    assert [H.CAP_HITS.get(n, 0) for n in names] == [7, over, 8, 0]
    return at_13200(names), [(i, TUNE_12000) for i in range(len(names)) for _ in range(copies)]


@pytest.mark.parametrize("over", [9, 12])
def test_a_row_past_its_hit_log_on_an_ordinary_handle_leaves_the_rows_around_it_alone(over):
    inputs, rows = cap_rows(over, 1)
    d = J.Bpsk(nstreams=4, max_batch_samples=H.CAP_BATCH)
    assert d.slot_info()["nfec_max"] == 8
    run(d, inputs, rows, H.cap_calls(), "t", {"k_fm", "k_front"}, flagged={1}, slots=True)


@pytest.mark.parametrize("over,nch", [(9, 1), (9, 2), (12, 1), (12, 2)])
def test_a_row_past_its_hit_log_on_a_channel_handle_leaves_the_rows_around_it_alone(over, nch):
    """4 inputs x 1 channel: the rows of the ordinary handle.  4 inputs x 2 channels, both at 12000 Hz: rows 7, 7, over, over, 8, 8,
    threshold, threshold -- two flagged rows side by side, the second with a full row directly behind it"""
    inputs, rows = cap_rows(over, nch)
    d = channels(4, [12000] * nch, max_batch=H.CAP_BATCH)
    assert d.slot_info()["nfec_max"] == 8 and d.channel_info() == (4, nch)
    run(d, inputs, rows, H.cap_calls(), "t", {"k_chan_front"}, flagged={1} if nch == 1 else {2, 3}, slots=True)


# ---------------------------------------------------------------------------------------------------------------- each kernel
NTESTS = 17


def child(env):
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__), "-k", "not child_process"],
                       env=dict(os.environ, JSDR_KNOBS="1", **env), capture_output=True, text=True, timeout=300)
    m = re.search(r"(\d+) passed", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) == NTESTS and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_once_more_through_the_strided_k_sync_in_a_child_process():
    child(dict(JSDR_SYNC_T="0"))


def test_once_more_through_k_tail8_in_a_child_process():
    child(dict(JSDR_TAIL8="2"))


def test_once_more_through_k_fec_bits_in_a_child_process():
    child(dict(JSDR_VITQ="1"))
