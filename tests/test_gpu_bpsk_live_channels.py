"""GPU: a channel handle whose channels switch between the tune mode and FFT-acquire live (jsdr_bpsk_create_live_channels):
every "FUNcube<idx>" tab's own "FFT/Tune" button (FUNcubeBPSKDemod.actionPerformed, :165-190) on one input.  Everything is
bit-exact: every stream against an ordinary handle given the same actions at the same points, one channel against the
pure-Python restatement's fixtures (tests/golden/live_control_fixtures.npz) with no GPU reference in the loop, the steady
state against the handles whose channel modes are fixed at creation, a seam call cut into several launches against the same
call in one, and every refusal against a twin handle that was never given the refused call."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O
import test_gpu_bpsk_live_control as LC  # (its helpers: the restatement's fixtures, actions(), check())
import test_gpu_bpsk_mode_channels as MC  # (mixed_input, slots_of, same_counters, same_state)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 96000
NIN = 3
# (tuning, do_fft, do_up) per channel at creation.  Five channels: the tune subset crosses k_chan_front's group of 4 as channels
# leave and join it
CHANNELS = [(12000, 0, 0), (12000, 1, 0), (12000, 1, 1), (30000, 0, 0), (12010, 0, 0)]
CALLS = [3, 1, 2, 1, 4, 2, 1, 3, 2]  # frames; then one call of frame + 77 samples (no FFT-acquire channel by then)
# before call k: ("mode", channel or None for every channel, do_fft, do_up) / ("tune", channel, Hz)
PLAN = {
    1: [("mode", 0, 1, 0)],                                    # channel 0 -> FFT-acquire
    2: [("mode", 1, 0, 0), ("mode", 3, 1, 1)],                 # channel 1 -> tune and channel 3 -> FFT-acquire, upper band: one call
    4: [("mode", 0, 0, 0)],                                    # channel 0 -> tune
    5: [("mode", 2, 0, 1), ("mode", 2, 1, 1)],                 # channel 2 -> tune and straight back: no seam, dmMaxCorr 0
    6: [("mode", None, 1, 0)],                                 # set_mode(1, 0) on all
    7: [("tune", 4, 11990.5), ("mode", None, 0, 0)],           # a retune while acquiring, then set_mode(0, 0) on all
}


def make_live(frame, chans, ninputs, max_samples):
    return J.BpskChannels(RATE, 4 * frame, [t for t, _, _ in chans], do_up=[u for _, _, u in chans], ninputs=ninputs,
                          max_batch_samples=max_samples, do_fft=[f for _, f, _ in chans], live=True)


def apply_plan(d, refs, conf, acts):
    """the actions before one call on the channel handle `d`, on the ordinary handles `refs` (one per channel, or None) and on
    the configuration list `conf`; channel_control after every action, dmMaxCorr == 0 on the acted channels only"""
    for a in acts:
        chans = range(len(conf)) if a[1] is None else [a[1]]
        if a[0] == "mode":
            _, ch, f, u = a
            if ch is None:
                d.set_mode(f, u)
            else:
                d.set_channel_mode(ch, f, u)
            for c in chans:
                conf[c] = (conf[c][0], f, u)
                if refs:
                    refs[c].set_mode(f, u)
        else:
            _, ch, hz = a
            d.set_channel_tuning(ch, hz)
            conf[ch] = (hz, conf[ch][1], conf[ch][2])
            if refs:
                refs[ch].set_tuning(hz)
        for c in range(len(conf)):
            assert d.channel_control(c) == (float(conf[c][0]), conf[c][1], conf[c][2]), (a, c)
            if refs:
                assert refs[c].control() == d.channel_control(c), (a, c)
                for i in range(d.ninputs):
                    assert d.counters(i, c)["dmMaxCorr"] == refs[c].counters(i)["dmMaxCorr"], (a, i, c)
            if c in chans:
                for i in range(d.ninputs):
                    assert d.counters(i, c)["dmMaxCorr"] == 0, (a, i, c)


_inputs = {}


def inputs_of(frame):
    """the three inputs of test 1's plan at this frame size, int16 (made once per frame size)"""
    if frame not in _inputs:
        n = (sum(CALLS) + 1) * frame + 77
        _inputs[frame] = [MC.mixed_input(500 + i, n)[0] for i in range(NIN)]
    return _inputs[frame]


# ---------------------------------------------------------------------------------------------------------------- 1
# k_acqc_fwd (both bands on a 2^k frame), k_acqm_fwd, the any-frame passes
@pytest.mark.parametrize("form", ["i16", "f32"])
@pytest.mark.parametrize("frame", [2048, 9600, 6000])
def test_every_stream_equals_an_ordinary_handle_given_the_same_actions(frame, form):
    xs = inputs_of(frame)
    n = xs[0].size // 2
    lens = [f * frame for f in CALLS] + [frame + 77]
    assert sum(lens) == n
    maxb = max(lens)
    d = make_live(frame, CHANNELS, NIN, maxb)
    assert d.channel_info() == (NIN, len(CHANNELS))
    refs = [J.Bpsk(rate=RATE, blen=4 * frame, tuning=t, do_fft=f, do_up=u, nstreams=NIN, max_batch_samples=maxb) for t, f, u in CHANNELS]
    if form == "i16":
        d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    else:
        d_iq = J.DeviceBuffer.from_host(np.concatenate([O.convert_i16(x) for x in xs]))
    conf = list(CHANNELS)
    pos = 0
    for k, L in enumerate(lens):
        apply_plan(d, refs, conf, PLAN.get(k, []))
        if form == "i16":
            d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        else:
            d.batch_f32(d_iq.ptr + 8 * pos, 2 * n, L)
        for c, r in enumerate(refs):
            if form == "i16":
                r.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
            else:
                r.batch_f32(d_iq.ptr + 8 * pos, 2 * n, L)
            for i in range(NIN):
                where = (frame, form, k, i, c)
                assert np.array_equal(d.bits(i, c), r.bits(i)), where
                assert np.array_equal(d.trace(i, c), r.trace(i)), where
                MC.same_counters(d.counters(i, c), r.counters(i), where)
                MC.same_state(d.state(i, c), r.state(i), where)
                fg, fo = d.fec_results(i, c), r.fec_results(i)
                assert [(a, b) for a, b, _ in fg] == [(a, b) for a, b, _ in fo], where
                for (_, _, x), (_, _, y) in zip(fg, fo):
                    assert np.array_equal(x, y), where
        pos += L
    # the plan did what it says: the retuned channel's tuPhase stood still while it acquired (calls 6) and moved on after
    assert conf == [(12000, 0, 0), (12000, 0, 0), (12000, 0, 0), (30000, 0, 0), (11990.5, 0, 0)]
    assert d.front_kernel_name() == "k_chan_front" and d.acq_last_launch() == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("form", ["batch", "i16"])
def test_one_channel_follows_the_restatement_and_its_neighbours_never_notice(form):
    """channel 1 is scenario "switch" of the restatement's fixtures (tune -> FFT -> tune -> FFT -> tune, "Track high" in both
    modes, +10 Hz); channels 0 (tune) and 2 (FFT-acquire, upper band) are never acted on and equal a handle whose modes are
    fixed at creation"""
    name = "switch"
    p = LC.M.SCENARIOS[name]
    raw = LC.M.scenario_input(name)
    frame, calls, N = p["frame"], p["calls"], sum(p["calls"])
    assert frame == 2048 and calls == [2048] * 40 and (p["tuning"], p["do_fft"], p["do_up"]) == (12000, 0, 0)
    d = make_live(frame, [(12000, 0, 0), (12000, 0, 0), (12000, 1, 1)], 1, frame)
    e = MC.make_handle(frame, [(12000, 0, 0), (12000, 1, 1)], 1, 1)
    acts = LC.actions(name)
    d_iq = J.DeviceBuffer.from_host(raw)
    rec = []
    modes = []
    pos = 0
    for c, L in enumerate(calls):
        for cmd, _ in acts.get(c, []):
            t, f, u = d.channel_control(1)
            if cmd == LC.FFT:
                d.set_channel_mode(1, 0 if f else 1, u)
            elif cmd == LC.HIGH:
                d.set_channel_mode(1, f, 0 if u else 1)
            elif cmd == LC.PLUS10:
                d.set_channel_tuning(1, t + 10.0)
            else:
                raise AssertionError(cmd)
            assert d.channel_control(0) == (12000.0, 0, 0) and d.channel_control(2) == (12000.0, 1, 1)
        for h in (d, e):
            if form == "batch":
                h.batch_i16(d_iq.ptr + 4 * pos, 2 * N, L)
            else:
                h.receive_raw(raw[2 * pos:2 * (pos + L)])
        pos += L
        rec.append((list(d.counters(0, 1).values()), d.state(0, 1).copy(), d.bits(0, 1).copy(), d.fec_results(0, 1), []))
        modes.append(d.channel_control(1)[1])
        for cd, ce in ((0, 0), (2, 1)):
            where = (form, c, cd)
            assert np.array_equal(d.bits(0, cd), e.bits(0, ce)), where
            assert np.array_equal(d.trace(0, cd), e.trace(0, ce)), where
            assert d.counters(0, cd) == e.counters(0, ce), where
            assert np.array_equal(d.state(0, cd), e.state(0, ce)), where
            assert [(a, b) for a, b, _ in d.fec_results(0, cd)] == [(a, b) for a, b, _ in e.fec_results(0, ce)], where
    LC.check(name, rec)
    # (the scenario is the one meant: both directions, twice)
    assert [c for c in range(1, 40) if modes[c] != modes[c - 1]] == [6, 16, 24, 30] and modes[0] == 0


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("frame", [2048, 9600])
def test_after_a_seam_call_the_launches_are_those_of_a_handle_created_that_way(frame):
    """Test 1's plan.  The call after every seam call (calls 2, 3, 5, 7, 8) reports the front kernel and the frames transformed
    that a fresh jsdr_bpsk_create_mode_channels handle of the then-current configuration reports for a call of that length.
    Calls 2 and 7 carry seams themselves: a seam re-runs no frame, so the counts are still the fresh handle's; call 7, in which
    EVERY channel returns to the tune mode, runs k_front_split alone and says so (no k_chan_front runs in it)."""
    xs = inputs_of(frame)
    n = xs[0].size // 2
    lens = [f * frame for f in CALLS]
    d = make_live(frame, CHANNELS, NIN, max(lens))
    d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    conf = list(CHANNELS)
    pos = 0
    checked = []
    for k, L in enumerate(lens):
        apply_plan(d, None, conf, PLAN.get(k, []))
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        if k - 1 in PLAN and k - 1 != 5:  # (call 5's two actions cancel: it carries no seam)
            fresh = MC.make_handle(frame, conf, NIN, L // frame)
            fresh.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
            assert d.acq_last_launch() == fresh.acq_last_launch(), (frame, k)
            if k == 7:
                assert (d.front_kernel_name(), fresh.front_kernel_name()) == ("k_front_split", "k_chan_front")
            else:
                assert d.front_kernel_name() == fresh.front_kernel_name(), (frame, k)
            checked.append((k, fresh.front_kernel_name()))
        pos += L
    both = {2048: "k_acqc_fwd", 9600: "k_acqm_fwd"}[frame]
    one = {2048: "k_acq_fwd", 9600: "k_acqm_fwd"}[frame]  # (from call 4 on the two FFT-acquire channels left both search the upper band)
    assert checked == [(2, both), (3, both), (5, one), (7, "k_chan_front"), (8, "k_chan_front")], checked


# ---------------------------------------------------------------------------------------------------------------- 4
def _chunked_case():
    """two calls on two inputs: 2 frames, then channels 0 (-> lower band) and 2 (-> upper band) switch tune -> FFT-acquire and
    a seam call of 7 frames follows -> sha256 of the slots and states after it, the frames transformed"""
    frame = 2048
    chans = [(12000, 0, 0), (12000, 1, 1), (13000, 0, 0)]
    xs = [MC.mixed_input(80 + i, 9 * frame)[0] for i in range(2)]
    d = make_live(frame, chans, 2, 7 * frame)
    d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    d.batch_i16(d_iq.ptr, 2 * 9 * frame, 2 * frame)
    d.set_channel_mode(0, 1, 0)
    d.set_channel_mode(2, 1, 1)
    d.profile_enable(True)
    d.batch_i16(d_iq.ptr + 4 * 2 * frame, 2 * 9 * frame, 7 * frame)
    slots = MC.slots_of(d, 6)
    states = np.concatenate([J.Bpsk.state(d, s) for s in range(6)])
    return hashlib.sha256(slots.tobytes() + states.tobytes()).hexdigest(), d.acq_last_launch(), d.profile_read()["k_acqc_fwd"][1]


def test_a_seam_call_cut_into_several_launches_gives_the_same_slots():
    want, launch, nfwd = _chunked_case()
    assert launch == (2 * 7, 2 * 3 * 7) and nfwd == 1
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_bpsk_live_channels as T\n"
            "print('RESULT', T._chunked_case())\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, JSDR_KNOBS="1", JSDR_ACQ_CHUNK="3", JSDR_ACQ_RUN="2")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(" ", 1)[1] for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
    assert lines == [repr((want, launch, 3))], (lines, want, launch)  # 7 frames in launches of 3, 3 and 1


# ---------------------------------------------------------------------------------------------------------------- 5
def test_refusals_leave_the_handle_and_its_pending_seams_as_they_were():
    frame, F = 2048, 4
    chans = [(12000, 0, 0), (13000, 1, 0), (14000, 1, 1)]
    x, _ = MC.mixed_input(91, 4 * F * frame)
    stride = x.size
    d_iq = J.DeviceBuffer.from_host(x)
    d = make_live(frame, chans, 1, F * frame)
    r = make_live(frame, chans, 1, F * frame)  # the same calls and actions, none of the refused ones
    conf = list(chans)

    def same(k):
        assert [d.channel_control(c) for c in range(3)] == [(float(t), f, u) for t, f, u in conf], k
        for c in range(3):
            assert d.channel_control(c) == r.channel_control(c), (k, c)
            assert d.counters(0, c) == r.counters(0, c), (k, c)
            assert np.array_equal(d.state(0, c), r.state(0, c)), (k, c)

    def refused(bad_calls):
        for k, (bad, match) in enumerate(bad_calls):
            with pytest.raises(J.JsdrError, match=match):
                bad()
            same(k)

    others = [
        (lambda: J.binding._check(J.lib().jsdr_bpsk_set_variant(d.h, 1), "jsdr_bpsk_set_variant"), "fast variant"),  # FAST
        (lambda: d.snapshot(), "no snapshot"),
        (lambda: d.set_channel_mode(3, 1, 0), "out of range"),
        (lambda: d.set_channel_mode(-1, 0, 0), "out of range"),
        (lambda: d.set_channel_tuning(5, 100.0), "out of range"),
        (lambda: d.set_channel_tuning(1, float("nan")), "not finite"),
    ]
    pos = 0
    for h in (d, r):
        h.batch_i16(d_iq.ptr, stride, F * frame)
    pos += F * frame
    # a tune -> FFT-acquire seam is pending: the call must be whole frames
    for h in (d, r):
        h.set_channel_mode(0, 1, 1)
    conf[0] = (12000, 1, 1)
    refused([(lambda: d.batch_i16(d_iq.ptr + 4 * pos, stride, 2 * frame - 1), "whole frames"),
             (lambda: d.batch_i16(d_iq.ptr + 4 * pos, stride, frame // 2), "whole frames")] + others)
    for h in (d, r):
        h.batch_i16(d_iq.ptr + 4 * pos, stride, 2 * frame)
    pos += 2 * frame
    assert np.array_equal(MC.slots_of(d, 3), MC.slots_of(r, 3))
    same("seam to FFT")
    # every channel returns to the tune mode: FFT-acquire -> tune seams are pending, the call needs 26 samples (and no more than that)
    for h in (d, r):
        h.set_mode(0, 0)
    conf = [(12000, 0, 0), (13000, 0, 0), (14000, 0, 0)]
    refused([(lambda: d.batch_i16(d_iq.ptr + 4 * pos, stride, 20), "at least 26 samples")] + others)
    for h in (d, r):
        h.batch_i16(d_iq.ptr + 4 * pos, stride, 26)
    pos += 26
    assert np.array_equal(MC.slots_of(d, 3), MC.slots_of(r, 3))
    for L in (1000, 3 * frame + 5):
        for h in (d, r):
            h.batch_i16(d_iq.ptr + 4 * pos, stride, L)
        pos += L
        assert np.array_equal(MC.slots_of(d, 3), MC.slots_of(r, 3))
        for c in range(3):
            assert np.array_equal(d.trace(0, c), r.trace(0, c))
    same("end")
    # the older creators keep their refusals, messages included
    e = MC.make_handle(frame, chans, 1, F)
    with pytest.raises(J.JsdrError, match="fixed at creation"):
        e.set_channel_mode(0, 1, 0)
    f = J.BpskChannels(RATE, 4 * frame, [12000, 13000])
    with pytest.raises(J.JsdrError, match="tune mode only"):
        f.set_channel_mode(0, 1, 0)
