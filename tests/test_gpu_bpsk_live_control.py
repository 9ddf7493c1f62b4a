"""GPU: live control of a BPSK demodulator (FUNcubeBPSKDemod.actionPerformed, :165-190) -- jsdr_bpsk_set_tuning /
jsdr_bpsk_set_mode between calls, every other piece of state kept.  Every scenario of tests/golden/live_control_fixtures.npz
(the pure-Python restatement, tests/golden/live_control.py) on a 1-stream handle through receive_i16 and receive_f32 and
through the batch call, and on 64 identical streams of one batch handle: bits, FECDecode rc and bytes, the ten counters
and the 18 state doubles after every call, centreBin after every FFT frame -- bit for bit."""
import os
import sys

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import live_control_cases as M  # noqa: E402  (scenarios and inputs only)

pytestmark = pytest.mark.gpu
FX = np.load(os.path.join(HERE, "golden", "live_control_fixtures.npz"))
FREQ, PLUS10, SUB10, FFT, HIGH = 0, 1, 2, 3, 4  # live_control.COMMANDS


def act(d, cmd, val):
    """actionPerformed on a handle (or a group, for FREQ / HIGH)"""
    t, f, u = d.control()
    if cmd == FREQ:
        d.set_tuning(val)
    elif cmd == PLUS10:
        d.set_tuning(t + 10.0)
    elif cmd == SUB10:
        d.set_tuning(t - 10.0)
    elif cmd == HIGH:
        d.set_mode(f, 0 if u else 1)
    elif cmd == FFT:
        d.set_mode(0 if f else 1, u)
    else:
        raise AssertionError(cmd)


def actions(name):
    k = "l_" + name + "_"
    out = {}
    for c, cmd, v in zip(FX[k + "act_call"], FX[k + "act_cmd"], FX[k + "act_val"]):
        out.setdefault(int(c), []).append((int(cmd), float(v)))
    return out


def run(name, form, S=1):
    """-> per call: (counters, state, bits, fec, front kernel) of stream `s` for every stream"""
    p = M.SCENARIOS[name]
    raw = M.scenario_input(name)
    n, calls, N = p["frame"], p["calls"], sum(p["calls"])
    d = J.Bpsk(rate=p["rate"], blen=4 * n, tuning=p["tuning"], do_fft=p["do_fft"], do_up=p["do_up"], nstreams=S,
               max_batch_samples=max(calls))
    acts = actions(name)
    if form == "batch":
        d_iq = J.DeviceBuffer.from_host(np.tile(raw, S))
    elif form == "f32":
        buf = O.convert_i16(raw)
    rec = [[] for _ in range(S)]
    pos = 0
    for c, L in enumerate(calls):
        for cmd, v in acts.get(c, []):
            act(d, cmd, v)
        bits = [[] for _ in range(S)]
        fec = [[] for _ in range(S)]
        fronts = []
        if form == "batch":
            d.batch_i16(d_iq.ptr + 4 * pos, 2 * N, L)
            for s in range(S):
                bits[s].append(d.bits(s).copy())
                fec[s].extend(d.fec_results(s))
            fronts.append(d.front_kernel_name())
        else:
            for f in range(L // n):
                a = pos + f * n
                if form == "i16":
                    d.receive_raw(raw[2 * a:2 * (a + n)])
                else:
                    d.receive(buf[2 * a:2 * (a + n)])
                bits[0].append(d.bits(0).copy())
                fec[0].extend(d.fec_results(0))
                fronts.append(d.front_kernel_name())
        pos += L
        for s in range(S):
            c_ = d.counters(s)
            rec[s].append((list(c_.values()), d.state(s).copy(), np.concatenate(bits[s]), fec[s], fronts))
    return d, rec


def check(name, rec):
    k = "l_" + name + "_"
    bits, fec = [], []
    for c, (cnt, st, b, f, _) in enumerate(rec):
        assert cnt == [int(v) for v in FX[k + "counters"][c]], (name, c, cnt, list(FX[k + "counters"][c]))
        assert st.tobytes() == FX[k + "state"][c].tobytes(), (name, c, st, FX[k + "state"][c])
        bits.append(b)
        fec.extend(f)
        assert sum(len(x) for x in bits) == int(FX[k + "nbits"][c]), (name, c)
    assert np.array_equal(np.concatenate(bits), FX[k + "bits"]), name
    assert [r[0] for r in fec] == [int(v) for v in FX[k + "fec_rc"]], name
    for r, want in zip(fec, FX[k + "fec_data"]):
        assert np.array_equal(r[2], want), name


@pytest.mark.parametrize("name", list(M.SCENARIOS))
@pytest.mark.parametrize("form", ["batch", "i16", "f32"])
def test_live_control_one_stream_equals_the_restatement(name, form):
    _, rec = run(name, form)
    check(name, rec[0])


@pytest.mark.parametrize("name", list(M.SCENARIOS))
def test_live_control_64_streams_equal_the_restatement(name):
    _, rec = run(name, "batch", S=64)
    for s in (0, 17, 63):
        check(name, rec[s])
    for s in range(64):
        assert rec[s][-1][0] == rec[0][-1][0] and rec[s][-1][2].tobytes() == rec[0][-1][2].tobytes(), s


def test_a_frame_collected_across_the_actions_still_decodes():
    """'retune': +10 Hz three times and -10 Hz while the first FEC frame's 5200 bits are being collected"""
    _, rec = run("retune", "batch")
    fec = [r for call in rec[0] for r in call[3]]
    assert [r[0] for r in fec] == [int(v) for v in FX["l_retune_fec_rc"]] and fec[0][0] >= 0
    last = int(FX["l_retune_act_call"][-1])
    assert int(FX["l_retune_counters"][last][3]) == 0  # no FECDecode yet when the last action came


def fresh_front(p, do_up):
    n = p["frame"]
    raw = M.scenario_input("fft_high")[:2 * n] if p["do_fft"] else O.make_dbpsk_stream(1, 1, 16384)[0]
    d = J.Bpsk(rate=p["rate"], blen=4 * n, tuning=p["tuning"], do_fft=p["do_fft"], do_up=do_up, max_batch_samples=raw.size // 2)
    d.batch_i16(J.DeviceBuffer.from_host(raw).ptr, raw.size, raw.size // 2)
    return d.front_kernel_name()


def test_front_end_after_an_action_is_the_steady_state_one():
    """the call whose tuner crosses 0 takes k_front_split; no other call does; an unchanged action keeps k_fm; after a doUp
    toggle the FFT front end is the one a handle created with that doUp launches"""
    _, rec = run("zero", "batch")
    fronts = [r[4][0] for r in rec[0]]
    split = [c for c, f in enumerate(fronts) if f == "k_front_split"]
    tu = FX["l_zero_state"][:, 0]
    crossing = [c for c in range(1, len(tu)) if (tu[c - 1] > 0) != (tu[c] > 0)]
    assert crossing == [8, 12, 20, 26] and split == crossing, fronts
    assert fronts[:4] == ["k_fm"] * 4
    _, rec = run("same", "batch")
    assert [r[4][0] for r in rec[0]] == ["k_fm"] * len(rec[0])
    p = M.SCENARIOS["fft_high"]
    _, rec = run("fft_high", "batch")
    want = {u: fresh_front(p, u) for u in (0, 1)}
    up = 1
    acts = actions("fft_high")
    for c, r in enumerate(rec[0]):
        for cmd, _ in acts.get(c, []):
            if cmd == HIGH:
                up ^= 1
        assert r[4][0] == want[up], (c, r[4][0], want)


def test_after_a_mode_switch_the_front_end_is_the_steady_state_one():
    """'switch': in FFT-acquire mode the front end a handle created in that mode launches, in the tune mode k_fm again
    (from the call after the first tune call, which carries the seam through k_front_split)"""
    p = M.SCENARIOS["switch"]
    _, rec = run("switch", "batch")
    fronts = [r[4][0] for r in rec[0]]
    fft = {u: fresh_front(dict(p, do_fft=1), u) for u in (0, 1)}
    mode = {c: (int(FX["l_switch_counters"][c][9]) != 0) for c in range(len(fronts))}
    for c, f in enumerate(fronts):
        if mode[c]:
            assert f in fft.values(), (c, f, fft)
        elif c in (16, 30):
            assert f == "k_front_split", (c, f)
        elif c < 31:  # (from call 31 on +10 Hz: 12 010 Hz is not periodic)
            assert f == "k_fm", (c, f)


def _outputs(d):
    return list(d.counters(0).values()), d.state(0).tobytes(), d.bits(0).tobytes()


def test_a_refused_action_leaves_the_handle_untouched():
    raw = O.make_dbpsk_stream(20021006, 1, 4 * 16384)[0]
    iq = J.DeviceBuffer.from_host(raw)
    # FFT-acquire mode on a frame size it cannot take (below 416 samples) is refused, and says why
    a = J.Bpsk(blen=4 * 400, max_batch_samples=16384)
    b = J.Bpsk(blen=4 * 400, max_batch_samples=16384)
    for h in (a, b):
        h.batch_i16(iq.ptr, raw.size, 16384)
    with pytest.raises(J.JsdrError, match="frame size"):
        a.set_mode(1, 0)
    assert a.control() == (12000.0, 0, 0)
    for h in (a, b):
        h.batch_i16(iq.ptr + 4 * 16384, raw.size, 16384)
    assert _outputs(a) == _outputs(b)
    # the fast variant has no live control
    a = J.Bpsk(max_batch_samples=16384, variant="fast")
    b = J.Bpsk(max_batch_samples=16384, variant="fast")
    for h in (a, b):
        h.batch_i16(iq.ptr, raw.size, 16384)
    with pytest.raises(J.JsdrError, match="fast variant"):
        a.set_tuning(12010.0)
    with pytest.raises(J.JsdrError, match="fast variant"):
        a.set_mode(0, 1)
    for h in (a, b):
        h.batch_i16(iq.ptr + 4 * 16384, raw.size, 16384)
    assert _outputs(a) == _outputs(b)
    # and a retuned handle cannot become fast
    c = J.Bpsk(max_batch_samples=16384)
    c.set_tuning(12010.0)
    assert J.lib().jsdr_bpsk_set_variant(c.h, 1) == -1


def test_group_set_tuning_equals_single_handles():
    """jsdr_group_set_tuning on 2 members on one device (copies in RCCL's place): the gathered slots equal a plain
    4-stream handle's given the same actions"""
    n = 2048 * 40
    chunks = [2048 * 10] * 4
    iq = [O.make_dbpsk_stream(20021007, s, n, noise_sigma=600.0 + 100 * s)[0] for s in range(4)]
    plan = {1: 12010.0, 2: -50.0, 3: 12000.0}
    d = J.Bpsk(nstreams=4, max_batch_samples=max(chunks))
    d_iq = J.DeviceBuffer.from_host(np.concatenate(iq))
    info = d.slot_info()
    g = J.Group(2, 4, max(chunks), devices=[0, 0], gather_copy=True)
    bufs = [J.DeviceBuffer.from_host(np.concatenate(iq[r * 2:(r + 1) * 2])) for r in range(2)]
    pos = 0
    for c, L in enumerate(chunks):
        if c in plan:
            d.set_tuning(plan[c])
            g.set_tuning(plan[c])
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        g.batch_i16([b.ptr + 4 * pos for b in bufs], 2 * n, L)
        slots = J.DeviceBuffer(4 * info["slot_bytes"])
        d.pack_slots(slots)
        want = slots.to_host(np.uint8).reshape(4, info["slot_bytes"])
        for r in range(2):
            assert np.array_equal(g.gathered(r), want), (c, r)
        pos += L
    for r in range(2):
        _, dem = g.device(r)
        assert dem.control() == (12000.0, 0, 0)


def test_reconfigure_keeps_dm_max_corr_and_an_action_zeroes_it():
    """setup() on an unchanged format (:192-209) takes the configuration's values and resets no DSP state; the action
    with the same values (:188-190) zeroes dmMaxCorr"""
    raw = O.make_dbpsk_stream(20021008, 1, 2 * 32768)[0]
    iq = J.DeviceBuffer.from_host(raw)
    d = J.Bpsk(max_batch_samples=32768)
    d.batch_i16(iq.ptr, raw.size, 32768)
    before = d.counters(0)["dmMaxCorr"]
    assert before > 0
    d.reconfigure(12000.0, 0, 0)
    assert d.counters(0)["dmMaxCorr"] == before
    d.set_tuning(12000.0)
    assert d.counters(0)["dmMaxCorr"] == 0
