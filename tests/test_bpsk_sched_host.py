"""The BPSK host scheduler (java-sdr_amd/csrc/bpsk_sched.hip) on the CPU: a stand-alone driver (tests/tools/sched_driver.hip) is
compiled with the unit, with the flags build.py gives it, and its schedules are compared with a restatement of the recurrences in
Python floats -- IEEE doubles, every operation rounded by itself, so the restatement is exact and independent of the C++.

No device and no library: what is checked here is what decides whether a stream stays bit-identical to the reference (the
tuner / VCO walk, the crossing after a retune, the 9-bit expansion) and which front end a call takes (the period searches,
the keys, the channel sharing)."""
import importlib.util
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "java-sdr_amd", "csrc")
HIST = 26
SLACK = 128  # FM_TABLE_SLACK
TWO_PI = 2.0 * math.pi
ZEROS = [0] * HIST


def _build_py():
    spec = importlib.util.spec_from_file_location("jsdr_build", os.path.join(ROOT, "java-sdr_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    b = _build_py()
    cc = b.hipcc()
    if not (os.path.exists(cc) if os.path.isabs(cc) else shutil.which(cc)):
        pytest.skip("no hipcc found: the scheduler driver cannot be compiled")
    exe = str(tmp_path_factory.mktemp("sched") / "sched_driver")
    cmd = [cc] + b.COMMON + b.SOURCES["bpsk_sched.hip"] + [os.path.join(ROOT, "tests", "tools", "sched_driver.hip"),
                                                          os.path.join(CSRC, "bpsk_sched.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout.split("\n")
    return run


# ------------------------------------------------------------------------------------------------ the restatement
def tuner_inc(tuning, rate):
    return 2.0 * math.pi * tuning / float(rate)  # :189 / :196, left to right


def tuner_walk(tu, inc, n):
    """FUNcubeBPSKDemod.java:384-390: the 9-bit index of every sample (256: passed through) and tuPhase at the end"""
    k9 = []
    for _ in range(n):
        tu += inc
        if tu > TWO_PI:
            tu -= TWO_PI
        k9.append(int(tu * 256.0 / TWO_PI) % 256 if tu > 0.0 else 256)
    return k9, tu


def vco_walk(vco, ds, decim, n):
    """:468, :511-516: the table index of every decimated sample, vcoPhase and dsCnt at the end"""
    vinc = 2.0 * math.pi * 1200.0 / float(9600)
    k = []
    for _ in range(n):
        ds += 1
        if ds >= decim:
            ds = 0
            vco += vinc
            if vco > TWO_PI:
                vco -= TWO_PI
            k.append(int(vco * 256.0 / TWO_PI) % 256)
    return k, vco, ds


def holds(k, p):
    return k[:len(k) - p] == k[p:]


def period_ordinary(k):
    """the first p whose 1024-sample head repeats is the one candidate; it counts if it holds over the whole call"""
    head = k[:1024]
    for p in range(1, min(256, len(k) - 1) + 1):
        if holds(head, p):
            return p if holds(k, p) else 0
    return 0


def period_channel(k):
    """the first p that holds over the whole call"""
    for p in range(1, min(256, len(k) - 1) + 1):
        if holds(k, p):
            return p
    return 0


def expected_schedule(tu0, inc, vco0, ds0, decim, L, do_fft, first, khist):
    k9, tu1 = ([256] * L, tu0) if do_fft else tuner_walk(tu0, inc, L)
    m = [k != 256 for k in k9]
    e = {"ktu": list(khist) + [k & 255 for k in k9], "tu1": tu1}
    e["mix"] = 1 if all(m) else (0 if not any(m) else -1)
    e["f0"] = int(m[0])
    e["n0"] = next((n for n in range(1, L) if m[n] != m[0]), L)
    e["kvco"], e["vco1"], e["ds1"] = vco_walk(vco0, ds0, decim, L)
    e["k9"] = k9
    e["tper"] = 0
    if not do_fft and e["mix"] == 1:
        e["tper"] = period_ordinary(e["ktu"][HIST if first else 0:])
    return e


# ------------------------------------------------------------------------------------------------ talking to the driver
def hx(v):
    return float(v).hex()


def tab8(k):
    return "".join("%02x" % v for v in k)


def tab16(k):
    return "".join("%04x" % v for v in k)


def untab(s, w):
    s = s.split(" ", 1)[1] if " " in s else ""
    return [int(s[i:i + w], 16) for i in range(0, len(s), w)]


def key_line(cmd, tu0, inc, vco0, ds0, decim, L, do_fft, first, khist):
    return "%s %s %s %s %d %d %d %d %d %s" % (cmd, hx(tu0), hx(inc), hx(vco0), ds0, decim, L, int(do_fft), int(first), tab8(khist))


def parse_sched(out, i):
    f = out[i].split()
    d = dict(mix=int(f[0]), f0=int(f[1]), n0=int(f[2]), tper=int(f[3]), nds=int(f[4]), tu1=float.fromhex(f[5]),
             vco1=float.fromhex(f[6]), ds1=int(f[7]))
    d["ktu"] = untab(out[i + 1], 2)
    d["kvco"] = untab(out[i + 2], 2)
    d["tcs"] = [tuple(int(v) for v in t.split(":")) for t in out[i + 3].split()[1:]]
    return d


def check_schedule(got, exp, L, first):
    assert got["ktu"] == exp["ktu"]
    assert got["kvco"] == exp["kvco"] and got["nds"] == len(exp["kvco"])
    assert (got["tu1"], got["vco1"], got["ds1"]) == (exp["tu1"], exp["vco1"], exp["ds1"])
    assert (got["mix"], got["f0"], got["n0"]) == (exp["mix"], exp["f0"], exp["n0"])
    assert got["ktu"][L:] == exp["ktu"][L:] and len(got["ktu"]) == L + HIST  # the history of the next call
    assert got["tper"] == exp["tper"]
    if got["tper"] > 0:
        p = got["tper"]
        assert len(got["tcs"]) == p + SLACK
        # entry e serves the samples n with (n + 26) mod p == e mod p; sample n's index is ktu[26 + n]
        lo = 0 if first else -HIST
        for e, (c, s) in enumerate(got["tcs"]):
            n = next(n for n in range(lo, L) if (n + HIST) % p == e % p)
            assert c == exp["ktu"][HIST + n] and s == 1000 + c, (e, n)
    else:
        assert got["tcs"] == []


def continuing(tuning, rate, warm=1000):
    """a state in mid-stream: tuPhase, vcoPhase and the 26-entry history after `warm` samples from the start"""
    inc = tuner_inc(tuning, rate)
    k9, tu = tuner_walk(0.0, inc, warm)
    _, vco, _ = vco_walk(0.0, 0, 10, warm)
    return tu, vco, k9[-HIST:]


LS = [1, 25, 26, 27, 1023, 1024, 1025, 4097]
DECIMS = [1, 4, 5, 10, 20]


# ------------------------------------------------------------------------------------------------ the ordinary handle
def test_tuner_inc_is_the_left_to_right_product(driver):
    cases = [(12000.0, 96000), (1234.5, 96000), (-250.5, 48000), (0.0, 44100), (95999.5, 96000)]
    out = driver(["inc %s %d" % (hx(t), r) for t, r in cases])
    assert [float.fromhex(o) for o in out[:len(cases)]] == [tuner_inc(t, r) for t, r in cases]


@pytest.mark.parametrize("tuning,rate", [(12000.0, 96000), (1234.5, 96000)])
def test_schedules_equal_the_restated_walk(driver, tuning, rate):
    """every L, first and continuing calls, every decimation with dsCnt at 0 and at decim - 1"""
    inc = tuner_inc(tuning, rate)
    tu_c, vco_c, k9_c = continuing(tuning, rate)
    cases = []
    for L in LS:
        for decim in DECIMS:
            for ds0 in sorted({0, decim - 1}):
                cases.append((0.0, inc, 0.0, ds0, decim, L, False, True, ZEROS))
                cases.append((tu_c, inc, vco_c, ds0, decim, L, False, False, [k & 255 for k in k9_c]))
    out = driver([key_line("sched", *c) for c in cases])
    for i, c in enumerate(cases):
        check_schedule(parse_sched(out, 4 * i), expected_schedule(*c), c[5], c[7])


def test_12_khz_at_96_khz_has_period_8_under_both_policies(driver):
    inc = tuner_inc(12000.0, 96000)
    tu_c, vco_c, k9_c = continuing(12000.0, 96000)
    lines, shapes = [], []
    for L in (27, 1023, 1024, 1025, 4097):
        for first, tu0, hist in ((True, 0.0, ZEROS), (False, tu_c, k9_c)):
            lines.append(key_line("sched", tu0, inc, 0.0, 0, 10, L, False, first, [k & 255 for k in hist]))
            lines += ["chans 1", "%s %s %d %d %s" % (hx(tu0), hx(inc), L, int(first), tab16(hist))]
            shapes.append((L, first, tu0, hist))
    out = driver(lines)
    for i, (L, first, tu0, hist) in enumerate(shapes):
        o = 8 * i
        got = parse_sched(out, o)
        assert got["tper"] == 8 and len(got["tcs"]) == 8 + SLACK
        check_schedule(got, expected_schedule(tu0, inc, 0.0, 0, 10, L, False, first, [k & 255 for k in hist]), L, first)
        assert out[o + 4] == "1"
        fresh, per, tu1 = out[o + 5].split()
        k9, tu_end = tuner_walk(tu0, inc, L)
        assert (int(fresh), int(per), float.fromhex(tu1)) == (1, 8, tu_end)
        tab = untab(out[o + 7], 4)
        full = list(hist) + k9
        lo = 0 if first else -HIST
        assert len(tab) == 8 and all(tab[(n + HIST) % 8] == full[HIST + n] for n in range(lo, L))  # entry (n + 26) mod p
        assert untab(out[o + 6], 4) == full[L:]


def test_a_tuning_without_a_short_period_gets_full_tables(driver):
    inc = tuner_inc(1234.5, 96000)
    tu_c, vco_c, k9_c = continuing(1234.5, 96000)
    L = 4097
    out = driver([key_line("sched", tu_c, inc, vco_c, 3, 10, L, False, False, [k & 255 for k in k9_c]),
                  "chans 1", "%s %s %d 0 %s" % (hx(tu_c), hx(inc), L, tab16(k9_c))])
    got = parse_sched(out, 0)
    k9, tu1 = tuner_walk(tu_c, inc, L)
    assert period_ordinary(k9_c + k9) == 0 and period_channel(k9_c + k9) == 0
    assert got["tper"] == 0 and got["tcs"] == [] and got["ktu"] == k9_c + k9 and got["mix"] == 1
    assert out[4] == "1" and out[5].split()[:2] == ["1", "0"]  # computed, fresh, per == 0
    assert untab(out[7], 4) == k9_c + k9  # a full table: 26 + L entries


def test_a_period_of_the_head_alone_does_not_count(driver):
    """12000.125 Hz at 96 kHz drifts off the 8-cycle after some 3000 samples: the 1024-sample head repeats with 8, the call does not.
    Both searches verify over every sample of the call, each by its own policy, and neither reports a period"""
    L = 4097
    inc = tuner_inc(12000.125, 96000)
    k9, _ = tuner_walk(0.0, inc, L)
    assert period_ordinary(k9[:1024]) == 8 and period_ordinary(k9) == 0 and period_channel(k9) == 0
    out = driver([key_line("sched", 0.0, inc, 0.0, 0, 10, L, False, True, ZEROS), "chans 1", chan_line(0.0, inc, L, True, ZEROS),
                  key_line("sched", 0.0, inc, 0.0, 0, 10, 1024, False, True, ZEROS)])
    assert parse_sched(out, 0)["tper"] == 0 and int(out[5].split()[1]) == 0
    assert parse_sched(out, 8)["tper"] == 8  # (the head as a call of its own)


@pytest.mark.parametrize("tuning", [0.0, -500.0])
def test_no_sample_is_mixed_at_a_tuning_of_zero_or_below(driver, tuning):
    inc = tuner_inc(tuning, 96000)
    lines = [key_line("sched", 0.0, inc, 0.0, 0, 10, L, False, True, ZEROS) for L in LS]
    lines += ["chans 1", "%s %s 1025 1 %s" % (hx(0.0), hx(inc), tab16(ZEROS))]
    out = driver(lines)
    for i, L in enumerate(LS):
        got = parse_sched(out, 4 * i)
        assert (got["mix"], got["f0"], got["n0"], got["tper"]) == (0, 0, L, 0)
        assert got["ktu"] == [0] * (HIST + L)
        check_schedule(got, expected_schedule(0.0, inc, 0.0, 0, 10, L, False, True, ZEROS), L, True)
    o = 4 * len(LS)
    assert out[o] == "1" and int(out[o + 1].split()[1]) == 1 and untab(out[o + 3], 4) == [256]  # every k9 is 256: one period of it


def _crossing_start(inc, steps):
    """tu0 > 0 from which `steps` whole steps of the (negative) increment stay above 0 and the next does not"""
    return -inc * (steps + 0.5)


@pytest.mark.parametrize("L", [27, 1025])
def test_a_retune_crossing_is_found_where_the_restated_walk_puts_it(driver, L):
    """tuPhase > 0 and a negative increment: the sign test (:388) flips inside the call.  The boundary placements: the last mixed
    sample is sample 0 (n0 == 1), the only unmixed sample is the last (n0 == L - 1); and in the middle."""
    inc = tuner_inc(-50.0, 96000)  # (small enough that the start stays below 2 pi: 1026 steps are 3.4 rad)
    hist = [(7 * i) % 256 for i in range(HIST)]
    mh = [1] * HIST
    lines, want = [], []
    for n0 in (1, L // 2, L - 1):
        tu0 = _crossing_start(inc, n0)
        lines.append(key_line("sched", tu0, inc, 0.5, 2, 10, L, False, False, hist))
        lines.append("expand8 " + tab8(mh))
        lines.append("expand8 -")
        want.append((n0, tu0))
    out = driver(lines)
    for i, (n0, tu0) in enumerate(want):
        got = parse_sched(out, 6 * i)
        exp = expected_schedule(tu0, inc, 0.5, 2, 10, L, False, False, hist)
        assert exp["n0"] == n0  # (the placement is what this case set out to build)
        assert (got["mix"], got["f0"], got["n0"]) == (-1, 1, n0)
        check_schedule(got, exp, L, False)
        # the 9-bit expansion of a crossing call: the history as its flags say, the schedule's index where mixed, 256 where not
        assert untab(out[6 * i + 4], 4) == hist + exp["k9"]
        assert untab(out[6 * i + 5], 4) == [256] * HIST + exp["k9"]


def test_crossings_at_and_past_the_ends_of_a_call(driver):
    inc = tuner_inc(-1000.0, 96000)
    L = 27
    up = tuner_inc(12000.0, 96000)
    cases = [(_crossing_start(inc, 0), inc),   # sample 0 is already at or below 0: no sample is mixed, no crossing in the call
             (_crossing_start(inc, L), inc),   # the flip comes with the next call's sample 0: every sample is mixed
             (-3.0, up)]                       # upward: passed through, then mixed
    out = driver([key_line("sched", tu0, i, 0.0, 0, 10, L, False, False, ZEROS) for tu0, i in cases])
    got = [parse_sched(out, 4 * i) for i in range(3)]
    for g, (tu0, i) in zip(got, cases):
        check_schedule(g, expected_schedule(tu0, i, 0.0, 0, 10, L, False, False, ZEROS), L, False)
    assert (got[0]["mix"], got[0]["f0"], got[0]["n0"]) == (0, 0, L)
    assert (got[1]["mix"], got[1]["f0"], got[1]["n0"]) == (1, 1, L)
    assert got[2]["mix"] == -1 and got[2]["f0"] == 0 and 0 < got[2]["n0"] < L


def test_fft_acquire_leaves_the_tuner_standing(driver):
    inc = tuner_inc(12000.0, 96000)
    lines, cases = [], []
    for L in LS:
        for decim in DECIMS:
            c = (1.25, inc, 0.75, decim - 1, decim, L, True, False, ZEROS)
            cases.append(c)
            lines.append(key_line("sched", *c))
    out = driver(lines)
    for i, c in enumerate(cases):
        got = parse_sched(out, 4 * i)
        assert got["tu1"] == 1.25 and got["ktu"] == [0] * (HIST + c[5]) and (got["mix"], got["f0"], got["n0"], got["tper"]) == (0, 0, c[5], 0)
        check_schedule(got, expected_schedule(*c), c[5], False)  # ... and only the VCO moves


def test_the_vco_schedule_is_the_schedules_own(driver):
    lines, cases = [], []
    for L in LS:
        for decim in DECIMS:
            for ds0 in sorted({0, decim - 1}):
                cases.append((0.625, ds0, decim, L))
                lines += ["vco %s %d %d %d" % (hx(0.625), ds0, decim, L)] * 2  # the second time it is there already
    out = driver(lines)
    for i, (vco0, ds0, decim, L) in enumerate(cases):
        k, vco1, ds1 = vco_walk(vco0, ds0, decim, L)
        f = out[4 * i].split()
        assert (int(f[0]), int(f[1]), float.fromhex(f[2]), int(f[3])) == (1, len(k), vco1, ds1)
        assert untab(out[4 * i + 1], 2) == k
        assert out[4 * i + 2].split()[0] == "0" and untab(out[4 * i + 3], 2) == k


def test_mix_flags_move_on_with_the_call(driver):
    mh = [(i % 3 != 0) * 1 for i in range(HIST)]
    cases = [(1, 1, 1), (25, 1, 10), (26, 1, 26), (27, 0, 5), (1025, 1, 1000), (1025, 0, 1025)]
    out = driver(["mhist %s %d %d %d" % (tab8(mh), L, f0, n0) for L, f0, n0 in cases])
    for o, (L, f0, n0) in zip(out, cases):
        flags = mh + [f0 if n < n0 else 1 - f0 for n in range(L)]
        assert untab(o, 2) == flags[-HIST:]


def test_the_key_holds_the_increment_and_the_mode(driver):
    """a schedule computed for one increment must not serve a request with another, or in the other mode, when everything else is
    equal -- live control needs no rule of its own for that"""
    inc = tuner_inc(12000.0, 96000)
    base = (0.0, inc, 0.0, 0, 10, 1024, False, True, ZEROS)

    def other(**kw):
        names = ["tu0", "inc", "vco0", "ds0", "decim", "L", "do_fft", "first", "khist"]
        return tuple(kw.get(n, v) for n, v in zip(names, base))
    asks = [base, other(inc=tuner_inc(12010.0, 96000)), other(do_fft=True), other(tu0=0.5), other(vco0=0.5), other(ds0=1), other(L=1025),
            other(first=False), other(khist=[1] + [0] * 25), other(decim=5)]
    out = driver([key_line("sched", *base)] + [key_line("match", *a) for a in asks])
    assert out[4:4 + len(asks)] == ["1"] + ["0"] * (len(asks) - 1)


# ------------------------------------------------------------------------------------------------ channels
def chan_line(tu0, inc, L, first, hist):
    return "%s %s %d %d %s" % (hx(tu0), hx(inc), L, int(first), tab16(hist))


def test_channels_with_equal_keys_share_one_computation(driver):
    a, b, L = tuner_inc(12000.0, 96000), tuner_inc(1234.5, 96000), 1025
    lines = ["chans 4", chan_line(0.0, a, L, True, ZEROS), chan_line(0.0, b, L, True, ZEROS), "-", chan_line(0.0, a, L, True, ZEROS),
             # the next call: the periodic pair from where it ended, and channel 1 once more from the start (its schedule is there)
             "chans 4"]
    k9a, tua = tuner_walk(0.0, a, L)
    lines += [chan_line(tua, a, L, False, k9a[-HIST:]), chan_line(0.0, b, L, True, ZEROS), "-", chan_line(tua, a, L, False, k9a[-HIST:])]
    out = driver(lines)
    assert out[0] == "2"  # channels 0 and 3 are one computation, channel 2 does not run the tuner
    ch = [(out[1 + 3 * c].split(), untab(out[2 + 3 * c], 4), untab(out[3 + 3 * c], 4)) for c in range(4)]
    assert [c[0][0] for c in ch] == ["1", "1", "0", "1"]
    assert ch[0] == ch[3] and int(ch[0][0][1]) == 8 and float.fromhex(ch[0][0][2]) == tua and ch[0][1] == k9a[-HIST:]
    k9b, tub = tuner_walk(0.0, b, L)
    assert int(ch[1][0][1]) == 0 and float.fromhex(ch[1][0][2]) == tub and ch[1][2] == ZEROS + k9b
    o = 13
    assert out[o] == "1"  # one more for the pair, none for channel 1
    ch2 = [(out[o + 1 + 3 * c].split(), untab(out[o + 3 + 3 * c], 4)) for c in range(4)]
    assert [c[0][0] for c in ch2] == ["1", "0", "0", "1"]
    assert ch2[0] == ch2[3] and ch2[1][1] == ZEROS + k9b


def test_seam_expansion_passes_the_history_through(driver):
    """a channel's first tune call after FFT-acquire frames: the history is all 256, the call's entries are the schedule's -- from
    a periodic table and from a full one"""
    L = 1025
    lines, walks = [], []
    for tuning in (12000.0, 1234.5):
        inc = tuner_inc(tuning, 96000)
        tu0, _, hist = continuing(tuning, 96000)
        walks.append(tuner_walk(tu0, inc, L)[0])
        lines += ["chans 1", chan_line(tu0, inc, L, False, hist), "expand9 0"]
    out = driver(lines)
    assert int(out[1].split()[1]) == 8 and untab(out[4], 4) == [256] * HIST + walks[0]
    assert int(out[6].split()[1]) == 0 and untab(out[9], 4) == [256] * HIST + walks[1]
