"""The demod handle's pure host unit (java-sdr_amd/csrc/demod_host.hip, demod_host.h) on the CPU: a stand-alone driver
(tests/tools/demod_host_driver.hip) is compiled with the unit, with the flags build.py gives it, and its answers are compared
bit for bit with restatements in Python float32 (tests/demod_numpy.py, which tests/test_demod.py holds the oracle to) and with
the oracle itself -- what tests/test_gpu_demod.py holds the handle's w_out and phi to.

No device and no library: what is checked here is what decides whether a handle's audio stays bit-identical to the reference
(the weights, the carrier walk) and what a channel call launches (which channels share a carrier table, which get float rows)."""
import importlib.util
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from demod_numpy import NumpyDemod, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "java-sdr_amd", "csrc")
RATE = 96000
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
OFF, RAW, AM, NFM, WFM = range(5)


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
        pytest.skip("no hipcc found: the demod host driver cannot be compiled")
    exe = str(tmp_path_factory.mktemp("demod_host") / "demod_host_driver")
    cmd = [cc] + b.COMMON + b.SOURCES["demod_host.hip"] + [os.path.join(ROOT, "tests", "tools", "demod_host_driver.hip"),
                                                          os.path.join(CSRC, "demod_host.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout.split("\n")
    return run


def hx(v):
    return float(v).hex()


def floats(line):
    return np.array([float.fromhex(t) for t in line.split()], np.float64).astype(f32)


def bits(v):
    return struct.pack("<f", float(v))


def same_bits(a, b):
    return np.asarray(a, f32).tobytes() == np.asarray(b, f32).tobytes()


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("flo,fhi", [(3000, 9000), (-12000, -3000), (0, 5000), (2000, 12000)])
def test_band_pass_weights_equal_the_restatement_and_the_oracle(driver, flo, fhi):
    """(0, 5000): phi = 0, still a band-pass -- car is reset and never moves"""
    out = driver(["weights %d %d %d" % (RATE, flo, fhi)])
    bandpass, phi = out[0].split()
    w = floats(out[1])
    p = NumpyDemod(RATE)
    p.weights(flo, fhi)
    ow, ophi = O.Demod(RATE).weights(flo, fhi)
    assert bandpass == "1"
    assert same_bits(w, p.wfir) and same_bits(f32(float.fromhex(phi)), p.phi)
    assert same_bits(w, ow) and same_bits(f32(float.fromhex(phi)), ophi)
    if flo == 0:
        assert bits(float.fromhex(phi)) == bits(0.0)


def test_the_all_pass_is_the_impulse_and_leaves_phi_alone(driver):
    out = driver(["weights %d %d %d" % (RATE, INT_MIN, INT_MAX)])
    bandpass, phi = out[0].split()
    assert bandpass == "0" and float.fromhex(phi) == 7.0  # (what the driver put there)
    want = np.zeros(21, f32)
    want[10] = 1
    assert same_bits(floats(out[1]), want)
    assert same_bits(floats(out[1]), O.Demod(RATE).weights(INT_MIN, INT_MAX)[0])


# ------------------------------------------------------------------------------------------------ the carrier walk
def walk(car, phi, L):
    p = NumpyDemod(RATE)
    p.car, p.phi = f32(car), f32(phi)
    tab = []
    for _ in range(L):
        tab.append(p.car)
        p.step_car()
    return np.array(tab, f32), p.car


def _phi(flo):
    p = NumpyDemod(RATE)
    p.weights(flo, flo + 6000)
    return p.phi


WALKS = [(0.0, _phi(3000), 1), (0.0, _phi(3000), 21), (0.0, _phi(3000), 100),   # 32 samples a turn: three wraps in 100
         (0.0, _phi(3000), 4099),                                                # (a tile and a bit)
         (1.25, _phi(-12000), 100),                                              # a negative phi: car only grows, as the reference's does
         (0.0, 0.0, 21), (2.5, 0.0, 21),                                         # phi = 0 never wraps
         (float(_phi(3000)), _phi(3000), 3),                                     # car - phi == 0 exactly: not below 0, no wrap
         (0.0, -0.0, 5), (-0.0, 0.0, 5)]                                         # signed zeros travel as they are


def test_carrier_walks_equal_the_restatement_entry_by_entry(driver):
    out = driver(["walk %s %s %d" % (hx(c), hx(p), L) for c, p, L in WALKS])
    for i, (c, p, L) in enumerate(WALKS):
        end, guard = out[2 * i].split()
        tab, car = walk(c, p, L)
        assert same_bits(floats(out[2 * i + 1]), tab), (c, p, L)
        assert bits(float.fromhex(end)) == bits(car), (c, p, L)
        assert float.fromhex(guard) == -1.0  # nothing written past L entries
    tab, _ = walk(*WALKS[2])
    assert int(np.sum(np.diff(tab) > 0)) >= 3  # (the three wraps are there)
    tab, car = walk(*WALKS[7])
    assert bits(tab[1]) == bits(0.0) and tab[2] > 6.0  # car hit +0 exactly and stayed; the next step went below and wrapped


# ------------------------------------------------------------------------------------------------ DemodConst / DemodChanConst
def test_both_const_structs_are_filled_alike(driver):
    cases = [(RATE, NFM, 1, 0, 1), (RATE, WFM, 0, 1, 0), (48000, AM, 1, 1, 1), (44100, OFF, 0, 0, 0), (RATE, RAW, 1, 1, 0)]
    out = driver(["const %d %d %d %d %d %s" % (c + (hx(0.375),)) for c in cases])
    for i, (rate, mode, fir, dwn, agc) in enumerate(cases):
        assert out[2 * i] == out[2 * i + 1]
        f = out[2 * i].split()
        fmgain = f32(rate) / (f32(5000) if mode == NFM else f32(75000))  # :410
        assert bits(float.fromhex(f[0])) == bits(fmgain)
        assert [int(x) for x in f[1:5]] == [mode, fir, dwn, agc]
        assert (float.fromhex(f[5]), float.fromhex(f[6])) == (0.375, -0.375)


# ------------------------------------------------------------------------------------------------ a channel call's plan
def expected_plan(chans, fused):
    """chans: (mode, dodwn, car, phi) a channel.  AM channels get the first float rows, the others follow when the call is not fused;
    the down-converting channels share a carrier table where car and phi are the same BITS"""
    K = len(chans)
    dslot, slot_chan = [-1] * K, []
    for c in range(K):
        if chans[c][0] == AM:
            dslot[c] = len(slot_chan)
            slot_chan.append(c)
    nam = len(slot_chan)
    if not fused:
        for c in range(K):
            if chans[c][0] != AM:
                dslot[c] = len(slot_chan)
                slot_chan.append(c)
    keys, row_chan, nco_row = [], [], [0] * K
    for c in range(K):
        if not chans[c][1]:
            continue
        k = bits(chans[c][2]) + bits(chans[c][3])
        if k not in keys:
            keys.append(k)
            row_chan.append(c)
        nco_row[c] = keys.index(k)
    return nam, dslot, slot_chan, nco_row, row_chan


def ask_plan(driver, chans, fused):
    out = driver(["plan %d %d" % (int(fused), len(chans))] + ["%d %d %s %s" % (m, d, hx(c), hx(p)) for m, d, c, p in chans])
    nam, nslots, rows = (int(x) for x in out[0].split())
    ints = [[int(x) for x in out[i].split()] for i in range(1, 5)]
    assert len(ints[1]) == nslots and len(ints[3]) == rows
    return nam, ints[0], ints[1], ints[2], ints[3]


PLANS = {
    "K = 1": [(NFM, 1, 0.5, 0.25)],
    "K = 1, AM": [(AM, 0, 0.0, 0.0)],
    "16 AM": [(AM, c % 2, 0.125 * (c % 4), 0.25) for c in range(16)],
    "mixed": [(NFM, 1, 0.5, 0.25), (AM, 1, 0.5, 0.25), (RAW, 0, 0.5, 0.25), (WFM, 1, 0.75, 0.25), (OFF, 1, 0.5, 0.5), (AM, 1, 0.75, 0.25)],
    "no down-conversion": [(NFM, 0, 0.5, 0.25), (AM, 0, 0.5, 0.25), (RAW, 0, 1.5, 0.75)],
    "signed zeros": [(NFM, 1, 0.5, 0.0), (NFM, 1, 0.5, -0.0), (RAW, 1, 0.0, 0.25), (RAW, 1, -0.0, 0.25), (WFM, 1, 0.5, 0.0)],
}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", list(PLANS))
def test_plans_equal_the_restatement(driver, name, fused):
    assert ask_plan(driver, PLANS[name], fused) == expected_plan(PLANS[name], fused)


def test_what_the_plans_are_about(driver):
    """the restated plans say what they should: the cases are what they were built to be"""
    nam, dslot, slot_chan, nco_row, row_chan = ask_plan(driver, PLANS["mixed"], True)
    assert (nam, slot_chan, dslot) == (2, [1, 5], [-1, 0, -1, -1, -1, 1])           # fused: the AM channels alone get float rows
    assert nco_row == [0, 0, 0, 1, 2, 1] and row_chan == [0, 3, 4]                   # channels 0, 1 share a table, and 3, 5
    nam, dslot, slot_chan, _, _ = ask_plan(driver, PLANS["mixed"], False)
    assert (nam, slot_chan, dslot) == (2, [1, 5, 0, 2, 3, 4], [2, 0, 3, 4, 5, 1])  # not fused: AM first, then the rest
    assert ask_plan(driver, PLANS["16 AM"], True)[:3] == (16, list(range(16)), list(range(16)))
    assert ask_plan(driver, PLANS["16 AM"], False)[:3] == (16, list(range(16)), list(range(16)))
    assert ask_plan(driver, PLANS["K = 1"], True) == (0, [-1], [], [0], [0])
    assert ask_plan(driver, PLANS["K = 1"], False) == (0, [0], [0], [0], [0])
    assert ask_plan(driver, PLANS["no down-conversion"], True)[3:] == ([0, 0, 0], [])  # rows = 0
    # +0.0 and -0.0 are different keys, as phi and as car; an equal pair still shares
    assert ask_plan(driver, PLANS["signed zeros"], True)[3:] == ([0, 1, 2, 3, 0], [0, 1, 2, 3])
