"""GPU: the 9600 Hz tail kernels on every bit-clock peak position and every move of the peak (peak_walk.py has the inputs and the
why; test_peak_walk_oracle.py counts, on the oracle alone, what they contain).

Ordinary tune-mode handles fed by batch_i16, one O.Bpsk per stream fed the same samples in frames of one sample.  After EVERY call:
the call's bits, all counters, the state doubles bit for bit (the eight dmEnergy slots, dmEnergyOut, energy1 / energy2, dmLastIQ,
the phases), and the FEC results (count, rc, bit index, bytes).

  locked   the eight delayed streams as the eight lane groups of one k_tail8 wave, locked at the eight positions; calls that start
           and end at every bit position, of 1 .. 9 outputs, of lengths that are no multiple of the decimation, and of several
           whole chunks; then with a ninth stream (a second wave of one live stream and seven shadow lane groups)
  walks    the noise-only and fading streams, all 56 moves: in one call, and in calls cut inside the bit period of a hand-over of
           every move
  mixed    one wandering stream among seven locked ones, in lane group 0, 3 and 7: the locked streams go through the general path

Without a knob these handles take k_tail (one wave a stream); a child process with JSDR_TAIL8=2 takes them through k_tail8 in its
four-wave workgroups, another with JSDR_TAIL8_WPB=1 as well in one-wave workgroups.  Every test asserts the tail kernel that served it."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O
import peak_walk as P
from test_gpu_bpsk import same_counters, same_state

pytestmark = pytest.mark.gpu

TAIL = "k_tail8" if os.environ.get("JSDR_TAIL8") == "2" else "k_tail"
STATE = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)  # (6, 7 belong to the FFT-acquire mode)


def samples_of(case, n):
    return P.stream_of(case)[:2 * n]


@functools.lru_cache(maxsize=None)
def expected(case, n, calls):
    """what the oracle holds after each call: (bits of the call, counters, state, FEC results so far) -- computed once per stream and
    schedule, shared, left unchanged"""
    iq = samples_of(case, n)
    o = O.Bpsk(blen=4)
    out, pos, nb = [], 0, 0
    for L in calls:
        o.receive_i16(iq[2 * pos:2 * (pos + L)])
        pos += L
        bits = o.bits()
        out.append((bits[nb:].copy(), o.counters(), o.state().copy(), [(rc, bi, dat.tobytes()) for rc, bi, dat in o.fec_results()]))
        nb = bits.size
    assert pos == n
    return out


def run(cases, n, calls):
    """the cases as the streams of one handle, in order -> the handle"""
    calls = tuple(calls)
    S = len(cases)
    want = [expected(c, n, calls) for c in cases]
    d = J.Bpsk(nstreams=S, max_batch_samples=max(calls))
    d_iq = J.DeviceBuffer.from_host(np.concatenate([samples_of(c, n) for c in cases]))
    pos = 0
    nbits, nfec = [0] * S, [0] * S
    for k, L in enumerate(calls):
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        for s in range(S):
            where = (P.name_of(cases[s]), "stream", s, "call", k, "input samples", pos, L)
            bits, counters, state, fec = want[s][k]
            got = d.bits(s)
            assert got.tobytes() == bits.tobytes(), (where, "bits", got.size, bits.size)
            same_counters(d.counters(s), counters)
            gs = d.state(s)
            same_state(gs, state)
            assert gs[list(STATE)].tobytes() == state[list(STATE)].tobytes(), (where, "state", gs, state)
            # (the library counts the trigger bit within the call, the oracle within the stream)
            gf = [(rc, nbits[s] + bi, dat.tobytes()) for rc, bi, dat in d.fec_results(s)]
            assert gf == fec[nfec[s]:], (where, "fec", [f[:2] for f in gf], [f[:2] for f in fec[nfec[s]:]])
            nbits[s] += bits.size
            nfec[s] = len(fec)
        pos += L
    assert pos == n and d.tail_kernel_name() == TAIL
    return d


# ---------------------------------------------------------------------------------------------------------------- locked
@pytest.mark.parametrize("S", [8, 9])
def test_locked_at_every_bit_position_calls_at_every_bit_position(S):
    cases = (P.DELAYED + [P.NINTH_LOCKED])[:S]
    run(cases, P.N_LOCKED, P.locked_calls())
    # (every stream sliced a bit at nearly every one of its 1280 bit clocks: the calls above ran on locked streams)
    for s, c in enumerate(cases):
        assert expected(c, P.N_LOCKED, tuple(P.locked_calls()))[-1][1]["cntBit"] > 1200, s


# ---------------------------------------------------------------------------------------------------------------- every move
@pytest.mark.parametrize("schedule", ["one_call", "seams"])
def test_every_move_of_the_peak(schedule):
    calls = [P.N_WALK] if schedule == "one_call" else P.seam_calls([tuple(x) for x in P.load()["seams"]], P.N_WALK)
    run(P.WALKS, P.N_WALK, calls)


# ---------------------------------------------------------------------------------------------------------------- mixed waves
@pytest.mark.parametrize("group", [0, 3, 7])
def test_one_wandering_stream_in_a_wave_of_locked_ones(group):
    cases = list(P.DELAYED)
    cases[group] = P.MIXED_WALK
    run(cases, P.N_LOCKED, P.mixed_calls())


# ---------------------------------------------------------------------------------------------------------------- each kernel
def child(env, least):
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__), "-k", "not child_process"],
                       env=dict(os.environ, JSDR_KNOBS="1", **env), capture_output=True, text=True, timeout=300)
    m = re.search(r"(\d+) passed", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) >= least and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_once_more_through_k_tail8_in_four_wave_workgroups_in_a_child_process():
    child(dict(JSDR_TAIL8="2"), 7)


def test_once_more_through_k_tail8_in_one_wave_workgroups_in_a_child_process():
    child(dict(JSDR_TAIL8="2", JSDR_TAIL8_WPB="1"), 7)
