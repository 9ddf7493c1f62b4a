"""GPU: the sync stage of the BPSK path on engineered hits, in all three kernel forms (sync_cases.py has the inputs and the why;
test_sync_cases_oracle.py counts, on the oracle alone, what they contain).

Ordinary tune-mode handles fed by batch_i16, one O.Bpsk per stream fed the same samples call by call.  After EVERY call and for
every stream: the call's bits, all counters (cntBit, cntFEC, cntDec, dmErrBits, dmCorr, dmMaxCorr, decodeOK), the state doubles
bit for bit, and the FEC results (count, rc, trigger bit, 256 bytes).  Every comparison is an equality.

  k_sync_t + k_sync_fin   all thirteen streams on one handle, under the one-call, the seam and the lengths schedule
  k_sync_t, fuse = 1      the streams of each family on one-stream handles, calls of at most 163 840 samples; the order family
                          once more in a single call, which one stream takes unfused
  k_sync + k_sync_fin     all streams on a handle created for calls so long that the transposed image outgrows its LDS, fed
                          the seam schedule's short calls: the shipped fallback, with no knob set

Child processes run the file again with JSDR_SYNC_T=0 (the fallback everywhere), JSDR_TAIL8=2 (k_tail8 carries the 5200-bit
register over in dwords) and JSDR_VITQ=1 (k_fec_bits gathers the window instead of k_fec_bpsk).  Every test asserts, from the
handle's launch counts, which sync kernels served it.

Checked by hand (scratch builds, not committed): `>= 45` as `> 45` in sync_fin_wave fails every test but the neighbours family's
one-stream handles (whose hits are all 65); `== 1` as `>= 0` in k_fec_bits -- in both of its ballots, or in the trellis words
alone -- fails the three all-family tests under JSDR_VITQ=1, on the early frame, which decodes only with the register's zeros
as 0x40."""
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
from test_gpu_bpsk import same_counters, same_state

pytestmark = pytest.mark.gpu

SYNC_T = os.environ.get("JSDR_SYNC_T") != "0"
TAIL = "k_tail8" if os.environ.get("JSDR_TAIL8") == "2" else "k_tail"
VITQ = os.environ.get("JSDR_VITQ") == "1"
STATE = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)  # (6, 7 belong to the FFT-acquire mode)


@functools.lru_cache(maxsize=None)
def expected(case, calls):
    """what the oracle holds after each call: (bits of the call, counters, state, FEC results so far) -- computed once per stream and
    schedule, shared, left unchanged"""
    iq = Y.stream_of(case)
    o = O.Bpsk(blen=4)
    out, pos, nb = [], 0, 0
    for L in calls:
        o.receive_i16(iq[2 * pos:2 * (pos + L)])
        pos += L
        bits = o.bits()
        out.append((bits[nb:].copy(), o.counters(), o.state().copy(), [(rc, bi, dat.tobytes()) for rc, bi, dat in o.fec_results()]))
        nb = bits.size
    assert pos == Y.N
    return out


def run(cases, calls, form, **handle):
    """the cases as the streams of one handle, in order, compared with the oracle after every call; form = the sync kernels that
    must have served every call: "fused" (k_sync_t alone), "t" (k_sync_t + k_sync_fin) or "strided" (k_sync + k_sync_fin)"""
    calls = tuple(int(L) for L in calls)
    S = len(cases)
    want = [expected(c, calls) for c in cases]
    handle.setdefault("max_batch_samples", max(calls))
    d = J.Bpsk(nstreams=S, **handle)
    d.profile_enable(True)
    d_iq = J.DeviceBuffer.from_host(np.concatenate([Y.stream_of(c) for c in cases]))
    try:
        pos = 0
        nbits, nfec = [0] * S, [0] * S
        for k, L in enumerate(calls):
            d.batch_i16(d_iq.ptr + 4 * pos, 2 * Y.N, L)
            for s in range(S):
                where = (Y.name_of(cases[s]), "stream", s, "call", k, "input samples", pos, L)
                bits, counters, state, fec = want[s][k]
                got = d.bits(s)
                assert got.tobytes() == bits.tobytes(), (where, "bits", got.size, bits.size)
                gc = d.counters(s)
                sync = ("cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK")
                assert [gc[n] for n in sync] == [counters[n] for n in sync], (where, sync, [gc[n] for n in sync], [counters[n] for n in sync])
                same_counters(gc, counters)  # (cntRaw and cntDS as well)
                gs = d.state(s)
                same_state(gs, state)
                assert gs[list(STATE)].tobytes() == state[list(STATE)].tobytes(), (where, "state", gs, state)
                # (the library counts the trigger bit within the call, the oracle within the stream)
                gf = [(rc, nbits[s] + bi, dat.tobytes()) for rc, bi, dat in d.fec_results(s)]
                assert gf == fec[nfec[s]:], (where, "fec", [f[:2] for f in gf], [f[:2] for f in fec[nfec[s]:]])
                nbits[s] += bits.size
                nfec[s] = len(fec)
            pos += L
        assert pos == Y.N and d.tail_kernel_name() == TAIL
        if S > 1:
            assert ("k_vitq" in d.fec_kernel_name()) == VITQ, d.fec_kernel_name()
        prof = d.profile_read()
        launches = {n: prof[n][1] for n in ("k_sync_t", "k_sync", "k_sync_fin")}
        if not SYNC_T:
            form = "strided"
        n = len(calls)
        assert launches == {"fused": dict(k_sync_t=n, k_sync=0, k_sync_fin=0), "t": dict(k_sync_t=n, k_sync=0, k_sync_fin=n),
                            "strided": dict(k_sync_t=0, k_sync=n, k_sync_fin=n)}[form], (form, n, launches)
    finally:
        d_iq.free()
    return d


# ---------------------------------------------------------------------------------------------------------------- k_sync_t + k_sync_fin
@pytest.mark.parametrize("schedule", ["one_call", "seams", "lengths"])
def test_every_family_on_one_handle(schedule):
    # (created for calls of the whole stream: a call of the neighbours streams holds up to twelve hits, which such a handle logs)
    run(Y.CASES, Y.schedule(schedule), "t", max_batch_samples=Y.N)


# ---------------------------------------------------------------------------------------------------------------- k_sync_t, fuse = 1
@pytest.mark.parametrize("family", ["threshold", "early", "neighbours", "order"])
def test_one_stream_handles_in_short_calls_the_fused_form(family):
    calls = Y.schedule("fused_" + family)
    assert max(calls) <= Y.FUSED_MAX
    for case in Y.family(family):
        run([case], calls, "fused")


def test_one_stream_in_a_single_long_call_is_not_fused():
    assert Y.N > Y.FUSED_MAX
    run(Y.family("order"), [Y.N], "t")


# ---------------------------------------------------------------------------------------------------------------- k_sync + k_sync_fin
def test_a_handle_too_large_for_the_transposed_image_takes_the_strided_kernel():
    big = Y.fallback_batch_samples()
    assert big == 6 << 20  # (about 5.7 M samples a call at 96 kHz, rounded up)
    cases = [c for c in Y.CASES if c[0] != "frames"]
    run(cases, Y.schedule("seams"), "strided", max_batch_samples=big)


# ---------------------------------------------------------------------------------------------------------------- each kernel
def child(env, least):
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__), "-k", "not child_process"],
                       env=dict(os.environ, JSDR_KNOBS="1", **env), capture_output=True, text=True, timeout=300)
    m = re.search(r"(\d+) passed", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) >= least and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_once_more_through_the_strided_k_sync_in_a_child_process():
    child(dict(JSDR_SYNC_T="0"), 9)


def test_once_more_through_k_tail8_in_a_child_process():
    child(dict(JSDR_TAIL8="2"), 9)


def test_once_more_through_k_fec_bits_in_a_child_process():
    child(dict(JSDR_VITQ="1"), 9)
