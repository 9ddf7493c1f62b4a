"""The fast BPSK variant on engineered slicer ties (tests/golden/fast_tie_fixtures.npz, tests/fast_ties.py), at the margins
the product runs with: no JSDR_FAST_* knob anywhere in this file.

On these streams the sign of di at the engineered decisions is the sign of the reference's own rounding, so the fast kernels'
(fi, fq) -- FMA-contracted, another rounding -- take other bits on a good part of them (test_..._can_tell counts how many).
The delivered bits equal the oracle's only if k_tail<true> notices the decision inside its margin and redoes it from the raw
input in the reference's exact order (tail_exact_sample: tuner, 27 taps, VCO, 65 taps in ring-slot order), at every
decimation, with and without DC correction and tuner, wherever the decision falls in a call -- or withholds the stream where
it cannot.  The reference is always the C oracle.
"""
import sys
import os

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O
import fast_ties as T

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from fixture_cases import STREAMS, stream_input  # noqa: E402

pytestmark = pytest.mark.gpu
FX = np.load(T.FIXTURE)
_streams = {}


def stream(fam):
    if fam not in _streams:
        _streams[fam] = T.patched_stream(fam, FX)
    return _streams[fam]


def oracle_calls(p, raw, cuts, n):
    """the oracle over the calls [cuts[i], cuts[i+1]): per call (bits, fec results), and the object after the last"""
    o = O.Bpsk(rate=p["rate"], blen=4, tuning=p["tuning"])  # frames of one sample: a call of any length
    per, nb, nf = [], 0, 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        o.receive_i16(raw[2 * a:2 * b], p["ic"], p["qc"])
        bits, fec = o.bits(), o.fec_results()
        per.append((bits[nb:].copy(), fec[nf:]))
        nb, nf = len(bits), len(fec)
    return per, o


def assert_call_equals(d, s, want, what):
    bits, fec = want
    assert np.array_equal(d.bits(s), bits), what
    got = d.fec_results(s)
    assert len(got) == len(fec) and all(a[0] == b[0] and np.array_equal(a[2], b[2]) for a, b in zip(got, fec)), what


def assert_counters_equal(d, s, o, what):
    c, oc = d.counters(s), o.counters()
    assert [c[k] for k in T.CKEYS] == [oc[k] for k in T.CKEYS], (what, c, oc)


# ------------------------------------------------------------------------------ where a decision falls in a call, by arithmetic
def place(g, gp, cuts_g):
    """the place of the decision at 9600 Hz sample g (predecessor gp) among the calls that start at the 9600 Hz samples cuts_g[:-1]
    and end at cuts_g[1:], as k_tail walks them: chunks of 64 bit periods from the period the call starts in"""
    i = int(np.searchsorted(cuts_g, g, side="right")) - 1
    G, G2 = cuts_g[i], cuts_g[i + 1]
    if gp - 64 - G < 7 or g - 64 - G < 7:
        return {"cannot"}  # a window reaches into the previous call (or the decision is a stream's first)
    m_first = G >> 3
    q, q_last = ((g >> 3) - m_first) // 64, (((G2 - 1) >> 3) - m_first) // 64
    start = 8 * (m_first + 64 * q)
    where = set()
    if q == 0 and q_last > 0:
        where.add("first")        # the first chunk of a call of several, 72 or more samples in
    if q == q_last and q > 0 and start + 512 > G2:
        where.add("last")         # the last, partial chunk
    if q > 0 and gp < start:
        where.add("chunk_first")  # the chunk's first decision: its predecessor is the carried last_g
    if 0 < q < q_last and gp >= start:
        where.add("interior")
    return where


# At 12 kHz / 192 kHz the tuner's table index has one irregular step (sample 266: 16 steps of 2 pi / 16 in double do not land on
# a table boundary the same way every time) before it settles into its 16-cycle, so a call that holds the stream's first 300
# samples finds no period and cannot redo; every later call can.  The plans of that family start with a short call of their own.
LEAD = {"c": 104}


def plans(fam):
    """cut lists (9600 Hz samples) that put engineered decisions of the family in each of the four places; every one is checked
    to leave no engineered decision where it cannot be redone"""
    g, gp = [int(v) for v in FX[fam + "_g"]], [int(v) for v in FX[fam + "_gp"]]
    nds = T.FAMILIES[fam]["n"] // (T.FAMILIES[fam]["rate"] // 9600)
    whole = [0, LEAD[fam], nds] if fam in LEAD else [0, nds]
    out = {"interior": whole}
    # (first, last: calls of more than a chunk, so that the first chunk is not the last one)
    for name, cut_of, shortest in (("first", lambda x, k: x - 80, 600), ("last", lambda x, k: x + 3, 600),
                                   ("chunk_first", lambda x, k: 8 * ((x >> 3) - 64 * k), 100)):
        cuts = list(whole)
        for x, xp in zip(g, gp):
            for k in (1, 2, 3):
                c = cut_of(x, k)
                trial = sorted(set(cuts + [c]))
                if c <= whole[-2] or c >= nds or min(np.diff(trial[len(whole) - 2:])) < shortest:
                    continue
                if any("cannot" in place(a, b, trial) for a, b in zip(g, gp)) or name not in place(x, xp, trial):
                    continue
                cuts = trial
                break
        out[name] = cuts
    return out


def run_plan(fam, cuts_g, nstreams=1, pad=0):
    """the fast handle over the calls of the plan; returns the handle after the last call (every call compared with the oracle)"""
    p = T.FAMILIES[fam]
    raw, n, D = stream(fam), p["n"], p["rate"] // 9600
    cuts = [D * c for c in cuts_g[:-1]] + [n]
    stride = 2 * n + pad
    host = np.full(nstreams * stride, 12345, np.int16)  # (the padding holds loud samples: reading them would show)
    for s in range(nstreams):
        host[s * stride:s * stride + 2 * n] = raw
    d = J.Bpsk(rate=p["rate"], blen=8192, tuning=p["tuning"], nstreams=nstreams, max_batch_samples=max(np.diff(cuts)), variant="fast")
    d_in = J.DeviceBuffer.from_host(host)
    per, o = oracle_calls(p, raw, cuts, n)
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        d.batch_i16(d_in.ptr + 4 * a, stride, b - a, p["ic"], p["qc"])
        assert d.uncertified_streams() == [], (fam, cuts_g, i)
        for s in range(nstreams):
            assert_call_equals(d, s, per[i], (fam, cuts_g, i, s))
    for s in range(nstreams):
        assert_counters_equal(d, s, o, (fam, cuts_g, s))
    return d


@pytest.mark.parametrize("fam", T.REDOABLE)
def test_fast_variant_redoes_engineered_ties_at_natural_margins_wherever_they_fall(fam):
    g, gp = [int(v) for v in FX[fam + "_g"]], [int(v) for v in FX[fam + "_gp"]]
    seen = set()
    for name, cuts in plans(fam).items():
        where = set().union(*[place(a, b, cuts) for a, b in zip(g, gp)])
        assert "cannot" not in where and name in where, (fam, name, cuts, where)
        seen |= where
        d = run_plan(fam, cuts)
        st = d.cert_stats()
        assert st["streams_uncertified"] == 0
        assert st["decisions_redone_exactly"] >= len(g), (fam, name, st)
    assert {"interior", "first", "last", "chunk_first"} <= seen, (fam, seen)


def test_fast_variant_redoes_engineered_ties_at_a_padded_stride():
    d = run_plan("b", plans("b")["first"], nstreams=3, pad=38)
    assert d.cert_stats()["decisions_redone_exactly"] >= 3 * len(FX["b_g"])


def test_the_fixture_can_tell_fast_values_alone_give_other_bits():
    """di of the engineered decisions from the fast handle's OWN (fi, fq) trace, with the kernel's expression: at least twelve
    have the other sign than the oracle's (measured on an MI355X: see DESIGN.md) -- the fast values alone would have delivered
    other bits, so the equality the tests above find is the redo's doing."""
    flips = total = 0
    for fam in T.REDOABLE:
        p = T.FAMILIES[fam]
        d = J.Bpsk(rate=p["rate"], blen=8192, tuning=p["tuning"], nstreams=1, max_batch_samples=p["n"], variant="fast")
        d_in = J.DeviceBuffer.from_host(stream(fam))
        lead = LEAD.get(fam, 0)  # (the call that finds no tuner period runs another front end: not the values in question)
        if lead:
            d.batch_i16(d_in, 2 * p["n"], lead * (p["rate"] // 9600), p["ic"], p["qc"])
        n0 = lead * (p["rate"] // 9600)
        d.batch_i16(d_in.ptr + 4 * n0, 2 * p["n"], p["n"] - n0, p["ic"], p["qc"])
        tr = d.trace(0)
        assert len(tr) == p["n"] // (p["rate"] // 9600) - lead
        fam_flips = 0
        for g, gp, di in zip(FX[fam + "_g"], FX[fam + "_gp"], FX[fam + "_di"]):
            fast = T.kernel_di(tr[gp - lead], tr[g - lead])
            fam_flips += int((fast < 0.0) != (di < 0.0))
        print("family %s: %d of %d engineered decisions flip on the fast (fi, fq)" % (fam, fam_flips, len(FX[fam + "_g"])))
        flips += fam_flips
        total += len(FX[fam + "_g"])
    print("fast values alone: %d of %d engineered decisions take the other bit" % (flips, total))
    assert flips >= 12, (flips, total)


# ------------------------------------------------------------------------------ cannot redo: must flag
def _cannot_case(fam, cut_g, label):
    """stream 0: the family's patched stream, stream 1: an untouched natural stream; calls [0, cut), [cut, mid), then recovery,
    then [mid, n)"""
    p = T.FAMILIES[fam]
    n, D = p["n"], p["rate"] // 9600
    raw = stream(fam)
    natural = {96000: "clean", 192000: "r192k"}[p["rate"]]
    clean = stream_input(natural)[:2 * n]
    assert STREAMS[natural]["rate"] == p["rate"] and p["ic"] == 0 and p["qc"] == 0
    mid = n - 4096
    cuts = sorted({0, mid, n} | ({D * cut_g} if cut_g is not None else set()))
    d = J.Bpsk(rate=p["rate"], blen=8192, tuning=p["tuning"], nstreams=2, max_batch_samples=max(np.diff(cuts)), variant="fast")
    d_in = J.DeviceBuffer.from_host(np.concatenate([raw, clean]))
    per0, o0 = oracle_calls(p, raw, cuts, n)
    per1, o1 = oracle_calls(p, clean, cuts, n)
    ptrs = [d_in.ptr + 4 * a for a in cuts[:-1]]
    lens = [int(b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    last = len(lens) - 1
    for i in range(last):
        d.batch_i16(ptrs[i], 2 * n, lens[i])
    assert d.uncertified_streams() == [0] and d.cert_stats()["streams_uncertified"] == 1, label
    for getter in (d.bits, d.fec_results, d.decoded, d.counters):
        with pytest.raises(J.JsdrError):
            getter(0)
    assert_call_equals(d, 1, per1[last - 1], label)  # the natural stream beside it is delivered
    assert d.recover_uncertified(ptrs[:last], lens[:last], 2 * n) == 1
    assert d.uncertified_streams() == []
    assert_call_equals(d, 0, per0[last - 1], label)
    d.batch_i16(ptrs[last], 2 * n, lens[last])  # the call after it stays exact
    assert d.uncertified_streams() == []
    assert_call_equals(d, 0, per0[last], label)
    assert_call_equals(d, 1, per1[last], label)
    assert_counters_equal(d, 0, o0, label)
    assert_counters_equal(d, 1, o1, label)
    assert d.state(0).tobytes() == o0.state().tobytes(), label


@pytest.mark.parametrize("fam", ["a", "d"])
def test_fast_variant_flags_a_tie_whose_window_reaches_into_the_previous_call(fam):
    g, gp = int(FX[fam + "_g"][3]), int(FX[fam + "_gp"][3])
    cut = g - 30  # the decision 30 samples into the call: its own window and its predecessor's lie in the call before
    nds = T.FAMILIES[fam]["n"] // 10
    assert place(g, gp, [0, cut, nds]) == {"cannot"}
    _cannot_case(fam, cut, (fam, cut))


def test_fast_variant_flags_a_tie_under_a_tuning_without_a_period():
    assert len(FX["f_g"]) >= 4
    _cannot_case("f", None, "f")


def test_fast_variant_flags_a_tie_in_the_call_that_holds_the_head_of_a_192_kHz_stream():
    """the limit LEAD steps round, pinned as it is: that call finds no tuner period, so its ties are withheld and recovered"""
    _cannot_case("c", None, "c")


# ------------------------------------------------------------------------------ soundness sweep
def _sweep_streams():
    """256 streams of 16 384 samples at 96 kHz: amplitudes 30 .. 30 000, noise sigma 0 .. 6000, 79.9 .. 80.1 samples a symbol
    (synthesised at ten times the rate with 799 / 801 samples a symbol and every tenth sample kept: the peak walks), and a loud
    burst ahead of a quiet signal (the sticky emax / amax widen the margins of everything after it)"""
    S, L = 256, 16384
    pay = np.stack([O.synth_payload(20021207, 0, f) for f in range(2)])
    dsign = O.synth_diffsign(np.concatenate([O.fec_encode(pay[f]) for f in range(2)]), 1)
    out = np.empty((S, 2 * L), np.int16)
    for s in range(S):
        amp = int(round(30.0 * 1000.0 ** ((s % 16) / 15.0)))
        sigma = 6000.0 * ((s // 16) % 4) / 3.0
        kind = s // 64  # 0: plain, 1: 79.9, 2: 80.1 samples a symbol, 3: loud burst, then this
        key = O.mix64((20021207 * 0x9E3779B1 + s) ^ 0xA5A5A5A5)
        gain = int(round(sigma / 37837.0 * 32768.0))
        ct, st = O.synth_tables(amp)
        if kind in (1, 2):
            x = O.synth_dbpsk(0, 10 * L, dsign, 799 if kind == 1 else 801, 0, O.phase_inc_u32(13200.0, 960000), ct, st, gain, key)
            out[s] = x.reshape(-1, 2)[::10].ravel()
        else:
            out[s] = O.synth_dbpsk(0, L, dsign, 80, 0, O.phase_inc_u32(13200.0, 96000), ct, st, gain, key)
            if kind == 3:
                lt, ls = O.synth_tables(30000)
                out[s, :2 * 2048] = O.synth_dbpsk(0, 2048, dsign, 80, 0, O.phase_inc_u32(13200.0, 96000), lt, ls, gain, key)
    return out


def test_fast_variant_is_sound_over_a_sweep_of_amplitudes_noise_and_symbol_rates():
    """every stream is either withheld or the oracle's in bits, counters and FEC results; at most 5 % are withheld"""
    iq = _sweep_streams()
    S, L = iq.shape[0], iq.shape[1] // 2
    d = J.Bpsk(nstreams=S, max_batch_samples=L, variant="fast")
    d.batch_i16(J.DeviceBuffer.from_host(iq), 2 * L, L)
    flagged = d.uncertified_streams()
    nbits = 0
    for s in range(S):
        if s in flagged:
            continue
        o = O.Bpsk(blen=4 * L)
        o.receive_i16(iq[s])
        assert np.array_equal(d.bits(s), o.bits()), s
        assert_counters_equal(d, s, o, s)
        fg, fo = d.fec_results(s), o.fec_results()
        assert len(fg) == len(fo) and all(a[0] == b[0] and np.array_equal(a[2], b[2]) for a, b in zip(fg, fo)), s
        nbits += len(o.bits())
    print("sweep: %d of %d streams withheld, %d bits compared, %d decisions redone" %
          (len(flagged), S, nbits, d.cert_stats()["decisions_redone_exactly"]))
    assert nbits > 20000  # the sweep does demodulate
    assert len(flagged) <= S * 5 // 100, flagged
