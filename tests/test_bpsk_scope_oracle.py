"""The BPSK scope without a device: tests/bpsk_scope.py's restatement (rows placed by the header's geometry from the C oracle's
instruments) against its literal transliteration of FUNcubeBPSKDemod.java (rings stepped sample by sample, the painter's loops)
on every case, bit for bit; the geometry on a grid of (rate, n); Java's cast and the Infinity / NaN paths of xs, ys, rs; and the
census that keeps the cases meaningful, held against tests/golden/bpsk_scope_census.json."""
import numpy as np
import pytest

import bpsk_scope as B

F64 = np.float64


@pytest.mark.parametrize("case", list(B.CASES))
def test_restatement_equals_the_java_text(case):
    c = B.CASES[case]
    r, lit, lrows = B.run_case(case, literal=True)
    rows = r.rows(0, c["frames"])
    for f in range(c["frames"]):
        bad = B.rows_equal({k: rows[k][f] for k in B.OUTPUTS}, lrows[f])
        assert not bad, (case, "frame", f, bad)
    assert lit.cntBit == r.o.counters()["cntBit"], case
    assert rows["tuned"].shape == (c["frames"], c["n"], 2) and rows["pts"].shape == (c["frames"], r.L, 4)


def test_restatement_equals_the_java_text_across_a_setup_and_a_retune():
    """setup() clears the rings and their indices and leaves the demodulator alone: the origin moves, and the restatement places
    the oracle's stream from there.  actionPerformed changes tuPhaseInc: the oracle has no actions, so from there on its (fi, fq)
    are another stream's and the tuned rows alone are held to the Java text (the GPU test holds the rest to it)"""
    rate, n = 96000, 2048
    form, data = B.case_input("96k", 1)
    x = B.as_float(form, data)
    r = B.Restated(rate, n, 12000, 8)
    t = B.Tuner(12000, rate)
    lit = B.Literal(rate, n, 12000)
    origin = 0
    for f in range(8):
        if f == 2:
            lit.setup(12000)
            origin = (f * n) // (rate // 9600)
        if f == 5:
            t.set(11990.0)
            lit.action(11990.0)
        buf = x[2 * f * n:2 * (f + 1) * n]
        r.receive(buf, t.step(n))
        lit.receive(buf)
        got = {k: v[0] for k, v in r.rows(f, 1, origin).items()}
        want = lit.rows()
        assert B.same(got["tuned"], want["tuned"]), f
        if f < 5:
            assert not B.rows_equal(got, want), f
        # ... and the restatement's placement over the Java text's own instruments, through the retune as well
        D = rate // 9600
        again = B.rows_of(r.L, (f * n) // D, ((f + 1) * n) // D, origin, *lit.logs(), want["tuned"])
        assert not B.rows_equal(again, want), f
    assert origin == 409 and origin % B.ring_len(rate, n) != 0  # the origin turns the slots


def test_geometry_on_a_grid():
    """every rate >= 9600 refills the rings in every frame; G_f counts what RxDownSample's counter lets through"""
    for rate in (9600, 11025, 19200, 22050, 44100, 48000, 88200, 96000, 176400, 192000, 250000):
        D = rate // 9600
        for n in list(range(1, 300)) + [1024, 2048, 2049, 4410, 4800, 9600, 19200]:
            L = B.ring_len(rate, n)
            G = B.g_first(rate, n, 7 * n, 9)
            assert (np.diff(G) >= L).all(), (rate, n)
            cnt, outs = (7 * n) % D, []  # dsCnt at the call's start (:476), then sample by sample
            for f in range(3):
                k = 0
                for _ in range(n):
                    cnt += 1
                    if cnt >= D:
                        cnt, k = 0, k + 1
                outs.append(k)
            assert outs == list(np.diff(G)[:3]), (rate, n)
    assert B.ring_len(96000, 2048) == 204 and B.ring_len(44100, 4410) == 960 and B.ring_len(48000, 4800) == 960
    assert list(B.g_first(96000, 2048, 2048 * 5, 2, origin=1000)) == [24, 228, 433]


def test_javas_cast():
    x = np.array([0.0, -0.0, 0.9, -0.9, 1.5, -1.5, 2147483646.9, 2147483647.0, 2147483648.5, -2147483648.0, -2147483649.0, 1e300,
                  -1e300, np.inf, -np.inf, np.nan], F64)
    want = [0, 0, 0, 0, 1, -1, 2147483646, 2147483647, 2147483647, -2147483648, -2147483648, 2147483647, -2147483648, 2147483647,
            -2147483648, 0]
    assert B.jint(x).tolist() == want


def test_the_painters_infinity_and_nan_paths():
    L = 8
    zero = np.zeros((L, 2), F64)
    mx, pts = B.painter(zero, np.zeros(L))
    assert mx.tolist() == [0.0, 0.0] and not pts.any()  # xs = Infinity, 0 * Infinity = NaN -> 0
    iq = zero.copy()
    iq[3] = (0.0, 5.0)  # mi == 0 alone: Q * xs = Infinity saturates, rs = 50 / 0 = Infinity
    re = np.zeros(L)
    re[3], re[4] = -2.0, 0.0
    mx, pts = B.painter(iq, re)
    assert mx.tolist() == [0.0, 5.0]
    assert pts[3].tolist() == [0, 100, B.INT_MAX, B.INT_MIN] and pts[4].tolist() == [0, 0, 0, 0]
    iq = np.array([[1.0, -2.0], [np.nan, 4.0], [-3.0, np.nan]] + [[0.0, 0.0]] * 5, F64)
    mx, pts = B.painter(iq, np.zeros(L))
    assert mx.tolist() == [3.0, 4.0]  # a NaN never wins
    assert pts[:3].tolist() == [[33, -50, -66, 0], [0, 100, 133, 0], [-100, 0, 0, 0]]
    lit = B.Literal(96000, 2048, 12000)
    lit.demodIQ[:6] = iq[:3].ravel()
    mx2, pts2 = lit.paint()
    assert B.same(mx, mx2) and np.array_equal(pts2[:3], pts[:3])


def test_the_census_is_the_committed_one_and_the_cases_hold_what_they_are_for():
    c = B.census()
    assert c == B.load_census()
    assert c["96k"]["L"] == 204 and c["96k"]["outputs"] == [204, 205]
    assert c["44k1"]["L"] == 960 and c["44k1"]["L"] % 8 == 0 and c["44k1"]["outputs"] == [1102, 1103]
    assert c["44k1"]["slots_marked_twice"] >= 1
    assert c["48k"]["outputs"] == [c["48k"]["L"]] == [960]
    assert c["silence"]["frames_without_a_bit"] == c["silence"]["frames_with_mi_zero"] == B.CASES["silence"]["frames"]
    assert c["96k"]["frames_in_which_peak_pos_moved"] >= 1
    assert c["fec"]["fec_decoded"] >= 1
    assert c["tiny_i"]["pts_saturated"] >= 1
    assert c["nan"]["nan_slots"] >= 1
    assert c["untuned"]["bits"] >= 1


def test_a_slot_marked_twice_keeps_the_later_bit():
    r, _, _ = B.run_case("44k1")
    dec_g, dec = r.o.declog_pos()
    n, D, L = r.n, r.D, r.L
    rows = r.rows(0, B.CASES["44k1"]["frames"])
    seen = 0
    for f in range(B.CASES["44k1"]["frames"]):
        lo, hi = np.searchsorted(dec_g, [(f * n) // D, ((f + 1) * n) // D])
        g = dec_g[lo:hi][dec[lo:hi, 1] > 100.0]
        di = dec[lo:hi, 0][dec[lo:hi, 1] > 100.0]
        slots = (g + 1) % L
        for s in set(slots.tolist()):
            k = np.flatnonzero(slots == s)
            if k.size > 1:
                seen += 1
                assert rows["bits"][f][s] == (1 if di[k[-1]] < 0 else -1)
                assert rows["pts"][f][s][3] == B.jint(di[k[-1]] * (50.0 / (rows["max"][f][0] * rows["max"][f][1])))
    assert seen >= 1
