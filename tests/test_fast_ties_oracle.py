"""tests/golden/fast_tie_fixtures.npz against the C oracle (CPU only): the engineered ties are what the fixture says they are,
and they have the power the GPU tests rely on -- another order of summation takes other decisions on them.
tests/fast_ties.py explains the construction, tests/golden/make_fast_tie_fixtures.py builds the file."""
import functools
import os

import numpy as np
import pytest

import fast_ties as T

FX = np.load(T.FIXTURE)
FAMS = list(T.FAMILIES)


@functools.lru_cache(maxsize=None)
def run(fam):
    raw = T.patched_stream(fam, FX)
    return raw, T.run_oracle(fam, raw)


@functools.lru_cache(maxsize=None)
def chain(fam):
    return T.Chain(fam)


def grades(fam):
    """(inside, true tie) per engineered decision, from the oracle's own run and the exact rational di"""
    raw, r = run(fam)
    ch = chain(fam)
    k = FX[fam + "_dec"]
    inside = (np.abs(r["di"][k]) <= T.INSIDE_REL * r["e2"][k]) & (r["e2"][k] > 1e4)
    exact = np.array([float(ch.exact_di(raw, int(r["g"][t]), *r["trace"][int(r["g"][t - 1])])) for t in k])
    return inside, inside & (np.abs(exact) <= T.TIE_ABS), exact


@pytest.mark.parametrize("fam", FAMS)
def test_patched_streams_reproduce_their_sha256(fam):
    p = T.FAMILIES[fam]
    assert [int(v) for v in FX[fam + "_params"]] == [p["rate"], p["tuning"], p["ic"], p["qc"], p["n"], p["seed"], p["stream"], T.AMP]
    assert [float(v) for v in FX[fam + "_carrier_noise"]] == [p["carrier"], p["noise_sigma"]]
    raw, _ = run(fam)
    assert T.sha(raw) == str(FX[fam + "_sha256"])
    assert 20000 <= raw.size // 2 <= 40000


@pytest.mark.parametrize("fam", FAMS)
def test_oracle_reproduces_every_recorded_decision_bit_for_bit(fam):
    _, r = run(fam)
    k = FX[fam + "_dec"]
    assert np.array_equal(r["g"][k], FX[fam + "_g"]) and np.array_equal(r["g"][k - 1], FX[fam + "_gp"])
    assert r["di"][k].tobytes() == FX[fam + "_di"].tobytes()
    assert r["e2"][k].tobytes() == FX[fam + "_e2"].tobytes()
    assert np.all(np.diff(FX[fam + "_g"]) >= 12 * 8)  # 12 symbols apart: no decision's patches reach an earlier one


@pytest.mark.parametrize("fam", FAMS)
def test_recorded_exact_di_is_the_rational_value(fam):
    _, _, exact = grades(fam)
    assert exact.tobytes() == FX[fam + "_exact_di"].tobytes()


def test_declog_pos_agrees_with_declog_and_the_trace():
    """the oracle addition itself: g is the 9600 Hz sample the detector read, (di, energy2) are declog(0)'s"""
    _, r = run("a")
    o = r["o"]
    assert np.array_equal(o.declog(0), np.stack([r["di"], r["e2"]], axis=1))
    g, tr = r["g"], r["trace"]
    assert np.all(np.diff(g) > 0) and g[-1] < len(tr)
    k = np.arange(1, len(g))
    di = -(tr[g[k - 1], 0] * tr[g[k], 0] + tr[g[k - 1], 1] * tr[g[k], 1])
    assert di.tobytes() == r["di"][k].tobytes()


def test_grades_and_counts():
    n_all = n_tie = 0
    for fam in FAMS:
        inside, tie, _ = grades(fam)
        assert np.all(FX[fam + "_e2"] > 1e4)
        assert inside.all(), (fam, "every engineered decision is at least of grade inside")
        n_all += inside.size
        n_tie += int(tie.sum())
        if fam in T.REDOABLE:
            assert inside.size >= 6, fam
        else:
            assert inside.size >= 4, fam
    assert n_all >= 48 and n_tie >= 24, (n_all, n_tie)


def test_power_another_summation_order_decides_otherwise():
    """Each true tie's two detector samples recomputed from the down-sampler's outputs with the restated VCO index, the matched
    filter in ascending-age order, numpy doubles: the same real number, another rounding.  At least twelve of them take the
    other bit (twelve: a redo that summed in this order would pass the GPU test by chance with probability 2^-12 at most).
    The same recomputation in the reference's ring-slot order reproduces the oracle's di bit for bit."""
    flips = ties = 0
    for fam in FAMS:
        _, r = run(fam)
        ch = chain(fam)
        _, tie, _ = grades(fam)
        for t in FX[fam + "_dec"][tie]:
            g, gp = int(r["g"][t]), int(r["g"][t - 1])
            ring = T.kernel_di(T.ring_order_fifq(r["trace_ds"], ch.kv, gp), T.ring_order_fifq(r["trace_ds"], ch.kv, g))
            assert ring == r["di"][t], (fam, t)
            age = T.kernel_di(T.age_order_fifq(r["trace_ds"], ch.kv, gp), T.age_order_fifq(r["trace_ds"], ch.kv, g))
            ties += 1
            flips += int((age < 0.0) != (r["di"][t] < 0.0))
    print("true ties %d, decided otherwise in ascending-age order: %d" % (ties, flips))
    assert flips >= 12, (flips, ties)
