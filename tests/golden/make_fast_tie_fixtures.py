"""Generator of tests/golden/fast_tie_fixtures.npz: input streams whose slicer decisions are ties (tests/fast_ties.py has the why).
Deterministic, CPU only (numpy, fractions, the C oracle); under a minute on six cores.  Run from the repository root:

    python tests/golden/make_fast_tie_fixtures.py

Per family of fast_ties.FAMILIES, on the O.make_dbpsk_stream base, decisions are engineered one after the other in time order:
  choose  among the detector instants with energy2 > 1e5 past the acquisition (g >= 640), the ones with the smallest |di|, at
          least 12 symbols apart and from the stream's end;
  exact   the rational coefficients of every input sample in (fi, fq) of the decision (fast_ties.Chain), and with the oracle's
          dmLastIQ doubles the real-number di of the stream as it stands;
  wide    Newton steps on the samples of both detector windows until the free samples can finish (see approach());
  coarse  the minimum-norm change of the FREE samples (those no earlier decision's window reaches: 8 symbols' worth, both rails)
          that cancels di, rounded to LSBs; then greedy +-1 steps down to |di| of a few hundredths;
  fine    a meet-in-the-middle over -1/0/+1 LSB on 2 x 13 more slots (3^26 = 2.5e12 combinations, sums in double, their error
          1e-14): the best few by the estimate are evaluated exactly and the smallest |exact di| is taken -- typically 1e-11;
  check   the oracle runs the patched stream: the decision and every earlier one sit where they sat (same g), earlier engineered
          decisions keep their (di, energy2) bit for bit.
What is stored: base parameters and sha256, the patched stream's sha256, the patches (sample, rail, delta), and per engineered
decision its index among the detector instants, g, the predecessor's g, the oracle's di and energy2, and the exact rational di
rounded to double.

The grades (fast_ties.INSIDE_REL, fast_ties.TIE_ABS): inside = |di| <= 1e-10 * energy2 in the oracle's double; true tie = |exact
rational di| <= 1e-10.  Measured basis of that threshold, printed by this script over the 61 engineered decisions: the oracle's
double di differs from the exact di by 9.4e-10 in the median (lower decile 2.7e-11, largest 1.1e-8) -- its own rounding, which
therefore sets the sign of a real number nine times smaller; the exact di reached is 3.6e-12 in the median, 4.6e-11 at worst.
"""
import multiprocessing
import os
import sys
import time
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fast_ties as T  # noqa: E402

G_MIN = 640          # past the acquisition, and past the first 512-sample chunk of a one-call run
SPACING = 12 * 8     # 9600 Hz samples between engineered decisions
MAX_DELTA = 400      # LSBs a coarse patch may move one sample (amplitude 3000)
NMITM = 13
E2_MIN = 1e5         # energy2 an engineered decision keeps (the grades ask for 1e4)


def x_of(v, c):
    return Fraction(float(T.convert(v, c)))


def approach(ch, fam, raw, run, k):
    """the wide step: di = -(last . cur) is bilinear in the samples that BOTH detector samples' windows hold, and those weigh a
    hundred times more than the free ones (which only the matched filter's outermost taps see).  Newton steps on the double
    gradient over every sample of the two windows, each rounded to LSBs and re-run through the oracle, bring |di| to where the
    free samples can take over with changes of MAX_DELTA / 2; none of these samples is in the window of a decision 12 symbols
    earlier.  Returns the new oracle run."""
    g, gp = int(run["g"][k]), int(run["g"][k - 1])
    cC, cP = ch.coeffs(g), ch.coeffs(gp)
    ns = sorted(set(cC) | set(cP))
    zero = [Fraction(0), Fraction(0)]
    cc = np.array([[float(v) for v in cC.get(n, zero)] for n in ns]) / 32767.0
    cp = np.array([[float(v) for v in cP.get(n, zero)] for n in ns]) / 32767.0
    idx = 2 * np.array(ns)
    free = np.array([n in set(ch.free_samples(g, gp)) for n in ns])

    def need():
        """LSBs the coarse step on the free samples would move its heaviest sample by, as things stand"""
        w = -(run["trace"][gp][None, :] * cc[free]).ravel()
        return abs(run["di"][k]) * np.abs(w).max() / float(w @ w)

    for it in range(12):
        if need() <= MAX_DELTA / 2:
            break
        di = run["di"][k]
        last, cur = run["trace"][gp], run["trace"][g]
        grad = -(cp * cur[None, :] + last[None, :] * cc)  # [sample][rail], per LSB
        # every second round on lighter samples only: the rounding to LSBs leaves a smaller residue
        grad = np.where(np.abs(grad) <= np.quantile(np.abs(grad), 0.5 ** (it // 2)), grad, 0.0)
        d = np.rint(-di * grad / float((grad * grad).sum())).astype(np.int64)
        assert np.abs(d).max() <= MAX_DELTA, (g, di, np.abs(d).max())
        for r in (0, 1):
            raw[idx + r] = (raw[idx + r].astype(np.int64) + d[:, r]).astype(np.int16)
        run = T.run_oracle(fam, raw)
        assert int(run["g"][k]) == g and int(run["g"][k - 1]) == gp
    assert need() <= MAX_DELTA / 2, (g, run["di"][k], need())
    return run


def engineer_one(ch, raw, run, k, log):
    """patch raw (in place) so that detector instant k becomes a tie; returns the exact di reached"""
    p = ch.p
    g, gp = int(run["g"][k]), int(run["g"][k - 1])
    lastI, lastQ = (Fraction(float(v)) for v in run["trace"][gp])
    co = ch.coeffs(g)
    # slots: (index into raw, DC correction, weight of the converted sample in di)
    slots = []
    for n in ch.free_samples(g, gp):
        slots.append((2 * n, p["ic"], -lastI * co[n][0]))
        slots.append((2 * n + 1, p["qc"], -lastQ * co[n][1]))
    wl = np.array([float(w) for _, _, w in slots]) / 32767.0  # di per LSB
    r = ch.exact_di(raw, g, run["trace"][gp][0], run["trace"][gp][1], co)

    def move(i, d):
        idx, c, w = slots[i]
        old = int(raw[idx])
        new = old + d
        assert -32000 < new + c < 32000
        raw[idx] = new
        return w * (x_of(new, c) - x_of(old, c))

    # ---- coarse: minimum norm, rounded
    d0 = np.rint(-float(r) * wl / float(wl @ wl)).astype(int)
    assert np.abs(d0).max() <= MAX_DELTA, (g, float(r), np.abs(d0).max())
    for i in np.nonzero(d0)[0]:
        r += move(int(i), int(d0[i]))
    # ---- the slots of the fine step: weights spread from the largest down to 2 % of it (all of them where the window is short),
    # the two halves interleaved
    order = [int(i) for i in np.argsort(-np.abs(wl), kind="stable")]
    usable = [i for i in order if abs(wl[i]) > 0.02 * abs(wl[order[0]])]
    if len(usable) < 2 * NMITM + 8:
        usable = order[:2 * NMITM + 8]
    pick = [usable[int(round(q))] for q in np.linspace(0, len(usable) - 1, 2 * NMITM)]
    assert len(set(pick)) == 2 * NMITM
    halves = (pick[0::2], pick[1::2])
    rest = [i for i in order if i not in pick]
    # ---- greedy +-1 on the other slots while it helps
    for _ in range(400):
        fr = float(r)
        i = min(rest, key=lambda i: abs(abs(fr) - abs(wl[i])))
        d = -1 if fr * wl[i] > 0 else 1
        if abs(fr + d * wl[i]) >= abs(fr):
            break
        r += move(i, d)
    # ---- fine: meet in the middle.  The effect of -1 / +1 on a slot, exactly (the float division makes them unequal)
    def effects(i):
        idx, c, w = slots[i]
        v = int(raw[idx])
        return [float(w * (x_of(v + d, c) - x_of(v, c))) for d in (-1, 0, 1)]

    sums = []
    for half in halves:
        s = np.zeros(1)
        for i in half:
            e = effects(i)
            s = np.concatenate([s + e[0], s + e[1], s + e[2]])  # digit of slot i = the most significant so far
        sums.append(s)
    A, B = sums
    ob = np.argsort(B, kind="stable")
    Bs = B[ob]
    want = -(float(r) + A)
    pos = np.clip(np.searchsorted(Bs, want), 1, len(Bs) - 1)
    cand = []
    for q in (pos - 1, pos):
        err = np.abs(Bs[q] - want)
        best = np.argsort(err, kind="stable")[:6]
        cand += [(float(err[a]), int(a), int(ob[q[a]])) for a in best]
    cand.sort()

    def digits(code, half):
        out = []
        for i in reversed(half):  # the last slot added is the most significant digit
            n3 = 3 ** (len(half) - 1 - len(out))
            out.append((i, code // n3 - 1))
            code %= n3
        return out

    best = None
    for est, ia, ib in cand[:8]:
        moves = [m for m in digits(ia, halves[0]) + digits(ib, halves[1]) if m[1]]
        rr = r
        for i, d in moves:
            idx, c, w = slots[i]
            v = int(raw[idx])
            rr += w * (x_of(v + d, c) - x_of(v, c))
        if best is None or abs(rr) < abs(best[0]):
            best = (rr, moves)
    for i, d in best[1]:
        r += move(i, d)
    assert r == best[0]
    log.append((g, gp, float(r), int(np.abs(d0).max())))
    return r


def engineer_family(fam):
    p = T.FAMILIES[fam]
    ch = T.Chain(fam)
    base = T.base_stream(fam)
    raw = base.copy()
    run = T.run_oracle(fam, raw)
    g0 = run["g"].copy()
    # ---- the targets, on the base: smallest |di| first, 12 symbols apart
    ok = np.nonzero((run["g"] >= G_MIN) & (run["g"] <= run["g"][-1] - SPACING) & (run["e2"] > 1e5))[0]
    targets = []
    for k in ok[np.argsort(np.abs(run["di"][ok]), kind="stable")]:
        if all(abs(int(run["g"][k]) - int(run["g"][t])) >= SPACING for t in targets):
            targets.append(int(k))
        if len(targets) == p["want"]:
            break
    assert len(targets) == p["want"], (fam, len(targets))
    targets.sort()
    log, exact, done = [], [], {}
    for k in targets:
        keep_raw, keep_run = raw.copy(), run
        run = approach(ch, fam, raw, run, k)
        r = engineer_one(ch, raw, run, k, log)
        new = T.run_oracle(fam, raw)
        if new["e2"][k] < E2_MIN:  # the approach took the energy with it (bypassed tuner: both rails near their zero): not this one
            print("  %s k=%d dropped: energy2 %.3e" % (fam, k, new["e2"][k]), flush=True)
            raw[:] = keep_raw
            run = keep_run
            continue
        assert np.array_equal(new["g"][:k + 1], g0[:k + 1]), (fam, k)
        for t, (di_t, e2_t) in done.items():
            assert new["di"][t] == di_t and new["e2"][t] == e2_t, (fam, k, t)
        run = new
        done[k] = (run["di"][k], run["e2"][k])
        exact.append(float(r))
        print("  %s k=%d g=%d coarse max %d LSB  exact di %.3e  oracle di %.3e  energy2 %.3e" %
              (fam, k, log[-1][0], log[-1][3], float(r), run["di"][k], run["e2"][k]), flush=True)
    targets = list(done)
    assert len(targets) >= p["want"] - 2, (fam, len(targets))
    k = np.array(targets)
    # the exact di of every engineered decision on the FINAL stream, with the final run's dmLastIQ (must be what was reached)
    for t, want in zip(targets, exact):
        gp = int(run["g"][t - 1])
        have = ch.exact_di(raw, int(run["g"][t]), run["trace"][gp][0], run["trace"][gp][1])
        assert float(have) == want, (fam, t, float(have), want)
    idx = np.nonzero(raw != base)[0]
    out = {
        "params": np.array([p["rate"], p["tuning"], p["ic"], p["qc"], p["n"], p["seed"], p["stream"], T.AMP], np.int64),
        "carrier_noise": np.array([p["carrier"], p["noise_sigma"]], np.float64),
        "base_sha256": np.array(T.sha(base)),
        "sha256": np.array(T.sha(raw)),
        "sample": (idx // 2).astype(np.int32),
        "rail": (idx % 2).astype(np.int8),
        "delta": (raw[idx].astype(np.int32) - base[idx].astype(np.int32)).astype(np.int16),
        "dec": k.astype(np.int32),
        "g": run["g"][k].astype(np.int64),
        "gp": run["g"][k - 1].astype(np.int64),
        "di": run["di"][k].copy(),
        "e2": run["e2"][k].copy(),
        "exact_di": np.array(exact, np.float64),
    }
    return {fam + "_" + n: v for n, v in out.items()}


def main():
    t0 = time.time()
    fx = {}
    with multiprocessing.Pool(len(T.FAMILIES)) as pool:  # the families are independent of each other
        for part in pool.map(engineer_family, list(T.FAMILIES)):
            fx.update(part)
    np.savez_compressed(T.FIXTURE, **fx)
    # ---- the basis of TIE_ABS: how far the oracle's double di lies from the real number
    spread = np.abs(np.concatenate([fx[f + "_di"] - fx[f + "_exact_di"] for f in T.FAMILIES]))
    ex = np.abs(np.concatenate([fx[f + "_exact_di"] for f in T.FAMILIES]))
    print("engineered decisions: %d; |oracle di - exact di|: min %.2e, 10 %% %.2e, median %.2e, max %.2e" %
          (spread.size, spread.min(), np.percentile(spread, 10), np.median(spread), spread.max()))
    print("|exact di|: median %.2e, max %.2e; true ties (<= %.1e): %d" % (np.median(ex), ex.max(), T.TIE_ABS, int((ex <= T.TIE_ABS).sum())))
    print("patched samples: %d, file %d bytes, %.0f s" % (sum(fx[f + "_delta"].size for f in T.FAMILIES), os.path.getsize(T.FIXTURE), time.time() - t0))


if __name__ == "__main__":
    main()
