"""The scalar rules of FFT-acquire (java-sdr_amd/csrc/bpsk_acq_rule.h) on the CPU: a stand-alone driver
(tests/tools/acq_rule_driver.hip) is compiled with the flags build.py gives the FFT-acquire units, and what it answers is compared
bit for bit with a restatement of FUNcubeBPSKDemod.java:399-456 in numpy float32 / float64 scalars -- IEEE, every operation rounded
by itself, so the restatement is exact and independent of the C++.

No device and no library: the centre-bin rule decides which 204 bins of a frame every FFT-acquire kernel keeps, and every one of
them steps it through this header.  The driver is built twice, plainly and with -fsanitize=address,undefined on the host side,
and both builds answer every test."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64

# :399-402 -- float expressions (the int sums promote to float), widened to double
CFREQ_INV = F64(F32(1.0) - (F32(2.0) / F32(1 + 1)))
CFREQ_AVG = F64(F32(2.0) / F32(1 + 1))
PSD_INV = F64(F32(1.0) - (F32(2.0) / F32(10 + 1)))
PSD_AVG = F64(F32(2.0) / F32(10 + 1))

BANDS = [(2048, 0), (2048, 1), (9600, 0), (9600, 1)]


def _build_py():
    spec = importlib.util.spec_from_file_location("jsdr_build", os.path.join(ROOT, "java-sdr_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    b = _build_py()
    cc = b.hipcc()
    if not (os.path.exists(cc) if os.path.isabs(cc) else shutil.which(cc)):
        pytest.skip("no hipcc found: the rule driver cannot be compiled")
    exe = str(tmp_path_factory.mktemp("acq_rule") / "acq_rule_driver")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    cmd = [cc] + b.COMMON + b.SOURCES["bpsk_fft.hip"] + extra + [os.path.join(ROOT, "tests", "tools", "acq_rule_driver.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout.split("\n")
    return run


def bits(x):
    return F64(x).tobytes()


def hx(x):
    return float(x).hex()


# ------------------------------------------------------------------------------------------------ the restatement
def band(n, up):
    return (n // 4 if up else 0), (n // 2 if up else n // 4)  # :429-430


class Rule:
    """:403-405 and :444-456.  avePsd is a fresh array of zeros per frame (:413) of which the loop fills [beg + 75, end - 75) only."""

    def __init__(self, n, up, app=0.0, acb=0.0, cb=0):
        self.beg, self.end = band(n, up)
        self.app, self.acb, self.cb = F64(app), F64(acb), int(cb)

    def clamped(self):
        cb = self.cb
        if cb < 0:
            cb = 0
        if cb > self.end - 1:
            cb = self.end - 1
        return cb

    def peak_after(self, psd):
        """avePeakPower as the frame leaves it, given what the loop put at the clamped centre bin"""
        cb = self.clamped()
        ave = F64(psd) if self.beg + 75 <= cb < self.end - 75 else F64(0.0)
        return (PSD_AVG * ave) + (PSD_INV * self.app)

    def threshold(self, psd):
        return (self.peak_after(psd) / F64(4)) * F64(5)

    def frame(self, psd, max_bin, bin_pos):
        self.cb = self.clamped()
        self.app = self.peak_after(psd)
        if F64(max_bin) > (self.app / F64(4)) * F64(5) and bin_pos > 0:
            self.acb = (CFREQ_AVG * F64(F32(bin_pos))) + (CFREQ_INV * self.acb)
            self.cb = int(self.acb + F64(F32(1.0)))
        if self.cb < 102:
            self.cb = 102
        return self.app, self.acb, self.cb


def check_rule(driver, n, up, app, acb, cb, frames, want):
    lines = ["rule %d %d %s %s %d %d" % (n, up, hx(app), hx(acb), cb, len(frames))]
    lines += ["%s %s %d" % (hx(p), hx(m), b) for p, m, b in frames]
    out = driver(lines)
    assert len([ln for ln in out if ln]) == len(frames)
    for k, (ln, w) in enumerate(zip(out, want)):
        a, c, b = ln.split()
        got = (bits(float.fromhex(a)), bits(float.fromhex(c)), int(b))
        assert got == (bits(w[0]), bits(w[1]), w[2]), "frame %d: driver %s, restatement %s" % (k, ln, (hx(w[0]), hx(w[1]), w[2]))


# ------------------------------------------------------------------------------------------------ the tests
def test_constants_and_bands(driver):
    out = driver(["consts"] + ["band %d %d" % b for b in BANDS])
    got = [float.fromhex(t) for t in out[0].split()]
    assert [bits(g) for g in got] == [bits(x) for x in (CFREQ_INV, CFREQ_AVG, PSD_INV, PSD_AVG, F64(0.9) * F64(32768.0))]
    for ln, (n, up) in zip(out[1:], BANDS):
        assert tuple(int(t) for t in ln.split()) == band(n, up)


@pytest.mark.parametrize("n,up", BANDS)
@pytest.mark.parametrize("cb0", ["below", "above", "inside"])
def test_rule_edges(driver, n, up, cb0):
    """starts outside [0, end - 1]; binPos -1 / 0 / 1; maxBin at the threshold and an ulp to either side; aveCentreBin + 1 < 102"""
    beg, end = band(n, up)
    start = {"below": -7, "above": end + 300, "inside": beg + 200}[cb0]
    r = Rule(n, up, 1234.5, float(beg + 200), start)
    mid = beg + (end - beg) // 2
    frames, want = [], []

    def push(psd, mb, bp):
        frames.append((F64(psd), F64(mb), bp))
        want.append(r.frame(psd, mb, bp))

    push(900.0, 5000.0, mid)  # the first frame meets the start as it is
    for bp in (-1, 0, 1):     # a maximum far above the threshold: only binPos > 0 moves the centre (and 1 lands below 102)
        push(1000.0, 1.0e9, bp)
        push(1000.0, 1.0e9, mid)
    for psd in (0.0, 777.25, 31337.0):
        for bp in (mid, end - 76):
            thr = r.threshold(psd)
            for mb in (np.nextafter(thr, F64(-np.inf)), thr, np.nextafter(thr, F64(np.inf))):
                push(psd, mb, bp)
    # aveCentreBin + 1 below 102: small bin positions, accepted every frame, the average walks down to them
    for bp in (60, 60, 60, 60, 60, 60, 60, 60, 3, 3, 3, 100, 101, 101, 101, 101, 101, 101, 101, 101):
        push(10.0, 1.0e9, bp)
    assert min(w[2] for w in want[-20:]) == 102 and any(float(w[1]) + 1.0 < 102.0 for w in want[-20:])
    # and back up to the band's far end (the clamp to end - 1 is the NEXT frame's)
    for bp in (end - 76,) * 12:
        push(10.0, 1.0e9, bp)
    check_rule(driver, n, up, 1234.5, float(beg + 200), start, frames, want)


@pytest.mark.parametrize("n,up", BANDS)
def test_rule_random_frames(driver, n, up):
    beg, end = band(n, up)
    rng = np.random.default_rng(20020109 + n + up)
    r = Rule(n, up)
    frames, want = [], []
    for _ in range(10000):
        psd = F64(rng.lognormal(6.0, 1.0))
        mb = psd * F64(rng.uniform(0.7, 1.9))  # around (5 / 4) avePeakPower: both outcomes of the test occur
        u = rng.uniform()
        if u < 0.05:
            bp = int(rng.choice([-1, 0, 1, 50, 100, 101]))
        else:
            bp = int(rng.integers(beg + 75, end - 75))
        frames.append((psd, mb, bp))
        want.append(r.frame(psd, mb, bp))
    moved = sum(1 for a, b in zip(want, want[1:]) if a[2] != b[2])
    assert 1000 < moved < 9000, moved  # the sequence exercises both branches
    check_rule(driver, n, up, 0.0, 0.0, 0, frames, want)


def test_first_maximum(driver):
    """strict '<': the first of equal maxima; nothing above 0.0 leaves (0.0, -1)"""
    cases = [[1.0, 3.0, 3.0, 2.0], [0.0, 0.0, 0.0], [5.0], [2.0, 2.0, 2.0], [1.0, 2.0, 3.0, 3.0], [0.0, 1e-300, 1e-300], [3.0, 1.0, 3.0, 4.0, 4.0, 0.5]]
    out = driver(["max %d %s" % (len(c), " ".join(hx(v) for v in c)) for c in cases])
    for c, ln in zip(cases, out):
        bv, bi = F64(0.0), -1
        for i, v in enumerate(c):  # :439-442
            if bv < F64(v):
                bv, bi = F64(v), i
        assert (bits(float.fromhex(ln.split()[0])), int(ln.split()[1])) == (bits(bv), bi), (c, ln)


def test_merge_is_the_search_over_the_whole(driver):
    """partial searches over pieces of an array, merged in any order, give the search over the whole array"""
    rng = np.random.default_rng(7)
    lines, want = [], []
    for trial in range(200):
        k = int(rng.integers(1, 40))
        v = rng.integers(0, 4, k).astype(np.float64)  # few distinct values: ties everywhere, all-zero arrays too
        bv, bi = 0.0, -1
        for i in range(k):
            if bv < v[i]:
                bv, bi = v[i], i
        want.append((bv, bi))
        # interleaved pieces (a thread's items ascend, pieces do not), each searched first-maximum
        npieces = int(rng.integers(1, 7))
        cand = []
        for p in range(npieces):
            pv, pi = 0.0, -1
            for i in range(p, k, npieces):
                if pv < v[i]:
                    pv, pi = v[i], i
            cand.append((pv, pi))
        order = rng.permutation(npieces)
        lines.append("merge %d %s" % (npieces, " ".join("%s %d" % (hx(cand[o][0]), cand[o][1]) for o in order)))
    out = driver(lines)
    for ln, (bv, bi) in zip(out, want):
        assert (float.fromhex(ln.split()[0]), int(ln.split()[1])) == (bv, bi), ln


def test_first_output(driver):
    """output j of a call ends at sample first_out + D j: the first one that ends at or behind t0"""
    cases = [(t0, fo, d) for d in (4, 5, 10, 20) for fo in (0, 3, d - 1, 2048, 5000) for t0 in (0, 2048, 4096, 9600, 4800 * 7, 19200 * 3)]
    out = driver(["first %d %d %d" % c for c in cases])
    for (t0, fo, d), ln in zip(cases, out):
        j = 0
        while fo + d * j < t0:
            j += 1
        assert int(ln) == j, (t0, fo, d, ln)
