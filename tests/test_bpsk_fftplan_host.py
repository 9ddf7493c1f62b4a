"""The FFT-acquire plan (java-sdr_amd/csrc/bpsk_fftplan.hip) on the CPU: a stand-alone driver (tests/tools/fftplan_driver.hip) is
compiled with the unit, with the flags build.py gives it, and what it answers is compared with the CPU oracle
(jo_fft_mixed_radices, jo_fft_mixed_table, jo_fft_twiddles_f64) and with restatements in Python.

No device and no library: what is checked here decides whether a stream stays bit-identical to the oracle (the pass order, the
table values), which kernel runs (the front-end selection) and whether a kernel reads its tables at the right offsets."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "java-sdr_amd", "csrc")
POW2, FFTM, FFT2X, GEN, NONE = range(5)
DEFAULT_OFFSETS = {9600: [0, 4, 20, 84, 212, 596, 2516], 4800: [0, 4, 20, 84, 276, 1236], 4410: [0, 2, 8, 26, 116, 746]}


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
        pytest.skip("no hipcc found: the plan driver cannot be compiled")
    exe = str(tmp_path_factory.mktemp("fftplan") / "fftplan_driver")
    cmd = [cc] + b.COMMON + b.SOURCES["bpsk_fftplan.hip"] + [os.path.join(ROOT, "tests", "tools", "fftplan_driver.hip"),
                                                            os.path.join(CSRC, "bpsk_fftplan.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        return p.stdout.split("\n")
    return run


# ------------------------------------------------------------------------------------------------ the oracle, talking to the driver
def oracle_radices(n):
    rad = (C.c_int * 64)()
    f = O.lib().jo_fft_mixed_radices
    f.argtypes = [C.c_int, C.c_void_p]
    f.restype = C.c_int
    return list(rad[:f(n, rad)])


_tables = {}


def oracle_table(length):
    """jo_fft_mixed_table(length) as the bit patterns of its doubles, [length, 2] uint64; computed once a length"""
    if length not in _tables:
        t = np.empty(2 * length, np.float64)
        f = O.lib().jo_fft_mixed_table
        f.argtypes = [C.c_void_p, C.c_int]
        f.restype = None
        f(O.ptr(t), length)
        _tables[length] = t.view(np.uint64).reshape(length, 2)
    return _tables[length]


def entries(line):
    """a line of table entries -> [n, 2] uint64 bit patterns"""
    b = bytes.fromhex(line.strip())
    return np.frombuffer(b, dtype=">u8").astype(np.uint64).reshape(-1, 2)


def plan(driver, n, kind):
    out = driver(["plan %d %d" % (n, kind), "w %d %d" % (n, kind)])
    f = [int(v) for v in out[0].split()]
    d = dict(ok=f[0], kind=f[1], logn=f[2], np=f[3], wsize=f[4], lds_tw=f[5], lds_tw_pair=f[6])
    for i, name in enumerate(["rad", "tw_off", "wr_off", "tw1_off", "pmagic"]):
        d[name] = [int(v) for v in out[1 + i].split()[1:]]
    d["w"] = entries(out[6])
    assert len(d["w"]) == d["wsize"]
    return d


def strides(rad):
    P, out = 1, []
    for r in rad:
        out.append(P)
        P *= r
    return out


# ------------------------------------------------------------------------------------------------ radices
def test_radices_are_the_oracles_for_every_frame_of_both_former_callers(driver):
    """every n up to 9600 (the LDS front ends' range, where the list has no leading radix 2) and the any-frame passes' frames"""
    ns = list(range(2, 9601)) + [17640, 19200, 38400, 2 * 11 * 11 * 13, 1103]
    out = driver(["radices %d" % n for n in ns])
    for n, o in zip(ns, out):
        f = [int(v) for v in o.split()]
        assert f[1:] == oracle_radices(n) and f[0] == len(f) - 1 and f[0] > 0, n
    assert oracle_radices(19200)[0] == 2 and oracle_radices(9600)[0] == 4  # (the leading radix 2 is there above 9600 samples only)


# ------------------------------------------------------------------------------------------------ tables and offsets
@pytest.mark.parametrize("n,kind", [(9600, FFTM), (4800, FFTM), (4410, FFTM), (7000, FFTM), (1100, FFTM), (1102, FFTM), (17640, GEN)])
def test_every_table_is_the_oracles_bit_for_bit(driver, n, kind):
    p = plan(driver, n, kind)
    assert p["ok"] == 1 and p["kind"] == kind and p["rad"] == oracle_radices(n) and p["logn"] == 0
    end = 0
    for r, P, off in zip(p["rad"], strides(p["rad"]), p["tw_off"]):
        assert off == end  # back to back
        assert np.array_equal(p["w"][off:off + P * r], oracle_table(P * r)), (n, r, P)
        end = off + P * r
    for r, off in zip(p["rad"], p["wr_off"]):  # the r-point tables of the prime radices above 7, behind every pass table
        if r > 7:
            assert off == end and np.array_equal(p["w"][off:off + r], oracle_table(r)), (n, r)
            end = off + r
        else:
            assert off == 0
    assert end == p["wsize"]
    assert any(r > 7 for r in p["rad"]) == (n in (1100, 1102))


def test_the_2m_front_ends_tables(driver):
    """19200: the m-point tables, then U_p[(j - 1) P' + k'] = T_{2 P' r}[(2 k' + 1) j] for every pass"""
    p = plan(driver, 19200, FFT2X)
    assert p["ok"] == 1 and p["rad"] == oracle_radices(9600) == oracle_radices(19200)[1:]
    assert p["tw_off"] == DEFAULT_OFFSETS[9600] and p["lds_tw"] == 0 and all(o == 0 for o in p["wr_off"])
    end = 0
    for r, P, off in zip(p["rad"], strides(p["rad"]), p["tw_off"]):
        assert off == end and np.array_equal(p["w"][off:off + P * r], oracle_table(P * r))
        end = off + P * r
    for r, P, off in zip(p["rad"], strides(p["rad"]), p["tw1_off"]):
        assert off == end
        T = oracle_table(2 * P * r)
        j, k = np.meshgrid(np.arange(1, r), np.arange(P), indexing="ij")
        assert np.array_equal(p["w"][off:off + (r - 1) * P], T[((2 * k + 1) * j).reshape(-1)]), (r, P)
        end = off + (r - 1) * P
    assert end == p["wsize"]


@pytest.mark.parametrize("n,kind", [(2048, POW2), (16384, GEN)])
def test_a_power_of_two_has_the_radix_2_networks_table(driver, n, kind):
    p = plan(driver, n, kind)
    assert (p["ok"], p["kind"], p["logn"], p["np"], p["wsize"]) == (1, kind, n.bit_length() - 1, 0, n)
    base = O.fft_twiddles_f64(n).view(np.uint64).reshape(n // 2, 2)
    half = 1
    while half < n:
        assert np.array_equal(p["w"][half - 1:2 * half - 1], base[::n // (2 * half)])
        half *= 2


def test_default_frames_offsets_and_lds_prefixes(driver):
    want = {9600: (596, 0), 4800: (1236, 276), 4410: (5156, 746)}
    for n, (single, pair) in want.items():
        p = plan(driver, n, FFTM)
        assert p["tw_off"] == DEFAULT_OFFSETS[n] and (p["lds_tw"], p["lds_tw_pair"]) == (single, pair), n
    out = driver(["args 9600 1 -1 0 0 0", "args 4800 1 -1 0 0 0", "args 4410 1 -1 0 0 0", "args 4800 1 -2 1 0 0", "args 4410 1 -2 1 0 0"])
    assert [o.split() for o in out[:5]] == [["1", "596"], ["1", "1236"], ["1", "5156"], ["1", "276"], ["1", "746"]]
    # a frame that is not a default one takes whatever prefix fits: 7000 = 4 2 5 5 5 7, every table but the last in 51 KB
    p = plan(driver, 7000, FFTM)
    assert p["lds_tw"] == sum(P * r for r, P in zip(p["rad"], strides(p["rad"])) if P * r < 7000)


# (n, pair form, the first pass whose table lies behind the LDS prefix, the prefix); 4410's single-frame form holds every table in LDS
BEHIND_THE_PREFIX = [(9600, 0, 5, 596), (4800, 0, 5, 1236), (4800, 1, 4, 276), (4410, 1, 5, 746)]


@pytest.mark.parametrize("n,pair", [(9600, 0), (4800, 0), (4410, 0), (4800, 1), (4410, 1)])
def test_a_default_frame_with_its_tables_moved_is_refused(driver, n, pair):
    """every table moved by one entry: the LDS prefix breaks with them"""
    room = -2 if pair else -1
    out = [o.split() for o in driver(["args %d 1 %d %d 0 0" % (n, room, pair), "args %d 1 %d %d 1 0" % (n, room, pair)])[:2]]
    assert out[0][0] == "1" and out[1] == ["0", "0"]
    assert driver(["args 7000 1 -1 0 1 0"])[0].split()[0] == "1"  # (no compile-time offsets there: the kernel reads them from the arguments)


@pytest.mark.parametrize("n,pair,first,prefix", BEHIND_THE_PREFIX)
def test_a_default_frame_with_a_table_behind_the_lds_prefix_moved_is_refused(driver, n, pair, first, prefix):
    """only the tables that stay in global memory moved by one entry: lds_tw is what the kernel expects, and the plan is refused
    all the same -- the check compares the offsets themselves, not the prefix alone"""
    room = -2 if pair else -1
    nps = len(DEFAULT_OFFSETS[n])
    for frm in range(first, nps):
        o = driver(["args %d 1 %d %d 1 %d" % (n, room, pair, frm)])[0].split()
        assert o == ["0", str(prefix)], (n, pair, frm)


def test_pmagic_divides_every_16_bit_index(driver):
    b = np.arange(1 << 16, dtype=np.uint64)
    seen = set()
    for n, kind in [(9600, FFTM), (4800, FFTM), (4410, FFTM), (7000, FFTM), (1100, FFTM), (1102, FFTM), (19200, FFT2X)]:
        p = plan(driver, n, kind)
        assert len(p["pmagic"]) == p["np"]
        for P, m in zip(strides(p["rad"]), p["pmagic"]):
            if P > 1:  # (2^32 / 1 does not fit: the passes take k = 0 at P = 1)
                assert np.array_equal((b * np.uint64(m)) >> np.uint64(32), b // np.uint64(P)), (n, P)
            seen.add(P)
    assert {1, 4, 16, 64, 128, 384, 1920, 192, 960, 2, 6, 18, 90, 630} <= seen


# ------------------------------------------------------------------------------------------------ front-end selection
def prime_factors(n):
    out, p = [], 2
    while p * p <= n:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1
    return out + ([n] if n > 1 else [])


def is_pow2(n):
    return n & (n - 1) == 0


def takes_pow2(n):
    return is_pow2(n) and 1024 <= n <= 8192


def takes_mixed(n):
    """any other frame up to 9600 samples -- from 416, where the 204 gathered bins end inside the frame"""
    return 416 <= n <= 9600 and not is_pow2(n)


def takes_2m(n):
    m = n // 2
    return n > 9600 and n % 2 == 0 and m % 16 == 0 and m % 7 != 0 and takes_mixed(m)


def takes_any(n):
    return 416 <= n <= 1 << 22 and (is_pow2(n) or all(n * r <= 1 << 31 for r in prime_factors(n) if r > 7))


def front_kind(n, decim, chan_form, force_gen):
    if chan_form:  # the three-phase front ends only
        lds = (takes_pow2(n) and decim >= 4) or n in (9600, 4800, 4410)
    else:
        lds = takes_mixed(n) or (decim >= 4 and (takes_pow2(n) or takes_2m(n)))
    if force_gen == 1 or (force_gen < 0 and not lds):
        return GEN if takes_any(n) else NONE
    if not lds:
        return NONE
    return POW2 if takes_pow2(n) else FFT2X if takes_2m(n) else FFTM


def test_front_end_selection_is_the_rule(driver):
    edge_primes = [p for p in range(46300, 46400) if len(prime_factors(p)) == 1]  # n = p: refused from p^2 > 2^31, p > 46340
    half_primes = [2 * p for p in range(32740, 32800) if len(prime_factors(p)) == 1]  # n = 2 p: from 2 p^2 > 2^31, p > 32768
    extra = [1 << k for k in range(22 + 1)] + [(1 << 22) + 2] + edge_primes + half_primes
    lines = ["sweep 400 20000"] + ["sweep %d %d" % (n, n) for n in extra]
    out = [o for o in driver(lines) if o]
    ns = list(range(400, 20001)) + extra
    assert len(out) == len(ns)
    refused = set()
    for n, o in zip(ns, out):
        f = o.split()
        assert int(f[0]) == n
        primes_above_7 = [r for r in prime_factors(n) if r > 7]
        assert [int(v) for v in f[1:6]] == [takes_mixed(n), takes_2m(n), n in (9600, 4800, 4410), takes_any(n),
                                            n if primes_above_7 else 0], n
        want = "".join(str(front_kind(n, d, c, g)) for d in (1, 2, 4, 10) for c in (False, True) for g in (-1, 0, 1))
        assert f[6] == want, n
        if 416 <= n <= 1 << 22 and primes_above_7:
            assert takes_any(n) == (n * max(primes_above_7) <= 1 << 31)
            if not takes_any(n):
                refused.add(n)
    assert refused and set(edge_primes) - refused and set(half_primes) - refused  # both sides of 2^31, for n = p and n = 2 p


def test_scratch_sizes(driver):
    out = driver(["scratch 1102", "scratch 9600", "scratch 19200", "scratch 17640", "scratch 16384"])
    assert out[0].split()[0] == "1102" and out[1].split()[0] == "0"
    assert out[2].split()[:3] == ["0", str(19200 // 4 + 52), str(19200 // 2 + 16)]
    assert out[3].split()[3] == str(16 * 17640 * 2) and out[4].split()[3] == str(16 * 16384)


def test_a_plan_is_refused_for_a_front_end_that_does_not_take_the_frame(driver):
    for n, kind in [(17640, FFTM), (9600, FFT2X), (2048, FFTM), (9600, POW2), (400, GEN), (9600, NONE)]:
        assert plan(driver, n, kind)["ok"] == 0, (n, kind)
