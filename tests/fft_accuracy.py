"""Round-off-level accuracy cases of the float spectrum path (fft_psd.hip, fft_mixed.hip, fft_rt.hip, fft_any.hip): the case
builders, the exact expectations and the bars shared by test_fft_accuracy_oracle.py (CPU) and test_gpu_fft_accuracy.py.

tests/test_gpu_fft.py holds the product's contract: 1e-5 of the frame's peak.  A correct float32 FFT of these sizes is wrong
by one to three float32 eps of the spectrum's norm, thirty to eighty times less, so a twiddle table that lost bits, a float
accumulator where a double one was or a coarser logarithm passes the contract.  The bars here are not constants: the yardstick
is a float32 FFT of the SAME frames on the CPU (torch.fft.fft on complex64), measured against the same exact DFT when the
test runs, and a kernel may be four times worse than the yardstick's worst frame of that size (two correct float FFTs with
different radix plans differ by small factors: the yardstick's own error spreads 0.8 ... 2.4 eps over these sizes).

  A  frames per size (noise, an off-bin real tone, a bin-centred tone with an off-bin one 46 dB below, x = 1, a full-scale
     int16 square wave) against the exact DFT:  E2 = |got - want|_2 / |want|_2,  Emax = max_k |got_k - want_k| / |x|_2
  B  impulses: bin k of the impulse at t0 is exp(-2 pi i (k t0 mod n) / n); with t0 = 1 it is the product of one entry of each
     pass's table, so one bad entry shows in one bin
  C  the frame a at sample 0: every bin of every family is exactly (a, 0), so the dB rule is tested alone, over the float range
"""
import functools
import math
import os

import numpy as np

import oracle_lib as O

EPS = 2.0 ** -23  # float32 eps

K_FFT = (64, 128, 256, 512, 1024, 2048, 4096, 8192)
K_MIXED = (4800, 9600, 19200)
# every other size: k_fft_rt where rt_plan (below) has a plan, k_dft_any for the rest.  22 = 2.11, 143 = 11.13 and 2.4099 are
# composite, but k_fft_rt takes a frame only while 8 x the sum of its prime factors above 7 is at most n (a term of such a pass
# costs several of k_dft_any's), so they run k_dft_any and are held to its tighter bar; the plan whose first and last pass are
# both generic is 97^2, the one with a generic pass behind butterflies 1102 = 2.19.29
OTHER = (12, 60, 210, 800, 3200, 4000, 4410, 9800, 22, 143, 1102, 2 * 4099, 97 * 97, 37, 9601, 17640, 19997)

EXACT_NMAX = 4410  # the oracle's long-double DFT is O(n^2): numpy's float64 FFT above


def kernel_for(n):
    """the family jsdr_fft_kernel must name for n"""
    if n in K_FFT:
        return "k_fft"
    if n in K_MIXED:
        return "k_fft_mixed_dual" if n == 19200 else "k_fft_mixed"
    return "k_fft_rt" if rt_plan(n) is not None else "k_dft_any"


# ---------------------------------------------------------------- radix plans (restated from the kernels' hosts)
_POW2_PLANS = {64: (8, 8), 128: (16, 8), 256: (16, 16), 512: (8, 8, 8), 1024: (16, 8, 8), 2048: (16, 16, 8), 4096: (16, 16, 16),
               8192: (16, 16, 8, 4)}                                     # fft_psd.hip pick_launcher
_MIXED_PLANS = {4800: (16, 4, 5, 5, 3), 9600: (16, 8, 5, 5, 3)}          # fft_mixed.hip mixed_plan


def rt_plan(n):
    """fft_rt.hip rt_plan: 16s, an 8, a 4, then the odd primes up to 7 (largest first; from 4000 samples merged into composite
    radices up to 25 while a pass keeps 192 butterflies), then the primes above 7 ascending; None where k_fft_rt does not serve n"""
    if n < 6 or n > 9800:
        return None
    m, rad = n, []
    while m % 16 == 0:
        rad.append(16)
        m //= 16
    for r in (8, 4):
        if m % r == 0:
            rad.append(r)
            m //= r
    odd = []
    for q in (7, 5, 3):
        while m % q == 0:
            odd.append(q)
            m //= q
    two = m % 2 == 0
    if two:
        m //= 2
    big, q = [], 11
    while m > 1:
        if q * q > m:
            q = m
        while m % q == 0:
            big.append(q)
            m //= q
        q += 2
    if 8 * sum(big) > n:
        return None
    merge, lo, hi = n >= 4000, 0, len(odd) - 1
    if two:
        if merge and odd and n // (2 * odd[lo]) >= 192:
            rad.append(2 * odd[lo])
            lo += 1
        else:
            rad.append(2)
    while lo <= hi:
        if merge and lo < hi and odd[lo] * odd[hi] <= 25 and n // (odd[lo] * odd[hi]) >= 192:
            rad.append(odd[lo] * odd[hi])
            lo, hi = lo + 1, hi - 1
        else:
            rad.append(odd[lo])
            lo += 1
    rad += big
    return tuple(rad) if len(rad) >= 2 else None


def plan(n):
    """the radix plan of n, first pass first; () for k_dft_any.  19200: the even / odd split, then the 9600-point plan."""
    if n in _POW2_PLANS:
        return _POW2_PLANS[n]
    if n in _MIXED_PLANS:
        return _MIXED_PLANS[n]
    if n == 19200:
        return (2,) + _MIXED_PLANS[9600]
    return rt_plan(n) or ()


K_RT = tuple(n for n in OTHER if rt_plan(n) is not None)
K_ANY = tuple(n for n in OTHER if rt_plan(n) is None)
SIZES = K_FFT + K_MIXED + OTHER


def plan_prefixes(n):
    """R0, R0 R1, ... below n (19200: of the split plan and of the half plan alone)"""
    out = set()
    plans = [plan(n)] + ([_MIXED_PLANS[9600]] if n == 19200 else [])
    for p in plans:
        prod = 1
        for r in p:
            prod *= r
            if prod < n:
                out.add(prod)
    return sorted(out)


# ---------------------------------------------------------------- small helpers
def ulp32(x):
    """spacing of float32 at |x| (float64 array in, float64 out)"""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (e - 23)


def lin(db):
    with np.errstate(over="ignore"):
        return 10.0 ** (np.asarray(db, np.float64) / 20.0)


def as_complex(buf):
    buf = np.asarray(buf, np.float64)
    return buf[..., 0::2] + 1j * buf[..., 1::2]


def interleave(z):
    z = np.asarray(z)
    out = np.empty(z.shape[:-1] + (2 * z.shape[-1],), np.float32)
    out[..., 0::2], out[..., 1::2] = z.real, z.imag
    return out


def exact_dft(buf):
    """the exact DFT of one float32 frame [2n] as complex128: long double below EXACT_NMAX, numpy's float64 FFT above"""
    n = buf.size // 2
    if n <= EXACT_NMAX:
        return as_complex(O.dft_exact(buf))
    return np.fft.fft(as_complex(buf))


def yardstick(bufs):
    """a float32 FFT of the same frames on the CPU: [frames, 2n] float32 -> complex128 [frames, n].  Called in the child process
    of yardstick_table() alone: importing a ROCm build of torch brings that build's own HIP / HSA runtime into the process, and
    RCCL, loaded later by the group tests of the same pytest run, then finds a runtime that was never initialised."""
    import torch
    z = torch.from_numpy(np.ascontiguousarray(bufs, np.float32).reshape(-1, bufs.shape[-1] // 2, 2).copy())
    return torch.fft.fft(torch.view_as_complex(z), dim=-1).numpy().astype(np.complex128)


def measures(got, want, x):
    """(E2, Emax) of one frame: got, want complex [n], x the frame [2n]"""
    d = np.abs(got - want)
    return float(np.sqrt((d ** 2).sum()) / np.sqrt((np.abs(want) ** 2).sum())), float(d.max() / np.linalg.norm(np.asarray(x, np.float64)))


# ---------------------------------------------------------------- A: frames
FRAME_NAMES = ("noise", "real tone off bin", "tone + off-bin tone 46 dB below", "x = 1", "int16 square wave")
NOISE = 0
SQUARE = 4  # index of the frame that goes through the int16 entry points


def square_i16(n):
    """a full-scale square wave of period 14 on I (32767 / -32768), the same three samples later on Q: int16 [2n]"""
    t = np.arange(n)
    raw = np.empty(2 * n, np.int16)
    raw[0::2] = np.where(t % 14 < 7, 32767, -32768)
    raw[1::2] = np.where((t + 11) % 14 < 7, 32767, -32768)
    return raw


@functools.lru_cache(maxsize=None)
def frames(n):
    """float32 [5, 2n] (read-only): FRAME_NAMES; the last is square_i16(n) as JavaAudio converts it"""
    rng = np.random.default_rng(1000003 * n + 17)
    t = np.arange(n, dtype=np.float64)
    f = np.zeros((5, 2 * n), np.float32)
    f[0] = (rng.standard_normal(2 * n) * 0.25).astype(np.float32)
    f[1, 0::2] = 0.4 * np.cos(2 * np.pi * (n / 5.0 + 0.25) * t / n)
    x = 0.3 * np.exp(2j * np.pi * (n // 7) * t / n) + 0.3 * 10.0 ** (-46.0 / 20.0) * np.exp(-2j * np.pi * (n / 9.0 + 0.5) * t / n)
    f[2] = interleave(x)
    f[3, 0::2] = 1.0
    f[4] = O.convert_i16(square_i16(n))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def want(n):
    """complex128 [5, n]: the exact DFT of frames(n), computed once a process"""
    w = np.stack([exact_dft(f) for f in frames(n)])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def yardstick_table():
    """{n: ([(E2, Emax)] over frames(n), the largest per-bin error over impulse_frames(n))} of the yardstick for every size,
    measured once a session in a child process (see yardstick) that prints it as JSON"""
    import json
    import subprocess
    import sys
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--yardstick"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("the yardstick's process failed:\n" + r.stdout + r.stderr)
    t = json.loads(r.stdout.strip().splitlines()[-1])
    return {int(n): (tuple((e2, em) for e2, em in v[0]), v[1]) for n, v in t.items()}


def yardstick_measures(n):
    """[(E2, Emax)] of the yardstick over frames(n)"""
    return yardstick_table()[n][0]


def bars(n):
    """(bar_E2, bar_Emax): four times the yardstick's largest value over the size's frames, at least one eps"""
    m = yardstick_measures(n)
    return max(4.0 * max(e for e, _ in m), EPS), max(4.0 * max(e for _, e in m), EPS)


def noise_emax_bar(n):
    """Emax is the error over |x|_2, and a tone's bin holds sqrt(n) |x|_2: over the size's frames the yardstick's largest Emax
    is the rounding of a few strong bins (up to 133 eps at n = 19997) and says little about a flat spectrum, where the
    yardstick stays below 7 eps.  The noise frame is therefore held to four times the yardstick's Emax on that frame as well."""
    return max(4.0 * yardstick_measures(n)[NOISE][1], EPS)


def psd_target(n, want_row):
    """what a PSD row's lin(dB) is compared with: |want_k| 2/n"""
    return np.abs(want_row) * (2.0 / n)


def level_m(n, t_db):
    """M of part C: |T| + 20 log10(n/2), the largest quantity the dB rule's float operations round"""
    return np.abs(t_db) + 20.0 * math.log10(n / 2.0)


def psd_bound(n, want_row, x, bar_emax):
    """per bin: (2/n) bar_Emax |x|_2  +  |want_k| (2/n) (ln 10 / 20) 4 ulp32(M_k) -- the spectrum's bar carried through the
    modulus, and the dB value's own rounding (part C) carried back through 10^(dB/20)"""
    a = psd_target(n, want_row)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = 20.0 * np.log10(a)
        db_term = np.where(a > 0, a * (math.log(10.0) / 20.0) * 4.0 * ulp32(level_m(n, t)), 0.0)
    return (2.0 / n) * bar_emax * np.linalg.norm(np.asarray(x, np.float64)) + db_term


def numpy_fft_allowance(n, want_row):
    """the float64 FFT's own error where `want` comes from it: 2^-52 log2(n) |want|_2"""
    return 0.0 if n <= EXACT_NMAX else 2.0 ** -52 * math.log2(n) * float(np.linalg.norm(want_row))


def correctly_rounded_bound(n, want_row, x):
    """k_dft_any's claim (fft_any.hip's header), per real / imaginary component: half a float32 ulp of the exact value plus the
    a-priori bound of n double additions and a 128-step double recurrence, (n + 256) 2^-52 |x|_1 (and numpy's own error where
    the exact value comes from it).  Returns (bound on .real, bound on .imag)."""
    slack = (n + 256) * 2.0 ** -52 * float(np.abs(np.asarray(x, np.float64)).sum()) + numpy_fft_allowance(n, want_row)
    return 0.5 * ulp32(want_row.real) + slack, 0.5 * ulp32(want_row.imag) + slack


# ---------------------------------------------------------------- B: impulses
def impulse_positions(n):
    """1, 2, 3, 5, 7, n/2 where even, n - 1, every prefix product of the plan, one seeded random position"""
    pos = {1, 2, 3, 5, 7, n - 1, int(np.random.default_rng(7919 * n + 1).integers(1, n))}
    if n % 2 == 0:
        pos.add(n // 2)
    pos.update(plan_prefixes(n))
    return sorted(p for p in pos if 0 < p < n)


def impulse_frames(n):
    pos = impulse_positions(n)
    f = np.zeros((len(pos), 2 * n), np.float32)
    for i, t0 in enumerate(pos):
        f[i, 2 * t0] = 1.0
    return f


def impulse_want(n):
    """complex128 [positions, n]: exp(-2 pi i ((k t0) mod n) / n), the product reduced in integers"""
    k = np.arange(n, dtype=np.int64)
    return np.stack([np.exp(-2j * np.pi * ((k * t0) % n).astype(np.float64) / n) for t0 in impulse_positions(n)])


def impulse_yardstick_error(n):
    """the yardstick's largest per-bin error over the size's impulses"""
    return yardstick_table()[n][1]


def impulse_bar(n):
    return max(4.0 * impulse_yardstick_error(n), EPS)


def impulse_db_bar(n):
    """a bin of modulus within impulse_bar of 1, in dB, plus part C's term at T = 20 log10(2/n)"""
    t = 20.0 * math.log10(2.0 / n)
    return -20.0 * math.log10(1.0 - impulse_bar(n)) + 4.0 * float(ulp32(level_m(n, t)))


# ---------------------------------------------------------------- C: levels
LONG_MANTISSAS = (1.0471975511965976, 1.2345678901234567, 1.6180339887498949)


def levels_f32(n):
    """a = 2^e (1 + m/16), e = -48 ... 60; m = 0 ... 15 up to 2048 samples, m in (0, 5, 11) above: float32 [levels].  The square
    of such a level has nine significant bits at the most, and a logarithm that is right on short arguments alone (one that
    drops the argument's low bits, say) would pass on them: three levels a binade more whose squares fill the mantissa."""
    ms = range(16) if n <= 2048 else (0, 5, 11)
    return np.array([math.ldexp(c, e) for e in range(-48, 61) for c in [1.0 + m / 16.0 for m in ms] + list(LONG_MANTISSAS)], np.float32)


LEVELS_I16 = (1, -1, 2, -2, 3, -3, 181, -181, 16384, -16384, 32767, -32768)


def levels_i16_as_float(n=None):
    """the int16 levels as JavaAudio converts them (the a of the int16 frames): float32 [12]"""
    raw = np.zeros(2 * len(LEVELS_I16), np.int16)
    raw[0::2] = LEVELS_I16
    return O.convert_i16(raw)[0::2].copy()


def level_frames_f32(n):
    a = levels_f32(n)
    f = np.zeros((a.size, 2 * n), np.float32)
    f[:, 0] = a
    return f


def level_frames_i16(n):
    f = np.zeros((len(LEVELS_I16), 2 * n), np.int16)
    f[:, 0] = LEVELS_I16
    return f


def level_power(a):
    """p = fl(a a): the float the kernel's re^2 + im^2 is for the bin (a, 0), as float32"""
    a = np.asarray(a, np.float32)
    return a * a


def level_pw(n, a):
    """the reference rule's own float product pw = p (2/n)^2 (fft.java:196-197, 207), float32"""
    cf = np.float32(2.0) / np.float32(n)
    cf = np.float32(cf * cf)
    return level_power(a) * cf


def level_target(n, a):
    """T = 10 log10(p 4 / n^2) in float64"""
    return 10.0 * np.log10(level_power(a).astype(np.float64) * 4.0 / (float(n) * float(n)))


def level_bound(n, a, ulps=4.0):
    return ulps * ulp32(level_m(n, level_target(n, a)))


if __name__ == "__main__" and "--yardstick" in __import__("sys").argv:  # the child process of yardstick_table()
    import json
    table = {}
    for size in SIZES:
        y = yardstick(frames(size))
        table[size] = ([measures(y[k], want(size)[k], frames(size)[k]) for k in range(5)],
                       float(np.abs(yardstick(impulse_frames(size)) - impulse_want(size)).max()))
    print(json.dumps(table))
