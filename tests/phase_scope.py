"""The batched phase scope (jsdr_phase_scope_i16 / _f32): what a frame's row must hold, restated on the CPU, and the case lists
of test_phase_scope_abi.py (CPU) and test_gpu_phase_scope.py.

The maximum and the column means are the oracle's (O.phase_maxabs, O.phase_columns on the frame as O.convert_i16 gives it); the
schedule's first / count and the painter's four integers (phase.java:85-86, 102, 107, 109) are restated here in numpy float32,
one rounding an operation, with Java's (int).  Everything is exact: floats are compared by nonfinite.same_f32 (the same bits, or
both NaN -- Java cannot tell NaNs apart and x86 and gfx950 make different ones), integers as they are.

Plain module (no device, no fixtures)."""
import numpy as np

import oracle_lib as O
from nonfinite import same_f32

F32 = np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
LDS_MAX_N = 8192  # frames up to here run "k_phase_scope", larger ones "k_phase_scope_g"

GRID_N = (64, 600, 800, 1002, 1102, 2048)


def grid_bx(n):
    return (0, 1, 3, 4, 7, 21, 63, n - 1, n, n + 1, 2 * n, 3 * n + 1)


# (n, bx) -> (closed columns, samples left over behind the last): float32 arithmetic, computed on the CPU
CENSUS = {(600, 1): (0, 600), (600, 4): (3, 149), (800, 7): (6, 114), (1102, 5): (4, 220), (9600, 700): (700, None),
          (9600, 1024): (1024, None), (64, 65): (64, 0), (64, 128): (64, 0), (64, 200): (64, 0), (2048, 2048): (2048, None)}


def java_int(x):
    """Java's (int) of float32 values: truncation, saturation, NaN -> 0"""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x.astype(np.float64))
    t = np.where(np.isnan(t), 0.0, np.clip(t, INT_MIN, INT_MAX))
    return t.astype(np.int64).astype(np.int32)


def layout_py(n, bx):
    """phase.java:81, 84, 93-99, 110-114 in float32: (pix, first sample, sample count) of every closed column"""
    step = F32(F32(bx * 2) / F32(2 * n))
    pos = F32(0)
    lpix = acnt = start = 0
    pix, first, count = [], [], []
    for s in range(n):
        acnt += 1
        pos = F32(pos + step)
        p = int(pos) if abs(pos) < 2 ** 31 else int(java_int(pos))  # (int() truncates as the cast does)
        if p > lpix:
            pix.append(p)
            first.append(start)
            count.append(acnt)
            lpix, acnt, start = p, 0, s + 1
    return np.array(pix, np.int32), np.array(first, np.int32), np.array(count, np.int32)


def layout_exact(n, bx):
    """the schedule a rational pos would give: after sample s, pix = floor((s + 1) * bx / n)"""
    lpix = start = 0
    first, count = [], []
    for s in range(n):
        p = (s + 1) * bx // n
        if p > lpix:
            first.append(start)
            count.append(s + 1 - start)
            lpix, start = p, s + 1
    return np.array(first, np.int32), np.array(count, np.int32)


_layouts = {}


def layout(n, bx):
    if (n, bx) not in _layouts:
        _layouts[n, bx] = layout_py(n, bx)
    return _layouts[n, bx]


def expected_row(frame, bx, half_size, quarter_height):
    """frame: float32 [2n] as the kernel takes it -> (max float32, avg float32 [ncol][2], pts int32 [ncol][4])"""
    frame = np.ascontiguousarray(frame, F32)
    n = frame.size // 2
    mx = F32(O.phase_maxabs(frame))
    pix, ai, aq = O.phase_columns(frame, bx)
    lpix, first, count = layout(n, bx)
    assert np.array_equal(pix, lpix), (n, bx)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hiq = F32(quarter_height) / mx  # phase.java:85-86
        hph = F32(half_size) / mx
        e = first + count - 1           # each column's closing sample
        pts = np.stack([java_int(ai * hiq), java_int(aq * hiq), java_int(frame[2 * e] * hph), java_int(frame[2 * e + 1] * hph)], 1)
    return mx, np.stack([ai, aq], 1).astype(F32), pts.astype(np.int32).reshape(-1, 4)


def expected_rows(frames, bx, half_size, quarter_height):
    """frames float32 [rows][2n] -> (max [rows], avg [rows][ncol][2], pts [rows][ncol][4])"""
    rows = [expected_row(f, bx, half_size, quarter_height) for f in frames]
    ncol = layout(frames.shape[1] // 2, bx)[0].size
    return (np.array([r[0] for r in rows], F32), np.array([r[1] for r in rows], F32).reshape(len(rows), ncol, 2),
            np.array([r[2] for r in rows], np.int32).reshape(len(rows), ncol, 4))


def assert_rows(got, want, where):
    """(max, avg, pts) of a call against expected_rows, every row of every output; avg / pts None where not asked for"""
    for name, g, w in zip(("max", "avg", "pts"), got, want):
        if g is None:
            continue
        g = np.asarray(g).reshape(w.shape)
        ok = same_f32(g, w) if w.dtype == F32 else g == w
        if not ok.all():
            i = np.argwhere(~ok)[0]
            raise AssertionError((where, name, "first of %d differences at" % int((~ok).sum()), tuple(int(k) for k in i), g[tuple(i)], w[tuple(i)]))


# ------------------------------------------------------------------------------------------------ frames
def max_places(n, bx):
    """where the rows of a case put their one largest sample (flat index into the 2n values): first sample, last sample, a sample
    behind the last closed column (where there is one), then others"""
    _, first, count = layout(n, bx)
    end = int(first[-1] + count[-1]) if first.size else 0
    tail = 2 * end + 1 if end < n else n + 1  # Q of the first dropped sample
    return [0, 2 * n - 1, tail, n, 2 * n - 2, 1, 2 * (n // 3), 3, 2 * n - 4]


_raw = {}


def raw_frames(n, count, seed=0):
    """int16 [count][2n]: noise within +-3000 on three turns of a circle of radius 9000 (column means that are not all near 0),
    every frame another"""
    key = (n, count, seed)
    if key not in _raw:
        x = np.random.default_rng([n, count, seed]).integers(-3000, 3000, (count, 2 * n)).astype(np.float64)
        w = 2 * np.pi * 3 * np.arange(n) / n
        for k in range(count):
            x[k, 0::2] += 9000 * np.cos(w + k)
            x[k, 1::2] += 9000 * np.sin(w + k)
        x = x.astype(np.int16)
        x.setflags(write=False)
        _raw[key] = x
    return _raw[key]


def grid_frames(form, n, bx, count):
    """count frames whose maximum sits at max_places: int16, or floats off the int16 grid; and the floats the kernel takes"""
    x = np.array(raw_frames(n, count))
    for k, p in enumerate(max_places(n, bx)[:count]):
        x[k, p] = (-1) ** k * (20000 + 13 * k)
    if form == "i16":
        return x
    return (O.convert_i16(x.ravel()) * F32(0.93)).astype(F32).reshape(count, 2 * n)


def as_floats(form, frames, ic=0, qc=0):
    """the frames as the kernel takes them: float32 [rows][2n]"""
    if form == "f32":
        return np.ascontiguousarray(frames, F32)
    return O.convert_i16(np.ascontiguousarray(frames, np.int16).ravel(), ic=ic, qc=qc).reshape(frames.shape)


def denormal_frame(n, seed=3):
    """denormals and zeros only, max 1e-40: the scales overflow to +Inf, the integers saturate both ways, zeros give 0"""
    vals = np.array([1e-40, -1e-40, 0.0, 5e-41, -3e-41, -0.0], F32)
    f = np.random.default_rng(seed).choice(vals, 2 * n).astype(F32)
    f[5] = F32(1e-40)
    return f


def check_denormal_row(frame, bx, half_size, quarter_height):
    """on the CPU: the expected row of denormal_frame really holds INT_MAX, INT_MIN and 0"""
    mx, _, pts = expected_row(frame, bx, half_size, quarter_height)
    with np.errstate(over="ignore"):
        assert mx == F32(1e-40) and np.isinf(F32(half_size) / mx)
    assert (pts == INT_MAX).any() and (pts == INT_MIN).any() and (pts == 0).any(), np.unique(pts)
