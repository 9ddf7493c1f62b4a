"""Padded and offset layouts for the batch entry points (tests/test_gpu_layouts.py).

A batch call reads and writes rows at `base + lead + r * stride` (include/jsdr_hip.h).  `Layout` is that arithmetic, in
elements of the buffer's dtype and in bytes.  `build_input` puts the rows of an input where the ABI says and fills every
other element -- the lead, the gap after each row and the tail -- with poison that would change a result if a kernel
read it: extreme int16 values, NaN and huge floats, or random bytes.  Each region draws its poison from its own seed, so
that it never looks like a continuation of the row before it.  `guard_fill` is the pattern an output buffer holds before
a call; `check_guards` names the first byte outside the declared rows that the call changed.

Offsets and strides are whole elements (`unit` dtype elements: 2 for an int16 or float IQ pair), never part of one.
"""
import numpy as np

GUARD = np.array([0xA5, 0x5A, 0xC3, 0x3C, 0x96, 0x69, 0xF0, 0x0F], np.uint8)
I16_POISON = np.array([32767, -32768, -32767], np.int16)
F32_POISON = np.array([np.nan, 3e38, -3e38, 1e30, -1e30, 7.5e9, -7.5e9], np.float32)


class Layout:
    """`rows` rows of `row` elements, row r at element lead + r * stride, `tail` elements after the last row"""

    def __init__(self, rows, row, stride=None, lead=0, tail=0, itemsize=1, unit=1):
        stride = row if stride is None else stride
        if rows < 0 or row < 0 or lead < 0 or tail < 0 or stride < row:
            raise ValueError(f"bad layout: rows={rows} row={row} stride={stride} lead={lead} tail={tail}")
        if row % unit or stride % unit or lead % unit or tail % unit:
            raise ValueError(f"row={row} stride={stride} lead={lead} tail={tail} split an element of {unit}")
        self.rows, self.row, self.stride, self.lead, self.tail = rows, row, stride, lead, tail
        self.itemsize, self.unit = itemsize, unit

    @property
    def starts(self):
        return [self.lead + r * self.stride for r in range(self.rows)]

    @property
    def nelems(self):
        body = (self.rows - 1) * self.stride + self.row if self.rows else 0
        return self.lead + body + self.tail

    @property
    def nbytes(self):
        return self.nelems * self.itemsize

    def regions(self):
        """(name, first byte, end byte) of every span that is not row data, in buffer order; empty spans are left out"""
        b = self.itemsize
        out = []
        if self.rows == 0:
            out.append(("lead", 0, self.nbytes))
        else:
            out.append(("lead", 0, self.lead * b))
            for r in range(self.rows - 1):
                end = (self.lead + r * self.stride + self.row) * b
                out.append((f"gap after row {r}", end, end + (self.stride - self.row) * b))
            end = (self.lead + (self.rows - 1) * self.stride + self.row) * b
            out.append(("tail", end, self.nbytes))
        return [(n, lo, hi) for n, lo, hi in out if hi > lo]

    def rows_of(self, flat):
        """the rows of an array whose first axis runs over the layout's elements, as an array [rows][row][...]"""
        flat = np.asarray(flat)
        assert flat.shape[0] == self.nelems, (flat.shape[0], self.nelems)
        if self.rows == 0:
            return np.zeros((0, self.row) + flat.shape[1:], flat.dtype)
        idx = np.asarray(self.starts)[:, None] + np.arange(self.row)[None, :]
        return flat[idx]


def poison(dtype, n, seed, region):
    """n elements of poison for one region: values that change a result if read, never the output guard bytes"""
    rng = np.random.default_rng([seed, region])
    dtype = np.dtype(dtype)
    if dtype == np.int16:
        return rng.choice(I16_POISON, n)
    if dtype == np.float32:
        return rng.choice(F32_POISON, n)
    if dtype == np.uint8:
        v = rng.integers(0, 256, n).astype(np.uint8)
        return np.where(np.isin(v, GUARD), v ^ 0x01, v).astype(np.uint8)  # no GUARD byte has a neighbour in GUARD
    raise TypeError(f"no poison for {dtype}")


def build_input(rows, stride=None, lead=0, tail=0, unit=1, seed=0):
    """rows: equal-length 1-D arrays of one dtype -> (the host array to upload, each row's element position)"""
    rows = [np.ascontiguousarray(r).ravel() for r in rows]
    dtype = rows[0].dtype if rows else np.dtype(np.int16)
    row = rows[0].size if rows else 0
    assert all(r.dtype == dtype and r.size == row for r in rows)
    lay = Layout(len(rows), row, stride, lead, tail, dtype.itemsize, unit)
    buf = np.empty(lay.nelems, dtype)
    b = dtype.itemsize
    for k, (_, lo, hi) in enumerate(lay.regions()):
        buf[lo // b:hi // b] = poison(dtype, (hi - lo) // b, seed, k)
    for r, p in zip(rows, lay.starts):
        buf[p:p + row] = r
    return buf, lay.starts


def guard_fill(nbytes):
    """the bytes an output buffer holds before the call"""
    return np.resize(GUARD, nbytes).astype(np.uint8)


def check_guards(got, lay, what="output"):
    """got: the output buffer's bytes after the call.  Raises on the first byte outside the rows that differs from the
    guard pattern, naming its region and its offset in that region and in the buffer."""
    got = np.ascontiguousarray(got).view(np.uint8).ravel()
    assert got.size == lay.nbytes, (got.size, lay.nbytes)
    want = guard_fill(lay.nbytes)
    for name, lo, hi in lay.regions():
        bad = np.flatnonzero(got[lo:hi] != want[lo:hi])
        if bad.size:
            k = int(bad[0])
            raise AssertionError(f"{what}: {name} changed at byte {k} of {hi - lo} (buffer byte {lo + k}): "
                                 f"0x{want[lo + k]:02x} -> 0x{got[lo + k]:02x}, {bad.size} bytes changed there")
