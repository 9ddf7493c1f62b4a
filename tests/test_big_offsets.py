"""CPU: the row picker and the twin comparator of tests/big_offsets.py.  A picker that quietly returned [0, last] would leave
every large-shape GPU test without teeth, so its boundary rows are checked against the byte arithmetic here."""
import numpy as np
import pytest

import big_offsets as B

CONFIG2_FRAMES = 1081344  # tests/test_gpu_large_shapes.py: k_fft at n = 2048, int16 in, float[n + 2] out


def covering(rows, stride, row_bytes, b):
    """rows whose bytes [r*stride, r*stride + row_bytes) hold byte b"""
    return [r for r in rows if r * stride <= b < r * stride + row_bytes]


@pytest.mark.parametrize("nrows,row_bytes,elem_bytes", [(CONFIG2_FRAMES, 4 * (2048 + 2), 4), (CONFIG2_FRAMES, 4 * 2048, 2),
                                                         (CONFIG2_FRAMES, 8 * 2048, 8), (CONFIG2_FRAMES, 1280 * 4, 4),
                                                         (10700000, 4 * (101 + 2), 4), (10700000, 4 * 101, 2)])
def test_every_boundary_at_the_config2_shape_has_rows_on_both_sides(nrows, row_bytes, elem_bytes):
    """the config-2 PSD, its input, the float input, the waterfall, and the direct DFT's 101-sample frames (412 / 404-byte rows,
    not multiples of 8)"""
    total = B.buffer_bytes(nrows, row_bytes)
    rows = B.boundary_rows(nrows, row_bytes, elem_bytes, extra=0)
    assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == nrows - 1
    inside = [b for b in B.boundaries(elem_bytes) if b < total]
    assert 2 ** 31 in inside and 2 ** 32 in inside  # the shape is meant to cross both
    straddled = 0
    for b in inside:
        lo, hi = covering(rows, row_bytes, row_bytes, b - 1), covering(rows, row_bytes, row_bytes, b)
        assert lo and hi, (b, row_bytes)
        r = hi[0]
        assert r - 1 in rows and (r + 1 in rows or r + 1 == nrows)
        if row_bytes & (row_bytes - 1):  # a row size that is not a power of two: one row holds both bytes, it straddles B
            assert lo == hi and r * row_bytes < b < (r + 1) * row_bytes, (b, row_bytes, lo, hi)
            straddled += 1
        else:  # a power of two: B is the first byte of row r, and row r - 1 ends at B - 1
            assert lo == [r - 1] and r * row_bytes == b
    assert straddled == (len(inside) if row_bytes & (row_bytes - 1) else 0)


def test_straddling_rows_with_a_padded_stride():
    L = 1 << 20
    row, stride = 4 * L, 4 * L + 4 * 4099
    rows = B.boundary_rows(8192, row, 4, stride_bytes=stride, extra=0)
    for b in B.boundaries(4):
        s = b // stride
        assert {s - 1, s, s + 1} <= set(rows), b
        s = (b - 1) // stride
        assert s in rows


def test_rows_at_exact_multiples_give_the_row_before_and_the_row_at():
    row = 8192  # 2^13: 2^31 B is the first byte of row 2^18
    rows = B.boundary_rows(CONFIG2_FRAMES, row, 2, extra=0)
    for k in (31, 32, 33):
        s = 2 ** k // row
        if 2 ** k < CONFIG2_FRAMES * row:
            assert s - 1 in rows and s in rows, k
            assert s * row == 2 ** k and covering(rows, row, row, 2 ** k - 1) == [s - 1]


def test_boundaries_past_the_end_are_dropped():
    rows = B.boundary_rows(1000, 4096, 4, extra=0)  # 4 MB: no boundary inside
    assert rows == [0, 999]
    nrows = (2 ** 31) // 4096 + 10  # just past 2^31 B only
    rows = B.boundary_rows(nrows, 4096, 2, extra=0)
    s = 2 ** 31 // 4096
    assert rows == [0, s - 2, s - 1, s, s + 1, nrows - 1]


def test_deterministic_for_a_seed_and_extra_rows_are_added():
    a = B.boundary_rows(CONFIG2_FRAMES, 8200, 4, extra=8, seed=5)
    assert a == B.boundary_rows(CONFIG2_FRAMES, 8200, 4, extra=8, seed=5)
    base = B.boundary_rows(CONFIG2_FRAMES, 8200, 4, extra=0)
    assert set(base) < set(a) and len(a) > len(base)
    assert a != B.boundary_rows(CONFIG2_FRAMES, 8200, 4, extra=8, seed=6)


def test_period_is_an_odd_prime_and_twins_differ_by_no_power_of_two():
    p = B.P
    assert p % 2 == 1 and all(p % q for q in range(2, int(p ** 0.5) + 1))
    for k in range(1, 40):  # a row shifted by 2^k rows never lands in its own class
        assert (2 ** k) % p != 0
    assert [B.twin(r) for r in (0, 96, 97, 98, 10 ** 9)] == [0, 96, 0, 1, 10 ** 9 % p]


class _HostBuffer:
    """stands in for a DeviceBuffer: to_host over a bytes array"""

    def __init__(self, arr):
        self.a = np.ascontiguousarray(arr).view(np.uint8).ravel()
        self.nbytes = self.a.nbytes

    def to_host(self, dtype, count=None, offset_bytes=0):
        dtype = np.dtype(dtype)
        count = (self.nbytes - offset_bytes) // dtype.itemsize if count is None else count
        return self.a[offset_bytes:offset_bytes + count * dtype.itemsize].view(dtype).copy()


def test_twin_comparator_passes_periodic_rows_and_names_a_displaced_one():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (B.P, 40), dtype=np.uint8)
    nrows, row = 1000, 32  # stride 40: 8 padding bytes per row that the comparator must ignore
    buf = np.tile(src, (nrows // B.P + 1, 1))[:nrows].copy()
    buf[:, row:] = rng.integers(0, 256, (nrows, 40 - row), dtype=np.uint8)
    flat = buf.ravel()[:B.buffer_bytes(nrows, row, 40)]
    B.check_twins(_HostBuffer(flat), nrows, row, stride_bytes=40, chunk_bytes=40 * 7)
    bad = flat.copy()
    bad[777 * 40 + 5] ^= 1
    with pytest.raises(AssertionError, match="row 777 differs from its twin"):
        B.check_twins(_HostBuffer(bad), nrows, row, stride_bytes=40, chunk_bytes=40 * 7)
    bad = flat.copy()
    bad[(nrows - 1) * 40:] = bad[(nrows - 1 - 64) * 40:(nrows - 64) * 40][:row]  # last row = a row 2^6 earlier
    with pytest.raises(AssertionError, match=f"row {nrows - 1} differs"):
        B.check_twins(_HostBuffer(bad), nrows, row, stride_bytes=40)


def test_class_rows_are_twins_of_the_named_classes():
    rows = B.class_rows(8192, per_class=2)
    assert {B.twin(r) for r in rows} == {0, 1, 48, 96} and all(r >= B.P for r in rows) and len(rows) == 8
