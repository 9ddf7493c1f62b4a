"""Helpers for the tests that push the batch kernels past 32-bit offsets (tests/test_gpu_large_shapes.py).

A large input is built from P = 97 source rows: row r of the buffer equals row r mod P.  P is an odd prime, so a read or a
write that lands 2^k bytes away from where it should never meets an identical twin row, and shows up as a difference.
`boundary_rows` picks the rows worth comparing with a reference: the first, the last, the ones on either side of every
2^31 / 2^32 / 2^33 byte (and element) boundary inside the buffer, and a few seeded random ones.  `check_twins` reads a
device buffer back in pieces of at most 256 MB and asserts that every row is byte-equal to the row of its class.
"""
import numpy as np

P = 97
CHUNK_BYTES = 256 << 20


def twin(r):
    """the class row whose bytes row r must repeat"""
    return r % P


def boundaries(elem_bytes):
    return sorted({2 ** 31, 2 ** 32, 2 ** 33, 2 ** 31 * elem_bytes, 2 ** 32 * elem_bytes})


def buffer_bytes(nrows, row_bytes, stride_bytes=None):
    stride = stride_bytes or row_bytes
    return (nrows - 1) * stride + row_bytes


def boundary_rows(nrows, row_bytes, elem_bytes, stride_bytes=None, extra=8, seed=20261016):
    """sorted row indices: 0, nrows-1, and for every boundary B (bytes) that lies inside the buffer the rows holding bytes
    B-1 and B plus one row on either side; then `extra` seeded random rows"""
    stride = stride_bytes or row_bytes
    assert nrows >= 1 and row_bytes >= 1 and stride >= row_bytes
    total = buffer_bytes(nrows, row_bytes, stride)
    rows = {0, nrows - 1}
    for b in boundaries(elem_bytes):
        if b >= total:
            continue
        lo, hi = (b - 1) // stride, b // stride
        rows.update(r for r in range(lo - 1, hi + 2) if 0 <= r < nrows)
    rng = np.random.default_rng(seed)
    rows.update(int(v) for v in rng.integers(0, nrows, extra))
    return sorted(rows)


def class_rows(nrows, per_class=1, classes=(0, 1, 48, 96)):
    """a few rows of some twin classes, away from row < P (whose class row is itself)"""
    out = set()
    for c in classes:
        r = c + P * (nrows // P - 1)
        for k in range(per_class):
            if 0 <= r - k * P < nrows:
                out.add(r - k * P)
    return sorted(out)


def tiled_block(src, max_bytes=CHUNK_BYTES):
    """src [P][stride_bytes] uint8 -> the largest whole number of periods that fits max_bytes (at least one)"""
    src = np.ascontiguousarray(src).view(np.uint8).reshape(P, -1)
    reps = max(1, max_bytes // src.nbytes)
    return np.tile(src, (reps, 1))


def fill_periodic(d_buf, src, nrows, offset_bytes=0):
    """write rows 0 .. nrows-1 of stride src.shape[1] bytes at d_buf + offset_bytes, row r = src[r % P] (src: [P][stride] uint8),
    by repeated host-to-device copies of one tiled block; the last row is cut to what the buffer holds"""
    import java_sdr_amd as J
    src = np.ascontiguousarray(src).view(np.uint8).reshape(P, -1)
    stride = src.shape[1]
    blk = tiled_block(src)
    brows = blk.shape[0]
    end = d_buf.nbytes
    r = 0
    while r < nrows:
        k = min(brows, nrows - r)
        off = offset_bytes + r * stride
        nb = min(k * stride, end - off)
        assert nb > 0 and off + nb <= end
        J.binding._check(J.lib().jsdr_memcpy_h2d(J.binding.C.c_void_p(d_buf.ptr + off), blk.ctypes.data_as(J.binding.C.c_void_p),
                                                J.binding.C.c_size_t(nb)), "h2d")
        r += k


def read_rows(d_buf, rows, row_bytes, stride_bytes=None, offset_bytes=0, dtype=np.uint8):
    """rows (host copies) of a [nrows][stride] device buffer; each row_bytes long, viewed as dtype"""
    stride = stride_bytes or row_bytes
    return {r: d_buf.to_host(np.uint8, count=row_bytes, offset_bytes=offset_bytes + r * stride).view(dtype) for r in rows}


def check_twins(d_buf, nrows, row_bytes, stride_bytes=None, offset_bytes=0, chunk_bytes=CHUNK_BYTES, what="row"):
    """every row r of the device buffer equals row r mod P byte for byte; reads at most chunk_bytes at a time"""
    stride = stride_bytes or row_bytes
    assert buffer_bytes(nrows, row_bytes, stride) + offset_bytes <= d_buf.nbytes
    ref = d_buf.to_host(np.uint8, count=buffer_bytes(min(P, nrows), row_bytes, stride), offset_bytes=offset_bytes)
    ref = np.concatenate([ref, np.zeros(stride - row_bytes, np.uint8)]).reshape(-1, stride)[:, :row_bytes]
    per = max(1, chunk_bytes // stride)
    r = P
    while r < nrows:
        k = min(per, nrows - r)
        got = d_buf.to_host(np.uint8, count=buffer_bytes(k, row_bytes, stride), offset_bytes=offset_bytes + r * stride)
        got = np.concatenate([got, np.zeros(stride - row_bytes, np.uint8)]).reshape(k, stride)[:, :row_bytes]
        cls = (r + np.arange(k)) % P
        bad = ~(got == ref[cls]).all(axis=1)
        if bad.any():
            first = r + int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{what} {first} differs from its twin {twin(first)} "
                                 f"({int(bad.sum())} of rows {r}..{r + k - 1} differ)")
        r += k
