"""CPU: the layout builder and the guard checker of tests/layouts.py, which tests/test_gpu_layouts.py relies on to see a
read outside a row (poisoned input gaps) and a write outside one (guarded outputs)."""
import numpy as np
import pytest

import layouts as LY


def rows_i16(k, n, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(-1000, 1000, 2 * n).astype(np.int16) for _ in range(k)]


@pytest.mark.parametrize("stride_extra,lead,tail", [(0, 0, 0), (2, 2, 0), (66, 2, 8), (6, 0, 2)])
def test_builder_puts_row_r_where_the_abi_says(stride_extra, lead, tail):
    n = 37
    rows = rows_i16(5, n)
    stride = 2 * n + stride_extra
    buf, starts = LY.build_input(rows, stride, lead, tail, unit=2, seed=3)
    assert starts == [lead + r * stride for r in range(5)]
    assert buf.size == lead + 4 * stride + 2 * n + tail
    for r, p in enumerate(starts):
        assert np.array_equal(buf[p:p + 2 * n], rows[r])  # raw[s * stride + 2 t ..] = I, Q of sample t of row s
    lay = LY.Layout(5, 2 * n, stride, lead, tail, 2, 2)
    assert np.array_equal(lay.rows_of(buf), np.stack(rows))
    # every element that is not row data is poison
    mask = np.ones(buf.size, bool)
    for p in starts:
        mask[p:p + 2 * n] = False
    assert np.isin(buf[mask], LY.I16_POISON).all()


def test_float_and_byte_poison_and_region_seeds():
    rows = [np.zeros(8, np.float32) for _ in range(3)]
    buf, starts = LY.build_input(rows, 8 + 40, 2, 40, unit=2, seed=9)
    lay = LY.Layout(3, 8, 48, 2, 40, 4, 2)
    for _, lo, hi in lay.regions():
        v = buf[lo // 4:hi // 4]
        assert np.all(np.isnan(v) | (np.abs(v) >= 7.5e9))
    # the two gaps are drawn from different seeds: neither repeats the other
    g0, g1 = (buf[lo // 4:hi // 4] for n, lo, hi in lay.regions() if n.startswith("gap"))
    assert not np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    b, _ = LY.build_input([np.zeros(16, np.uint8)] * 2, 16 + 300, 4, 300, unit=4, seed=1)
    assert not np.isin(b[b != 0], LY.GUARD).any()


def test_offsets_that_split_an_element_are_refused():
    with pytest.raises(ValueError):
        LY.Layout(2, 8, 9, unit=2)
    with pytest.raises(ValueError):
        LY.Layout(2, 8, 10, lead=1, unit=2)
    with pytest.raises(ValueError):
        LY.Layout(2, 8, 6)  # stride below the row


def test_poison_never_equals_the_guard_pattern():
    words = {bytes(np.roll(LY.GUARD, -k)[:w]) for w in (1, 2, 4) for k in range(len(LY.GUARD))}
    for dtype in (np.int16, np.float32, np.uint8):
        p = LY.poison(dtype, 4096, 5, 0)
        w = p.dtype.itemsize
        assert not any(bytes(e) in words for e in p.view(np.uint8).reshape(-1, w))


def layout_cases():
    return [LY.Layout(4, 10, 13, 3, 5, 4), LY.Layout(3, 6, 8, 2, 0, 16, 2), LY.Layout(1, 7, 7, 1, 1, 1),
            LY.Layout(5, 4, 4, 0, 4, 8)]


@pytest.mark.parametrize("k", range(4))
def test_checker_passes_untouched_guards_and_any_row_data(k):
    lay = layout_cases()[k]
    got = LY.guard_fill(lay.nbytes)
    b = lay.itemsize
    for p in lay.starts:
        got[p * b:(p + lay.row) * b] = np.arange(lay.row * b) % 251
    LY.check_guards(got, lay)


@pytest.mark.parametrize("k", range(4))
def test_checker_catches_one_changed_byte_in_every_region(k):
    lay = layout_cases()[k]
    regions = lay.regions()
    assert regions
    for name, lo, hi in regions:
        for off in sorted({0, hi - lo - 1, (hi - lo) // 2}):  # the first, the last and a middle byte of the region
            got = LY.guard_fill(lay.nbytes)
            got[lo + off] ^= 0x40
            with pytest.raises(AssertionError, match=f"{name} changed at byte {off} of {hi - lo} "):
                LY.check_guards(got, lay)


def test_checker_catches_a_row_shifted_by_one_element():
    lay = LY.Layout(3, 8, 10, 2, 2, 4, 2)  # float IQ: 4 pairs per row, one pair of gap, one pair of lead and of tail
    base = LY.guard_fill(lay.nbytes)
    for shift, where in ((2, "gap after row 0 changed at byte 0 "), (-2, "lead changed at byte 0 ")):
        got = base.copy()
        for p in lay.starts:
            q = (p + shift) * 4
            got[q:q + 32] = 1
        with pytest.raises(AssertionError, match=where):
            LY.check_guards(got, lay)
    # the last row alone shifted forward lands in the tail
    got = base.copy()
    q = (lay.starts[-1] + 2) * 4
    got[q:q + 32] = 1
    with pytest.raises(AssertionError, match="tail changed at byte 0 "):
        LY.check_guards(got, lay)


def test_zero_rows_guard_the_whole_buffer():
    lay = LY.Layout(0, 0, 0, 0, 64, 16)
    assert lay.regions() == [("lead", 0, 1024)]
    got = LY.guard_fill(1024)
    LY.check_guards(got, lay)
    got[1023] = 0
    with pytest.raises(AssertionError, match="lead changed at byte 1023 "):
        LY.check_guards(got, lay)
