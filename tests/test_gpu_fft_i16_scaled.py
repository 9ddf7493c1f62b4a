"""GPU: k_fft's int16 path against its float path, byte for byte, at every power-of-two frame size.

The int16 path converts with one fused multiply-add to 2^15 times the reference's float (common.h: i16_to_float_java_2p15),
runs its first pass on the scaled values and takes the factor out in the second pass's twiddles (fft_psd.hip, SC).  The float
path is handed the reference rule's floats (the oracle's conversion) and does the same arithmetic from there, so the two PSD
rows -- the n bins, the peak's Hz and its value -- must be the same bytes: for every int16 value as I and as Q, for an all-zero
frame, for full-scale frames, and with a DC correction that wraps."""
import functools

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O

pytestmark = pytest.mark.gpu

SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
CORRECTIONS = [(0, 0), (11, -7), (32767, -32768)]


@functools.lru_cache(maxsize=None)
def frames(n):
    """[65536 / n + 2][2 n] int16: every value once as I and once as Q (two different permutations), one frame of zeros, one
    frame of +32767 / -32767 / -32768 only"""
    rng = np.random.default_rng(1000 + n)
    allv = np.arange(-32768, 32768, dtype=np.int32)
    body = np.empty((65536, 2), np.int16)
    body[:, 0] = rng.permutation(allv)
    body[:, 1] = rng.permutation(allv)
    full = np.array([32767, -32767, -32768], np.int16)[rng.integers(0, 3, 2 * n)]
    full[:6] = [32767, -32768, -32768, 32767, -32767, -32767]
    out = np.concatenate([body.reshape(65536 // n, 2 * n), np.zeros((1, 2 * n), np.int16), full[None, :]])
    assert set(out[:-2, 0::2].ravel().tolist()) == set(out[:-2, 1::2].ravel().tolist()) == set(allv.tolist())
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_int16_rows_are_the_float_rows(n):
    raw = frames(n)
    nf = raw.shape[0]
    f = J.Fft(n, 96000)
    assert f.kernel_name() == "k_fft"
    d_raw = J.DeviceBuffer.from_host(raw)
    d_a, d_b = J.DeviceBuffer(nf * (n + 2) * 4), J.DeviceBuffer(nf * (n + 2) * 4)
    for ic, qc in CORRECTIONS:
        x = O.convert_i16(raw.ravel(), ic=ic, qc=qc)  # (float)(short)(s + corr) / 32767f
        d_x = J.DeviceBuffer.from_host(x)
        d_a.zero()
        d_b.zero()
        f.batch_i16(d_raw, nf, d_a, ic, qc)
        f.batch_f32(d_x, nf, d_b)
        a = d_a.to_host(np.float32).reshape(nf, n + 2)
        b = d_b.to_host(np.float32).reshape(nf, n + 2)
        for k in range(nf):
            assert a[k].tobytes() == b[k].tobytes(), (n, ic, qc, k, int((a[k].view(np.int32) != b[k].view(np.int32)).sum()))
        if (ic, qc) == (0, 0):
            assert np.all(np.isneginf(a[nf - 2, :n]))  # the zero frame: log of 0 in every bin, in both
            assert np.isfinite(a[nf - 1, n + 1]) and np.isfinite(a[:nf - 2]).all()
