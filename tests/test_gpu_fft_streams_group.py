"""GPU: a group with PSD fed with stride != 2 * nsamples (the chunked calls of a longer buffer, a 2 * max_batch stride): its PSD
rows equal, bit for bit, jsdr_fft_batch_i16 of a separate handle called a stream at a time.  The group makes that PSD with one
jsdr_fft_batch_streams_i16 call; it made it with a launch a stream, so this holds before and after the switch-over."""
import numpy as np
import pytest

import java_sdr_amd as J

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stride_extra", [2 * 2048 * 2, 2 * 7])
def test_group_psd_of_strided_streams_equals_per_stream_batches(stride_extra):
    frame, streams, nf = 2048, 4, 6
    nsamples = frame * nf
    stride = 2 * nsamples + stride_extra  # int16 values between two streams' first samples
    rng = np.random.default_rng(20261020 + stride_extra)
    host = rng.integers(-12000, 12000, streams * stride).astype(np.int16)
    g = J.Group(1, streams, nsamples, with_psd=True)
    d_in = J.DeviceBuffer.from_host(host)
    d_psd = J.DeviceBuffer.from_host(np.full(streams * nf * (frame + 2) + 16, 0xDEADBEEF, np.uint32))
    g.batch_i16([d_in], stride, nsamples, 11, -7, psd_devs=[d_psd])
    g.sync()
    got = d_psd.to_host(np.uint32)
    assert (got[streams * nf * (frame + 2):] == 0xDEADBEEF).all(), "words behind the last row"
    f = J.Fft(frame, 96000)
    ref = J.DeviceBuffer(4 * nf * (frame + 2))
    for s in range(streams):
        f.batch_i16(d_in.ptr + 2 * s * stride, nf, ref, 11, -7)
        J.binding.stream_sync()
        want = ref.to_host(np.uint32)
        assert np.array_equal(got[s * nf * (frame + 2):(s + 1) * nf * (frame + 2)], want), ("stream", s)
    for d in (d_in, d_psd, ref):
        d.free()
    del g
