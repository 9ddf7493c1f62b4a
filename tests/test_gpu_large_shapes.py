"""GPU: the batch kernels past 32-bit offsets, at the benchmark's shapes.

bench.py runs the batch kernels over buffers of tens of GB; every other test keeps its offsets below 2^31.  Here each buffer
named in a test's docstring is asserted to pass the boundary it is meant to cross, its input is built from P = 97 source
rows (row r = row r mod P, tests/big_offsets.py) so that a read or write that wraps by 2^k bytes lands on a row with other
bytes, and then:
 (b) sampled input rows are non-trivial, differ between twin classes and equal their class row;
 (c) rows around every 2^31 / 2^32 / 2^33 byte boundary (plus the first, the last, seeded random ones and a few per twin class)
     are compared with the plain reference at the suite's existing tolerances;
 (d) every output row equals its twin's, read back in pieces of at most 256 MB.
"""
import ctypes as C

import numpy as np
import pytest

import big_offsets as B
import java_sdr_amd as J
import oracle_lib as O
from test_gpu_fft import FFT_RTOL, check_psd

pytestmark = pytest.mark.gpu
P = B.P
CN = ["cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK"]
STATE_IDX = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)


def free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


def check_inputs(d_in, rows, row_bytes, stride_bytes, src):
    """(b): sampled input rows are not all zero, equal their class's source row, and the classes differ"""
    got = B.read_rows(d_in, rows, row_bytes, stride_bytes)
    for r, v in got.items():
        assert v.any(), f"input row {r} is all zero"
        assert np.array_equal(v, src[B.twin(r)].view(np.uint8)[:row_bytes]), f"input row {r} is not its twin's"
    assert not np.array_equal(src[0].view(np.uint8)[:row_bytes], src[1].view(np.uint8)[:row_bytes])
    assert not np.array_equal(src[B.twin(rows[-1])].view(np.uint8)[:row_bytes], src[B.twin(rows[-1]) - 1].view(np.uint8)[:row_bytes])


def sample_rows(nrows, row_bytes, elem_bytes, stride_bytes=None, extra=6):
    return sorted(set(B.boundary_rows(nrows, row_bytes, elem_bytes, stride_bytes, extra=extra)) | set(B.class_rows(nrows)))


def tone_source(n, seed):
    """P frames of k_synth_tones (1-3 tones + noise), made on the device, as host int16 [P][2n]"""
    ct, _ = O.synth_tables(6000)
    d_ct = J.DeviceBuffer.from_host(ct)
    d = J.DeviceBuffer(P * n * 4)
    try:
        J.synth_tones(d, 0, P, n, d_ct, 250, O.mix64(seed))
        return d.to_host(np.int16).reshape(P, 2 * n)
    finally:
        free(d, d_ct)


def random_source(n, seed, lo=-20000, hi=20000):
    return np.random.default_rng(seed).integers(lo, hi, (P, 2 * n)).astype(np.int16)


def dbpsk_source(L, n0, nfr, seed, stride_pairs=None):
    """P FEC-carrying DBPSK streams (the bench's generator, csrc/synth.hip): samples n0 .. n0+L of each, host int16 [P][2*stride]
    (zero padding after the samples), and the payloads [P][nfr][256]"""
    stride_pairs = stride_pairs or L
    pay = J.synth_payloads(seed, 0, P, nfr)
    d_sym = J.DeviceBuffer(P * nfr * 5200)
    d_ds = J.DeviceBuffer(P * nfr * 5200)
    ct, st = O.synth_tables(3000)
    d_ct, d_st = J.DeviceBuffer.from_host(ct), J.DeviceBuffer.from_host(st)
    keys = np.array([O.mix64((seed * 0x9E3779B1 + s) ^ 0xA5A5A5A5) for s in range(P)], np.uint64)
    d_keys = J.DeviceBuffer.from_host(keys)
    d_iq = J.DeviceBuffer(P * stride_pairs * 4)
    try:
        J.fec_encode_dev(pay, P * nfr, d_sym)
        J.synth_diffsign(d_sym, nfr * 5200, P, d_ds)
        d_iq.zero()
        gain = int(round(1500.0 / 37837.0 * 32768.0))
        J.synth_dbpsk(d_iq, 2 * stride_pairs, P, n0, L, d_ds, nfr * 5200, 80, 0, O.phase_inc_u32(13200.0, 96000), d_ct, d_st,
                      gain, d_keys)
        return d_iq.to_host(np.int16).reshape(P, 2 * stride_pairs), pay.to_host(np.uint8).reshape(P, nfr, 256)
    finally:
        free(pay, d_sym, d_ds, d_ct, d_st, d_keys, d_iq)


# ------------------------------------------------------------------ fft.java: k_fft and the waterfall
def test_fft_psd_config2_past_2_to_33_bytes_and_its_waterfall():
    """k_fft at n = 2048 over 1 081 344 int16 frames: d_in 8.86 GB and d_psd 8.87 GB both cross 2^31, 2^32 and 2^33 bytes
    (d_psd also 2^31 float elements); the grid strides (workgroups < work items).  Then k_waterfall at width 1280 over that
    PSD: d_pix 5.5 GB crosses 2^31 and 2^32 bytes.  Sampled PSD rows against O.fft_receive (check_psd), sampled pixel rows
    bit-exact against O.waterfall_line, every row of both against its twin."""
    n, nfr, width = 2048, 1081344, 1280
    src = tone_source(n, 20261016)
    f = J.Fft(n, 96000)
    d_in = d_psd = d_pix = None
    try:
        d_in = J.DeviceBuffer(nfr * 4 * n)
        d_psd = J.DeviceBuffer(nfr * 4 * (n + 2))
        assert d_in.nbytes > 2 ** 33 and d_psd.nbytes > 2 ** 33
        B.fill_periodic(d_in, src, nfr)
        rows_in = sample_rows(nfr, 4 * n, 2)
        check_inputs(d_in, rows_in, 4 * n, None, src)
        f.batch_i16(d_in, nfr, d_psd)
        J.binding.stream_sync()
        assert f.kernel_name() == "k_fft", f.kernel_name()
        wi, wg = f.last_launch()
        assert wg < wi, (wi, wg)
        rows = sorted(set(rows_in) | set(sample_rows(nfr, 4 * (n + 2), 4)))
        got = B.read_rows(d_psd, rows, 4 * (n + 2), dtype=np.float32)
        refs = {c: O.fft_receive(O.convert_i16(src[c]), 96000) for c in {B.twin(r) for r in rows}}
        for r in rows:
            check_psd(got[r], refs[B.twin(r)], n, 96000)
        B.check_twins(d_psd, nfr, 4 * (n + 2), what="psd row")
        # the waterfall of that PSD
        free(d_in)
        d_in = None
        d_pix = J.DeviceBuffer(nfr * 4 * width)
        assert d_pix.nbytes > 2 ** 32
        J.waterfall_lines_dev(d_psd, nfr, n, width, d_pix)
        J.binding.stream_sync()
        rows = sorted(set(rows) | set(sample_rows(nfr, 4 * width, 4)))
        psd = B.read_rows(d_psd, rows, 4 * (n + 2), dtype=np.float32)
        pix = B.read_rows(d_pix, rows, 4 * width, dtype=np.uint32)
        for r in rows:
            assert np.array_equal(pix[r], O.waterfall_line(psd[r], n, width)), f"waterfall row {r}"
        B.check_twins(d_pix, nfr, 4 * width, what="pixel row")
    finally:
        free(d_in, d_psd, d_pix)
        del f


def test_float_input_path_past_2_to_33_bytes():
    """jsdr_convert_i16 then jsdr_fft_spectrum_f32 and jsdr_fft_batch_f32 at n = 2048 over 540 672 frames: the float (I,Q)
    buffer d_f (8.86 GB, 2^31 floats at 2^33 B) and the spectrum d_spec (8.86 GB) cross 2^31, 2^32 and 2^33 bytes; the int16
    input (4.43 GB) and the PSD (4.43 GB) cross 2^31 and 2^32.  Converted rows bit-exact against O.convert_i16, spectra
    within 1e-5 of the peak of numpy's float64 FFT, PSD rows by check_psd, every row of all three outputs against its twin."""
    n, nfr = 2048, 540672
    src = tone_source(n, 20261017)
    f = J.Fft(n, 96000)
    d_in = d_f = d_spec = d_psd = None
    lib = J.lib()
    try:
        d_in = J.DeviceBuffer(nfr * 4 * n)
        d_f = J.DeviceBuffer(nfr * 8 * n)
        d_spec = J.DeviceBuffer(nfr * 8 * n)
        d_psd = J.DeviceBuffer(nfr * 4 * (n + 2))
        assert d_f.nbytes > 2 ** 33 and d_spec.nbytes > 2 ** 33 and d_in.nbytes > 2 ** 32 and d_psd.nbytes > 2 ** 32
        B.fill_periodic(d_in, src, nfr)
        rows = sorted(set(sample_rows(nfr, 8 * n, 4)) | set(sample_rows(nfr, 4 * n, 2)) | set(sample_rows(nfr, 4 * (n + 2), 4)))
        check_inputs(d_in, rows, 4 * n, None, src)
        J.binding._check(lib.jsdr_convert_i16(C.c_void_p(d_in.ptr), C.c_int64(nfr * n), 2, 0, 0, C.c_void_p(d_f.ptr), None),
                         "jsdr_convert_i16")
        J.binding._check(lib.jsdr_fft_spectrum_f32(f.h, C.c_void_p(d_f.ptr), C.c_int64(nfr), C.c_void_p(d_spec.ptr), None),
                         "jsdr_fft_spectrum_f32")
        f.batch_f32(d_f, nfr, d_psd)
        J.binding.stream_sync()
        bufs = {c: O.convert_i16(src[c]) for c in range(P)}
        conv = B.read_rows(d_f, rows, 8 * n, dtype=np.float32)
        spec = B.read_rows(d_spec, rows, 8 * n, dtype=np.float32)
        psd = B.read_rows(d_psd, rows, 4 * (n + 2), dtype=np.float32)
        for r in rows:
            c = B.twin(r)
            assert np.array_equal(conv[r], bufs[c]), f"converted row {r}"
            x = bufs[c].astype(np.float64)
            want = np.fft.fft(x[0::2] + 1j * x[1::2])
            got = spec[r][0::2].astype(np.float64) + 1j * spec[r][1::2].astype(np.float64)
            assert np.abs(got - want).max() <= FFT_RTOL * np.abs(want).max(), f"spectrum row {r}"
            check_psd(psd[r], O.fft_receive(bufs[c], 96000), n, 96000)
        B.check_twins(d_f, nfr, 8 * n, what="converted row")
        B.check_twins(d_spec, nfr, 8 * n, what="spectrum row")
        B.check_twins(d_psd, nfr, 4 * (n + 2), what="psd row")
    finally:
        free(d_in, d_f, d_spec, d_psd)
        del f


@pytest.mark.parametrize("n,rate,nfr,kernel,cross", [
    (9600, 96000, 224000, "k_fft_mixed", 2 ** 33),
    (19200, 192000, 112000, "k_fft_mixed_dual", 2 ** 33),
    (4410, 44100, 487000, "k_fft_rt", 2 ** 33),
    # the direct DFT is O(n^2): 10.7 M frames of 101 keep it short and cross 2^32 bytes (not 2^33) in and out
    (101, 1010, 10700000, "k_dft_any", 2 ** 32),
])
def test_fft_other_frame_sizes_past_32_bit_offsets(n, rate, nfr, kernel, cross):
    """k_fft_mixed (9600), k_fft_mixed_dual (19200), k_fft_rt (4410) over int16 frames: d_in and d_psd both cross 2^31, 2^32
    and 2^33 bytes; k_dft_any (101): d_in 4.3 GB and d_psd 4.4 GB cross 2^31 and 2^32 bytes.  Raw frames with DC correction;
    sampled PSD rows against numpy's float64 FFT (1e-5 of the peak) and O.fft_receive (check_psd, on a few rows: the oracle's
    DFT is O(n^2)); every PSD row against its twin."""
    src = random_source(n, n)
    f = J.Fft(n, rate)
    d_in = d_psd = None
    try:
        assert f.kernel_name() == kernel, f.kernel_name()
        d_in = J.DeviceBuffer(nfr * 4 * n)
        d_psd = J.DeviceBuffer(nfr * 4 * (n + 2))
        assert d_in.nbytes > cross and d_psd.nbytes > cross
        B.fill_periodic(d_in, src, nfr)
        rows = sorted(set(sample_rows(nfr, 4 * n, 2)) | set(sample_rows(nfr, 4 * (n + 2), 4)))
        check_inputs(d_in, rows, 4 * n, None, src)
        f.batch_i16(d_in, nfr, d_psd, ic=11, qc=-7)
        J.binding.stream_sync()
        psd = B.read_rows(d_psd, rows, 4 * (n + 2), dtype=np.float32)
        oracle_done = set()
        for r in rows:
            c = B.twin(r)
            x = O.convert_i16(src[c], ic=11, qc=-7).astype(np.float64)
            pw = np.sqrt(np.abs(np.fft.fft(x[0::2] + 1j * x[1::2])) ** 2 * (2.0 / n) ** 2)
            assert np.abs(10.0 ** (psd[r][:n].astype(np.float64) / 20) - pw).max() <= FFT_RTOL * pw.max(), f"psd row {r}"
            if c not in oracle_done and len(oracle_done) < (2 if n > 4410 else 6):
                check_psd(psd[r], O.fft_receive(O.convert_i16(src[c], ic=11, qc=-7), rate), n, rate)
                oracle_done.add(c)
        B.check_twins(d_psd, nfr, 4 * (n + 2), what="psd row")
    finally:
        free(d_in, d_psd)
        del f


# ------------------------------------------------------------------ config 3: batched FIR + decimate
@pytest.mark.parametrize("ntaps,decim", [(27, 10), (33, 3)])
def test_fir_batch_config3_past_2_to_33_bytes(ntaps, decim):
    """jsdr_fir_batch_decimate_i16 over 2100 streams x 2^20 samples at a padded stride of 2L + 2*4099 int16, so that the
    boundaries cut through rows: d_in 8.84 GB crosses 2^31, 2^32 and 2^33 bytes.  27 taps / 10 (HOWARD's down-sampler, the
    register-blocked k_fir_batch<27,10,4>): d_out [2100][104 870] double2 (out stride > nout) is 3.5 GB and crosses 2^31
    bytes; 33 taps / 3 (the generic kernel): d_out [2100][349 538] double2 is 11.7 GB and crosses 2^33 bytes.  Sampled
    streams bit-exact against O.fir_decimate, every stream's outputs against its twin's."""
    S, L = 2100, 1 << 20
    stride = 2 * L + 2 * 4099
    src, _ = dbpsk_source(L, 0, 6, 20261018, stride_pairs=stride // 2)
    taps = O.bpsk_table(0) if ntaps == 27 else np.random.default_rng(33).standard_normal(33)
    assert taps.size == ntaps  # the kernel is picked by (ntaps, decim): 27 / 10 is the register-blocked one
    scale = 1.25
    nout = L // decim
    ostride = nout + 13
    d_in = d_out = None
    try:
        d_in = J.DeviceBuffer(S * 2 * stride)
        d_out = J.DeviceBuffer(S * ostride * 16)
        assert d_in.nbytes > 2 ** 33 and d_out.nbytes > (2 ** 31 if ntaps == 27 else 2 ** 33)
        B.fill_periodic(d_in, src, S)
        rows = sample_rows(S, 4 * L, 2, stride_bytes=2 * stride)
        rows = sorted(set(rows) | set(sample_rows(S, 16 * nout, 8, stride_bytes=16 * ostride)))
        check_inputs(d_in, rows, 4 * L, 2 * stride, src)
        got_n = J.fir_batch_decimate_i16(d_in, S, stride, L, taps, decim, scale, d_out, ostride)
        J.binding.stream_sync()
        assert got_n == nout
        got = B.read_rows(d_out, rows, 16 * nout, 16 * ostride, dtype=np.float64)
        refs = {}
        for r in rows:
            c = B.twin(r)
            if c not in refs:
                refs[c] = O.fir_decimate(src[c][:2 * L], taps, decim, scale)
            assert got[r].tobytes() == refs[c].tobytes(), f"stream {r}"
        B.check_twins(d_out, S, 16 * nout, stride_bytes=16 * ostride, what="stream")
    finally:
        free(d_in, d_out)


# ------------------------------------------------------------------ demod.java, batched
@pytest.mark.parametrize("mode", [2, 3])
def test_demod_batch_past_2_to_33_bytes(mode):
    """jsdr_demod_batch_i16 over 2176 streams x 2^20 samples (512 frames of 2048) in one call: the float detector buffer
    d[S][L] (9.1 GB, 2^31 floats at 2^33 B) and the int16 stereo audio d_audio [S][2L] (9.1 GB) cross 2^31, 2^32 and 2^33
    bytes, as does d_in.  AM takes k_demod_front + k_demod_out (mean subtraction) through d[S][L]; NFM takes the fused kernel,
    which never touches d, so only the AM case covers that buffer (NFM covers d_in and d_audio).  Sampled streams'
    audio bit-exact against O.Demod frame by frame, and their last frame's max / mean; every stream's audio against its twin."""
    S, L, n = 2176, 1 << 20, 2048
    src, _ = dbpsk_source(L, 0, 6, 20261019)
    d = J.Demod(rate=96000, n=n, nstreams=S, max_batch_samples=L)
    d.configure(mode, 1, 1, 1)
    w, _ = d.weights(3000, 11000)
    d_in = d_audio = None
    try:
        assert S * L * 4 > 2 ** 33
        d_in = J.DeviceBuffer(S * 4 * L)
        d_audio = J.DeviceBuffer(S * 4 * L)
        assert d_in.nbytes > 2 ** 33 and d_audio.nbytes > 2 ** 33
        B.fill_periodic(d_in, src, S)
        rows = sample_rows(S, 4 * L, 4, extra=1)
        check_inputs(d_in, rows, 4 * L, None, src)
        d.profile_enable(True)
        d.batch_i16(d_in, 2 * L, L, d_audio, 2 * L)
        J.binding.stream_sync()
        prof = d.profile_read()
        d.profile_enable(False)
        assert prof["k_demod_front"][1] > 0
        assert (prof["k_demod_out"][1] > 0) == (mode == 2), prof
        got = B.read_rows(d_audio, rows, 4 * L, dtype=np.int16)
        for r in rows:
            o = O.Demod(96000)
            o.configure(mode, 1, 1, 1)
            ow, _ = o.weights(3000, 11000)
            assert np.array_equal(w, ow)
            buf = O.convert_i16(src[B.twin(r)])
            for k in range(L // n):
                want = o.receive(buf[2 * k * n:2 * (k + 1) * n])
                assert np.array_equal(got[r][2 * k * n:2 * (k + 1) * n], want), f"stream {r} frame {k}"
            mx, av = d.frame_stats(r)
            assert mx == o.max and av == o.avg, (r, mx, o.max, av, o.avg)
        B.check_twins(d_audio, S, 4 * L, what="audio row")
    finally:
        free(d_in, d_audio)
        del d


# ------------------------------------------------------------------ FECDecoder.java, batched
def test_fec_batch_past_2_to_32_bytes():
    """jsdr_fec_encode_batch / jsdr_fec_decode_batch over 830 000 blocks: the symbol buffer d_sym (4.3 GB) crosses 2^31 and
    2^32 bytes.  Symbol errors go into the blocks holding bytes 2^31 - 1, 2^31, 2^32 - 1 and 2^32 and a few others.  Every
    block's decoded bytes equal its payload, the clean blocks' rc is 0, the corrupted blocks' rc and bytes equal O.fec_decode's;
    every encoded block equals its twin's."""
    nb = 830000
    pay = J.synth_payloads(20261020, 0, P, 1)
    payloads = pay.to_host(np.uint8).reshape(P, 256)
    d_pay = d_sym = d_out = d_rc = None
    try:
        d_pay = J.DeviceBuffer(nb * 256)
        d_sym = J.DeviceBuffer(nb * 5200)
        d_out = J.DeviceBuffer(nb * 256)
        d_rc = J.DeviceBuffer(nb * 4)
        assert d_sym.nbytes > 2 ** 32
        B.fill_periodic(d_pay, payloads, nb)
        J.fec_encode_dev(d_pay, nb, d_sym)
        J.binding.stream_sync()
        rows = sample_rows(nb, 5200, 1, extra=4)
        syms = B.read_rows(d_sym, rows, 5200)
        for r in rows:
            assert np.array_equal(syms[r], O.fec_encode(payloads[B.twin(r)])), f"encoded block {r}"
        B.check_twins(d_sym, nb, 5200, what="encoded block")
        # hard symbols -> soft bytes with errors in the blocks at the boundaries
        soft_cls = np.where(np.stack([O.fec_encode(p) for p in payloads]) == 1, 0xC0, 0x40).astype(np.uint8)
        B.fill_periodic(d_sym, soft_cls, nb)
        rng = np.random.default_rng(7)
        bad = sorted({(2 ** 31 - 1) // 5200, 2 ** 31 // 5200, (2 ** 32 - 1) // 5200, 2 ** 32 // 5200, 1, nb - 1, 500001})
        corrupt = {}
        for i, blk in enumerate(bad):
            raw = soft_cls[B.twin(blk)].copy()
            raw[rng.choice(5200, (40, 200, 600)[i % 3], replace=False)] ^= 0x80
            corrupt[blk] = raw
            J.binding._check(J.lib().jsdr_memcpy_h2d(C.c_void_p(d_sym.ptr + blk * 5200), raw.ctypes.data_as(C.c_void_p),
                                                     C.c_size_t(5200)), "h2d")
        d_out.zero()
        J.fec_decode_dev(d_sym, nb, d_out, d_rc)
        J.binding.stream_sync()
        rc = d_rc.to_host(np.int32)
        out = d_out.to_host(np.uint8).reshape(nb, 256)
        want = payloads[np.arange(nb) % P]
        clean = np.ones(nb, bool)
        clean[bad] = False
        assert (rc[clean] == 0).all(), np.flatnonzero(clean & (rc != 0))[:10]
        ok = (out == want).all(axis=1)
        assert ok[clean].all(), np.flatnonzero(clean & ~ok)[:10]
        for blk, raw in corrupt.items():
            orc, oout = O.fec_decode(raw)
            assert rc[blk] == orc, (blk, rc[blk], orc)
            if orc >= 0:
                assert np.array_equal(out[blk], oout) and np.array_equal(out[blk], want[blk]), blk
    finally:
        free(pay, d_pay, d_sym, d_out, d_rc)


# ------------------------------------------------------------------ FUNcubeBPSKDemod.java at the bench's shape
def oracle_rows(nrows, row_bytes, stride_bytes, sampled):
    """the rows holding bytes B-1 and B of every boundary inside the buffer, row 0, the last row, two class rows"""
    out = {0, nrows - 1}
    for b in B.boundaries(4):
        if b < B.buffer_bytes(nrows, row_bytes, stride_bytes):
            out.update({(b - 1) // stride_bytes, b // stride_bytes})
    out.update(B.class_rows(nrows)[:2])
    assert out <= set(sampled)
    return sorted(out)


def replay(iqs, trace, **kw):
    o = O.Bpsk(trace=trace, **kw)
    for iq in iqs:
        o.receive_i16(iq)
    return o


def check_against_oracle(dem, s, bits, trace, fec, o, fft=False):
    """stream s of the handle against its oracle: bits, (fi,fq) trace, FEC results, counters, state, decoded bytes (and the
    FFT-acquire centre bin and its state doubles)"""
    assert np.array_equal(np.concatenate(bits), o.bits()), f"stream {s}: bits differ"
    assert np.concatenate(trace).tobytes() == o.trace().tobytes(), f"stream {s}: (fi,fq) differ"
    fo = o.fec_results()
    assert len(fec) == len(fo), (s, len(fec), len(fo))
    for (rc, _, data), (orc, _, odata) in zip(fec, fo):
        assert rc == orc and np.array_equal(data, odata), s
    cg, co = dem.counters(s), o.counters()
    names = CN + ["centreBin"] if fft else CN
    assert [cg[k] for k in names] == [co[k] for k in names], (s, cg, co)
    gs, os_ = dem.state(s), o.state()
    for i in STATE_IDX + ((6, 7) if fft else ()):
        assert gs[i] == os_[i], (s, i, gs[i], os_[i])
    assert np.array_equal(dem.decoded(s), o.decoded()), s


def test_bpsk_tune_bench_shape_past_2_to_33_pairs():
    """The benchmark's demodulator shape: 8192 streams x 2^20 samples per call, two calls (the second's input generated from
    n0 = L into the same buffer), stride 2L + 2*4099 int16: d_in is 34.5 GB, its sample-pair index runs past 2^33 and its
    byte offsets past 2^34 (2^31, 2^32 and 2^33 B and 2^31 / 2^32 pairs all inside); k_fm, k_tail8 and the batch FEC decoder.
    Sampled streams against O.Bpsk: bits, (fi,fq) trace, counters, every state double, FEC bytes; every stream's payloads out
    of pack_slots, and every stream's slot equal to its twin's."""
    S, L, nfr = 8192, 1 << 20, 6
    stride = 2 * L + 2 * 4099
    src1, payloads = dbpsk_source(L, 0, nfr, 20261021, stride_pairs=stride // 2)
    src2, _ = dbpsk_source(L, L, nfr, 20261021, stride_pairs=stride // 2)
    dem = J.Bpsk(nstreams=S, max_batch_samples=L)
    d_in = slots = None
    rows = sample_rows(S, 4 * L, 4, stride_bytes=2 * stride, extra=2)
    assert len(rows) <= 24
    bits = {s: [] for s in rows}
    trace = {s: [] for s in rows}
    fec = {s: [] for s in rows}
    nfec = np.zeros(S, np.int64)
    try:
        d_in = J.DeviceBuffer(S * 2 * stride)
        assert d_in.nbytes > 2 ** 34 and (S - 1) * (stride // 2) + L > 2 ** 33
        info = None
        for src in (src1, src2):
            B.fill_periodic(d_in, src, S)
            check_inputs(d_in, rows, 4 * L, 2 * stride, src)
            dem.batch_i16(d_in, stride, L)
            assert dem.front_kernel_name() == "k_fm", dem.front_kernel_name()
            assert dem.tail_kernel_name() == "k_tail8", dem.tail_kernel_name()
            assert "k_vitq" in dem.fec_kernel_name(), dem.fec_kernel_name()
            for s in rows:
                bits[s].append(dem.bits(s).copy())
                trace[s].append(dem.trace(s).copy())
                fec[s].extend(dem.fec_results(s))
            info = dem.slot_info()
            if slots is None:
                slots = J.DeviceBuffer(S * info["slot_bytes"])
            dem.pack_slots(slots)
            J.binding.stream_sync()
            B.check_twins(slots, S, info["slot_bytes"], what="slot of stream")
            blob = slots.to_host(np.uint8).reshape(S, info["slot_bytes"])
            for s in range(S):
                for rc, _, data in J.sharding.unpack_slot(blob[s], info)["fec"]:
                    if rc >= 0:
                        assert np.array_equal(data, payloads[B.twin(s), nfec[s]]), (s, rc, nfec[s])
                        nfec[s] += 1
        assert nfec.min() >= 3, np.flatnonzero(nfec < 3)[:10]
        # the oracle replays the streams holding the bytes on either side of every boundary, the first and the last, and two
        # rows of other twin classes (about 12 streams)
        for s in oracle_rows(S, 4 * L, 2 * stride, rows):
            c = B.twin(s)
            check_against_oracle(dem, s, bits[s], trace[s], fec[s], replay([src1[c][:2 * L], src2[c][:2 * L]], trace=2 * L // 10 + 8))
    finally:
        free(d_in, slots)
        del dem


def acq3_scratch_per_frame(n, do_up=0):
    """bytes of FFT-acquire scratch per (stream, frame) of a three-phase launch (csrc/bpsk_acq.hip acq3_layout and
    acq3_frame_bytes, + 64): nsb double2 band bins, na doubles of |X|, the peak (16), 16, 52 edge doubles"""
    beg, end = (n // 4, n // 2) if do_up else (0, n // 4)
    nsb = max(204, 204 + (n // 2 + 28 - (n // 4 - 26)) if do_up else n // 4 + 28)
    na = max(2, ((end - beg - 150) + 1) & ~1)
    return 16 * nsb + 8 * na + 16 + 16 + 8 * 52 + 64, nsb


@pytest.mark.parametrize("n,L,front,payloads", [(2048, 1 << 20, "k_acq_fwd", False), (9600, 1046400, "k_acqm_fwd", True)])
def test_bpsk_fft_acquire_8192_streams_in_scratch_chunks(n, L, front, payloads, monkeypatch):
    """FFT-acquire (do_fft = 1) over 8192 streams in one call at stride 2L: d_in [8192][L] int16 pairs is 34.4 GB (n = 2048,
    L = 2^20, config 4) or 34.3 GB (n = 9600, L = 1 046 400 = 109 frames), past 2^31 / 2^32 / 2^33 bytes and 2^31 / 2^32 pairs.
    The three-phase kernels' scratch is capped at 6 GiB, so the call runs in several launches of `chunk` frames per stream:
      n = 2048: 540 band bins, 362 |X| doubles: 16*540 + 8*362 + 448 + 64 = 12 048 B per frame; chunk = floor(6 GiB / (12 048 *
                8192)) = 65; ceil(512 / 65) = 8 launches.  The band spectrum a.spec is 16 * 540 * 8192 * 65 = 4.6 GB: g * a.nsb
                (g = s * 65 + f) passes 2^32 bytes.
      n = 9600: 2428 bins, 2250 doubles: 57 360 B per frame; chunk = 13; ceil(109 / 13) = 9 launches; the scratch is 6.1 GB.
    n = 2048 runs k_acq_fwd / k_acq_inv, which the handle takes by itself; n = 9600 runs k_acqm_fwd / k_acqm_inv (JSDR_ACQ3=1:
    where streams fill the chip the handle picks the fused k_front_fftm instead).  The launch count is read from the handle's
    profile.  The streams either side of every boundary, the first, the last and two class rows against O.Bpsk(do_fft=1):
    bits, (fi,fq), FEC, counters, centre bin, state; every stream's slot against its twin's; at n = 9600 also every stream's
    decoded payloads, in order, plus the first stream that decodes none replayed by the oracle (at 2048 the block-wise filter's
    seams keep FEC blocks from decoding, as bench.py notes)."""
    S, nfr = 8192, 3
    if n == 9600:
        monkeypatch.setenv("JSDR_ACQ3", "1")
    per, nsb = acq3_scratch_per_frame(n)
    chunk = min((6144 << 20) // (per * S), L // n)
    nlaunch = -(-(L // n) // chunk)
    assert nlaunch >= 8 and per * S * chunk > 2 ** 32
    if n == 2048:
        assert 16 * nsb * S * chunk > 2 ** 32
    src, pay = dbpsk_source(L, 0, nfr, 20261022 + n)
    dem = J.Bpsk(rate=96000, blen=4 * n, do_fft=1, nstreams=S, max_batch_samples=L)
    d_in = slots = None
    rows = sample_rows(S, 4 * L, 4, extra=2)
    try:
        d_in = J.DeviceBuffer(S * 4 * L)
        assert d_in.nbytes > 2 ** 34
        B.fill_periodic(d_in, src, S)
        check_inputs(d_in, rows, 4 * L, None, src)
        dem.profile_enable(True)
        dem.batch_i16(d_in, 2 * L, L)
        dem.sync()
        prof = dem.profile_read()
        dem.profile_enable(False)
        assert dem.front_kernel_name() == front, dem.front_kernel_name()
        assert prof["k_acq_fwd"][1] == nlaunch and prof["k_acq_inv"][1] == nlaunch, (nlaunch, prof["k_acq_fwd"], prof["k_acq_inv"])
        info = dem.slot_info()
        slots = J.DeviceBuffer(S * info["slot_bytes"])
        dem.pack_slots(slots)
        J.binding.stream_sync()
        B.check_twins(slots, S, info["slot_bytes"], what="slot of stream")
        if payloads:
            blob = slots.to_host(np.uint8).reshape(S, info["slot_bytes"])
            nfec = np.zeros(S, np.int64)
            for s in range(S):
                for rc, _, data in J.sharding.unpack_slot(blob[s], info)["fec"]:
                    if rc >= 0:
                        assert np.array_equal(data, pay[B.twin(s), nfec[s]]), (s, rc, nfec[s])
                        nfec[s] += 1
            # (a few payload classes decode no FEC block in this one call; that this is the reference's behaviour too is checked
            #  by replaying the first such stream in the oracle below)
            assert (nfec >= 1).mean() > 0.8 and nfec.max() >= 2, np.bincount(nfec)
            silent = [int(v) for v in np.flatnonzero(nfec == 0)[:1]]
        else:
            silent = []
        for s in sorted(set(oracle_rows(S, 4 * L, 4 * L, rows)) | set(silent)):
            o = replay([src[B.twin(s)]], trace=L // 10 + 8, blen=4 * n, do_fft=1)
            check_against_oracle(dem, s, [dem.bits(s)], [dem.trace(s)], dem.fec_results(s), o, fft=True)
    finally:
        free(d_in, slots)
        del dem
