"""GPU: every batch entry point of include/jsdr_hip.h at the padded and offset layouts the header allows, with each byte
either right or untouched (tests/layouts.py).

Inputs sit at a one-element base offset, with strides one and 33 elements longer than the row where the call takes a
stride; every byte that is not row data is poison (extreme int16 values, NaN and +-3e38), so that a read outside a row
changes a result.  Outputs are filled with a guard pattern before the call, and after it every byte outside the declared
rows must still hold it.  The rows themselves are compared with the plain reference each call already has in the suite:
the oracle, a float64 FFT, or the same call at the contiguous layout.  Shapes are small: tests/test_gpu_large_shapes.py
covers the far end."""
import os

import numpy as np
import pytest

import java_sdr_amd as J
import layouts as LY
import oracle_lib as O

from test_gpu_bpsk import same_counters, same_state
from test_gpu_bpsk_channels import check_against_oracles, mixed_input
from test_gpu_demod import fm_am_signal, same
from test_gpu_fft import FFT_RTOL, check_psd

pytestmark = pytest.mark.gpu
SH = J.sharding
CN = ["cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK"]


def upload(buf):
    return J.DeviceBuffer.from_host(buf)


class Guarded:
    """an output buffer of layout `lay`, filled with the guard pattern; `ptr` is where row 0 starts"""

    def __init__(self, lay, what):
        self.lay, self.what = lay, what
        self.dev = J.DeviceBuffer.from_host(LY.guard_fill(lay.nbytes))
        self.ptr = self.dev.ptr + lay.lead * lay.itemsize

    def rows(self, dtype):
        """check every guard byte, then return the rows [rows][row * itemsize / dtype size] viewed as dtype"""
        J.binding.stream_sync()
        raw = self.dev.to_host(np.uint8)
        LY.check_guards(raw, self.lay, self.what)
        r = self.lay.rows_of(raw.reshape(-1, self.lay.itemsize))
        return np.ascontiguousarray(r).reshape(self.lay.rows, self.lay.row * self.lay.itemsize).view(dtype)


# ------------------------------------------------------------------ jsdr_fir_batch_decimate_i16
@pytest.mark.parametrize("ntaps,decim", [(27, 10), (65, 10), (65, 1), (33, 3)])  # three register-blocked kernels, the generic one
@pytest.mark.parametrize("S,n,extra,ox", [
    (1, 2507, 2, 0),     # one row; nsamples not a multiple of 10 or 3
    (3, 2513, 2, 1),     # stride one pair longer, out_stride_pairs = nout + 1
    (5, 1999, 66, 3),    # stride 33 pairs longer, out_stride_pairs = nout + 3
    (67, 601, 2, 1),     # a row count that is no multiple of 4 or 64; the blocked kernels' last, partial wave
    (3, 20, 66, 1),      # nsamples < ntaps: every output's window reaches before the row
    (3, 7, 2, 3),        # nsamples < decim at decimation 10 (no output), nsamples < ntaps otherwise
    (3, 0, 2, 3),        # nsamples = 0: nothing may be written
])
def test_fir_batch_padded_rows_and_output_strides(ntaps, decim, S, n, extra, ox):
    """k_fir_batch reads its window with 16-byte loads from a 4-byte-aligned row start and stores the last wave's outputs
    under a predicate; k_fir_batch_generic indexes by stride_pairs.  Poisoned input gaps catch a read past a row or by
    s * 2n instead of s * stride; the guarded gaps between output rows catch a store past nout or by s * nout."""
    rng = np.random.default_rng(ntaps * 1000 + decim * 10 + S)
    rows = [rng.integers(-32768, 32768, 2 * n).astype(np.int16) for _ in range(S)]
    taps = O.bpsk_table(1)[:65] if ntaps == 65 else (O.bpsk_table(0) if ntaps == 27 else rng.standard_normal(ntaps))
    stride = 2 * n + extra
    buf, _ = LY.build_input(rows, stride, lead=2, tail=2 * 17, unit=2, seed=ntaps + S)
    d_in = upload(buf)
    nout = n // decim
    out = Guarded(LY.Layout(S, nout, nout + ox, lead=1, tail=3, itemsize=16), "fir out")
    got_n = J.fir_batch_decimate_i16(d_in.ptr + 4, S, stride, n, taps, decim, 1.25, out.ptr, nout + ox)
    assert got_n == nout
    got = out.rows(np.float64)
    for s in range(S):
        want = O.fir_decimate(rows[s], taps, decim, 1.25) if nout else np.zeros((0, 2))
        assert got[s].tobytes() == want.tobytes(), (ntaps, decim, s)


# ------------------------------------------------------------------ jsdr_demod_batch_i16 / _f32
DEMOD_LAYOUTS = [  # (streams, input stride - 2L, audio stride - 2L, audio base offset in int16, dodwn)
    (3, 0, 0, 0, 0),  # contiguous and aligned: the 16-byte stores
    (5, 0, 2, 2, 1),  # every audio row after the first starts 1 pair past a multiple of 4: the scalar stores
    (3, 2, 6, 2, 0),  # 3 pairs past
    (5, 6, 0, 2, 1),  # input rows off by 3 pairs; audio at a one-pair offset (16-byte stores at 4-byte-aligned addresses)
]


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("n", [2048, 12288])  # one tile (k_demod_fused; AM: the three-kernel path), six tiles (three-kernel path)
def test_demod_batch_i16_and_f32_padded_rows_and_audio_strides(mode, n):
    """k_demod_fused and k_demod_out choose their 16-byte store from the row index: an audio stride of 2L + 2 or 2L + 6
    sends rows to the scalar store fallbacks, which only an odd frame size reached before.  The f32 form
    (k_demod_fused<true> / k_demod_front<true>) had no batch caller at all: fed the same frames as JavaAudio's floats it
    must give exactly the int16 form's audio.  Two calls per layout, so the filter, NCO and FM state carry over."""
    rate, frames = 96000, [1, 2]
    for S, xin, xout, olead, dodwn in DEMOD_LAYOUTS:
        rng = np.random.default_rng(1000 * mode + n + S + xin)
        total = sum(frames) * n
        raws = [fm_am_signal(rng, total, rate, fc=5000.0 + 900.0 * s, seed_shift=31.0 * s) for s in range(S)]
        hs = [J.Demod(rate=rate, n=n, nstreams=S, max_batch_samples=max(frames) * n) for _ in range(2)]
        oracles = [O.Demod(rate) for _ in range(S)]
        for h in hs + oracles:
            h.configure(mode, 1, dodwn, 1)
            h.weights(3000, 11000)
        pos = 0
        for call, nf in enumerate(frames):
            L = nf * n
            chunk = [r[2 * pos:2 * (pos + L)] for r in raws]
            ftab = [O.convert_i16(c) for c in chunk]
            si = 2 * L + xin
            got = []
            for form, rows in (("i16", chunk), ("f32", ftab)):
                buf, _ = LY.build_input(rows, si, lead=2, tail=2 * 17, unit=2, seed=10 * call + len(got))
                d_in = upload(buf)
                out = Guarded(LY.Layout(S, 2 * L, 2 * L + xout, lead=olead, tail=2 * 9, itemsize=2, unit=2),
                              f"demod {form} audio (S={S}, +{xin}/+{xout}, lead {olead})")
                if form == "i16":
                    hs[0].batch_i16(d_in.ptr + 2 * 2, si, L, out.ptr, 2 * L + xout)
                else:
                    hs[1].batch_f32(d_in.ptr + 2 * 4, si, L, out.ptr, 2 * L + xout)
                got.append(out.rows(np.int16))
            assert np.array_equal(got[1], got[0]), (mode, n, S, call, "f32 form differs from the int16 form")
            for s in range(S):
                for f in range(nf):
                    want = oracles[s].receive(ftab[s][2 * f * n:2 * (f + 1) * n])
                    assert np.array_equal(got[0][s, 2 * f * n:2 * (f + 1) * n], want), (mode, n, S, xin, xout, call, s, f)
                for h in hs:
                    mx, av = h.frame_stats(s)
                    assert same(mx, oracles[s].max) and same(av, oracles[s].avg), (mode, s)
            pos += L
        if dodwn:
            assert hs[0].state()[0] == oracles[0].car and hs[1].state()[0] == oracles[0].car


# ------------------------------------------------------------------ jsdr_fft_batch_i16 / _f32 / _spectrum_f32
FFT_CASES = [  # (n, rate, nframes, kernel); k_fft takes FPB frames per workgroup: 32 at n = 64, 2 at 2048, 1 at 8192
    (64, 96000, 1, "k_fft"), (64, 96000, 31, "k_fft"), (64, 96000, 33, "k_fft"),
    (2048, 96000, 1, "k_fft"), (2048, 96000, 3, "k_fft"),
    (8192, 96000, 1, "k_fft"), (8192, 96000, 2, "k_fft"),
    (9600, 96000, 1, "k_fft_mixed"), (9600, 96000, 3, "k_fft_mixed"),
    (19200, 192000, 1, "k_fft_mixed_dual"), (19200, 192000, 3, "k_fft_mixed_dual"),
    (4410, 44100, 1, "k_fft_rt"), (4410, 44100, 3, "k_fft_rt"),
    (37, 370, 1, "k_dft_any"), (37, 370, 5, "k_dft_any"),
]


def fft_frames(n, rate, nf, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(nf * n)
    ph = 2 * np.pi * (rate / 7.3) * t / rate
    iq = np.empty(2 * nf * n)
    iq[0::2] = 9000 * np.cos(ph) + rng.standard_normal(nf * n) * 700
    iq[1::2] = 9000 * np.sin(ph) + rng.standard_normal(nf * n) * 700
    return np.clip(np.round(iq), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("n,rate,nf,kernel", FFT_CASES)
def test_fft_batch_poisoned_around_the_frames_and_guarded_psd(n, rate, nf, kernel):
    """k_fft's surplus part-workgroup (a frame count that is not a multiple of FPB) computes the last frame again: it must
    store it to the last row, never past it.  The mixed-radix, two-half, run-time-plan and direct-DFT kernels cover their
    last frame with their own predicates.  Frames start one element past the allocation and poison lies on both sides."""
    f = J.Fft(n, rate)
    assert f.kernel_name() == kernel
    raw = fft_frames(n, rate, nf, n + nf)
    flt = O.convert_i16(raw)
    psds = []
    for form, rows in (("i16", raw), ("f32", flt)):
        buf, _ = LY.build_input([rows], lead=2, tail=2 * 33, unit=2, seed=nf)
        d_in = upload(buf)
        out = Guarded(LY.Layout(nf, n + 2, lead=2, tail=2 * 5, itemsize=4), f"fft {form} psd")
        if form == "i16":
            f.batch_i16(d_in.ptr + 2 * 2, nf, out.ptr)
        else:
            f.batch_f32(d_in.ptr + 2 * 4, nf, out.ptr)
        psds.append(out.rows(np.float32))
    assert psds[0].tobytes() == psds[1].tobytes()
    for k in range(nf):
        frame = raw[2 * n * k:2 * n * (k + 1)]
        assert psds[0][k].tobytes() == f.receive_raw(frame).tobytes(), (n, nf, k)
        check_psd(psds[0][k], O.fft_receive(flt[2 * n * k:2 * n * (k + 1)], rate), n, rate)
    # the complex spectrum: equal to the contiguous call, and within FFT_RTOL of a float64 FFT
    buf, _ = LY.build_input([flt], lead=2, tail=2 * 33, unit=2, seed=100 + nf)
    d_in = upload(buf)
    out = Guarded(LY.Layout(nf, 2 * n, lead=2, tail=2 * 7, itemsize=4, unit=2), "fft spectrum")
    J.binding._check(J.lib().jsdr_fft_spectrum_f32(f.h, J.binding.C.c_void_p(d_in.ptr + 8), J.binding.C.c_int64(nf),
                                                  J.binding.C.c_void_p(out.ptr), None), "jsdr_fft_spectrum_f32")
    spec = out.rows(np.float32)
    assert spec.tobytes() == f.spectrum(flt.reshape(nf, 2 * n)).tobytes()
    for k in range(nf):
        x = flt[2 * n * k:2 * n * (k + 1)].astype(np.float64)
        ref = np.fft.fft(x[0::2] + 1j * x[1::2])
        g = spec[k, 0::2].astype(np.float64) + 1j * spec[k, 1::2]
        assert np.abs(g - ref).max() <= FFT_RTOL * np.abs(ref).max(), (n, k)


# ------------------------------------------------------------------ jsdr_fec_decode_batch / _encode_batch
@pytest.mark.parametrize("nb", [1, 3, 65])
def test_fec_batch_guarded_blocks_and_failed_blocks_keep_the_callers_bytes(nb):
    """k_fec_decode / k_fec_encode: one workgroup per block, grid-strided.  A block whose RS decode fails (rc = -1) must
    leave its 256 output bytes as the caller had them (FECDecoder.java:780, as the single call does); nothing may land
    before the first block or after the last, in `out`, `rc` or the encoder's symbols."""
    rng = np.random.default_rng(nb)
    datas = rng.integers(0, 256, (nb, 256), dtype=np.uint8)
    raws = []
    for k in range(nb):
        if k % 3 == 1 or nb == 1:
            raws.append(rng.integers(0, 256, 5200, dtype=np.uint8))  # junk: RS fails
        else:
            soft = np.where(O.fec_encode(datas[k]) == 1, 0xC0, 0x40).astype(np.uint8)
            e = (37 * k) % 400
            if e:
                soft[rng.choice(5200, e, replace=False)] ^= 0x80
            raws.append(soft)
    buf, _ = LY.build_input(raws, lead=4, tail=60, unit=4, seed=nb)
    d_raw = upload(buf)
    out = Guarded(LY.Layout(nb, 256, lead=4, tail=60), "fec out")
    rc = Guarded(LY.Layout(nb, 1, lead=1, tail=3, itemsize=4), "fec rc")
    J.fec_decode_dev(d_raw.ptr + 4, nb, out.ptr, rc.ptr)
    got_rc = rc.rows(np.int32)[:, 0]
    got = out.rows(np.uint8)
    kept = LY.guard_fill(out.lay.nbytes)
    failed = 0
    for k in range(nb):
        wrc, wout = O.fec_decode(raws[k])
        assert got_rc[k] == wrc, (nb, k)
        if wrc >= 0:
            assert np.array_equal(got[k], wout), (nb, k)
        else:
            failed += 1
            p = out.lay.starts[k]
            assert np.array_equal(got[k], kept[p:p + 256]), (nb, k, "a failed block changed the caller's bytes")
    assert failed >= 1
    # the encoder: data rows at a 4-byte offset, symbols guarded
    buf, _ = LY.build_input(list(datas), lead=4, tail=60, unit=4, seed=10 + nb)
    d_data = upload(buf)
    sym = Guarded(LY.Layout(nb, 5200, lead=4, tail=60), "fec symbols")
    J.fec_encode_dev(d_data.ptr + 4, nb, sym.ptr)
    got = sym.rows(np.uint8)
    for k in range(nb):
        assert np.array_equal(got[k], O.fec_encode(datas[k])), (nb, k)


# ------------------------------------------------------------------ jsdr_waterfall_lines
@pytest.mark.parametrize("n,width,nf", [(2048, 801, 5), (64, 101, 3), (2048, 1918, 1), (9600, 1918, 3)])
def test_waterfall_lines_guarded_pixel_rows(n, width, nf):
    """k_waterfall: odd frame counts, widths that are no multiple of 4 (the row's last partial store) and a width above n
    (several pixels per bin); psd rows at an 8-byte offset with NaN / 3e38 around them"""
    rng = np.random.default_rng(n + width)
    psd = (rng.standard_normal((nf, n + 2)) * 35 - 70).astype(np.float32)
    psd[0, rng.integers(0, n, 9)] = 25.0
    buf, _ = LY.build_input([psd.ravel()], lead=2, tail=2 * 21, unit=2, seed=nf)
    d_in = upload(buf)
    out = Guarded(LY.Layout(nf, width, lead=1, tail=3, itemsize=4), "waterfall pixels")
    J.waterfall_lines_dev(d_in.ptr + 8, nf, n, width, out.ptr, 0x00FFFF)
    got = out.rows(np.uint32)
    for k in range(nf):
        assert np.array_equal(got[k], O.waterfall_line(psd[k], n, width)), (n, width, k)


# ------------------------------------------------------------------ jsdr_convert_i16, jsdr_phase_maxabs
@pytest.mark.parametrize("nframes", [1, 7, 1001, 4097])
def test_convert_and_phase_maxabs_guarded(nframes):
    """k_convert_i16 is grid-strided with a bound on the frame count; k_phase_maxabs takes 16-byte loads with a scalar
    tail.  Odd counts, inputs at a one-element offset between poison, outputs guarded after the last value."""
    rng = np.random.default_rng(nframes)
    raw = rng.integers(-32768, 32768, 2 * nframes).astype(np.int16)
    for chns, lead in ((2, 2), (1, 1)):
        src = raw if chns == 2 else raw[:nframes].copy()
        buf, _ = LY.build_input([src], lead=lead, tail=2 * 9, unit=chns, seed=chns)
        d_in = upload(buf)
        out = Guarded(LY.Layout(1, 2 * nframes, lead=2, tail=2 * 3, itemsize=4, unit=2), f"convert out ({chns} channels)")
        J.binding._check(J.lib().jsdr_convert_i16(J.binding.C.c_void_p(d_in.ptr + 2 * lead), J.binding.C.c_int64(nframes), chns,
                                                 5, -7, J.binding.C.c_void_p(out.ptr), None), "jsdr_convert_i16")
        got = out.rows(np.float32)[0]
        assert got.tobytes() == O.convert_i16(src, chns=chns, ic=5, qc=-7).tobytes(), (nframes, chns)
    # max|x| per frame: frame length 2n floats with n even (the call's rule), nframes frames at an 8-byte offset
    n = 2 * (nframes % 50) + 2
    frames = (rng.standard_normal((nframes, 2 * n)) * 0.3).astype(np.float32)
    buf, _ = LY.build_input([frames.ravel()], lead=2, tail=2 * 9, unit=2, seed=3)
    d_in = upload(buf)
    out = Guarded(LY.Layout(nframes, 1, lead=1, tail=3, itemsize=4), "phase max")
    J.binding._check(J.lib().jsdr_phase_maxabs(J.binding.C.c_void_p(d_in.ptr + 8), J.binding.C.c_int64(nframes), n,
                                               J.binding.C.c_void_p(out.ptr), None), "jsdr_phase_maxabs")
    got = out.rows(np.float32)[:, 0]
    for k in range(nframes):
        assert got[k] == np.float32(O.phase_maxabs(frames[k])), (nframes, k)


# ------------------------------------------------------------------ jsdr_bpsk_batch_i16, jsdr_bpsk_pack_slots
def pack_slots_guarded(d, nstreams, what):
    """the handle's slots written 16 bytes into a guarded buffer; -> [nstreams][slot_bytes]"""
    info = d.slot_info()
    out = Guarded(LY.Layout(nstreams, info["slot_bytes"], lead=16, tail=64), what)
    d.sync()
    d.pack_slots(out.ptr)
    return info, out.rows(np.uint8)


def check_slots_against_getters(d, info, slots, streams):
    for s in streams:
        c = d.counters(s)
        bits = d.bits(s)
        assert len(bits) <= info["slot_bits"]
        want = SH.pack_slot(info, [c[k] for k in CN], bits, d.fec_results(s))
        assert np.array_equal(slots[s], want), s


def run_bpsk_padded(S, n, chunks, extra, rate=96000, blen=8192, tuning=12000, do_fft=0, seed=20020109):
    """S streams at stride 2n + extra, one pair into a poisoned buffer; the calls in `chunks`; everything against one
    reference demodulator per stream"""
    streams = [O.make_dbpsk_stream(seed, s, n, rate=rate, noise_sigma=900.0 + 60.0 * (s % 9))[0] for s in range(S)]
    stride = 2 * n + extra
    buf, starts = LY.build_input(streams, stride, lead=2, tail=2 * 33, unit=2, seed=S + extra)
    d_iq = upload(buf)
    d = J.Bpsk(rate=rate, blen=blen, tuning=tuning, do_fft=do_fft, nstreams=S, max_batch_samples=max(chunks))
    gbits, gtrace, gfec = ([[] for _ in range(S)] for _ in range(3))
    pos = 0
    for L in chunks:
        d.batch_i16(d_iq.ptr + 2 * 2 + 4 * pos, stride, L)
        for s in range(S):
            gbits[s].append(d.bits(s).copy())
            gtrace[s].append(d.trace(s).copy())
            gfec[s].extend(d.fec_results(s))
        pos += L
    assert pos == n
    for s in range(S):
        o = O.Bpsk(rate=rate, blen=(blen if do_fft else 4), tuning=tuning, do_fft=do_fft,
                   trace=n // max(1, rate // 9600) + 8)
        o.receive_i16(streams[s])
        assert np.array_equal(np.concatenate(gbits[s]), o.bits()), f"stream {s}: bits differ"
        assert np.array_equal(np.concatenate(gtrace[s]), o.trace()), f"stream {s}: (fi,fq) differ"
        fo = o.fec_results()
        assert len(gfec[s]) == len(fo), (s, len(gfec[s]), len(fo))
        for (rc, _, data), (orc, _, odata) in zip(gfec[s], fo):
            assert rc == orc and np.array_equal(data, odata), s
        same_counters(d.counters(s), o.counters())
        same_state(d.state(s), o.state())
        if do_fft:
            assert d.counters(s)["centreBin"] == o.counters()["centreBin"]
            assert d.state(s)[6] == o.state()[6] and d.state(s)[7] == o.state()[7]
        assert np.array_equal(d.decoded(s), o.decoded())
    return d


@pytest.mark.parametrize("S,n,extra,tuning", [
    (3, 458752, 2, 12000),     # an FEC frame decoded; periodic tuning (the cached tuner schedule)
    (3, 458752, 66, 12010),    # a tuning with no period inside the schedule
    (67, 40000, 66, 12000),    # a stream count that fills no whole wave of the per-stream kernels
    (67, 40000, 2, 12010),
])
def test_bpsk_tune_mode_padded_streams_and_guarded_slots(S, n, extra, tuning):
    """the tune-mode front end (k_fm / k_front_any) reads 4-byte-aligned 16-byte loads at s * stride: poisoned gaps of one
    and 33 pairs catch a read past the row, ragged calls move every row start by odd pair counts.  pack_slots writes the
    slots 16 bytes into a guarded buffer."""
    chunks = [77, 1, 2048 * 8 + 3, 26, 4099] if n < 100000 else [77, 2048 * 8 + 3, 26, 200000]
    chunks.append(n - sum(chunks))
    d = run_bpsk_padded(S, n, chunks, extra, tuning=tuning)
    info, slots = pack_slots_guarded(d, S, "bpsk slots")
    check_slots_against_getters(d, info, slots, range(S))
    if S == 3:
        assert all(d.counters(s)["cntFEC"] >= 1 for s in range(S))


@pytest.mark.parametrize("nsf,blen,rate", [(2048, 8192, 96000), (9600, 38400, 96000)])
def test_bpsk_fft_acquire_padded_streams(nsf, blen, rate):
    """FFT-acquire (k_acq_* at 2048, k_acqm_* at 9600) loads whole frames of each stream from s * stride"""
    n = nsf * 40
    chunks = [nsf * 3, nsf, n - nsf * 4]
    d = run_bpsk_padded(3, n, chunks, 66, rate=rate, blen=blen, do_fft=1, seed=31)
    info, slots = pack_slots_guarded(d, 3, "bpsk fft-acquire slots")
    check_slots_against_getters(d, info, slots, range(3))


def test_bpsk_channel_handle_padded_input_stride_and_slots():
    """k_chan_front reads each input once for all its channels at i * stride: two inputs one pair apart, a one-pair base
    offset, poison between.  Slots of the channel handle at a 16-byte offset: each equal to the getters and, for input
    0, to an ordinary handle's slot with that channel's tuning fed the same calls."""
    tunings = [12000, 24000, 12010]
    n = 60000
    chunks = [77, 4099, 26, n - 77 - 4099 - 26]
    inputs = [mixed_input(41 + i, n, [13200.0, 25200.0])[0] for i in range(2)]
    stride = 2 * n + 2
    buf, _ = LY.build_input(inputs, stride, lead=2, tail=2 * 33, unit=2, seed=5)
    d_iq = upload(buf)
    d = J.BpskChannels(96000, 8192, tunings, ninputs=2, max_batch_samples=max(chunks))
    S = d.nstreams
    bits, trace, fec = ([[] for _ in range(S)] for _ in range(3))
    pos = 0
    for L in chunks:
        d.batch_i16(d_iq.ptr + 4 + 4 * pos, stride, L)
        for s in range(S):
            bits[s].append(J.Bpsk.bits(d, s).copy())
            trace[s].append(J.Bpsk.trace(d, s).copy())
            fec[s].extend(J.Bpsk.fec_results(d, s))
        pos += L
    check_against_oracles(d, bits, trace, fec, inputs, tunings)
    info, slots = pack_slots_guarded(d, S, "channel slots")
    for s in range(S):
        c = J.Bpsk.counters(d, s)
        want = SH.pack_slot(info, [c[k] for k in CN], J.Bpsk.bits(d, s), J.Bpsk.fec_results(d, s))
        assert np.array_equal(slots[s], want), s
    for ch, t in enumerate(tunings):
        r = J.Bpsk(rate=96000, blen=8192, tuning=t, max_batch_samples=max(chunks))
        pos = 0
        for L in chunks:
            r.batch_i16(d_iq.ptr + 4 + 4 * pos, stride, L)
            pos += L
        rinfo, rslot = pack_slots_guarded(r, 1, "ordinary slot")
        assert rinfo == info
        assert np.array_equal(slots[ch], rslot[0]), ch


# ------------------------------------------------------------------ jsdr_group_batch_i16
def test_group_strided_psd_and_slots_of_two_members_on_one_device():
    """jsdr_group_batch_i16 with stride 2n + 2 takes the group's strided PSD path: one jsdr_fft_batch_i16 per stream,
    row s of psd_dev starting at s * nframes.  200 streams per member, psd rows at an 8-byte offset and guarded; sampled
    frames (first, last, and either side of the member boundary) against the float64 oracle; gathered slots against one
    ordinary handle fed the same calls."""
    S, n, calls = 400, 2048, [2048 * 2, 2048 * 3]
    per = S // 2
    g = J.Group(2, S, max(calls), devices=[0, 0], gather_copy=True, with_psd=True, frame=n)
    ref = J.Bpsk(nstreams=S, max_batch_samples=max(calls))
    info = ref.slot_info()
    rng = np.random.default_rng(400)
    for call, L in enumerate(calls):
        nf = L // n
        rows = [fft_frames(n, 96000, nf, 1000 * call + s) for s in range(S)]
        rows = [np.clip(r.astype(np.int32) + rng.integers(-500, 500, r.size), -32768, 32767).astype(np.int16) for r in rows]
        stride = 2 * L + 2
        bufs = [upload(LY.build_input(rows[m * per:(m + 1) * per], stride, lead=2, tail=2 * 33, unit=2, seed=m)[0])
                for m in range(2)]
        psds = [Guarded(LY.Layout(per * nf, n + 2, lead=2, tail=2 * 5, itemsize=4), f"group psd member {m}") for m in range(2)]
        g.batch_i16([b.ptr + 4 for b in bufs], stride, L, psd_devs=[p.ptr for p in psds])
        g.sync()
        got = [p.rows(np.float32).reshape(per, nf, n + 2) for p in psds]
        f = J.Fft(n, 96000)
        for s in (0, 1, per - 2, per - 1, per, per + 1, S - 2, S - 1):
            m, sl = divmod(s, per)
            for k in (0, nf - 1):
                frame = rows[s][2 * n * k:2 * n * (k + 1)]
                assert got[m][sl, k].tobytes() == f.receive_raw(frame).tobytes(), (call, s, k)
                check_psd(got[m][sl, k], O.fft_receive(O.convert_i16(frame), 96000), n, 96000)
        one = upload(LY.build_input(rows, stride, lead=2, tail=2 * 33, unit=2, seed=7)[0])
        ref.batch_i16(one.ptr + 4, stride, L)
        _, want = pack_slots_guarded(ref, S, "reference slots")
        for m in range(2):
            assert np.array_equal(g.gathered(m), want), (call, m)


# ------------------------------------------------------------------ jsdr_synth_dbpsk, jsdr_recordings_load
def test_synth_dbpsk_leaves_the_gaps_between_rows_alone():
    """k_synth_dbpsk writes row s at s * stride: a stride 17 pairs longer than the row and a one-pair offset, guarded"""
    nstreams, n, n0 = 3, 1001, 777
    pay = np.stack([O.synth_payload(5, s, 0) for s in range(nstreams)])
    sym = np.stack([O.fec_encode(pay[s]) for s in range(nstreams)])
    ds = np.stack([O.synth_diffsign(sym[s]) for s in range(nstreams)]).astype(np.int8)
    ct, st = O.synth_tables(3000)
    keys = np.array([O.mix64(70 + s) for s in range(nstreams)], np.uint64)
    inc = O.phase_inc_u32(13200.0, 96000)
    stride = 2 * n + 34
    out = Guarded(LY.Layout(nstreams, 2 * n, stride, lead=2, tail=2 * 9, itemsize=2, unit=2), "synth rows")
    dev = [upload(a) for a in (ds, ct, st, keys)]  # held until the asynchronous call has run
    J.synth_dbpsk(out.ptr, stride, nstreams, n0, n, dev[0], 5200, 80, 77, inc, dev[1], dev[2], 1299, dev[3])
    got = out.rows(np.int16)
    for s in range(nstreams):
        assert np.array_equal(got[s], O.synth_dbpsk(n0, n, ds[s], 80, 77, inc, ct, st, 1299, int(keys[s]))), s


def test_recordings_load_zero_fills_exactly_its_own_row(tmp_path):
    """jsdr_recordings_load copies each file to row s at s * stride and zero-fills a short file's row to nframes: the fill
    must end at the row's end, the gaps and the bytes around the rows keep what the caller had"""
    rng = np.random.default_rng(12)
    lens = [900, 250, 1200]
    data = [rng.integers(-32768, 32768, 2 * m).astype(np.int16) for m in lens]
    paths = []
    for k, x in enumerate(data):
        p = os.path.join(tmp_path, f"rec{k}.raw")
        x.astype("<i2").tofile(p)
        paths.append(p)
    first, nframes = 100, 700
    stride = 2 * nframes + 10
    out = Guarded(LY.Layout(3, 2 * nframes, stride, lead=2, tail=2 * 9, itemsize=2, unit=2), "recording rows")
    got_n = J.recordings_load(paths, 2, 96000, first, nframes, out.ptr, stride)
    assert got_n == [nframes, lens[1] - first, nframes]
    got = out.rows(np.int16)
    for s, x in enumerate(data):
        k = got_n[s]
        assert np.array_equal(got[s, :2 * k], x[2 * first:2 * (first + k)]), s
        assert np.all(got[s, 2 * k:] == 0), s
