"""ctypes binding of libjsdr_hip.so (the C ABI declared in include/jsdr_hip.h).

Plain pointers and sizes only; numpy arrays are used for host buffers, DeviceBuffer (or any integer
device address, e.g. torch.Tensor.data_ptr()) for HBM buffers.
"""
import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# JSDR_LIB: developer knob for same-box A/B timing of two builds (tools/build_variant.sh)
_SO = os.environ.get("JSDR_LIB") or os.path.join(HERE, "libjsdr_hip.so")


class JsdrError(RuntimeError):
    pass


def library_path():
    return _SO


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "jsdr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(jsdr_[a-z0-9_]+)\s*\(", hdr)))


EXPORTED_SYMBOLS = _declared_symbols()

_lib = None


def lib():
    """Load the library (building nothing: run java-sdr_amd/build.py or __graft_entry__.build() first)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise JsdrError(f"{_SO} is missing: build it with `python java-sdr_amd/build.py` "
                            "(there is no CPU fallback)")
        _lib = C.CDLL(_SO)
        _lib.jsdr_last_error.restype = C.c_char_p
        _lib.jsdr_bpsk_profile_name.restype = C.c_char_p
        _lib.jsdr_demod_profile_name.restype = C.c_char_p
        for fn in ("jsdr_bpsk_front_kernel", "jsdr_bpsk_tail_kernel", "jsdr_bpsk_fec_kernel", "jsdr_fft_kernel",
                   "jsdr_fft_waterfall_kernel", "jsdr_phase_scope_kernel", "jsdr_demod_scope_kernel", "jsdr_bpsk_scope_kernel"):
            getattr(_lib, fn).restype = C.c_char_p
            getattr(_lib, fn).argtypes = [C.c_void_p]
        for name in EXPORTED_SYMBOLS:
            if name not in ("jsdr_last_error", "jsdr_bpsk_profile_name", "jsdr_demod_profile_name", "jsdr_bpsk_front_kernel",
                            "jsdr_bpsk_tail_kernel", "jsdr_bpsk_fec_kernel", "jsdr_fft_kernel", "jsdr_fft_waterfall_kernel",
                            "jsdr_phase_scope_kernel", "jsdr_demod_scope_kernel", "jsdr_bpsk_scope_kernel"):
                getattr(_lib, name).restype = C.c_int
    return _lib


def _check(rc, what=""):
    if rc != 0:
        msg = lib().jsdr_last_error()
        raise JsdrError(f"{what}: {msg.decode() if msg else 'error'}")


def have_gpu():
    try:
        n = C.c_int(0)
        return lib().jsdr_device_count(C.byref(n)) == 0 and n.value > 0
    except Exception:
        return False


def _addr(x):
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return C.c_void_p(x.ptr)
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    raise TypeError(type(x))


class DeviceBuffer:
    """HBM allocation owned through jsdr_malloc/jsdr_free."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(lib().jsdr_malloc(C.byref(p), C.c_size_t(self.nbytes)), "jsdr_malloc")
        self.ptr = p.value

    @classmethod
    def from_host(cls, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes)
        _check(lib().jsdr_memcpy_h2d(C.c_void_p(b.ptr), _addr(arr), C.c_size_t(arr.nbytes)), "h2d")
        return b

    def to_host(self, dtype, count=None, offset_bytes=0):
        dtype = np.dtype(dtype)
        if count is None:
            count = (self.nbytes - offset_bytes) // dtype.itemsize
        out = np.empty(count, dtype)
        _check(lib().jsdr_memcpy_d2h(_addr(out), C.c_void_p(self.ptr + offset_bytes), C.c_size_t(out.nbytes)), "d2h")
        return out

    def zero(self):
        _check(lib().jsdr_memset(C.c_void_p(self.ptr), 0, C.c_size_t(self.nbytes)), "memset")

    def free(self):
        if self.ptr:
            lib().jsdr_free(C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def live_resources():
    """(device buffers, device bytes, pinned buffers, streams + events) the library's handles and calls hold at the moment"""
    v = [C.c_int64(0) for _ in range(4)]
    _check(lib().jsdr_live_resources(*[C.byref(x) for x in v]), "jsdr_live_resources")
    return tuple(x.value for x in v)


class Stream:
    """a non-blocking HIP stream (pass `.ptr` as the `stream` argument of the batch calls)"""

    def __init__(self):
        self.h = C.c_void_p()
        _check(lib().jsdr_stream_create(C.byref(self.h)), "jsdr_stream_create")
        self.ptr = self.h.value

    def sync(self):
        stream_sync(self.ptr)

    def __del__(self):
        try:
            if self.h:
                lib().jsdr_stream_destroy(self.h)
        except Exception:
            pass


def stream_sync(stream=None):
    _check(lib().jsdr_stream_sync(C.c_void_p(stream)), "jsdr_stream_sync")


class Timer:
    """HIP-event pair on the stream the kernels are launched on."""

    def __init__(self):
        self.h = C.c_void_p()
        _check(lib().jsdr_timer_create(C.byref(self.h)), "timer_create")

    def start(self, stream=None):
        _check(lib().jsdr_timer_start(self.h, C.c_void_p(stream)), "timer_start")

    def stop(self, stream=None):
        _check(lib().jsdr_timer_stop(self.h, C.c_void_p(stream)), "timer_stop")

    def elapsed_ms(self):
        ms = C.c_float()
        _check(lib().jsdr_timer_elapsed_ms(self.h, C.byref(ms)), "timer_elapsed")
        return ms.value

    def __del__(self):
        try:
            lib().jsdr_timer_destroy(self.h)
        except Exception:
            pass


# ------------------------------------------------------------------ JavaAudio conversion rule
def convert_i16(raw, chns=2, ic=0, qc=0):
    raw = np.ascontiguousarray(raw, np.int16)
    nframes = raw.size // chns
    d_in = DeviceBuffer.from_host(raw)
    d_out = DeviceBuffer(8 * nframes)
    _check(lib().jsdr_convert_i16(_addr(d_in), C.c_int64(nframes), chns, ic, qc, _addr(d_out), None), "convert_i16")
    return d_out.to_host(np.float32)


# ------------------------------------------------------------------ fft.java
class Fft:
    """fft.receive: n = blen/size samples per frame -> psd float[n+2] (fft.java:190-228)."""

    def __init__(self, n, rate):
        self.n, self.rate = n, rate
        self.h = C.c_void_p()
        _check(lib().jsdr_fft_create(C.byref(self.h), n, rate), "jsdr_fft_create")

    def receive(self, buf):
        buf = np.ascontiguousarray(buf, np.float32)
        assert buf.size == 2 * self.n
        psd = np.empty(self.n + 2, np.float32)
        _check(lib().jsdr_fft_receive_f32(self.h, _addr(buf), _addr(psd)), "jsdr_fft_receive_f32")
        return psd

    def receive_raw(self, raw, ic=0, qc=0):
        raw = np.ascontiguousarray(raw, np.int16)
        assert raw.size == 2 * self.n
        psd = np.empty(self.n + 2, np.float32)
        _check(lib().jsdr_fft_receive_i16(self.h, _addr(raw), ic, qc, _addr(psd)), "jsdr_fft_receive_i16")
        return psd

    def set_cu_share(self, wgs_per_cu):
        _check(lib().jsdr_fft_set_cu_share(self.h, int(wgs_per_cu)), "jsdr_fft_set_cu_share")

    def kernel_name(self):
        return lib().jsdr_fft_kernel(self.h).decode()

    def last_launch(self):
        a, b = C.c_int64(), C.c_int64()
        _check(lib().jsdr_fft_last_launch(self.h, C.byref(a), C.byref(b)), "jsdr_fft_last_launch")
        return a.value, b.value

    def batch_i16(self, raw_dev, nframes, psd_dev, ic=0, qc=0, stream=None):
        _check(lib().jsdr_fft_batch_i16(self.h, _addr(raw_dev), C.c_int64(nframes), ic, qc, _addr(psd_dev),
                                        C.c_void_p(stream)), "jsdr_fft_batch_i16")

    def batch_f32(self, iq_dev, nframes, psd_dev, stream=None):
        _check(lib().jsdr_fft_batch_f32(self.h, _addr(iq_dev), C.c_int64(nframes), _addr(psd_dev),
                                        C.c_void_p(stream)), "jsdr_fft_batch_f32")

    def waterfall_i16(self, raw_dev, nframes, width, pix_dev, ic=0, qc=0, peak_rgb=0x00FFFF, max_dev=None, peak_dev=None,
                      stream=None):
        """fft.receive + waterfall.paintLine of nframes int16 frames: pix_dev uint32 [nframes][width]; optionally max_dev float
        [nframes][width] (the pooled maxima, unrotated) and peak_dev float [nframes][2] = (Hz, max dB).  No PSD array is written."""
        _check(lib().jsdr_fft_waterfall_i16(self.h, _addr(raw_dev), C.c_int64(nframes), int(ic), int(qc), int(width),
                                            C.c_uint32(peak_rgb), _addr(pix_dev), _addr(max_dev), _addr(peak_dev),
                                            C.c_void_p(stream)), "jsdr_fft_waterfall_i16")

    def waterfall_f32(self, iq_dev, nframes, width, pix_dev, peak_rgb=0x00FFFF, max_dev=None, peak_dev=None, stream=None):
        _check(lib().jsdr_fft_waterfall_f32(self.h, _addr(iq_dev), C.c_int64(nframes), int(width), C.c_uint32(peak_rgb),
                                            _addr(pix_dev), _addr(max_dev), _addr(peak_dev), C.c_void_p(stream)),
               "jsdr_fft_waterfall_f32")

    def batch_streams_i16(self, raw_dev, nstreams, stream_stride_i16, frames_per_stream, psd_dev, psd_stream_stride_f32=0, ic=0,
                          qc=0, stream=None):
        """batch_i16 over raw[stream][stride]: frame j of stream s at int16 s * stream_stride_i16 + j * 2n, its PSD row at float
        s * psd_stream_stride_f32 + j * (n + 2) (0: packed).  One launch; each stream's rows are batch_i16's, bit for bit."""
        _check(lib().jsdr_fft_batch_streams_i16(self.h, _addr(raw_dev), int(nstreams), C.c_int64(stream_stride_i16),
                                                C.c_int64(frames_per_stream), int(ic), int(qc), _addr(psd_dev),
                                                C.c_int64(psd_stream_stride_f32), C.c_void_p(stream)), "jsdr_fft_batch_streams_i16")

    def batch_streams_f32(self, iq_dev, nstreams, stream_stride_f32, frames_per_stream, psd_dev, psd_stream_stride_f32=0, stream=None):
        _check(lib().jsdr_fft_batch_streams_f32(self.h, _addr(iq_dev), int(nstreams), C.c_int64(stream_stride_f32),
                                                C.c_int64(frames_per_stream), _addr(psd_dev), C.c_int64(psd_stream_stride_f32),
                                                C.c_void_p(stream)), "jsdr_fft_batch_streams_f32")

    def waterfall_streams_i16(self, raw_dev, nstreams, stream_stride_i16, frames_per_stream, width, pix_dev, ic=0, qc=0,
                              peak_rgb=0x00FFFF, max_dev=None, peak_dev=None, stream=None):
        """waterfall_i16 over raw[stream][stride]; the outputs are packed, row s * frames_per_stream + j."""
        _check(lib().jsdr_fft_waterfall_streams_i16(self.h, _addr(raw_dev), int(nstreams), C.c_int64(stream_stride_i16),
                                                    C.c_int64(frames_per_stream), int(ic), int(qc), int(width), C.c_uint32(peak_rgb),
                                                    _addr(pix_dev), _addr(max_dev), _addr(peak_dev), C.c_void_p(stream)),
               "jsdr_fft_waterfall_streams_i16")

    def waterfall_streams_f32(self, iq_dev, nstreams, stream_stride_f32, frames_per_stream, width, pix_dev, peak_rgb=0x00FFFF,
                              max_dev=None, peak_dev=None, stream=None):
        _check(lib().jsdr_fft_waterfall_streams_f32(self.h, _addr(iq_dev), int(nstreams), C.c_int64(stream_stride_f32),
                                                    C.c_int64(frames_per_stream), int(width), C.c_uint32(peak_rgb), _addr(pix_dev),
                                                    _addr(max_dev), _addr(peak_dev), C.c_void_p(stream)),
               "jsdr_fft_waterfall_streams_f32")

    def waterfall_kernel(self):
        """what the last waterfall_* call launched: "k_fft_pix", or "<batch kernel>+k_waterfall" """
        return lib().jsdr_fft_waterfall_kernel(self.h).decode()

    def spectrum(self, bufs):
        """complex spectra of a [nframes, 2n] float32 array (for the 1e-5 parity tests)"""
        bufs = np.ascontiguousarray(bufs, np.float32).reshape(-1, 2 * self.n)
        d_in = DeviceBuffer.from_host(bufs)
        d_out = DeviceBuffer(bufs.nbytes)
        _check(lib().jsdr_fft_spectrum_f32(self.h, _addr(d_in), C.c_int64(bufs.shape[0]), _addr(d_out), None),
               "jsdr_fft_spectrum_f32")
        return d_out.to_host(np.float32).reshape(bufs.shape)

    def batch_host_i16(self, raw, ic=0, qc=0):
        raw = np.ascontiguousarray(raw, np.int16).reshape(-1, 2 * self.n)
        d_in = DeviceBuffer.from_host(raw)
        d_out = DeviceBuffer(4 * raw.shape[0] * (self.n + 2))
        self.batch_i16(d_in, raw.shape[0], d_out, ic, qc)
        return d_out.to_host(np.float32).reshape(raw.shape[0], self.n + 2)

    def __del__(self):
        try:
            lib().jsdr_fft_destroy(self.h)
        except Exception:
            pass


# ------------------------------------------------------------------ phase.java
def phase_maxabs(bufs, n):
    bufs = np.ascontiguousarray(bufs, np.float32).reshape(-1, 2 * n)
    d_in = DeviceBuffer.from_host(bufs)
    d_out = DeviceBuffer(4 * bufs.shape[0])
    _check(lib().jsdr_phase_maxabs(_addr(d_in), C.c_int64(bufs.shape[0]), n, _addr(d_out), None), "jsdr_phase_maxabs")
    return d_out.to_host(np.float32)


def phase_columns(buf, bx):
    buf = np.ascontiguousarray(buf, np.float32)
    n = buf.size // 2
    d_in = DeviceBuffer.from_host(buf)
    cap = n + 1
    pix = np.empty(cap, np.int32)
    ai = np.empty(cap, np.float32)
    aq = np.empty(cap, np.float32)
    ncol = C.c_int()
    _check(lib().jsdr_phase_columns(_addr(d_in), n, bx, _addr(pix), _addr(ai), _addr(aq), cap, C.byref(ncol)),
           "jsdr_phase_columns")
    k = ncol.value
    return pix[:k].copy(), ai[:k].copy(), aq[:k].copy()


def phase_layout(n, bx):
    """the painter's column schedule of (n, bx), host only: (pix, first sample, sample count) of every closed column"""
    ncol = C.c_int()
    _check(lib().jsdr_phase_layout(int(n), int(bx), None, None, None, 0, C.byref(ncol)), "jsdr_phase_layout")
    k = ncol.value
    pix, first, count = (np.empty(k, np.int32) for _ in range(3))
    if k:
        _check(lib().jsdr_phase_layout(int(n), int(bx), _addr(pix), _addr(first), _addr(count), k, C.byref(ncol)), "jsdr_phase_layout")
    return pix, first, count


class Phase:
    """phase.java as a handle (the IAudioHandler drop-in): receive() keeps the frame on the device and takes max|x|
    (phase.java:75-80,123-128); columns(bx) are the painter's per-pixel-column means (:93-116)"""

    def __init__(self, n):
        self.n = n
        self.h = C.c_void_p()
        _check(lib().jsdr_phase_create(C.byref(self.h), n), "jsdr_phase_create")

    def receive(self, buf):
        buf = np.ascontiguousarray(buf, np.float32)
        assert buf.size == 2 * self.n
        _check(lib().jsdr_phase_receive_f32(self.h, _addr(buf)), "jsdr_phase_receive_f32")

    def max(self):
        m = C.c_float()
        _check(lib().jsdr_phase_get_max(self.h, C.byref(m)), "jsdr_phase_get_max")
        return np.float32(m.value)

    def columns(self, bx):
        cap = self.n + 1
        pix = np.empty(cap, np.int32)
        ai = np.empty(cap, np.float32)
        aq = np.empty(cap, np.float32)
        ncol = C.c_int()
        _check(lib().jsdr_phase_get_columns(self.h, bx, _addr(pix), _addr(ai), _addr(aq), cap, C.byref(ncol)),
               "jsdr_phase_get_columns")
        k = ncol.value
        return pix[:k].copy(), ai[:k].copy(), aq[:k].copy()

    def scope_i16(self, raw_dev, nstreams, stream_stride_i16, frames_per_stream, ic, qc, bx, half_size, quarter_height, max_dev,
                  avg_dev=None, pts_dev=None, stream=None):
        """phase.paintComponent's arithmetic for every frame of raw[stream][stride] in one launch: max_dev float [rows], avg_dev
        float [rows][ncol][2] = (avgi, avgq), pts_dev int32 [rows][ncol][4] = (line_i, line_q, dot_i, dot_q), rows = nstreams *
        frames_per_stream packed, ncol = len(phase_layout(n, bx)[0]).  bx == 0 writes max_dev alone."""
        _check(lib().jsdr_phase_scope_i16(self.h, _addr(raw_dev), int(nstreams), C.c_int64(stream_stride_i16),
                                          C.c_int64(frames_per_stream), int(ic), int(qc), int(bx), int(half_size), int(quarter_height),
                                          _addr(max_dev), _addr(avg_dev), _addr(pts_dev), C.c_void_p(stream)), "jsdr_phase_scope_i16")

    def scope_f32(self, iq_dev, nstreams, stream_stride_f32, frames_per_stream, bx, half_size, quarter_height, max_dev, avg_dev=None,
                  pts_dev=None, stream=None):
        _check(lib().jsdr_phase_scope_f32(self.h, _addr(iq_dev), int(nstreams), C.c_int64(stream_stride_f32),
                                          C.c_int64(frames_per_stream), int(bx), int(half_size), int(quarter_height), _addr(max_dev),
                                          _addr(avg_dev), _addr(pts_dev), C.c_void_p(stream)), "jsdr_phase_scope_f32")

    def scope_kernel(self):
        """what the last scope_* call launched: "k_phase_scope" (the frame's image in LDS) or "k_phase_scope_g" """
        return lib().jsdr_phase_scope_kernel(self.h).decode()

    def __del__(self):
        try:
            lib().jsdr_phase_destroy(self.h)
        except Exception:
            pass


# ------------------------------------------------------------------ fir.java
class Fir:
    def __init__(self, rate=44100.0):
        self.h = C.c_void_p()
        _check(lib().jsdr_fir_create(C.byref(self.h), C.c_float(rate)), "jsdr_fir_create")

    def weights(self, f1, f2):
        w = np.empty(21, np.float64)
        _check(lib().jsdr_fir_weights(self.h, f1, f2, _addr(w)), "jsdr_fir_weights")
        return w

    def filter_block(self, xs):
        xs = np.ascontiguousarray(xs, np.int32)
        out = np.empty_like(xs)
        _check(lib().jsdr_fir_filter(self.h, _addr(xs), _addr(out), C.c_int64(xs.size)), "jsdr_fir_filter")
        return out

    def complex_gen(self, freq, count, start=0):
        out = np.empty((count, 2), np.int32)
        _check(lib().jsdr_fir_complex_gen(self.h, freq, start, _addr(out), C.c_int64(count)), "jsdr_fir_complex_gen")
        return out

    def complex_mod(self, a, b):
        a = np.ascontiguousarray(a, np.int32)
        b = np.ascontiguousarray(b, np.int32)
        out = np.empty_like(a)
        _check(lib().jsdr_fir_complex_mod(self.h, _addr(a), _addr(b), _addr(out), C.c_int64(a.shape[0])),
               "jsdr_fir_complex_mod")
        return out

    def __del__(self):
        try:
            lib().jsdr_fir_destroy(self.h)
        except Exception:
            pass


def fir_batch_decimate_i16(raw_dev, nstreams, stride_i16, nsamples, taps, decim, scale, out_dev, out_stride_pairs, stream=None):
    """batched FIR + decimate (BASELINE config 3); returns the number of outputs per stream"""
    taps = np.ascontiguousarray(taps, np.float64)
    nout = C.c_int64()
    _check(lib().jsdr_fir_batch_decimate_i16(_addr(raw_dev), nstreams, C.c_int64(stride_i16), C.c_int64(nsamples), _addr(taps),
                                             int(taps.size), int(decim), C.c_double(scale), _addr(out_dev),
                                             C.c_int64(out_stride_pairs), C.byref(nout), C.c_void_p(stream)),
           "jsdr_fir_batch_decimate_i16")
    return nout.value


# ------------------------------------------------------------------ FECDecoder.java
def fec_decode(raw, out_init=None):
    raw = np.ascontiguousarray(raw, np.uint8)
    assert raw.size == 5200
    out = np.zeros(256, np.uint8) if out_init is None else np.array(out_init, np.uint8)
    rc = C.c_int()
    _check(lib().jsdr_fec_decode(_addr(raw), _addr(out), C.byref(rc)), "jsdr_fec_decode")
    return rc.value, out


def fec_encode(data):
    data = np.ascontiguousarray(data, np.uint8)
    assert data.size == 256
    sym = np.empty(5200, np.uint8)
    _check(lib().jsdr_fec_encode(_addr(data), _addr(sym)), "jsdr_fec_encode")
    return sym


def fec_decode_batch(raws):
    raws = np.ascontiguousarray(raws, np.uint8).reshape(-1, 5200)
    nb = raws.shape[0]
    d_raw = DeviceBuffer.from_host(raws)
    d_out = DeviceBuffer(256 * nb)
    d_out.zero()
    d_rc = DeviceBuffer(4 * nb)
    _check(lib().jsdr_fec_decode_batch(_addr(d_raw), C.c_int64(nb), _addr(d_out), _addr(d_rc), None),
           "jsdr_fec_decode_batch")
    return d_rc.to_host(np.int32), d_out.to_host(np.uint8).reshape(nb, 256)


def fec_encode_batch(datas):
    datas = np.ascontiguousarray(datas, np.uint8).reshape(-1, 256)
    nb = datas.shape[0]
    d_in = DeviceBuffer.from_host(datas)
    d_out = DeviceBuffer(5200 * nb)
    _check(lib().jsdr_fec_encode_batch(_addr(d_in), C.c_int64(nb), _addr(d_out), None), "jsdr_fec_encode_batch")
    return d_out.to_host(np.uint8).reshape(nb, 5200)


def fec_encode_dev(data_dev, nblocks, sym_dev, stream=None):
    """device-resident form: data_dev[nblocks][256] -> sym_dev[nblocks][5200]"""
    _check(lib().jsdr_fec_encode_batch(_addr(data_dev), C.c_int64(nblocks), _addr(sym_dev), C.c_void_p(stream)),
           "jsdr_fec_encode_batch")


def fec_decode_dev(raw_dev, nblocks, out_dev, rc_dev, stream=None):
    _check(lib().jsdr_fec_decode_batch(_addr(raw_dev), C.c_int64(nblocks), _addr(out_dev), _addr(rc_dev),
                                       C.c_void_p(stream)), "jsdr_fec_decode_batch")


# ------------------------------------------------------------------ FUNcubeBPSKDemod.java
COUNTER_NAMES = ["cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK",
                 "centreBin"]


class BpskSnapshot(C.Structure):
    _fields_ = [("frames", C.c_int64), ("counters", C.c_int32 * 10), ("nbits", C.c_int32), ("state", C.c_double * 18),
                ("decoded", C.c_uint8 * 256), ("bits", C.c_int8 * 512)]


def bpsk_table(which):
    out = np.empty(256, np.float64)
    _check(lib().jsdr_bpsk_table(which, _addr(out), 256), "jsdr_bpsk_table")
    return out[:{0: 27, 1: 65, 2: 65}.get(which, 256)].copy()


class Bpsk:
    """`nstreams` lock-step FUNcubeBPSKDemod instances (FUNcubeBPSKDemod.java:357-595)."""

    def __init__(self, rate=96000, blen=8192, size=4, tuning=12000, do_fft=0, do_up=0, nstreams=1,
                 max_batch_samples=None, variant="exact"):
        self.samples = blen // size
        self.nstreams = nstreams
        self.max_batch = max_batch_samples or self.samples
        self.h = C.c_void_p()
        _check(lib().jsdr_bpsk_create(C.byref(self.h), rate, self.samples, tuning, do_fft, do_up, nstreams,
                                      C.c_int64(self.max_batch)), "jsdr_bpsk_create")
        if variant != "exact":
            _check(lib().jsdr_bpsk_set_variant(self.h, {"exact": 0, "fast": 1}[variant]), "jsdr_bpsk_set_variant")

    def snapshot(self):
        """results of the last completed receive(); callable from any thread while another one is inside receive()"""
        sn = BpskSnapshot()
        _check(lib().jsdr_bpsk_snapshot_read(self.h, C.byref(sn)), "jsdr_bpsk_snapshot_read")
        return sn

    def cert_stats(self):
        r, u, e = C.c_int64(), C.c_int64(), C.c_double()
        _check(lib().jsdr_bpsk_cert_stats(self.h, C.byref(r), C.byref(u), C.byref(e)), "jsdr_bpsk_cert_stats")
        return dict(decisions_redone_exactly=r.value, streams_uncertified=u.value, fi_fq_error_bound=e.value)

    def uncertified_streams(self):
        """fast variant: ids of the streams whose results are withheld (jsdr_hip.h); [] for the exact variant"""
        n = C.c_int()
        _check(lib().jsdr_bpsk_uncertified_streams(self.h, None, 0, C.byref(n)), "jsdr_bpsk_uncertified_streams")
        ids = np.empty(max(n.value, 1), np.int32)
        _check(lib().jsdr_bpsk_uncertified_streams(self.h, _addr(ids), n.value, C.byref(n)), "jsdr_bpsk_uncertified_streams")
        return [int(v) for v in ids[:n.value]]

    def schedule_stats(self):
        a, b = C.c_int64(), C.c_int64()
        _check(lib().jsdr_bpsk_schedule_stats(self.h, C.byref(a), C.byref(b)), "jsdr_bpsk_schedule_stats")
        return dict(computed_inline=a.value, prefetched=b.value)

    def front_kernel_name(self):
        return lib().jsdr_bpsk_front_kernel(self.h).decode()

    def tail_kernel_name(self):
        return lib().jsdr_bpsk_tail_kernel(self.h).decode()

    def fec_kernel_name(self):
        return lib().jsdr_bpsk_fec_kernel(self.h).decode()

    def side_stream(self):
        on = C.c_int()
        _check(lib().jsdr_bpsk_side_stream(self.h, C.byref(on)), "jsdr_bpsk_side_stream")
        return bool(on.value)

    def receive(self, buf):
        buf = np.ascontiguousarray(buf, np.float32)
        assert buf.size == 2 * self.samples
        _check(lib().jsdr_bpsk_receive_f32(self.h, _addr(buf)), "jsdr_bpsk_receive_f32")

    def receive_raw(self, raw, ic=0, qc=0):
        raw = np.ascontiguousarray(raw, np.int16)
        assert raw.size == 2 * self.samples
        _check(lib().jsdr_bpsk_receive_i16(self.h, _addr(raw), ic, qc), "jsdr_bpsk_receive_i16")

    def batch_i16(self, raw_dev, stride_i16, nsamples, ic=0, qc=0, stream=None):
        _check(lib().jsdr_bpsk_batch_i16(self.h, _addr(raw_dev), C.c_int64(stride_i16), C.c_int64(nsamples), ic, qc,
                                         C.c_void_p(stream)), "jsdr_bpsk_batch_i16")

    def batch_f32(self, iq_dev, stride_f32, nsamples, stream=None):
        """float IQ [S][stride_f32], taken as receive(float[]) takes buf[] (any float: no DC correction, no scaling); otherwise
        as batch_i16"""
        _check(lib().jsdr_bpsk_batch_f32(self.h, _addr(iq_dev), C.c_int64(stride_f32), C.c_int64(nsamples),
                                         C.c_void_p(stream)), "jsdr_bpsk_batch_f32")

    # the scope (jsdr_hip.h "The BPSK scope over batches"): the batch call plus the painter's rings and first panel, a row per frame
    def scope_i16(self, raw_dev, stride_i16, nsamples, ic=0, qc=0, tuned=None, ds=None, iq=None, max=None, pts=None, bits=None,
                  stream=None):
        """batch_i16, then per frame (row = s * frames + f) the outputs given: tuned f64 [rows][n][2], ds / iq f64 [rows][L][2],
        max f64 [rows][2], pts i32 [rows][L][4], bits i8 [rows][L]; None passes NULL"""
        _check(lib().jsdr_bpsk_scope_i16(self.h, _addr(raw_dev), C.c_int64(stride_i16), C.c_int64(nsamples), ic, qc, _addr(tuned),
                                         _addr(ds), _addr(iq), _addr(max), _addr(pts), _addr(bits), C.c_void_p(stream)),
               "jsdr_bpsk_scope_i16")

    def scope_f32(self, iq_in_dev, stride_f32, nsamples, tuned=None, ds=None, iq=None, max=None, pts=None, bits=None, stream=None):
        """batch_f32, then the outputs as scope_i16"""
        _check(lib().jsdr_bpsk_scope_f32(self.h, _addr(iq_in_dev), C.c_int64(stride_f32), C.c_int64(nsamples), _addr(tuned), _addr(ds),
                                         _addr(iq), _addr(max), _addr(pts), _addr(bits), C.c_void_p(stream)), "jsdr_bpsk_scope_f32")

    # the scope's spectra (jsdr_hip.h "The BPSK scope's spectra"): the scope call plus the painter's green and cyan spectra per frame
    def scope_spectra_i16(self, raw_dev, stride_i16, nsamples, ic=0, qc=0, tuned=None, ds=None, iq=None, max=None, pts=None, bits=None,
                          plot_width=0, tspec=None, tpeak=None, tpsd=None, dspec=None, dpeak=None, dpsd=None, stream=None):
        """scope_i16, then per frame of the `tuned` row (t...) and of the `ds` row (d...): spec i32 [rows][plot_width], peak f64
        [rows][2] = (max, mo), psd f64 [rows][n] / [rows][L]; None passes NULL"""
        _check(lib().jsdr_bpsk_scope_spectra_i16(self.h, _addr(raw_dev), C.c_int64(stride_i16), C.c_int64(nsamples), ic, qc, _addr(tuned),
                                                 _addr(ds), _addr(iq), _addr(max), _addr(pts), _addr(bits), int(plot_width), _addr(tspec),
                                                 _addr(tpeak), _addr(tpsd), _addr(dspec), _addr(dpeak), _addr(dpsd), C.c_void_p(stream)),
               "jsdr_bpsk_scope_spectra_i16")

    def scope_spectra_f32(self, iq_in_dev, stride_f32, nsamples, tuned=None, ds=None, iq=None, max=None, pts=None, bits=None,
                          plot_width=0, tspec=None, tpeak=None, tpsd=None, dspec=None, dpeak=None, dpsd=None, stream=None):
        """scope_f32, then the spectra as scope_spectra_i16"""
        _check(lib().jsdr_bpsk_scope_spectra_f32(self.h, _addr(iq_in_dev), C.c_int64(stride_f32), C.c_int64(nsamples), _addr(tuned),
                                                 _addr(ds), _addr(iq), _addr(max), _addr(pts), _addr(bits), int(plot_width), _addr(tspec),
                                                 _addr(tpeak), _addr(tpsd), _addr(dspec), _addr(dpeak), _addr(dpsd), C.c_void_p(stream)),
               "jsdr_bpsk_scope_spectra_f32")

    def scope_chunk(self, frames):
        """frames of one pass of the handle's own rows in a spectra call (0: the default, what 64 MiB of rows hold)"""
        _check(lib().jsdr_bpsk_scope_chunk(self.h, int(frames)), "jsdr_bpsk_scope_chunk")

    def scope_layout(self, nsamples):
        """(L, origin, G[frames + 1]) of a scope call of nsamples from the handle's present counters (host only)"""
        frames = max(int(nsamples) // self.samples, 0)
        ring, origin = C.c_int(), C.c_int64()
        g = np.zeros(frames + 1, np.int64)
        _check(lib().jsdr_bpsk_scope_layout(self.h, C.c_int64(nsamples), C.byref(ring), C.byref(origin), _addr(g), frames + 1),
               "jsdr_bpsk_scope_layout")
        return ring.value, origin.value, g

    def scope_kernel(self):
        """what the last scope call launched, joined with '+' ("" after a call with no output)"""
        return lib().jsdr_bpsk_scope_kernel(self.h).decode()

    def is_recovered(self, stream):
        """fast variant: this stream is served by the exact shadow handle (jsdr_bpsk_recover_uncertified replayed it)"""
        v = C.c_int()
        _check(lib().jsdr_bpsk_stream_recovered(self.h, int(stream), C.byref(v)), "jsdr_bpsk_stream_recovered")
        return bool(v.value)

    def recover_uncertified(self, raw_devs, nsamples, stride_i16, ic=0, qc=0, stream=None):
        """fast variant: replay the streams the calls so far left uncertified on an internal exact handle that serves them from
        then on; raw_devs / nsamples: every call since creation.  Returns the number of streams now served in exact order."""
        n = len(raw_devs)
        ptrs = (C.c_void_p * max(n, 1))(*[_addr(r) for r in raw_devs])
        ns = (C.c_int64 * max(n, 1))(*[int(v) for v in nsamples])
        rec = C.c_int()
        _check(lib().jsdr_bpsk_recover_uncertified(self.h, ptrs, ns, n, C.c_int64(stride_i16), ic, qc, C.byref(rec), C.c_void_p(stream)),
               "jsdr_bpsk_recover_uncertified")
        return rec.value

    def set_cu_share(self, wgs_per_cu):
        _check(lib().jsdr_bpsk_set_cu_share(self.h, int(wgs_per_cu)), "jsdr_bpsk_set_cu_share")

    def pair_shares(self):
        """(fft share, bpsk share) the library recommends for running fft.receive beside this demodulator; (0, 0): one after the other"""
        a, b = C.c_int(), C.c_int()
        _check(lib().jsdr_bpsk_pair_shares(self.h, C.byref(a), C.byref(b)), "jsdr_bpsk_pair_shares")
        return a.value, b.value

    def last_launch(self):
        a, b = C.c_int64(), C.c_int64()
        _check(lib().jsdr_bpsk_last_launch(self.h, C.byref(a), C.byref(b)), "jsdr_bpsk_last_launch")
        return a.value, b.value

    def fm_form(self):
        """(specialised, phase) of the last call's k_fm: (True, 0..7) for the 8-phase tuner's form, (False, -1) otherwise"""
        a, b = C.c_int(), C.c_int()
        _check(lib().jsdr_bpsk_fm_form(self.h, C.byref(a), C.byref(b)), "jsdr_bpsk_fm_form")
        return bool(a.value), b.value

    def sync(self):
        _check(lib().jsdr_bpsk_sync(self.h), "jsdr_bpsk_sync")

    # live control, FUNcubeBPSKDemod.actionPerformed (:165-190): between calls, every stream, nothing else reset
    def set_tuning(self, tuning_hz):
        _check(lib().jsdr_bpsk_set_tuning(self.h, C.c_double(tuning_hz)), "jsdr_bpsk_set_tuning")

    def set_mode(self, do_fft, do_up):
        _check(lib().jsdr_bpsk_set_mode(self.h, int(do_fft), int(do_up)), "jsdr_bpsk_set_mode")

    def reconfigure(self, tuning_hz, do_fft, do_up):
        """setup() (:192-209) on an unchanged format: the configuration's values, dmMaxCorr kept"""
        _check(lib().jsdr_bpsk_reconfigure(self.h, C.c_double(tuning_hz), int(do_fft), int(do_up)), "jsdr_bpsk_reconfigure")

    def control(self):
        """(tuning_hz, do_fft, do_up) now in effect"""
        t, f, u = C.c_double(), C.c_int(), C.c_int()
        _check(lib().jsdr_bpsk_get_control(self.h, C.byref(t), C.byref(f), C.byref(u)), "jsdr_bpsk_get_control")
        return t.value, f.value, u.value

    def counters(self, stream=0):
        out = np.empty(10, np.int32)
        _check(lib().jsdr_bpsk_get_counters(self.h, stream, _addr(out)), "jsdr_bpsk_get_counters")
        return dict(zip(COUNTER_NAMES, (int(v) for v in out)))

    def bits(self, stream=0):
        n = C.c_int()
        _check(lib().jsdr_bpsk_get_bits(self.h, stream, None, 0, C.byref(n)), "jsdr_bpsk_get_bits")
        out = np.empty(max(n.value, 1), np.int8)
        _check(lib().jsdr_bpsk_get_bits(self.h, stream, _addr(out), n.value, C.byref(n)), "jsdr_bpsk_get_bits")
        return out[:n.value]

    def fec_results(self, stream=0):
        cnt = C.c_int()
        _check(lib().jsdr_bpsk_get_fec_count(self.h, stream, C.byref(cnt)), "jsdr_bpsk_get_fec_count")
        res = []
        for i in range(cnt.value):
            rc = C.c_int32()
            bi = C.c_int32()
            out = np.empty(256, np.uint8)
            _check(lib().jsdr_bpsk_get_fec(self.h, stream, i, C.byref(rc), C.byref(bi), _addr(out)),
                   "jsdr_bpsk_get_fec")
            res.append((rc.value, bi.value, out))
        return res

    def decoded(self, stream=0):
        out = np.empty(256, np.uint8)
        _check(lib().jsdr_bpsk_get_decoded(self.h, stream, _addr(out)), "jsdr_bpsk_get_decoded")
        return out

    def trace(self, stream=0):
        n = C.c_int64()
        _check(lib().jsdr_bpsk_get_trace(self.h, stream, None, C.c_int64(0), C.byref(n)), "jsdr_bpsk_get_trace")
        out = np.empty((max(n.value, 1), 2), np.float64)
        _check(lib().jsdr_bpsk_get_trace(self.h, stream, _addr(out), n, C.byref(n)), "jsdr_bpsk_get_trace")
        return out[:n.value]

    def state(self, stream=0):
        out = np.empty(18, np.float64)
        _check(lib().jsdr_bpsk_get_state(self.h, stream, _addr(out)), "jsdr_bpsk_get_state")
        return out

    def profile_enable(self, on=True):
        _check(lib().jsdr_bpsk_profile_enable(self.h, int(on)), "jsdr_bpsk_profile_enable")

    def profile_read(self):
        """{kernel name: (total ms, launches)} since the last read"""
        k = lib().jsdr_bpsk_profile_count()
        ms = np.zeros(k, np.float64)
        cnt = np.zeros(k, np.int32)
        _check(lib().jsdr_bpsk_profile_read(self.h, _addr(ms), _addr(cnt)), "jsdr_bpsk_profile_read")
        return {lib().jsdr_bpsk_profile_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(k)}

    def slot_info(self):
        sb, bo, fo = C.c_int64(), C.c_int64(), C.c_int64()
        nb, nf = C.c_int(), C.c_int()
        _check(lib().jsdr_bpsk_slot_info(self.h, C.byref(sb), C.byref(bo), C.byref(fo), C.byref(nb), C.byref(nf)),
               "jsdr_bpsk_slot_info")
        return dict(slot_bytes=sb.value, bits_offset=bo.value, fec_offset=fo.value, slot_bits=nb.value,
                    nfec_max=nf.value)

    def pack_slots(self, slots_dev, stream=None):  # stream: raw hipStream_t value
        _check(lib().jsdr_bpsk_pack_slots(self.h, _addr(slots_dev), C.c_void_p(stream)), "jsdr_bpsk_pack_slots")

    # checkpoints (jsdr_hip.h "Checkpoints"): the state of a range of streams as a self-contained blob
    def state_bytes(self, count):
        n = C.c_size_t()
        _check(lib().jsdr_bpsk_state_bytes(self.h, int(count), C.byref(n)), "jsdr_bpsk_state_bytes")
        return n.value

    def save(self, first=0, count=None):
        """streams first .. first + count - 1 (None: to the last) -> bytes; the handle is not changed"""
        count = self.nstreams - int(first) if count is None else int(count)
        buf = np.empty(max(self.state_bytes(count), 1), np.uint8)
        n = C.c_size_t()
        _check(lib().jsdr_bpsk_save(self.h, int(first), count, _addr(buf), C.c_size_t(buf.size), C.byref(n)), "jsdr_bpsk_save")
        return buf[:n.value].tobytes()

    def state_kernel_ms(self):
        """(device ms of the last save's k_state_pack, of the last restore's k_state_unpack); -1.0: none yet"""
        a, b = C.c_double(), C.c_double()
        _check(lib().jsdr_bpsk_state_kernel_ms(self.h, C.byref(a), C.byref(b)), "jsdr_bpsk_state_kernel_ms")
        return a.value, b.value

    def restore(self, blob, dst_first=0):
        """all of the blob's streams into streams dst_first ..; a handle that has taken no sample and no blob adopts its shared block"""
        buf = np.frombuffer(bytes(blob), np.uint8)
        _check(lib().jsdr_bpsk_restore(self.h, int(dst_first), _addr(buf) if buf.size else None, C.c_size_t(buf.size)), "jsdr_bpsk_restore")

    def __del__(self):
        try:
            if getattr(self, "borrowed", False):
                return
            lib().jsdr_bpsk_destroy(self.h)
        except Exception:
            pass


class BpskTuned(Bpsk):
    """len(tunings) lock-step FUNcubeBPSKDemod instances in the tune mode, every stream with its own tuning
    (jsdr_bpsk_create_tuned): stream s is a demodulator created with tunings[s]; batches, getters and slots as Bpsk's."""

    def __init__(self, rate, blen, tunings, max_batch_samples=None, size=4):
        tunings = [float(t) for t in tunings]
        self.samples = blen // size
        self.nstreams = len(tunings)
        self.max_batch = max_batch_samples or self.samples
        self.h = C.c_void_p()
        tu = (C.c_double * max(self.nstreams, 1))(*tunings)
        _check(lib().jsdr_bpsk_create_tuned(C.byref(self.h), rate, self.samples, self.nstreams, tu if tunings else None,
                                            C.c_int64(self.max_batch)), "jsdr_bpsk_create_tuned")

    # actionPerformed's tuning change (:174-189) on those streams only, between calls
    def set_stream_tuning(self, stream, tuning_hz):
        _check(lib().jsdr_bpsk_set_stream_tuning(self.h, int(stream), C.c_double(tuning_hz)), "jsdr_bpsk_set_stream_tuning")

    def set_stream_tunings(self, first, tunings):
        tunings = [float(t) for t in tunings]
        tu = (C.c_double * max(len(tunings), 1))(*tunings)
        _check(lib().jsdr_bpsk_set_stream_tunings(self.h, int(first), len(tunings), tu), "jsdr_bpsk_set_stream_tunings")

    def stream_tuning(self, stream):
        t = C.c_double()
        _check(lib().jsdr_bpsk_get_stream_tuning(self.h, int(stream), C.byref(t)), "jsdr_bpsk_get_stream_tuning")
        return t.value

    def plan_tunings(self, streams, at_samples, tunings):
        """retunes inside the next batch call (jsdr_bpsk_plan_stream_tunings): stream streams[i] takes tunings[i] from sample
        at_samples[i] of that call on; entries by stream, then by ascending sample.  No entries: a pending plan is cleared."""
        st = np.ascontiguousarray(streams, np.int32)
        at = np.ascontiguousarray(at_samples, np.int64)
        tu = np.ascontiguousarray(tunings, np.float64)
        if not (st.ndim == at.ndim == tu.ndim == 1 and st.size == at.size == tu.size):
            raise ValueError("plan_tunings: streams, at_samples and tunings are three lists of one length")
        n = st.size
        _check(lib().jsdr_bpsk_plan_stream_tunings(self.h, _addr(st) if n else None, _addr(at) if n else None, _addr(tu) if n else None,
                                                   C.c_int64(n)), "jsdr_bpsk_plan_stream_tunings")

    def plan_ramps(self, streams, at_samples, tunings, slopes):
        """plan_tunings with moving entries (jsdr_bpsk_plan_stream_ramps): from sample at_samples[i] of the next batch call on, sample n
        of stream streams[i] has the tuning tunings[i] + float(n - at_samples[i]) * slopes[i] (Hz, Hz per sample), until the stream's
        next entry or the call's end.  A slope of zero is a step; no entries: a pending plan is cleared."""
        st = np.ascontiguousarray(streams, np.int32)
        at = np.ascontiguousarray(at_samples, np.int64)
        tu = np.ascontiguousarray(tunings, np.float64)
        sl = np.ascontiguousarray(slopes, np.float64)
        if not (st.ndim == at.ndim == tu.ndim == sl.ndim == 1 and st.size == at.size == tu.size == sl.size):
            raise ValueError("plan_ramps: streams, at_samples, tunings and slopes are four lists of one length")
        n = st.size
        _check(lib().jsdr_bpsk_plan_stream_ramps(self.h, _addr(st) if n else None, _addr(at) if n else None, _addr(tu) if n else None,
                                                 _addr(sl) if n else None, C.c_int64(n)), "jsdr_bpsk_plan_stream_ramps")

    def planned(self):
        """entries of a tuning plan waiting for the next batch call"""
        n = C.c_int64()
        _check(lib().jsdr_bpsk_planned_tunings(self.h, C.byref(n)), "jsdr_bpsk_planned_tunings")
        return n.value


class BpskTunedChannels(BpskTuned):
    """`ninputs` inputs x `nchannels` FUNcubeBPSKDemod instances in the tune mode, every channel of every input with its own tuning,
    the channels of an input reading one input row (jsdr_bpsk_create_tuned_channels).  Channel c of input i is stream
    i * nchannels + c and is created with tunings[i * nchannels + c]; retunes, plans and getters by stream, as BpskTuned's."""

    def __init__(self, rate, blen, ninputs, nchannels, tunings, max_batch_samples=None, size=4):
        tunings = [float(t) for t in tunings]
        if len(tunings) != int(ninputs) * int(nchannels):
            raise ValueError("BpskTunedChannels: one tuning per channel of every input (ninputs * nchannels of them)")
        self.samples = blen // size
        self.ninputs = int(ninputs)
        self.nchannels = int(nchannels)
        self.nstreams = self.ninputs * self.nchannels
        self.max_batch = max_batch_samples or self.samples
        self.h = C.c_void_p()
        tu = (C.c_double * max(self.nstreams, 1))(*tunings)
        _check(lib().jsdr_bpsk_create_tuned_channels(C.byref(self.h), rate, self.samples, self.ninputs, self.nchannels,
                                                     tu if tunings else None, C.c_int64(self.max_batch)),
               "jsdr_bpsk_create_tuned_channels")

    def stream(self, inp, ch):
        return inp * self.nchannels + ch

    def channel_info(self):
        a, b = C.c_int(), C.c_int()
        _check(lib().jsdr_bpsk_channel_info(self.h, C.byref(a), C.byref(b)), "jsdr_bpsk_channel_info")
        return a.value, b.value

    def batch_i16(self, raw_dev, input_stride_i16, nsamples, ic=0, qc=0, stream=None):
        """input_stride_i16: between INPUTS"""
        Bpsk.batch_i16(self, raw_dev, input_stride_i16, nsamples, ic, qc, stream)

    def batch_f32(self, iq_dev, input_stride_f32, nsamples, stream=None):
        """input_stride_f32: between INPUTS"""
        Bpsk.batch_f32(self, iq_dev, input_stride_f32, nsamples, stream)


class BpskBlobInfo(C.Structure):
    _fields_ = [("version", C.c_int32), ("kind", C.c_int32), ("rate", C.c_int32), ("nsamples_per_frame", C.c_int32),
                ("nstreams", C.c_int32), ("do_fft", C.c_int32), ("do_up", C.c_int32), ("seam", C.c_int32),
                ("record_bytes", C.c_int32), ("header_bytes", C.c_int32), ("n_in", C.c_int64), ("n_ds", C.c_int64),
                ("tuning_hz", C.c_double)]


def blob_info(blob):
    """what a checkpoint blob says of itself (no device, no handle): the fields of jsdr_bpsk_blob_info_t as a dict"""
    buf = np.frombuffer(bytes(blob), np.uint8)
    info = BpskBlobInfo()
    _check(lib().jsdr_bpsk_blob_info(_addr(buf) if buf.size else None, C.c_size_t(buf.size), C.byref(info)), "jsdr_bpsk_blob_info")
    return {name: getattr(info, name) for name, _ in BpskBlobInfo._fields_}


def tuner_walk_host(tu0, inc, n):
    """the tuner recurrence as the tuned handle's kernels walk it, on the host (no device): n samples from tuPhase tu0 at
    tuPhaseInc inc -> (9-bit table index per sample, 256: passed through; tuPhase at the end)"""
    k9 = np.empty(max(int(n), 1), np.uint16)
    end = C.c_double()
    _check(lib().jsdr_bpsk_tuner_walk_host(C.c_double(tu0), C.c_double(inc), C.c_int64(int(n)), _addr(k9), C.byref(end)),
           "jsdr_bpsk_tuner_walk_host")
    return k9[:int(n)], end.value


def tuner_walk_plan_host(tu0, inc, n, at_samples=(), incs=()):
    """tuner_walk_host with a plan for one stream (no device): from sample at_samples[e] on the increment is incs[e]
    -> (9-bit table index per sample, tuPhase at the end)"""
    at = np.ascontiguousarray(at_samples, np.int64)
    ia = np.ascontiguousarray(incs, np.float64)
    if at.size != ia.size:
        raise ValueError("tuner_walk_plan_host: one increment per position")
    k9 = np.empty(max(int(n), 1), np.uint16)
    end = C.c_double()
    _check(lib().jsdr_bpsk_tuner_walk_plan_host(C.c_double(tu0), C.c_double(inc), C.c_int64(int(n)), _addr(at) if at.size else None,
                                                _addr(ia) if ia.size else None, C.c_int64(at.size), _addr(k9), C.byref(end)),
           "jsdr_bpsk_tuner_walk_plan_host")
    return k9[:int(n)], end.value


def tuner_walk_ramp_host(tu0, inc, n, rate, at_samples=(), tunings=(), slopes=()):
    """tuner_walk_plan_host with ramp entries (no device): from sample at_samples[e] on, sample i has the tuning tunings[e] +
    float(i - at_samples[e]) * slopes[e] and the increment 2 pi tuning / rate -> (9-bit table index per sample, tuPhase at the end,
    tuPhaseInc at the end)"""
    at = np.ascontiguousarray(at_samples, np.int64)
    ta = np.ascontiguousarray(tunings, np.float64)
    sa = np.ascontiguousarray(slopes, np.float64)
    if not at.size == ta.size == sa.size:
        raise ValueError("tuner_walk_ramp_host: one tuning and one slope per position")
    k9 = np.empty(max(int(n), 1), np.uint16)
    end, inc_end = C.c_double(), C.c_double()
    _check(lib().jsdr_bpsk_tuner_walk_ramp_host(C.c_double(tu0), C.c_double(inc), C.c_int64(int(n)), C.c_int(int(rate)),
                                                _addr(at) if at.size else None, _addr(ta) if ta.size else None,
                                                _addr(sa) if sa.size else None, C.c_int64(at.size), _addr(k9), C.byref(end),
                                                C.byref(inc_end)), "jsdr_bpsk_tuner_walk_ramp_host")
    return k9[:int(n)], end.value, inc_end.value


class BpskChannels(Bpsk):
    """`ninputs` inputs x len(tunings) independently tuned FUNcubeBPSKDemod instances (jsdr.java:479-483's nfcs tabs fed the
    same audio).  Channel c of input i is stream i * nchannels + c; every getter takes (input, channel)."""

    def __init__(self, rate, blen, tunings, do_up=None, ninputs=1, max_batch_samples=None, size=4, do_fft=None, live=False):
        """do_fft (per channel, fixed at creation): the channels that run FFT-acquire, each searching the band its do_up names
        (jsdr_bpsk_create_mode_channels); None: jsdr_bpsk_create_channels, every channel in the tune mode.
        live=True: jsdr_bpsk_create_live_channels -- do_fft (None: all 0) gives the initial modes, and set_channel_mode /
        set_mode / reconfigure switch a channel between the modes between calls"""
        tunings = [float(t) for t in tunings]
        self.samples = blen // size
        self.ninputs = ninputs
        self.nchannels = len(tunings)
        self.nstreams = ninputs * self.nchannels
        self.max_batch = max_batch_samples or self.samples
        self.h = C.c_void_p()
        tu = (C.c_double * max(self.nchannels, 1))(*tunings)
        up = None if do_up is None else (C.c_int * max(self.nchannels, 1))(*[int(v) for v in do_up])
        if live:
            ff = None if do_fft is None else (C.c_int * max(self.nchannels, 1))(*[int(v) for v in do_fft])
            _check(lib().jsdr_bpsk_create_live_channels(C.byref(self.h), rate, self.samples, ninputs, self.nchannels,
                                                        tu if tunings else None, ff, up, C.c_int64(self.max_batch)),
                   "jsdr_bpsk_create_live_channels")
            return
        if do_fft is not None:
            ff = (C.c_int * max(self.nchannels, 1))(*[int(v) for v in do_fft])
            _check(lib().jsdr_bpsk_create_mode_channels(C.byref(self.h), rate, self.samples, ninputs, self.nchannels,
                                                        tu if tunings else None, ff, up, C.c_int64(self.max_batch)),
                   "jsdr_bpsk_create_mode_channels")
            return
        _check(lib().jsdr_bpsk_create_channels(C.byref(self.h), rate, self.samples, ninputs, self.nchannels, tu if tunings else None,
                                               up, C.c_int64(self.max_batch)), "jsdr_bpsk_create_channels")

    def acq_last_launch(self):
        """(frames transformed forward, frames inverted) by the last call's FFT-acquire channels"""
        a, b = C.c_int64(), C.c_int64()
        _check(lib().jsdr_bpsk_acq_last_launch(self.h, C.byref(a), C.byref(b)), "jsdr_bpsk_acq_last_launch")
        return a.value, b.value

    def stream(self, inp, ch):
        return inp * self.nchannels + ch

    def channel_info(self):
        a, b = C.c_int(), C.c_int()
        _check(lib().jsdr_bpsk_channel_info(self.h, C.byref(a), C.byref(b)), "jsdr_bpsk_channel_info")
        return a.value, b.value

    def batch_i16(self, raw_dev, input_stride_i16, nsamples, ic=0, qc=0, stream=None):
        """input_stride_i16: between INPUTS"""
        super().batch_i16(raw_dev, input_stride_i16, nsamples, ic, qc, stream)

    def batch_f32(self, iq_dev, input_stride_f32, nsamples, stream=None):
        """input_stride_f32: between INPUTS"""
        super().batch_f32(iq_dev, input_stride_f32, nsamples, stream)

    def set_channel_tuning(self, channel, tuning_hz):
        _check(lib().jsdr_bpsk_set_channel_tuning(self.h, int(channel), C.c_double(tuning_hz)), "jsdr_bpsk_set_channel_tuning")

    def set_channel_mode(self, channel, do_fft, do_up):
        _check(lib().jsdr_bpsk_set_channel_mode(self.h, int(channel), int(do_fft), int(do_up)), "jsdr_bpsk_set_channel_mode")

    def channel_control(self, channel):
        """(tuning_hz, do_fft, do_up) of that channel"""
        t, f, u = C.c_double(), C.c_int(), C.c_int()
        _check(lib().jsdr_bpsk_get_channel_control(self.h, int(channel), C.byref(t), C.byref(f), C.byref(u)),
               "jsdr_bpsk_get_channel_control")
        return t.value, f.value, u.value

    def counters(self, inp=0, ch=0):
        return super().counters(self.stream(inp, ch))

    def bits(self, inp=0, ch=0):
        return super().bits(self.stream(inp, ch))

    def fec_results(self, inp=0, ch=0):
        return super().fec_results(self.stream(inp, ch))

    def decoded(self, inp=0, ch=0):
        return super().decoded(self.stream(inp, ch))

    def trace(self, inp=0, ch=0):
        return super().trace(self.stream(inp, ch))

    def state(self, inp=0, ch=0):
        return super().state(self.stream(inp, ch))


class Group:
    """jsdr_group_*: `total_streams` demodulators of ONE process over `ndev` devices, one host thread per device, the result
    slots gathered to every device after each call (RCCL, or device-to-device copies with gather_copy=True)."""

    def __init__(self, ndev, total_streams, max_batch_samples, devices=None, rate=96000, frame=2048, tuning=12000, do_fft=0,
                 do_up=0, gather_copy=False, with_psd=False):
        self.h = C.c_void_p()
        self.ndev = ndev
        devs = (C.c_int * ndev)(*devices) if devices is not None else None
        flags = (1 if gather_copy else 0) | (2 if with_psd else 0)
        _check(lib().jsdr_group_create(C.byref(self.h), ndev, devs, rate, frame, tuning, do_fft, do_up, total_streams,
                                       C.c_int64(max_batch_samples), flags), "jsdr_group_create")
        n, s, sb, v = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
        _check(lib().jsdr_group_info(self.h, C.byref(n), C.byref(s), C.byref(sb), C.byref(v)), "jsdr_group_info")
        self.streams_per_device, self.slot_bytes, self.rccl_version = s.value, sb.value, v.value
        self.total_streams = total_streams

    def device(self, index):
        """(device ordinal, a borrowed Bpsk view of that device's handle)"""
        d, dem, fft = C.c_int(), C.c_void_p(), C.c_void_p()
        _check(lib().jsdr_group_device(self.h, index, C.byref(d), C.byref(dem), C.byref(fft)), "jsdr_group_device")
        view = Bpsk.__new__(Bpsk)
        view.h, view.nstreams, view.borrowed = dem, self.streams_per_device, True
        return d.value, view

    def batch_i16(self, raw_devs, stride_i16, nsamples, ic=0, qc=0, psd_devs=None):
        raws = (C.c_void_p * self.ndev)(*[_addr(r) for r in raw_devs])
        psds = (C.c_void_p * self.ndev)(*[_addr(p) for p in psd_devs]) if psd_devs is not None else None
        _check(lib().jsdr_group_batch_i16(self.h, raws, C.c_int64(stride_i16), C.c_int64(nsamples), ic, qc, psds),
               "jsdr_group_batch_i16")

    def sync(self):
        _check(lib().jsdr_group_sync(self.h), "jsdr_group_sync")

    def set_tuning(self, tuning_hz):
        _check(lib().jsdr_group_set_tuning(self.h, C.c_double(tuning_hz)), "jsdr_group_set_tuning")

    def set_mode(self, do_fft, do_up):
        _check(lib().jsdr_group_set_mode(self.h, int(do_fft), int(do_up)), "jsdr_group_set_mode")

    def read_slot(self, index, stream):
        out = np.empty(self.slot_bytes, np.uint8)
        _check(lib().jsdr_group_read_slot(self.h, index, stream, _addr(out)), "jsdr_group_read_slot")
        return out

    def gathered(self, index):
        """device `index`'s gathered buffer as a host array [total_streams][slot_bytes] (the device must be current-able)"""
        p, nb = C.c_void_p(), C.c_int64()
        self.sync()
        _check(lib().jsdr_group_gathered(self.h, index, C.byref(p), C.byref(nb)), "jsdr_group_gathered")
        dev, _ = self.device(index)
        out = np.empty(nb.value, np.uint8)
        _check(lib().jsdr_set_device(dev), "jsdr_set_device")
        _check(lib().jsdr_memcpy_d2h(_addr(out), p, C.c_size_t(nb.value)), "jsdr_memcpy_d2h")
        return out.reshape(self.total_streams, self.slot_bytes)

    def __del__(self):
        try:
            lib().jsdr_group_destroy(self.h)
        except Exception:
            pass


def unpack_slot(slot, info):
    """decode one result slot (bytes) -> dict(counters, bits, fec)"""
    hdr = np.frombuffer(slot[:64], np.int32)
    nb, nt = int(hdr[0]), int(hdr[1])
    bits = np.frombuffer(slot[info["bits_offset"]:info["bits_offset"] + nb], np.int8)
    fec = []
    for t in range(nt):
        o = info["fec_offset"] + t * 264
        rc, bi = np.frombuffer(slot[o:o + 8], np.int32)
        fec.append((int(rc), int(bi), np.frombuffer(slot[o + 8:o + 264], np.uint8)))
    names = ["nbits", "nfec"] + COUNTER_NAMES[:9]
    return dict(header=dict(zip(names, (int(v) for v in hdr[:11]))), bits=bits, fec=fec)


def scope_spec_layout(len, plot_width):
    """the BPSK scope's spectra: (first, count) int32 [plot_width], i and l of every column of a spectrum of `len` bins drawn
    plot_width wide, host only (jsdr_bpsk_scope_spec_layout)"""
    out = [np.zeros(max(int(plot_width), 0), np.int32) for _ in range(2)]
    _check(lib().jsdr_bpsk_scope_spec_layout(int(len), int(plot_width), *[_addr(a) if a.size else None for a in out], int(plot_width)),
           "jsdr_bpsk_scope_spec_layout")
    return tuple(out)


# ------------------------------------------------------------------ demod.java
def demod_scope_layout(n, width):
    """demod.paintComponent's two column schedules of (n, width), host only: (trace_first, trace_count, spec_first, spec_count),
    `width` entries each (jsdr_demod_scope_layout)"""
    out = [np.zeros(max(int(width), 0), np.int32) for _ in range(4)]
    _check(lib().jsdr_demod_scope_layout(int(n), int(width), *[_addr(a) if a.size else None for a in out], int(width)),
           "jsdr_demod_scope_layout")
    return tuple(out)


class Demod:
    """demod.receive batched over streams: mode 0 OFF, 1 RAW, 2 AM, 3 NFM, 4 WFM (demod.java:39-43)"""

    def __init__(self, rate=96000, n=2048, nstreams=1, max_batch_samples=None):
        self.rate, self.n, self.S = rate, n, nstreams
        self.max_batch = max_batch_samples or n
        self.h = C.c_void_p()
        _check(lib().jsdr_demod_create(C.byref(self.h), rate, n, nstreams, C.c_int64(self.max_batch)), "jsdr_demod_create")

    def configure(self, mode, dofir=0, dodwn=0, doagc=0):
        _check(lib().jsdr_demod_configure(self.h, mode, dofir, dodwn, doagc), "jsdr_demod_configure")

    def weights(self, flo, fhi):
        w = np.empty(21, np.float32)
        phi = C.c_float()
        _check(lib().jsdr_demod_weights(self.h, flo, fhi, _addr(w), C.byref(phi)), "jsdr_demod_weights")
        return w, np.float32(phi.value)

    def batch_i16(self, raw_dev, stride_i16, nsamples, audio_dev, audio_stride_i16, ic=0, qc=0, stream=None):
        _check(lib().jsdr_demod_batch_i16(self.h, _addr(raw_dev), C.c_int64(stride_i16), C.c_int64(nsamples), ic, qc,
                                          _addr(audio_dev), C.c_int64(audio_stride_i16), C.c_void_p(stream)),
               "jsdr_demod_batch_i16")

    def batch_f32(self, iq_dev, stride_f32, nsamples, audio_dev, audio_stride_i16, stream=None):
        """float IQ [S][stride_f32] (JavaAudio's (float)s/32767f frames, or any float) -> int16 audio, as batch_i16"""
        _check(lib().jsdr_demod_batch_f32(self.h, _addr(iq_dev), C.c_int64(stride_f32), C.c_int64(nsamples),
                                          _addr(audio_dev), C.c_int64(audio_stride_i16), C.c_void_p(stream)),
               "jsdr_demod_batch_f32")

    def batch_host_i16(self, raw, nsamples, ic=0, qc=0):
        """raw: int16 [S][2*nsamples] on the host -> audio int16 [S][2*nsamples]"""
        raw = np.ascontiguousarray(raw, np.int16).reshape(self.S, 2 * nsamples)
        d_in = DeviceBuffer.from_host(raw)
        d_out = DeviceBuffer(raw.nbytes)
        self.batch_i16(d_in, 2 * nsamples, nsamples, d_out, 2 * nsamples, ic, qc)
        return d_out.to_host(np.int16).reshape(self.S, 2 * nsamples)

    def receive(self, buf):
        buf = np.ascontiguousarray(buf, np.float32)
        assert buf.size == 2 * self.n
        out = np.empty(2 * self.n, np.int16)
        _check(lib().jsdr_demod_receive_f32(self.h, _addr(buf), _addr(out)), "jsdr_demod_receive_f32")
        return out

    def frame_stats(self, stream=0):
        mx, av = C.c_float(), C.c_float()
        _check(lib().jsdr_demod_frame_stats(self.h, stream, C.byref(mx), C.byref(av)), "jsdr_demod_frame_stats")
        return np.float32(mx.value), np.float32(av.value)

    def state(self):
        car, phi = C.c_float(), C.c_float()
        _check(lib().jsdr_demod_state(self.h, C.byref(car), C.byref(phi)), "jsdr_demod_state")
        return np.float32(car.value), np.float32(phi.value)

    def scope_i16(self, raw_dev, stride_i16, nsamples, audio_dev, audio_stride_i16, width, height, trace_dev=None, spec_dev=None,
                  dbg_dev=None, ic=0, qc=0, stream=None):
        """batch_i16 plus demod.paintComponent for every frame of the call (jsdr_demod_scope_i16): trace_dev / spec_dev int32
        [S * frames][width], dbg_dev float32 [S * frames][2n], each optional, rows packed, row = stream * frames + frame"""
        _check(lib().jsdr_demod_scope_i16(self.h, _addr(raw_dev), C.c_int64(stride_i16), C.c_int64(nsamples), int(ic), int(qc),
                                          _addr(audio_dev), C.c_int64(audio_stride_i16), int(width), int(height), _addr(trace_dev),
                                          _addr(spec_dev), _addr(dbg_dev), C.c_void_p(stream)), "jsdr_demod_scope_i16")

    def scope_f32(self, iq_dev, stride_f32, nsamples, audio_dev, audio_stride_i16, width, height, trace_dev=None, spec_dev=None,
                  dbg_dev=None, stream=None):
        _check(lib().jsdr_demod_scope_f32(self.h, _addr(iq_dev), C.c_int64(stride_f32), C.c_int64(nsamples), _addr(audio_dev),
                                          C.c_int64(audio_stride_i16), int(width), int(height), _addr(trace_dev), _addr(spec_dev),
                                          _addr(dbg_dev), C.c_void_p(stream)), "jsdr_demod_scope_f32")

    def scope_chunk(self, frames):
        """frames of one scope pass (0: the default, what 64 MiB of rows hold)"""
        _check(lib().jsdr_demod_scope_chunk(self.h, int(frames)), "jsdr_demod_scope_chunk")

    def scope_kernel(self):
        """what the last scope_* call launched, joined with '+': "k_demod_scope_front+k_demod_trace+k_fft+k_demod_spec" """
        return lib().jsdr_demod_scope_kernel(self.h).decode()

    def profile_enable(self, on):
        _check(lib().jsdr_demod_profile_enable(self.h, int(on)), "jsdr_demod_profile_enable")

    def profile_read(self):
        k = lib().jsdr_demod_profile_count()
        ms = np.zeros(k, np.float64)
        cnt = np.zeros(k, np.int32)
        _check(lib().jsdr_demod_profile_read(self.h, _addr(ms), _addr(cnt)), "jsdr_demod_profile_read")
        return {lib().jsdr_demod_profile_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(k)}

    def __del__(self):
        try:
            lib().jsdr_demod_destroy(self.h)
        except Exception:
            pass


class DemodChannels(Demod):
    """`ninputs` inputs x `nchannels` independently controlled demod.receive channels (each its own band, NCO, mode and
    switches).  Channel c of input i is stream i * nchannels + c; `frame_stats` takes that stream index."""

    def __init__(self, rate=96000, n=2048, ninputs=1, nchannels=1, max_batch_samples=None):
        self.rate, self.n, self.ninputs, self.nchannels = rate, n, ninputs, nchannels
        self.S = ninputs * nchannels
        self.max_batch = max_batch_samples or n
        self.h = C.c_void_p()
        _check(lib().jsdr_demod_create_channels(C.byref(self.h), rate, n, ninputs, nchannels, C.c_int64(self.max_batch)),
               "jsdr_demod_create_channels")

    def stream(self, inp, ch):
        return inp * self.nchannels + ch

    def channel_info(self):
        a, b = C.c_int(), C.c_int()
        _check(lib().jsdr_demod_channel_info(self.h, C.byref(a), C.byref(b)), "jsdr_demod_channel_info")
        return a.value, b.value

    def configure_channel(self, channel, mode, dofir=0, dodwn=0, doagc=0):
        _check(lib().jsdr_demod_configure_channel(self.h, int(channel), int(mode), int(dofir), int(dodwn), int(doagc)),
               "jsdr_demod_configure_channel")

    def channel_weights(self, channel, flo, fhi):
        w = np.empty(21, np.float32)
        phi = C.c_float()
        _check(lib().jsdr_demod_channel_weights(self.h, int(channel), int(flo), int(fhi), _addr(w), C.byref(phi)),
               "jsdr_demod_channel_weights")
        return w, np.float32(phi.value)

    def channel_control(self, channel):
        """(mode, dofir, dodwn, doagc, flo, fhi) of that channel"""
        v = [C.c_int() for _ in range(6)]
        _check(lib().jsdr_demod_get_channel(self.h, int(channel), *[C.byref(x) for x in v]), "jsdr_demod_get_channel")
        return tuple(x.value for x in v)

    def channel_state(self, channel):
        car, phi = C.c_float(), C.c_float()
        _check(lib().jsdr_demod_channel_state(self.h, int(channel), C.byref(car), C.byref(phi)), "jsdr_demod_channel_state")
        return np.float32(car.value), np.float32(phi.value)

    def batch_i16(self, raw_dev, input_stride_i16, nsamples, audio_dev, audio_stride_i16, ic=0, qc=0, stream=None):
        """input_stride_i16: between INPUTS; audio_stride_i16: between the ninputs * nchannels output rows"""
        super().batch_i16(raw_dev, input_stride_i16, nsamples, audio_dev, audio_stride_i16, ic, qc, stream)

    def batch_f32(self, iq_dev, input_stride_f32, nsamples, audio_dev, audio_stride_i16, stream=None):
        super().batch_f32(iq_dev, input_stride_f32, nsamples, audio_dev, audio_stride_i16, stream)

    def batch_host_i16(self, raw, nsamples, ic=0, qc=0):
        """raw: int16 [ninputs][2*nsamples] on the host -> audio int16 [ninputs][nchannels][2*nsamples]"""
        raw = np.ascontiguousarray(raw, np.int16).reshape(self.ninputs, 2 * nsamples)
        d_in = DeviceBuffer.from_host(raw)
        d_out = DeviceBuffer(self.S * 2 * nsamples * 2)
        self.batch_i16(d_in, 2 * nsamples, nsamples, d_out, 2 * nsamples, ic, qc)
        return d_out.to_host(np.int16).reshape(self.ninputs, self.nchannels, 2 * nsamples)

    def receive(self, buf):
        """one frame (2n floats) of a 1-input handle -> int16 [nchannels][2n]"""
        buf = np.ascontiguousarray(buf, np.float32)
        assert buf.size == 2 * self.n
        out = np.empty(self.nchannels * 2 * self.n, np.int16)
        _check(lib().jsdr_demod_receive_f32(self.h, _addr(buf), _addr(out)), "jsdr_demod_receive_f32")
        return out.reshape(self.nchannels, 2 * self.n)


# ------------------------------------------------------------------ formats either side
class RecordingInfo(C.Structure):
    _fields_ = [("format", C.c_int), ("encoding", C.c_int), ("channels", C.c_int), ("rate", C.c_int),
                ("bits", C.c_int), ("frames", C.c_int64), ("data_offset", C.c_int64)]


def waterfall_lines(psd, n, width, peak_rgb=0x00FFFF):
    """waterfall.paintLine for every frame of psd [nframes][n+2] -> uint32 ARGB [nframes][width]"""
    psd = np.ascontiguousarray(psd, np.float32).reshape(-1, n + 2)
    d_in = DeviceBuffer.from_host(psd)
    d_out = DeviceBuffer(4 * psd.shape[0] * width)
    _check(lib().jsdr_waterfall_lines(_addr(d_in), C.c_int64(psd.shape[0]), n, width, C.c_uint32(peak_rgb),
                                      _addr(d_out), None), "jsdr_waterfall_lines")
    return d_out.to_host(np.uint32).reshape(psd.shape[0], width)


def waterfall_lines_dev(psd_dev, nframes, n, width, pix_dev, peak_rgb=0x00FFFF, stream=None):
    _check(lib().jsdr_waterfall_lines(_addr(psd_dev), C.c_int64(nframes), n, width, C.c_uint32(peak_rgb),
                                      _addr(pix_dev), C.c_void_p(stream)), "jsdr_waterfall_lines")


def recording_probe(path, raw_channels=2):
    info = RecordingInfo()
    _check(lib().jsdr_recording_probe(os.fsencode(path), raw_channels, C.byref(info)), "jsdr_recording_probe")
    return info


def recordings_load(paths, channels, rate, first_frame, nframes, raw_dev, stream_stride_i16):
    """files -> raw_dev[s*stride ...] as int16 (I,Q) pairs; returns the frames really read per stream"""
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    got = (C.c_int64 * len(paths))()
    _check(lib().jsdr_recordings_load(arr, len(paths), channels, rate, C.c_int64(first_frame), C.c_int64(nframes),
                                      _addr(raw_dev), C.c_int64(stream_stride_i16), got, None), "jsdr_recordings_load")
    return list(got)


# ------------------------------------------------------------------ synthetic inputs
def synth_mix64(z):
    """splitmix64 finaliser: the counter hash of the synthetic-input generators (csrc/synth.hip)"""
    m = 0xFFFFFFFFFFFFFFFF
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def synth_carrier_tables(amp):
    """1024-entry int16 cos / sin tables of amplitude amp (round half to even), the carrier of jsdr_synth_dbpsk / _tones"""
    a = 2.0 * np.pi * np.arange(1024, dtype=np.float64) / 1024.0
    return np.rint(amp * np.cos(a)).astype(np.int16), np.rint(amp * np.sin(a)).astype(np.int16)


def synth_phase_inc_u32(freq_hz, rate):
    return int(round(freq_hz / rate * 2 ** 32)) & 0xFFFFFFFF


def synth_payloads(seed, stream0, nstreams, nframes, out_dev=None, stream=None):
    own = out_dev is None
    if own:
        out_dev = DeviceBuffer(nstreams * nframes * 256)
    _check(lib().jsdr_synth_payloads(C.c_uint64(seed), stream0, nstreams, nframes, _addr(out_dev), C.c_void_p(stream)),
           "jsdr_synth_payloads")
    return out_dev


def synth_diffsign(sym_dev, nsym, nstreams, dsign_dev, stream=None):
    _check(lib().jsdr_synth_diffsign(_addr(sym_dev), C.c_int64(nsym), nstreams, _addr(dsign_dev), C.c_void_p(stream)),
           "jsdr_synth_diffsign")


def synth_dbpsk(out_dev, stride_i16, nstreams, n0, n, dsign_dev, nsym, sps, phase0, phase_inc, cos_dev, sin_dev,
                noise_gain, keys_dev, stream=None):
    _check(lib().jsdr_synth_dbpsk(_addr(out_dev), C.c_int64(stride_i16), nstreams, C.c_int64(n0), C.c_int64(n),
                                  _addr(dsign_dev), C.c_int64(nsym), sps, C.c_uint32(phase0), C.c_uint32(phase_inc),
                                  _addr(cos_dev), _addr(sin_dev), noise_gain, _addr(keys_dev), C.c_void_p(stream)),
           "jsdr_synth_dbpsk")


def synth_tones(out_dev, frame0, nframes, n, cos_dev, noise_gain, key, stream=None):
    _check(lib().jsdr_synth_tones(_addr(out_dev), C.c_int64(frame0), C.c_int64(nframes), n, _addr(cos_dev), noise_gain,
                                  C.c_uint64(key), C.c_void_p(stream)), "jsdr_synth_tones")
