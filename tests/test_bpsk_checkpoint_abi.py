"""The checkpoint C ABI (jsdr_bpsk_state_bytes / _save / _restore / _blob_info): declared with its prototypes, exported, bound,
and checked before any device work.  jsdr_bpsk_blob_info needs neither a device nor a handle: it is given damaged blobs here,
and the golden blob (tests/golden/bpsk_checkpoint_v1.bin, written by the library on an MI355X: tools/make_checkpoint_golden.py),
whose recorded fields it must report."""
import ctypes as C
import os
import re

import pytest

import java_sdr_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "jsdr_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bpsk_checkpoint_v1.bin")
PROTOTYPES = {
    "jsdr_bpsk_state_bytes": "int jsdr_bpsk_state_bytes(jsdr_bpsk *h, int count, size_t *bytes);",
    "jsdr_bpsk_save": "int jsdr_bpsk_save(jsdr_bpsk *h, int first, int count, void *blob_host, size_t cap, size_t *bytes);",
    "jsdr_bpsk_restore": "int jsdr_bpsk_restore(jsdr_bpsk *h, int dst_first, const void *blob_host, size_t bytes);",
    "jsdr_bpsk_blob_info": "int jsdr_bpsk_blob_info(const void *blob_host, size_t bytes, jsdr_bpsk_blob_info_t *out);",
    "jsdr_bpsk_state_kernel_ms": "int jsdr_bpsk_state_kernel_ms(jsdr_bpsk *h, double *pack_ms, double *unpack_ms);",
}


def _code(text):
    """the header without its comments, white space folded"""
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))


def test_checkpoint_symbols_are_declared_exported_and_bound():
    code = _code(open(HDR).read())
    lib = J.lib()
    for name, proto in PROTOTYPES.items():
        assert name in J.EXPORTED_SYMBOLS, name
        assert _code(proto).strip() in code, proto
        assert hasattr(lib, name), name
    for m in ("save", "restore", "state_bytes"):
        assert callable(getattr(J.Bpsk, m, None)), m
        assert getattr(J.BpskTuned, m) is getattr(J.Bpsk, m) and getattr(J.BpskChannels, m) is getattr(J.Bpsk, m)
    assert callable(J.blob_info)
    assert "typedef struct jsdr_bpsk_blob_info_t" in code


def test_header_names_what_a_checkpoint_does_not_cover():
    text = open(HDR).read()
    start = text.index("Checkpoints:")
    comment = re.sub(r"\s+", " ", text[start:text.index("*/", start)])
    for what in ("shared-block rule", "ADOPTS", "exactly as it was", "checksum"):
        assert what in comment, what
    tail = comment[comment.index("Not covered"):]
    for what in ("channel handles", "FAST variant", "jsdr_group_*", "JNI / Java classes", "jsdr_demod_*"):
        assert what in tail, what


@pytest.mark.parametrize("name,call", [
    ("jsdr_bpsk_state_bytes", lambda lib: lib.jsdr_bpsk_state_bytes(None, 1, C.byref(C.c_size_t()))),
    ("jsdr_bpsk_save", lambda lib: lib.jsdr_bpsk_save(None, 0, 1, C.create_string_buffer(16), C.c_size_t(16), C.byref(C.c_size_t()))),
    ("jsdr_bpsk_restore", lambda lib: lib.jsdr_bpsk_restore(None, 0, C.create_string_buffer(16), C.c_size_t(16))),
    ("jsdr_bpsk_state_kernel_ms", lambda lib: lib.jsdr_bpsk_state_kernel_ms(None, C.byref(C.c_double()), C.byref(C.c_double()))),
    ("jsdr_bpsk_blob_info", lambda lib: lib.jsdr_bpsk_blob_info(None, C.c_size_t(16), C.byref(J.binding.BpskBlobInfo()))),
    ("jsdr_bpsk_blob_info", lambda lib: lib.jsdr_bpsk_blob_info(C.create_string_buffer(16), C.c_size_t(16), None)),
])
def test_checkpoint_calls_refuse_null_arguments(name, call):
    assert call(J.lib()) != 0
    msg = J.lib().jsdr_last_error().decode()
    assert name in msg and "null" in msg, msg


def _golden():
    return open(GOLDEN, "rb").read()


def test_blob_info_refuses_what_is_not_a_blob():
    good = _golden()
    wrong_magic = b"X" + good[1:]
    wrong_version = good[:8] + (2).to_bytes(4, "little") + good[12:]
    for blob, what in ((b"", "null"), (good[:7], "too short"), (wrong_magic, "magic"), (wrong_version, "version"),
                       (good[:-1], "truncated"), (good[:300] + bytes([good[300] ^ 0x40]) + good[301:], "checksum")):
        with pytest.raises(J.JsdrError) as e:
            J.blob_info(blob)
        assert "jsdr_bpsk_blob_info" in str(e.value) and what in str(e.value), str(e.value)
    # ... and straight through the C ABI, with the sizes as given
    lib = J.lib()
    info = J.binding.BpskBlobInfo()
    for blob in (b"", good[:7], wrong_magic, wrong_version):
        buf = C.create_string_buffer(blob, max(len(blob), 1))
        assert lib.jsdr_bpsk_blob_info(buf, C.c_size_t(len(blob)), C.byref(info)) != 0
        assert "jsdr_bpsk_blob_info" in lib.jsdr_last_error().decode()


def test_a_forged_checksum_does_not_get_out_of_range_values_through():
    """the header's index-like values are range-checked behind the checksum: each is set out of range and the checksum recomputed"""
    import struct
    good = _golden()

    def fnv1a(data):
        h = 0xcbf29ce484222325
        for b in data:
            h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
        return h

    def forged(off, fmt, val):
        b = bytearray(good)
        struct.pack_into(fmt, b, off, val)
        struct.pack_into("<Q", b, 24, fnv1a(bytes(b[32:])))
        return bytes(b)
    assert J.blob_info(forged(104, "<d", 12000.0))["tuning_hz"] == 12000.0  # (the forging itself is sound)
    for off, fmt, val, what in ((104, "<d", float("nan"), "tuning"), (112, "<d", float("inf"), "tuPhase"), (112, "<d", 1e9, "tuPhase"),
                                (120, "<d", float("nan"), "tuPhaseInc"), (128, "<d", 7.0, "vcoPhase"), (128, "<d", -1.0, "vcoPhase"),
                                (76, "<i", 10, "counters"), (76, "<i", -1, "counters"), (88, "<q", -5, "counters"),
                                (64, "<I", 3, "flag"), (162, "<B", 2, "mix flag"), (44, "<I", 2, "flag")):
        with pytest.raises(J.JsdrError) as e:
            J.blob_info(forged(off, fmt, val))
        assert "jsdr_bpsk_blob_info" in str(e.value) and what in str(e.value), (off, str(e.value))


def test_blob_info_reports_the_golden_blob():
    """2 streams of make_dbpsk_stream(777, s, 65536) at 96 kHz, tuning 12000, cut after 40000 samples"""
    blob = _golden()
    assert len(blob) == 192 + 2 * 7184
    assert J.blob_info(blob) == dict(version=1, kind=0, rate=96000, nsamples_per_frame=2, nstreams=2, do_fft=0, do_up=0, seam=0,
                                     record_bytes=7184, header_bytes=192, n_in=40000, n_ds=4000, tuning_hz=12000.0)
