"""The checkpoint blob's codec (java-sdr_amd/csrc/bpsk_blob.hip) on the CPU: a stand-alone program (tests/tools/blob_driver.hip)
is compiled with the unit alone, with the flags build.py gives it, twice -- plainly and with -fsanitize=address,undefined on
the host side.  It writes a 3-stream blob of patterned records through the codec's writer, parses it back field for field,
and gives the parser every truncation of the blob (each in a heap block of exactly its length, so that a read past the end is
a sanitizer report) and the blob with each single byte inverted in turn.  Every one of those inputs must be refused, and the
sanitized build must have nothing to report.

No device and no library: the parser is what stands between bytes from a file or a network and a handle's device buffers.
The layout the program wrote is then read here, byte by byte, against the offsets bpsk_blob.h documents."""
import importlib.util
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "java-sdr_amd", "csrc")
HEADER, RECORD, NSTREAMS = 192, 7184, 3


def _build_py():
    spec = importlib.util.spec_from_file_location("jsdr_build", os.path.join(ROOT, "java-sdr_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver_run(request, tmp_path_factory):
    b = _build_py()
    cc = b.hipcc()
    if not (os.path.exists(cc) if os.path.isabs(cc) else shutil.which(cc)):
        pytest.skip("no hipcc found: the blob driver cannot be compiled")
    d = tmp_path_factory.mktemp("blob")
    exe = str(d / "blob_driver")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    cmd = [cc] + b.COMMON + b.SOURCES["bpsk_blob.hip"] + extra + [os.path.join(ROOT, "tests", "tools", "blob_driver.hip"),
                                                                 os.path.join(CSRC, "bpsk_blob.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = str(d / "blob.bin")
    p = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)
    return p, open(out, "rb").read() if os.path.exists(out) else b""


def test_round_trip_and_every_truncation_and_flip_is_refused(driver_run):
    p, blob = driver_run
    assert p.returncode == 0, p.stderr
    assert p.stderr == ""  # (the sanitized build: nothing to report)
    total = HEADER + NSTREAMS * RECORD
    # one parse of every length 0 .. total - 1, one of every inverted byte: all refused
    assert p.stdout.split() == ["ok", str(total), str(total), str(total)]
    assert len(blob) == total


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_the_layout_is_the_documented_one(driver_run):
    """the header of the blob the program wrote, read with struct at the offsets of bpsk_blob.h; the checksum restated"""
    p, blob = driver_run
    assert p.returncode == 0, p.stderr
    assert blob[:8] == b"JSDRBPSK"
    version, hbytes, rbytes, zero = struct.unpack_from("<4I", blob, 8)
    assert (version, hbytes, rbytes, zero) == (1, HEADER, RECORD, 0)
    (checksum, total), (count, kind, rate, nsf, do_fft, do_up, seam, hfloat, fftst) = struct.unpack_from("<2Q", blob, 24), struct.unpack_from("<9I", blob, 40)
    assert total == len(blob) and checksum == fnv1a(blob[32:])
    assert (count, kind, rate, nsf, do_fft, do_up, seam, hfloat, fftst) == (NSTREAMS, 0, 96000, 2048, 1, 1, 1, 1, 1)
    ds_cnt, roff, zero2 = struct.unpack_from("<iII", blob, 76)
    assert (ds_cnt, roff, zero2) == (7, HEADER, 0)
    n_in, n_ds = struct.unpack_from("<2q", blob, 88)
    assert (n_in, n_ds) == (0x123456789a, 0x12345678a)
    tuning, tu, inc, vco = struct.unpack_from("<4d", blob, 104)
    assert (tuning, tu, inc) == (12345.678, 1.25, 0.8080808080808081) and vco == 0.0 and struct.pack("<d", vco)[7] == 0x80  # -0.0 kept
    assert all(v <= 1 for v in blob[162:188]) and blob[188:192] == b"\0" * 4
    # a record: the zero words between its fields, and a register of -1 / 0 / +1 entries
    for i in range(NSTREAMS):
        rec = blob[HEADER + i * RECORD:HEADER + (i + 1) * RECORD]
        assert rec[156:160] == b"\0" * 4 and rec[180:192] == b"\0" * 12 and rec[424:432] == b"\0" * 8 and rec[484:496] == b"\0" * 12
        assert set(struct.unpack_from("<5200b", rec, 1984)) <= {-1, 0, 1}
        assert all(k <= 256 for k in struct.unpack_from("<26H", rec, 432))
