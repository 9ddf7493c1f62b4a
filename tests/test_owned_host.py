"""The move-only owner of HIP objects (java-sdr_amd/csrc/common.h: Owned, behind every handle's streams and events) on the
CPU: a stand-alone program (tests/tools/owned_driver.hip) instantiates it with an integer handle and a destroy function that
counts, and asserts the rules of ownership -- nothing destroyed by an empty owner, exactly one destroy per handle through
destruction, moves, self-assignment, reset(), a reallocating std::vector and std::swap.  Compiled with build.py's flags twice,
plainly and with -fsanitize=address,undefined on the host side; the sanitized build must have nothing to report.

No device and no library.  The static_asserts next to the types in common.h (DevBuf, Stream, Event, PinnedStage: not
copyable, nothrow-movable) are compiled with it."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_py():
    spec = importlib.util.spec_from_file_location("jsdr_build", os.path.join(ROOT, "java-sdr_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("kind", ["plain", "sanitized"])
def test_every_handle_is_destroyed_exactly_once(kind, tmp_path):
    b = _build_py()
    cc = b.hipcc()
    if not (os.path.exists(cc) if os.path.isabs(cc) else shutil.which(cc)):
        pytest.skip("no hipcc found: the owner's driver cannot be compiled")
    exe = str(tmp_path / "owned_driver")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if kind == "sanitized" else []
    cmd = [cc] + b.COMMON + extra + [os.path.join(ROOT, "tests", "tools", "owned_driver.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "warning" not in r.stderr, r.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stderr == ""  # (the sanitized build: nothing to report)
    out = p.stdout.split()
    assert out[0] == "ok" and int(out[1]) >= 130, p.stdout
