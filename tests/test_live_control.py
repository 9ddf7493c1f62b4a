"""Live control of a BPSK demodulator (FUNcubeBPSKDemod.actionPerformed, :165-190) without a GPU: the C ABI's five entry
points, its refusals that need no device, the fixture pin (tests/golden/live_control_fixtures.npz regenerated for one
scenario), the restatement held against the unmodified C oracle up to the first action, and the JNI natives of
HipLiveControl.java against their C definitions."""
import hashlib
import os
import re
import sys

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import live_control_cases as M  # noqa: E402

FX = np.load(os.path.join(HERE, "golden", "live_control_fixtures.npz"))
LIVE = ["jsdr_bpsk_set_tuning", "jsdr_bpsk_set_mode", "jsdr_bpsk_get_control", "jsdr_bpsk_reconfigure", "jsdr_group_set_tuning", "jsdr_group_set_mode"]
REFERENCE = os.environ.get("JSDR_REFERENCE", "/root/reference")


def test_the_library_exports_and_the_header_declares_the_live_control_calls():
    lib = J.lib()
    for name in LIVE:
        assert name in J.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name


def test_live_control_refuses_a_null_handle():
    import ctypes as C
    lib = J.lib()
    assert lib.jsdr_bpsk_set_tuning(None, C.c_double(12010.0)) == -1
    assert b"null handle" in lib.jsdr_last_error()
    assert lib.jsdr_bpsk_set_mode(None, 0, 1) == -1
    assert b"null handle" in lib.jsdr_last_error()
    t, f, u = C.c_double(), C.c_int(), C.c_int()
    assert lib.jsdr_bpsk_get_control(None, C.byref(t), C.byref(f), C.byref(u)) == -1
    assert lib.jsdr_group_set_tuning(None, C.c_double(0.0)) == -1
    assert lib.jsdr_group_set_mode(None, 0, 0) == -1


def test_fixture_inputs_are_the_committed_ones():
    for name in M.SCENARIOS:
        raw = M.scenario_input(name)
        assert hashlib.sha256(raw.tobytes()).digest() == FX["l_" + name + "_sha256"].tobytes(), name


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the restatement parses its tables from the reference's source text")
def test_generator_reproduces_the_committed_fixture():
    import make_live_control_fixtures as G  # (imports the restatement, which reads the reference's source text)
    got = G.run(M.PIN)
    for k, v in got.items():
        assert v.tobytes() == FX[k].tobytes(), k


@pytest.mark.parametrize("name", list(M.SCENARIOS))
def test_restatement_agrees_with_the_oracle_up_to_the_first_action(name):
    """the unmodified C oracle (no live control) and the restatement, call by call, before anything is changed"""
    p = M.SCENARIOS[name]
    k = "l_" + name + "_"
    raw = M.scenario_input(name)
    first = int(FX[k + "act_call"][0])
    assert first >= 1
    n = p["frame"]
    o = O.Bpsk(rate=p["rate"], blen=4 * n, tuning=p["tuning"], do_fft=p["do_fft"], do_up=p["do_up"])
    pos = 0
    for c, L in enumerate(p["calls"][:first]):
        if p["do_fft"]:
            for f in range(L // n):
                o.receive_i16(raw[2 * (pos + f * n):2 * (pos + (f + 1) * n)])
        else:
            o.receive_i16(raw[2 * pos:2 * (pos + L)])
        pos += L
        assert list(o.counters().values()) == [int(v) for v in FX[k + "counters"][c]], (name, c)
        st = np.array(o.state(), np.float64)
        assert st.tobytes() == FX[k + "state"][c].tobytes(), (name, c)
    nb = int(FX[k + "nbits"][first - 1])
    assert np.array_equal(o.bits(), FX[k + "bits"][:nb])


def _strip(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


JNI_TYPES = {"long": "jlong", "int": "jint", "double": "jdouble", "float": "jfloat", "byte[]": "jbyteArray",
             "float[]": "jfloatArray", "int[]": "jintArray", "double[]": "jdoubleArray"}


def test_every_live_control_native_has_a_matching_jni_definition():
    jsrc = _strip(open(os.path.join(ROOT, "java", "com", "ashbysoft", "java_sdr", "HipLiveControl.java")).read())
    csrc = _strip(open(os.path.join(ROOT, "jni", "jsdr_jni.c")).read())
    nat = {m.group(2): (m.group(1), [a.split()[0] for a in m.group(3).split(",") if a.strip()])
           for m in re.finditer(r"static\s+native\s+(\w+)\s+(\w+)\s*\(([^)]*)\)\s*;", jsrc)}
    assert set(nat) == {"bpskSetTuning", "bpskSetMode", "bpskReconfigure"}
    pre = "Java_com_ashbysoft_java_1sdr_HipLiveControl_"
    jni = {m.group(2): (m.group(1), [a.split()[0] for a in m.group(3).split(",")])
           for m in re.finditer(r"JNIEXPORT\s+(\w+)\s+JNICALL\s+" + pre + r"(\w+)\s*\(([^)]*)\)", csrc)}
    assert set(jni) == set(nat)
    for name, (ret, args) in nat.items():
        cret, cargs = jni[name]
        assert cret == ("void" if ret == "void" else JNI_TYPES[ret]), name
        assert cargs[:2] == ["JNIEnv", "jclass"], name
        assert cargs[2:] == [JNI_TYPES[a] for a in args], (name, cargs, args)
    # the plugin's actions reach them
    plug = _strip(open(os.path.join(ROOT, "java", "com", "ashbysoft", "java_sdr", "HipFUNcubeBPSKDemod.java")).read())
    assert set(re.findall(r"HipLiveControl\.(\w+)\s*\(", plug)) == set(nat)
    for action in ("plus10", "sub10", "setFrequency", "toggleFft", "toggleHigh"):
        assert re.search(r"public\s+synchronized\s+void\s+" + action + r"\s*\(", plug), action
    assert "retune(" not in plug
