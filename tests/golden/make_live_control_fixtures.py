#!/usr/bin/env python3
"""Generate tests/golden/live_control_fixtures.npz: the demodulator driven through FUNcubeBPSKDemod.actionPerformed
(:165-190) between calls, restated in pure Python (live_control.py over java_restatement.py).

Per scenario: the input's sha256, the call lengths, the action schedule (before which call, which command, the value
freqDialog returned), and after EVERY call the 10 counters (jsdr_bpsk_get_counters' layout, centreBin in the last), the
18 state doubles (jsdr_bpsk_get_state's layout) and the bits sliced so far; the FECDecode log (rc, bit index, bytes).
Runs where the reference's source text is (java_restatement parses its tables from it):

    python tests/golden/make_live_control_fixtures.py        (about a minute)
"""
import hashlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import java_restatement as J  # noqa: E402
import live_control as LC  # noqa: E402
import oracle_lib as O  # noqa: E402  (the twiddle table's generator)
from live_control_cases import SCENARIOS, PIN, scenario_input  # noqa: E402,F401

def run(name):
    p = SCENARIOS[name]
    raw = scenario_input(name)
    buf = J.convert_i16(raw)
    n = p["frame"]
    tw = [float(v) for v in O.fft_twiddles_f64(n)]
    d = LC.make_demod(n, tw, p["rate"], p["tuning"], p["do_fft"], p["do_up"])
    acts = {}
    for k, cmd, v in p["actions"]:
        acts.setdefault(k, []).append((cmd, v))
    counters, states, nbits = [], [], []
    pos = 0
    for k, L in enumerate(p["calls"]):
        for cmd, v in acts.get(k, []):
            LC.action_performed(d, cmd, v)
        if d.doFFT:
            for f in range(L // n):
                LC.receive(d, buf[2 * (pos + f * n):2 * (pos + (f + 1) * n)])
        else:
            LC.receive(d, buf[2 * pos:2 * (pos + L)])
        pos += L
        c = d.counters()
        c[9] = d.centreBin if d.doFFT else 0
        counters.append(c)
        st = d.state()
        if d.doFFT:
            st[6], st[7] = d.avePeakPower, d.aveCentreBin
        states.append(st)
        nbits.append(len(d.bits))
    k = "l_" + name + "_"
    out = {
        k + "sha256": np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), np.uint8),
        k + "calls": np.array(p["calls"], np.int64),
        k + "act_call": np.array([a[0] for a in p["actions"]], np.int32),
        k + "act_cmd": np.array([LC.COMMANDS.index(a[1]) for a in p["actions"]], np.int32),
        k + "act_val": np.array([a[2] for a in p["actions"]], np.float64),
        k + "counters": np.array(counters, np.int32),
        k + "state": np.array(states, np.float64),
        k + "nbits": np.array(nbits, np.int64),
        k + "bits": np.array(d.bits, np.int8),
        k + "fec_rc": np.array([r[0] for r in d.fec_log], np.int32),
        k + "fec_bit": np.array([r[1] for r in d.fec_log], np.int32),
        k + "fec_data": np.array([r[2] for r in d.fec_log], np.uint8).reshape(-1, 256),
    }
    return out


def main():
    t0 = time.time()
    out = {}
    for name in SCENARIOS:
        o = run(name)
        out.update(o)
        k = "l_" + name + "_"
        print(f"{name:8s} counters={list(o[k + 'counters'][-1])} fec={list(o[k + 'fec_rc'])}  [{time.time() - t0:.0f} s]", flush=True)
    path = os.path.join(HERE, "live_control_fixtures.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
