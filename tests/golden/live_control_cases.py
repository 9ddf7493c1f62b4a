"""Scenarios of tests/golden/live_control_fixtures.npz: shared by the generator (make_live_control_fixtures.py, where the
reference's source text is) and by the tests that hold the C oracle and the HIP path to the fixture.  Inputs are synthetic
DBPSK from the repo's integer generator (oracle/o_synth.c == csrc/synth.hip); the fixture stores their sha256."""
import numpy as np

import oracle_lib as O  # input generator only (jo_synth_*)

# actions: (before call k, command, freqDialog value or 0.0)
SCENARIOS = {
    # +10 Hz x3 then -10 Hz inside the first FEC frame: the tuner stops being periodic (not k_fm)
    "retune": dict(rate=96000, frame=2048, tuning=12000, do_fft=0, do_up=0, carrier=13200.0, seed=20021001, noise=300.0,
                   calls=[16384] * 28,
                   actions=[(4, "bpsk-plus10", 0.0), (8, "bpsk-plus10", 0.0), (12, "bpsk-plus10", 0.0), (18, "bpsk-sub10", 0.0)]),
    # 0 Hz while tuPhase > 0 (tuPhase frozen), -100 Hz (crosses 0 downward, then passes samples through), back to 12 kHz
    # (crosses upward inside a call), a fractional negative tuning (down again inside a call) and back
    "zero": dict(rate=96000, frame=2048, tuning=12000, do_fft=0, do_up=0, carrier=13200.0, seed=20021002, noise=600.0,
                 calls=[2048] * 32,
                 actions=[(4, "bpsk-freq", 0.0), (8, "bpsk-freq", -100.0), (12, "bpsk-freq", 12000.0),
                          (20, "bpsk-freq", -250.5), (26, "bpsk-freq", 12000.0)]),
    # FFT-acquire, upper band: doUp off (the centre bin is clamped into the lower band), then on again, then an unchanged action
    "fft_high": dict(rate=96000, frame=2048, tuning=12000, do_fft=1, do_up=1, carrier=30000.0, seed=20021003, noise=600.0,
                     calls=[2048] * 24,
                     actions=[(8, "bpsk-high", 0.0), (16, "bpsk-high", 0.0), (20, "bpsk-freq", 12000.0)]),
    # the 1-stream drop-in at 48 kHz (decimation 5): one frame per receive(), actions between frames
    "rx48k": dict(rate=48000, frame=2048, tuning=12000, do_fft=0, do_up=0, carrier=13200.0, seed=20021004, noise=600.0,
                  calls=[2048] * 48,
                  actions=[(10, "bpsk-plus10", 0.0), (20, "bpsk-sub10", 0.0), (30, "bpsk-freq", 11990.5), (40, "bpsk-high", 0.0)]),
    # tune -> FFT -> tune -> FFT -> tune, doUp toggled in FFT-acquire mode and in the tune mode
    "switch": dict(rate=96000, frame=2048, tuning=12000, do_fft=0, do_up=0, carrier=13200.0, seed=20021006, noise=600.0,
                   calls=[2048] * 40,
                   actions=[(6, "bpsk-fft-tune", 0.0), (10, "bpsk-high", 0.0), (13, "bpsk-high", 0.0), (16, "bpsk-fft-tune", 0.0),
                            (20, "bpsk-high", 0.0), (24, "bpsk-fft-tune", 0.0), (30, "bpsk-fft-tune", 0.0), (31, "bpsk-plus10", 0.0)]),
    # actions that change nothing but dmMaxCorr
    "same": dict(rate=96000, frame=2048, tuning=12000, do_fft=0, do_up=0, carrier=13200.0, seed=20021005, noise=300.0,
                 calls=[32768] * 4,
                 actions=[(1, "bpsk-freq", 12000.0), (2, "bpsk-high", 0.0), (3, "bpsk-high", 0.0)]),
}
# the scenario the CPU test regenerates (the fixture pin)
PIN = "zero"


def scenario_input(name):
    p = SCENARIOS[name]
    n = sum(p["calls"])
    raw, _, _ = O.make_dbpsk_stream(p["seed"], 1, n, rate=p["rate"], carrier_hz=p["carrier"], amp=3000, noise_sigma=p["noise"])
    assert raw.size == 2 * n
    return raw
