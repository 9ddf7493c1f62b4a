#!/usr/bin/env python3
"""FUNcubeBPSKDemod.actionPerformed (:165-190) restated in pure Python over the restated demodulator
(java_restatement.Demod / DemodFFT), for tests/golden/live_control_fixtures.npz.

TEST INFRASTRUCTURE, generation time only (java_restatement parses its tables from the reference's source text).

A DemodFFT object holds the whole state of both front ends, so one object runs either chain on the same state:
`receive(obj, buf)` runs the tune chain (Demod.receive, doBufferTune :366-379) or the FFT-acquire chain
(DemodFFT.receive, doBufferFFT :399-464) as obj.doFFT says -- the choice :357-363 makes per call.
"""
import math

import java_restatement as J

# the action commands of :174-187, and their codes in the fixture
COMMANDS = ["bpsk-freq", "bpsk-plus10", "bpsk-sub10", "bpsk-fft-tune", "bpsk-high"]


def make_demod(samples, twiddles, rate, tuning, do_fft, do_up):
    d = J.DemodFFT(samples, twiddles, rate=rate, tuning=tuning, do_up=bool(do_up))
    d.doFFT = bool(do_fft)
    return d


def action_performed(d, command, freq=None):
    """:177-190.  `freq` is what freqDialog() returned for "bpsk-freq"."""
    if command == "bpsk-freq":
        d.tuning = float(freq)
    elif command == "bpsk-plus10":
        d.tuning += 10.0
    elif command == "bpsk-sub10":
        d.tuning -= 10.0
    elif command == "bpsk-fft-tune":
        d.doFFT = not d.doFFT
    elif command == "bpsk-high":
        d.doUp = not d.doUp
    else:
        raise ValueError(command)
    d.tuPhaseInc = 2.0 * math.pi * d.tuning / float(d.rate)
    d.dmMaxCorr = 0


def receive(d, buf):
    """:357-363: one receive() of the plugin; the FFT chain takes one frame of d.samples complex samples"""
    if d.doFFT:
        J.DemodFFT.receive(d, buf)
    else:
        J.Demod.receive(d, buf)
