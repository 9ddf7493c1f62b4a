"""GPU: the demod.java AM/FM chain at its tile, halo and mean-block edges (tests/demod_cases.py has the cases and the why;
tests/test_demod_cases_oracle.py counts, on the oracle alone, what they contain).

Everything is compared bit for bit with oracle_lib.Demod, one oracle per stream or (input, channel), frame by frame: the int16
audio after every call, frame_stats after every call (NaN equal to NaN), and state() / channel_state() after every call.  No
tolerance anywhere.  Every audio buffer is allocated with guard bytes behind its last row, which a call must leave unchanged, and
every case asserts from the handle's launch counts (profile_read) which kernels served it, against demod_cases.geometry:
k_demod_out zero (fused) or one per call, k_demod_mean exactly for AM, k_demod_chan against k_demod_front by handle kind.

  grid, ordinary handle   every frame size x modes 0 .. 4 x switch sets, int16 with DC correction and the float form fed
                          convert_i16 of the same frames, three streams, calls of demod_cases.calls_of(n)
  grid, channel handle    the same sizes and schedules on 2 inputs x 5 channels (one per mode); at 8192 also 16 channels, three AM
  receive_f32             n = 1, 7, 22, 2049 on a one-stream handle and a one-input channel handle, against batch_f32 and the oracle
  planted maxima          AGC on: RAW and AM with filter and mixer off (the census makes the frame maximum the planted sample),
                          NFM and AM with both on, on both handle kinds
  filter run-out          RAW, AM, NFM with the filter on over a tone it removes: the padded lanes of a ragged tile hold partial
                          sums many times the frame's maximum
  mean blocks             AM at 63, 64, 65, 129, 200 frames a launch and at frame sizes of vector + ragged and scalar chunks; channel
                          handles whose AM rows number 65 and 129
  switch schedule         filter off / on over a stale ring, mixer off / on, FM -> RAW -> AM -> FM, AGC, weights() in between
  three-kernel path       a child process runs this file again with JSDR_DEMOD_FUSED=0: the launch assertions then demand
                          k_demod_out for every mode on ordinary handles; channel handles ignore the knob, and say so

Checked by hand (scratch builds, not committed).  Dropping the `t0 + u < len` guard on demod_tile's maximum fails 50 tests here
(grid, receive, planted, run-out, mean blocks, switches) -- and one test from before this file, which saw it in NFM at 9600.  Two edits of
that guard that the earlier demod tests do not see: `t0 + u <= len` (one padded lane too many) fails 42 tests here, `t0 + u < len - 1`
(a tile's last sample left out) fails 38, the planted maxima at every size among them.  k_demod_state zeroing the inherited part
of a history (`g >= 0` for `g >= -DHALO`) fails the ordinary grid at every frame size below 21, receive_f32 at 1 and 7 and the
run-out case at 9; the earlier demod tests pass."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import demod_cases as D
import java_sdr_amd as J
import layouts as LY
import oracle_lib as O
from test_gpu_demod import same
from test_gpu_demod_channels import ALLPASS, FIVE, Bank
from test_gpu_layouts import Guarded

pytestmark = pytest.mark.gpu

FUSED_OK = os.environ.get("JSDR_DEMOD_FUSED") != "0"
TAIL = 2 * 9  # guard elements (int16) behind the last audio row
# what the child process must at least pass (every test of this file but the child test itself)
NTESTS = 2 * len(D.SIZE_LIST) + 1 + 2 * 4 + 2 * len(D.PLANTED_SIZES) + len(D.RUNOUT_SIZES) + len(D.MEAN_BLOCKS) + len(D.MEAN_CHANNEL_BLOCKS) + 1


def guarded(rows, L, what):
    return Guarded(LY.Layout(rows, 2 * L, 2 * L, lead=0, tail=TAIL, itemsize=2, unit=2), what)


def launches(h):
    return {k: v[1] for k, v in h.profile_read().items()}


def ordinary_form(h, mode, dodwn_calls, ncalls, what):
    """the kernels of `ncalls` calls of an ordinary handle in one mode, `dodwn_calls` of them with the mixer on"""
    got = launches(h)
    g = D.geometry(h.n, mode, FUSED_OK)
    want = dict(k_demod_nco=dodwn_calls, k_demod_front=ncalls, k_demod_state=ncalls, k_demod_mean=ncalls if mode == D.AM else 0,
                k_demod_out=0 if g["fused"] else ncalls, k_demod_chan=0)
    assert got == want, (what, g, got, want)


def channel_form(h, ncalls, am, what):
    """a channel handle of frames up to five tiles: k_demod_chan + k_demod_chan_state a call, k_demod_chan_out where a channel is
    AM, never k_demod_front / k_demod_out -- whatever JSDR_DEMOD_FUSED says"""
    got = launches(h)
    assert D.geometry(h.n, D.NFM)["tiles"] <= D.FUSED_TILES
    assert got["k_demod_front"] == 0 and got["k_demod_out"] == 0 and got["k_demod_state"] == 0, (what, got)
    assert got["k_demod_chan"] == (3 if am else 2) * ncalls and got["k_demod_mean"] == (ncalls if am else 0), (what, got)


class Ordinary:
    """an int16-fed and a float-fed ordinary handle and one oracle per stream, given the same controls and calls"""

    def __init__(self, n, streams, max_frames, forms=("i16", "f32")):
        self.n, self.S = n, streams
        self.h = {k: J.Demod(D.RATE, n, streams, max_frames * n) for k in forms}
        self.o = [O.Demod(D.RATE) for _ in range(streams)]
        for h in self.h.values():
            h.profile_enable(True)

    def configure(self, mode, fir, dwn, agc):
        for x in list(self.h.values()) + self.o:
            x.configure(mode, fir, dwn, agc)

    def weights(self, flo, fhi):
        for o in self.o:
            ow, ophi = o.weights(flo, fhi)
        for h in self.h.values():
            w, phi = h.weights(flo, fhi)
            assert np.array_equal(w, ow) and phi == ophi

    def call(self, chunk, nf, ic, qc, what):
        """chunk: int16 [S][2L]"""
        n, L = self.n, nf * self.n
        bufs = [O.convert_i16(chunk[s], ic=ic, qc=qc) for s in range(self.S)]
        want = [np.concatenate([o.receive(b[2 * f * n:2 * (f + 1) * n]) for f in range(nf)]) for o, b in zip(self.o, bufs)]
        for form, h in self.h.items():
            out = guarded(self.S, L, ("ordinary audio", form, what))
            if form == "i16":
                d_in = J.DeviceBuffer.from_host(np.ascontiguousarray(chunk))
                h.batch_i16(d_in, 2 * L, L, out.ptr, 2 * L, ic, qc)
            else:
                d_in = J.DeviceBuffer.from_host(np.stack(bufs))
                h.batch_f32(d_in, 2 * L, L, out.ptr, 2 * L)
            got = out.rows(np.int16)
            for s in range(self.S):
                if not np.array_equal(got[s], want[s]):
                    bad = np.flatnonzero(got[s] != want[s])
                    raise AssertionError((what, form, "stream", s, "first sample", int(bad[0]) // 2, "frame", int(bad[0]) // (2 * n),
                                          bad.size // 2, "samples differ", got[s][bad[:6]], want[s][bad[:6]]))
                mx, av = h.frame_stats(s)
                assert same(mx, self.o[s].max) and same(av, self.o[s].avg), (what, form, s, mx, av, self.o[s].max, self.o[s].avg)
            # (checked with the mixer off as well: car must neither advance nor reset)
            assert h.state() == (self.o[0].car, np.float32(self.o[0].d.phi)), (what, form, h.state(), self.o[0].car)


def run_ordinary(n, raws, frames, configs, ic=0, qc=0, band=D.BAND, what=""):
    """every config (mode, dofir, dodwn, doagc) on handles and oracles of its own, over the whole schedule"""
    streams = raws.shape[0]
    for cfg in configs:
        x = Ordinary(n, streams, max(frames))
        x.configure(*cfg)
        x.weights(*band)
        pos = 0
        for k, nf in enumerate(frames):
            x.call(raws[:, 2 * pos:2 * (pos + nf * n)], nf, ic, qc, (what, n, cfg, "call", k))
            pos += nf * n
        for form, h in x.h.items():
            ordinary_form(h, cfg[0], len(frames) * cfg[2], len(frames), (what, n, cfg, form))


def run_channels(n, raws, frames, chans, ic=0, qc=0, what=""):
    """raws: int16 [inputs][2 * total]; chans: (mode, dofir, dodwn, doagc, band) per channel"""
    nin = raws.shape[0]
    bank = Bank(D.RATE, n, nin, chans, max(frames))
    bank.h.profile_enable(True)
    pos = 0
    for k, nf in enumerate(frames):
        L = nf * n
        chunk = np.ascontiguousarray(raws[:, 2 * pos:2 * (pos + L)])
        out = guarded(nin * bank.K, L, ("channel audio", what, n, k))
        d_in = J.DeviceBuffer.from_host(chunk)
        bank.h.batch_i16(d_in, 2 * L, L, out.ptr, 2 * L, ic, qc)
        got = out.rows(np.int16).reshape(nin, bank.K, 2 * L)
        bank.check(got, [O.convert_i16(x, ic=ic, qc=qc) for x in chunk], nf, (what, n, "call", k))
        pos += L
    channel_form(bank.h, len(frames), any(c[0] == D.AM for c in chans), (what, n))


# ---------------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("n", D.SIZE_LIST)
def test_grid_ordinary_handle(n):
    configs = [(mode,) + sw for mode in D.MODES for sw in D.switches_of(n)]
    run_ordinary(n, D.grid_signal(n), D.calls_of(n), configs, ic=D.IC, qc=D.QC, what="grid")


# DCHAN_MAX channels: the modes in turn (AM at 1, 6, 11), switches and bands of their own, two all-pass
SIXTEEN = [((D.NFM, D.AM, D.RAW, D.WFM, D.OFF)[c % 5], int(c % 3 != 1), int(c % 4 != 2), int(c % 5 != 3),
            ALLPASS if c % 7 == 6 else (1000 * (c - 8), 1000 * (c - 8) + 4000 + 500 * c)) for c in range(16)]


@pytest.mark.parametrize("n", D.SIZE_LIST)
def test_grid_channel_handle(n):
    raws = D.grid_signal(n, 2, 2100.0)
    run_channels(n, raws, D.calls_of(n), FIVE, ic=D.IC, qc=D.QC, what="grid")
    if n == 8192:  # DCHAN_MAX channels, three of them AM, on k_demod_chan<*, 4>
        assert len(SIXTEEN) == 16 and sum(c[0] == D.AM for c in SIXTEEN) == 3 and {c[0] for c in SIXTEEN} == set(D.MODES)
        run_channels(n, raws, D.calls_of(n), SIXTEEN, ic=D.IC, qc=D.QC, what="sixteen")


def test_grid_channel_handle_float_input():
    """batch_f32 of a channel handle at the tile edges, fed convert_i16 of the int16 frames: the same audio"""
    for n in (7, 2049, 6145):
        raws = D.grid_signal(n, 2, 2100.0)
        frames = D.calls_of(n)
        bank = Bank(D.RATE, n, 2, FIVE, max(frames))
        bank.h.profile_enable(True)
        pos = 0
        for k, nf in enumerate(frames):
            L = nf * n
            bufs = [O.convert_i16(r[2 * pos:2 * (pos + L)], ic=D.IC, qc=D.QC) for r in raws]
            out = guarded(2 * bank.K, L, ("channel audio, float input", n, k))
            d_in = J.DeviceBuffer.from_host(np.stack(bufs))
            bank.h.batch_f32(d_in, 2 * L, L, out.ptr, 2 * L)
            bank.check(out.rows(np.int16).reshape(2, bank.K, 2 * L), bufs, nf, ("f32", n, k))
            pos += L
        channel_form(bank.h, len(frames), True, ("f32", n))


# ---------------------------------------------------------------------------------------------------------------- receive_f32
RECEIVE = [(D.NFM, 1, 1, 1, D.BAND), (D.AM, 1, 1, 1, (-12000, -3000)), (D.RAW, 0, 1, 0, ALLPASS), (D.WFM, 1, 0, 1, D.BAND)]


@pytest.mark.parametrize("n", [1, 7, 22, 2049])
def test_receive_f32_ordinary_handle(n):
    raw = D.grid_signal(n, 1)[0]
    for mode, fir, dwn, agc, band in RECEIVE:
        rx, bt, o = J.Demod(D.RATE, n, 1), J.Demod(D.RATE, n, 1, n), O.Demod(D.RATE)
        for x in (rx, bt, o):
            x.configure(mode, fir, dwn, agc)
            x.weights(*band)
            if x is not o:
                x.profile_enable(True)
        for k in range(4):
            buf = O.convert_i16(raw[2 * k * n:2 * (k + 1) * n])
            got = rx.receive(buf)
            out = guarded(1, n, ("receive twin", n, k))
            d_in = J.DeviceBuffer.from_host(buf)
            bt.batch_f32(d_in, 2 * n, n, out.ptr, 2 * n)
            want = o.receive(buf)
            assert np.array_equal(got, want) and np.array_equal(out.rows(np.int16)[0], want), (n, mode, k)
            for h in (rx, bt):
                mx, av = h.frame_stats(0)
                assert same(mx, o.max) and same(av, o.avg) and h.state() == (o.car, np.float32(o.d.phi)), (n, mode, k)
        for h in (rx, bt):
            ordinary_form(h, mode, 4 * dwn, 4, ("receive", n, mode))


@pytest.mark.parametrize("n", [1, 7, 22, 2049])
def test_receive_f32_channel_handle(n):
    raw = D.grid_signal(n, 1)[0]
    rx = Bank(D.RATE, n, 1, RECEIVE, 1)
    bt = J.DemodChannels(D.RATE, n, 1, len(RECEIVE), n)
    for c, (mode, fir, dwn, agc, band) in enumerate(RECEIVE):
        bt.configure_channel(c, mode, fir, dwn, agc)
        bt.channel_weights(c, *band)
    for h in (rx.h, bt):
        h.profile_enable(True)
    for k in range(4):
        buf = O.convert_i16(raw[2 * k * n:2 * (k + 1) * n])
        got = rx.h.receive(buf)
        out = guarded(len(RECEIVE), n, ("channel receive twin", n, k))
        d_in = J.DeviceBuffer.from_host(buf)
        bt.batch_f32(d_in, 2 * n, n, out.ptr, 2 * n)
        assert np.array_equal(got, out.rows(np.int16)), (n, k)
        rx.check(got[None], [buf], 1, ("receive", n, k))
        assert [bt.channel_state(c) for c in range(rx.K)] == [rx.h.channel_state(c) for c in range(rx.K)]
    for h in (rx.h, bt):
        channel_form(h, 4, True, ("receive", n))


# ---------------------------------------------------------------------------------------------------------------- the frame maximum
PLANTED_CONFIGS = [(D.RAW, 0, 0, 1), (D.AM, 0, 0, 1), (D.NFM, 1, 1, 1), (D.AM, 1, 1, 1)]


@pytest.mark.parametrize("n", D.PLANTED_SIZES)
def test_planted_maxima_ordinary_handle(n):
    raws, plan = D.planted(n)
    run_ordinary(n, raws, D.PLANTED_CALLS, PLANTED_CONFIGS, what="planted")


@pytest.mark.parametrize("n", D.PLANTED_SIZES)
def test_planted_maxima_channel_handle(n):
    """the planted streams as the inputs: behind a call's last, quiet frame lies the next input's loud first one"""
    raws, plan = D.planted(n)
    run_channels(n, raws, D.PLANTED_CALLS, [c + (D.BAND,) for c in PLANTED_CONFIGS], what="planted")


@pytest.mark.parametrize("n", D.RUNOUT_SIZES)
def test_filter_run_out_past_a_ragged_tile_stays_out_of_the_maximum(n):
    configs = [(D.RAW, 1, 0, 1), (D.AM, 1, 0, 1), (D.NFM, 1, 1, 1)]
    run_ordinary(n, D.runout(n), D.calls_of(n), configs, what="run-out")
    run_channels(n, D.runout(n), D.calls_of(n), [c + (D.BAND,) for c in configs], what="run-out")


# ---------------------------------------------------------------------------------------------------------------- k_demod_mean
@pytest.mark.parametrize("n,streams,nf", D.MEAN_BLOCKS)
def test_mean_blocks_ordinary_handle(n, streams, nf):
    run_ordinary(n, D.mean_signal(n, streams, nf), (nf, nf), [(D.AM, 1, 1, 1)], what=("mean", D.mean_blocks(streams * nf)))


@pytest.mark.parametrize("n,nin,nf", D.MEAN_CHANNEL_BLOCKS)
def test_mean_blocks_channel_handle(n, nin, nf):
    """one AM channel of five: its rows (inputs x frames) come first in the float buffer, 65 and 129 of them"""
    chans = [FIVE[0], FIVE[1], FIVE[3], FIVE[2], FIVE[4]]  # (the AM channel is not the first)
    assert sum(c[0] == D.AM for c in chans) == 1 and D.mean_blocks(nin * nf)[0] >= 1 and D.mean_blocks(nin * nf)[1] == 1
    run_channels(n, D.mean_signal(n, nin, nf), (nf, nf), chans, what="mean")


# ---------------------------------------------------------------------------------------------------------------- live switches
def test_switches_on_a_live_ordinary_handle():
    n, raws = D.SWITCH_N, D.switch_signal()
    x = Ordinary(n, D.S, max(D.SWITCH_FRAMES))
    x.weights(*D.BAND)
    pos = 0
    for k, (nf, (cfg, reweight)) in enumerate(zip(D.SWITCH_FRAMES, D.SWITCH_CALLS)):
        if reweight:
            x.weights(*D.SWITCH_BAND2)
        x.configure(*cfg)
        x.call(raws[:, 2 * pos:2 * (pos + nf * n)], nf, 0, 0, ("switches", "call", k + 1, cfg))
        for form, h in x.h.items():  # (the launch counts are read, and so reset, after every call)
            ordinary_form(h, cfg[0], cfg[2], 1, ("switches", k + 1, form))
        pos += nf * n
    assert pos * 2 == raws.shape[1]


# ---------------------------------------------------------------------------------------------------------------- k_demod_front + k_demod_out
def test_once_more_through_the_three_kernel_path_in_a_child_process():
    """JSDR_DEMOD_FUSED=0: every mode of every ordinary handle above through k_demod_front + k_demod_out, at one to five tiles
    (ordinary_form demands it).  The time limit: these tests take 14 s in the parent and 17 s as a child, interpreter and library
    start included, on an MI355X; three times that and a little."""
    assert FUSED_OK, "the child test is deselected in the child"
    t = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__), "-k", "not child_process"],
                       env=dict(os.environ, JSDR_KNOBS="1", JSDR_DEMOD_FUSED="0"), capture_output=True, text=True, timeout=60)
    m = re.search(r"(\d+) passed", r.stdout)
    print("child: %.1f s, %s" % (time.perf_counter() - t, r.stdout.strip().splitlines()[-1:]))
    assert r.returncode == 0 and m and int(m.group(1)) >= NTESTS and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
