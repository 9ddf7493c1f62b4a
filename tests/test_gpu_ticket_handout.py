"""GPU: the persistent forms of k_fft, k_fm and k_fm_f32 on more work than workgroups.  Held to a CU share (jsdr_fft_set_cu_share /
jsdr_bpsk_set_cu_share) k_fm and k_fm_f32 hand their tiles out by TICKET -- a workgroup takes its next tile from a counter when it
is through with the last -- and k_fft strides over its frame groups.  Either changes who does which item and when, never a
result: every case is compared byte for byte with the same calls made without a share (PSD, bits, (fi,fq) trace, counters, state
doubles, decoded blocks), the PSD buffer starts as a sentinel that no row may keep, and two streams / two frames of each case are
compared with the oracle as well.

tests/test_gpu_cu_share.py never gives a persistent workgroup a second item; the shapes here do (the launch sizes are asserted):
more items than workgroups and not a multiple of them, group counts that 4 and 16 do not divide, an odd frame count (the surplus
part-group), fewer items than workgroups, consecutive calls on one pair of handles (a counter that is not reset makes the second
call do nothing), two pairs of handles at once, share 0 after a shared call, and the float entry point.
No test reads a clock."""
import functools

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O

pytestmark = pytest.mark.gpu
N = 2048
RATE = 96000
SENTINEL = 0x7FC0DEAD  # a NaN payload the PSD kernel never writes (finite input: every bin is a number or -inf)
STATE = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)  # (6, 7: FFT-acquire only)
CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK", "centreBin")
FFT_RTOL = 1e-5  # BASELINE.json: FFT floats within 1e-5 of the frame's peak (tests/test_gpu_fft.py)
LMAX = N * 200


@functools.lru_cache(maxsize=None)
def carriers():
    """three DBPSK streams of LMAX samples (the generator takes about a second each: made once)"""
    return [O.make_dbpsk_stream(90 + k, k, LMAX, carrier_hz=13200.0 + 41.0 * k, noise_sigma=500.0 + 200 * k)[0][:2 * LMAX].astype(np.int32)
            for k in range(3)]


@functools.lru_cache(maxsize=None)
def batch(S, L, seed):
    """[S][2 L] int16: stream s is carrier s % 3 (repeated where L is longer) plus noise of its own -- no two streams alike"""
    rng = np.random.default_rng(seed)
    base = carriers()
    reps = -(-L // LMAX)
    out = np.empty((S, 2 * L), np.int16)
    for s in range(S):
        x = np.tile(base[s % 3], reps)[:2 * L] + rng.integers(-600, 600, 2 * L)
        out[s] = np.clip(x, -32768, 32767)
    out.setflags(write=False)
    return out


def frames_of(raw, nframes):
    """the first nframes 2048-sample frames of a batch, as the PSD kernel's input"""
    return np.ascontiguousarray(raw.reshape(-1, 2 * N)[:nframes])


def make_pair(S, max_batch):
    return J.Fft(N, RATE), J.Bpsk(nstreams=S, max_batch_samples=max_batch)


def launch(pair, streams, d_iq, stride, c, d_fft_in, nframes, d_psd, f32):
    fft, dem = pair
    if f32:
        dem.batch_f32(d_iq, stride, c, stream=streams[0].ptr)
    else:
        dem.batch_i16(d_iq, stride, c, stream=streams[0].ptr)
    fft.batch_i16(d_fft_in, nframes, d_psd, stream=streams[1].ptr)


def collect(pair, streams, S, d_psd, nframes):
    fft, dem = pair
    streams[1].sync()
    streams[0].sync()
    dem.sync()
    psd = d_psd.to_host(np.uint32)
    assert psd.size == nframes * (N + 2)
    rows = (psd.reshape(nframes, N + 2) == SENTINEL).any(axis=1)
    assert not rows.any(), f"PSD rows never written: {np.flatnonzero(rows)[:8]} of {nframes}"
    return psd, [dem.bits(s).copy() for s in range(S)], [dem.trace(s).copy() for s in range(S)]


def sentinel_psd(nframes):
    return J.DeviceBuffer.from_host(np.full(nframes * (N + 2), SENTINEL, np.uint32))


def run(raw, chunks, shares, fft_in, f32=False, pair=None, two_streams=True):
    """the calls of `chunks` on one pair of handles: the demodulator on raw [S][2 L] (its float conversion with f32), the PSD
    kernel on fft_in[k] ([nframes][2 N] int16) beside it.  shares: (fft, bpsk) per call, or one pair for all, or None."""
    S = raw.shape[0]
    pair = pair or make_pair(S, max(chunks))
    s1 = J.Stream()
    streams = (s1, J.Stream() if two_streams else s1)
    # (the demodulator is returned and read later, and its getters synchronise the stream of its last call: the streams live as
    #  long as the handle does, not only until this function returns)
    pair[1].call_streams = getattr(pair[1], "call_streams", []) + [streams]
    out, launches, pos = [], [], 0
    for k, c in enumerate(chunks):
        sh = shares[k] if shares and isinstance(shares[0], tuple) else shares
        pair[0].set_cu_share(sh[0] if sh else 0)
        pair[1].set_cu_share(sh[1] if sh else 0)
        part = np.ascontiguousarray(raw[:, 2 * pos:2 * (pos + c)])
        if f32:
            part = np.stack([O.convert_i16(r) for r in part])
        d_iq = J.DeviceBuffer.from_host(part)
        fin = fft_in[k]
        d_fin = J.DeviceBuffer.from_host(fin)
        d_psd = sentinel_psd(len(fin))
        launch(pair, streams, d_iq, 2 * c, c, d_fin, len(fin), d_psd, f32)
        out.append(collect(pair, streams, S, d_psd, len(fin)))
        launches.append((pair[0].last_launch(), pair[1].last_launch(), pair[1].front_kernel_name()))
        pos += c
    return pair[1], out, launches


def same_results(ref, got, S):
    (d0, o0, _), (d1, o1, _) = ref, got
    assert len(o0) == len(o1)
    for (p0, b0, t0), (p1, b1, t1) in zip(o0, o1):
        assert p0.tobytes() == p1.tobytes(), "PSD bytes differ"
        for s in range(S):
            assert np.array_equal(b0[s], b1[s]), f"stream {s}: bits differ"
            assert t0[s].tobytes() == t1[s].tobytes(), f"stream {s}: (fi,fq) differ"
    for s in range(S):
        assert d0.counters(s) == d1.counters(s), s
        assert d0.state(s).tobytes() == d1.state(s).tobytes(), s
        assert np.array_equal(d0.decoded(s), d1.decoded(s)), s


def lin(db):
    return 10.0 ** (np.asarray(db, np.float64) / 20.0)


def psd_against_oracle(psd_u32, fin, k):
    """frame k of a call's PSD against fft.receive (the rule of tests/test_gpu_fft.py::check_psd)"""
    got = psd_u32.view(np.float32).reshape(len(fin), N + 2)[k]
    ref = O.fft_receive(O.convert_i16(fin[k]), RATE)
    a, b = lin(got[:N]), lin(ref[:N])
    assert np.abs(a - b).max() <= FFT_RTOL * b.max()
    strong = ref[:N] > ref[:N].max() - 60.0
    assert np.abs(got[:N][strong] - ref[:N][strong]).max() < 1e-3
    if got[N] != ref[N]:
        kg, kr = int(np.argmax(got[:N])), int(np.argmax(ref[:N]))
        assert abs(ref[kg] - ref[kr]) < 1e-3, "argmax moved to a bin that is not a numerical tie"
    assert abs(got[N + 1] - ref[N + 1]) < 1e-3


def dem_against_oracle(got, raw, s, f32=False):
    """stream s of a run against the reference demodulator given the same samples in one piece: no tolerance"""
    d, outs, _ = got
    L = raw.shape[1] // 2
    if f32:
        o = O.Bpsk(rate=RATE, blen=4 * L, trace=L // 10 + 8)
        o.receive(O.convert_i16(raw[s]))
    else:
        o = O.Bpsk(rate=RATE, blen=4, trace=L // 10 + 8)
        o.receive_i16(raw[s])
    assert np.array_equal(np.concatenate([b[s] for _, b, _ in outs]), o.bits()), f"stream {s}: bits differ from the oracle's"
    assert np.array_equal(np.concatenate([t[s] for _, _, t in outs]), o.trace()), f"stream {s}: (fi,fq) differ from the oracle's"
    g, r = d.counters(s), o.counters()
    assert all(g[k] == r[k] for k in CKEYS), (g, r)
    gs, rs = d.state(s), o.state()
    assert all(gs[i] == rs[i] for i in STATE), (gs, rs)
    assert np.array_equal(d.decoded(s), o.decoded())


def against_oracle(got, raw, fft_in, f32=False):
    S = raw.shape[0]
    for s in sorted({0, S - 1}):
        dem_against_oracle(got, raw, s, f32)
    for (psd, _, _), fin in zip(got[1], fft_in):
        for k in sorted({0, len(fin) - 1}):
            psd_against_oracle(psd, fin, k)


def cus():
    """CUs of the device, from a launch: a share of one workgroup per CU on more groups than any part has CUs"""
    fft = J.Fft(N, RATE)
    fft.set_cu_share(1)
    fin = np.zeros((4096, 2 * N), np.int16)
    d_in, d_psd = J.DeviceBuffer.from_host(fin), J.DeviceBuffer(len(fin) * (N + 2) * 4)
    fft.batch_i16(d_in, len(fin), d_psd)
    J.binding.stream_sync(None)
    return fft.last_launch()[1]


@functools.lru_cache(maxsize=None)
def num_cu():
    return cus()


# ---- items above the grid, and not a multiple of it: 1032 frames = 516 groups for k_fft (8 streams x 129 frames), 11 tiles x 32
#      streams = 352 tiles for k_fm, on 256 workgroups each at shares (1, 1)
S1, L1, F1 = 32, N * 200, 8 * 129


@functools.lru_cache(maxsize=None)
def first_shape():
    raw = batch(S1, L1, 1)
    fft_in = [frames_of(raw, F1)]
    return raw, fft_in, run(raw, [L1], None, fft_in, two_streams=False)


@pytest.mark.parametrize("shares", [(1, 1), (2, 1), (4, 2)])
def test_more_items_than_workgroups(shares):
    raw, fft_in, ref = first_shape()
    got = run(raw, [L1], shares, fft_in)
    (fitems, fgrid), (ditems, dgrid), front = got[2][0]
    assert front == "k_fm"
    assert (fitems, ditems) == (516, 352)
    assert fgrid == min(fitems, shares[0] * num_cu()) and dgrid == min(ditems, shares[1] * num_cu())
    if shares == (1, 1) and num_cu() <= 256:
        assert fitems > fgrid and fitems % fgrid and ditems > dgrid and ditems % dgrid  # what the case is about
    same_results(ref, got, S1)
    against_oracle(got, raw, fft_in)


# ---- group counts that neither 4 nor 16 divides, many more of them than workgroups, and odd frame counts: the last group's
#      second frame is the surplus part-group
@pytest.mark.parametrize("nframes", [9613, 1029])  # 4807 and 515 groups
def test_ragged_runs_and_an_odd_frame_count(nframes):
    rng = np.random.default_rng(nframes)
    fft_in = [rng.integers(-20000, 20000, (nframes, 2 * N)).astype(np.int16)]
    raw = batch(3, N * 9, 2)
    ref = run(raw, [N * 9], None, fft_in, two_streams=False)
    got = run(raw, [N * 9], (1, 1), fft_in)
    (fitems, fgrid), _, _ = got[2][0]
    assert fitems == (nframes + 1) // 2 and fitems % 16 and fitems % 4 and nframes % 2
    assert fgrid == min(fitems, num_cu())
    same_results(ref, got, 3)
    against_oracle(got, raw, fft_in)


# ---- items below the grid: one frame (half a group), one tile
def test_fewer_items_than_workgroups():
    raw = batch(1, N, 3)
    fft_in = [frames_of(raw, 1)]
    ref = run(raw, [N], None, fft_in, two_streams=False)
    got = run(raw, [N], (1, 1), fft_in)
    assert got[2][0][:2] == ((1, 1), (1, 1))
    same_results(ref, got, 1)
    against_oracle(got, raw, fft_in)


# ---- consecutive calls on one pair of handles (96 streams x 60 frames a call: 384 tiles, 2880 groups -- every call hands out),
#      and share 0 after a shared call
S3, C3 = 96, [N * 60] * 3


@functools.lru_cache(maxsize=None)
def three_calls():
    raw = batch(S3, sum(C3), 4)
    fft_in = [frames_of(raw[:, 2 * N * 60 * k:2 * N * 60 * (k + 1)], S3 * 60) for k in range(3)]
    return raw, fft_in, run(raw, C3, None, fft_in, two_streams=False)


def test_three_consecutive_calls_on_one_pair():
    raw, fft_in, ref = three_calls()
    got = run(raw, C3, (1, 1), fft_in)
    for (fitems, fgrid), (ditems, dgrid), front in got[2]:
        assert front == "k_fm" and (fitems, ditems) == (2880, 384)
        assert fgrid == min(fitems, num_cu()) and dgrid == min(ditems, num_cu())
    same_results(ref, got, S3)
    against_oracle(got, raw, fft_in)


def test_share_zero_after_a_shared_call():
    raw, fft_in, ref = three_calls()
    got = run(raw, C3, [(1, 1), None, (2, 1)], fft_in)
    assert got[2][1][0][1] > got[2][0][0][1]  # the second call's launch is the form without a share: more workgroups
    assert got[2][1][1] == (384, 384)         # ... and a workgroup a tile
    same_results(ref, got, S3)
    against_oracle(got, raw, fft_in)


# ---- two pairs of handles at work at the same time, on four streams
def test_two_pairs_at_the_same_time():
    S, L = 48, N * 120  # 7 tiles x 48 = 336 tiles, 2880 groups
    raws = [batch(S, L, 5), batch(S, L, 6)]
    fins = [[frames_of(r, S * 120)] for r in raws]
    refs = [run(r, [L], None, f, two_streams=False) for r, f in zip(raws, fins)]
    pairs = [make_pair(S, L) for _ in raws]
    streams = [(J.Stream(), J.Stream()) for _ in raws]
    bufs = []
    for p, r, f in zip(pairs, raws, fins):
        p[0].set_cu_share(1)
        p[1].set_cu_share(1)
        bufs.append((J.DeviceBuffer.from_host(r), J.DeviceBuffer.from_host(f[0]), sentinel_psd(len(f[0]))))
    for p, st, (d_iq, d_fin, d_psd), f in zip(pairs, streams, bufs, fins):  # all four launches, then the first wait
        launch(p, st, d_iq, 2 * L, L, d_fin, len(f[0]), d_psd, False)
    for p, st, (_, _, d_psd), f, r, ref in zip(pairs, streams, bufs, fins, raws, refs):
        got = (p[1], [collect(p, st, S, d_psd, len(f[0]))], None)
        assert p[1].last_launch()[0] == 336 and p[0].last_launch()[0] == 2880
        same_results(ref, got, S)
        against_oracle(got, r, f)


# ---- the float entry point: jsdr_bpsk_batch_f32 with a share is k_fm_f32's ticket form
def test_float_entry_point():
    raw, fft_in, _ = first_shape()
    ref = run(raw, [L1], None, fft_in, f32=True, two_streams=False)
    got = run(raw, [L1], (1, 1), fft_in, f32=True)
    _, (ditems, dgrid), front = got[2][0]
    assert front == "k_fm_f32" and ditems == 352 and dgrid == min(ditems, num_cu())
    same_results(ref, got, S1)
    against_oracle(got, raw, fft_in, f32=True)
