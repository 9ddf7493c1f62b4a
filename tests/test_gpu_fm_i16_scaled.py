"""GPU: k_fm with the one-instruction int16 conversion and the exact fused multiply-adds, and matched_block outside k_fm.

k_fm converts with fm_convert_2p15 (common.h): its samples, tuner products and 27-tap sums are 2^15 times the reference's and
the factor leaves in the HOWARD constant; the first tap of every output and the taps that are powers of two are written as
fma (bpsk_fm.hip), and so is the first product of every matched-filter accumulator (bpsk_matched.h).  None of it may change a
bit: the handle is compared with the C oracle replaying the same calls (counters, the 18 state doubles, bits, FEC results and
every (fi, fq)) and with the float path (k_fm_f32) fed the reference rule's floats.

4 streams x 2 calls of 81 920 samples = 8192 outputs a call: three tiles of 62 x 65, so the batch kernel runs and not the
short-call one; the second call uses the edge images and the 64-sample halo.  Stream 0 is silence (the signed-zero case of the
first-tap fma), stream 1 silence but for one -1 and one +1, stream 2 walks every int16 value in I and a permutation of them in
Q, stream 3 is a DBPSK signal."""
import functools

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O

pytestmark = pytest.mark.gpu

S, L, CALLS = 4, 81920, 2
N = L * CALLS
CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK")
STATE = [i for i in range(18) if i not in (6, 7)]  # (avePeakPower, aveCentreBin: live in FFT-acquire only)
CONFIGS = [(12000, 0, 0), (12000, 11, -7), (0, 0, 0), (0, 11, -7)]  # tuning (MIX / no MIX), DC correction off / on


@functools.lru_cache(maxsize=None)
def streams():
    rng = np.random.default_rng(20240)
    raws = np.zeros((S, 2 * N), np.int16)
    raws[1, 2 * 1000] = -1
    raws[1, 2 * (L + 33) + 1] = 1
    raws[2, 0::2] = (np.arange(N, dtype=np.int64) % 65536 - 32768).astype(np.int16)
    raws[2, 1::2] = np.tile(rng.permutation(np.arange(-32768, 32768, dtype=np.int32)).astype(np.int16), N // 65536 + 1)[:N]
    raws[3] = O.make_dbpsk_stream(4242, 3, N, noise_sigma=600.0)[0]
    assert set(raws[2, 0::2].tolist()) == set(raws[2, 1::2].tolist()) == set(range(-32768, 32768))
    raws.setflags(write=False)
    return raws


def result(bits, fec, trace, counters, state, decoded):
    return dict(bits=np.concatenate(bits).tobytes(), fec=[(rc, data.tobytes()) for rc, _, data in fec],
                trace=np.concatenate(trace).tobytes(), counters=[counters[k] for k in CKEYS], state=state[STATE].tobytes(),
                decoded=decoded.tobytes())


@functools.lru_cache(maxsize=None)
def oracle(tuning, ic, qc, s):
    """the C oracle replaying the two calls of stream s"""
    o = O.Bpsk(tuning=tuning, trace=N // 10 + 8)
    for c in range(CALLS):
        o.receive_i16(streams()[s, 2 * L * c:2 * L * (c + 1)], ic, qc)
    return result([o.bits()], o.fec_results(), [o.trace()], o.counters(), o.state(), o.decoded())


def run(d, nstreams, call):
    """`call(c)` feeds call c to the handle -> per stream what the calls produced"""
    bits, fec, trace = ([[] for _ in range(nstreams)] for _ in range(3))
    names = []
    for c in range(CALLS):
        call(c)
        names.append(d.front_kernel_name())
        for s in range(nstreams):
            bits[s].append(d.bits(s).copy())
            fec[s].extend(d.fec_results(s))
            trace[s].append(d.trace(s).copy())
    return [result(bits[s], fec[s], trace[s], d.counters(s), d.state(s), d.decoded(s)) for s in range(nstreams)], names


def same(got, want, keys, where):
    for k in keys:
        assert got[k] == want[k], (where, k)


@pytest.mark.parametrize("tuning,ic,qc", CONFIGS)
def test_exact_variant_is_the_oracle_and_the_float_path(tuning, ic, qc):
    raws = streams()
    d_raw = J.DeviceBuffer.from_host(raws)
    d = J.Bpsk(tuning=tuning, nstreams=S, max_batch_samples=L)
    got, names = run(d, S, lambda c: d.batch_i16(d_raw.ptr + 4 * L * c, 2 * N, L, ic, qc))
    assert names == ["k_fm"] * CALLS
    assert d.last_launch()[0] == 3 * S  # three tiles a stream: the batch kernel
    for s in range(S):
        same(got[s], oracle(tuning, ic, qc, s), ("counters", "state", "bits", "fec", "decoded", "trace"), (tuning, ic, qc, s))
    assert len(got[3]["bits"]) > 2000 and len(got[0]["bits"]) == 0  # the signal is demodulated, silence is not
    # y of the float path on the reference rule's floats
    x = np.stack([O.convert_i16(raws[s], ic=ic, qc=qc) for s in range(S)])
    d_x = J.DeviceBuffer.from_host(x)
    f = J.Bpsk(tuning=tuning, nstreams=S, max_batch_samples=L)
    gotf, namesf = run(f, S, lambda c: f.batch_f32(d_x.ptr + 8 * L * c, 2 * N, L))
    assert namesf == ["k_fm_f32"] * CALLS
    for s in range(S):
        assert len(got[s]["trace"]) == 16 * (N // 10)
        same(got[s], gotf[s], ("trace", "state", "bits", "counters"), ("f32", tuning, ic, qc, s))


@pytest.mark.parametrize("tuning,ic,qc", CONFIGS)
def test_fast_variant_gives_the_oracles_bits_and_bytes(tuning, ic, qc):
    """A stream the fast variant cannot certify is LISTED after the call and its results are withheld until it has been
    replayed in exact order (the variant's contract, jsdr_hip.h) -- the near-silent streams can be such streams (a slicer decision
    between energies of 1e-9 is inside every margin), the signal stream must never be.  So: every call's bits and FEC results of
    the streams never listed are the fast kernel's own and are compared call by call; a listed stream is replayed, and then
    its counters, last call and decoded block are compared as well."""
    raws = streams()
    d_raw = J.DeviceBuffer.from_host(raws)
    d = J.Bpsk(tuning=tuning, nstreams=S, max_batch_samples=L, variant="fast")
    bits, fec, listed = [[] for _ in range(S)], [[] for _ in range(S)], set()
    for c in range(CALLS):
        d.batch_i16(d_raw.ptr + 4 * L * c, 2 * N, L, ic, qc)
        assert d.front_kernel_name() == "k_fm"
        listed |= set(d.uncertified_streams())
        for s in set(range(S)) - listed:
            bits[s].append(d.bits(s).copy())
            fec[s].extend(d.fec_results(s))
    assert 3 not in listed, listed
    if listed:
        d.recover_uncertified([d_raw.ptr + 4 * L * c for c in range(CALLS)], [L] * CALLS, 2 * N, ic, qc)
    for s in range(S):
        want = oracle(tuning, ic, qc, s)
        c = d.counters(s)
        assert [c[k] for k in CKEYS] == want["counters"], (tuning, ic, qc, s)
        assert d.decoded(s).tobytes() == want["decoded"], (tuning, ic, qc, s)
        fg = [(rc, data.tobytes()) for rc, _, data in (fec[s] if s not in listed else d.fec_results(s))]
        if s not in listed:
            assert np.concatenate(bits[s]).tobytes() == want["bits"] and fg == want["fec"], (tuning, ic, qc, s)
        else:  # (the last call's: the oracle's lists are cumulative)
            assert want["bits"].endswith(d.bits(s).tobytes()) and fg == want["fec"][len(want["fec"]) - len(fg):], (tuning, ic, qc, s)
    assert len(bits[3]) == CALLS and sum(len(b) for b in bits[3]) > 2000


def test_matched_block_outside_k_fm():
    """a tuner schedule that is not periodic (12 010 Hz) takes the three-kernel path: a front-end kernel, then k_matched --
    matched_block from the rows the front end wrote"""
    raws = streams()[2:4]
    d_raw = J.DeviceBuffer.from_host(raws)
    d = J.Bpsk(tuning=12010, nstreams=2, max_batch_samples=L)
    got, names = run(d, 2, lambda c: d.batch_i16(d_raw.ptr + 4 * L * c, 2 * N, L))
    assert names[0] == names[1] and names[0] in ("k_front", "k_front_reg"), names  # (either front end writes dm rows for k_matched)
    for s in range(2):
        o = O.Bpsk(tuning=12010, trace=N // 10 + 8)
        for c in range(CALLS):
            o.receive_i16(raws[s, 2 * L * c:2 * L * (c + 1)])
        want = result([o.bits()], o.fec_results(), [o.trace()], o.counters(), o.state(), o.decoded())
        same(got[s], want, ("counters", "state", "bits", "fec", "decoded", "trace"), s)
