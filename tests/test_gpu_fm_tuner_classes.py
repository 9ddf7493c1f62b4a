"""GPU: k_fm's form for the 8-phase tuner (bpsk_fm.hip, k_fm<PH>) against the C oracle, and its fallbacks.

At 12 kHz / 96 kHz five of the tuner's sixteen (phase, rail) factors are exactly 1.0, -1.0 or 0.0; the form drops their products,
fuses every tap of a +-1.0 sample into one fma and skips a 0.0 rail altogether.  None of it may change a bit.

4 streams x 8 calls of odd lengths 40 961, 40 963, ..: every call has two tiles of 62 x 65 outputs, the second one short, and the
call's table rotates against the sample number from call to call.  Stream 0 is silence (signed zeros through the fused taps and
past the skipped rail), stream 1 silence but for one -1 and one +1, stream 2 walks every int16 value in I and a permutation of them
in Q, stream 3 is a DBPSK signal.  Counters, the 16 state doubles, bits, FEC results, decoded bytes and every (fi, fq) must be
the oracle's, with DC correction off and on.

The phase jsdr_bpsk_fm_form reports is the tuner phase of the first window sample of the call's first tile.  Tiles start on
multiples of 65 outputs of the STREAM, 650 samples, so however long the calls are a stream that has run the tuner from its first
sample sees the even phases only; the odd ones belong to a stream whose tuner started an odd number of samples late
(test_odd_phases_after_a_late_start: created untuned, tuned to 12 kHz after 4097 samples), where the reference is the float
kernel k_fm_f32 -- the generic arithmetic, which has no such form -- fed the reference rule's floats."""
import functools

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O

pytestmark = pytest.mark.gpu

S, CALLS = 4, 8
LENS = [40961 + 2 * c for c in range(CALLS)]
OFFS = [sum(LENS[:c]) for c in range(CALLS + 1)]
N = OFFS[-1]
CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK")
STATE = [i for i in range(18) if i not in (6, 7)]  # (avePeakPower, aveCentreBin: live in FFT-acquire only)
ALL = ("counters", "state", "bits", "fec", "decoded", "trace")


@functools.lru_cache(maxsize=None)
def streams():
    rng = np.random.default_rng(20241)
    raws = np.zeros((S, 2 * N), np.int16)
    raws[1, 2 * 1000] = -1
    raws[1, 2 * (LENS[0] + 33) + 1] = 1
    raws[2, 0::2] = (np.arange(N, dtype=np.int64) % 65536 - 32768).astype(np.int16)
    raws[2, 1::2] = np.tile(rng.permutation(np.arange(-32768, 32768, dtype=np.int32)).astype(np.int16), N // 65536 + 1)[:N]
    raws[3] = O.make_dbpsk_stream(4243, 3, N, noise_sigma=600.0)[0]
    assert set(raws[2, 0::2].tolist()) == set(raws[2, 1::2].tolist()) == set(range(-32768, 32768))
    raws.setflags(write=False)
    return raws


def result(bits, fec, trace, counters, state, decoded):
    return dict(bits=np.concatenate(bits).tobytes(), fec=[(rc, data.tobytes()) for rc, _, data in fec],
                trace=np.concatenate(trace).tobytes(), counters=[counters[k] for k in CKEYS], state=state[STATE].tobytes(),
                decoded=decoded.tobytes())


@functools.lru_cache(maxsize=None)
def oracle(tuning, ic, qc, s, ncalls):
    """the C oracle replaying the first ncalls calls of stream s (frames of one sample: it takes whole frames, the calls are odd)"""
    o = O.Bpsk(tuning=tuning, blen=1, size=1, trace=N // 10 + 8)
    for c in range(ncalls):
        o.receive_i16(streams()[s, 2 * OFFS[c]:2 * OFFS[c + 1]], ic, qc)
    return result([o.bits()], o.fec_results(), [o.trace()], o.counters(), o.state(), o.decoded())


def run(d, ids, ncalls, call):
    """`call(c)` feeds call c to the handle -> per stream what the calls produced, the kernel names and the k_fm forms"""
    bits, fec, trace = ([[] for _ in ids] for _ in range(3))
    names, forms = [], []
    for c in range(ncalls):
        call(c)
        names.append(d.front_kernel_name())
        forms.append(d.fm_form())
        for i in range(len(ids)):
            bits[i].append(d.bits(i).copy())
            fec[i].extend(d.fec_results(i))
            trace[i].append(d.trace(i).copy())
    return [result(bits[i], fec[i], trace[i], d.counters(i), d.state(i), d.decoded(i)) for i in range(len(ids))], names, forms


def same(got, want, keys, where):
    for k in keys:
        assert got[k] == want[k], (where, k)


def batch(tuning, ids, ncalls, ic=0, qc=0, variant="exact"):
    raws = np.ascontiguousarray(streams()[list(ids)])
    d_raw = J.DeviceBuffer.from_host(raws)
    d = J.Bpsk(tuning=tuning, nstreams=len(ids), max_batch_samples=max(LENS), variant=variant)
    return run(d, ids, ncalls, lambda c: d.batch_i16(d_raw.ptr + 4 * OFFS[c], 2 * N, LENS[c], ic, qc))


@pytest.mark.parametrize("ic,qc", [(0, 0), (11, -7)])
def test_the_form_is_the_oracle(ic, qc):
    got, names, forms = batch(12000, range(S), CALLS, ic, qc)
    assert names == ["k_fm"] * CALLS
    assert all(sp for sp, _ in forms), forms
    # a stream tuned from its first sample: tile starts are multiples of 650 samples, the phases 0, 2, 4, 6 -- all of them
    assert {ph for _, ph in forms} == {0, 2, 4, 6}, forms
    for s in range(S):
        same(got[s], oracle(12000, ic, qc, s, CALLS), ALL, (ic, qc, s))
        assert len(got[s]["trace"]) == 16 * (N // 10)
    assert len(got[3]["bits"]) > 2000 and len(got[0]["bits"]) == 0  # the signal is demodulated, silence is not


def test_odd_phases_after_a_late_start():
    """untuned for 4097 samples, then 12 kHz: the tuner's 8-cycle starts an odd number of samples into the stream, so the tiles
    start on its odd phases; with the even ones of the test above, all eight.  int16 through the form == floats through k_fm_f32"""
    raws = streams()
    L0 = 4097
    lens = [L0] + LENS[:5]
    offs = [sum(lens[:c]) for c in range(len(lens) + 1)]
    x = np.stack([O.convert_i16(raws[s], ic=0, qc=0) for s in range(S)])
    d_raw, d_x = J.DeviceBuffer.from_host(raws), J.DeviceBuffer.from_host(x)
    d = J.Bpsk(tuning=0, nstreams=S, max_batch_samples=max(lens))
    f = J.Bpsk(tuning=0, nstreams=S, max_batch_samples=max(lens))

    def feed(h, c, fn):
        if c == 1:
            h.set_tuning(12000.0)
        fn(c)

    got, names, forms = run(d, range(S), len(lens), lambda c: feed(d, c, lambda c: d.batch_i16(d_raw.ptr + 4 * offs[c], 2 * N, lens[c])))
    gotf, namesf, formsf = run(f, range(S), len(lens), lambda c: feed(f, c, lambda c: f.batch_f32(d_x.ptr + 8 * offs[c], 2 * N, lens[c])))
    # (the call after the retune has unmixed history and takes the split front end; k_fm from the next one on)
    assert names[0] == "k_fm" and names[2:] == ["k_fm"] * 4 and namesf[2:] == ["k_fm_f32"] * 4, (names, namesf)
    assert forms[0] == (False, -1) and forms[1] == (False, -1) and all(sp for sp, _ in forms[2:]), forms
    assert {ph for _, ph in forms[2:]} == {1, 3, 5, 7}, forms
    assert all(fm == (False, -1) for fm in formsf), formsf
    for s in range(S):
        same(got[s], gotf[s], ("trace", "state", "bits", "counters", "fec", "decoded"), ("f32", s))
    assert len(got[3]["bits"]) > 1000


@pytest.mark.parametrize("tuning", [24000, 12010, 0])
def test_other_tunings_take_the_generic_kernels(tuning):
    """a period of 4, no period at all, no tuner: the oracle's results from the kernels these calls took before"""
    ids, ncalls = (2, 3), 3
    got, names, forms = batch(tuning, ids, ncalls)
    assert all(fm == (False, -1) for fm in forms), forms
    if tuning == 12010:  # (either front end writes dm rows for k_matched)
        assert names == [names[0]] * ncalls and names[0] in ("k_front", "k_front_reg"), names
    else:
        assert names == ["k_fm"] * ncalls, names
    for i, s in enumerate(ids):
        same(got[i], oracle(tuning, 0, 0, s, ncalls), ALL, (tuning, s))


def test_fast_variant_and_float_batches_take_the_generic_kernels():
    ids, ncalls = (3,), 3
    raws = np.ascontiguousarray(streams()[list(ids)])
    d_raw = J.DeviceBuffer.from_host(raws)
    d = J.Bpsk(tuning=12000, nstreams=1, max_batch_samples=max(LENS), variant="fast")
    bits, fec = [], []
    for c in range(ncalls):
        d.batch_i16(d_raw.ptr + 4 * OFFS[c], 2 * N, LENS[c])
        assert d.front_kernel_name() == "k_fm" and d.fm_form() == (False, -1)
        assert d.uncertified_streams() == []
        bits.append(d.bits(0).copy())
        fec.extend(d.fec_results(0))
    want = oracle(12000, 0, 0, 3, ncalls)
    assert np.concatenate(bits).tobytes() == want["bits"] and [(rc, data.tobytes()) for rc, _, data in fec] == want["fec"]
    assert [d.counters(0)[k] for k in CKEYS] == want["counters"] and d.decoded(0).tobytes() == want["decoded"]
    # float batches of the reference rule's floats
    x = np.stack([O.convert_i16(raws[0])])
    d_x = J.DeviceBuffer.from_host(x)
    f = J.Bpsk(tuning=12000, nstreams=1, max_batch_samples=max(LENS))
    gotf, namesf, formsf = run(f, ids, ncalls, lambda c: f.batch_f32(d_x.ptr + 8 * OFFS[c], 2 * N, LENS[c]))
    assert namesf == ["k_fm_f32"] * ncalls and all(fm == (False, -1) for fm in formsf), (namesf, formsf)
    same(gotf[0], want, ALL, "f32")
