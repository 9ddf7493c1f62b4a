"""GPU: the tune-mode front ends and matched filters at their tile, halo and call-length edges (tests/fm_cases.py has the cases and
the why; tests/test_fm_cases_oracle.py counts, from the definitions and on the oracle alone, what they contain).

Everything is compared bit for bit with oracle_lib.Bpsk, one oracle per stream or (input, channel): after EVERY call the call's
(fi, fq) trace, its bits, the counters, the state doubles (all 18 but avePeakPower and aveCentreBin) and the FEC results, at the end
the decoded block.  No tolerance anywhere.  Every call asserts its launch form from fm_cases.geometry: the front kernel's name,
last_launch() == (ntiles * S, ntiles * S), fm_form(), and from profile_read() which kernels ran (k_fm_prep + k_fm and no k_matched;
in the three-kernel children k_front + k_matched + k_dm_history and no k_fm; nothing at all for a call without output).

  seams              every (a, k, delta) of the cross at every (rate, tuning), ten schedules a test; int16 through k_fm and the
                     same samples as floats through k_fm_f32.  At 96 kHz / 12 kHz the 8-phase form: its tiles take both phase bodies
  seams, fast        the cross at 96 kHz / 12 kHz on variant="fast": bits, counters, FEC; a stream the variant leaves uncertified is
                     left out and named in the output
  alignment walks    66 and 513 outputs a call, every a = 0 .. 64 under either matched half
  form boundary      511, 512, 513 outputs at a = 0 and 64, exact and fast
  short calls        1 .. 257 samples as first call, after a long call, after short calls; DC correction off, ordinary and wrapping twice;
                     the float form without DC
  no output          runs of calls that yield nothing, then a long call
  CU share           3 streams x 3 tiles held to one workgroup a CU: what last_launch() says, the same results
  channel handles    1 x 1, 1 x 4, 1 x 5 and 2 x 5 (k_chan_front, groups of four channels): 255 .. 513 outputs, the short lengths,
                     k_matched's seams at 4160 - a + delta
  three-kernel path  two child processes run this file again with JSDR_FM=0, the second with JSDR_FRONT_REG=0 as well: the seam list is
                     then k_matched's (4160) and the front end's (64 R); the second child is not started behind a first that crashed

Checked by hand (scratch builds of three one-line edits, not committed; this file without its child tests, 130 tests, beside
test_gpu_bpsk.py -k "ragged or random_call or dc_correction", 20 tests, and test_gpu_fm_tuner_classes.py, 7 tests, on the same build):
  1. k_fm's halo save from t = 65 + threadIdx.x (a tile's first own output is never saved): 80 tests fail here -- every seam group at
     every (rate, tuning), the fast seams, the short calls at 44.1 kHz, the CU share; 3 of the 20 fail, none of the 7.
  2. k_fm's splice for nds < 63 in place of nds < 64: 72 fail here -- every seam group (the followers of 63 outputs), one fast group,
     the CU share; none of the 20, none of the 7.
  3. k_matched's staging with rel >= -63 (the oldest halo sample reads as zero): the 4 channel-handle tests fail here, and the two child
     tests are that kernel's other users; 6 of the 20 fail (random_call) and 1 of the 7 (tuning 12 010, which k_fm does not take)."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import fm_cases as F
import java_sdr_amd as J
import oracle_lib as O

pytestmark = pytest.mark.gpu

KNOBS = os.environ.get("JSDR_KNOBS") == "1"
FUSED = not (KNOBS and os.environ.get("JSDR_FM") == "0")             # k_fm / k_fm_f32 serve the calls
REG = not (KNOBS and os.environ.get("JSDR_FRONT_REG") == "0")        # k_front_reg where the three-kernel path applies it
CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK")
STATE = [i for i in range(18) if i not in (6, 7)]  # (avePeakPower, aveCentreBin: live in FFT-acquire only)
PHASES = {}  # (rate, tuning) -> the 8-phase bodies the seam tiles took


def launches(h):
    return {k: v[1] for k, v in h.profile_read().items()}


def expect_form(h, rate, tuning, form, n_in, L, nstreams, where):
    """the launch form of the call just made, from geometry"""
    got = launches(h)
    fused = FUSED and F.fm_takes(rate, tuning, n_in, L)
    g = F.geometry(rate, n_in, L, "fm" if fused else "split")
    if g["nds"] == 0:
        assert all(got[k] == 0 for k in ("k_fm", "k_front", "k_matched", "k_dm_history")), (where, got)
        return g
    if fused:
        assert h.front_kernel_name() == ("k_fm_f32" if form == "f32" else "k_fm"), (where, h.front_kernel_name())
        assert h.last_launch() == (g["ntiles"] * nstreams, g["ntiles"] * nstreams), (where, h.last_launch(), g)
        special = (rate, tuning) == (96000, 12000) and not g["small"] and form == "i16"
        sp, ph = h.fm_form()
        assert sp == special and (0 <= ph < 8 if special else ph == -1), (where, sp, ph, g)
        assert got["k_fm"] == 1 and got["k_fm_prep"] == 1 and got["k_matched"] == 0 and got["k_dm_history"] == 0 and got["k_front"] == 0, (where, got)
        if special:  # tile t starts 4030 D samples, half a period, behind tile t - 1: the bodies of ph and ph + 4 in turn
            PHASES.setdefault((rate, tuning), set()).update((ph + 4 * t) % 8 for t in range(g["ntiles"]))
    else:
        name = "k_front_reg" if REG and form != "f32" and L >= 64 else "k_front"  # (a fast handle off k_fm: the exact order)
        assert h.front_kernel_name() == name, (where, h.front_kernel_name(), name)
        assert got["k_fm"] == 0 and got["k_front"] == 1 and got["k_matched"] == 1 and got["k_dm_history"] == 1, (where, got, g)
    return g


class Follow:
    """one oracle per stream and what it has handed out so far: after a call, the call's share of the cumulative results"""

    def __init__(self, rate, tunings, total):
        self.o = [O.Bpsk(rate=rate, tuning=t, blen=1, size=1, trace=total // F.decim(rate) + 8) for t in tunings]
        self.nt, self.nb, self.nf = ([0] * len(tunings) for _ in range(3))

    def call(self, s, chunk, ic, qc):
        o = self.o[s]
        o.receive_i16(chunk, ic, qc)
        tr, bits, fec = o.trace(), o.bits(), o.fec_results()
        want = dict(trace=tr[self.nt[s]:].tobytes(), bits=bits[self.nb[s]:].tobytes(), counters=[o.counters()[k] for k in CKEYS],
                    state=o.state()[STATE].tobytes(), fec=[(rc, data.tobytes()) for rc, _, data in fec[self.nf[s]:]])
        self.nt[s], self.nb[s], self.nf[s] = len(tr), len(bits), len(fec)
        return want


def got_of(h, *idx):
    return dict(trace=h.trace(*idx).tobytes(), bits=h.bits(*idx).tobytes(), counters=[h.counters(*idx)[k] for k in CKEYS],
                state=h.state(*idx)[STATE].tobytes(), fec=[(rc, data.tobytes()) for rc, _, data in h.fec_results(*idx)])


def compare(got, want, keys, where):
    for k in keys:
        if got[k] != want[k]:
            if k == "trace":
                a, b = np.frombuffer(got[k]).reshape(-1, 2), np.frombuffer(want[k]).reshape(-1, 2)
                bad = np.flatnonzero((a != b).any(axis=1)) if a.shape == b.shape else []
                raise AssertionError((where, k, a.shape, b.shape, "outputs that differ:", len(bad), "first", list(bad[:8]), "last", list(bad[-3:])))
            raise AssertionError((where, k, got[k][:64], want[k][:64]))


ALL = ("trace", "bits", "counters", "state", "fec")
FAST_KEYS = ("bits", "counters", "fec")  # (the fast variant's (fi, fq) are not the oracle's)


def run_schedule(rate, tuning, sch, forms=("i16",), share=None):
    """one schedule on a handle per form, every call against the oracles; -> [(call, geometry)]"""
    raws = F.streams(rate, tuning, sch)
    total, maxL = raws.shape[1] // 2, max(c.L for c in sch.calls)
    ref = Follow(rate, [tuning] * F.S, total)
    hs, bufs, skipped = {}, {}, {}
    for form in forms:
        hs[form] = J.Bpsk(rate=rate, tuning=tuning, nstreams=F.S, max_batch_samples=maxL, variant="fast" if form == "fast" else "exact")
        hs[form].profile_enable(True)
        if share is not None:
            hs[form].set_cu_share(share)
        if form == "f32":
            bufs[form] = J.DeviceBuffer.from_host(np.stack([O.convert_i16(r, ic=sch.ic, qc=sch.qc) for r in raws]))
        else:
            bufs[form] = J.DeviceBuffer.from_host(raws)
        skipped[form] = {}
    out = []
    for k, (call, n_in, _) in enumerate(F.walk(sch)):
        want = [ref.call(s, raws[s, 2 * n_in:2 * (n_in + call.L)], sch.ic, sch.qc) for s in range(F.S)]
        for form, h in hs.items():
            where = (sch.name, rate, tuning, form, "call", k, call.role, call.L, "after", n_in)
            if form == "f32":
                h.batch_f32(bufs[form].ptr + 8 * n_in, 2 * total, call.L)
            else:
                h.batch_i16(bufs[form].ptr + 4 * n_in, 2 * total, call.L, sch.ic, sch.qc)
            g = expect_form(h, rate, tuning, form, n_in, call.L, F.S, where)
            if share is not None and "ntiles" in g and g["nds"]:
                items, grid = h.last_launch()
                assert 1 <= grid <= items, (where, items, grid)
            if form == "fast":
                for s in h.uncertified_streams():
                    skipped[form].setdefault(s, "left uncertified by call %d (%s, %d samples)" % (k, call.role, call.L))
            for s in range(F.S):
                if s in skipped[form]:
                    continue
                compare(got_of(h, s), want[s], FAST_KEYS if form == "fast" else ALL, where + ("stream", s))
        out.append((call, g))
    for form, h in hs.items():
        for s in range(F.S):
            if s not in skipped[form]:
                assert h.decoded(s).tobytes() == ref.o[s].decoded().tobytes(), (sch.name, form, s, "decoded")
        if skipped[form]:
            print("fast variant, %s at %d / %d: streams left out: %s" % (sch.name, rate, tuning, skipped[form]))
        assert len(skipped[form]) < F.S, (sch.name, form, skipped[form])
    return out


FORMS = ("i16", "f32")


# ---------------------------------------------------------------------------------------------------------------- seams
def seam_list(rate):
    return F.seam_cases(rate) if FUSED else F.split_seam_cases(rate)


def seam_groups():
    """(rate, tuning, first case, cases): ten schedules a test"""
    out = []
    for rate, tuning in F.CONFIGS:
        n = len(seam_list(rate))
        out += [(rate, tuning, i, min(10, n - i)) for i in range(0, n, 10)]
    return out


@pytest.mark.parametrize("rate,tuning,first,count", seam_groups())
def test_seams(rate, tuning, first, count):
    for key, sch in seam_list(rate)[first:first + count]:
        calls = run_schedule(rate, tuning, sch, FORMS)
        g = [g for c, g in calls if c.role == "seam"][0]
        if FUSED:
            a, k, d = key
            assert (g["a"], g["ntiles"], g["nds"]) == (a, k + (d >= 1), F.TILE * k - a + d)


def test_seams_took_both_bodies_of_the_eight_phase_form():
    """(behind test_seams) at 12 kHz / 96 kHz a launch of two tiles or more holds a tile at phase p and one at p + 4"""
    if not FUSED:
        return
    if (96000, 12000) not in PHASES:  # (selected alone)
        run_schedule(96000, 12000, dict(F.seam_cases(96000))[(63, 2, 3)])
    ph = PHASES[(96000, 12000)]
    assert ph and {p // 4 for p in ph} == {0, 1} and len({p % 4 for p in ph}) >= 2, ph


@pytest.mark.parametrize("first", range(0, 100, 20))
def test_seams_fast_variant(first):
    if not FUSED:
        return  # (a fast handle off k_fm runs in exact order: the children's exact tests are that path)
    for key, sch in F.seam_cases(96000)[first:first + 20]:
        run_schedule(96000, 12000, sch, ("fast",))


# ---------------------------------------------------------------------------------------------------------------- walks, boundary
@pytest.mark.parametrize("rate,tuning", F.CONFIGS)
def test_alignment_walks(rate, tuning):
    for sch in F.walk_schedules(rate):
        calls = run_schedule(rate, tuning, sch, FORMS)
        assert FUSED is False or {g["small"] for c, g in calls if c.role == "walk"} == {sch.name == "walk-66"}


@pytest.mark.parametrize("rate,tuning", F.CONFIGS)
def test_form_boundary(rate, tuning):
    run_schedule(rate, tuning, F.boundary_schedule(rate), FORMS + (("fast",) if FUSED and (rate, tuning) == (96000, 12000) else ()))


# ---------------------------------------------------------------------------------------------------------------- short calls
@pytest.mark.parametrize("dc", range(len(F.DCS)))
@pytest.mark.parametrize("rate,tuning", F.CONFIGS)
def test_short_calls(rate, tuning, dc):
    for sch in F.short_schedules(rate, F.DCS[dc]):
        run_schedule(rate, tuning, sch, FORMS if dc == 0 else ("i16",))


@pytest.mark.parametrize("rate,tuning", F.CONFIGS)
def test_calls_without_output(rate, tuning):
    calls = run_schedule(rate, tuning, F.zero_schedule(rate), FORMS)
    assert sum(g["nds"] == 0 for _, g in calls) >= 3


# ---------------------------------------------------------------------------------------------------------------- CU share
def test_cu_share_hands_out_the_same_tiles():
    """three streams x three tiles on a handle held to one workgroup a CU"""
    if not FUSED:
        return
    (key, sch), = [c for c in F.seam_cases(96000) if c[0] == (63, 2, 3)]
    calls = run_schedule(96000, 12000, sch, ("i16",), share=1)
    assert [g["ntiles"] for c, g in calls if c.role == "seam"] == [3]


# ---------------------------------------------------------------------------------------------------------------- channel handles
CHAN_TUNINGS = (12000.0, 24000.0, 0.0, -5000.0, 12010.0)
CHAN_NDS = (255, 256, 257, 511, 512, 513)


def chan_schedules(rate):
    """calls of 256 k +- 1 outputs, the short lengths behind them; k_matched's seams"""
    b = F._Builder(rate)
    for i, nds in enumerate(CHAN_NDS):
        b.out(nds, b.n % F.decim(rate) + 3, "chan", "%d outputs: k_chan_front's workgroups of 256" % nds)
        b.add(F.SHORT_LIST[i], "short", "a short call")
    for L in F.SHORT_LIST[len(CHAN_NDS):]:
        b.add(L, "short", "a short call")
        b.add(L, "short", "after a short call")
    b.out(131, 0, "flush", "takes what the short calls left")
    out = [b.done("chan-256", 0, F.DCS[1])]
    out += [sch for (kind, _, _), sch in F.split_seam_cases(rate) if kind == "matched"]
    return out


def run_channels(rate, nin, nch, sch):
    tunings = CHAN_TUNINGS[:nch]
    raws = F.streams(rate, 12000, sch)[:nin]
    total, maxL = raws.shape[1] // 2, max(c.L for c in sch.calls)
    h = J.BpskChannels(rate, 8192, tunings, ninputs=nin, max_batch_samples=maxL)
    h.profile_enable(True)
    ref = Follow(rate, [int(t) for t in tunings] * nin, total)
    d_raw = J.DeviceBuffer.from_host(raws)
    for k, (call, n_in, g) in enumerate(F.walk(sch, "chan")):
        h.batch_i16(d_raw.ptr + 4 * n_in, 2 * total, call.L, sch.ic, sch.qc)
        got = launches(h)
        where = (sch.name, rate, nin, nch, "call", k, call.role, call.L, "after", n_in)
        if g["nds"]:
            assert h.front_kernel_name() == "k_chan_front" and got["k_front"] == 1 and got["k_matched"] == 1 and got["k_fm"] == 0, (where, got)
        else:
            assert got["k_front"] == 0 and got["k_matched"] == 0 and got["k_fm"] == 0, (where, got)
        for i in range(nin):
            for c in range(nch):
                want = ref.call(i * nch + c, raws[i, 2 * n_in:2 * (n_in + call.L)], sch.ic, sch.qc)
                compare(got_of(h, i, c), want, ALL, where + ("input", i, "channel", c))
    for i in range(nin):
        for c in range(nch):
            assert h.decoded(i, c).tobytes() == ref.o[i * nch + c].decoded().tobytes()


@pytest.mark.parametrize("nin,nch", [(1, 1), (1, 4), (1, 5), (2, 5)])
def test_channel_handles(nin, nch):
    assert 12010.0 in CHAN_TUNINGS[:5] and len(CHAN_TUNINGS) == 5  # (five channels: a group of four and one; one has no period)
    for sch in chan_schedules(96000):
        run_channels(96000, nin, nch, sch)
    if (nin, nch) == (2, 5):
        for rate in (192000, 48000, 44100):
            run_channels(rate, nin, nch, chan_schedules(rate)[0])


# ---------------------------------------------------------------------------------------------------------------- three-kernel path
CHILD = {}  # name -> how it ended
CRASHED = (134, 139, 124, 137)
CHILD_K = "not channel and not child_process and not fast_variant and not cu_share and not both_bodies"


def child(name, env, limit):
    t = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__), "-k", CHILD_K],
                           env=dict(os.environ, JSDR_KNOBS="1", **env), capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        CHILD[name] = "crashed: no end within %d s" % limit
        raise AssertionError((name, CHILD[name], (e.stdout or b"")[-2000:]))
    crashed = r.returncode < 0 or r.returncode in CRASHED
    CHILD[name] = "crashed: status %d" % r.returncode if crashed else "status %d" % r.returncode
    m = re.search(r"(\d+) passed", r.stdout)
    print("child %s: %.1f s, %s" % (name, time.perf_counter() - t, r.stdout.strip().splitlines()[-1:]))
    assert r.returncode == 0 and m and int(m.group(1)) >= NCHILD and "skipped" not in r.stdout and "failed" not in r.stdout, \
        (name, CHILD[name], r.stdout[-3000:] + r.stderr[-2000:])


# what a child must at least pass: the seam groups of its list, walks, boundary, short calls x DC, no output
NCHILD = sum(-(-len(F.split_seam_cases(rate)) // 10) for rate, _ in F.CONFIGS) + len(F.CONFIGS) * (3 + len(F.DCS))


def test_once_more_in_a_child_process_with_k_fm_off():
    """JSDR_FM=0: k_front_reg (k_front below 64 samples and for floats) + k_matched + k_dm_history serve every call.  The time limit:
    a child takes 30 s on an MI355X, interpreter and library start included (the parent's own tests 55 s), and the whole file was seen to take three times as long on a loaded machine: eight times a child's 30 s."""
    assert FUSED and REG, "the child tests are deselected in the children"
    child("JSDR_FM=0", dict(JSDR_FM="0"), CHILD_LIMIT)


def test_once_more_in_a_child_process_with_k_fm_and_k_front_reg_off():
    """JSDR_FM=0 JSDR_FRONT_REG=0: k_front serves every call.  Not started behind a first child that crashed or hung."""
    assert FUSED and REG, "the child tests are deselected in the children"
    first = CHILD.get("JSDR_FM=0")
    assert first is None or not first.startswith("crashed"), "not started: the child JSDR_FM=0 " + first
    child("JSDR_FM=0 JSDR_FRONT_REG=0", dict(JSDR_FM="0", JSDR_FRONT_REG="0"), CHILD_LIMIT)


CHILD_LIMIT = 240
