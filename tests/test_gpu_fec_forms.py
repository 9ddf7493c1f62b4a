"""GPU: every form of the FEC decoder (csrc/fec.hip) on the constructed blocks of tests/fec_cases.py, against the oracle.

  form A  jsdr_fec_decode / jsdr_fec_decode_batch -> k_fec_decode: lane = state Viterbi, decision words in LDS, any soft byte
  form B  the demodulator's hook below 256 streams -> k_fec_bpsk (and its fused form for 1-stream receive() calls)
  form C  the hook's batch form from 256 streams (or JSDR_VITQ=1) -> k_fec_bits + k_vitq (four lanes per block) + k_fec_rs
  form D  the remainder inside k_vitq's launch (lane = state decoder on the blocks beyond a whole number of quad rounds)

Form A takes families 1-7 directly.  Forms B-D see hard bits only, so the hard families travel as the symbols of synthetic DBPSK
streams without noise: the slicer returns the constructed symbols, the sync correlation fires at the end of every frame, and the
hook decodes the last 5200 bits.  What the hook saw is cut out of the stream's own bit history at the logged bit index and put
through O.fec_decode -- for EVERY stream and hit; the rule is validated on sampled streams against O.Bpsk, which also covers
bits, counters, decoded[] and the log.  All checks are equalities.

Checked by hand against one-line changes of fec.hip (scratch builds): the Chien search losing the root of column 254, Berlekamp-
Massey's `2 el <= r - 1` as `<`, k_vitq's tie broken the other way (form C alone notices), the parallel chain-back accepted
unmerged after a warm-up of 8, and the remainder reading work_list[ridx] (form D alone notices) each fail tests here.  One change
is invisible by construction: skipping Forney's store when the column lies in the padding.  Miscorrections (b) and (c) do put
roots there -- the kernel must count them and patch the other columns -- but nothing reads a padding byte after the correction:
the payload, the re-encoding and the error count take columns 95 .. 222 only.
"""
import numpy as np
import pytest

import big_offsets as B
import fec_cases as F
import java_sdr_amd as J
import oracle_lib as O
from test_gpu_headline_mode import check_stream_against_oracle

pytestmark = pytest.mark.gpu
SPS, PAD, SLACK = 80, 400, 50  # samples per symbol; filler symbols that lead every stream in; symbols a call runs past a frame's end
FRAME = F.SYMPBLOCK * SPS
PATTERN = (np.arange(256) * 7 + 3).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ form A
def check_form_a(rows, rc, out, what):
    nfail = 0
    for i, (fam, name, _, soft) in enumerate(rows):
        buf = PATTERN.copy()
        orc = O.lib().jo_fec_decode(O.ptr(np.ascontiguousarray(soft)), O.ptr(buf))
        assert rc[i] == orc, (what, fam, name, int(rc[i]), orc)
        assert np.array_equal(out[i], buf), (what, fam, name, orc)  # on rc = -1 the caller's bytes stay (FECDecoder.java:780)
        nfail += orc < 0
    return nfail


def decode_batch_prefilled(softs):
    nb = len(softs)
    d_raw = J.DeviceBuffer.from_host(np.stack(softs))
    d_out = J.DeviceBuffer.from_host(np.tile(PATTERN, nb))
    d_rc = J.DeviceBuffer.from_host(np.full(nb, -77, np.int32))
    try:
        J.fec_decode_dev(d_raw, nb, d_out, d_rc)
        J.binding.stream_sync()
        return d_rc.to_host(np.int32), d_out.to_host(np.uint8).reshape(nb, 256)
    finally:
        for b in (d_raw, d_out, d_rc):
            b.free()


def test_form_a_every_block_of_every_family_in_one_batch_and_reversed():
    rows = F.all_rows()
    assert len(rows) >= 2300
    rc, out = decode_batch_prefilled([r[3] for r in rows])
    nfail = check_form_a(rows, rc, out, "forward")
    assert 300 <= nfail <= len(rows) - 1500  # (both outcomes are well represented)
    rev = rows[::-1]
    rc, out = decode_batch_prefilled([r[3] for r in rev])  # no state from block to block: another neighbour, another workgroup
    check_form_a(rev, rc, out, "reversed")
    print(f"form A: {2 * len(rows)} blocks ({len(rows)} forward + reversed), {nfail} of {len(rows)} fail on the oracle")


def test_form_a_single_block_call_one_block_of_each_family():
    n = 0
    for fam in F.FAMILIES:
        rows = F.family(fam)
        res = [O.fec_decode(r[2])[0] for r in rows]
        picks = [next((i for i, v in enumerate(res) if v > 0), None), next((i for i, v in enumerate(res) if v < 0), None)]
        for i in (p for p in picks if p is not None):
            name, _, soft = rows[i]
            rc, out = J.fec_decode(soft, out_init=PATTERN)
            buf = PATTERN.copy()
            orc = O.lib().jo_fec_decode(O.ptr(np.ascontiguousarray(soft)), O.ptr(buf))
            assert rc == orc and np.array_equal(out, buf), (name, rc, orc)
            n += 1
    assert n >= len(F.FAMILIES)  # (beyond has no block that decodes, positions and miscorrections none that fails)


# ------------------------------------------------------------------------------------------------ streams that carry chosen blocks
def stream_symbols(blocks, rng):
    """the frames' symbols, then PAD filler symbols whose last one makes the number of phase reversals even: the differential
    signs then wrap without a seam, and a stream generated from the filler on runs filler, frame 0, 1, ..., filler again"""
    sym = np.concatenate([np.asarray(b) >> 7 for b in blocks] + [rng.integers(0, 2, PAD, dtype=np.uint8)]).astype(np.uint8)
    if np.count_nonzero(sym == 0) & 1:
        sym[-1] ^= 1
    return sym


def synth_iq(sym, n0, n, stride_pairs=None):
    """sym [S][nsym] (0 / 1) -> device int16 IQ [S][stride_pairs] pairs: samples n0 .. n0 + n of each stream, carrier 13 200 Hz,
    no noise (the generator of bench.py, csrc/synth.hip)"""
    S, nsym = sym.shape
    stride_pairs = stride_pairs or n
    ct, st = O.synth_tables(3000)
    bufs = [J.DeviceBuffer.from_host(sym), J.DeviceBuffer(S * nsym), J.DeviceBuffer.from_host(ct), J.DeviceBuffer.from_host(st),
            J.DeviceBuffer.from_host(np.zeros(S, np.uint64))]
    d_iq = J.DeviceBuffer(S * stride_pairs * 4)
    try:
        if stride_pairs != n:
            d_iq.zero()
        J.synth_diffsign(bufs[0], nsym, S, bufs[1])
        J.synth_dbpsk(d_iq, 2 * stride_pairs, S, n0, n, bufs[1], nsym, SPS, 0, O.phase_inc_u32(13200.0, 96000), bufs[2], bufs[3], 0, bufs[4])
        J.binding.stream_sync()
    finally:
        for b in bufs:
            b.free()
    return d_iq


def whole_frames(n):
    return -(-n // 2048) * 2048


def call_lengths(nfr):
    """one frame's end per call: the first call runs SLACK symbols past frame 0, the last to the stream's end.  The calls are
    ragged; their sum is a whole number of 2048-sample frames, which is what the oracle's receive() takes."""
    first = (PAD + F.SYMPBLOCK + SLACK) * SPS
    total = whole_frames((PAD + nfr * F.SYMPBLOCK + 2 * SLACK) * SPS)
    return [first] + [FRAME] * (nfr - 2) + [total - first - FRAME * (nfr - 2)]


def cut_block(hist, end):
    """the 5200 hard symbols the hook decodes at a hit whose trigger bit is bit end - 1 of the stream's history (0xc0 for a bit
    of +1, else 0x40; bits from before the stream began are 0: FUNcubeBPSKDemod.java:562-564)"""
    w = np.zeros(F.SYMPBLOCK, np.int8)
    lo = end - F.SYMPBLOCK
    w[max(0, -lo):] = hist[max(0, lo):end]
    return np.where(w == 1, 0xC0, 0x40).astype(np.uint8)


def check_hits(bits, fec, decoded, what):
    """one stream: bits / fec = per call; every hit's rc and bytes against O.fec_decode of the block cut out of the stream's own
    bits, with the reference's rule that a failed decode keeps the previous bytes.  Returns the cut blocks."""
    hist = np.concatenate(bits)
    cur = np.zeros(256, np.uint8)
    base, cuts = 0, []
    for b, hits in zip(bits, fec):
        for rc, bi, data in hits:
            soft = cut_block(hist, base + bi)
            orc, oout = O.fec_decode(soft)
            assert rc == orc, (what, len(cuts), rc, orc)
            if orc >= 0:
                cur = oout
            assert np.array_equal(data, cur), (what, len(cuts), rc)
            cuts.append(soft)
        base += len(b)
    assert np.array_equal(decoded, cur), what
    return cuts


def validate_cut_rule(iq, bits, what):
    """the cutting rule itself, on the oracle's own log: O.Bpsk's hits are O.fec_decode of the cut blocks"""
    o = O.Bpsk()
    o.receive_i16(iq)
    hist = o.bits()
    assert np.array_equal(hist, np.concatenate(bits)), what
    res = o.fec_results()
    assert res, what
    cur = np.zeros(256, np.uint8)
    for rc, bidx, data in res:
        orc, oout = O.fec_decode(cut_block(hist, bidx))
        cur = oout if orc >= 0 else cur
        assert rc == orc and np.array_equal(data, cur), (what, rc, orc)


class Rows:
    """rows base .. of a device buffer [S][L] int16 pairs, for check_stream_against_oracle"""

    def __init__(self, d_iq, base, L):
        self.d_iq, self.off = d_iq, 4 * L * base

    def to_host(self, dtype, count=None, offset_bytes=0):
        return self.d_iq.to_host(dtype, count=count, offset_bytes=self.off + offset_bytes)


class HardStreams:
    """the hard families, shuffled, three frames a stream"""

    NFR = 3

    def __init__(self):
        rows = F.all_rows(F.HARD_FAMILIES)
        rng = np.random.default_rng(20261120)
        order = rng.permutation(len(rows))
        rows = [rows[i] for i in order]
        while len(rows) % self.NFR:
            rows.append(rows[len(rows) % 7])
        frames = [rows[i:i + self.NFR] for i in range(0, len(rows), self.NFR)]
        # at 10 and 12 % flips the sync column may fall below the correlation threshold and the frame ends without a hit: those
        # streams go last, so that the tests which count on one hit per stream and call can take theirs from the front
        weak = [any(r[1].startswith(("dense_10pc", "dense_12pc")) for r in fr) for fr in frames]
        self.frames = [fr for fr, w in zip(frames, weak) if not w] + [fr for fr, w in zip(frames, weak) if w]
        self.nsure = len(weak) - sum(weak)
        self.S = len(self.frames)
        self.sym = np.stack([stream_symbols([r[3] for r in fr], rng) for fr in self.frames])
        self.nsym = self.sym.shape[1]
        self.chunks = call_lengths(self.NFR)
        self.L = sum(self.chunks)
        self.d_iq = synth_iq(self.sym, self.NFR * FRAME, self.L)  # from the filler on

    def free(self):
        self.d_iq.free()

    def run(self, dem, base, n, d_iq=None):
        """rows base .. base + n of d_iq (default: the streams' own buffer) through a handle of n streams, call by call;
        per stream (bits, fec) per call"""
        d_iq = d_iq or self.d_iq
        bits = [[] for _ in range(n)]
        fec = [[] for _ in range(n)]
        pos = 0
        for c in self.chunks:
            dem.batch_i16(d_iq.ptr + 4 * (self.L * base + pos), 2 * self.L, c)
            info = dem.slot_info()
            slots = J.DeviceBuffer(n * info["slot_bytes"])
            try:
                dem.pack_slots(slots)
                J.binding.stream_sync()
                blob = slots.to_host(np.uint8).reshape(n, info["slot_bytes"])
            finally:
                slots.free()
            for s in range(n):
                bits[s].append(dem.bits(s).copy())
                fec[s].append(dem.fec_results(s))
                u = J.sharding.unpack_slot(blob[s], info)  # the packed slot carries the same bits, rc, bit index and bytes
                assert np.array_equal(u["bits"], bits[s][-1]), (base + s, "slot bits")
                assert len(u["fec"]) == len(fec[s][-1]), (base + s, "slot hits")
                for (a, b, c2), (x, y, z) in zip(u["fec"], fec[s][-1]):
                    assert a == x and b == y and np.array_equal(c2, z), (base + s, "slot fec")
            pos += c
        return bits, fec

    def check(self, dem, base, n, bits, fec, sampled, what):
        """every stream's hits against the oracle on its own cut blocks; the constructed blocks of the exact families arrive
        unchanged; `sampled` streams in full against O.Bpsk.  Returns (hits, cut blocks equal to their construction)."""
        nhits = nexact = 0
        for s in range(n):
            cuts = check_hits(bits[s], fec[s], dem.decoded(s), (what, base + s))
            nhits += len(cuts)
            for fam, name, _, soft in self.frames[base + s]:
                there = any(np.array_equal(c, soft) for c in cuts)
                nexact += there
                if fam in F.EXACT_FAMILIES:
                    assert there, (what, base + s, name, "the hook did not see the constructed block")
        for s in sampled:
            iq = check_stream_against_oracle(dem, Rows(self.d_iq, base, self.L), self.L, s, bits[s], None, [h for call in fec[s] for h in call])
            validate_cut_rule(iq, bits[s], (what, base + s))
        return nhits, nexact


@pytest.fixture(scope="module")
def hard():
    h = HardStreams()
    yield h
    h.free()


def test_form_c_batch_decoder_at_its_native_width(hard):
    """every hard block through k_fec_bits + k_vitq + k_fec_rs: one handle over all streams (>= 256: no environment override)"""
    assert hard.S >= 256
    dem = J.Bpsk(nstreams=hard.S, max_batch_samples=max(hard.chunks))
    bits, fec = hard.run(dem, 0, hard.S)
    assert "k_vitq" in dem.fec_kernel_name(), dem.fec_kernel_name()
    sampled = sorted({0, 1, hard.S // 3, hard.S // 2, hard.S - 2, hard.S - 1, 100, 255})
    nhits, nexact = hard.check(dem, 0, hard.S, bits, fec, sampled, "form C")
    assert nhits >= hard.S * hard.NFR - 128  # (the 128 frames at 10 and 12 % flips may end without a hit)
    fails = sum(rc < 0 for s in range(hard.S) for call in fec[s] for rc, _, _ in call)
    assert fails >= 300 and nhits - fails >= 800, (nhits, fails)
    print(f"form C: {nhits} blocks ({fails} fail), {nexact} of {hard.S * hard.NFR} frames arrived as constructed")


def test_form_b_one_wave_per_block(hard):
    """every hard block through k_fec_bpsk: handles below 256 streams over slices of the same input"""
    nhits = nexact = 0
    base = 0
    while base < hard.S:
        n = min(250, hard.S - base)
        dem = J.Bpsk(nstreams=n, max_batch_samples=max(hard.chunks))
        bits, fec = hard.run(dem, base, n)
        assert dem.fec_kernel_name() == "k_fec_bpsk", dem.fec_kernel_name()
        a, b = hard.check(dem, base, n, bits, fec, sorted({0, n // 2, n - 1, 7}), "form B")
        nhits += a
        nexact += b
        base += n
        del dem
    assert nhits >= hard.S * hard.NFR - 128
    print(f"form B: {nhits} blocks, {nexact} of {hard.S * hard.NFR} frames arrived as constructed")


def test_form_b_fused_single_stream_frame_by_frame(hard):
    """three streams, each on a 1-stream handle driven through receive() frame by frame: k_fec_bpsk's fused form, in which the
    block that finishes last runs stage 2 itself"""
    nfr = hard.L // 2048
    picked = []
    for want in ("miscorrections", "beyond", "grid"):
        picked.append(next(s for s in range(hard.nsure) if s not in picked and any(r[0] == want for r in hard.frames[s])))
    nhits = 0
    for s in picked:
        iq = hard.d_iq.to_host(np.int16, count=2 * hard.L, offset_bytes=4 * hard.L * s)
        dem = J.Bpsk(nstreams=1)
        bits, fec = [], []
        for k in range(nfr):
            dem.receive_raw(iq[4096 * k:4096 * (k + 1)])
            bits.append(dem.bits(0).copy())
            fec.append(dem.fec_results(0))
        assert dem.fec_kernel_name() == "k_fec_bpsk", dem.fec_kernel_name()
        cuts = check_hits(bits, fec, dem.decoded(0), ("fused", s))
        assert len(cuts) >= hard.NFR - 1  # (whole frames of 2048 samples: the stream's last few symbols are not fed)
        for fam, name, _, soft in hard.frames[s][:len(cuts)]:
            if fam in F.EXACT_FAMILIES:
                assert any(np.array_equal(c, soft) for c in cuts), (s, name)
        o = O.Bpsk()
        o.receive_i16(iq[:4096 * nfr])
        assert np.array_equal(np.concatenate(bits), o.bits())
        got = [h for call in fec for h in call]
        assert [(a, d.tobytes()) for a, _, d in got] == [(a, d.tobytes()) for a, _, d in o.fec_results()]
        assert np.array_equal(dem.decoded(0), o.decoded())
        nhits += len(cuts)
        del dem
    print(f"form B fused: {nhits} blocks")


@pytest.mark.parametrize("nhits_per_call", [1, 15, 16, 17])
def test_form_c_partly_filled_wave(hard, nhits_per_call, monkeypatch):
    """small handles forced into the batch form: calls that end 1, 15, 16 and 17 frames -- k_vitq's partly filled wave, in which
    the surplus quads shadow the last block and store nothing"""
    monkeypatch.setenv("JSDR_VITQ", "1")
    n = max(nhits_per_call, 2)
    base = {1: 40, 15: 60, 16: 90, 17: 120}[nhits_per_call]
    assert base + n <= hard.nsure
    dem = J.Bpsk(nstreams=n, max_batch_samples=max(hard.chunks))
    d_two = None
    try:
        if nhits_per_call == 1:  # two streams, the second one silent (no signal: no bits, no hits)
            row = hard.d_iq.to_host(np.int16, count=2 * hard.L, offset_bytes=4 * hard.L * base)
            d_two = J.DeviceBuffer.from_host(np.stack([row, np.zeros_like(row)]))
            bits, fec = hard.run(dem, 0, 2, d_two)
            assert "k_vitq" in dem.fec_kernel_name(), dem.fec_kernel_name()
            assert all(len(b) == 0 for b in bits[1]) and all(len(f) == 0 for f in fec[1])
            assert [len(f) for f in fec[0]] == [1] * hard.NFR, [len(f) for f in fec[0]]
            cuts = check_hits(bits[0], fec[0], dem.decoded(0), ("1 hit", base))
            for fam, name, _, soft in hard.frames[base]:
                assert fam not in F.EXACT_FAMILIES or any(np.array_equal(c, soft) for c in cuts), name
        else:
            bits, fec = hard.run(dem, base, n)
            assert "k_vitq" in dem.fec_kernel_name(), dem.fec_kernel_name()
            per_call = [sum(len(fec[s][c]) for s in range(n)) for c in range(hard.NFR)]
            assert nhits_per_call in per_call, per_call  # (a false alarm of the sync correlation may add a hit to a call)
            hard.check(dem, base, n, bits, fec, [0, n - 1], f"{nhits_per_call} hits")
    finally:
        if d_two is not None:
            d_two.free()
        del dem


# ------------------------------------------------------------------------------------------------ form D
def remainder_classes():
    """97 classes x 3 frames: the first 48 classes carry hard cases of families 1, 2, 4 and 7, the rest clean frames"""
    grid = {r[0]: r for r in F.family("grid")}
    edges = ["grid_16_0", "grid_0_16", "grid_1_16", "grid_17_0", "grid_0_17", "grid_16_17", "grid_16_16", "grid_18_18", "grid_0_0"]
    rows = [("grid", *grid[n]) for n in edges] + [("grid", *r) for r in F.family("grid")[5::11]][:31]
    rows += [("beyond", *r) for r in F.family("beyond")[::7]][:29]
    rows += [("miscorrections", *r) for r in F.family("miscorrections")]
    rows += [("dense", *r) for r in F.family("dense")[3::6]][:62]
    assert len(rows) == 144, len(rows)
    rng = np.random.default_rng(20261121)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    while len(rows) < 3 * B.P:
        pay = rng.integers(0, 256, 256, dtype=np.uint8)
        rows.append(("clean", f"clean_{len(rows)}", pay, F.soft_of(O.fec_encode(pay))))
    frames = [rows[3 * c:3 * c + 3] for c in range(B.P)]
    return frames, np.stack([stream_symbols([r[3] for r in fr], rng) for fr in frames])


def class_iq(sym, n0, n, stride_pairs):
    d = synth_iq(sym, n0, n, stride_pairs)
    try:
        return d.to_host(np.int16).reshape(B.P, 2 * stride_pairs)
    finally:
        d.free()


def unpack_all(dem, slots, S):
    info = dem.slot_info()
    dem.pack_slots(slots)
    J.binding.stream_sync()
    B.check_twins(slots, S, info["slot_bytes"], what="slot of stream")  # bits, rc, bit index and bytes: twins equal twins
    blob = slots.to_host(np.uint8, count=S * info["slot_bytes"]).reshape(S, info["slot_bytes"])
    return [J.sharding.unpack_slot(blob[s], info) for s in range(S)]


def device_cu_count():
    """(CU count of device 0, what went wrong): torch's device properties, read in a child process -- torch brings a HIP runtime
    of its own, and this process has the library's loaded"""
    import subprocess
    import sys
    code = "import torch; print('CUS', torch.cuda.get_device_properties(0).multi_processor_count)"
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        for line in r.stdout.splitlines():
            if line.startswith("CUS "):
                return int(line.split()[1]), ""
        return 0, (r.stderr or r.stdout).strip()[-300:]
    except Exception as e:  # noqa: BLE001
        return 0, repr(e)


def test_form_d_the_remainder_of_a_quad_launch():
    """One call whose hit count H leaves k_vitq a remainder: H >= quad_cap and 0 < H mod quad_cap < 4096 (vq_quad_blocks), with
    quad_cap = 64 x the device's CU count; asserted on the measured H before anything else, so the test cannot pass without the
    lane = state branch of k_vitq (and k_fec_rs's matching early return) having run.  Streams: quad_cap / 2 + about 250, two
    frames in the first call, input rows filled periodically from 97 classes (tests/big_offsets.py) at a padded stride: 29 GB on
    a 256-CU device.  Which items land in the remainder is decided by an atomic compaction and is not reproducible: every stream
    is checked (one oracle call per class and hit on the class's own cut block; every stream's slot equals its twin's), and every
    hard case recurs in about 87 streams.  A second call with one frame a stream follows on the same handle: H < quad_cap, all
    quad waves, over the stale rows of the first call.
    The other tests that reach 8192 streams (test_gpu_large_shapes.py) give every stream 2, then 3 hits a call: 16 384 and
    24 576 hits, remainders 0 and 8192 on 256 CUs -- all quad waves; test_gpu_headline_mode.py stays below quad_cap."""
    cus, why = device_cu_count()
    if cus <= 0:
        pytest.skip(f"the device's CU count cannot be read through torch: {why}")
    quad_cap = 64 * cus
    frames, sym = remainder_classes()
    n1 = whole_frames((PAD + 2 * F.SYMPBLOCK + SLACK) * SPS)  # (whole 2048-sample frames: the oracle replays call by call)
    n2 = whole_frames((F.SYMPBLOCK + SLACK) * SPS)
    stride = n1 + 4099
    src1 = class_iq(sym, 3 * FRAME, n1, stride)
    src2 = class_iq(sym, 3 * FRAME + n1, n2, stride)
    # the oracle's hits per class and call (bit-exact demodulator: the handle logs the same), and from them the stream count
    bits, hits = [], []
    for c in range(B.P):
        o = O.Bpsk()
        b, h = [], []
        for src, n in ((src1, n1), (src2, n2)):
            nb, nf = len(o.bits()), len(o.fec_results())
            o.receive_i16(src[c][:2 * n])
            b.append(o.bits()[nb:].copy())
            h.append([(rc, bidx - nb, data) for rc, bidx, data in o.fec_results()[nf:]])
        bits.append(b)
        hits.append(h)
        check_hits(b, h, o.decoded(), ("oracle", c))  # the cutting rule on the oracle's own log
    per = np.array([len(h[0]) for h in hits])
    assert per.min() >= 2, per
    cum = np.cumsum(per[np.arange(quad_cap) % B.P])
    S = int(np.searchsorted(cum, quad_cap + 512) + 1)
    H_want = int(cum[S - 1])
    assert H_want >= quad_cap and 0 < H_want % quad_cap < 4096, (S, H_want, quad_cap)
    H2_want = int(sum(len(hits[s % B.P][1]) for s in range(S)))
    assert 0 < H2_want < quad_cap, (H2_want, quad_cap)
    dem = J.Bpsk(nstreams=S, max_batch_samples=n1)
    d_in = slots = None
    try:
        d_in = J.DeviceBuffer(S * 4 * stride)
        assert d_in.nbytes <= 34.5e9 * cus / 256, d_in.nbytes
        slots = J.DeviceBuffer(S * dem.slot_info()["slot_bytes"])
        cur = [np.zeros(256, np.uint8) for _ in range(B.P)]
        for call, (src, n, want) in enumerate(((src1, n1, H_want), (src2, n2, H2_want))):
            B.fill_periodic(d_in, src, S)
            dem.batch_i16(d_in, 2 * stride, n)
            assert "k_vitq" in dem.fec_kernel_name(), dem.fec_kernel_name()
            u = unpack_all(dem, slots, S)
            H = sum(len(x["fec"]) for x in u)
            print(f"form D call {call}: H = {H}, quad_cap = {quad_cap}, H mod quad_cap = {H % quad_cap}, {S} streams, d_in {d_in.nbytes / 1e9:.1f} GB")
            if call == 0:
                assert H >= quad_cap and 0 < H % quad_cap < 4096, (H, quad_cap)  # the remainder branch has run
            else:
                assert H < quad_cap, (H, quad_cap)  # all quad waves
            assert H == want, (H, want)
            for s in range(S):
                c = B.twin(s)
                assert np.array_equal(u[s]["bits"], bits[c][call]), (call, s, "bits")
                got = u[s]["fec"]
                assert len(got) == len(hits[c][call]), (call, s)
                for (rc, bi, data), (orc, obi, odata) in zip(got, hits[c][call]):
                    assert rc == orc and bi == obi and np.array_equal(data, odata), (call, s, frames[c][0][1], rc, orc)
            for c in range(B.P):
                for rc, _, data in hits[c][call]:
                    cur[c] = data if rc >= 0 else cur[c]
            for s in list(range(0, S, 61)) + [S - 1]:
                assert np.array_equal(dem.decoded(s), cur[B.twin(s)]), (call, s)
        nfail = sum(rc < 0 for c in range(B.P) for h in hits[c] for rc, _, _ in h)
        assert nfail >= 20  # (the hard classes do fail where they should: the log's "previous bytes" rule is in play)
        print(f"form D: {H_want} + {H2_want} blocks, {H_want % quad_cap} of the first call's through the remainder")
    finally:
        for b in (d_in, slots):
            if b is not None:
                b.free()
        del dem
