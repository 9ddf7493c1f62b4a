"""Constructed AO-40 FEC blocks: chosen errors behind the convolutional code, and chosen damage in front of it.

Host side only (numpy + the oracle's constant tables); tests/test_fec_cases.py pins every construction against the oracle,
tests/test_gpu_fec_forms.py sends the blocks through the four forms of the decoder in csrc/fec.hip.

The byte-stream half of encode_FEC40 (FECDecoder.java:549-606, 662-688) is restated here from its definition:
  stream[320] = 256 payload bytes, then 64 RS parity bytes; byte i belongs to RS word i & 1, column 95 + (i >> 1)
  -> xor Scrambler[i] -> bits MSB first, six zero tail bits (2566 bits)
  -> K = 7 encoder: sr = (sr << 1) | bit; symbols parity(sr & 0x4f), 1 - parity(sr & 0x6d)
  -> interleaver: de-interleaved symbol j sits at block index (j % 65) * 80 + j // 65 + 1; column 0 holds the sync vector.
A stream whose bytes carry errors THE PARITY DOES NOT KNOW ABOUT is still a valid convolutional code word, so on a clean
channel the Viterbi decoder returns exactly those bytes and the RS stage sees exactly the chosen error pattern.

RS(255,223): the roots of the generator are alpha^(PRIM (FCR + i)), i < 32; decode_rs_8's Horner loop (:336-347) takes column 0
as the highest power, so the parity check matrix is H[i][j] = alpha^((FCR + i) PRIM (254 - j)).

Every family is seeded; a family is a list of rows (name, sent payload uint8[256], soft uint8[5200]).
"""
import numpy as np

import oracle_lib as O

NN, KK, NROOTS, FCR, PRIM, RSPAD = 255, 223, 32, 112, 11, 95
NBITS, ROWS, COLUMNS, SYMPBLOCK = 2566, 80, 65, 5200
NCOLS = NN - RSPAD  # 160 columns of a word travel; 95 .. 222 data, 223 .. 254 parity
SPECIAL_COLUMNS = (95, 96, 222, 223, 253, 254)  # first two, last data, first parity, last two (254: the Chien search's i = 255)
DENSE_RATES = (2, 4, 6, 8, 10, 12)  # per cent of the 5200 symbols flipped (family 7); see dense_hard_noise()

_T = {}


def tables():
    """exp / log of GF(256) and the scrambler from the oracle (pinned to the reference's literals by tests/test_oracle_tables.py),
    the 256 x 256 product table, and the generator polynomial's coefficients from x^32 down"""
    if not _T:
        exp = [int(v) for v in O.fec_table("ALPHA_TO")]
        log = [int(v) for v in O.fec_table("INDEX_OF")]
        mul = np.zeros((256, 256), np.uint8)
        for a in range(1, 256):
            for b in range(1, 256):
                mul[a, b] = exp[(log[a] + log[b]) % 255]
        g = [1]  # ascending powers; g(x) = prod (x - alpha^(PRIM (FCR + i)))
        for i in range(NROOTS):
            r = exp[(PRIM * (FCR + i)) % 255]
            g = [(g[k - 1] if k > 0 else 0) ^ (int(mul[g[k], r]) if k < len(g) else 0) for k in range(len(g) + 1)]
        assert len(g) == NROOTS + 1 and g[NROOTS] == 1
        _T.update(exp=exp, log=log, mul=mul, gdesc=np.array(g[::-1], np.uint8), scr=np.array(O.fec_table("Scrambler"), np.uint8))
        # interleaver position of de-interleaved symbol j, and the sync column (:600-605)
        j = np.arange(2 * NBITS)
        _T["pos"] = (j % COLUMNS) * ROWS + j // COLUMNS + 1
        sync = np.zeros(COLUMNS, np.uint8)
        sr = 0x7F
        for i in range(COLUMNS):
            sync[i] = 1 if sr & 64 else 0
            sr = ((sr << 1) | (bin(sr & 0x48).count("1") & 1)) & 0xFFFF
        _T["sync"] = sync
    return _T


def rs_parity(payload):
    """uint8[64]: the parity bytes of the stream (byte 256 + 2 q + w = parity symbol q of word w): payload(x) x^32 mod g(x)"""
    t = tables()
    payload = np.asarray(payload, np.uint8)
    out = np.zeros(64, np.uint8)
    gd = t["gdesc"][1:]
    for w in range(2):
        rem = np.zeros(NROOTS, np.uint8)
        for d in payload[w::2]:
            fb = int(d) ^ int(rem[0])
            rem = np.concatenate([rem[1:], np.zeros(1, np.uint8)])
            if fb:
                rem ^= t["mul"][fb][gd]
        out[w::2] = rem
    return out


def stream_of(payload):
    payload = np.asarray(payload, np.uint8)
    assert payload.size == 256
    return np.concatenate([payload, rs_parity(payload)])


def symbols_of_stream(stream320):
    """uint8[5200] of 0 / 1: scrambler, K = 7 encoder with the second output inverted, 65 x 80 interleaver, sync column"""
    t = tables()
    stream320 = np.asarray(stream320, np.uint8)
    assert stream320.size == 320
    bits = np.zeros(6 + NBITS, np.uint8)  # six zeros in front: the shift register's start
    bits[6:6 + 2560] = np.unpackbits(stream320 ^ t["scr"])  # MSB first (:559-566); the tail stays zero
    tap = lambda d: bits[6 - d:6 - d + NBITS]  # noqa: E731  bit k - d for every step k
    a = tap(0) ^ tap(1) ^ tap(2) ^ tap(3) ^ tap(6)       # 0x4f
    b = 1 ^ tap(0) ^ tap(2) ^ tap(3) ^ tap(5) ^ tap(6)   # 0x6d, inverted
    sym = np.zeros(SYMPBLOCK, np.uint8)
    sym[t["pos"][0::2]] = a
    sym[t["pos"][1::2]] = b
    sym[ROWS * np.arange(COLUMNS)] = t["sync"]
    return sym


def soft_of(sym):
    """hard symbols 0 / 1 as the demodulator files them (FUNcubeBPSKDemod.java:562-564)"""
    return np.where(np.asarray(sym) == 1, 0xC0, 0x40).astype(np.uint8)


def errored_stream(payload, errs0, errs1):
    """the 320-byte stream whose RS word 0 / 1 carries errs0 / errs1 = {column 95 .. 254: xor mask} behind its parity"""
    s = stream_of(payload)
    for w, errs in ((0, errs0), (1, errs1)):
        for col, mask in errs.items():
            assert RSPAD <= col < NN and 0 < mask < 256, (col, mask)
            s[2 * (col - RSPAD) + w] ^= mask
    return s


def with_byte_errors(payload, errs0, errs1):
    """symbols uint8[5200] (0 / 1) of that stream"""
    return symbols_of_stream(errored_stream(payload, errs0, errs1))


def codeword_of(payload, w):
    """the 255 columns of RS word w of a payload"""
    s = stream_of(payload)
    cw = np.zeros(NN, np.uint8)
    cw[RSPAD:] = s[w::2]
    return cw


def syndromes(cw):
    """H cw, plain: 32 field elements"""
    t = tables()
    out = []
    for i in range(NROOTS):
        s = 0
        for j in range(NN):
            if cw[j]:
                s ^= t["exp"][(t["log"][int(cw[j])] + (FCR + i) * PRIM * (254 - j)) % 255]
        out.append(s)
    return out


def weight33_codeword(support):
    """the RS(255,223) code word (unique up to scale; here its entry at support[-1] is 1) whose support lies in the 33 given
    columns: the null vector of the 32 x 33 system H[:, support], by Gaussian elimination over GF(256)"""
    t = tables()
    exp, log = t["exp"], t["log"]
    support = [int(c) for c in support]
    assert len(support) == 33 and len(set(support)) == 33 and all(0 <= c < NN for c in support)

    def gmul(a, b):
        return 0 if a == 0 or b == 0 else exp[(log[a] + log[b]) % 255]

    def ginv(a):
        return exp[(255 - log[a]) % 255]

    m = [[exp[((FCR + i) * PRIM * (254 - c)) % 255] for c in support] for i in range(NROOTS)]
    for p in range(NROOTS):
        piv = next(r for r in range(p, NROOTS) if m[r][p])  # any 32 columns of H are independent
        m[p], m[piv] = m[piv], m[p]
        inv = ginv(m[p][p])
        m[p] = [gmul(v, inv) for v in m[p]]
        for r in range(NROOTS):
            if r != p and m[r][p]:
                f = m[r][p]
                m[r] = [v ^ gmul(f, u) for v, u in zip(m[r], m[p])]
    cw = np.zeros(NN, np.uint8)
    for p in range(NROOTS):
        cw[support[p]] = m[p][32]  # x_p + m[p][32] x_32 = 0, x_32 = 1 (characteristic 2)
    cw[support[32]] = 1
    assert all(cw[c] for c in support), "a code word of weight < 33 cannot exist (minimum distance 33)"
    return cw


# ---------------------------------------------------------------------------------------------- families
def _payload(rng):
    return rng.integers(0, 256, 256, dtype=np.uint8)


def _errs(rng, n, cols=None):
    cols = rng.choice(np.arange(RSPAD, NN), n, replace=False) if cols is None else cols
    return {int(c): int(rng.integers(1, 256)) for c in cols}


def error_count_grid():
    """family 1: every (n0, n1), n0, n1 in 0 .. 18: random distinct columns, random non-zero masks (361 blocks)"""
    rng = np.random.default_rng(20261101)
    rows = []
    for n0 in range(19):
        for n1 in range(19):
            pay = _payload(rng)
            rows.append((f"grid_{n0}_{n1}", pay, soft_of(with_byte_errors(pay, _errs(rng, n0), _errs(rng, n1)))))
    return rows


def beyond_the_limit(nblocks=200):
    """family 2: one or both words carry 17 .. 40 errors (the other 0 .. 16): locator degrees up to 32, root count != degree"""
    rng = np.random.default_rng(20261102)
    rows = []
    for b in range(nblocks):
        big = int(rng.integers(17, 41))
        other = int(rng.integers(17, 41)) if b % 3 == 2 else int(rng.integers(0, 17))
        n0, n1 = (big, other) if b % 2 == 0 else (other, big)
        pay = _payload(rng)
        rows.append((f"beyond_{b}_{n0}_{n1}", pay, soft_of(with_byte_errors(pay, _errs(rng, n0), _errs(rng, n1)))))
    return rows


def positions():
    """family 3: single errors and 16-error sets at the special columns, 16 adjacent columns at either end, the same set in both
    words, and all 255 non-zero masks at one column (alternating words)"""
    rng = np.random.default_rng(20261103)
    rows = []

    def add(name, e0, e1):
        pay = _payload(rng)
        rows.append((name, pay, soft_of(with_byte_errors(pay, e0, e1))))

    others = [c for c in range(RSPAD, NN) if c not in SPECIAL_COLUMNS]
    for c in SPECIAL_COLUMNS:
        for w in range(2):
            e = _errs(rng, 1, [c])
            add(f"pos_single_{c}_w{w}", e if w == 0 else {}, e if w == 1 else {})
            e = _errs(rng, 16, [c] + [int(v) for v in rng.choice(others, 15, replace=False)])
            add(f"pos_set16_{c}_w{w}", e if w == 0 else {}, e if w == 1 else {})
    allsix = list(SPECIAL_COLUMNS) + [int(v) for v in rng.choice(others, 10, replace=False)]
    for w in range(2):
        e = _errs(rng, 16, allsix)
        add(f"pos_set16_all_special_w{w}", e if w == 0 else {}, e if w == 1 else {})
    for lo in (RSPAD, NN - 16):
        for w in range(2):
            e = _errs(rng, 16, range(lo, lo + 16))
            add(f"pos_adjacent_{lo}_w{w}", e if w == 0 else {}, e if w == 1 else {})
        add(f"pos_adjacent_{lo}_both", _errs(rng, 16, range(lo, lo + 16)), _errs(rng, 16, range(lo, lo + 16)))
    same = [int(v) for v in rng.choice(np.arange(RSPAD, NN), 16, replace=False)]
    add("pos_same_set_both", _errs(rng, 16, same), _errs(rng, 16, same))
    e = _errs(rng, 16, same)
    add("pos_same_set_same_masks_both", dict(e), dict(e))
    for mask in range(1, 256):
        c = SPECIAL_COLUMNS[mask % len(SPECIAL_COLUMNS)]
        add(f"pos_mask_{mask}_col{c}_w{mask & 1}", {c: mask} if mask & 1 == 0 else {}, {c: mask} if mask & 1 else {})
    return rows


def miscorrection_errors(rng, kind):
    """(errs, D): 17 errors on non-padding columns T of a weight-33 code word D's support, D's values as the masks.  The received
    word is 16 symbols from the valid word sent + D, so decode_rs_8 patches D's other 16 columns U and returns 16.
      kind a: U in the data / parity columns; b: U half in the padding, columns 0 and 94 among them; c: all of U in the padding
      (a, b, c: T holds a data column, so the payload comes back wrong); p: as c with T in the parity columns only (nothing of
      D touches the data: the payload still comes back, out of a word that is not the one sent)"""
    live = np.arange(RSPAD, NN)
    if kind == "p":
        t_cols = [int(v) for v in rng.choice(np.arange(KK, NN), 17, replace=False)]
    else:
        t_cols = [int(v) for v in rng.choice(live, 17, replace=False)]
        if not any(c < KK for c in t_cols):
            t_cols[0] = RSPAD + 3
    rest = [int(c) for c in live if c not in t_cols]
    if kind == "a":
        u_cols = [int(v) for v in rng.choice(rest, 16, replace=False)]
    elif kind == "b":
        u_cols = [0, 94] + [int(v) for v in rng.choice(np.arange(1, 94), 6, replace=False)] + [int(v) for v in rng.choice(rest, 8, replace=False)]
    else:
        u_cols = [0, 94] + [int(v) for v in rng.choice(np.arange(1, 94), 14, replace=False)]
    d = weight33_codeword(t_cols + u_cols)
    return {c: int(d[c]) for c in t_cols}, d


MISC_EXPECTED = {}  # name -> the payload decode_rs_8 is led to: the sent words + their D on the data columns


def miscorrections():
    """family 4: kinds a, b, c in word 0, in word 1 and in both; two blocks with different kinds in the two words; kind p in
    either word: 13 blocks.  A word without a miscorrection carries 0 .. 16 ordinary errors."""
    rng = np.random.default_rng(20261104)
    rows = []

    def add(name, k0, k1):
        pay = _payload(rng)
        want = pay.copy()
        errs = []
        for w, k in ((0, k0), (1, k1)):
            if k is None:
                errs.append(_errs(rng, int(rng.integers(0, 17))))
            else:
                e, d = miscorrection_errors(rng, k)
                errs.append(e)
                want[w::2] ^= d[RSPAD:KK]
        MISC_EXPECTED[name] = want
        rows.append((name, pay, soft_of(with_byte_errors(pay, errs[0], errs[1]))))

    for kind in "abc":
        add(f"misc_{kind}_w0", kind, None)
        add(f"misc_{kind}_w1", None, kind)
        add(f"misc_{kind}_both", kind, kind)
    add("misc_mixed_w0b_w1c", "b", "c")
    add("misc_mixed_w0c_w1a", "c", "a")
    add("misc_p_w0", "p", None)
    add("misc_p_w1", None, "p")
    return rows


SPAN_LENGTHS = sorted(set(range(0, 401, 8)) | set(range(120, 137)))  # across WARM = 128 of the parallel chain-back


def span_symbols(k, where):
    """block indices of the 2 k symbols of k consecutive trellis steps at the start, the middle or the end of the trellis"""
    s0 = {"start": 0, "middle": (NBITS - k) // 2, "end": NBITS - k}[where]
    return tables()["pos"][2 * s0:2 * (s0 + k)]


def chain_back_soft():
    """family 5 (soft input): spans of near-erasures (127 / 128) or of random soft bytes, everything else clean; all 256 soft
    byte values at one position against a sent 0 and a sent 1 (mettab's two irregular entries); a block of all 128"""
    rng = np.random.default_rng(20261105)
    rows = []
    for where in ("start", "middle", "end"):
        for k in SPAN_LENGTHS:
            for kind in ("erase", "random"):
                pay = _payload(rng)
                soft = soft_of(O.fec_encode(pay))
                idx = span_symbols(k, where)
                soft[idx] = rng.integers(127, 129, idx.size, dtype=np.uint8) if kind == "erase" else rng.integers(0, 256, idx.size, dtype=np.uint8)
                rows.append((f"span_soft_{kind}_{where}_{k}", pay, soft))
    pay = _payload(rng)
    sym = O.fec_encode(pay)
    pos = tables()["pos"]
    for sent in (0, 1):
        at = int(pos[next(j for j in range(2000, 2 * NBITS) if sym[pos[j]] == sent)])
        for v in range(256):
            soft = soft_of(sym)
            soft[at] = v
            rows.append((f"soft_value_{v}_sent{sent}", pay, soft))
    rows.append(("soft_all_128", pay, np.full(SYMPBLOCK, 128, np.uint8)))
    return rows


def chain_back_hard():
    """family 6 (hard input): the same spans with the symbols inverted"""
    rng = np.random.default_rng(20261106)
    rows = []
    for where in ("start", "middle", "end"):
        for k in SPAN_LENGTHS:
            pay = _payload(rng)
            sym = O.fec_encode(pay).copy()
            sym[span_symbols(k, where)] ^= 1
            rows.append((f"span_hard_{where}_{k}", pay, soft_of(sym)))
    return rows


def dense_hard_noise(per_rate=64):
    """family 7: random flips at DENSE_RATES per cent of the 5200 symbols, 64 blocks each.  Hard metrics take two values, so the
    add-compare-select meets m1 == m0 everywhere.  (The rates straddle the code's limit on the oracle: tests/test_fec_cases.py
    counts the blocks that decode and those that do not and asks for 32 of each.)"""
    rng = np.random.default_rng(20261107)
    rows = []
    for rate in DENSE_RATES:
        for b in range(per_rate):
            pay = _payload(rng)
            sym = O.fec_encode(pay).copy()
            sym[rng.choice(SYMPBLOCK, SYMPBLOCK * rate // 100, replace=False)] ^= 1
            rows.append((f"dense_{rate}pc_{b}", pay, soft_of(sym)))
    return rows


FAMILIES = {
    "grid": error_count_grid, "beyond": beyond_the_limit, "positions": positions, "miscorrections": miscorrections,
    "chain_back_soft": chain_back_soft, "chain_back_hard": chain_back_hard, "dense": dense_hard_noise,
}
HARD_FAMILIES = ("grid", "beyond", "positions", "miscorrections", "chain_back_hard", "dense")
EXACT_FAMILIES = ("grid", "positions", "miscorrections")  # behind the demodulator the cut block must EQUAL the constructed symbols

_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def all_rows(names=tuple(FAMILIES)):
    return [(f, *row) for f in names for row in family(f)]
