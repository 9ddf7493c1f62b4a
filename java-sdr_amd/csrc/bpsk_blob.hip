// bpsk_blob.hip -- the checkpoint blob's codec (bpsk_blob.h): writer, parser, checksum.  Host code only, no HIP runtime call,
// no handle: bytes in, bytes out.  Every field is placed and fetched byte by byte, so the image is the same on any host and
// nothing of a struct's padding ever reaches it.
#include "bpsk_blob.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace jsdr {

static const unsigned char kMagic[8] = {'J', 'S', 'D', 'R', 'B', 'P', 'S', 'K'};

// header offsets (bpsk_blob.h)
enum {
    H_MAGIC = 0, H_VERSION = 8, H_HBYTES = 12, H_RBYTES = 16, H_ZERO = 20, H_SUM = 24, H_TOTAL = 32, H_COUNT = 40, H_KIND = 44,
    H_RATE = 48, H_NSF = 52, H_FFT = 56, H_UP = 60, H_SEAM = 64, H_HFLOAT = 68, H_FFTST = 72, H_DSCNT = 76, H_ROFF = 80,
    H_NIN = 88, H_NDS = 96, H_TUNING = 104, H_TUPH = 112, H_TUINC = 120, H_VCO = 128, H_KHIST = 136, H_MHIST = 162,
    H_COVERED = 32  // the checksum covers [H_COVERED, total)
};
static_assert(H_MHIST + BLOB_HIST <= BLOB_HEADER_BYTES, "the header holds its fields");

static void put_u32(unsigned char *p, uint32_t v)
{
    for (int i = 0; i < 4; i++) p[i] = (unsigned char)(v >> (8 * i));
}
static void put_u64(unsigned char *p, uint64_t v)
{
    for (int i = 0; i < 8; i++) p[i] = (unsigned char)(v >> (8 * i));
}
static uint32_t get_u32(const unsigned char *p)
{
    uint32_t v = 0;
    for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i);
    return v;
}
static uint64_t get_u64(const unsigned char *p)
{
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i);
    return v;
}
static uint64_t f64_bits(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}
static double bits_f64(uint64_t b)
{
    double v;
    memcpy(&v, &b, 8);
    return v;
}

void blob_put_f64(unsigned char *p, double v) { put_u64(p, f64_bits(v)); }
double blob_get_f64(const unsigned char *p) { return bits_f64(get_u64(p)); }

uint64_t blob_fnv1a(const unsigned char *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

bool blob_shared_equal(const BlobShared &a, const BlobShared &b)
{
    return a.kind == b.kind && a.rate == b.rate && a.nsf == b.nsf && a.do_fft == b.do_fft && a.do_up == b.do_up && a.seam == b.seam &&
           a.hist_float == b.hist_float && a.ds_cnt == b.ds_cnt && a.n_in == b.n_in && a.n_ds == b.n_ds &&
           f64_bits(a.tuning) == f64_bits(b.tuning) && f64_bits(a.tu_phase) == f64_bits(b.tu_phase) &&
           f64_bits(a.tu_inc) == f64_bits(b.tu_inc) && f64_bits(a.vco_phase) == f64_bits(b.vco_phase) &&
           memcmp(a.khist, b.khist, BLOB_HIST) == 0 && memcmp(a.mhist, b.mhist, BLOB_HIST) == 0;
}

size_t blob_bytes(uint32_t count)
{
    if (count < 1 || count > BLOB_MAX_COUNT) return 0;
    return (size_t)BLOB_HEADER_BYTES + (size_t)count * BLOB_RECORD_BYTES;
}

bool blob_begin(void *blob, size_t cap, const BlobShared &sh, uint32_t count)
{
    const size_t total = blob_bytes(count);
    if (!blob || total == 0 || cap < total) return false;
    unsigned char *b = static_cast<unsigned char *>(blob);
    memset(b, 0, BLOB_HEADER_BYTES);  // (the records are written whole by whoever fills them)
    memcpy(b + H_MAGIC, kMagic, 8);
    put_u32(b + H_VERSION, BLOB_VERSION);
    put_u32(b + H_HBYTES, BLOB_HEADER_BYTES);
    put_u32(b + H_RBYTES, BLOB_RECORD_BYTES);
    put_u64(b + H_TOTAL, (uint64_t)total);
    put_u32(b + H_COUNT, count);
    put_u32(b + H_KIND, sh.kind);
    put_u32(b + H_RATE, sh.rate);
    put_u32(b + H_NSF, sh.nsf);
    put_u32(b + H_FFT, sh.do_fft);
    put_u32(b + H_UP, sh.do_up);
    put_u32(b + H_SEAM, sh.seam);
    put_u32(b + H_HFLOAT, sh.hist_float);
    put_u32(b + H_FFTST, sh.fft_state);
    put_u32(b + H_DSCNT, (uint32_t)sh.ds_cnt);
    put_u32(b + H_ROFF, BLOB_HEADER_BYTES);
    put_u64(b + H_NIN, (uint64_t)sh.n_in);
    put_u64(b + H_NDS, (uint64_t)sh.n_ds);
    blob_put_f64(b + H_TUNING, sh.tuning);
    blob_put_f64(b + H_TUPH, sh.tu_phase);
    blob_put_f64(b + H_TUINC, sh.tu_inc);
    blob_put_f64(b + H_VCO, sh.vco_phase);
    memcpy(b + H_KHIST, sh.khist, BLOB_HIST);
    memcpy(b + H_MHIST, sh.mhist, BLOB_HIST);
    return true;
}

void blob_record_put(unsigned char *rec, const BlobRecord &r)
{
    memset(rec, 0, BLOB_RECORD_BYTES);
    for (int i = 0; i < 13; i++) blob_put_f64(rec + REC_TAIL_F64 + 8 * i, r.tail_f64[i]);
    for (int i = 0; i < 10; i++) put_u32(rec + REC_TAIL_I32 + 4 * i, (uint32_t)r.tail_i32[i]);
    for (int i = 0; i < 3; i++) put_u32(rec + REC_FEC_I32 + 4 * i, (uint32_t)r.fec_i32[i]);
    blob_put_f64(rec + REC_FFT_AVE, r.ave_peak_power);
    blob_put_f64(rec + REC_FFT_AVE + 8, r.ave_centre_bin);
    put_u32(rec + REC_FFT_BIN, (uint32_t)r.centre_bin);
    for (int i = 0; i < BLOB_HIST; i++) blob_put_f64(rec + REC_FFT_HIST + 8 * i, r.fft_hist[i]);
    for (int i = 0; i < 3; i++) blob_put_f64(rec + REC_PST_F64 + 8 * i, r.pst_f64[i]);
    for (int i = 0; i < BLOB_HIST; i++) {
        rec[REC_PST_KH + 2 * i] = (unsigned char)(r.pst_kh[i] & 0xff);
        rec[REC_PST_KH + 2 * i + 1] = (unsigned char)(r.pst_kh[i] >> 8);
        put_u32(rec + REC_HIST + 8 * i, r.hist[i][0]);
        put_u32(rec + REC_HIST + 8 * i + 4, r.hist[i][1]);
    }
    for (int i = 0; i < BLOB_HALO; i++) {
        blob_put_f64(rec + REC_HALO + 16 * i, r.halo[i][0]);
        blob_put_f64(rec + REC_HALO + 16 * i + 8, r.halo[i][1]);
    }
    memcpy(rec + REC_DECODED, r.decoded, 256);
    memcpy(rec + REC_REG, r.reg, BLOB_REG);
}

void blob_record_get(const unsigned char *rec, BlobRecord &r)
{
    for (int i = 0; i < 13; i++) r.tail_f64[i] = blob_get_f64(rec + REC_TAIL_F64 + 8 * i);
    for (int i = 0; i < 10; i++) r.tail_i32[i] = (int32_t)get_u32(rec + REC_TAIL_I32 + 4 * i);
    for (int i = 0; i < 3; i++) r.fec_i32[i] = (int32_t)get_u32(rec + REC_FEC_I32 + 4 * i);
    r.ave_peak_power = blob_get_f64(rec + REC_FFT_AVE);
    r.ave_centre_bin = blob_get_f64(rec + REC_FFT_AVE + 8);
    r.centre_bin = (int32_t)get_u32(rec + REC_FFT_BIN);
    for (int i = 0; i < BLOB_HIST; i++) r.fft_hist[i] = blob_get_f64(rec + REC_FFT_HIST + 8 * i);
    for (int i = 0; i < 3; i++) r.pst_f64[i] = blob_get_f64(rec + REC_PST_F64 + 8 * i);
    for (int i = 0; i < BLOB_HIST; i++) {
        r.pst_kh[i] = (uint16_t)(rec[REC_PST_KH + 2 * i] | (rec[REC_PST_KH + 2 * i + 1] << 8));
        r.hist[i][0] = get_u32(rec + REC_HIST + 8 * i);
        r.hist[i][1] = get_u32(rec + REC_HIST + 8 * i + 4);
    }
    for (int i = 0; i < BLOB_HALO; i++) {
        r.halo[i][0] = blob_get_f64(rec + REC_HALO + 16 * i);
        r.halo[i][1] = blob_get_f64(rec + REC_HALO + 16 * i + 8);
    }
    memcpy(r.decoded, rec + REC_DECODED, 256);
    memcpy(r.reg, rec + REC_REG, BLOB_REG);
}

void blob_seal(void *blob, size_t bytes)
{
    unsigned char *b = static_cast<unsigned char *>(blob);
    put_u64(b + H_SUM, blob_fnv1a(b + H_COVERED, bytes - H_COVERED));
}

// the reason of a refusal as text; the compiler checks every format against its arguments
__attribute__((format(printf, 3, 4))) static bool refuse(char *why, size_t cap, const char *fmt, ...)
{
    if (why && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, cap, fmt, ap);
        va_end(ap);
    }
    return false;
}

static bool finite_f64(double v) { return (f64_bits(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

bool blob_parse(const void *blob, size_t bytes, BlobShared *sh, uint32_t *count, char *why, size_t why_cap)
{
    if (!blob) return refuse(why, why_cap, "null blob");
    const unsigned char *b = static_cast<const unsigned char *>(blob);
    // the fixed part first: nothing beyond `bytes` is read
    if (bytes < (size_t)BLOB_HEADER_BYTES) return refuse(why, why_cap, "%zu bytes are too short for a blob's header (%d)", bytes, (int)BLOB_HEADER_BYTES);
    if (memcmp(b + H_MAGIC, kMagic, 8) != 0) return refuse(why, why_cap, "wrong magic: not a BPSK checkpoint blob");
    if (get_u32(b + H_VERSION) != BLOB_VERSION) return refuse(why, why_cap, "format version %u, this library reads version %d", get_u32(b + H_VERSION), (int)BLOB_VERSION);
    if (get_u32(b + H_HBYTES) != BLOB_HEADER_BYTES || get_u32(b + H_ROFF) != BLOB_HEADER_BYTES)
        return refuse(why, why_cap, "header of %u bytes, version 1 has %d", get_u32(b + H_HBYTES), (int)BLOB_HEADER_BYTES);
    if (get_u32(b + H_RBYTES) != BLOB_RECORD_BYTES) return refuse(why, why_cap, "record size %u, version 1 has %d", get_u32(b + H_RBYTES), (int)BLOB_RECORD_BYTES);
    if (get_u32(b + H_ZERO) != 0) return refuse(why, why_cap, "a reserved header word is not zero");
    // the count is bounded before it is multiplied; then the blob must be exactly as long as it says
    const uint32_t n = get_u32(b + H_COUNT);
    const size_t total = blob_bytes(n);
    if (total == 0) return refuse(why, why_cap, "stream count %u outside 1 .. %d", n, (int)BLOB_MAX_COUNT);
    if (get_u64(b + H_TOTAL) != (uint64_t)total) return refuse(why, why_cap, "the header gives %llu bytes, %u streams take %zu", (unsigned long long)get_u64(b + H_TOTAL), n, total);
    if (bytes != total) return refuse(why, why_cap, "%zu bytes given, the blob is %zu bytes long (truncated, or not a whole blob)", bytes, total);
    if (get_u64(b + H_SUM) != blob_fnv1a(b + H_COVERED, total - H_COVERED)) return refuse(why, why_cap, "checksum mismatch: the blob is damaged");
    BlobShared s;
    s.kind = get_u32(b + H_KIND);
    s.rate = get_u32(b + H_RATE);
    s.nsf = get_u32(b + H_NSF);
    s.do_fft = get_u32(b + H_FFT);
    s.do_up = get_u32(b + H_UP);
    s.seam = get_u32(b + H_SEAM);
    s.hist_float = get_u32(b + H_HFLOAT);
    s.fft_state = get_u32(b + H_FFTST);
    s.ds_cnt = (int32_t)get_u32(b + H_DSCNT);
    s.n_in = (int64_t)get_u64(b + H_NIN);
    s.n_ds = (int64_t)get_u64(b + H_NDS);
    s.tuning = blob_get_f64(b + H_TUNING);
    s.tu_phase = blob_get_f64(b + H_TUPH);
    s.tu_inc = blob_get_f64(b + H_TUINC);
    s.vco_phase = blob_get_f64(b + H_VCO);
    memcpy(s.khist, b + H_KHIST, BLOB_HIST);
    memcpy(s.mhist, b + H_MHIST, BLOB_HIST);
    // values no handle can have written
    if (s.kind > BLOB_KIND_TUNED || s.do_fft > 1 || s.do_up > 1 || s.seam > 2 || s.hist_float > 1 || s.fft_state > 1)
        return refuse(why, why_cap, "a flag of the shared block is out of range");
    if (s.rate < 1 || s.rate > 0x7fffffffu || s.nsf < 1 || s.nsf > 0x7fffffffu) return refuse(why, why_cap, "rate %u or frame size %u out of range", s.rate, s.nsf);
    const int32_t decim = (int32_t)(s.rate / 9600 > 0 ? s.rate / 9600 : 1);
    if (s.ds_cnt < 0 || s.ds_cnt >= decim || s.n_in < 0 || s.n_ds < 0 || s.n_ds > s.n_in)
        return refuse(why, why_cap, "the shared block's counters are out of range");
    if (s.kind == BLOB_KIND_TUNED && (s.do_fft || s.seam || s.fft_state)) return refuse(why, why_cap, "a tuned handle's blob in FFT-acquire");
    if ((s.do_fft || s.seam) && !s.fft_state) return refuse(why, why_cap, "FFT-acquire without FFT-acquire state");
    for (int i = 0; i < BLOB_HIST; i++)
        if (s.mhist[i] > 1) return refuse(why, why_cap, "a mix flag of the shared block is out of range");
    // the phases the host scheduler turns into table indices: finite, and inside the range its casts take
    if (!finite_f64(s.tuning) || !finite_f64(s.tu_inc) || !finite_f64(s.tu_phase) || !(s.tu_phase < BLOB_TU_MAX))
        return refuse(why, why_cap, "the shared block's tuning (%g Hz), tuPhaseInc (%g) or tuPhase (%g) is not a finite value in range", s.tuning,
                      s.tu_inc, s.tu_phase);
    if (!finite_f64(s.vco_phase) || !(s.vco_phase >= 0.0 && s.vco_phase <= BLOB_TWO_PI))
        return refuse(why, why_cap, "the shared block's vcoPhase (%g) is outside 0 .. 2 pi", s.vco_phase);
    if (sh) *sh = s;
    if (count) *count = n;
    return true;
}

bool blob_record_check(const unsigned char *rec, const BlobShared &sh, char *why, size_t why_cap)
{
    const int32_t peak = (int32_t)get_u32(rec + REC_TAIL_I32), newp = (int32_t)get_u32(rec + REC_TAIL_I32 + 4);
    if (peak < 0 || peak > 7 || newp < 0 || newp > 7) return refuse(why, why_cap, "bit-clock position %d / %d outside 0 .. 7", peak, newp);
    const uint32_t ov = get_u32(rec + REC_TAIL_I32 + 36);
    if (ov > 1) return refuse(why, why_cap, "overflow flag %u", ov);
    // the centre bin the FFT-acquire front ends gather 204 bins around: 0 (no frame yet) or what the rule can leave (:446-459)
    const int32_t cb = (int32_t)get_u32(rec + REC_FFT_BIN);
    const int32_t cb_max = (int32_t)(sh.nsf / 2) - 74 > 102 ? (int32_t)(sh.nsf / 2) - 74 : 102;
    if (cb != 0 && (cb < 102 || cb > cb_max)) return refuse(why, why_cap, "centre bin %d outside 102 .. %d", cb, cb_max);
    if (sh.kind == BLOB_KIND_TUNED) {
        for (int i = 0; i < BLOB_HIST; i++) {
            const unsigned k = rec[REC_PST_KH + 2 * i] | ((unsigned)rec[REC_PST_KH + 2 * i + 1] << 8);
            if (k > 256) return refuse(why, why_cap, "tuner index %u above 256", k);
        }
        const double tuning = blob_get_f64(rec + REC_PST_F64), tu = blob_get_f64(rec + REC_PST_F64 + 8), inc = blob_get_f64(rec + REC_PST_F64 + 16);
        if (!finite_f64(tuning) || !(tuning < (double)sh.rate) || !finite_f64(inc) || !finite_f64(tu) || !(tu <= BLOB_TWO_PI))
            return refuse(why, why_cap, "a tuned stream's tuning (%g Hz), tuPhaseInc (%g) or tuPhase (%g) is not a finite value in range", tuning, inc, tu);
    }
    return true;
}

}  // namespace jsdr
