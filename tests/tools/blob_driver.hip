// blob_driver.hip -- a stand-alone program over the checkpoint blob's codec (java-sdr_amd/csrc/bpsk_blob.hip), for
// tests/test_bpsk_blob_host.py: no device, no library.  It writes a 3-stream blob of patterned records through the codec's
// writer, parses it back field for field, and then gives the parser every truncation of the blob and the blob with each
// single byte inverted in turn, each in a heap block of exactly its length.  Every one of those must be refused.
//   stdout: "ok <blob bytes> <truncations refused> <flips refused>"; anything wrong: a line on stderr and exit status 1.
//   With an argument, the blob is also written to that file.
#include "../../java-sdr_amd/csrc/bpsk_blob.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace jsdr;

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return g_seed;
}
static double rnd_f64()
{
    // any finite bit pattern, negative zero and subnormals included now and then
    const uint64_t r = rnd();
    if ((r & 63) == 0) return -0.0;
    if ((r & 63) == 1) return 4.9406564584124654e-324;
    return (double)(int64_t)(r >> 8) * 1.1102230246251565e-16 - 0.25 * (double)(r & 0xff);
}

static int fail(const char *what, long long a = 0, long long b = 0)
{
    fprintf(stderr, "blob_driver: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

static void pattern(BlobRecord &r)
{
    for (double &v : r.tail_f64) v = rnd_f64();
    for (int32_t &v : r.tail_i32) v = (int32_t)rnd();
    for (int32_t &v : r.fec_i32) v = (int32_t)rnd();
    r.ave_peak_power = rnd_f64();
    r.ave_centre_bin = rnd_f64();
    r.centre_bin = (int32_t)(rnd() % 4096);
    for (double &v : r.fft_hist) v = rnd_f64();
    for (double &v : r.pst_f64) v = rnd_f64();
    for (uint16_t &v : r.pst_kh) v = (uint16_t)(rnd() % 257);
    for (auto &v : r.hist) {
        v[0] = (uint32_t)rnd();
        v[1] = (uint32_t)rnd();
    }
    for (auto &v : r.halo) {
        v[0] = rnd_f64();
        v[1] = rnd_f64();
    }
    for (uint8_t &v : r.decoded) v = (uint8_t)rnd();
    for (int8_t &v : r.reg) v = (int8_t)((int)(rnd() % 3) - 1);
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

static bool same_record(const BlobRecord &a, const BlobRecord &b)
{
    for (int i = 0; i < 13; i++)
        if (!same_bits(a.tail_f64[i], b.tail_f64[i])) return false;
    for (int i = 0; i < BLOB_HIST; i++)
        if (!same_bits(a.fft_hist[i], b.fft_hist[i]) || a.pst_kh[i] != b.pst_kh[i] || a.hist[i][0] != b.hist[i][0] || a.hist[i][1] != b.hist[i][1]) return false;
    for (int i = 0; i < 3; i++)
        if (!same_bits(a.pst_f64[i], b.pst_f64[i]) || a.fec_i32[i] != b.fec_i32[i]) return false;
    for (int i = 0; i < BLOB_HALO; i++)
        if (!same_bits(a.halo[i][0], b.halo[i][0]) || !same_bits(a.halo[i][1], b.halo[i][1])) return false;
    return memcmp(a.tail_i32, b.tail_i32, sizeof(a.tail_i32)) == 0 && same_bits(a.ave_peak_power, b.ave_peak_power) &&
           same_bits(a.ave_centre_bin, b.ave_centre_bin) && a.centre_bin == b.centre_bin && memcmp(a.decoded, b.decoded, 256) == 0 &&
           memcmp(a.reg, b.reg, BLOB_REG) == 0;
}

int main(int argc, char **argv)
{
    const uint32_t N = 3;
    BlobShared sh;
    sh.kind = BLOB_KIND_ORDINARY;
    sh.rate = 96000;
    sh.nsf = 2048;
    sh.do_fft = 1;
    sh.do_up = 1;
    sh.seam = 1;
    sh.hist_float = 1;
    sh.fft_state = 1;
    sh.ds_cnt = 7;
    sh.n_in = 0x123456789all;
    sh.n_ds = 0x12345678all;
    sh.tuning = 12345.678;
    sh.tu_phase = 1.25;
    sh.tu_inc = 0.8080808080808081;
    sh.vco_phase = -0.0;
    for (int i = 0; i < BLOB_HIST; i++) {
        sh.khist[i] = (uint8_t)(rnd() & 0xff);
        sh.mhist[i] = (uint8_t)(rnd() & 1);
    }
    const size_t total = blob_bytes(N);
    if (total != (size_t)BLOB_HEADER_BYTES + N * (size_t)BLOB_RECORD_BYTES) return fail("blob_bytes", (long long)total);
    if (blob_bytes(0) != 0 || blob_bytes(BLOB_MAX_COUNT + 1u) != 0 || blob_bytes(0xffffffffu) != 0) return fail("blob_bytes takes a count out of range");
    std::vector<BlobRecord> recs(N);
    std::vector<unsigned char> blob(total, 0xa5);  // (not zeros: the writer must clear what it does not set)
    if (blob_begin(blob.data(), total - 1, sh, N)) return fail("blob_begin wrote into a buffer that is too small");
    if (!blob_begin(blob.data(), total, sh, N)) return fail("blob_begin");
    for (uint32_t i = 0; i < N; i++) {
        pattern(recs[i]);
        blob_record_put(blob_record(blob.data(), i), recs[i]);
    }
    blob_seal(blob.data(), total);

    // ---- back, field for field
    {
        BlobShared got;
        uint32_t n = 0;
        char why[192] = "";
        if (!blob_parse(blob.data(), total, &got, &n, why, sizeof(why))) {
            fprintf(stderr, "blob_driver: the parser refuses the writer's blob: %s\n", why);
            return 1;
        }
        if (n != N || !blob_shared_equal(got, sh) || got.fft_state != sh.fft_state) return fail("the shared block does not come back", n);
        for (uint32_t i = 0; i < N; i++) {
            BlobRecord r;
            memset(&r, 0x5a, sizeof(r));
            blob_record_get(blob_record(static_cast<const void *>(blob.data()), i), r);
            if (!same_record(r, recs[i])) return fail("a record does not come back", i);
            // the image holds the fields and zeros, nothing else: writing what was read gives the same bytes
            std::vector<unsigned char> again(BLOB_RECORD_BYTES, 0xa5);
            blob_record_put(again.data(), r);
            if (memcmp(again.data(), blob_record(blob.data(), i), BLOB_RECORD_BYTES) != 0) return fail("a record's image is not canonical", i);
        }
        // a changed field of the shared block is a different block
        BlobShared other = sh;
        other.n_in += 1;
        if (blob_shared_equal(other, sh)) return fail("blob_shared_equal ignores n_in");
        other = sh;
        other.vco_phase = 0.0;  // (+0.0 against -0.0: bit for bit)
        if (blob_shared_equal(other, sh)) return fail("blob_shared_equal compares doubles by value");
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "wb");
        if (!f || fwrite(blob.data(), 1, total, f) != total) return fail("could not write the blob");
        fclose(f);
    }

    // ---- every truncation, in a heap block of exactly that length
    long long ntrunc = 0, nflip = 0;
    char why[192];
    for (size_t len = 0; len < total; len++) {
        unsigned char *p = static_cast<unsigned char *>(malloc(len ? len : 1));
        if (!p) return fail("malloc");
        memcpy(p, blob.data(), len);
        why[0] = 0;
        const bool ok = blob_parse(p, len, nullptr, nullptr, why, sizeof(why));
        free(p);
        if (ok) return fail("a truncated blob was accepted", (long long)len);
        if (!why[0]) return fail("a refusal without a reason", (long long)len);
        ntrunc++;
    }
    // ---- every single byte inverted
    {
        unsigned char *p = static_cast<unsigned char *>(malloc(total));
        if (!p) return fail("malloc");
        memcpy(p, blob.data(), total);
        for (size_t i = 0; i < total; i++) {
            p[i] = (unsigned char)~p[i];
            if (blob_parse(p, total, nullptr, nullptr, why, sizeof(why))) {
                free(p);
                return fail("a blob with one byte inverted was accepted", (long long)i);
            }
            p[i] = (unsigned char)~p[i];
            nflip++;
        }
        if (!blob_parse(p, total, nullptr, nullptr, why, sizeof(why))) {
            free(p);
            return fail("the blob is refused after its bytes were put back");
        }
        free(p);
    }
    // ---- the index-like fields of a record, one at a time out of range (what a forged checksum would let through)
    {
        BlobRecord r;
        memset(&r, 0, sizeof(r));
        r.tail_i32[0] = 7;     // peakPos
        r.tail_i32[1] = 0;     // newPeak
        r.tail_i32[4] = -123;  // (cntBit: data, any value)
        r.centre_bin = 950;    // (n / 2 - 74 for the 2048-sample frame)
        for (int8_t &v : r.reg) v = 77;  // (data)
        std::vector<unsigned char> img(BLOB_RECORD_BYTES);
        auto ok = [&](const BlobRecord &q, const BlobShared &s2) {
            blob_record_put(img.data(), q);
            why[0] = 0;
            const bool a = blob_record_check(img.data(), s2, why, sizeof(why));
            return a && !why[0] ? 1 : (!a && why[0] ? 0 : -1);
        };
        if (ok(r, sh) != 1) return fail("a record in range was refused");
        BlobRecord q = r;
        q.tail_i32[0] = 8;
        if (ok(q, sh) != 0) return fail("peakPos 8 was accepted");
        q = r;
        q.tail_i32[1] = -1;
        if (ok(q, sh) != 0) return fail("newPeak -1 was accepted");
        q = r;
        q.tail_i32[9] = 2;
        if (ok(q, sh) != 0) return fail("overflow 2 was accepted");
        for (int cb : {-1, 1, 101, 951, 0x7fffffff}) {
            q = r;
            q.centre_bin = cb;
            if (ok(q, sh) != 0) return fail("a centre bin out of range was accepted", cb);
        }
        for (int cb : {0, 102, 950}) {
            q = r;
            q.centre_bin = cb;
            if (ok(q, sh) != 1) return fail("a centre bin in range was refused", cb);
        }
        BlobShared tuned = sh;
        tuned.kind = BLOB_KIND_TUNED;
        r.pst_f64[0] = 12345.678;
        r.pst_f64[1] = -3.5;
        r.pst_f64[2] = 0.8;
        r.pst_kh[25] = 256;
        if (ok(r, tuned) != 1) return fail("a tuned record in range was refused");
        q = r;
        q.pst_kh[3] = 257;
        if (ok(q, tuned) != 0) return fail("tuner index 257 was accepted");
        if (ok(q, sh) != 1) return fail("an ordinary record is checked as a tuned one");
        const double nan = __builtin_nan(""), inf = __builtin_inf();
        for (int f = 0; f < 3; f++)
            for (double bad : {nan, inf}) {
                q = r;
                q.pst_f64[f] = bad;
                if (ok(q, tuned) != 0) return fail("a non-finite tuned field was accepted", f);
            }
        q = r;
        q.pst_f64[0] = 96000.0;
        if (ok(q, tuned) != 0) return fail("a tuning at the rate was accepted");
        q = r;
        q.pst_f64[1] = 6.5;
        if (ok(q, tuned) != 0) return fail("a tuPhase above 2 pi was accepted");
    }
    // a null blob, and a blob that is longer than it says
    if (blob_parse(nullptr, total, nullptr, nullptr, why, sizeof(why))) return fail("a null blob was accepted");
    {
        std::vector<unsigned char> longer(blob);
        longer.push_back(0);
        if (blob_parse(longer.data(), longer.size(), nullptr, nullptr, why, sizeof(why))) return fail("a blob with a byte behind it was accepted");
    }
    printf("ok %zu %lld %lld\n", total, ntrunc, nflip);
    return 0;
}
