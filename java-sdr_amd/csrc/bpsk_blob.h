// bpsk_blob.h -- the checkpoint blob of a BPSK handle (jsdr_bpsk_save / jsdr_bpsk_restore): its layout, writer and parser.
//
// A blob is what a range of a handle's streams needs to carry on in another handle, process or machine: one SHARED block (the
// input-independent state every stream of the handle has in common) and one RECORD per stream.  Little-endian, fixed-width
// fields at the fixed offsets below; no pointer, no struct padding and no uninitialised byte: the writer starts from a zeroed
// image and places every field by itself.  Nothing in it depends on the handle's max_batch_samples, strides or buffer choices.
//
//   header (BLOB_HEADER_BYTES)            records (count x BLOB_RECORD_BYTES, from records_offset, each 16-byte aligned)
//     0  magic "JSDRBPSK"                   0     dmEnergy[8], dmEnergyOut, lastI, lastQ, energy1, energy2   (13 doubles)
//     8  u32 version (1)                    104   peakPos, newPeak, dmCorr, dmMaxCorr, cntBit, cntFEC, cntDec, dmErrBits,
//     12 u32 header bytes                         decodeOK, overflow (TailState's ten ints that are state; its fast-variant
//     16 u32 record bytes                         fields and nbits_prev are not)
//     20 u32 zero                           144   fec_last[2] (dmErrBits, decodeOK as the counters report them), cnt_dec, zero
//     24 u64 checksum of [32, total)        160   avePeakPower, aveCentreBin, i32 centreBin, zero          (FftFrontState)
//     32 u64 total bytes                    192   FftFrontState::hist[26]                                   (doubles)
//     40 u32 count                          400   tuned handle: tuning, tuPhase, tuPhaseInc of the stream   (else zero)
//     44 u32 kind (0 ordinary, 1 tuned)     432   tuned handle: the 26 nine-bit tuner indices, u16          (else zero)
//     48 u32 rate                           496   the 26 input samples: 8 bytes each -- (int16 I | int16 Q << 16, 0) or the
//     52 u32 samples per frame                    float pair's bits, as the shared block's hist_float says
//     56 u32 do_fft  60 u32 do_up           704   the 64 VCO-mixed samples before the next matched-filter window (double2)
//     64 u32 seam    68 u32 hist_float      1728  decoded[256]
//     72 u32 fft_state (the handle holds    1984  the 5200-entry FEC register (dmFECCorr), oldest first, one int8 a bit
//        FFT-acquire state)                 7184  = BLOB_RECORD_BYTES
//     76 i32 dsCnt
//     80 u32 records_offset  84 u32 zero
//     88 i64 n_in   96 i64 n_ds
//     104 tuning  112 tuPhase  120 tuPhaseInc  128 vcoPhase   (doubles)
//     136 h_khist[26]   162 h_mhist[26]   188 zero .. 192
//
// The checksum is FNV-1a, 64 bit (offset basis 0xcbf29ce484222325, prime 0x100000001b3), over every byte from offset 32 to the
// blob's end: each step is a bijection of the running value, so two blobs that differ in one byte never share a checksum.
// The bytes before it (magic, version, the two sizes, the zero word) are compared with their only valid values.
//
// The parser takes the bytes as untrusted: every length is checked against `bytes` before it is used, and the count is bounded
// before it is multiplied.  A checksum is easy to forge, so what a handle or a kernel would use as an INDEX is range-checked as
// well before anything is written (blob_parse: the flags, counters and phases of the shared block; blob_record_check: the bit-clock
// positions, the centre bin, a tuned stream's tuner indices and phases).  Everything else in a record is data to the kernels --
// energies, counters, register entries of any value are carried as they are and cannot make a kernel leave its buffers.
// No device, no HIP runtime call and no handle in here: tests/test_bpsk_blob_host.py drives this unit through a stand-alone program, plainly and under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace jsdr {
// (internal to the library: nothing here is part of what libjsdr_hip.so exports)
#pragma GCC visibility push(hidden)

enum {
    BLOB_VERSION = 1,
    BLOB_HEADER_BYTES = 192,
    BLOB_HIST = 26,         // input samples a record carries (SCHED_HIST)
    BLOB_HALO = 64,         // VCO-mixed samples
    BLOB_REG = 5200,        // FEC register entries (HIST_BITS)
    BLOB_MAX_COUNT = 65535  // streams a handle can have
};
constexpr double BLOB_TWO_PI = 2.0 * 3.14159265358979323846;  // what the tuner and the VCO wrap at (:385, :513)
constexpr double BLOB_TU_MAX = 4.0e7;                         // tuPhase x 256 / 2 pi stays inside an int (:389)
// offsets inside a record
enum {
    REC_TAIL_F64 = 0,       // 13 doubles
    REC_TAIL_I32 = 104,     // 10 ints
    REC_FEC_I32 = 144,      // 3 ints + zero
    REC_FFT_AVE = 160,      // 2 doubles
    REC_FFT_BIN = 176,      // int + zero
    REC_FFT_HIST = 192,     // 26 doubles
    REC_PST_F64 = 400,      // 3 doubles
    REC_PST_KH = 432,       // 26 u16
    REC_HIST = 496,         // 26 x 8 bytes
    REC_HALO = 704,         // 64 x 16 bytes
    REC_DECODED = 1728,     // 256 bytes
    REC_REG = 1984,         // 5200 bytes
    BLOB_RECORD_BYTES = 7184,
    REC_HEAD_BYTES = REC_HIST  // the part in front of the bulk arrays: small fields and the zero words between them
};
static_assert(REC_REG + BLOB_REG == BLOB_RECORD_BYTES && BLOB_RECORD_BYTES % 16 == 0 && BLOB_HEADER_BYTES % 16 == 0, "records are 16-byte aligned");
static_assert(REC_HIST % 16 == 0 && REC_HALO % 16 == 0 && REC_DECODED % 16 == 0 && REC_REG % 16 == 0, "bulk arrays are 16-byte aligned");

enum { BLOB_KIND_ORDINARY = 0, BLOB_KIND_TUNED = 1 };

// the shared block: what every stream of the handle has in common
struct BlobShared {
    uint32_t kind = 0, rate = 0, nsf = 0, do_fft = 0, do_up = 0, seam = 0, hist_float = 0, fft_state = 0;
    int32_t ds_cnt = 0;
    int64_t n_in = 0, n_ds = 0;
    double tuning = 0.0, tu_phase = 0.0, tu_inc = 0.0, vco_phase = 0.0;
    uint8_t khist[BLOB_HIST] = {0}, mhist[BLOB_HIST] = {0};
};
// bit for bit (doubles compared as their bit patterns).  fft_state is left out: it says whether the records' FFT-acquire fields
// were read from state the saving handle held or are the zeros of a handle that never acquired -- the same values either way
bool blob_shared_equal(const BlobShared &a, const BlobShared &b);

// One stream's record as a host struct, with blob_record_put / blob_record_get below: these three exist for the stand-alone
// driver (tests/tools/blob_driver.hip), which writes and reads patterned records through them.  They are NOT the library's
// path: the library's writer of a record is k_state_pack and its reader k_state_unpack (bpsk_state.hip), which state the same
// offsets (the REC_* above); the GPU tests -- the oracle continuation, the golden blob -- are what ties those to this layout.
struct BlobRecord {
    double tail_f64[13];
    int32_t tail_i32[10];
    int32_t fec_i32[3];
    double ave_peak_power, ave_centre_bin;
    int32_t centre_bin;
    double fft_hist[BLOB_HIST];
    double pst_f64[3];
    uint16_t pst_kh[BLOB_HIST];
    uint32_t hist[BLOB_HIST][2];
    double halo[BLOB_HALO][2];
    uint8_t decoded[256];
    int8_t reg[BLOB_REG];
};

// bytes of a blob of `count` streams; 0: count outside 1 .. BLOB_MAX_COUNT
size_t blob_bytes(uint32_t count);
// the header of a blob of `count` streams, from a zeroed image of its 192 bytes; the records behind it are not touched (each is
// written whole: by the device image's copy, or by blob_record_put).  false: cap too small or count out of range
bool blob_begin(void *blob, size_t cap, const BlobShared &sh, uint32_t count);
// where record i of a blob that blob_begin laid out, or blob_parse accepted, sits
inline unsigned char *blob_record(void *blob, uint32_t i) { return static_cast<unsigned char *>(blob) + BLOB_HEADER_BYTES + (size_t)i * BLOB_RECORD_BYTES; }
inline const unsigned char *blob_record(const void *blob, uint32_t i) { return static_cast<const unsigned char *>(blob) + BLOB_HEADER_BYTES + (size_t)i * BLOB_RECORD_BYTES; }
// (the driver's) field by field into / out of a record image (put: the image's other bytes are set to zero)
void blob_record_put(unsigned char *rec, const BlobRecord &r);
void blob_record_get(const unsigned char *rec, BlobRecord &r);
// one double at a byte offset of an image
void blob_put_f64(unsigned char *p, double v);
double blob_get_f64(const unsigned char *p);
// the checksum over the finished image: the last step of writing
void blob_seal(void *blob, size_t bytes);
uint64_t blob_fnv1a(const unsigned char *p, size_t n);

// Validates `bytes` bytes as a blob.  true: *sh and *count are its shared block and stream count, and records 0 .. count - 1 lie
// inside it.  false: `why` (if given) holds the reason as text.
bool blob_parse(const void *blob, size_t bytes, BlobShared *sh, uint32_t *count, char *why, size_t why_cap);
// the index-like fields of one record of a parsed blob (see above); false: `why` holds the reason
bool blob_record_check(const unsigned char *rec, const BlobShared &sh, char *why, size_t why_cap);

#pragma GCC visibility pop
}  // namespace jsdr
