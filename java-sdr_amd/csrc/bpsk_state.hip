// bpsk_state.hip -- the checkpoint kernels of a BPSK handle (jsdr_bpsk_save / jsdr_bpsk_restore): bpsk_blob.h's per-stream record
// gathered from, and scattered into, the buffers a handle keeps its streams' state in.
//
//   k_state_pack   : one workgroup per stream.  The record's head (the scalar fields and the zero words between them) is put
//                    together in LDS from a zeroed image and leaves in 16-byte stores; the input history, the matched filter's
//                    64 samples, decoded[] and the 5200-entry FEC register move as 16-byte loads and stores.  The register
//                    starts at byte nbits_prev of its row, at any byte: two aligned loads and a funnel shift per 16 bytes.
//   k_state_unpack : the way back.  The register goes to the head of the row of the CURRENT bit log with nbits_prev = 0,
//                    which is where the next call's tail -- k_tail and k_tail8 alike -- picks it up (old = row + nbits_prev),
//                    and where the sync kernels and both FEC forms then find it in the log that tail writes.  nbits and
//                    trig_count of the stream are zeroed: the restored stream reports an empty last call.  The fast variant's
//                    fields of TailState are set to their values at creation.
//
// The kernels hold no policy: which log, which history buffer, dm or dmh arrive as pointers (bpsk_state.h).  No arithmetic on
// data; compiled with -ffp-contract=off like its neighbours.  stream x stride products are 64-bit.
#include "bpsk_state.h"
#include "bpsk_blob.h"

namespace jsdr {

enum { STATE_THREADS = 256 };
static_assert(sizeof(TailState) == 176 && offsetof(TailState, peakPos) == 104, "the record's head follows TailState's first 13 doubles and its ints");
static_assert(sizeof(FftFrontState) == 24 + 8 * BLOB_HIST && sizeof(double2) == 16 && sizeof(int2) == 8, "element sizes of the record's arrays");

__device__ __forceinline__ double *tail_f64(TailState &t, int i)
{
    switch (i) {
        case 8: return &t.dmEnergyOut;
        case 9: return &t.lastI;
        case 10: return &t.lastQ;
        case 11: return &t.energy1;
        case 12: return &t.energy2;
        default: return &t.dmEnergy[i & 7];
    }
}

__global__ __launch_bounds__(STATE_THREADS) void k_state_pack(StateArgs a, int reg_max)
{
    __shared__ __align__(16) unsigned char head[REC_HEAD_BYTES];
    const int r = blockIdx.x, t = threadIdx.x;
    if (r >= a.count) return;
    const long long s = (long long)a.first + r;
    unsigned char *rec = a.img + (long long)r * BLOB_RECORD_BYTES;
    if (t < REC_HEAD_BYTES / 8) reinterpret_cast<unsigned long long *>(head)[t] = 0ull;
    __syncthreads();
    TailState &ts = a.tail[s];
    if (t < 13) reinterpret_cast<double *>(head + REC_TAIL_F64)[t] = *tail_f64(ts, t);
    if (t == 13) {
        int *q = reinterpret_cast<int *>(head + REC_TAIL_I32);
        q[0] = ts.peakPos;
        q[1] = ts.newPeak;
        q[2] = ts.dmCorr;
        q[3] = ts.dmMaxCorr;
        q[4] = ts.cntBit;
        q[5] = ts.cntFEC;
        q[6] = ts.cntDec;
        q[7] = ts.dmErrBits;
        q[8] = ts.decodeOK;
        q[9] = ts.overflow;
        int *f = reinterpret_cast<int *>(head + REC_FEC_I32);
        f[0] = a.fec_last[2 * s];
        f[1] = a.fec_last[2 * s + 1];
        f[2] = a.cnt_dec[s];
    }
    if (a.fft) {
        const FftFrontState &fs = a.fft[s];
        if (t >= 32 && t < 32 + BLOB_HIST) reinterpret_cast<double *>(head + REC_FFT_HIST)[t - 32] = fs.hist[t - 32];
        if (t == 32 + BLOB_HIST) {
            reinterpret_cast<double *>(head + REC_FFT_AVE)[0] = fs.avePeakPower;
            reinterpret_cast<double *>(head + REC_FFT_AVE)[1] = fs.aveCentreBin;
            reinterpret_cast<int *>(head + REC_FFT_BIN)[0] = fs.centreBin;
        }
    }
    if (a.pst_kh) {
        // (the stream's tuning is a host value: the handle sets it in the image)
        if (t >= 64 && t < 64 + BLOB_HIST) reinterpret_cast<unsigned short *>(head + REC_PST_KH)[t - 64] = a.pst_kh[s * 32 + (t - 64)];
        if (t == 64 + BLOB_HIST) {
            reinterpret_cast<double *>(head + REC_PST_F64)[1] = a.pst_tu[s];
            reinterpret_cast<double *>(head + REC_PST_F64)[2] = a.pst_inc[s];
        }
    }
    __syncthreads();
    if (t < REC_HEAD_BYTES / 16) reinterpret_cast<uint4 *>(rec)[t] = reinterpret_cast<const uint4 *>(head)[t];
    // the arrays, 16 bytes a lane
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.hist + s * 32);
        uint4 *dst = reinterpret_cast<uint4 *>(rec + REC_HIST);
        for (int i = t; i < BLOB_HIST * 8 / 16; i += STATE_THREADS) dst[i] = src[i];
    }
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.halo + s * a.halo_stride);
        uint4 *dst = reinterpret_cast<uint4 *>(rec + REC_HALO);
        for (int i = t; i < BLOB_HALO; i += STATE_THREADS) dst[i] = src[i];
    }
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.decoded + s * 256);
        uint4 *dst = reinterpret_cast<uint4 *>(rec + REC_DECODED);
        for (int i = t; i < 256 / 16; i += STATE_THREADS) dst[i] = src[i];
    }
    {
        // the register: bytes nprev .. nprev + 5199 of the row (the row is 16-byte aligned, nprev is not)
        int nprev = ts.nbits_prev;
        nprev = nprev < 0 ? 0 : (nprev > reg_max ? reg_max : nprev);  // (what the tail leaves is 0 .. max_bits: inside the row)
        const uint4 *row = reinterpret_cast<const uint4 *>(a.bitlog + s * a.bitlog_stride) + (nprev >> 4);
        const int sh0 = nprev & 15;
        uint4 *dst = reinterpret_cast<uint4 *>(rec + REC_REG);
        for (int i = t; i < BLOB_REG / 16; i += STATE_THREADS) {
            const uint4 lo4 = row[i], hi4 = row[i + 1];
            unsigned long long v0 = (unsigned long long)lo4.x | ((unsigned long long)lo4.y << 32), v1 = (unsigned long long)lo4.z | ((unsigned long long)lo4.w << 32);
            unsigned long long v2 = (unsigned long long)hi4.x | ((unsigned long long)hi4.y << 32), v3 = (unsigned long long)hi4.z | ((unsigned long long)hi4.w << 32);
            int sh = sh0;
            if (sh >= 8) {
                v0 = v1;
                v1 = v2;
                v2 = v3;
                sh -= 8;
            }
            const int b = 8 * sh;
            const unsigned long long lo = b ? (v0 >> b) | (v1 << (64 - b)) : v0, hi = b ? (v1 >> b) | (v2 << (64 - b)) : v1;
            dst[i] = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
        }
    }
}

__global__ __launch_bounds__(STATE_THREADS) void k_state_unpack(StateArgs a)
{
    __shared__ __align__(16) unsigned char head[REC_HEAD_BYTES];
    const int r = blockIdx.x, t = threadIdx.x;
    if (r >= a.count) return;
    const long long s = (long long)a.first + r;
    const unsigned char *rec = a.img + (long long)r * BLOB_RECORD_BYTES;
    if (t < REC_HEAD_BYTES / 16) reinterpret_cast<uint4 *>(head)[t] = reinterpret_cast<const uint4 *>(rec)[t];
    __syncthreads();
    TailState &ts = a.tail[s];
    if (t < 13) *tail_f64(ts, t) = reinterpret_cast<const double *>(head + REC_TAIL_F64)[t];
    if (t == 13) {
        const int *q = reinterpret_cast<const int *>(head + REC_TAIL_I32);
        ts.peakPos = q[0];
        ts.newPeak = q[1];
        ts.dmCorr = q[2];
        ts.dmMaxCorr = q[3];
        ts.cntBit = q[4];
        ts.cntFEC = q[5];
        ts.cntDec = q[6];
        ts.dmErrBits = q[7];
        ts.decodeOK = q[8];
        ts.overflow = q[9];
        ts.nbits_prev = 0;  // the register sits at the head of the current log's row
        ts.uncertified = 0;
        ts.emax = 0.0;
        ts.last_g = -1;
        ts.redone = 0;
        const int *f = reinterpret_cast<const int *>(head + REC_FEC_I32);
        a.fec_last[2 * s] = f[0];
        a.fec_last[2 * s + 1] = f[1];
        a.cnt_dec[s] = f[2];
        a.nbits[s] = 0;
        a.trig_count[s] = 0;
    }
    if (a.fft) {
        FftFrontState &fs = a.fft[s];
        if (t >= 32 && t < 32 + BLOB_HIST) fs.hist[t - 32] = reinterpret_cast<const double *>(head + REC_FFT_HIST)[t - 32];
        if (t == 32 + BLOB_HIST) {
            fs.avePeakPower = reinterpret_cast<const double *>(head + REC_FFT_AVE)[0];
            fs.aveCentreBin = reinterpret_cast<const double *>(head + REC_FFT_AVE)[1];
            fs.centreBin = reinterpret_cast<const int *>(head + REC_FFT_BIN)[0];
            fs.pad = 0;
        }
    }
    if (a.pst_kh) {
        if (t >= 64 && t < 64 + 32) a.pst_kh[s * 32 + (t - 64)] = t - 64 < BLOB_HIST ? reinterpret_cast<const unsigned short *>(head + REC_PST_KH)[t - 64] : (unsigned short)0;
        if (t == 64 + 32) {
            a.pst_tu[s] = reinterpret_cast<const double *>(head + REC_PST_F64)[1];
            a.pst_inc[s] = reinterpret_cast<const double *>(head + REC_PST_F64)[2];
        }
    }
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(rec + REC_HIST);
        uint4 *dst = reinterpret_cast<uint4 *>(a.hist + s * 32);
        for (int i = t; i < BLOB_HIST * 8 / 16; i += STATE_THREADS) dst[i] = src[i];
    }
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(rec + REC_HALO);
        uint4 *dst = reinterpret_cast<uint4 *>(a.halo + s * a.halo_stride);
        for (int i = t; i < BLOB_HALO; i += STATE_THREADS) dst[i] = src[i];
    }
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(rec + REC_DECODED);
        uint4 *dst = reinterpret_cast<uint4 *>(a.decoded + s * 256);
        for (int i = t; i < 256 / 16; i += STATE_THREADS) dst[i] = src[i];
    }
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(rec + REC_REG);
        uint4 *dst = reinterpret_cast<uint4 *>(a.bitlog + s * a.bitlog_stride);
        for (int i = t; i < BLOB_REG / 16; i += STATE_THREADS) dst[i] = src[i];
    }
}

static int state_check(const StateArgs &a)
{
    JSDR_REQUIRE(a.img && a.count > 0 && a.first >= 0 && a.tail && a.bitlog && a.hist && a.halo && a.decoded && a.fec_last && a.cnt_dec && a.nbits &&
                 a.trig_count, "bpsk state: null buffer");
    JSDR_REQUIRE((a.bitlog_stride & 15) == 0 && a.bitlog_stride >= BLOB_REG + 32 && a.halo_stride >= BLOB_HALO, "bpsk state: row strides %lld / %lld", a.bitlog_stride, a.halo_stride);
    return JSDR_OK;
}

int launch_state_pack(const StateArgs &a, hipStream_t st)
{
    if (state_check(a) != JSDR_OK) return JSDR_ERR;
    // the last 16-byte pair a register at nprev reads ends at byte 16 (nprev / 16) + 5200 + 31 of the row
    const int reg_max = (int)(a.bitlog_stride - BLOB_REG - 32);
    hipLaunchKernelGGL(k_state_pack, dim3((unsigned)a.count), dim3(STATE_THREADS), 0, st, a, reg_max);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

int launch_state_unpack(const StateArgs &a, hipStream_t st)
{
    if (state_check(a) != JSDR_OK) return JSDR_ERR;
    hipLaunchKernelGGL(k_state_unpack, dim3((unsigned)a.count), dim3(STATE_THREADS), 0, st, a);
    JSDR_LAUNCH_CHECK();
    return JSDR_OK;
}

}  // namespace jsdr
