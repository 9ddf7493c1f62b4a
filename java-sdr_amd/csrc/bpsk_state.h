// bpsk_state.h -- the checkpoint kernels (bpsk_state.hip) as the handle (bpsk_ckpt.hip) starts them: k_state_pack gathers the
// records of a range of streams from the handle's live buffers into one stream-major image (bpsk_blob.h's record layout),
// k_state_unpack scatters such an image back.  Every buffer choice -- which bit log and where the register starts in it, dm or
// dmh, which input history and tuner-index buffer -- is resolved by the handle and arrives here as a pointer and a stride.
#pragma once
#include "common.h"
#include "bpsk_kernels.h"

namespace jsdr {

struct StateArgs {
    unsigned char *img;        // [count][BLOB_RECORD_BYTES], 16-byte aligned
    int first, count;          // streams first .. first + count - 1 of the handle <-> records 0 .. count - 1
    TailState *tail;           // [S]
    signed char *bitlog;       // [S][bitlog_stride] the CURRENT log: the register is its row's bytes nbits_prev .. nbits_prev + 5199
    long long bitlog_stride;   // (a multiple of 16)
    int *nbits, *trig_count;   // [S] the last call's bits / FEC calls (unpack: zeroed, the restored streams report an empty call)
    int *fec_last, *cnt_dec;   // [S][2], [S]
    unsigned char *decoded;    // [S][256]
    int2 *hist;                // [S][32] the current input history
    double2 *halo;             // [S][halo_stride] the 64 VCO-mixed samples: dm's rows or the current dmh
    long long halo_stride;
    FftFrontState *fft;        // [S] or null: the handle holds no FFT-acquire state (pack: zeros in the record)
    double *pst_tu, *pst_inc;  // [S] or null: not a tuned handle
    unsigned short *pst_kh;    // [S][32] the current tuner-index history, or null
};

int launch_state_pack(const StateArgs &a, hipStream_t st);
int launch_state_unpack(const StateArgs &a, hipStream_t st);

}  // namespace jsdr
