// bpsk_acq_rule.h -- the scalar arithmetic of doBufferFFT (FUNcubeBPSKDemod.java:399-456) around its transforms, each stated
// once for the host and the device: the averaging factors, the searched band, the first-maximum search, the centre-bin rule
// and the first RxDownSample output of a frame.  Every FFT-acquire kernel (bpsk_fft.hip, bpsk_fftm.hip, bpsk_fft2x.hip, bpsk_acq.hip,
// bpsk_acq_chan.hip, bpsk_acqg.hip) steps them through these functions; tests/tools/acq_rule_driver.hip runs them on the host.
//
// No HIP call.  Every unit that includes this is compiled with -ffp-contract=off: each operation rounds by itself, as Java's do.
#pragma once
#include "common.h"

namespace jsdr {

// :399-402 -- float expressions widened to double
constexpr double ACQ_CFREQ_INV = (double)(1.0F - (2.0F / (1 + 1))), ACQ_CFREQ_AVG = (double)(2.0F / (1 + 1));
constexpr double ACQ_PSD_INV = (double)(1.0F - (2.0F / (10 + 1))), ACQ_PSD_AVG = (double)(2.0F / (10 + 1));
constexpr double ACQ_HOWARD = 0.9 * 32768.0;

// the quarter band of an n-sample frame that the boxcar searches (:433): bins [acq_band_beg, acq_band_end)
__host__ __device__ __forceinline__ int acq_band_beg(int n, int do_up) { return do_up ? n / 4 : 0; }
__host__ __device__ __forceinline__ int acq_band_end(int n, int do_up) { return do_up ? n / 2 : n / 4; }

// avePsd is cleared per frame (:431) and only [beg + 75, end - 75) is filled (:433): everywhere else it reads 0.0
__host__ __device__ __forceinline__ bool acq_band_filled(int i, int beg, int end) { return i >= beg + 75 && i < end - 75; }

// maxBin starts at 0.0 and binPos at -1; i ascends, and the strict '<' keeps the FIRST maximum (:439-442)
__host__ __device__ __forceinline__ void first_max_update(double &bestv, int &besti, double v, int i)
{
    if (bestv < v) {
        bestv = v;
        besti = i;
    }
}

// two partial searches into one: the larger value, then the smaller index; an empty candidate (index -1) never wins
__host__ __device__ __forceinline__ void first_max_merge(double &bestv, int &besti, double ov, int oi)
{
    if (oi >= 0 && (ov > bestv || (ov == bestv && (besti < 0 || oi < besti)))) {
        bestv = ov;
        besti = oi;
    }
}

// :444-445 -- the centre bin under which avePsd is read
__host__ __device__ __forceinline__ int centre_bin_clamp(int centreBin, int end)
{
    if (centreBin < 0) centreBin = 0;
    if (centreBin > end - 1) centreBin = end - 1;
    return centreBin;
}

// :446-456 -- atc = avePsd[centreBin] under the clamped centre bin; (maxBin, binPos) the frame's first maximum
__host__ __device__ __forceinline__ void centre_bin_step(double &avePeakPower, double &aveCentreBin, int &centreBin, double atc,
                                                         double maxBin, int binPos)
{
    avePeakPower = (ACQ_PSD_AVG * atc) + (ACQ_PSD_INV * avePeakPower);
    if (maxBin > (avePeakPower / 4) * 5 && binPos > 0) {
        aveCentreBin = (ACQ_CFREQ_AVG * (double)(float)binPos) + (ACQ_CFREQ_INV * aveCentreBin);
        centreBin = (int)(aveCentreBin + (double)1.0F);
    }
    if (centreBin < 102) centreBin = 102;
}

// the first RxDownSample output whose window ends in the frame that starts at t0 (call-relative): output j ends at first_out + D j
__host__ __device__ __forceinline__ long long ds_first_output(long long t0, long long first_out, int D)
{
    long long jlo = (t0 - first_out + D - 1) / D;
    if (t0 <= first_out) jlo = 0;
    return jlo;
}

}  // namespace jsdr
