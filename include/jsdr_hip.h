/*
 * jsdr_hip.h -- C ABI of libjsdr_hip.so: the MI355X (gfx950) implementation of java-sdr's
 * FFT / FIR / BPSK-demod hot path.
 *
 * This is the drop-in boundary.  java-sdr itself defines no native ABI (it is pure Java); each
 * entry point below replaces the arithmetic of one reference method and is what a JNI shim
 * for that class binds (INTEGRATION.md shows the stubs).  Citations are file:line in the
 * reference tree.
 *
 * Conventions:
 *   - every function returns JSDR_OK (0) or JSDR_ERR (-1)  (cf. FCD.OK/ERR, FCD.java:46-47);
 *     on error jsdr_last_error() returns a thread-local message.  Nothing throws or aborts.
 *   - handles are opaque; one handle is used by one thread at a time (the reference calls
 *     every handler from its single audio thread, JavaAudio.java:298-304).
 *   - "_host" buffers are caller-owned host memory, read/written before the call returns (the
 *     reference re-uses its frame buffers every iteration, JavaAudio.java:220-224).
 *   - "_dev" buffers are device (HBM) pointers valid on the current device; `stream` is a
 *     hipStream_t passed as void* (NULL = default stream); batch calls are asynchronous on it.
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails.
 */
#ifndef JSDR_HIP_H
#define JSDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JSDR_OK 0
#define JSDR_ERR (-1)

/* ------------------------------------------------------------------ runtime */
const char *jsdr_last_error(void);
int jsdr_version(void);                       /* ABI version, currently 1 */
int jsdr_device_count(int *count);
int jsdr_set_device(int device);
int jsdr_get_device(int *device);            /* the calling thread's current device (to restore after a per-device loop) */
int jsdr_device_name(char *buf, int cap);     /* gcnArchName of the current device */
int jsdr_malloc(void **dev, size_t bytes);
int jsdr_free(void *dev);
/* what the library's handles and calls hold at the moment, process-wide: device buffers and their bytes, pinned host buffers,
 * streams + events.  The caller's own jsdr_malloc / jsdr_stream_create are not counted; any pointer may be null.  Back at its
 * earlier value once every handle created since has been destroyed. */
int jsdr_live_resources(int64_t *device_buffers, int64_t *device_bytes, int64_t *pinned_buffers, int64_t *streams_and_events);
int jsdr_memset(void *dev, int value, size_t bytes);
int jsdr_memcpy_h2d(void *dev, const void *host, size_t bytes);
int jsdr_memcpy_d2h(void *host, const void *dev, size_t bytes);
/* a non-blocking HIP stream for the `stream` argument of the batch calls (independent handles on different streams
 * run concurrently: the HBM-bound PSD kernel beside the FP64-bound demodulator) */
int jsdr_stream_create(void **stream);
int jsdr_stream_destroy(void *stream);
int jsdr_stream_sync(void *stream);
/* HIP-event timing on `stream` (what bench.py brackets kernels with) */
int jsdr_timer_create(void **timer);
int jsdr_timer_destroy(void *timer);
int jsdr_timer_start(void *timer, void *stream);
int jsdr_timer_stop(void *timer, void *stream);
int jsdr_timer_elapsed_ms(void *timer, float *ms); /* synchronises on the stop event */

/* ------------------------------------------------------------------ sample conversion
 * JavaAudio.java:276-293: short s = LE16; s += (short)ic (wraps); f = (float)s/32767f; mono => Q=0.
 * Fused into every *_i16 kernel below; exposed on its own for parity tests.                */
int jsdr_convert_i16(const int16_t *raw_dev, int64_t nframes, int chns, int ic, int qc,
                     float *iq_dev, void *stream);

/* ------------------------------------------------------------------ fft.java
 * fft.receive (fft.java:190-228): complex forward FFT (replaces JTransforms FloatFFT_1D,
 * fft.java:194-195), psd[k]=10*log10((re^2+im^2)*(2/n)^2), first strict maximum, bin->Hz in
 * Java int arithmetic; output float[n+2] = what the reference publishes as "fft-psd".
 * n = blen/size (fft.java:67); supported: every n from 2 to 20 000.  Powers of two 64..8192 (2048 is the tuned size) and
 * the reference's default frames n = 4800 / 9600 / 19200 (blen = rate*size/10 at 48 / 96 / 192 kHz, JavaAudio.java:58-59)
 * have kernels of their own; jsdr_fft_kernel below names the one that serves a handle.  */
typedef struct jsdr_fft jsdr_fft;
int jsdr_fft_create(jsdr_fft **h, int n, int rate);
int jsdr_fft_destroy(jsdr_fft *h);
int jsdr_fft_receive_f32(jsdr_fft *h, const float *iq_host, float *psd_host);      /* IAudioHandler.receive(float[]) */
int jsdr_fft_receive_i16(jsdr_fft *h, const int16_t *raw_host, int ic, int qc,
                         float *psd_host);                                          /* IRawHandler.receive(byte[]) + a0 */
int jsdr_fft_batch_f32(jsdr_fft *h, const float *iq_dev, int64_t nframes, float *psd_dev, void *stream);
/* Running fft.receive and FUNcubeBPSKDemod.receive over the same batch SIDE BY SIDE (jsdr.java:476,482 feeds both from
 * one audio buffer): the PSD kernel is bound by memory latency, the demodulator's front-end kernel by FP64 issue, and
 * each, left alone, fills every CU -- launched on two streams they simply run one after the other.  With a share set on
 * both handles the batch kernels are launched as that many PERSISTENT workgroups per CU (0 = the default: all a CU takes):
 * jsdr_fft_set_cu_share(f, 2) + jsdr_bpsk_set_cu_share(h, 1) is the split that fits one CU's registers and LDS (2 x 128 +
 * 2 x 120 VGPRs per SIMD, 2 x 40 + 69.5 KB), both kernels resident from the start whichever stream gets there first.
 * Results are unchanged (bit for bit); measured on 8192 streams x 2^20 samples: 33.8 ms a step against 35.0 one after the
 * other (DESIGN.md "the step") -- and SLOWER than one after the other on batches of 4096 streams and below, and with the
 * fast variant: it is for the full-size batch of the exact variant.  A handle used on its own keeps the default. */
int jsdr_fft_set_cu_share(jsdr_fft *h, int wgs_per_cu);
/* diagnostics: what the handle's last power-of-two batch launch covered -- work items (groups of frames) and the
 * workgroups that strode over them.  workgroups < work_items means the persistent-stride path ran (the tests assert it). */
int jsdr_fft_last_launch(jsdr_fft *h, int64_t *work_items, int64_t *workgroups);
/* which kernel serves the handle's frame size: "k_fft" (powers of two 64 .. 8192), "k_fft_mixed" (9600 / 4800), "k_fft_mixed_dual"
 * (19200), "k_fft_rt" (any other composite frame up to 9800: 4410, 2205, 3200, 800, 1102 ...), "k_dft_any" (primes, and everything else up to 20 000) */
const char *jsdr_fft_kernel(jsdr_fft *h);
int jsdr_fft_batch_i16(jsdr_fft *h, const int16_t *raw_dev, int64_t nframes, int ic, int qc,
                       float *psd_dev, void *stream);
/* complex spectrum only (float2[n] per frame), for the 1e-5 FFT parity tests */
int jsdr_fft_spectrum_f32(jsdr_fft *h, const float *iq_dev, int64_t nframes, float *spec_dev, void *stream);
/* fft.receive + waterfall.paintLine in one call (fft.java:226 publishes "fft-psd", waterfall.java:28-47, 87-109 is its one
 * consumer): pixel rows straight from IQ frames, and no PSD array in caller memory.  Defined by composition, bit for bit:
 *   pix_dev row f  = what jsdr_waterfall_lines(psd, .., n, width, peak_rgb, ..) writes for the row psd that
 *                    jsdr_fft_batch_i16 / _f32 of this handle writes for frame f;
 *   max_dev[f][p]  = the pooled maximum itself, unrotated: getMax(psd, (int)(p*step), (int)step) as fft.paintComponent
 *                    takes it (fft.java:147); with width == n the PSD row without its two trailing floats;
 *   peak_dev[f]    = {psd[n], psd[n+1]}: Hz of the first strict maximum and its value (fft.java:138-140 prints them).
 * Powers of two 64 .. 8192 run one fused kernel, "k_fft_pix": the batch kernel's frame loop, whose last pass leaves the dB
 * row in the frame's LDS image, where the frame's own threads pool it.  Every other frame size runs the handle's batch kernel
 * into PSD rows owned by the handle (at most 1024 frames at a time, allocated at the first such call, counted by
 * jsdr_live_resources), then k_waterfall: "<kernel>+k_waterfall".  Asynchronous on `stream`; calls on one handle share
 * those rows, so they belong on one stream at a time.  jsdr_fft_set_cu_share and jsdr_fft_last_launch apply to the fused
 * kernel as to the batch kernel.  JSDR_ERR before any device work, the message naming the argument: a null handle, input
 * or pix_dev; width <= 0; nframes < 0.  nframes == 0 is JSDR_OK and launches nothing. */
int jsdr_fft_waterfall_i16(jsdr_fft *h, const int16_t *raw_dev, int64_t nframes, int ic, int qc,
                           int width, uint32_t peak_rgb,
                           uint32_t *pix_dev   /* [nframes][width], required                       */,
                           float    *max_dev   /* [nframes][width], may be NULL                    */,
                           float    *peak_dev  /* [nframes][2] = {Hz, max dB}, may be NULL         */,
                           void *stream);
int jsdr_fft_waterfall_f32(jsdr_fft *h, const float *iq_dev, int64_t nframes, int width, uint32_t peak_rgb,
                           uint32_t *pix_dev, float *max_dev, float *peak_dev, void *stream);
const char *jsdr_fft_waterfall_kernel(jsdr_fft *h);   /* what the last waterfall call launched */
/* The batch and the waterfall calls over raw[stream][stride], as every other batch entry point takes its IQ: one launch
 * where rows longer than a call (a ring per stream, the chunked calls of a longer capture, a 2 * max_batch stride) took one
 * launch a stream.
 *   frame j of stream s   starts at element s * stream_stride + j * 2n of the input (int16 / float values);
 *   its PSD row           is at psd_dev + s * psd_stream_stride_f32 + j * (n + 2); psd_stream_stride_f32 == 0 means packed,
 *                         frames_per_stream * (n + 2);
 *   the waterfall outputs are packed: row s * frames_per_stream + j of pix_dev, max_dev and peak_dev, each
 *                         [nstreams * frames_per_stream][...] as in jsdr_fft_waterfall_*.
 * Defined by composition, bit for bit: what stream s receives equals what jsdr_fft_batch_i16(h, raw_dev + s * stream_stride,
 * frames_per_stream, ic, qc, psd_dev + s * psd_stride, stream) writes, likewise _f32 and jsdr_fft_waterfall_* with that
 * stream's block of rows.  Input outside the frames is not read into any result; output between a stream's last row and the
 * next stream's first is not written.  Every frame size jsdr_fft_create accepts is served by a strided instantiation of the
 * handle's own kernel (jsdr_fft_kernel / jsdr_fft_waterfall_kernel name it as before; the fallback's chunks of 1024 rows run
 * across stream boundaries); a frame's (stream, frame) pair is found once per frame -- one division when a workgroup starts,
 * additions from there on.  jsdr_fft_set_cu_share and jsdr_fft_last_launch apply as to the batch kernel.  A call whose rows
 * are in fact packed -- stream_stride == frames_per_stream * 2n and a packed PSD stride, or nstreams == 1 -- IS the contiguous
 * call of nstreams * frames_per_stream frames: the same launch of the same kernel.  Asynchronous on `stream`.
 * JSDR_ERR before any device work, the message naming the argument: a null handle, input or required output (psd_dev,
 * pix_dev); nstreams <= 0; frames_per_stream < 0; with nstreams > 1 an input stride that is odd or below
 * frames_per_stream * 2n; a non-zero PSD stride below frames_per_stream * (n + 2); width <= 0.  frames_per_stream == 0 is
 * JSDR_OK and launches nothing.  (Not covered: the JNI shim and the Java classes, jsdr_fft_spectrum_f32, jsdr_harness.) */
int jsdr_fft_batch_streams_i16(jsdr_fft *h, const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16,
                               int64_t frames_per_stream, int ic, int qc,
                               float *psd_dev, int64_t psd_stream_stride_f32, void *stream);
int jsdr_fft_batch_streams_f32(jsdr_fft *h, const float *iq_dev, int nstreams, int64_t stream_stride_f32,
                               int64_t frames_per_stream, float *psd_dev, int64_t psd_stream_stride_f32, void *stream);
int jsdr_fft_waterfall_streams_i16(jsdr_fft *h, const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16,
                                   int64_t frames_per_stream, int ic, int qc, int width, uint32_t peak_rgb,
                                   uint32_t *pix_dev, float *max_dev, float *peak_dev, void *stream);
int jsdr_fft_waterfall_streams_f32(jsdr_fft *h, const float *iq_dev, int nstreams, int64_t stream_stride_f32,
                                   int64_t frames_per_stream, int width, uint32_t peak_rgb,
                                   uint32_t *pix_dev, float *max_dev, float *peak_dev, void *stream);

/* ------------------------------------------------------------------ phase.java
 * phase.java:75-80 max|x| over the 2n floats of a frame; :93-116 per-pixel-column means of I and Q
 * for a panel `bx` pixels wide.  cols_dev = int32[ncol_cap] pixel indices, avg*_dev float[ncol_cap].  */
int jsdr_phase_maxabs(const float *iq_dev, int64_t nframes, int n, float *max_dev, void *stream);
int jsdr_phase_columns(const float *iq_dev, int n, int bx, int32_t *pix_host, float *avgi_host,
                       float *avgq_host, int cap, int *ncol);
/* the IAudioHandler drop-in for phase.java: receive() copies the frame (phase.java:123-128) to the device and takes
 * max|x| at once; the painter asks for `max` (:75-80) and, for its panel width, the column means (:93-116). */
typedef struct jsdr_phase jsdr_phase;
int jsdr_phase_create(jsdr_phase **h, int n);
int jsdr_phase_destroy(jsdr_phase *h);
int jsdr_phase_receive_f32(jsdr_phase *h, const float *iq_host);   /* 2n floats */
int jsdr_phase_get_max(jsdr_phase *h, float *max_out);
int jsdr_phase_get_columns(jsdr_phase *h, int bx, int32_t *pix_host, float *avgi_host, float *avgq_host, int cap,
                           int *ncol);
/* The phase scope over batches: everything phase.paintComponent computes from a frame (phase.java:75-116), for every frame of
 * raw[stream][stride], in one launch that reads each frame once.  For a frame dpy[2n] and a strip bx pixels wide:
 *   max_dev[r]          = max|x| as :75-80 takes it: from -1, `max < a` never admits a NaN (an all-NaN frame gives -1);
 *   the column schedule = step = (float)(bx*2)/(float)(2n); `pos += step` in float; a column closes at the sample where
 *                         (int)pos > lpix (:81, 84, 93-99, 110-114).  It depends on (n, bx) alone -- jsdr_phase_layout states it
 *                         on the host: pix (the closing (int)pos), first sample and sample count of every closed column.  It is the
 *                         float recurrence, not floor((s+1)*bx/n): (600, 1) closes no column.  Samples behind the last closed
 *                         column belong to none;
 *   avg_dev[r][c]       = {avgi, avgq}: float sums in sample order divided by (float)count -- jsdr_phase_columns' values;
 *   pts_dev[r][c]       = {(int)(avgi*hiq), (int)(avgq*hiq), (int)(dpy[2e]*hph), (int)(dpy[2e+1]*hph)}, e the column's closing
 *                         sample, hiq = (float)quarter_height/max, hph = (float)half_size/max (:85-86, 102, 107, 109) with
 *                         quarter_height = getHeight()/4 and half_size = size/2; (int) is Java's cast (truncates, saturates,
 *                         NaN -> 0).  The pixel offsets around these values stay with the caller; a column's lsti / lstq is the
 *                         entry before it, 0 in front of the first.
 * int16 samples are taken as jsdr_convert_i16 takes them (wrapping s += (short)ic, then (float)s/32767f).  Bit-exact throughout.
 * Geometry: n is the handle's; rows = nstreams * frames_per_stream; frame j of stream s starts at element s * stream_stride +
 * j * 2n of the input; the outputs are packed, row s * frames_per_stream + j, ncol entries a row (ncol from jsdr_phase_layout).
 * bx == 0, or any (n, bx) that closes no column: only max_dev is written (the batched int16 maxabs).  avg_dev and pts_dev may each
 * be NULL.  The input starts on an IQ pair (4 / 8 bytes); max_dev, avg_dev and pts_dev on a row entry (4 / 8 / 16 bytes).
 * Frames up to 8192 samples run "k_phase_scope" (the converted frame in LDS), larger ones "k_phase_scope_g" (the columns read the
 * samples again, from cache); jsdr_phase_scope_kernel names what the last call launched.
 * Asynchronous on `stream`.  The first scope call on a handle allocates the schedule table (n columns, counted by
 * jsdr_live_resources, gone with jsdr_phase_destroy; jsdr_phase_create allocates nothing for it); no later call allocates or
 * waits for the device, a change of bx included: the table is rebuilt by a one-thread kernel on `stream`, behind the previous
 * call's readers.  Scope calls on one handle share that table, so they belong on one stream at a time.
 * JSDR_ERR before any device work, the message naming the argument: a null handle, input or max_dev; nstreams <= 0;
 * frames_per_stream < 0; rows >= 2^31; bx < 0; with nstreams > 1 a stride that is odd or below frames_per_stream * 2n; a
 * misaligned pointer.  frames_per_stream == 0 is JSDR_OK and launches nothing.
 * (Not covered: the JNI shim and the Java classes, jsdr_harness, jsdr_group_*, strided outputs.) */
/* host only, no device: the schedule of (n, bx).  pix / first / count may each be NULL; *ncol is always set */
int jsdr_phase_layout(int n, int bx, int32_t *pix_host, int32_t *first_host, int32_t *count_host, int cap, int *ncol);
int jsdr_phase_scope_i16(jsdr_phase *h, const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16,
                         int64_t frames_per_stream, int ic, int qc, int bx, int half_size, int quarter_height,
                         float   *max_dev   /* [rows], required                                              */,
                         float   *avg_dev   /* [rows][ncol][2] = {avgi, avgq}, may be NULL                   */,
                         int32_t *pts_dev   /* [rows][ncol][4] = {line_i, line_q, dot_i, dot_q}, may be NULL */,
                         void *stream);
int jsdr_phase_scope_f32(jsdr_phase *h, const float *iq_dev, int nstreams, int64_t stream_stride_f32,
                         int64_t frames_per_stream, int bx, int half_size, int quarter_height,
                         float *max_dev, float *avg_dev, int32_t *pts_dev, void *stream);
const char *jsdr_phase_scope_kernel(jsdr_phase *h);   /* what the last scope call launched */

/* ------------------------------------------------------------------ fir.java
 * weights (fir.java:169-195) is setup arithmetic (host); filter (:198-211) runs on the GPU over a
 * block of samples with carried delay line; complex_gen/complex_mod (:214-228) likewise.      */
typedef struct jsdr_fir jsdr_fir;
int jsdr_fir_create(jsdr_fir **h, float sample_rate);
int jsdr_fir_destroy(jsdr_fir *h);
int jsdr_fir_weights(jsdr_fir *h, int f1, int f2, double w_out[21]);
int jsdr_fir_filter(jsdr_fir *h, const int32_t *in_host, int32_t *out_host, int64_t n);
int jsdr_fir_complex_gen(jsdr_fir *h, int freq, int start, int32_t *sig_host /*[n][2]*/, int64_t n);
int jsdr_fir_complex_mod(jsdr_fir *h, const int32_t *a_host, const int32_t *b_host, int32_t *out_host, int64_t n);
/* batched complex FIR + decimate over device-resident int16 IQ streams (BASELINE config 3), exact-order FP64:
 *   out[s][j] = scale * SUM_{a<ntaps} x[s][decim*(j+1)-1-a] * taps[a]   per rail, newest sample first, every product
 *   and sum rounded separately; x = (double)((float)int16/32767f); samples before the batch are zero (cleared delay
 *   line).  = RxDownSample (FUNcubeBPSKDemod.java:466-492) for taps = dsFilter, decim = rate/9600, scale = 0.9*32768;
 *   any ntaps <= 128 and decim >= 1 (27/65/21 taps x decimation 1/10/20 have register-blocked kernels).
 * out_dev: double[nstreams][out_stride_pairs][2]; *nout = nsamples / decim outputs per stream.  Asynchronous. */
int jsdr_fir_batch_decimate_i16(const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16, int64_t nsamples,
                                const double *taps_host, int ntaps, int decim, double scale, double *out_dev,
                                int64_t out_stride_pairs, int64_t *nout, void *stream);

/* ------------------------------------------------------------------ FECDecoder.java
 * FECDecode (FECDecoder.java:703-852): 5200 soft symbols -> 256 bytes, return -1 or channel errors.
 * encode_FEC40 (:677-688) is the (private) re-encoder, exposed for test-vector generation.     */
int jsdr_fec_decode(const uint8_t raw_host[5200], uint8_t out_host[256], int *rc);
int jsdr_fec_encode(const uint8_t data_host[256], uint8_t sym_host[5200]);
int jsdr_fec_decode_batch(const uint8_t *raw_dev, int64_t nblocks, uint8_t *out_dev, int32_t *rc_dev, void *stream);
int jsdr_fec_encode_batch(const uint8_t *data_dev, int64_t nblocks, uint8_t *sym_dev, void *stream);

/* ------------------------------------------------------------------ FUNcubeBPSKDemod.java
 * One handle = `nstreams` independent demodulators with identical configuration that advance in
 * lock-step (stream-major batches).  nstreams=1 + receive_* is the IAudioHandler drop-in.
 *   rate, blen/size : AudioDescriptor (FUNcubeBPSKDemod.java:193-194)
 *   tuning_hz       : "bpsk-tuning" (:195), do_fft "bpsk-dofft" (:199), do_up "bpsk-upper" (:200)
 * Frames: tune mode takes any frame; FFT-acquire mode (do_fft) frames of 1024 / 2048 / 4096 / 8192 samples, any other
 * n = 2^a 3^b 5^c 7^d from 1025 to 9600 (java-sdr's defaults 9600 / 4800 at 96 / 48 kHz, 4410 at 44.1 kHz, 3200 at 32 kHz)
 * and twice a 2^a 3^b 5^c frame that is a multiple of 16 (19200, the 192 kHz default) through kernels that hold the frame
 * in LDS; every other frame of 416 .. 4194304 samples (and power-of-two / 2 m frames below 38400 Hz) through passes in
 * global memory -- the same results, about ten times the time per sample.  Below 416 samples: refused (the reference's
 * arraycopy of 204 bins, :458, would run off the frame).
 * max_batch_samples bounds one batch call; the per-call result log holds max_batch/40 + 16 bits and
 * max(8, bits/2600 + 4) FECDecode calls per stream -- a call that exceeds either flags the stream (getters fail).  */
typedef struct jsdr_bpsk jsdr_bpsk;
int jsdr_bpsk_create(jsdr_bpsk **h, int rate, int nsamples_per_frame, int tuning_hz, int do_fft,
                     int do_up, int nstreams, int64_t max_batch_samples);
int jsdr_bpsk_destroy(jsdr_bpsk *h);
/* the constant tables as the library holds them (host side): which = 0 dsFilter[27] (:27-55), 1 dmFilter[65] (:58-77),
 * 2 SYNC_VECTOR[65] (:79-81) as +1/-1, 3 cosTab[256] and 4 sinTab[256] (:159-162) of the tuner and the VCO */
int jsdr_bpsk_table(int which, double *out, int cap);
/* arithmetic of the demodulator (before the first sample): EXACT = every double product and sum rounded separately in
 * the reference's order (bits, bytes AND doubles identical to the Java arithmetic); FAST = fused multiply-adds in the
 * two FIR stages, every slicer decision certified by a proven error margin or recomputed in exact order (bits and
 * bytes identical, doubles within 1e-12 relative).                                                          */
enum { JSDR_VARIANT_EXACT = 0, JSDR_VARIANT_FAST = 1 };
int jsdr_bpsk_set_variant(jsdr_bpsk *h, int variant);
/* FAST: decisions recomputed in exact order so far (all streams), streams that could not be certified (their getters
 * fail), and the bound on |fi' - fi|, |fq' - fq| the margins are built on.  In FAST mode the input buffer of a batch
 * call must stay unmodified until the next jsdr_bpsk_sync() / getter: the certification pass may re-read it. */
int jsdr_bpsk_cert_stats(jsdr_bpsk *h, int64_t *redone, int64_t *uncertified_streams, double *ey);
/* FAST, the contract for a drop-in: a stream whose 8-way energy argmax (FUNcubeBPSKDemod.java:586-592) falls inside the
 * error margin cannot be decided without the exact IIR history and is marked UNCERTIFIED by the call in which that
 * happens.  The mark is sticky: from that call on every getter of that stream (counters, bits, fec, decoded, trace,
 * state), the snapshot and receive_*() of a 1-stream handle return JSDR_ERR with a message that says so, and the
 * result slot's header[12] is 1 -- a wrong bit is never delivered, and neither is a silent gap.  Measured rate on the
 * benchmark's streams: about 1 stream in 8192 per 1.4e9 bit periods; a stream that carried signal and then
 * goes silent for ~5 s also ends here (its energies decay below the margin, which scales with the largest sample seen).
 * What the caller does: jsdr_bpsk_uncertified_streams() lists the stream ids after a call (count > 0 <=> some results
 * of that call were withheld); those streams are re-run on a JSDR_VARIANT_EXACT handle -- from the start of the stream,
 * or from the flagged call on an exact handle that was fed the same earlier input -- which decides the same near-tie by
 * the reference's own arithmetic (tests/test_gpu_fixtures.py::test_fast_variant_uncertified_streams_are_listed_and_
 * recovered_on_an_exact_handle).  There is no automatic fallback: it would need the exact state kept beside the fast
 * one for every stream, i.e. the exact variant's cost.  ids: ascending, at most cap; *count: all of them. */
int jsdr_bpsk_uncertified_streams(jsdr_bpsk *h, int32_t *ids, int cap, int *count);
/* Fast variant, batch use over retained input (round 6): REPLAYS every stream the calls so far left uncertified, from the
 * handle's first call, on an internal exact handle that serves those streams from then on -- their getters, their packed
 * slots; the flag no longer withholds them; jsdr_bpsk_uncertified_streams / _cert_stats stop counting them; every later
 * batch call advances the exact shadow in lock-step.  raw_dev_calls[k] / nsamples_calls[k]: the device pointer and sample
 * count jsdr_bpsk_batch_i16 was given at call k, ALL calls since creation (checked against the handle's own counts), the
 * buffers still holding those samples; ic / qc as in those calls.  *recovered = streams now served in exact order (0: none
 * was uncertified).  Cost: one small exact handle's call per call replayed.  Mirrors what a caller of
 * FUNcubeBPSKDemod.receive would do with a recording: run the doubtful streams again in the reference's own arithmetic
 * (FUNcubeBPSKDemod.java:533-594). */
int jsdr_bpsk_stream_recovered(jsdr_bpsk *h, int stream, int *recovered); /* 1: served by the exact shadow (replayed) */
int jsdr_bpsk_recover_uncertified(jsdr_bpsk *h, const int16_t *const *raw_dev_calls, const int64_t *nsamples_calls, int ncalls,
                                  int64_t stream_stride_i16, int ic, int qc, int *recovered, void *stream);
/* Live control: FUNcubeBPSKDemod.actionPerformed (:165-190) between two calls, applied to every stream of the handle.
 * Takes effect from the next sample of the next call; nothing else is reset (tuPhase, the down-sampler and matched-filter
 * histories, vcoPhase, the bit clock and energies, the 5200-bit FEC register and the counters carry on).  Both calls wait
 * for the handle's own pending work first: the previous call's tail and FEC finish with the settings they started with.
 *   set_tuning: tuning = tuning_hz; tuPhaseInc = 2 pi tuning / rate; dmMaxCorr = 0.  Any finite value: tuning <= 0 follows
 *     :388-396 (samples pass through unmixed once tuPhase <= 0; tuning == 0 freezes tuPhase).
 *   set_mode: doFFT = do_fft, doUp = do_up; tuPhaseInc recomputed; dmMaxCorr = 0.  A switch between the tune and the
 *     FFT-acquire front end keeps the down-sampler history across it exactly (the first call after it carries the seam; calls
 *     in FFT-acquire mode must be whole frames, and the first tune call after FFT-acquire frames at least 26 samples).  The
 *     FFT-acquire buffers of a handle created in the tune mode are allocated, zeroed, at its first switch.
 *   Calling either with the current values still zeroes dmMaxCorr, as the Java does.
 * JSDR_ERR, with the handle exactly as it was, for a null handle, a non-finite tuning, set_mode(do_fft = 1) on a frame size
 * FFT-acquire mode cannot take or when its buffers cannot be allocated (jsdr_last_error says which), and on a
 * JSDR_VARIANT_FAST handle (jsdr_bpsk_recover_uncertified replays from creation and would replay the wrong tuning; a
 * handle that has been retuned cannot become FAST either).  get_control: the values now in effect. */
int jsdr_bpsk_set_tuning(jsdr_bpsk *h, double tuning_hz);
int jsdr_bpsk_set_mode(jsdr_bpsk *h, int do_fft, int do_up);
int jsdr_bpsk_get_control(jsdr_bpsk *h, double *tuning_hz, int *do_fft, int *do_up);
/* FUNcubeBPSKDemod.setup (:192-209) on an unchanged AudioDescriptor: tuning, doFFT, doUp and tuPhaseInc from the
 * configuration, dmMaxCorr left as it is (setup resets no DSP state); otherwise as set_tuning + set_mode */
int jsdr_bpsk_reconfigure(jsdr_bpsk *h, double tuning_hz, int do_fft, int do_up);
/* Channel handle: jsdr.java's nfcs FUNcubeBPSKDemod tabs (:479-483, each "FUNcube<idx>" with its own bpsk-tuning / -upper,
 * FUNcubeBPSKDemod.java:129,195-200) fed the same audio.  One handle of ninputs x nchannels demodulators in the tune mode
 * (doBufferTune, :366-397); channel c of input i is stream i * nchannels + c, so every per-stream getter, pack_slots and
 * the slot layout apply unchanged.  Every channel has its own tuning (tuning_hz[c], any finite value; <= 0: pass-through
 * per :388-396) and doUp (do_up[c], may be NULL: 0; stored and reported, no effect in the tune mode).  1 <= nchannels <= 16.
 * Each input is read from memory once for all its channels.  Results are bit-identical to nchannels independent
 * demodulators created with those tunings and fed the same input.
 *   jsdr_bpsk_batch_i16: stream_stride_i16 is the stride between INPUTS (>= 2 nsamples when ninputs > 1).
 *   receive_i16 / receive_f32 on a 1-input handle feed the frame to every channel.  receive_f32 takes the frames JavaAudio
 *     produces ((float)s/32767f values, run through the int16 kernels) and refuses any other float with JSDR_ERR.
 *   set_channel_tuning: actionPerformed's tuning change (:177-189) on the streams of that channel on every input: tuning,
 *     tuPhaseInc = 2 pi tuning / rate, dmMaxCorr = 0; everything else carries on, the other channels are not touched.
 *   set_channel_mode: do_fft must be 0; do_up stored; dmMaxCorr = 0 on that channel.  set_tuning / set_mode / reconfigure
 *     apply to every channel; get_control reports channel 0.
 *   channel_info: an ordinary handle reports nstreams x 1 (and takes channel 0 in the per-channel calls).
 * JSDR_ERR, the handle unchanged: do_fft = 1 in set_mode / set_channel_mode / reconfigure, set_variant(FAST), snapshot_read
 * when nchannels > 1, a channel out of range, a non-finite tuning; float input through receive_f32 other than JavaAudio's values (jsdr_bpsk_batch_f32 takes any float,
 * its stride between INPUTS as batch_i16's).  Not covered on this
 * handle: FFT-acquire channels (jsdr_bpsk_create_mode_channels below has them; jsdr_bpsk_create_live_channels switches a
 * channel between the modes live), the FAST variant, jsdr_group, JNI / Java classes, a per-channel snapshot. */
int jsdr_bpsk_create_channels(jsdr_bpsk **h, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                              const double *tuning_hz, const int *do_up, int64_t max_batch_samples);
/* Channel handle whose channels are each in the tune mode or in FFT-acquire ("FFT/Tune", FUNcubeBPSKDemod.java:180-186),
 * fixed at creation: do_fft[c] (may be NULL: every channel in the tune mode), each FFT-acquire channel searching its own
 * half of the band, do_up[c] ("Track high", :183-189).  Streams, getters, pack_slots, the slot layout, receive_* and the
 * per-channel calls are jsdr_bpsk_create_channels'; handles from that creator keep every refusal they have.
 *   Tune-mode channels behave exactly as there.  FFT-acquire channels follow doBufferFFT (:406-464): the tuner never
 *     runs (tuPhase stands still, tuning is stored and reported), state doubles 6 / 7 (avePeakPower, aveCentreBin) and
 *     counter centreBin are live for their streams and 0 for the others.  Results are bit-identical to an ordinary handle
 *     created with that (tuning, do_fft, do_up) and fed the same calls.
 *   The forward half of doBufferFFT (conversion, forward transform, |X|; :416-427) runs once per INPUT and frame, whatever
 *     the number of FFT-acquire channels: frames of 1024 .. 8192 samples (2^k) in one transform that serves both bands,
 *     every other frame once per band in use (at most twice).  A handle whose FFT-acquire channels all search one band
 *     pays nothing for the other.  jsdr_bpsk_acq_last_launch: the frames transformed forward and the frames inverted by
 *     the last call (inverted: inputs x FFT-acquire channels x frames).
 *   With at least one FFT-acquire channel every call is whole frames, and the frame must be one FFT-acquire takes (416
 *     samples and more).  Frames other than 2^k of 1024 .. 8192 and 9600 / 4800 / 4410 -- 19200 among them, and the other
 *     frames an ordinary handle runs through its fused kernels -- take the any-frame passes.
 *   set_channel_mode(c, do_fft, do_up): do_fft must equal the channel's creation mode; do_up on an FFT-acquire channel is
 *     "Track high": the band changes from the next call, centreBin, avePeakPower, aveCentreBin and everything else carry
 *     on, dmMaxCorr = 0 on that channel (also when do_up is the current value), other channels untouched.  set_mode /
 *     reconfigure take a do_fft that changes no channel's mode (so none at all on a handle with both kinds).
 * JSDR_ERR, the handle unchanged: a change of a channel's do_fft by any route, a call that is not whole frames,
 * set_variant(FAST), snapshot_read when nchannels > 1, a channel out of range, a non-finite tuning -- all checked before
 * any device work.  Not covered on this handle: switching a channel between the modes live (jsdr_bpsk_create_live_channels
 * below has it), the FAST variant, jsdr_group, JNI / Java classes, a per-channel snapshot. */
int jsdr_bpsk_create_mode_channels(jsdr_bpsk **h, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                                   const double *tuning_hz, const int *do_fft, const int *do_up, int64_t max_batch_samples);
/* Channel handle whose channels switch between the tune mode and FFT-acquire LIVE: every "FUNcube<idx>" tab's own "FFT/Tune"
 * button (FUNcubeBPSKDemod.actionPerformed, :165-190), which works while audio runs.  Arguments, stream numbering
 * (i * nchannels + c), getters, pack_slots, the slot layout, receive_*, batch_i16 / batch_f32 and the per-channel calls are
 * jsdr_bpsk_create_mode_channels'; do_fft[c] / do_up[c] are the INITIAL modes.  Handles from the two older creators behave
 * exactly as before, every refusal and message included.  What differs here:
 *   The frame must be one FFT-acquire takes (416 samples and more), whatever the initial modes.
 *   Everything a switch needs per channel and stream is allocated and zeroed at creation, for every channel (the FFT state
 *     rows, the seam's copies, the tuner state of channels that start in FFT-acquire): a switch allocates nothing per stream.
 *     The per-input three-phase scratch is cut for the bands in use; an action that changes them ("FFT/Tune", "Track high")
 *     cuts it again, and is refused with the handle unchanged if that cannot be had.
 *   set_channel_mode(c, do_fft, do_up) with a do_fft other than the channel's current one is that tab's "FFT/Tune" action:
 *     doFFT changes, tuPhaseInc is recomputed, dmMaxCorr = 0 on that channel's streams, nothing else is reset and no other
 *     channel is touched.  While a channel acquires its tuPhase stands still and carries on from there when it returns to
 *     the tune mode.  set_mode / reconfigure apply to every channel, each switching or not by its own current mode.  The action
 *     takes effect from the next call, whose streams of that channel carry the seam, on every input: the down-sampler history
 *     crosses it exactly, in both directions (tune -> FFT-acquire: the tune path's I and Q columns; FFT-acquire -> tune: the
 *     FFT path's doubles).  Several channels may carry a seam in one call, in different directions.  A switch that is switched
 *     back before any call cancels the seam; each action still zeroes dmMaxCorr.
 *   A call is whole frames whenever at least one channel is in FFT-acquire for it (a channel that just switched to it
 *     included); a call in which a channel carries the FFT-acquire -> tune seam needs at least 26 samples.
 *   Results: stream (i, c) is bit-identical to an ordinary handle created with channel c's initial (tuning, do_fft, do_up),
 *     fed input i in the same calls and given jsdr_bpsk_set_mode / jsdr_bpsk_set_tuning at the same points -- bits, FEC rc /
 *     bit index / bytes, the ten counters, the 18 state doubles and the (fi, fq) trace, through both seams, int16 and float input.
 *   A call that carries no seam launches exactly what a jsdr_bpsk_create_mode_channels handle of the current configuration
 *     launches; jsdr_bpsk_front_kernel and jsdr_bpsk_acq_last_launch mean what they mean there.  On a seam call
 *     jsdr_bpsk_acq_last_launch counts the same frames as a steady call of the new configuration: the tune -> FFT-acquire seam
 *     re-runs no frame (it forms the Q rail of the few outputs that reach into the tune path's history from the Q column, in
 *     one small kernel behind the channel's edges), and the FFT-acquire -> tune seam is a tune-mode front end
 *     (jsdr_bpsk_front_kernel: "k_front_split" when no other front end ran in the call).
 *   After "Track high" on a channel that has run FFT-acquire frames in the other band, that channel's frames go through the
 *     ordinary handle's one-kernel front end until a frame's peak has moved its centre bin into the new band (the bins around
 *     the carried one are not in the three-phase rows of one band); such a call waits for that kernel, and
 *     jsdr_bpsk_acq_last_launch counts the three-phase launches alone (a tune -> FFT-acquire seam in such a call runs the
 *     channel's first frame twice, as the ordinary handle's does).  Frames only the any-frame passes take keep the
 *     three-phase launches and their rows.
 * JSDR_ERR, the handle and its pending seams unchanged, each checked before any device work: a frame FFT-acquire cannot take,
 * a call that is not whole frames where it must be, fewer than 26 samples with a pending FFT-acquire -> tune seam,
 * set_variant(FAST), snapshot_read when nchannels > 1, a channel out of range, a non-finite tuning.  Not covered:
 * jsdr_group_*, the FAST variant, JNI / Java classes, a per-channel snapshot, switching on handles of the two older creators. */
int jsdr_bpsk_create_live_channels(jsdr_bpsk **h, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                                   const double *tuning_hz, const int *do_fft, const int *do_up, int64_t max_batch_samples);
/* Tuned handle: nstreams lock-step demodulators in the tune mode (doBufferTune, FUNcubeBPSKDemod.java:366-397), EVERY STREAM WITH
 * ITS OWN TUNING -- each FUNcubeBPSKDemod's own bpsk-tuning and its own "Freq: +10Hz / -10Hz" actions (:173-190, :195-196), for
 * signals that sit at different offsets and drift with Doppler.  Stream s is a demodulator created with tuning_hz[s]; all streams
 * advance together through jsdr_bpsk_batch_i16 / jsdr_bpsk_batch_f32.  Strides, ragged call lengths, the getters, pack_slots, the
 * slot layout and the profile calls are an ordinary handle's.  Handles from every other creator behave exactly as before.
 *   Result: stream s is bit-identical to a one-stream handle of jsdr_bpsk_create made with (int) of its tuning, given
 *     jsdr_bpsk_set_tuning(tuning_hz[s]) before its first sample, fed the same calls, and given jsdr_bpsk_set_tuning wherever
 *     stream s got jsdr_bpsk_set_stream_tuning: the bits of every call, FEC rc / bit index / bytes, the ten counters, the 18 state
 *     doubles (double 0, tuPhase, is the stream's own) and the (fi, fq) trace.
 *   The tuner recurrence (:384-390) is walked per stream on the device, once a call ("k_tuner_walk" in the profile); the front end
 *     is "k_front_pst" (jsdr_bpsk_front_kernel), behind it the three-kernel path.  The walk keeps tuPhase as it stands before
 *     every 64th sample of the call: 1/8 byte per sample and stream of max_batch_samples, beside the handle's other buffers.
 *   set_stream_tuning / set_stream_tunings (streams first .. first + count - 1): actionPerformed's tuning change (:174-189) on
 *     those streams only -- tuning, tuPhaseInc = 2 pi tuning / rate, dmMaxCorr = 0 (also when the value is the current one);
 *     tuPhase, all histories, the bit clock, the FEC register and the counters carry on; the other streams are not touched.  The
 *     change takes effect from the next call; the last 26 samples keep the factors they were mixed with (the pass-through of
 *     :395 included).  The bulk form checks every value before it applies any.
 *   Whole-handle controls: set_tuning applies to every stream; get_control reports stream 0; set_mode(0, do_up) and
 *     reconfigure(t, 0, do_up) store do_up (no effect in the tune mode) and treat dmMaxCorr as they do on an ordinary handle.
 *   Tunings: any finite value below `rate`.  <= 0 follows :388-396 per stream: samples pass unmixed once that stream's
 *     tuPhase <= 0, and 0 freezes tuPhase.  A tuning >= rate is refused: tuPhaseInc >= 2 pi, the single subtraction of :385 no
 *     longer bounds tuPhase and the table index leaves the range in which host and device agree.
 * JSDR_ERR, the handle unchanged, each checked before any device work: a null handle or pointer, a non-finite tuning or one
 * >= rate, a stream or range out of bounds, do_fft = 1 by any route (set_mode, reconfigure), set_variant(FAST), receive_i16 /
 * receive_f32 (the 1-stream form of jsdr_bpsk_create), the three per-stream calls on a handle of any other creator, and the
 * per-channel calls (set_channel_tuning, set_channel_mode, get_channel_control) on a tuned handle.
 * Not covered on this handle: FFT-acquire, the FAST variant, jsdr_group_*, receive_*, JNI / Java classes. */
int jsdr_bpsk_create_tuned(jsdr_bpsk **h, int rate, int nsamples_per_frame, int nstreams,
                           const double *tuning_hz /*[nstreams]*/, int64_t max_batch_samples);
int jsdr_bpsk_set_stream_tuning(jsdr_bpsk *h, int stream, double tuning_hz);
int jsdr_bpsk_set_stream_tunings(jsdr_bpsk *h, int first, int count, const double *tuning_hz);
int jsdr_bpsk_get_stream_tuning(jsdr_bpsk *h, int stream, double *tuning_hz);
/* host only, no device: the tuner recurrence exactly as the device walks it (CPU tests): n samples from tuPhase tu0 at tuPhaseInc
 * tu_inc -- k9_out[i]: the table index of sample i, 0 .. 255, or 256 where the sample passes through unmixed; *tu_end: tuPhase
 * after the last one (may be NULL) */
int jsdr_bpsk_tuner_walk_host(double tu0, double tu_inc, int64_t n, uint16_t *k9_out, double *tu_end);
/* Tuning plans: retunes INSIDE the next batch call of a tuned handle, each stream at samples of its own -- what two thousand
 * signals on two thousand Doppler curves need, which do not retune at the same instants and not only where a call ends.
 *   Entry i = (stream[i], at_sample[i], tuning_hz[i]): from sample at_sample of the NEXT batch call on, that stream has
 *     tuning = tuning_hz and tuPhaseInc = 2 pi tuning_hz / rate; the tuner's advance of sample at_sample is the first at the new
 *     increment -- exactly what cutting the call in front of that sample and changing the tuning between the two pieces does.
 *     The change is the configuration path's, setup (:192-209), as jsdr_bpsk_reconfigure states it: tuPhase, all histories, the bit
 *     clock, the FEC register, the counters and dmMaxCorr carry on.  dmMaxCorr is NOT zeroed: a plan is not the button, and the
 *     bookkeeping of the sync stage runs over the call's bits and has no sample positions to reset at.
 *   Result: stream s is bit-identical to a one-stream handle of jsdr_bpsk_create fed the same samples in pieces cut at stream s's
 *     own entries, with jsdr_bpsk_reconfigure(tuning, 0, 0) between the pieces: bits, FEC results, counters, state, trace.
 *   Order: entries go by stream, within a stream by strictly ascending at_sample >= 0; any number per stream, consecutive samples
 *     included; streams without entries are ordinary streams of that call.  Tunings as for jsdr_bpsk_create_tuned.
 *   Lifetime: one-shot.  The next batch call that succeeds (batch_i16 or batch_f32) consumes the plan, and the call after it runs
 *     with the tunings the plan left: get_stream_tuning, get_control (stream 0) and a saved record show each stream's last entry,
 *     state double 0 is the stream's own tuPhase, and the last 26 samples keep the factors they were mixed with.  A later plan
 *     replaces a pending one; n = 0 clears it.  set_stream_tuning(s), set_tuning, reconfigure and jsdr_bpsk_restore between the
 *     plan and the call act before sample 0, as they do without a plan; the entries come after them in sample order.  A plan is
 *     not state: jsdr_bpsk_save does not carry it (the blob format stays at version 1).
 *   On the device: a planned call runs the planned forms of the walk and of the front end ("k_front_pst_plan" from
 *     jsdr_bpsk_front_kernel; the profile slots are the same two); a call without a plan runs exactly the kernels it ran before.
 *     The plan is copied to the device when it is given (16 bytes an entry); the first plan adds 4 bytes per 64 samples and
 *     stream of max_batch_samples to the handle.
 * JSDR_ERR, the handle AND a pending plan unchanged, each checked before any device work: a handle that is null or not from
 * jsdr_bpsk_create_tuned, n < 0, a null array with n > 0, a stream out of range, entries out of order or duplicated, a negative
 * at_sample, a tuning that is not finite or >= rate.  A batch call whose nsamples does not exceed every pending at_sample is
 * refused, the handle unchanged, and the plan stays pending.  planned_tunings: the entries pending (0 after the call that took
 * them).  Not built: plans on ordinary or channel handles, JNI / Java classes, jsdr_group_*, the FAST variant, FFT-acquire. */
int jsdr_bpsk_plan_stream_tunings(jsdr_bpsk *h, const int32_t *stream, const int64_t *at_sample, const double *tuning_hz, int64_t n);
int jsdr_bpsk_planned_tunings(jsdr_bpsk *h, int64_t *n);
/* host only, no device (CPU tests): jsdr_bpsk_tuner_walk_host with a plan for one stream -- from sample at_sample[e] on
 * tuPhaseInc is inc_at[e], e = 0 .. nev - 1, at_sample >= 0 and strictly ascending (entries at or behind n are not reached);
 * nev = 0 with null arrays is jsdr_bpsk_tuner_walk_host */
int jsdr_bpsk_tuner_walk_plan_host(double tu0, double tu_inc, int64_t n, const int64_t *at_sample, const double *inc_at, int64_t nev,
                                   uint16_t *k9_out, double *tu_end);
/* Ramp plans: a tuning plan whose entries move -- one entry follows a stretch of a Doppler curve where steps need one entry per
 * tolerated error.  Everything said of tuning plans above holds (tuned handles only, one-shot, order, replacement, n = 0, what
 * acts before sample 0, refusals, the two profile slots); an entry gains a slope.
 *   Entry i = (stream[i], at_sample[i], tuning_hz[i], slope_hz_per_sample[i]), in effect from sample at_sample of the NEXT batch
 *     call until the stream's next entry or the call's last sample.  Sample n of that span has
 *         k        = n - at_sample                      (exact in a double)
 *         tuning_n = tuning_hz + (double)k * slope      one product, one sum, each rounded by itself
 *         inc_n    = 2 pi tuning_n / rate               left to right, as tuPhaseInc always is
 *     and the tuner's advance of sample n uses inc_n.  That is, by definition, a jsdr_bpsk_plan_stream_tunings plan with one entry
 *     per sample n at tuning_n computed in doubles by those two operations -- so stream s is bit-identical to a one-stream handle
 *     of jsdr_bpsk_create fed the samples one at a time with jsdr_bpsk_reconfigure(tuning_n, 0, 0) in front of each: bits, FEC
 *     results, counters, state, decoded[], trace.  dmMaxCorr is not zeroed.
 *   Zero slope: the entry takes tuning_hz itself, with no arithmetic, and means what it means in jsdr_bpsk_plan_stream_tunings.  A
 *     plan whose slopes are ALL zero is a step plan and runs as one ("k_front_pst_plan").  Before its first entry a stream runs at
 *     the increment it came into the call with, which is not recomputed.
 *   After the call: a stream whose last entry is a ramp holds the tuning of the call's LAST sample, tuning_hz +
 *     (double)(nsamples - 1 - at_sample) * slope, computed by the host at the call by the same two operations: get_stream_tuning,
 *     get_control (stream 0) and a saved record show it, and the device's tuPhaseInc is 2 pi / rate of exactly that double (what
 *     jsdr_bpsk_restore checks).  A ramp does not outlive its call.  To continue it, give the next call an entry at sample 0 with
 *     tuning_hz' = tuning_hz + (double)(nsamples - at_sample) * slope and the same slope (k restarts at 0 there: the curve is the
 *     same line, its roundings are the new entry's).
 *   Tunings: every tuning_n must be finite and below the rate.  They are monotone in k, so the two ends of a span decide: the one
 *     in front of the stream's next entry is checked when the plan is given; the one at the call's last sample is checked by the
 *     call, with "every at_sample inside the call" -- such a call is refused, the handle unchanged, and the plan stays pending.
 *     A slope that is not finite is refused when the plan is given.  Every refusal names the entry, leaves the handle AND a
 *     pending plan unchanged and comes before any device work.
 *   On the device: a call with a ramp plan runs the ramp forms of the walk and of the front end ("k_front_pst_ramp" from
 *     jsdr_bpsk_front_kernel).  Under a slope every sample costs an FP64 division in both kernels; samples under no slope cost
 *     what they cost a step plan.  The plan is copied when it is given: 24 bytes an entry (position, tuning, slope) and 8 per
 *     stream; the per-handle 4 bytes per 64 samples and stream are the step plans'.  jsdr_bpsk_planned_tunings counts ramp entries
 *     too.
 * Not built: ramps on ordinary or channel handles, JNI / Java classes, jsdr_group_*, the FAST variant, FFT-acquire, ramps that
 * outlive a call. */
int jsdr_bpsk_plan_stream_ramps(jsdr_bpsk *h, const int32_t *stream, const int64_t *at_sample, const double *tuning_hz,
                                const double *slope_hz_per_sample, int64_t n);
/* host only, no device (CPU tests): jsdr_bpsk_tuner_walk_plan_host with ramp entries -- from sample at_sample[e] on, sample i has
 * the tuning tuning_at[e] + (double)(i - at_sample[e]) * slope_at[e] (slope 0: tuning_at[e] itself) and tuPhaseInc 2 pi tuning /
 * rate; before the first entry tuPhaseInc is tu_inc.  *tu_end / *inc_end: tuPhase and tuPhaseInc after the last sample (may be
 * NULL).  nev = 0 with null arrays is jsdr_bpsk_tuner_walk_host */
int jsdr_bpsk_tuner_walk_ramp_host(double tu0, double tu_inc, int64_t n, int rate, const int64_t *at_sample, const double *tuning_at,
                                   const double *slope_at, int64_t nev, uint16_t *k9_out, double *tu_end, double *inc_end);
/* Tuned channel handle: ninputs x nchannels lock-step demodulators in the tune mode, EVERY CHANNEL OF EVERY INPUT WITH ITS OWN
 * TUNING, the channels of an input reading ONE input row -- several satellites inside one wideband capture, each on its own
 * Doppler curve, without the capture repeated once per satellite in device memory.  It is a tuned handle (above) of
 * ninputs x nchannels streams: channel c of input i is stream i * nchannels + c, as on every channel handle, and is created with
 * tuning_hz[i * nchannels + c].  1 <= nchannels <= 16, ninputs x nchannels <= 65535.
 *   Batch calls: jsdr_bpsk_batch_i16 (with ic, qc) and jsdr_bpsk_batch_f32 take the stride BETWEEN INPUTS, as on channel
 *     handles; ragged call lengths as on tuned handles.  The 26-sample input history is kept per input; the two input forms may
 *     alternate under the channel handle's rule (converted, or the int16 call refused when a float of it is no (float)s/32767f).
 *   Result: stream i * nchannels + c is bit-identical to stream i * nchannels + c of a jsdr_bpsk_create_tuned handle of
 *     ninputs x nchannels streams that reads a buffer in which every input is repeated nchannels times -- and so to the
 *     one-stream handle named there: bits, FEC results, counters, the 18 state doubles, decoded[], the (fi, fq) trace.
 *   Per-stream calls, with that stream numbering, exactly as on a jsdr_bpsk_create_tuned handle: set_stream_tuning /
 *     set_stream_tunings / get_stream_tuning, jsdr_bpsk_plan_stream_tunings, jsdr_bpsk_plan_stream_ramps,
 *     jsdr_bpsk_planned_tunings -- validation, messages, one-shot plans that survive a refused call, a ramp's tuning of the call's
 *     last sample afterwards.  set_tuning, set_mode(0, do_up), reconfigure(t, 0, do_up) and get_control as on a tuned handle.
 *     jsdr_bpsk_channel_info reports ninputs x nchannels; the per-stream getters, pack_slots, the slot layout and the profile
 *     calls apply unchanged.
 *   On the device: the walk is the tuned handle's ("k_tuner_walk" in the profile, over ninputs x nchannels rows); the front end
 *     is "k_chan_front_pst", "k_chan_front_pst_plan" or "k_chan_front_pst_ramp" (jsdr_bpsk_front_kernel): a tile of an input is
 *     read, DC-corrected and converted once, and mixed for every channel with the indices expanded from that channel's
 *     checkpoints.  Memory per stream as a tuned handle's; the input is ninputs rows, not ninputs x nchannels.
 * JSDR_ERR, the handle unchanged, each checked before any device work: null pointers, bad geometry, a non-finite tuning or one
 * >= rate at create; do_fft = 1 by any route; set_variant(FAST); receive_i16 / receive_f32; the per-channel calls
 * (set_channel_tuning, set_channel_mode, get_channel_control: the message names the per-stream call to use); jsdr_bpsk_save /
 * _restore / _state_bytes (a record carries a per-stream input history, this handle keeps one per input).
 * Not covered on this handle: FFT-acquire, the FAST variant, checkpoints, jsdr_group_*, receive_*, JNI / Java classes. */
int jsdr_bpsk_create_tuned_channels(jsdr_bpsk **h, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                                    const double *tuning_hz /*[ninputs * nchannels]*/, int64_t max_batch_samples);
/* Checkpoints: the state of a range of streams out of a handle and into one -- across a restart, a library upgrade, another
 * machine, or between handles (a split is two saves with ranges, a merge two restores at offsets).  A blob is self-contained,
 * versioned (format 1) and position-independent: little-endian fixed-width fields, a 192-byte header with the sizes and a
 * 64-bit FNV-1a checksum over everything behind it, then one 7184-byte record per stream (DESIGN.md 7 has the layout).  It
 * holds a SHARED block -- tuning, do_fft, do_up, tuPhase, tuPhaseInc, vcoPhase, dsCnt, the samples consumed and demodulated, the
 * tuner indices and mix flags of the last 26 samples, a pending mode-switch seam, the form (int16 / float) of the input
 * history -- and per stream: the bit clock and energy IIRs, the differential memory, the counters, the 5200-entry FEC
 * register, decoded[], the 26-sample down-sampler and 64-sample matched-filter histories, avePeakPower / aveCentreBin /
 * centreBin and the FFT path's history, and on a tuned handle the stream's tuning, tuPhase, tuPhaseInc and tuner indices.  A
 * record does not depend on max_batch_samples, on the handle's strides, on which buffers were current or on which kernels
 * the last call took: a blob restores into a handle of another max_batch_samples and another nstreams, and blobs of the
 * same streams from two such handles are byte-identical.
 *   state_bytes: the size of a blob of `count` streams.
 *   save: waits for the handle's pending work (as the getters do), writes streams first .. first + count - 1 into blob_host
 *     (cap bytes; *bytes: the blob's size) and changes nothing in the handle: a call after it gives what it would have given.
 *     A save between set_mode / set_tuning / reconfigure and the next call carries the pending seam.
 *   restore: writes all of the blob's streams into streams dst_first .. dst_first + count - 1.  From the next call on they
 *     continue bit for bit as the saved ones would have: bits, (fi, fq) trace, FEC rc / bit index / bytes, the ten counters,
 *     the 18 state doubles, decoded[].  Per-call results are not state: until that call get_bits / get_fec_count / get_trace
 *     report an empty call for the restored streams; get_counters / get_state / get_decoded report the restored values.
 *     jsdr_bpsk_snapshot_read of a one-stream handle is not touched: it reports "nothing received yet" (or the frame it held)
 *     until the next receive_*.
 *   The shared-block rule: a handle that has consumed no sample and has had nothing restored ADOPTS the blob's shared block,
 *     a pending seam included (the FFT-acquire buffers are allocated as jsdr_bpsk_set_mode allocates them).  Any other handle
 *     must already be at exactly that block, bit for bit, and then only the streams are written.  Streams of an adopting
 *     handle that no blob fills run on from the zero state at the adopted sample count: which streams mean something is the
 *     caller's business.  A restored handle cannot become JSDR_VARIANT_FAST (as a retuned one cannot).
 *   blob_info: no device, no handle -- what a caller needs to create the right handle for a blob.
 *   state_kernel_ms: a diagnostic -- the device time of the last save's gather kernel and of the last restore's scatter kernel
 *     on this handle (HIP events around the launch; -1: none yet).
 * JSDR_ERR, the handle exactly as it was, everything checked before the first write: a null pointer, a range outside the
 * handle, cap too small, a blob that is short, has a wrong magic / version / record size or fails its checksum, a rate, frame
 * size or kind (ordinary / tuned) other than the blob's, a shared block that is not a non-fresh handle's, a handle of
 * jsdr_bpsk_create_channels / _create_mode_channels / _create_live_channels, a JSDR_VARIANT_FAST handle; and, because a
 * checksum is easy to forge, a blob whose index-like values are out of range: non-finite or out-of-range tuning and phases, a
 * tuPhaseInc that is not 2 pi tuning / rate, dsCnt or the sample counts, a bit-clock position outside 0 .. 7, a centre bin the
 * FFT-acquire rule cannot leave, a tuned stream's tuner index above 256.  Everything else in a record (energies, counters,
 * register entries) is data the kernels carry without indexing by it.  The promise covers REFUSALS: a call that fails later, in
 * a device allocation, copy or launch, may leave allocated what it allocated (the staging image, the FFT-acquire buffers --
 * which a blob holding FFT-acquire state makes any handle allocate, whatever its mode).
 * Not covered: channel handles of all three kinds, the FAST variant and its shadow, jsdr_group_*, JNI / Java classes, device-
 * resident blobs, jsdr_demod_* handles. */
typedef struct jsdr_bpsk_blob_info_t {
    int32_t version;            /* format version (1) */
    int32_t kind;               /* 0: jsdr_bpsk_create, 1: jsdr_bpsk_create_tuned */
    int32_t rate, nsamples_per_frame, nstreams;
    int32_t do_fft, do_up;      /* the mode the streams continue in */
    int32_t seam;               /* 0, or a mode switch whose first call is still to come (1: to FFT-acquire, 2: to the tune mode) */
    int32_t record_bytes, header_bytes;
    int64_t n_in, n_ds;         /* samples consumed / demodulated per stream (cntRaw, cntDS) */
    double tuning_hz;           /* the shared tuning (a tuned handle: 0, each record has its own) */
} jsdr_bpsk_blob_info_t;
int jsdr_bpsk_state_bytes(jsdr_bpsk *h, int count, size_t *bytes);
int jsdr_bpsk_save(jsdr_bpsk *h, int first, int count, void *blob_host, size_t cap, size_t *bytes);
int jsdr_bpsk_restore(jsdr_bpsk *h, int dst_first, const void *blob_host, size_t bytes);
int jsdr_bpsk_blob_info(const void *blob_host, size_t bytes, jsdr_bpsk_blob_info_t *out);
int jsdr_bpsk_state_kernel_ms(jsdr_bpsk *h, double *pack_ms, double *unpack_ms);
int jsdr_bpsk_acq_last_launch(jsdr_bpsk *h, int64_t *fwd_frames, int64_t *inv_frames);
int jsdr_bpsk_channel_info(jsdr_bpsk *h, int *ninputs, int *nchannels);
int jsdr_bpsk_set_channel_tuning(jsdr_bpsk *h, int channel, double tuning_hz);
int jsdr_bpsk_set_channel_mode(jsdr_bpsk *h, int channel, int do_fft, int do_up);
int jsdr_bpsk_get_channel_control(jsdr_bpsk *h, int channel, double *tuning_hz, int *do_fft, int *do_up);
/* receive(float[]) / raw form for stream 0 of a 1-stream handle (:357-364).
 * Non-finite input (NaN, +-Infinity) and huge floats are taken as Java takes them: a comparison with a NaN is false, the filters
 * and IIRs carry it.  One NaN therefore freezes the peak tracker (dmNewPeak, :586-592) for the life of the stream, as in the
 * reference; bits go on being sliced at the frozen position. */
int jsdr_bpsk_receive_f32(jsdr_bpsk *h, const float *iq_host);
int jsdr_bpsk_receive_i16(jsdr_bpsk *h, const int16_t *raw_host, int ic, int qc);
/* batched: raw_dev[s*stream_stride + 2*t .. +1] = I,Q of sample t of stream s; nsamples must be a
 * multiple of nsamples_per_frame in FFT mode; asynchronous on `stream`.                        */
int jsdr_bpsk_batch_i16(jsdr_bpsk *h, const int16_t *raw_dev, int64_t stream_stride_i16,
                        int64_t nsamples, int ic, int qc, void *stream);
/* batched IAudioHandler.receive(float[]): iq_dev[s*stream_stride_f32 + 2t], [.. + 2t+1] = I, Q of sample t of stream s, taken as
 * the reference takes buf[] (no DC correction, no scaling: x = (double)f).  Otherwise as jsdr_bpsk_batch_i16: asynchronous on
 * `stream`, the tail, sync and FEC on the side stream, live control between calls as between int16 calls.
 *   Serves an ordinary handle of any nstreams (the tune mode at any call length, FFT-acquire at whole frames of every frame
 *   jsdr_bpsk_create accepts) and the handles of jsdr_bpsk_create_channels / jsdr_bpsk_create_mode_channels (the stride is
 *   between INPUTS).  Results are bit-identical to nstreams one-stream handles of the same configuration, each fed the same
 *   floats through jsdr_bpsk_receive_f32.  FFT-acquire channels of float input run the forward phase once per band in use
 *   (the both-band transform is an int16 kernel); jsdr_bpsk_acq_last_launch reports what ran.
 *   Calls of the two forms may alternate on one handle: float after int16 converts the 26-sample input history (per input on
 *   a channel handle), int16 after floats that are (float)s/32767f values converts it back, int16 after any other float is
 *   refused with the handle unchanged (a NaN or an Infinity among the last 26 floats is such a float).
 *   Non-finite input (NaN, +-Infinity) and huge floats are taken as Java takes them: a comparison with a NaN is false, the
 *   filters and IIRs carry it.  One NaN therefore freezes the peak tracker (dmNewPeak, :586-592) of ITS stream for the life of
 *   that stream, as in the reference, while its bits go on being sliced at the frozen position; other streams are untouched.
 *   jsdr_bpsk_front_kernel: "k_fm_f32", the fused float kernel, where an int16 call would take "k_fm" (a standard decimation, a
 *   periodic tuner schedule or none, no call that straddles a retune); jsdr_bpsk_set_cu_share / _last_launch and the k_fm and
 *   k_fm_prep profile slots apply to it.  JSDR_FM=0 (JSDR_KNOBS=1): always the three-kernel path.
 * JSDR_ERR, the handle unchanged, each checked before any device work: a null handle or pointer, an odd stride, a stride below
 * 2 nsamples with more than one stream or input, nsamples outside (0, max_batch_samples], a call that is not whole frames
 * where FFT-acquire needs them, a JSDR_VARIANT_FAST handle (its certification re-reads int16).
 * Not covered: jsdr_group_*, the FAST variant, JNI and the Java classes (they feed floats through receive_f32). */
int jsdr_bpsk_batch_f32(jsdr_bpsk *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples, void *stream);
/* The BPSK scope over batches: the five debug rings of FUNcubeBPSKDemod (tuned, downSmpl, demodIQ, demodBits, demodRe,
 * FUNcubeBPSKDemod.java:118-125) and everything paintComponent's first panel computes from them (:231-268), for every frame of a
 * batch call.  A scope call IS the batch call plus the painter: it runs jsdr_bpsk_batch_i16 / _f32 with the same arguments --
 * every getter and the carried state come out bit for bit as the batch call leaves them -- and then, on the caller's stream, the
 * scope passes over the frames of the call.  The painter's two spectra (:270-327) are jsdr_bpsk_scope_spectra_i16 / _f32 below; the
 * tuned and ds rows are their inputs.
 * Geometry: n the handle's frame, D = rate / 9600, L = n * 9600 / rate (Java's int arithmetic, :201: the length of the three
 * short rings in pairs), frames = nsamples / n, row = s * frames + f for frame f of stream s, rows packed.  The decimated sample
 * number g (the g-th RxDemodulate call since the origin, from 0) belongs to frame f when G_f <= g < G_{f+1}, G_f =
 * (n_in + f n) / D - origin, n_in the samples the handle had taken before the call.  origin is 0 at creation;
 * jsdr_bpsk_reconfigure is the reference's setup, which resets the ring indices (:198-204), and sets origin to the decimated
 * samples taken so far.  jsdr_bpsk_restore leaves origin as it is, 0 on a fresh handle: the blob does not carry it, and a
 * handle that adopts a blob counts its slots as if the saved stream had never been reconfigured.
 * What the painter sees after frame f, all rings in slot order; each output may be NULL:
 *   tuned_dev[row][n][2]  slot k: the pair RxDownSample received for the frame's sample k (:471-473): (i cosTab[..], q sinTab[..]),
 *                         or (i, q) where tuPhase <= 0 (:388-396), from the call's own tuner schedule (after jsdr_bpsk_set_tuning too);
 *   ds_dev[row][L][2]     downSmpl: slot g mod L holds the down-sampler output g after HOWARD_FUDGE_FACTOR (:486, :507-509); of
 *                         the frame's g that share a slot the largest wins;
 *   iq_dev[row][L][2]     demodIQ: slot (g + 1) mod L holds (fi, fq) of sample g (the index moves before the write, :529-531);
 *                         again the largest g of the frame wins;
 *   bits_dev[row][L]      demodBits: zero (:367-370), then for g ascending through the frame, at every detector instant with
 *                         energy2 > 100.0, slot (g + 1) mod L takes +1 or -1 (:549-551); a later bit overwrites an earlier one,
 *                         a later sample that is no bit does not clear it;
 *   max_dev[row][2]       mi, mq of :232-238: from 0.0 under the strict mi < Math.abs(x); a NaN never wins;
 *   pts_dev[row][L][4]    per slot, with xs = 100.0 / mi, ys = 100.0 / mq, rs = 50.0 / (mi * mq) (:239, :260): (int)(I * xs), the
 *                         yellow x and the red trace; (int)(Q * ys), the yellow y; (int)(Q * xs), the blue trace (xs, as written,
 *                         :256); (int)(demodRe[slot] * rs), the grey trace -- demodRe zeroed and marked like demodBits, holding di.
 * (int) is Java's cast (truncates, saturates, NaN -> 0); every product and quotient is one IEEE double operation; mi == 0 gives
 * xs = Infinity and 0 * Infinity = NaN -> 0, as in Java.  The window offsets (101 +, getHeight() - 301 -, xo + n / 2, * 50) are
 * the caller's arithmetic.  With all six outputs NULL the call is the batch call and launches nothing more.
 * jsdr_bpsk_scope_layout (host only) states L, origin and G_0 .. G_frames (g_first, cap entries of room, frames + 1 needed) for
 * a call of nsamples from the handle's present counters; any of the three may be NULL.  It refuses what the scope calls refuse
 * of the handle and of nsamples.
 * Passes: "k_bpsk_scope_front" (tuned and ds: the input converted and mixed again with the call's tuner schedule, the 27 taps at
 * the frame's decimated instants from the input history of before the call), "k_bpsk_scope_walk" (bits and pts: the bit clock of
 * :533-593 again over the call's (fi, fq), from the clock state of before the call, which is copied on the device ahead of the
 * call's own tail kernel, ordered by events, no host wait) and "k_bpsk_scope_pts" (iq, max, pts); jsdr_bpsk_scope_kernel joins
 * what the last scope call launched with '+' ("" before the first and after a call with no output).  The scratch between the
 * passes (the clock copy, the call's tuner index table) belongs to the handle: allocated at the first scope call that needs it,
 * counted by jsdr_live_resources, gone with jsdr_bpsk_destroy.  A handle that makes no scope call allocates and launches what it
 * did before.  Scope calls belong on one stream at a time, the stream of the handle's batch calls.
 * Serves handles of jsdr_bpsk_create in the tune mode, JSDR_VARIANT_EXACT, any nstreams, int16 and float input, live
 * jsdr_bpsk_set_tuning between calls, restored handles.
 * JSDR_ERR before any device work, the handle unchanged, the message naming the reason: a null handle or input; nsamples not
 * whole frames or outside (0, max_batch_samples]; the stride rules of the batch call; n_in not a multiple of n (the reference
 * never paints such a state); L < 1; rate < 9600 (a frame does not refill the rings); do_fft set or a mode switch pending (in
 * FFT-acquire `tuned` is the inverse transform's real part twice); every channel handle and tuned handle; the FAST variant; an
 * output not aligned to its element size (tuned_dev: 16 bytes).  What only the batch call inside refuses (int16 input behind float
 * frames whose last 26 samples no int16 holds) is refused after the scope's scratch exists and the clock copy is queued: the
 * demodulator's state is unchanged, and nothing of the scope is launched. */
int jsdr_bpsk_scope_i16(jsdr_bpsk *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc,
                        double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev,
                        void *stream);
int jsdr_bpsk_scope_f32(jsdr_bpsk *h, const float *iq_in_dev, int64_t stream_stride_f32, int64_t nsamples,
                        double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev,
                        void *stream);
int jsdr_bpsk_scope_layout(jsdr_bpsk *h, int64_t nsamples, int *ring_len, int64_t *origin, int64_t *g_first /* [frames + 1] */,
                           int cap);                              /* host only */
const char *jsdr_bpsk_scope_kernel(jsdr_bpsk *h);                 /* what the last scope call launched, joined with '+' */
/* The BPSK scope's spectra: the second half of the painter's panel (:270-327), the green spectrum of the `tuned` ring and the
 * cyan one of the `downSmpl` ring, for every frame of a batch call.  A spectra call IS the scope call with the same arguments --
 * its six outputs come out bit for bit as jsdr_bpsk_scope_* leaves them, and so does everything of the batch call -- plus, for
 * row = s * frames + f, with X the row tuned_dev[row] (len = n) or ds_dev[row] (len = L) as the scope call defines them, in slot
 * order, nothing rotated:
 *   Y = DoubleFFT_1D.complexForward(X): this project's jo_fft_f64 (oracle/o_fft.c), operation for operation -- the bit-reversed
 *       radix-2 network for len = 2^k, else Stockham passes in jo_fft_mixed_radices order, a prime radix above 7 as its definition;
 *   psd[k] = sqrt(Yre * Yre + Yim * Yim) for all len bins (:277): two products, one sum, a correctly rounded root;
 *   max = 0.0, mo = 0, and for k ascending over all len bins under the strict max < psd[k] they take psd[k] and k (:274-282): a NaN
 *       never wins, ties go to the lowest bin, a row of NaN bins or of silence leaves (0.0, 0);
 *   with Wp = plot_width (the reference's getWidth() - xo), pi = (double)(len / 2) / (double)Wp, ys = 100.0 / max (:285, :293):
 *       y[0] = (int)(psd[0] * ys), and for m = 1 .. Wp - 1, i = (int)(pi * (double)m), l = (int)pi, y[m] = (int)(getMax(psd, i, l) * ys)
 *       -- getMax as written (:348-355): from psd[i], strict m < psd[j] for j < i + l, psd[i] itself when l == 0.  (int) is Java's
 *       cast; max == 0 gives ys = Infinity and 0 * Infinity = NaN -> 0.  Only the lower half of psd[] reaches the polyline; the
 *       window arithmetic (getHeight() - 1 - y, xo + m) stays the caller's.
 * Outputs, rows packed, each may be NULL: tspec_dev[row][Wp] and dspec_dev[row][Wp] the y[] of the green and the cyan spectrum,
 * tpeak_dev[row][2] and dpeak_dev[row][2] (max, (double)mo), tpsd_dev[row][n] and dpsd_dev[row][L] the whole psd[].  With all six
 * NULL the call is jsdr_bpsk_scope_* launch for launch; with the scope's six NULL as well it is the batch call.  The painter
 * transforms its rings in place and every later receive() overwrites them whole, so the spectra change nothing downstream.
 * Rows: a spectrum reads the caller's tuned_dev / ds_dev rows where they are given.  Where they are not, the rows come from the
 * handle: k_bpsk_scope_front fills them a pass of frames at a time -- as many frames as 64 MiB of rows hold, one at least;
 * jsdr_bpsk_scope_chunk(h, frames_per_pass) lowers that (0: the default) -- each pass followed by its spectra kernels.
 * Kernels, one workgroup a row, the row's image in LDS, the epilogue (magnitudes, first maximum, pooled casts) in the same kernel:
 *   "k_bpsk_spec_pow2"      len = 2^k, 64 .. 8192;
 *   "k_bpsk_spec_mixed64"   any other len up to 512 (L = 204 = 4 3 17, 102, 409), one wave a row;
 *   "k_bpsk_spec_mixed256"  ... up to 2048;   "k_bpsk_spec_mixed768"  ... up to 9600 (4800, 4410).
 * Served lengths: powers of two 64 .. 8192 and every other length of 2 .. 9600 with at most 12 passes.  Not served, refused with
 * the length named: powers of two below 64 and above 8192, every other length above 9600 (19200 among them).
 * jsdr_bpsk_scope_kernel names the spectra kernels behind the scope's passes, the green spectrum's first.  The plans of n and L,
 * their tables and the handle's rows are allocated at the first spectra call that needs them, counted by jsdr_live_resources and
 * gone with the handle; a later call with the same outputs and sizes neither allocates nor waits for the device.  A handle that
 * makes no spectra call allocates and launches what it did before.
 * JSDR_ERR before any device work, the handle unchanged: whatever jsdr_bpsk_scope_* refuses, with its message; plot_width outside
 * 1 .. 32768 where tspec_dev or dspec_dev is given; an output not aligned (the int32 rows: 4 bytes, the double rows: 16 bytes); a
 * row length that no kernel serves, where a spectrum of that row is asked for.
 * jsdr_bpsk_scope_spec_layout (host only, no device): first[m] = i and count[m] = l of column m in the double arithmetic above,
 * (0, 0) at m = 0, for a row of len points -- any len >= 2, served by a kernel or not; JSDR_ERR for len < 2, plot_width outside
 * 1 .. 32768, cap < plot_width, and for a column that would read outside psd[] (none exists: i + l <= len / 2 + 1). */
int jsdr_bpsk_scope_spectra_i16(jsdr_bpsk *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc,
                                double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev,
                                int plot_width, int32_t *tspec_dev, double *tpeak_dev, double *tpsd_dev, int32_t *dspec_dev,
                                double *dpeak_dev, double *dpsd_dev, void *stream);
int jsdr_bpsk_scope_spectra_f32(jsdr_bpsk *h, const float *iq_in_dev, int64_t stream_stride_f32, int64_t nsamples,
                                double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev,
                                int plot_width, int32_t *tspec_dev, double *tpeak_dev, double *tpsd_dev, int32_t *dspec_dev,
                                double *dpeak_dev, double *dpsd_dev, void *stream);
int jsdr_bpsk_scope_spec_layout(int len, int plot_width, int32_t *first /* [plot_width] */, int32_t *count, int cap);  /* host only */
int jsdr_bpsk_scope_chunk(jsdr_bpsk *h, int frames_per_pass);     /* frames of one pass of handle-owned rows; 0: the default */
int jsdr_bpsk_set_cu_share(jsdr_bpsk *h, int wgs_per_cu); /* see jsdr_fft_set_cu_share; applies to the tune-mode front-end kernel */
/* The library's own answer to "should fft.receive and this demodulator, fed the same batch on two streams, share the CUs?":
 * the shares to pass to jsdr_fft_set_cu_share / jsdr_bpsk_set_cu_share (2 and 1 where the split was measured to pay: the
 * exact variant's tune-mode kernel, 96 kHz, 2048-sample frames, 8192 streams and more per device), 0 and 0 everywhere else.
 * bench.py and jsdr_group_* ask this instead of carrying the rule themselves. */
int jsdr_bpsk_pair_shares(jsdr_bpsk *h, int *fft_wgs_per_cu, int *bpsk_wgs_per_cu);
/* diagnostics: tiles x streams of the last tune-mode front-end launch (k_fm, k_fm_f32) and the workgroups that strode over them */
int jsdr_bpsk_last_launch(jsdr_bpsk *h, int64_t *work_items, int64_t *workgroups);
/* diagnostics: which form of k_fm the last call took.  *specialised 1: the form with the 8-phase tuner's exact factors built in
 * (tuning an eighth of the rate, exact variant, decimation 10, int16 batches of more than FM_THREADS outputs), *phase the tuner
 * phase (0 .. 7, table index 32 * phase) of the first window sample of the call's first tile; its other tiles alternate
 * between that phase and the one four further.  0 and -1: the generic form, or a call that did not take k_fm.  The results are
 * bit-identical either way. */
int jsdr_bpsk_fm_form(jsdr_bpsk *h, int *specialised, int *phase);
/* wait until every kernel of the calls made so far has finished (the 9600 Hz tail and the FEC decoder run on
 * an internal side stream so that they overlap the next call's front end; the getters below call this). */
int jsdr_bpsk_sync(jsdr_bpsk *h);
/* results */
enum { JSDR_BPSK_NCOUNTERS = 10 };
/* cntRaw,cntDS,cntBit,cntFEC,cntDec,dmErrBits,dmCorr,dmMaxCorr,decodeOK,centreBin (:110-115,:405,:498) */
int jsdr_bpsk_get_counters(jsdr_bpsk *h, int stream, int32_t out[JSDR_BPSK_NCOUNTERS]);
/* bits sliced during the LAST batch/receive call, +1/-1 each (:545-554) */
int jsdr_bpsk_get_bits(jsdr_bpsk *h, int stream, int8_t *bits_host, int cap, int *nbits);
/* FECDecode calls made during the last call: rc + index (1-based, within the call) of the bit that triggered */
int jsdr_bpsk_get_fec(jsdr_bpsk *h, int stream, int idx, int32_t *rc, int32_t *bit_index, uint8_t out_host[256]);
int jsdr_bpsk_get_fec_count(jsdr_bpsk *h, int stream, int *count);
int jsdr_bpsk_get_decoded(jsdr_bpsk *h, int stream, uint8_t out_host[256]);   /* decoded[] (:111) */
/* matched-filter outputs (fi,fq) of the last call, double[npairs][2] (:518-531) */
int jsdr_bpsk_get_trace(jsdr_bpsk *h, int stream, double *out_host, int64_t cap_pairs, int64_t *npairs);
/* scalar state, same 18-value layout as the oracle: tuPhase,vcoPhase,dmBitPhase,dmEnergyOut,energy1,
 * energy2,avePeakPower,aveCentreBin,dmEnergy[8],dmLastIQ[2]                                       */
int jsdr_bpsk_get_state(jsdr_bpsk *h, int stream, double out[18]);
/* Results of the last completed receive_f32 / receive_i16 of a 1-stream handle, for a reader on ANOTHER thread (the
 * reference's Swing thread paints these fields while the audio thread is inside receive(), FUNcubeBPSKDemod.java:
 * 220-228,331-337): double-buffered on the host, published after every receive; the read takes no lock, makes no
 * device call and never sees a half-written frame.  The getters above belong to the thread that calls receive. */
typedef struct jsdr_bpsk_snapshot {
    int64_t frames;                        /* receive() calls completed */
    int32_t counters[JSDR_BPSK_NCOUNTERS]; /* as jsdr_bpsk_get_counters */
    int32_t nbits;                         /* bits sliced during that frame (first 512 kept) */
    double state[18];                      /* as jsdr_bpsk_get_state */
    uint8_t decoded[256];                  /* decoded[] (:111) */
    int8_t bits[512];
} jsdr_bpsk_snapshot;
int jsdr_bpsk_snapshot_read(jsdr_bpsk *h, jsdr_bpsk_snapshot *out);
/* per-kernel HIP-event timing of the batch pipeline (events recorded on the caller's stream around each
 * launch while enabled).  profile_read sums and clears what was recorded since the last read.          */
int jsdr_bpsk_profile_enable(jsdr_bpsk *h, int on);
int jsdr_bpsk_profile_count(void);                 /* number of kernels in the pipeline */
const char *jsdr_bpsk_front_kernel(jsdr_bpsk *h);  /* name of the front-end kernel the last call launched */
const char *jsdr_bpsk_tail_kernel(jsdr_bpsk *h);   /* ... of its tail kernel: k_tail (one wave per stream) or k_tail8 (eight streams per wave) */
const char *jsdr_bpsk_fec_kernel(jsdr_bpsk *h);    /* ... of its FEC form: k_fec_bpsk, or the batch form's k_fec_bits+k_vitq+k_fec_rs */
/* 1 when the handle runs its tail / sync / FEC on a side stream of its own (batch handles), 0 when on the caller's stream
 * (1-stream handles; FFT-acquire with a mixed-radix frame; JSDR_NO_OVERLAP): *on receives it.  What a benchmark reports
 * instead of re-deriving the library's rule.                                                                        */
int jsdr_bpsk_side_stream(jsdr_bpsk *h, int *on);
/* the input-independent tuner / VCO schedules built so far: on the calling thread / taken from the look-ahead worker
 * (periodic configurations reuse one schedule and build none after the first calls) */
int jsdr_bpsk_schedule_stats(jsdr_bpsk *h, int64_t *computed_inline, int64_t *prefetched);
const char *jsdr_bpsk_profile_name(int k);
int jsdr_bpsk_profile_read(jsdr_bpsk *h, double *ms_total, int *launches);
/* device-resident result slots for the multi-GPU all-gather: per stream
 * int32 header[16] = {nbits, nfec, counters[10], 0...} followed by int8 bits[slot_bits] and
 * nfec_max x {int32 rc, int32 bit_index, uint8 data[256]}.  Layout constants via slot_info.      */
int jsdr_bpsk_slot_info(jsdr_bpsk *h, int64_t *slot_bytes, int64_t *bits_offset, int64_t *fec_offset,
                        int *slot_bits, int *nfec_max);
int jsdr_bpsk_pack_slots(jsdr_bpsk *h, uint8_t *slots_dev, void *stream);

/* ------------------------------------------------------------------ synthetic inputs (bench / tests)
 * Integer-only generators, bit-identical to oracle/o_synth.c.  Not part of the reference.        */
int jsdr_synth_diffsign(const uint8_t *sym_dev, int64_t nsym, int nstreams, int8_t *dsign_dev, void *stream);
int jsdr_synth_dbpsk(int16_t *out_dev, int64_t stream_stride_i16, int nstreams, int64_t n0, int64_t n,
                     const int8_t *dsign_dev, int64_t nsym, int samples_per_sym, uint32_t phase0,
                     uint32_t phase_inc, const int16_t *cos_tab_dev, const int16_t *sin_tab_dev,
                     int noise_gain, const uint64_t *noise_keys_dev, void *stream);
int jsdr_synth_tones(int16_t *out_dev, int64_t frame0, int64_t nframes, int n, const int16_t *cos_tab_dev,
                     int noise_gain, uint64_t key, void *stream);
int jsdr_synth_payloads(uint64_t seed, int stream0, int nstreams, int nframes, uint8_t *out_dev, void *stream);

/* ------------------------------------------------------------------ demod.java
 * The AM/FM IAudioHandler, demod.receive (demod.java:398-483), batched over `nstreams` independent streams that
 * share one set of controls: 21-tap complex float band-pass (filter(), :378-396), down-conversion NCO
 * (:423-434), AM envelope minus its running mean (:448-451) or FM quadrature-delay detector (:453-461), the
 * frame maximum, AGC and the (short)(x*32767f) stereo output (:465-481).  Float arithmetic in the reference's
 * order (no FMA), so int16 outputs are bit-identical to the CPU restatement; cos/sin of the NCO phase come
 * from the device math library.  A frame is blen/size samples (`sam.length/2`, :229-231); AGC and
 * the AM mean are per frame, the filter, NCO and FM states run on across frames and calls.                    */
typedef struct jsdr_demod jsdr_demod;
#define JSDR_DEMOD_OFF 0 /* demod.java:39-43 */
#define JSDR_DEMOD_RAW 1
#define JSDR_DEMOD_AM 2
#define JSDR_DEMOD_NFM 3
#define JSDR_DEMOD_WFM 4
int jsdr_demod_create(jsdr_demod **h, int rate, int nsamples_per_frame, int nstreams, int64_t max_batch_samples);
int jsdr_demod_destroy(jsdr_demod *h);
/* "demod-mode", "demod-fir-enable", the down-conversion toggle, "demod-agc-enable" (:36-38,198-203) */
int jsdr_demod_configure(jsdr_demod *h, int mode, int dofir, int dodwn, int doagc);
/* demod.weights() (:341-375) for the band [flo, fhi] Hz (flo = INT_MIN: the all-pass impulse); clears every
 * stream's delay line and (band-pass) restarts the carrier phase; returns the 21 weights and phi if asked.
 * The range check of filterMove (:300-312) is the caller's (host mirror: java_sdr::demod).                     */
int jsdr_demod_weights(jsdr_demod *h, int flo, int fhi, float w_out[21], float *phi_out);
/* whole frames of every stream; audio_dev receives one (L,R) int16 pair per input sample (:473-478) */
int jsdr_demod_batch_i16(jsdr_demod *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples,
                         int ic, int qc, int16_t *audio_dev, int64_t audio_stride_i16, void *stream);
int jsdr_demod_batch_f32(jsdr_demod *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples,
                         int16_t *audio_dev, int64_t audio_stride_i16, void *stream);
/* IAudioHandler.receive(float[]) for a 1-stream handle: one frame (2n floats) in, 2n int16 out */
int jsdr_demod_receive_f32(jsdr_demod *h, const float *buf_host, int16_t *audio_host);
/* the reference's `max` / `avg` fields after the last frame of the last call (:465-467) */
int jsdr_demod_frame_stats(jsdr_demod *h, int stream, float *max_out, float *avg_out);
int jsdr_demod_state(jsdr_demod *h, float *car_out, float *phi_out);
/* Channel handle: demod.java's controls each pick a channel out of the passband (the band-pass of weights(), the NCO at
 * flo, filterMove, the mode / AGC / FIR / down-conversion switches, :184-218, 341-375); one handle of ninputs x nchannels
 * receivers, each channel with its own controls.  Channel c of input i is stream i * nchannels + c.  1 <= nchannels <= 16;
 * ninputs * nchannels and the frames per call obey jsdr_demod_create's limits.  Every channel starts as a new ordinary
 * handle does (MODE_OFF, switches 0, flo = INT_MIN, fhi = INT_MAX, weights 0, car = phi = 0).  Each input is read and
 * converted once for all its channels (k_demod_chan); results are bit-identical to nchannels ordinary handles fed the same
 * input and given the same controls.
 *   configure_channel: actionPerformed's mode / AGC / FIR / down-conversion change (:184-218) on that channel: fields only.
 *   channel_weights: weights() (:341-375) for that channel: its delay line cleared on every input (after the handle's
 *     pending calls, without waiting for the device) and, for a band-pass, phi set and car restarted at 0; the other
 *     channels' rings, car and FM state carry on.  w_out / phi_out may be NULL.  filterMove's range check is the caller's.
 *   get_channel: the controls now in effect; channel_state: that channel's car and phi.
 *   configure / weights apply to every channel; state reports channel 0; frame_stats takes the stream i * nchannels + c.
 *   batch_i16 / batch_f32: stream_stride is between INPUTS, audio_stride between the ninputs * nchannels output rows.
 *   receive_f32 on a 1-input handle: one 2n-float frame in, nchannels 2n-sample frames out, channel c at c * 2n.
 *   channel_info: an ordinary handle reports nstreams x 1 (and takes channel 0 in the per-channel calls).
 *   The float rows of AM channels (of every channel, for frames above 10240 samples) are allocated when a call first
 *     needs more of them than before: that call waits for the whole device once (a live switch to AM included).
 * JSDR_ERR, every channel's controls and state as before the call: a channel out of range, a mode outside 0..4, a null
 * handle or output pointer, nsamples not whole frames or above max_batch, strides too small, receive_f32 with ninputs > 1,
 * bad create_channels arguments (checked before any device work).  Not covered: JNI / Java classes, jsdr_group. */
int jsdr_demod_create_channels(jsdr_demod **h, int rate, int nsamples_per_frame, int ninputs, int nchannels,
                               int64_t max_batch_samples);
int jsdr_demod_channel_info(jsdr_demod *h, int *ninputs, int *nchannels);
int jsdr_demod_configure_channel(jsdr_demod *h, int channel, int mode, int dofir, int dodwn, int doagc);
int jsdr_demod_channel_weights(jsdr_demod *h, int channel, int flo, int fhi, float w_out[21], float *phi_out);
int jsdr_demod_get_channel(jsdr_demod *h, int channel, int *mode, int *dofir, int *dodwn, int *doagc, int *flo, int *fhi);
int jsdr_demod_channel_state(jsdr_demod *h, int channel, float *car_out, float *phi_out);
/* per-kernel HIP-event timing of the batch calls (bench.py), as jsdr_bpsk_profile_* */
int jsdr_demod_profile_enable(jsdr_demod *h, int on);
int jsdr_demod_profile_count(void);
const char *jsdr_demod_profile_name(int kernel);
int jsdr_demod_profile_read(jsdr_demod *h, double *ms_total, int *launches);
/* The demod scope over batches: what demod.paintComponent (demod.java:509-558) draws from a frame, for every frame of a batch
 * call.  A scope call IS the batch call plus the painter: it runs jsdr_demod_batch_i16 / _f32 with the same arguments -- the
 * same launches, the same audio, frame_stats, jsdr_demod_state and carried state, bit for bit -- and then, on the same stream,
 * the scope passes over the frames of the call.  After receive() of a frame of n samples (:398-483) the painter sees
 *   sam[2k]     the final float of sample k, (AM ? d - avg : d) * (doagc ? 1.0f / max : 1) (:472), before the cast to short;
 *   sam[2k + 1] the mixed Q of sample k, behind filter() and the NCO (0 in MODE_OFF, :443);
 *   dbg[]       the frame's mixed (I, Q) pairs in order (:436-437), in every mode, MODE_OFF included.
 * For a panel W = width pixels wide and H = height pixels high:
 *   trace_dev[row][W]  the magenta polyline (:519-531): entry 0 is H/4 (the start, `ly`); entry x + 1 is y of column x < W - 1,
 *                      y = H/4 - (int)(getAbsMax(sam, 2i, (int)scale, 2) * (float)(H/4)), scale = (float)(n / W) (an int
 *                      division), i = (int)((float)x * scale).  getAbsMax as written (:569-578, `c = |r|` outside the if, the
 *                      walk from o + 1 in steps of 2): r = sam[2i], then the Qs of samples i, i + 1, .. while 2k + 1 <
 *                      (int)scale, each taken when |Q| > |r| (strict; a NaN never wins, and nothing beats a NaN r);
 *   spec_dev[row][W]   the green polyline (:534-555) before the caller's column arithmetic (m - 1 + W/2) % W: entry 0 is
 *                      H/2 + (int)(psd[0] * h), entry m is H/2 + (int)(getMax(psd, i, (int)pi) * h) with pi = n / (float)W,
 *                      i = (int)(pi * (float)m), h = (H/2) / -100.0f, getMax (:560-567) from psd[i] with strict >;
 *                      psd is fft.java's formula over dbg, 10f * (float)log10((re^2 + im^2) * (2f/n)^2) -- defined by
 *                      composition, bit for bit: the row jsdr_fft_batch_f32 of a jsdr_fft of n samples writes for the dbg row;
 *   dbg_dev[row][2n]   the dbg row itself.
 * (int) is Java's cast (truncates, saturates, NaN -> 0); the subtraction and the additions wrap as Java's ints do.  row =
 * s * frames + f for frame f of stream s, rows packed; each of the three may be NULL, and with all three NULL the call is the
 * batch call and launches nothing more.  dbg_dev starts on 16 bytes, trace_dev and spec_dev on 4.
 * jsdr_demod_scope_layout (host only, no device) states the two column schedules of (n, width) in the reference's float
 * arithmetic, `width` entries each: trace_first[x] = i and trace_count[x] = (int)scale for x < W - 1 (the last entry is (0, 0));
 * spec_first[m] = i and spec_count[m] = (int)pi for m >= 1 (entry 0 is (0, 0)).  Any of the four may be NULL; cap is the room
 * of each.  JSDR_ERR for n < 1, width outside 1 .. 32768, cap < width, and for a pair at which the reference would index
 * outside sam[] or psd[] (none is known for n up to 20000 and width up to 2n); the scope calls refuse what it refuses.
 * Passes, a chunk of frames at a time: "k_demod_scope_front" (one workgroup a tile: the mixed IQ and the final floats
 * again, from the caller's input, the filter history and FM state of before the call, the call's carrier table and its
 * (max, avg) rows), "k_demod_trace", and for the spectrum the handle's own jsdr_fft (its kernel as jsdr_fft_kernel names it)
 * and "k_demod_spec"; jsdr_demod_scope_kernel joins what the last scope call launched with '+' ("" before the first and after
 * a call with no output).  The rows between the passes belong to the handle: allocated at the first scope call or when a call
 * needs more, counted by jsdr_live_resources, gone with jsdr_demod_destroy, and bounded: a pass takes at most
 * 64 MiB / (16 n + 8) frames (one frame at least), which jsdr_demod_scope_chunk lowers (0: the default).  The schedule table
 * lives on the device and is rebuilt by a kernel on `stream` when width changes; no call after the first with its outputs
 * and size waits for the device.  A handle that makes no scope call allocates and launches what it did before.  Scope
 * calls share those rows, so they belong on one stream at a time, the stream of the handle's batch calls.
 * JSDR_ERR before any device work, handle and state untouched, the message naming the argument: a null handle, input or
 * audio_dev; nsamples not whole frames or above max_batch_samples; a stride that is odd or below 2 * nsamples; width outside
 * 1 .. 32768; height < 0; spec_dev with a frame size jsdr_fft_create refuses (outside 2 .. 20000); a misaligned output; a
 * channel handle (jsdr_demod_create_channels): its channels have no scope yet.
 * (Not covered: channel handles, the host receive_f32 form, the JNI shim and the Java classes.) */
int jsdr_demod_scope_layout(int n, int width, int32_t *trace_first, int32_t *trace_count,
                            int32_t *spec_first, int32_t *spec_count, int cap);
int jsdr_demod_scope_i16(jsdr_demod *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc,
                         int16_t *audio_dev, int64_t audio_stride_i16, int width, int height,
                         int32_t *trace_dev, int32_t *spec_dev, float *dbg_dev, void *stream);
int jsdr_demod_scope_f32(jsdr_demod *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples,
                         int16_t *audio_dev, int64_t audio_stride_i16, int width, int height,
                         int32_t *trace_dev, int32_t *spec_dev, float *dbg_dev, void *stream);
int jsdr_demod_scope_chunk(jsdr_demod *h, int frames_per_pass);   /* 0: the default */
const char *jsdr_demod_scope_kernel(jsdr_demod *h);               /* what the last scope call launched */

/* ------------------------------------------------------------------ formats either side of the path
 * waterfall.paintLine / getMax (waterfall.java:87-109): one pixel row per PSD frame as fft.receive publishes it
 * ("fft-psd", n bins + 2).  step = (float)n/width; pixel p = max of bins [(int)(p*step), +(int)step), mapped
 * 255-(int)(m*-2.55f), clamped to 0..255, scaled into the peak colour (0xRRGGBB, Color.CYAN = 0x00ffff in the
 * reference) with /256, stored at column (p + width/2) % width as ARGB with alpha 0xff.  Bit-exact.          */
int jsdr_waterfall_lines(const float *psd_dev /*[nframes][n+2]*/, int64_t nframes, int n, int width,
                         uint32_t peak_rgb, uint32_t *pix_dev /*[nframes][width]*/, void *stream);

/* IQ recordings -> the stream-major device layout raw[S][stride] of the batch calls.
 * JavaAudio.openFile (JavaAudio.java:369-395): a file AudioSystem reads as PCM_SIGNED 16-bit little-endian with
 * the configured channel count and rate (compareFormat :397-406); RIFF/WAVE is parsed here, other containers and
 * the AudioSystem format conversion are not.  A file without a RIFF header is taken as the headerless dump
 * recorder.receive (recorder.java:66-74) / FCD.main (FCD.java:286-303) write.                                  */
#define JSDR_REC_RAW 0
#define JSDR_REC_WAV 1
typedef struct jsdr_recording_info {
    int format;          /* JSDR_REC_RAW / JSDR_REC_WAV */
    int encoding;        /* WAVE format tag: 1 = PCM */
    int channels, rate, bits;
    int64_t frames;      /* sample frames (one per IQ pair) in the file */
    int64_t data_offset; /* byte offset of the first sample */
} jsdr_recording_info;
int jsdr_recording_probe(const char *path, int raw_channels, jsdr_recording_info *info);
/* loads frames [first_frame, first_frame+nframes) of every file to raw_dev + s*stream_stride_i16 as int16 (I,Q)
 * pairs; a mono file (channels = 1, audio-mode-I) becomes (I,0) pairs -- equal to JavaAudio.java:286-288 as long
 * as the Q correction passed to the kernels is 0; a short file is zero-filled and frames_loaded[s] (optional)
 * says how many frames were real.  Format mismatch -> JSDR_ERR "Incompatible audio format" (:388).             */
int jsdr_recordings_load(const char *const *paths, int nstreams, int channels, int rate, int64_t first_frame,
                         int64_t nframes, int16_t *raw_dev, int64_t stream_stride_i16, int64_t *frames_loaded,
                         void *stream);

/* ------------------------------------------------------------------ one process, several GPUs
 * The reference hosts all its demodulators in one JVM (jsdr.java:479-483: `new FUNcubeBPSKDemod(i, ...)` in a loop) and one
 * audio thread feeds them (JavaAudio.java:298-304).  A group is that across `ndev` GPUs: `total_streams` lock-step
 * demodulators split into contiguous equal shards (device index g owns streams [g S, (g+1) S), S = total_streams / ndev),
 * ONE host thread per device that owns the device's jsdr_bpsk (and, with JSDR_GROUP_WITH_PSD, jsdr_fft) handle and its
 * HIP streams, and after every batch call ONE ncclAllGather per device (RCCL over xGMI, librccl.so loaded at the first
 * create) of the fixed-size per-stream result slots (jsdr_bpsk_pack_slots' layout), on a gather stream of its own beside
 * the next call's kernels.  There is no other exchange: streams are independent.
 *   devices: ndev device ordinals, or NULL for 0 .. ndev-1.
 *   JSDR_GROUP_GATHER_COPY: gather with device-to-device copies instead of RCCL (a host without librccl; or several
 *     group members on ONE device, which RCCL refuses -- the rehearsal a one-GPU box can run).
 * jsdr_group_batch_i16: raw_dev[g] = device g's [S][stream_stride] int16 IQ (on THAT device); psd_dev[g] (optional,
 * WITH_PSD) = float[S * nsamples / n][n + 2] on that device.  Returns when every device thread has enqueued its work;
 * a failure on any device abandons the step's gather on ALL of them (nobody waits in a collective for a rank that is
 * gone) and is reported here.  jsdr_group_sync waits for kernels, tails and gathers of every device.
 * jsdr_group_gathered: device g's copy of ALL total_streams slots, ordered by global stream id.                  */
typedef struct jsdr_group jsdr_group;
#define JSDR_GROUP_GATHER_COPY 1
#define JSDR_GROUP_WITH_PSD 2
int jsdr_group_create(jsdr_group **g, int ndev, const int *devices, int rate, int nsamples_per_frame, int tuning_hz,
                      int do_fft, int do_up, int total_streams, int64_t max_batch_samples, int flags);
int jsdr_group_destroy(jsdr_group *g);
int jsdr_group_info(jsdr_group *g, int *ndev, int *streams_per_device, int64_t *slot_bytes, int *rccl_version);
int jsdr_group_device(jsdr_group *g, int index, int *device, jsdr_bpsk **dem, jsdr_fft **fft);
int jsdr_group_batch_i16(jsdr_group *g, const int16_t *const *raw_dev, int64_t stream_stride_i16, int64_t nsamples,
                         int ic, int qc, float *const *psd_dev);
int jsdr_group_sync(jsdr_group *g);
int jsdr_group_gathered(jsdr_group *g, int index, const uint8_t **slots_dev, int64_t *bytes);
int jsdr_group_read_slot(jsdr_group *g, int index, int stream, uint8_t *slot_host);
/* jsdr_bpsk_set_tuning / jsdr_bpsk_set_mode on every member, after the group's pending steps; every member is checked
 * before any is changed */
int jsdr_group_set_tuning(jsdr_group *g, double tuning_hz);
int jsdr_group_set_mode(jsdr_group *g, int do_fft, int do_up);

#ifdef __cplusplus
}
#endif
#endif /* JSDR_HIP_H */
