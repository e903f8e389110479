/*
 * wavmetric.h -- C ABI of the evaluation metrics in libdptnav.so (gfx950): SI-SDR and STOI / ESTOI of the four
 * (prediction, target) pairs of a two-speaker batch, computed on the device.
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   SISDRMetric (torchmetrics ScaleInvariantSignalDistortionRatio)         src/metrics/si_sdr.py   -> wavmetric_sisdr_pairs
 *   STOIMetric  (torchmetrics ShortTimeObjectiveIntelligibility -> pystoi) src/metrics/stoi.py     -> wavmetric_stoi_pairs
 *   The batch means and the batch-level permutation of SS2BaseMetric.forward (src/metrics/base_metric.py) stay on the
 *   host: speech_separation_amd.STOIMetric / SISDRMetric reduce the B x 4 values these calls leave on the device.
 *
 * STOI is Taal et al. 2011, ESTOI Jensen & Taal 2016, as pystoi implements them: resample to 10 kHz, drop the frames
 * of the clean signal more than 40 dB below its loudest frame (the processed signal loses the same frames), STFT
 * (frame 256, hop 128, 512-point DFT), 15 one-third octave bands from 150 Hz, correlation over segments of 30 frames.
 * pystoi is not a dependency; the definition the kernels are held to is the fp64 restatement tests/stoi_ref.py, which
 * fixes the points on which pystoi releases differ: frames start at 0, 128, ... <= len - 256
 * with the last full frame included, in the silent-frame removal and in the STFT; the resampler is the polyphase FIR
 * below; EPS is 2^-52 at every precision.
 *   resampler: p / q = 10000 / fs in lowest terms, fc = 1 / (2 max(p, q)), L = ceil(52 / (28.714 fc / 10)),
 *     h[t] = kaiser(2 L + 1, 0.1102 * 51.3)[t + L] * 2 p fc sinc(2 fc t), g = p h / sum(h),
 *     y[m] = sum_j g[L + m q - j p] x[j] for m < ceil(T p / q)   (scipy.signal.resample_poly(x, p, q, window = h / sum h))
 *
 * Conventions (as include/wavloss.h): plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by the
 * caller, with no alignment requirement beyond that of a float; a call allocates nothing, enqueues its launches on
 * `stream` (a hipStream_t) and never synchronises the device or the host (wavmetric_stoi_create / _destroy excepted:
 * they allocate, fill and free the handle's device constants).  The number of launches depends on B, T and fs alone.
 * Every function that returns int returns 0 on success and a WAVMETRIC_ERR_* code on error (message:
 * wavmetric_strerror).  Nothing is summed with atomics: two calls on the same inputs give bitwise-equal outputs.
 */
#ifndef WAVMETRIC_H_
#define WAVMETRIC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WAVMETRIC_ABI_VERSION 1

/* error codes (same values as dptnav.h) */
#define WAVMETRIC_OK 0
#define WAVMETRIC_ERR_INVALID 1   /* bad argument, scratch too small or misaligned included: nothing was launched */
#define WAVMETRIC_ERR_HIP 4       /* an allocation, a copy or a launch failed */

int wavmetric_abi_version(void);
const char* wavmetric_strerror(int code);

/*
 * SI-SDR of the pairs (s1_pred, s1) (s1_pred, s2) (s2_pred, s1) (s2_pred, s2) of every item, in dB: torchmetrics'
 * ScaleInvariantSignalDistortionRatio() with its defaults (no mean removal).  With eps = FLT_EPSILON:
 *   a = (<p, t> + eps) / (<t, t> + eps),   value = 10 log10((|a t|^2 + eps) / (|a t - p|^2 + eps))
 * Sums are double precision in a fixed order.  Inputs [B][T], out [B][4].  Stateless, one launch.
 * WAVMETRIC_ERR_INVALID: a null pointer, B < 1 or B >= 2^20, T < 1.
 */
int wavmetric_sisdr_pairs(const float* s1_pred, const float* s2_pred, const float* s1, const float* s2, int B, int64_t T,
                          float* out, void* stream);

/*
 * A STOI (extended == 0) or ESTOI (extended != 0) evaluator for signals sampled at fs = 8000, 10000 or 16000 Hz (any
 * other rate: WAVMETRIC_ERR_INVALID, *handle untouched).  The handle owns the device constants -- resampling taps,
 * window, DFT twiddles, band edges -- computed on the host in double and rounded once; it lives on the device that is
 * current at creation and may be used from any stream of it, by one call at a time per scratch buffer.
 */
int wavmetric_stoi_create(int fs, int extended, void** handle);
void wavmetric_stoi_destroy(void* handle);

/* Scratch of one wavmetric_stoi_pairs call on [B][T] inputs; a multiple of 16; 0 for a null handle, B < 1 or T < 1. */
size_t wavmetric_stoi_scratch_bytes(void* handle, int B, int64_t T);

/*
 * out [B][4]: STOI (ESTOI for an extended handle) of the pairs (s1_pred, s1) (s1_pred, s2) (s2_pred, s1) (s2_pred, s2)
 *   of every item; the target is the clean signal of its pair.  Fewer than 30 frames after the silent-frame removal give
 *   1e-5 (pystoi's warning path); an all-zero target gives 0.
 * kept [B][2] (int32): the number of frames of item b that survive the silent-frame removal under target s1 / s2.
 * scratch: >= wavmetric_stoi_scratch_bytes(handle, B, T) bytes, 16-byte aligned.
 * Three launches at fs = 10000, four otherwise.  Any T >= 1 below 2^27 and any B >= 1 below 2^20 whose launches fit
 * (B * 6 * ceil(frames / 64) below 2^31).
 * WAVMETRIC_ERR_INVALID (a null handle or pointer, B or T out of range, a scratch that is too small or misaligned)
 * launches nothing and leaves every output untouched.
 */
int wavmetric_stoi_pairs(void* handle, const float* s1_pred, const float* s2_pred, const float* s1, const float* s2, int B,
                         int64_t T, float* out, int32_t* kept, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAVMETRIC_H_ */
