/*
 * vfwave.h -- C ABI of VoiceFilter's two waveform ends in libdptnav.so (gfx950): the mixture waveform to the normalised
 * dB magnitude and the unit phasor that VoiceFilter.forward takes, and the predicted magnitudes back to waveforms on the
 * mixture's phase.
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   get_magnitude: STFT, abs, clamp, log10, scale, clamp, angle                 src/datasets/base_dataset.py:167-180  -> vfwave_analysis
 *   nothing: the reference never turns s*_spec_pred back into audio; the inverse is the reconstruction of the VoiceFilter
 *   code base that get_magnitude was copied from (reference level 20 dB, floor -100 dB)                               -> vfwave_synthesis
 *
 * With S the one-sided Hann STFT of include/specfe.h (n_fft = N, hop = H, F = N / 2 + 1, W = 1 + T / H frames):
 *   spec[b][f][w]        = clamp((20 log10(max(|S|, 1e-5)) - 20) / 100, -1, 0) + 1          in [0, 1]
 *   phasor[b][0|1][f][w] = (Re S, Im S) / |S|, and (1, 0) exactly where |S| == 0 (angle(0) = 0)
 *   mag                  = 10^(5 clamp(p, 0, 1) - 4)                                         in [1e-4, 10]
 *   X                    = mag (phasor[0] + i phasor[1])
 *   y                    = specfe_istft(X, length): Im of bins 0 and N / 2 ignored, division by the envelope, the same
 *                          behaviour for a length beyond the natural (W - 1) H
 * Both maps are frequency-major, [F][W]: the layout of VoiceFilter's input and outputs.  The two clamps lose information
 * by the reference's convention: a bin with |S| < 1e-4 comes back as 1e-4, one with |S| > 10 as 10.
 *
 * Conventions: those of include/specfe.h.  The handle IS a specfe handle (specfe_create / specfe_destroy; any accepted
 * n_fft and hop).  Tensor arguments are DEVICE pointers to contiguous fp32 owned by the caller, 4-byte aligned; a call
 * allocates nothing, needs no scratch, enqueues ONE launch on `stream` (a hipStream_t) and never synchronises.  Nothing
 * is summed with atomics and every sum has a fixed order: two calls on the same inputs give bitwise-equal outputs, an
 * item's outputs do not depend on the rest of the batch, and a source's waveform does not depend on n_src.
 * VFWAVE_ERR_INVALID launches nothing and leaves every output untouched.
 * Sizes: 1 <= B < 2^20, T and every output length below 2^27, a launch grid below 2^31 workgroups, 1 <= n_src <= 4.
 */
#ifndef VFWAVE_H_
#define VFWAVE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VFWAVE_ABI_VERSION 1
#define VFWAVE_MAX_SRC 4

/* error codes (same values as specfe.h) */
#define VFWAVE_OK 0
#define VFWAVE_ERR_INVALID 1      /* bad argument: nothing was launched */
#define VFWAVE_ERR_HIP 4          /* the launch failed */

int vfwave_abi_version(void);
const char* vfwave_strerror(int code);

/* x [B][T] -> spec [B][F][W], phasor [B][2][F][W], W = 1 + T / hop.  Needs T > n_fft / 2. */
int vfwave_analysis(void* handle, const float* x, int B, int64_t T, float* spec, float* phasor, void* stream);

/*
 * pred [n_src][B][F][W], phasor [B][2][F][W] (shared by the n_src maps of an item) -> y [n_src][B][L]; L = length if
 * length > 0, else the natural (W - 1) hop (which must be >= 1).  A length beyond the natural one reads on into the last
 * half window; y[j] = 0 for j >= (W - 1) hop + n_fft / 2.
 */
int vfwave_synthesis(void* handle, const float* pred, const float* phasor, int n_src, int B, int64_t W, int64_t length, float* y,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VFWAVE_H_ */
