/*
 * specfe.h -- C ABI of the spectral front end in libdptnav.so (gfx950): STFT, inverse STFT, their two adjoints and the
 * log-mel spectrogram, computed on the device.
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   STFT.stft (torch.stft + stack + transpose + contiguous -> [B, 2, T, F])   src/encoders/stft.py:25-38        -> specfe_stft
 *   AudioDecoder's torch.istft(n_fft, hop, hann window, length)               src/model/rtfsnet.py:843-849      -> specfe_istft
 *   loss.backward() through either                                            src/trainer/trainer.py:44         -> specfe_*_backward
 *   get_spectrogram: log(clamp(MelSpectrogram(sample_rate=16000)(x), 1e-5))   src/datasets/base_dataset.py:115-123,165 -> specfe_logmel
 *
 * The transform, for n_fft = N, hop = H, F = N / 2 + 1 (torch.stft / torch.istft with win_length = N, the periodic Hann
 * window w[t] = 0.5 - 0.5 cos(2 pi t / N), center = True with reflect padding, one-sided, not normalised):
 *   xp = x reflect-padded by N / 2 on both sides, M = 1 + T / H frames (integer division), T > N / 2
 *   X[b][0][m][k] =  sum_t w[t] xp[m H + t] cos(2 pi k t / N)
 *   X[b][1][m][k] = -sum_t w[t] xp[m H + t] sin(2 pi k t / N)
 *   r_m[t] = (1 / N) [Re X_0 + (-1)^t Re X_{N/2} + 2 sum_{0<k<N/2} (Re X_k cos(2 pi k t / N) - Im X_k sin(2 pi k t / N))]
 *   z[n] = sum_m w[n - m H] r_m[n - m H],  env[n] = sum_m w[n - m H]^2,  y[j] = z[N / 2 + j] / env[N / 2 + j]
 * The imaginary parts of bins 0 and N / 2 do not enter the inverse (torch.istft ignores them exactly).
 *
 * Log-mel: torchaudio's MelSpectrogram defaults at sample_rate sr -- power 2, f_min 0, f_max sr / 2, HTK scale, no norm:
 *   mel(f) = 2595 log10(1 + f / 700); n_mels + 2 points equally spaced in mel between mel(0) and mel(sr / 2), mapped back to
 *   Hz as f_0 .. f_{n_mels+1}; with g_k = k (sr / 2) / (F - 1) the filter of band j at bin k is
 *   max(0, min((g_k - f_j) / (f_{j+1} - f_j), (f_{j+2} - g_k) / (f_{j+2} - f_{j+1})))
 *   S[b][j][m] = log(max(sum_k fb[k][j] (Re X[m][k]^2 + Im X[m][k]^2), 1e-5))
 * torchaudio is not a dependency and the parity of this one table with torchaudio's is UNPINNED: the definition the
 * kernel is held to is the fp64 restatement tests/spec_ref.py.
 *
 * Conventions (as include/wavmetric.h): plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by
 * the caller, with no alignment requirement beyond that of a float; a call allocates nothing, needs no scratch, enqueues
 * ONE launch on `stream` (a hipStream_t) and never synchronises the device or the host (specfe_create* / _destroy
 * excepted: they allocate, fill and free the handle's device constants).  Every function that returns int returns 0 on
 * success and a SPECFE_ERR_* code on error (message: specfe_strerror).  Nothing is summed with atomics and every sum has a
 * fixed order: two calls on the same inputs give bitwise-equal outputs, and an item's outputs do not depend on the rest
 * of the batch.  SPECFE_ERR_INVALID launches nothing and leaves every output untouched.
 * Sizes: 1 <= B < 2^20, T and every output length below 2^27, and a launch grid below 2^31 workgroups.
 */
#ifndef SPECFE_H_
#define SPECFE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPECFE_ABI_VERSION 1

/* error codes (same values as dptnav.h) */
#define SPECFE_OK 0
#define SPECFE_ERR_INVALID 1      /* bad argument: nothing was launched */
#define SPECFE_ERR_HIP 4          /* an allocation, a copy or a launch failed */

int specfe_abi_version(void);
const char* specfe_strerror(int code);

/*
 * A transform of size n_fft with hop `hop`.  The handle owns the device constants -- window, the cos / -sin tables in
 * the layout of the MFMA B operand, one period of cos / sin for the gathers, the mel filterbank of specfe_create_mel --
 * computed on the host in double and rounded once; it lives on the device that is current at creation and may be used
 * from any stream of it.  Accepted: n_fft a multiple of 16 in [32, 512], 1 <= hop <= n_fft / 2; specfe_create_mel also
 * needs sample_rate >= 2 and 1 <= n_mels <= 256.  Anything else: SPECFE_ERR_INVALID, *handle untouched.
 */
int specfe_create(int n_fft, int hop, void** handle);
int specfe_create_mel(int n_fft, int hop, int sample_rate, int n_mels, void** handle);
void specfe_destroy(void* handle);

/* x [B][T] -> X [B][2][M][F], M = 1 + T / hop.  Needs T > n_fft / 2. */
int specfe_stft(void* handle, const float* x, int B, int64_t T, float* X, void* stream);

/* The adjoint of specfe_stft: gX [B][2][M][F] (M = 1 + T / hop) -> gx [B][T], overwritten, the reflected ends folded back. */
int specfe_stft_backward(void* handle, const float* gX, int B, int64_t T, float* gx, void* stream);

/*
 * X [B][2][M][F] -> y [B][L]; L = length if length > 0, else the natural (M - 1) hop (which must be >= 1).  A length
 * beyond the natural one reads on into the last half window, as torch.istft does; y[j] = 0 for j >= (M - 1) hop + n_fft / 2.
 */
int specfe_istft(void* handle, const float* X, int B, int64_t M, int64_t length, float* y, void* stream);

/* The adjoint of specfe_istft: gy [B][L] (L as above) -> gX [B][2][M][F], overwritten; Im of bins 0 and n_fft / 2 gets 0. */
int specfe_istft_backward(void* handle, const float* gy, int B, int64_t M, int64_t length, float* gX, void* stream);

/* x [B][T] -> S [B][n_mels][M], M = 1 + T / hop, one pass.  The handle must come from specfe_create_mel; T > n_fft / 2. */
int specfe_logmel(void* handle, const float* x, int B, int64_t T, float* S, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPECFE_H_ */
