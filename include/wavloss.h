/*
 * wavloss.h -- C ABI of the waveform criteria in libdptnav.so (gfx950): MAE / MSE / SI-SNR under batch-level or
 * utterance-level permutation-invariant training (PIT), forward AND backward, two speakers.
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   BaseSSLoss.forward (batch-level PIT)       src/loss/ss_losses.py:21-26     -> wavloss_pit_loss, WAVLOSS_PIT_BATCH
 *   MAEWavLoss (nn.L1Loss, reduction "mean")   src/loss/ss_losses.py:65-77     -> kind WAVLOSS_MAE
 *   MSEWavLoss (nn.MSELoss, reduction "mean")  src/loss/ss_losses.py:80-93     -> kind WAVLOSS_MSE
 *   SiSNRLoss                                  src/loss/ss_losses.py:100-114   -> kind WAVLOSS_SISNR
 *   SiSNRWavLoss                               src/loss/ss_losses.py:117-130   -> kind WAVLOSS_SISNR
 *   loss.backward() through the criterion      src/trainer/trainer.py:44       -> d_s1_pred / d_s2_pred of the same call
 *   WAVLOSS_PIT_UTTERANCE has no counterpart there: it is the reference's class applied to every item alone (B = 1
 *   slices) and averaged over the batch.
 *   The Python classes speech_separation_amd.MAEWavLoss / MSEWavLoss / SiSNRWavLoss call the entry points below through
 *   ctypes with raw device pointers.
 *
 * Conventions (as include/dptnav.h): plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by the
 * caller, with no alignment requirement beyond that of a float; the unit is stateless (no handle, no weights), allocates
 * nothing, enqueues its two launches on `stream` (a hipStream_t) and never synchronises the device or the host; every
 * function returns 0 on success and a WAVLOSS_ERR_* code on error (message: wavloss_strerror).  Nothing is summed with
 * atomics: two calls on the same inputs give bitwise-equal outputs.
 */
#ifndef WAVLOSS_H_
#define WAVLOSS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WAVLOSS_ABI_VERSION 1

/* error codes (same values as dptnav.h) */
#define WAVLOSS_OK 0
#define WAVLOSS_ERR_INVALID 1     /* bad argument, scratch too small or misaligned included: nothing was launched */
#define WAVLOSS_ERR_SCRATCH 2     /* kept for value parity with the other headers; scratch faults report ERR_INVALID */
#define WAVLOSS_ERR_HIP 4         /* a launch failed */

/* element loss l_i(p, s) of item i (ss_losses.py:65-93, :100-114) */
#define WAVLOSS_MAE 0             /* mean_t |p_it - s_it| */
#define WAVLOSS_MSE 1             /* mean_t (p_it - s_it)^2 */
#define WAVLOSS_SISNR 2           /* zero-mean, -20 log10(|a s|^2 / |p - a s|^2), a = <p,s> / |s|^2; needs T >= 2 */

/* where the speaker permutation is resolved */
#define WAVLOSS_PIT_BATCH 0       /* ss_losses.py:21-26: one permutation for the batch, from the two batch means */
#define WAVLOSS_PIT_UTTERANCE 1   /* one permutation per item, from the item's own four terms */

int wavloss_abi_version(void);
const char* wavloss_strerror(int code);

/* Scratch of one call on B items (the per-item statistics of the first launch); 0 if B < 1.  A multiple of 8. */
size_t wavloss_scratch_bytes(int B);

/*
 * BaseSSLoss.forward over MAEWavLoss / MSEWavLoss / SiSNRWavLoss (ss_losses.py:21-26, :65-93, :100-114, :117-130) and
 * its backward, on predictions and targets [B][T].
 *   permutation 0 pairs (s1_pred, s1) (s2_pred, s2); permutation 1 pairs (s1_pred, s2) (s2_pred, s1)
 *   L0 = (mean_i l_i(p1,s1) + mean_i l_i(p2,s2)) / 2, L1 likewise with the targets swapped
 *   batch level:      loss = L1 if L1 < L0 (strictly, ss_losses.py:24) else L0; every item is on that permutation
 *   utterance level:  item i is on permutation 1 iff (l_i(p1,s2) + l_i(p2,s1)) / 2 < (l_i(p1,s1) + l_i(p2,s2)) / 2
 *                     (strictly); loss = mean_i of the chosen value
 *   d_s1_pred, d_s2_pred [B][T], overwritten: grad_scale * d loss / d prediction
 *       MAE    w sign(p - s), w = 1 / (2 B T), sign(0) = 0 (torch's L1 backward)
 *       MSE    w 2 (p - s)
 *       SI-SNR w (-20 / ln 10) (2 s~ / <p~,s~> - 2 e / |e|^2), w = 1 / (2 B), s~ p~ zero-mean, e = p~ - a s~
 *   loss_out [4]: loss, number of items on permutation 1, L0, L1 (L0 and L1 are the batch-level values in both modes)
 *   perm_out [B]: permutation of every item (batch level: the same value B times)
 *   scratch: >= wavloss_scratch_bytes(B) bytes, 8-byte aligned
 * Any T >= 1 (SI-SNR: T >= 2) and any B >= 1 below 2^20 with B * T below 2^32 (what one launch can carry).  A silent (constant) SI-SNR target is 0/0 in the
 * reference too (ss_losses.py:106): the nan / inf it gives there is reproduced here, not handled.
 * WAVLOSS_ERR_INVALID (B < 1, T < 1, a null pointer, an unknown kind or level, SI-SNR with T < 2, a scratch that is too
 * small or misaligned) launches nothing and leaves every output untouched.
 */
int wavloss_pit_loss(int kind, int level, const float* s1_pred, const float* s2_pred, const float* s1, const float* s2,
                     int B, int64_t T, float grad_scale, float* d_s1_pred, float* d_s2_pred, float* loss_out,
                     int32_t* perm_out, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAVLOSS_H_ */
