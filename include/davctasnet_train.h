/*
 * davctasnet_train.h -- C ABI of the deep audio-visual Conv-TasNet training step in libdptnav.so (gfx950).
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   model         DeepAVConvTasNet.forward + autograd backward  src/model/deepavconvtasnet.py  -> davtrain_train_forward,
 *                                                                                             davtrain_train_backward
 *   clip          clip_grad_norm_(params, max_grad_norm)  src/trainer/base_trainer.py:383-391  -> davtrain_grad_clip
 *   optimizer     torch.optim.AdamW                       src/configs/deepavconvtasnet.yaml    -> davtrain_adamw_step
 *   The Python module speech_separation_amd.TrainableDeepAVConvTasNet calls the entry points below through ctypes.  The
 *   inference forward stays in dctasnet.h (av = 1) and the audio-only training step in dctasnet_train.h; this header adds the
 *   audio-visual training step next to them and changes nothing there.
 *
 * Conventions (as dctasnet_train.h): C99, plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by
 * the caller; the library allocates nothing on the hot path (the caller passes a workspace of davtrain_workspace_bytes(),
 * 256-byte aligned, which also holds the tape between train_forward and train_backward); work is enqueued on `stream`
 * (a hipStream_t) and nothing synchronises the device; every function returns 0 on success and a DAVTRAIN_ERR_* code on
 * error (message: davtrain_last_error).  A handle is bound to the device current at davtrain_create() and is not
 * thread-safe.  Every reduction runs in a fixed order without atomics: two backward calls on the same tape give
 * bitwise-identical gradients.  The speaker embeddings e1, e2 [B][512][Tv] come from a frozen lip-reader: they get no
 * gradient.
 */
#ifndef DAVCTASNET_TRAIN_H_
#define DAVCTASNET_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAVTRAIN_ABI_VERSION 1

/* error codes (same values as dctasnet_train.h) */
#define DAVTRAIN_OK 0
#define DAVTRAIN_ERR_INVALID 1     /* bad argument / unsupported shape */
#define DAVTRAIN_ERR_WORKSPACE 2   /* workspace too small or misaligned */
#define DAVTRAIN_ERR_WEIGHTS 3     /* weights or gradients not bound / wrong count */
#define DAVTRAIN_ERR_HIP 4         /* a HIP call or launch failed */

typedef struct davtrain_ctx* davtrain_handle;

int davtrain_abi_version(void);

/* The model is fixed by the reference (N=512, B=128, H=512, X=8, P=3, R=3, L=16, video_emb_size = hidden_video = 512).
 * Fails without a HIP device. */
int davtrain_create(davtrain_handle* out);
void davtrain_destroy(davtrain_handle h);
/* last error of `h`; h == NULL: the last davtrain_create() failure of this thread */
const char* davtrain_last_error(davtrain_handle h);

/* Weight table in the reference's state_dict() order (376 tensors, the table of dctasnet_create(.., 1): the audio-only
 * table, then visual_compression.{weight,bias}, video_ln.{weight,bias}). */
int davtrain_num_weights(davtrain_handle h);
const char* davtrain_weight_name(davtrain_handle h, int i);
int64_t davtrain_weight_numel(davtrain_handle h, int i);
/* Borrow `n` device pointers (state_dict order).  The step reads them as they are at launch time: nothing derived from
 * them is cached, so an optimizer step or load_state_dict in place is seen by the next call. */
int davtrain_bind_weights(davtrain_handle h, const float* const* dev_ptrs, int n);
/* Borrow `n` device pointers the backward WRITES (overwrites) the gradient of each weight into (state_dict order). */
/* decoder.deconv.weight is a parameter the reference's forward never reads: its buffer is never written (it keeps what
 * the caller put there: zeros) and davtrain_adamw_step never changes the weight. */
int davtrain_bind_grads(davtrain_handle h, float* const* dev_ptrs, int n);

/* Flat layout of gradients / optimizer state: slot i starts at offset(i) floats (64-float aligned, zero padding);
 * offset(num_weights) is the total. */
int64_t davtrain_flat_offset(davtrain_handle h, int slot);
int64_t davtrain_flat_numel(davtrain_handle h);

/* Encoder frames F = (T + 16) / 16 + 1 and output length 16 * (T / 16); 0 if T < 16. */
int64_t davtrain_frames(int64_t T);
int64_t davtrain_out_len(int64_t T);
/* Workspace (tape + scratch) of one step of B mixtures of T samples with Tv >= 1 video frames; 0 for an unsupported
 * shape. */
size_t davtrain_workspace_bytes(davtrain_handle h, int B, int64_t T, int Tv);

/* Forward that records its tape in `ws`: mix [B][T], e1, e2 [B][512][Tv] -> s1_pred, s2_pred [B][davtrain_out_len(T)],
 * bitwise equal to dctasnet_forward (av = 1) with the same weights.  NULL embeddings or Tv < 1: DAVTRAIN_ERR_INVALID. */
int davtrain_train_forward(davtrain_handle h, const float* mix, const float* e1, const float* e2, int B, int64_t T, int Tv,
                           float* s1_pred, float* s2_pred, void* ws, size_t ws_bytes, void* stream);
/* Introspection for tests and tools: byte offset in the workspace of a tensor the last davtrain_train_forward of
 * B x T x Tv left on the tape, or -1.  V1, U, SKIP, ENC_Z, DEC_Z as dcttrain_tape_offset.  VCAT: vcat[b * Tv + t][512] fp32,
 * the two speakers' compressed embeddings (visual_compression) side by side, before the interpolation to F frames
 * (`block` is ignored). */
#define DAVTRAIN_TAPE_V1 0
#define DAVTRAIN_TAPE_U 1
#define DAVTRAIN_TAPE_SKIP 2
#define DAVTRAIN_TAPE_ENC_Z 3
#define DAVTRAIN_TAPE_DEC_Z 4
#define DAVTRAIN_TAPE_VCAT 5
int64_t davtrain_tape_offset(davtrain_handle h, int B, int64_t T, int Tv, int which, int block);
/* Backward of the last davtrain_train_forward on this workspace (same mix, e1, e2, B, T, Tv): d loss / d s1_pred,
 * d_s2_pred [B][out_len] -> every bound gradient buffer (overwritten), except decoder.deconv.weight's. */
int davtrain_train_backward(davtrain_handle h, const float* mix, const float* e1, const float* e2, int B, int64_t T, int Tv,
                            const float* d_s1, const float* d_s2, void* ws, size_t ws_bytes, void* stream);

/* clip_grad_norm_ over a flat gradient (davtrain_flat_numel floats): scale in place when max_norm > 0; the pre-clip norm
 * goes to norm_out[0].  scratch: davtrain_clip_scratch_bytes(), 8-byte aligned. */
size_t davtrain_clip_scratch_bytes(davtrain_handle h);
int davtrain_grad_clip(davtrain_handle h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                       float* norm_out, void* stream);
/* torch.optim.AdamW step (amsgrad / maximize off) of the bound weights, gradient and state in the flat layout.
 * decoder.deconv.weight is skipped: torch.optim.AdamW skips a parameter whose .grad is None, weight decay included. */
int davtrain_adamw_step(davtrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                        double beta1, double beta2, double eps, double weight_decay, int step, void* stream);

/* Cost model of one mixture's training step (forward + backward): algorithmic FLOPs, 2 per MAC: 3 x
 * dctasnet_flops_per_mixture.  The video head is left out, as there. */
double davtrain_flops_per_mixture(davtrain_handle h, int64_t T);

#ifdef __cplusplus
}
#endif
#endif /* DAVCTASNET_TRAIN_H_ */
