/*
 * dctasnet_train.h -- C ABI of the deep Conv-TasNet training step in libdptnav.so (gfx950).
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   model         DeepConvTasNet.forward + autograd backward  src/model/deepconvtasnet.py   -> dcttrain_train_forward,
 *                                                                                           dcttrain_train_backward
 *   clip          clip_grad_norm_(params, max_grad_norm)  src/trainer/base_trainer.py:383-391 -> dcttrain_grad_clip
 *   optimizer     torch.optim.AdamW                       src/configs/deepconvtasnet.yaml    -> dcttrain_adamw_step
 *   The Python module speech_separation_amd.TrainableDeepConvTasNet calls the entry points below through ctypes.  The inference
 *   forward stays in dctasnet.h (DeepConvTasNet); this header adds the training step next to it and changes nothing there.
 *
 * Conventions (as dctasnet.h): C99, plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by the
 * caller; the library allocates nothing on the hot path (the caller passes a workspace of dcttrain_workspace_bytes(),
 * 256-byte aligned, which also holds the tape between train_forward and train_backward); work is enqueued on `stream`
 * (a hipStream_t) and nothing synchronises the device; every function returns 0 on success and a DCTTRAIN_ERR_* code on
 * error (message: dcttrain_last_error).  A handle is bound to the device current at dcttrain_create() and is not
 * thread-safe.  Every reduction runs in a fixed order without atomics: two backward calls on the same tape give
 * bitwise-identical gradients.
 */
#ifndef DCTASNET_TRAIN_H_
#define DCTASNET_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCTTRAIN_ABI_VERSION 1

/* error codes (same values as dctasnet.h) */
#define DCTTRAIN_OK 0
#define DCTTRAIN_ERR_INVALID 1     /* bad argument / unsupported shape */
#define DCTTRAIN_ERR_WORKSPACE 2   /* workspace too small or misaligned */
#define DCTTRAIN_ERR_WEIGHTS 3     /* weights or gradients not bound / wrong count */
#define DCTTRAIN_ERR_HIP 4         /* a HIP call or launch failed */

typedef struct dcttrain_ctx* dcttrain_handle;

int dcttrain_abi_version(void);

/* The model is fixed by the reference (N=512, B=128, H=512, X=8, P=3, R=3, L=16).  av = 0: DeepConvTasNet.  av != 0
 * (DeepAVConvTasNet) fails with DCTTRAIN_ERR_INVALID: the audio-visual training step is not built.  Fails without a HIP
 * device. */
int dcttrain_create(dcttrain_handle* out, int av);
void dcttrain_destroy(dcttrain_handle h);
/* last error of `h`; h == NULL: the last dcttrain_create() failure of this thread */
const char* dcttrain_last_error(dcttrain_handle h);

/* Weight table in the reference's state_dict() order (372 tensors, the audio-only table of dctasnet.h). */
int dcttrain_num_weights(dcttrain_handle h);
const char* dcttrain_weight_name(dcttrain_handle h, int i);
int64_t dcttrain_weight_numel(dcttrain_handle h, int i);
/* Borrow `n` device pointers (state_dict order).  The step reads them as they are at launch time: nothing derived from
 * them is cached, so an optimizer step or load_state_dict in place is seen by the next call. */
int dcttrain_bind_weights(dcttrain_handle h, const float* const* dev_ptrs, int n);
/* Borrow `n` device pointers the backward WRITES (overwrites) the gradient of each weight into (state_dict order). */
/* decoder.deconv.weight is a parameter the reference's forward never reads: its buffer is never written (it keeps what
 * the caller put there: zeros) and dcttrain_adamw_step never changes the weight. */
int dcttrain_bind_grads(dcttrain_handle h, float* const* dev_ptrs, int n);

/* Flat layout of gradients / optimizer state: slot i starts at offset(i) floats (64-float aligned, zero padding);
 * offset(num_weights) is the total. */
int64_t dcttrain_flat_offset(dcttrain_handle h, int slot);
int64_t dcttrain_flat_numel(dcttrain_handle h);

/* Encoder frames F = (T + 16) / 16 + 1 and output length 16 * (T / 16); 0 if T < 16. */
int64_t dcttrain_frames(int64_t T);
int64_t dcttrain_out_len(int64_t T);
/* Workspace (tape + scratch) of one step of B mixtures of T samples; 0 for an unsupported shape. */
size_t dcttrain_workspace_bytes(dcttrain_handle h, int B, int64_t T);

/* Forward that records its tape in `ws`: mix [B][T] -> s1_pred, s2_pred [B][dcttrain_out_len(T)], bitwise equal to
 * dctasnet_forward with the same weights. */
int dcttrain_train_forward(dcttrain_handle h, const float* mix, int B, int64_t T, float* s1_pred, float* s2_pred, void* ws,
                          size_t ws_bytes, void* stream);
/* Introspection for tests and tools: byte offset in the workspace of a tensor the last dcttrain_train_forward of B x T left
 * on the tape, or -1.  V1, U (Separator block `block`) and SKIP (block 0 only) as cttrain_tape_offset.  ENC_Z: the
 * pre-activation (input of the PReLU) of dense encoder layer `block` (0..3), [B * F][512] fp32, frame-major; DEC_Z: that of
 * dense decoder layer `block` (0..3), [2 * B * F][512], rows in (b, f, speaker) order. */
#define DCTTRAIN_TAPE_V1 0
#define DCTTRAIN_TAPE_U 1
#define DCTTRAIN_TAPE_SKIP 2
#define DCTTRAIN_TAPE_ENC_Z 3
#define DCTTRAIN_TAPE_DEC_Z 4
int64_t dcttrain_tape_offset(dcttrain_handle h, int B, int64_t T, int which, int block);
/* Backward of the last dcttrain_train_forward on this workspace (same mix, B, T): d loss / d s1_pred, d_s2_pred
 * [B][out_len] -> every bound gradient buffer (overwritten). */
int dcttrain_train_backward(dcttrain_handle h, const float* mix, int B, int64_t T, const float* d_s1, const float* d_s2,
                           void* ws, size_t ws_bytes, void* stream);

/* clip_grad_norm_ over a flat gradient (dcttrain_flat_numel floats): scale in place when max_norm > 0; the pre-clip norm
 * goes to norm_out[0].  scratch: dcttrain_clip_scratch_bytes(), 8-byte aligned. */
size_t dcttrain_clip_scratch_bytes(dcttrain_handle h);
int dcttrain_grad_clip(dcttrain_handle h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                      float* norm_out, void* stream);
/* torch.optim.AdamW step (amsgrad / maximize off) of the bound weights, gradient and state in the flat layout.
 * decoder.deconv.weight is skipped: torch.optim.AdamW skips a parameter whose .grad is None, weight decay included. */
int dcttrain_adamw_step(dcttrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                       double beta1, double beta2, double eps, double weight_decay, int step, void* stream);

/* Cost model of one mixture's training step (forward + backward): algorithmic FLOPs, 2 per MAC: 3 x dctasnet_flops_per_mixture. */
double dcttrain_flops_per_mixture(dcttrain_handle h, int64_t T);

#ifdef __cplusplus
}
#endif
#endif /* DCTASNET_TRAIN_H_ */
