/*
 * ctasnet_train.h -- C ABI of the Conv-TasNet training step in libdptnav.so (gfx950).
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   model         ConvTasNet.forward + autograd backward  src/model/convtasnet.py:1-116   -> cttrain_train_forward,
 *                                                                                           cttrain_train_backward
 *   clip          clip_grad_norm_(params, max_grad_norm)  src/trainer/base_trainer.py:383-391 -> cttrain_grad_clip
 *   optimizer     torch.optim.AdamW                       src/configs/convtasnet.yaml     -> cttrain_adamw_step
 *   The Python module speech_separation_amd.TrainableConvTasNet calls the entry points below through ctypes.  The inference
 *   forward stays in ctasnet.h (ConvTasNet); this header adds the training step next to it and changes nothing there.
 *
 * Conventions (as ctasnet.h): C99, plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by the
 * caller; the library allocates nothing on the hot path (the caller passes a workspace of cttrain_workspace_bytes(),
 * 256-byte aligned, which also holds the tape between train_forward and train_backward); work is enqueued on `stream`
 * (a hipStream_t) and nothing synchronises the device; every function returns 0 on success and a CTTRAIN_ERR_* code on
 * error (message: cttrain_last_error).  A handle is bound to the device current at cttrain_create() and is not
 * thread-safe.  Every reduction runs in a fixed order without atomics: two backward calls on the same tape give
 * bitwise-identical gradients.
 */
#ifndef CTASNET_TRAIN_H_
#define CTASNET_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTTRAIN_ABI_VERSION 1

/* error codes (same values as ctasnet.h) */
#define CTTRAIN_OK 0
#define CTTRAIN_ERR_INVALID 1     /* bad argument / unsupported shape */
#define CTTRAIN_ERR_WORKSPACE 2   /* workspace too small or misaligned */
#define CTTRAIN_ERR_WEIGHTS 3     /* weights or gradients not bound / wrong count */
#define CTTRAIN_ERR_HIP 4         /* a HIP call or launch failed */

typedef struct cttrain_ctx* cttrain_handle;

int cttrain_abi_version(void);

/* The model is fixed by the reference (N=512, B=128, H=512, X=8, P=3, R=3, L=16).  Fails without a HIP device. */
int cttrain_create(cttrain_handle* out);
void cttrain_destroy(cttrain_handle h);
/* last error of `h`; h == NULL: the last cttrain_create() failure of this thread */
const char* cttrain_last_error(cttrain_handle h);

/* Weight table in the reference's state_dict() order (345 tensors, the same table as ctasnet.h). */
int cttrain_num_weights(cttrain_handle h);
const char* cttrain_weight_name(cttrain_handle h, int i);
int64_t cttrain_weight_numel(cttrain_handle h, int i);
/* Borrow `n` device pointers (state_dict order).  The step reads them as they are at launch time: nothing derived from
 * them is cached, so an optimizer step or load_state_dict in place is seen by the next call. */
int cttrain_bind_weights(cttrain_handle h, const float* const* dev_ptrs, int n);
/* Borrow `n` device pointers the backward WRITES (overwrites) the gradient of each weight into (state_dict order). */
int cttrain_bind_grads(cttrain_handle h, float* const* dev_ptrs, int n);

/* Flat layout of gradients / optimizer state: slot i starts at offset(i) floats (64-float aligned, zero padding);
 * offset(num_weights) is the total. */
int64_t cttrain_flat_offset(cttrain_handle h, int slot);
int64_t cttrain_flat_numel(cttrain_handle h);

/* Encoder frames F = (T + 16) / 16 + 1 and output length 16 * (T / 16); 0 if T < 16. */
int64_t cttrain_frames(int64_t T);
int64_t cttrain_out_len(int64_t T);
/* Workspace (tape + scratch) of one step of B mixtures of T samples; 0 for an unsupported shape. */
size_t cttrain_workspace_bytes(cttrain_handle h, int B, int64_t T);

/* Forward that records its tape in `ws`: mix [B][T] -> s1_pred, s2_pred [B][cttrain_out_len(T)], bitwise equal to
 * ctasnet_forward with the same weights. */
int cttrain_train_forward(cttrain_handle h, const float* mix, int B, int64_t T, float* s1_pred, float* s2_pred, void* ws,
                          size_t ws_bytes, void* stream);
/* Introspection for tests and tools: byte offset in the workspace of a tensor the last cttrain_train_forward of B x T left
 * on the tape, or -1.  V1: block `block`'s conv1d output + bias (the input of PReLU_1), [B * F][512] fp32, frame-major;
 * U: its depthwise conv output + bias (the input of PReLU_2), [B * F][512]; SKIP: the summed skip paths (the input of the
 * head's PReLU), [B * F][128], block 0 only. */
#define CTTRAIN_TAPE_V1 0
#define CTTRAIN_TAPE_U 1
#define CTTRAIN_TAPE_SKIP 2
int64_t cttrain_tape_offset(cttrain_handle h, int B, int64_t T, int which, int block);
/* Backward of the last cttrain_train_forward on this workspace (same mix, B, T): d loss / d s1_pred, d_s2_pred
 * [B][out_len] -> every bound gradient buffer (overwritten). */
int cttrain_train_backward(cttrain_handle h, const float* mix, int B, int64_t T, const float* d_s1, const float* d_s2,
                           void* ws, size_t ws_bytes, void* stream);

/* clip_grad_norm_ over a flat gradient (cttrain_flat_numel floats): scale in place when max_norm > 0; the pre-clip norm
 * goes to norm_out[0].  scratch: cttrain_clip_scratch_bytes(), 8-byte aligned. */
size_t cttrain_clip_scratch_bytes(cttrain_handle h);
int cttrain_grad_clip(cttrain_handle h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                      float* norm_out, void* stream);
/* torch.optim.AdamW step (amsgrad / maximize off) of the bound weights, gradient and state in the flat layout. */
int cttrain_adamw_step(cttrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                       double beta1, double beta2, double eps, double weight_decay, int step, void* stream);

/* Cost model of one mixture's training step (forward + backward): algorithmic FLOPs, 2 per MAC. */
double cttrain_flops_per_mixture(cttrain_handle h, int64_t T);

#ifdef __cplusplus
}
#endif
#endif /* CTASNET_TRAIN_H_ */
