/*
 * vfilt_train.h -- C ABI of the VoiceFilter training step in libdptnav.so (gfx950), fp32.
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   model       VoiceFilter.forward from the embeddings on, in training mode, + autograd backward
 *                                                           src/model/voicefilter.py:108-145  -> vftrain_train_forward,
 *                                                                                                vftrain_train_backward
 *   clip        clip_grad_norm_(params, max_grad_norm)      src/trainer/base_trainer.py:383-391 -> vftrain_grad_clip
 *   optimizer   torch.optim.Adam (vf_mse.yaml, vf_mae.yaml) = AdamW with weight_decay 0         -> vftrain_adamw_step
 *   The Python module speech_separation_amd.TrainableVoiceFilter calls the entry points below through ctypes.  The
 *   inference forward stays in vfilt.h; this header adds the training step next to it and changes nothing there.
 *
 * Conventions (as dctasnet_train.h): C99, plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by
 * the caller; the library allocates nothing on the hot path (the caller passes a workspace of vftrain_workspace_bytes(),
 * 256-byte aligned, which also holds the tape between train_forward and train_backward); work is enqueued on `stream` (a
 * hipStream_t) and nothing synchronises the device; the bound weights are read as they are at launch time; every function
 * returns 0 on success and a VFTRAIN_ERR_* code on error (message: vftrain_last_error).  A handle is bound to the device
 * current at vftrain_create() and is not thread-safe.  No atomics, one fixed summation order, and no split that depends
 * on the device's size: two backward calls on the same tape give bitwise-identical gradients.
 *
 * Training-mode semantics:
 *   BatchNorm   the batch's statistics: mean and BIASED variance over B * F * W values per channel, eps 1e-5.
 *   Dropout     nn.Dropout2d(0.35) on the 3-D tensor [2B][W][600] zeroes whole frames: one draw per (sequence q, frame t),
 *               survivors scaled by 1 / (1 - p).  keep <=> drop_rand_q(drop_qseed(seed, q * W + t), 0) >= p * 2^24, the
 *               library's counter-based generator (csrc/common.h); torch's Philox stream is not reproduced, the contract
 *               is the same distribution.  The mask is stored on the tape and read by the backward.
 *   sequences   q = speaker * B + item, as vfilt.h.  The CNN runs once per item and feeds both speakers: where the two
 *               speakers' gradients meet, speaker 1 is added first.
 *   gradients   none for the mixture and the embeddings.  The eight conv biases sit in front of a batch-statistics
 *               BatchNorm: their gradient is mathematically zero (autograd returns rounding noise there) and the
 *               library writes exact zeros into these eight slots.  gru.weight_hh_l1_reverse only ever meets h = 0 (the
 *               model reads gru_out[:, -1, :]): its gradient is exactly zero too.
 * Supported shapes: as vfilt.h, and B * input_size * W >= 2.
 */
#ifndef VFILT_TRAIN_H_
#define VFILT_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VFTRAIN_ABI_VERSION 1

/* error codes (same values as vfilt.h) */
#define VFTRAIN_OK 0
#define VFTRAIN_ERR_INVALID 1     /* bad argument / unsupported shape / no tape */
#define VFTRAIN_ERR_WORKSPACE 2   /* workspace too small or misaligned */
#define VFTRAIN_ERR_WEIGHTS 3     /* weights or gradients not bound / wrong count */
#define VFTRAIN_ERR_HIP 4         /* a HIP call or launch failed */

typedef struct vftrain_ctx* vftrain_handle;

int vftrain_abi_version(void);

/* input_size, embed_size as vfilt_create.  Fails without a HIP device. */
int vftrain_create(vftrain_handle* out, int input_size, int embed_size);
void vftrain_destroy(vftrain_handle h);
/* last error of `h`; h == NULL: the last vftrain_create() failure of this thread */
const char* vftrain_last_error(vftrain_handle h);

/* Weight table: the 74 float tensors of vfilt.h, in its order. */
int vftrain_num_weights(vftrain_handle h);
const char* vftrain_weight_name(vftrain_handle h, int i);
int64_t vftrain_weight_numel(vftrain_handle h, int i);
/* Borrow `n` device pointers (table order).  The step reads them as they are at launch time: nothing derived from them
 * is cached, so an optimizer step or load_state_dict in place is seen by the next call. */
int vftrain_bind_weights(vftrain_handle h, const float* const* dev_ptrs, int n);
/* Borrow `n` device pointers the backward WRITES (overwrites) the gradient of each weight into (table order).  The 16
 * slots of the running statistics (running_mean, running_var) are never written and vftrain_adamw_step never changes
 * those buffers. */
int vftrain_bind_grads(vftrain_handle h, float* const* dev_ptrs, int n);

/* Flat layout of gradients / optimizer state: slot i starts at offset(i) floats (64-float aligned, zero padding);
 * offset(num_weights) is the total. */
int64_t vftrain_flat_offset(vftrain_handle h, int slot);
int64_t vftrain_flat_numel(vftrain_handle h);

/* Workspace (tape + scratch) of one step of B items with W spectrogram frames and Tv video frames; 0 for an unsupported
 * shape (message: vftrain_last_error). */
size_t vftrain_workspace_bytes(vftrain_handle h, int B, int W, int Tv);

/* Forward in training mode that records its tape in `ws`: mix_magnitude [B][F][W], emb1 / emb2 [B][Tv][E] -> out1 / out2
 * [B][F][W].  dropout_ppm: the drop probability in parts per million (the reference: 350000; 0 switches it off);
 * dropout_seed: seed of this call's mask. */
int vftrain_train_forward(vftrain_handle h, const float* mix_magnitude, const float* emb1, const float* emb2, int B, int W,
                          int Tv, int dropout_ppm, uint32_t dropout_seed, float* out1, float* out2, void* ws, size_t ws_bytes,
                          void* stream);
/* Backward of the last vftrain_train_forward on this workspace: d loss / d out1, d out2 [B][F][W] -> every bound gradient
 * buffer (overwritten).  The workspace and (B, W, Tv) are checked against that forward and anything else is refused;
 * mix_magnitude, emb1 and emb2 must hold the forward's values, which is the caller's duty (they are not compared). */
int vftrain_train_backward(vftrain_handle h, const float* mix_magnitude, const float* emb1, const float* emb2, int B, int W,
                           int Tv, const float* d_out1, const float* d_out2, void* ws, size_t ws_bytes, void* stream);

/* Introspection for tests and tools: byte offset in the workspace of a tensor the last train_forward of (B, W, Tv) left on
 * the tape, or -1.  pos = B * F * W positions in (item, f, w) order; rows = 2B * W in (q, t) order.
 *   Z       index l = 0..7: the raw output (conv + bias) of CNN layer l + 1 in front of its BatchNorm; l < 7: [pos][64];
 *           l = 7: [B][W][F][8], the memory order the reference VIEWS as [B][8F][W]
 *   ACT     index l = 0..6: BatchNorm + ReLU of Z_l, [pos][64]; the ReLU kept an element where this is > 0
 *   LSTM_H  the LSTM's output h, [rows][400]; the ReLU behind it kept an element where this is > 0
 *   FC1     ReLU(fc.1(..)) in front of the dropout's scale, [rows][600]; the ReLU behind fc.1 kept an element where this
 *           is > 0 (ReLU and the dropout's non-negative scale commute)
 *   DROP    the dropout keep mask, [2B][W], 1.0 = kept
 *   GATES   the LSTM's gate activations i, f, g, o, [rows][1600];  CELL: its cell state c, [rows][400]
 *   STATS   [8][2][64]: per layer the batch mean and the UNBIASED batch variance of Z_l (zeros past a layer's channels),
 *           what the running buffers are updated with */
#define VFTRAIN_TAPE_Z 0
#define VFTRAIN_TAPE_ACT 1
#define VFTRAIN_TAPE_LSTM_H 2
#define VFTRAIN_TAPE_FC1 3
#define VFTRAIN_TAPE_DROP 4
#define VFTRAIN_TAPE_GATES 5
#define VFTRAIN_TAPE_STATS 6
#define VFTRAIN_TAPE_CELL 7
int64_t vftrain_tape_offset(vftrain_handle h, int B, int W, int Tv, int which, int index);

/* clip_grad_norm_ over a flat gradient (vftrain_flat_numel floats): scale in place when max_norm > 0; the pre-clip norm
 * goes to norm_out[0].  scratch: vftrain_clip_scratch_bytes(), 8-byte aligned. */
size_t vftrain_clip_scratch_bytes(vftrain_handle h);
int vftrain_grad_clip(vftrain_handle h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                      float* norm_out, void* stream);
/* torch.optim.AdamW step (amsgrad / maximize off) of the bound trainable weights, gradient and state in the flat layout;
 * weight_decay = 0 is torch.optim.Adam. */
int vftrain_adamw_step(vftrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                       double beta1, double beta2, double eps, double weight_decay, int step, void* stream);

/* Cost model of one item's training step (forward + backward, both speakers): algorithmic FLOPs, 2 per MAC:
 * 3 x vfilt_flops_per_item.  0 for an unsupported shape. */
double vftrain_flops_per_item(vftrain_handle h, int W, int Tv);

#ifdef __cplusplus
}
#endif
#endif /* VFILT_TRAIN_H_ */
