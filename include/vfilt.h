/*
 * vfilt.h -- C ABI of the VoiceFilter separator in libdptnav.so (gfx950): a mixture's magnitude spectrogram and one lip
 * embedding sequence per speaker -> one masked spectrogram per speaker.  Inference only (eval mode), fp32.
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   construction  VoiceFilter(input_size, lipreader_path, lipreader_config)   src/model/voicefilter.py:11-84
 *   call          VoiceFilter.forward from the embeddings on                  src/model/voicefilter.py:108-145
 *     d-vector    nn.GRU(E, F, num_layers=2, bidirectional=True) -> fc_dvector(gru_out[:, -1, :])      :24-33, :109-114
 *     CNN         8 x (Conv2d + BatchNorm2d), ReLU on the first seven, dilations 1..16 along F          :37-68, :118-119
 *     view        permute(0, 3, 2, 1).contiguous().view(B, 8F, W): a reinterpretation, not a transpose  :122-124
 *     mask        nn.LSTM(9F, 400) -> ReLU, Linear(400, 600), ReLU, Linear(600, F), Sigmoid; x mixture  :72-84, :128-142
 *   The lip reader in front of it is include/lipfe.h; the Python module speech_separation_amd.VoiceFilter joins the two.
 *   checkpoint    state_dict()/load_state_dict()                              (keys: vfilt_weight_name)
 *
 * Conventions (as include/lipfe.h): plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by the
 * caller; the library allocates nothing on the hot path (the caller passes a workspace of vfilt_workspace_bytes(),
 * 256-byte aligned); work is enqueued on `stream` (a hipStream_t) and nothing synchronises the device; every function
 * returns 0 on success and a VFILT_ERR_* code on error (message: vfilt_last_error).  A handle is bound to the device
 * current at vfilt_create() and is not thread-safe.  No atomics and one fixed summation order: results are bit-identical
 * from call to call, and an item's result does not depend on the other items of its batch.
 *
 * Supported: 1 <= input_size <= 257, embed_size 512 or 1024, B >= 1, W >= 1, Tv >= 1, as long as
 * B * input_size * W * 64 (the largest activation map, in floats) and 2 * B * max(W, Tv) * 1600 stay below 2^31.
 * Everything else is refused with a message before anything is launched.
 */
#ifndef VFILT_H_
#define VFILT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VFILT_ABI_VERSION 1

#define VFILT_OK 0
#define VFILT_ERR_INVALID 1     /* bad argument / unsupported shape */
#define VFILT_ERR_WORKSPACE 2   /* workspace too small or misaligned */
#define VFILT_ERR_WEIGHTS 3     /* weights not bound / wrong count */
#define VFILT_ERR_HIP 4         /* a HIP call or launch failed */

typedef struct vfilt_ctx* vfilt_handle;

int vfilt_abi_version(void);

/* input_size: frequency bins F of the spectrogram (the reference: 201); embed_size: width E of a lip embedding (the
 * reference: 1024; this library's ResNet-18 lip reader: 512).  Fails without a HIP device. */
int vfilt_create(vfilt_handle* out, int input_size, int embed_size);
void vfilt_destroy(vfilt_handle h);
/* last error of `h`; h == NULL: the last vfilt_create() failure of this thread */
const char* vfilt_last_error(vfilt_handle h);

/* Weight table: the 74 float tensors of the reference's state_dict(), in its order, without the eight int64
 * num_batches_tracked counters (and without the lip reader's entries). */
int vfilt_num_weights(vfilt_handle h);
const char* vfilt_weight_name(vfilt_handle h, int i);
int64_t vfilt_weight_numel(vfilt_handle h, int i);
/* Borrow `n` device pointers (table order); they must stay valid while forwards run.  Nothing is copied at bind time:
 * every forward derives its own K-major conv weights and folded BatchNorm scale / shift from the current values. */
int vfilt_bind_weights(vfilt_handle h, const float* const* dev_ptrs, int n);

/* Workspace of one forward of B items with W spectrogram frames and Tv video frames; 0 for an unsupported shape
 * (message: vfilt_last_error). */
size_t vfilt_workspace_bytes(vfilt_handle h, int B, int W, int Tv);

/* forward: mix_magnitude [B][F][W], emb1 / emb2 [B][Tv][E] -> out1 / out2 [B][F][W] (s1_spec_pred / s2_spec_pred).
 * out1 / out2 must not overlap mix_magnitude. */
int vfilt_forward(vfilt_handle h, const float* mix_magnitude, const float* emb1, const float* emb2, int B, int W, int Tv,
                  float* out1, float* out2, void* ws, size_t ws_bytes, void* stream);

/* Cost model of one item's forward (both speakers): algorithmic FLOPs (2 per MAC, padding taps counted) and the bytes
 * the launches of this implementation read and write when nothing stays cached between them (the recurrent weights are
 * counted once per step).  0 for an unsupported shape. */
double vfilt_flops_per_item(vfilt_handle h, int W, int Tv);
double vfilt_min_bytes_per_item(vfilt_handle h, int W, int Tv);

#ifdef __cplusplus
}
#endif
#endif /* VFILT_H_ */
