/*
 * dctasnet.h -- C ABI of the deep Conv-TasNet inference forward in libdptnav.so (gfx950): DeepConvTasNet and its
 * audio-visual form DeepAVConvTasNet.
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   construction  hydra.utils.instantiate(config.model)   src/configs/model/deepconvtasnet.yaml, deepavconvtasnet.yaml
 *                 DeepConvTasNet.__init__ (N, L ignored)  src/model/deepconvtasnet.py:122-129
 *                 DeepAVConvTasNet.__init__               src/model/deepavconvtasnet.py:122-134
 *   call          forward(mix, [s1_embedding, s2_embedding,] **batch)
 *     Encoder     pad (16, 32) + Conv1d(1,512,32,s=16) + bias, 4 x [Conv1d(512,512,3,d) + PReLU]   :7-26   -> dctasnet_forward
 *     AV head     Linear(512->256) per speaker, concat, linear interpolation Tv -> F, LayerNorm(512),
 *                 added to the encoder output (DeepAV only)                                        :140-153
 *     Separator   Conv-TasNet's (masks multiply the encoder output, AV: the fused one)             :66-94
 *     Decoder     4 x [ConvTranspose1d(512,512,3,d) + PReLU], ConvTranspose1d(512,1,32,s=16) + bias,
 *                 crop [16, len - 32)                                                               :96-120
 *   checkpoint    state_dict()/load_state_dict()          (keys: dctasnet_weight_name)
 *   The Python modules speech_separation_amd.DeepConvTasNet / DeepAVConvTasNet keep the reference's duck type and call the
 *   entry points below through ctypes with raw device pointers.
 *
 * Conventions (as include/ctasnet.h): plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by the
 * caller; the library allocates nothing on the hot path (the caller passes a workspace of dctasnet_workspace_bytes(),
 * 256-byte aligned); work is enqueued on `stream` (a hipStream_t) and nothing synchronises the device; every function
 * returns 0 on success and a DCTASNET_ERR_* code on error (message: dctasnet_last_error).  A handle is bound to the device
 * current at dctasnet_create() and is not thread-safe.  Inference only: no training entry points.
 */
#ifndef DCTASNET_H_
#define DCTASNET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCTASNET_ABI_VERSION 1

/* error codes (same values as ctasnet.h) */
#define DCTASNET_OK 0
#define DCTASNET_ERR_INVALID 1     /* bad argument / unsupported shape */
#define DCTASNET_ERR_WORKSPACE 2   /* workspace too small or misaligned */
#define DCTASNET_ERR_WEIGHTS 3     /* weights not bound / wrong count */
#define DCTASNET_ERR_HIP 4         /* a HIP call or launch failed */

typedef struct dctasnet_ctx* dctasnet_handle;

int dctasnet_abi_version(void);

/* av = 0: DeepConvTasNet; av != 0: DeepAVConvTasNet (video_emb_size = hidden_video = 512).  The sizes are fixed by the
 * reference (N=512, L=16, separator B=128, H=512, X=8, P=3, R=3).  Fails without a HIP device. */
int dctasnet_create(dctasnet_handle* out, int av);
void dctasnet_destroy(dctasnet_handle h);
/* last error of `h`; h == NULL: the last dctasnet_create() failure of this thread */
const char* dctasnet_last_error(dctasnet_handle h);

/* Weight table in the reference's state_dict() order (372 tensors; 376 for the audio-visual model).
 * decoder.deconv.weight is a parameter of the reference that its forward never uses: it is bound and never read. */
int dctasnet_num_weights(dctasnet_handle h);
const char* dctasnet_weight_name(dctasnet_handle h, int i);
int64_t dctasnet_weight_numel(dctasnet_handle h, int i);
/* Borrow `n` device pointers (state_dict order); they must stay valid while forwards run.  Nothing is copied: every
 * forward reads the current values. */
int dctasnet_bind_weights(dctasnet_handle h, const float* const* dev_ptrs, int n);

/* Encoder frames F = (T + 16) / 16 + 1 and output length 16 * (T / 16); 0 if T < 16. */
int64_t dctasnet_frames(int64_t T);
int64_t dctasnet_out_len(int64_t T);
/* Workspace of one forward of B mixtures of T samples with Tv video frames (ignored by the audio-only model); 0 for an
 * unsupported shape (message: dctasnet_last_error). */
size_t dctasnet_workspace_bytes(dctasnet_handle h, int B, int64_t T, int Tv);

/* forward: mix [B][T], e1 / e2 [B][512][Tv] (the audio-visual model; NULL for the audio-only one)
 *   -> s1_pred, s2_pred [B][dctasnet_out_len(T)]. */
int dctasnet_forward(dctasnet_handle h, const float* mix, const float* e1, const float* e2, int B, int64_t T, int Tv,
                     float* s1_pred, float* s2_pred, void* ws, size_t ws_bytes, void* stream);

/* Cost model of one mixture's forward: algorithmic FLOPs (2 per MAC; the video head, < 0.1 %, is left out) and the bytes
 * the launches of this implementation read and write when nothing stays cached between them.  Each forward also repacks
 * the dense convs' weights once, whatever B: dctasnet_weight_pack_bytes() read + written. */
double dctasnet_flops_per_mixture(dctasnet_handle h, int64_t T);
double dctasnet_min_bytes_per_mixture(dctasnet_handle h, int64_t T);
size_t dctasnet_weight_pack_bytes(dctasnet_handle h);

#ifdef __cplusplus
}
#endif
#endif /* DCTASNET_H_ */
