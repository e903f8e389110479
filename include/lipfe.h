/*
 * lipfe.h -- C ABI of the lip-reading front end in libdptnav.so (gfx950): mouth video -> one 512-wide embedding per frame,
 * the input of the audio-visual separators (DPTNAVWavEncDec, DPRNNAVEncDec, DeepAVConvTasNet).  Inference only, fp32.
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   construction  init_lipreader(config, path)                        src/utils/init_utils.py:168-207
 *                 Lipreading(modality="video", backbone_type="resnet", relu_type=..., extract_feats=True)
 *                                                                     src/lipreader/lipreading/model.py:141-250
 *   call          Lipreading.forward(x, lengths)                      src/lipreader/lipreading/model.py:252-273
 *     stem        Conv3d(1,64,(5,7,7),s=(1,2,2),p=(2,3,3)) + BatchNorm3d + act + MaxPool3d((1,3,3),(1,2,2),(0,1,1))   :193-207
 *     trunk       ResNet(BasicBlock, [2,2,2,2]) per frame + AdaptiveAvgPool2d(1)   src/lipreader/lipreading/models/resnet.py:32-145
 *     With extract_feats=True the TCN back end never runs; it is not part of this boundary.
 *   preprocessing Normalize(0,255), CenterCrop((88,88)), Normalize(0.421,0.165)
 *                                                                     src/lipreader/lipreading/dataloaders.py:25-27, preprocess.py:62-103
 *                 -> the window (Hin, Win, y0, x0, H, W) and the affine (a, b) of lipfe_forward
 *   callers       make_embeddings.py (offline), profiler.py VideoSSModel (online)
 *   checkpoint    state_dict()/load_state_dict()                      (keys: lipfe_weight_name)
 *   The Python module speech_separation_amd.Lipreading keeps the reference's duck type and calls the entry points below
 *   through ctypes with raw device pointers.
 *
 * Conventions (as include/dctasnet.h): plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by the
 * caller; the library allocates nothing on the hot path (the caller passes a workspace of lipfe_workspace_bytes(),
 * 256-byte aligned); work is enqueued on `stream` (a hipStream_t) and nothing synchronises the device; every function
 * returns 0 on success and a LIPFE_ERR_* code on error (message: lipfe_last_error).  A handle is bound to the device
 * current at lipfe_create() and is not thread-safe.  Results are bit-identical from call to call, and a stream's result
 * does not depend on the other streams of its batch.
 */
#ifndef LIPFE_H_
#define LIPFE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIPFE_ABI_VERSION 1

#define LIPFE_OK 0
#define LIPFE_ERR_INVALID 1     /* bad argument / unsupported shape */
#define LIPFE_ERR_WORKSPACE 2   /* workspace too small or misaligned */
#define LIPFE_ERR_WEIGHTS 3     /* weights not bound / wrong count */
#define LIPFE_ERR_HIP 4         /* a HIP call or launch failed */

/* relu_type of the reference's constructor */
#define LIPFE_RELU 0
#define LIPFE_PRELU 1           /* per-channel slopes: 17 more weight tensors */
#define LIPFE_SWISH 2           /* x * sigmoid(x): what every resnet config of the reference uses */

typedef struct lipfe_ctx* lipfe_handle;

int lipfe_abi_version(void);

/* Fails without a HIP device. */
int lipfe_create(lipfe_handle* out, int relu_type);
void lipfe_destroy(lipfe_handle h);
/* last error of `h`; h == NULL: the last lipfe_create() failure of this thread */
const char* lipfe_last_error(lipfe_handle h);

/* Weight table: the float tensors of the reference's state_dict(), in its order, without the tcn.* entries and without
 * the int64 num_batches_tracked counters (100 tensors; 117 with PReLU slopes). */
int lipfe_num_weights(lipfe_handle h);
const char* lipfe_weight_name(lipfe_handle h, int i);
int64_t lipfe_weight_numel(lipfe_handle h, int i);
/* Borrow `n` device pointers (table order); they must stay valid while forwards run.  Nothing is copied at bind time:
 * every forward derives its own K-major weights and folded BatchNorm scale / shift from the current values. */
int lipfe_bind_weights(lipfe_handle h, const float* const* dev_ptrs, int n);

/* Workspace of one forward of S streams of T frames with an H x W window; 0 for an unsupported shape (supported:
 * S >= 1, T >= 1, 8 <= H, W <= 256; message: lipfe_last_error). */
size_t lipfe_workspace_bytes(lipfe_handle h, int S, int T, int H, int W);

/* forward: x [S][T][Hin][Win] (the reference's (S, 1, T, Hin, Win)) -> out [S][T][512].
 * The network sees the window x[.., y0 : y0 + H, x0 : x0 + W] after the affine a * x + b; its padding taps are zero in
 * that normalised domain.  Temporal taps see zeros outside [0, T) of their own stream.
 * a = 1, b = 0, y0 = x0 = 0, Hin = H, Win = W is the plain forward. */
int lipfe_forward(lipfe_handle h, const float* x, int S, int T, int Hin, int Win, int y0, int x0, int H, int W, float a, float b,
                  float* out, void* ws, size_t ws_bytes, void* stream);

/* Cost model of one stream's forward: algorithmic FLOPs of the convolutions (2 per MAC, padding taps counted) and the bytes
 * the launches of this implementation read and write when nothing stays cached between them.  Each forward also derives
 * its weight copies once, whatever S: lipfe_weight_pack_bytes() read + written. */
double lipfe_flops_per_stream(int T, int H, int W);
double lipfe_min_bytes_per_stream(int T, int H, int W);
size_t lipfe_weight_pack_bytes(lipfe_handle h);

#ifdef __cplusplus
}
#endif
#endif /* LIPFE_H_ */
