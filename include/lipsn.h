/*
 * lipsn.h -- C ABI of the ShuffleNet-v2 lip reader in libdptnav.so (gfx950): mouth video -> one 1024-wide embedding per frame,
 * the lip reader the reference's VoiceFilter is written for (model/voicefilter.yaml -> lrw_snv1x_tcn1x.json).  Inference
 * only, fp32.  include/lipfe.h is the ResNet-18 lip reader (512 wide); the two share nothing at this boundary.
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   construction  init_lipreader(config, path)                        src/utils/init_utils.py:168-207
 *                 Lipreading(modality="video", backbone_type="shufflenet", width_mult=0.5 | 1.0, relu_type=...,
 *                            extract_feats=True)                      src/lipreader/lipreading/model.py:141-250
 *   call          Lipreading.forward(x, lengths)                      src/lipreader/lipreading/model.py:252-273
 *     stem        Conv3d(1,24,(5,7,7),s=(1,2,2),p=(2,3,3)) + BatchNorm3d + act + MaxPool3d((1,3,3),(1,2,2),(0,1,1))   :193-207
 *     trunk       ShuffleNetV2.features (16 InvertedResidual blocks, repeats 4 / 8 / 4), conv_last (1 x 1 -> 1024 + BN +
 *                 ReLU), globalpool = AvgPool2d(3)                    src/lipreader/lipreading/models/shufflenetv2.py:44-160
 *     relu_type touches the stem's activation only; the trunk is ReLU throughout.
 *     With extract_feats=True the TCN back end never runs; it is not part of this boundary.
 *   preprocessing as include/lipfe.h: the window (Hin, Win, y0, x0, H, W) and the affine (a, b) of lipsn_forward
 *   callers       VoiceFilter (model/voicefilter.py), make_embeddings.py, profiler.py VideoSSModel
 *   checkpoint    state_dict()/load_state_dict()                      (keys: lipsn_weight_name)
 *   The Python module speech_separation_amd.ShuffleNetLipreading keeps the reference's duck type and calls the entry points
 *   below through ctypes with raw device pointers.
 *
 * Conventions (as include/lipfe.h): plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by the
 * caller; the library allocates nothing on the hot path (the caller passes a workspace of lipsn_workspace_bytes(),
 * 256-byte aligned); work is enqueued on `stream` (a hipStream_t) and nothing synchronises the device; every function
 * returns 0 on success and a LIPSN_ERR_* code on error (message: lipsn_last_error).  A handle is bound to the device
 * current at lipsn_create() and is not thread-safe.  Results are bit-identical from call to call, and a stream's result
 * does not depend on the other streams of its batch.
 */
#ifndef LIPSN_H_
#define LIPSN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIPSN_ABI_VERSION 1

#define LIPSN_OK 0
#define LIPSN_ERR_INVALID 1     /* bad argument / unsupported shape */
#define LIPSN_ERR_WORKSPACE 2   /* workspace too small or misaligned */
#define LIPSN_ERR_WEIGHTS 3     /* weights not bound / wrong count */
#define LIPSN_ERR_HIP 4         /* a HIP call or launch failed */

/* relu_type of the reference's constructor: the stem's activation */
#define LIPSN_RELU 0
#define LIPSN_PRELU 1           /* 24 slopes: one more weight tensor (frontend3D.2.weight) */
#define LIPSN_SWISH 2

#define LIPSN_EMBED 1024        /* width of an embedding (backend_out) */
#define LIPSN_MIN_HW 65         /* supported window: 65 <= H, W <= 160, where the reference's AvgPool2d(3) yields one position */
#define LIPSN_MAX_HW 160

typedef struct lipsn_ctx* lipsn_handle;

int lipsn_abi_version(void);

/* width_x2: twice the reference's width_mult: 1 (stages 48 / 96 / 192) or 2 (116 / 232 / 464).  width_mult 1.5 and 2.0
 * (3, 4) are refused: no config of the reference uses them.  Fails without a HIP device. */
int lipsn_create(lipsn_handle* out, int relu_type, int width_x2);
void lipsn_destroy(lipsn_handle h);
/* last error of `h`; h == NULL: the last lipsn_create() failure of this thread */
const char* lipsn_last_error(lipsn_handle h);

/* Weight table: the float tensors of the reference's state_dict(), in its order, without the tcn.* entries and without
 * the int64 num_batches_tracked counters (280 tensors; 281 with PReLU slopes). */
int lipsn_num_weights(lipsn_handle h);
const char* lipsn_weight_name(lipsn_handle h, int i);
int64_t lipsn_weight_numel(lipsn_handle h, int i);
/* Borrow `n` device pointers (table order); they must stay valid while forwards run.  Nothing is copied at bind time:
 * every forward derives its own K-major weights and folded BatchNorm scale / shift from the current values. */
int lipsn_bind_weights(lipsn_handle h, const float* const* dev_ptrs, int n);

/* Workspace of one forward of S streams of T frames with an H x W window; 0 for an unsupported shape (supported:
 * S >= 1, T >= 1, 65 <= H, W <= 160; message: lipsn_last_error). */
size_t lipsn_workspace_bytes(lipsn_handle h, int S, int T, int H, int W);

/* forward: x [S][T][Hin][Win] (the reference's (S, 1, T, Hin, Win)) -> out [S][T][1024].
 * The network sees the window x[.., y0 : y0 + H, x0 : x0 + W] after the affine a * x + b; its padding taps are zero in
 * that normalised domain.  Temporal taps see zeros outside [0, T) of their own stream.
 * a = 1, b = 0, y0 = x0 = 0, Hin = H, Win = W is the plain forward. */
int lipsn_forward(lipsn_handle h, const float* x, int S, int T, int Hin, int Win, int y0, int x0, int H, int W, float a, float b,
                  float* out, void* ws, size_t ws_bytes, void* stream);

/* Launches one forward enqueues (fold, pack, stem, max-pool, 16 blocks, conv_last + pool). */
int lipsn_launches_per_forward(void);

/* Cost model of one stream's forward: algorithmic FLOPs of the convolutions (2 per MAC, padding taps counted, conv_last on
 * the whole final map as the reference computes it) and the bytes the launches of this implementation read and write when
 * nothing stays cached between them.  Each forward also derives its weight copies once, whatever S:
 * lipsn_weight_pack_bytes() read + written.  0 for an unsupported width or shape. */
double lipsn_flops_per_stream(int width_x2, int T, int H, int W);
double lipsn_min_bytes_per_stream(int width_x2, int T, int H, int W);
size_t lipsn_weight_pack_bytes(lipsn_handle h);

#ifdef __cplusplus
}
#endif
#endif /* LIPSN_H_ */
