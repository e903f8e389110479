/*
 * ctasnet.h -- C ABI of the Conv-TasNet inference forward in libdptnav.so (gfx950).
 *
 * What this boundary replaces in the reference (paths relative to the reference repository):
 *   construction  hydra.utils.instantiate(config.model)   src/configs/model/convtasnet.yaml:1
 *                 ConvTasNet.__init__ (N, L ignored)      src/model/convtasnet.py:102-108
 *   call          ConvTasNet.forward(mix, **batch)        src/model/convtasnet.py:110-116
 *     Encoder     pad (16, 32) + Conv1d(1,512,32,s=16)    :6-15        -> ctasnet_forward
 *     Separator   GlobalNorm, 1x1 512->128, 24 blocks,    :18-83       -> ctasnet_forward
 *                 PReLU + 1x1 128->1024 + sigmoid masks
 *     Decoder     ConvTranspose1d(512,1,32,s=16), crop    :85-99       -> ctasnet_forward
 *   checkpoint    state_dict()/load_state_dict()          (keys: ctasnet_weight_name)
 *   The Python module speech_separation_amd.ConvTasNet keeps the reference's duck type and calls the entry points below
 *   through ctypes with raw device pointers.
 *
 * Conventions (as include/dptnav.h): plain C types; tensor arguments are DEVICE pointers to contiguous fp32 owned by the
 * caller; the library allocates nothing on the hot path (the caller passes a workspace of ctasnet_workspace_bytes(),
 * 256-byte aligned); work is enqueued on `stream` (a hipStream_t) and nothing synchronises the device; every function
 * returns 0 on success and a DPTNAV_ERR_* style code on error (message: ctasnet_last_error).  A handle is bound to the
 * device current at ctasnet_create() and is not thread-safe.  Inference only: no training entry points.
 */
#ifndef CTASNET_H_
#define CTASNET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTASNET_ABI_VERSION 1

/* error codes (same values as dptnav.h) */
#define CTASNET_OK 0
#define CTASNET_ERR_INVALID 1     /* bad argument / unsupported shape */
#define CTASNET_ERR_WORKSPACE 2   /* workspace too small or misaligned */
#define CTASNET_ERR_WEIGHTS 3     /* weights not bound / wrong count */
#define CTASNET_ERR_HIP 4         /* a HIP call or launch failed */

typedef struct ctasnet_ctx* ctasnet_handle;

int ctasnet_abi_version(void);

/* The model is fixed by the reference (N=512, B=128, H=512, X=8, P=3, R=3, L=16).  Fails without a HIP device. */
int ctasnet_create(ctasnet_handle* out);
void ctasnet_destroy(ctasnet_handle h);
/* last error of `h`; h == NULL: the last ctasnet_create() failure of this thread */
const char* ctasnet_last_error(ctasnet_handle h);

/* Weight table in the reference's state_dict() order (convtasnet.py module order, 345 tensors). */
int ctasnet_num_weights(ctasnet_handle h);
const char* ctasnet_weight_name(ctasnet_handle h, int i);
int64_t ctasnet_weight_numel(ctasnet_handle h, int i);
/* Borrow `n` device pointers (state_dict order); they must stay valid while forwards run. */
int ctasnet_bind_weights(ctasnet_handle h, const float* const* dev_ptrs, int n);

/* Encoder frames F = (T + 16) / 16 + 1 and output length 16 * (T / 16) (convtasnet.py:14-15, :93-96); 0 if T < 16. */
int64_t ctasnet_frames(int64_t T);
int64_t ctasnet_out_len(int64_t T);
/* Workspace of one forward of B mixtures of T samples; 0 for an unsupported shape (message: ctasnet_last_error). */
size_t ctasnet_workspace_bytes(ctasnet_handle h, int B, int64_t T);

/* ConvTasNet.forward (convtasnet.py:110-116): mix [B][T] -> s1_pred, s2_pred [B][ctasnet_out_len(T)]. */
int ctasnet_forward(ctasnet_handle h, const float* mix, int B, int64_t T, float* s1_pred, float* s2_pred, void* ws,
                    size_t ws_bytes, void* stream);

/* Cost model of one mixture's forward: algorithmic FLOPs (2 per MAC) and the bytes the launches of this implementation
 * read and write when nothing stays cached between them. */
double ctasnet_flops_per_mixture(ctasnet_handle h, int64_t T);
double ctasnet_min_bytes_per_mixture(ctasnet_handle h, int64_t T);

#ifdef __cplusplus
}
#endif
#endif /* CTASNET_H_ */
