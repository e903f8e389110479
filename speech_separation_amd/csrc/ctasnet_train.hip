// ctasnet_train.hip -- Conv-TasNet training step (src/model/convtasnet.py forward + its autograd backward) for gfx950:
// handle and the extern "C" boundary declared in include/ctasnet_train.h.
//
// Training forward: the launch sequence of ctasnet.hip in its TAPE mode (ctasnet_kernels.h: one text for both), every
// block writing into its own slice of a tape; the predictions are bitwise those of ctasnet_forward and the backward sees
// the sign of each pre-activation whatever the slope.  Tape per block: x_i [M][128], v1 [M][512], u [M][512], two
// statistics pairs per mixture; once: enc [M][512], GlobalNorm statistics, the final skip sum [M][128], ym [M][1024] and
// the sigmoid masks [M][1024].
//
// Backward (reverse order): decoder taps gradient and d D; then launch_separator_backward (ctasnet_train_kernels.h, shared
// with the deep model's training unit): mask head (sigmoid, both d enc contributions of the head, d v, seq.1 weight / bias,
// PReLU seq.0), 24 blocks (res|skip dgrad, norm_2, PReLU_2, depthwise conv, norm_1, PReLU_1, 1x1 dgrad + residual),
// bottleneck and GlobalNorm; encoder weight.  Every partial is summed by cttrain_reduce_kernel in slab order: no atomics,
// fixed grids, so repeated backward calls are bitwise identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ctasnet_train.h"
#include "ctasnet_train_kernels.h"

static_assert(CTTRAIN_OK == CTASNET_OK && CTTRAIN_ERR_INVALID == CTASNET_ERR_INVALID &&
                  CTTRAIN_ERR_WORKSPACE == CTASNET_ERR_WORKSPACE && CTTRAIN_ERR_WEIGHTS == CTASNET_ERR_WEIGHTS &&
                  CTTRAIN_ERR_HIP == CTASNET_ERR_HIP,
              "the shared Conv-TasNet code returns CTASNET_* codes");

static_assert(CTTRAIN_TAPE_V1 == SEP_TAPE_V1 && CTTRAIN_TAPE_U == SEP_TAPE_U && CTTRAIN_TAPE_SKIP == SEP_TAPE_SKIP,
              "sep_tape_offset takes the header's tape kinds");

struct cttrain_ctx : CtTrainHandle {
  cttrain_ctx() : CtTrainHandle("cttrain", -1) {}
};

namespace {

thread_local std::string g_create_error;

using Plan = TrainPlanBase;

int make_plan(CtHandle* c, int B, int64_t T, Plan& p) {
  if (int rc = plan_train_head(c, B, T, "B*F*1024", p)) return rc;
  ByteCursor cur;
  plan_separator_train(p, cur, B, (size_t)p.M);
  p.total = cur.o;
  return CTTRAIN_OK;
}

}  // namespace

extern "C" {

int cttrain_abi_version(void) { return CTTRAIN_ABI_VERSION; }

int cttrain_create(cttrain_handle* out) {
  if (int rc = ct_create(out, "Conv-TasNet training step", g_create_error)) return rc;
  cttrain_ctx* c = *out;
  add_convtasnet_names(c);
  c->w.assign(c->names.size(), nullptr);
  c->g.assign(c->names.size(), nullptr);
  return CTTRAIN_OK;
}

void cttrain_destroy(cttrain_handle h) { delete h; }

const char* cttrain_last_error(cttrain_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int cttrain_num_weights(cttrain_handle h) { return h ? (int)h->names.size() : 0; }

const char* cttrain_weight_name(cttrain_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t cttrain_weight_numel(cttrain_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int cttrain_bind_weights(cttrain_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n) : CTTRAIN_ERR_INVALID;
}

int cttrain_bind_grads(cttrain_handle h, float* const* dev_ptrs, int n) {
  return h ? bind_grads(h, dev_ptrs, n) : CTTRAIN_ERR_INVALID;
}

int64_t cttrain_flat_offset(cttrain_handle h, int slot) { return h ? flat_offset(h, slot) : -1; }

int64_t cttrain_flat_numel(cttrain_handle h) { return h ? flat_numel(h) : -1; }

int64_t cttrain_frames(int64_t T) { return frames_of(T); }

int64_t cttrain_out_len(int64_t T) { return out_len_of(T); }

size_t cttrain_workspace_bytes(cttrain_handle h, int B, int64_t T) {
  if (!h) return 0;
  Plan p;
  if (make_plan(h, B, T, p)) return 0;
  return p.total;
}

int64_t cttrain_tape_offset(cttrain_handle h, int B, int64_t T, int which, int block) {
  if (!h) return -1;
  Plan p;
  if (make_plan(h, B, T, p)) return -1;
  return sep_tape_offset(h, p, which, block);
}

int cttrain_train_forward(cttrain_handle h, const float* mix, int B, int64_t T, float* s1_pred, float* s2_pred, void* ws,
                          size_t ws_bytes, void* stream) {
  cttrain_ctx* c = h;
  Plan p;
  WsPtr at;
  if (int rc = train_prologue(c, make_plan, false, mix, s1_pred, s2_pred, B, T, ws, ws_bytes, p, at)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  float* enc = at.fp(p.off_enc);
  float* taps = at.fp(p.off_taps);
  const SepBuffers sb = sep_tape_buffers(p, ws);
  const unsigned row_wgs = (unsigned)((M + CT_ROWS_PER_WG - 1) / CT_ROWS_PER_WG);

  // as ctasnet_forward, on the tape: encoder (convtasnet.py:12-15), Separator (:55-83), decoder taps and overlap-add (:92-97)
  hipLaunchKernelGGL(ctasnet_encoder_kernel<false>, dim3(row_wgs), dim3(256), 0, st, mix, T, F, M, W[0], nullptr, enc, sb.part);
  HANDLE_LAUNCH_CHECK(c, "cttrain encoder");
  if (int rc = launch_separator<true>(c, st, W.data() + 1, enc, 2, 256.0f, B, F, M, sb)) return rc;
  if (int rc = launch_taps(c, st, sb.ym, W[1 + CT_SEP_W], M, taps)) return rc;
  return launch_overlap_add<false>(c, st, taps, nullptr, B, F, p.Lout, s1_pred, s2_pred);
}

int cttrain_train_backward(cttrain_handle h, const float* mix, int B, int64_t T, const float* d_s1, const float* d_s2, void* ws,
                           size_t ws_bytes, void* stream) {
  cttrain_ctx* c = h;
  Plan p;
  WsPtr at;
  if (int rc = train_prologue(c, make_plan, true, mix, d_s1, d_s2, B, T, ws, ws_bytes, p, at)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  const auto& G = c->g;
  const int SEP = 1, DEC = 1 + CT_SEP_W;
  float* ym = at.fp(p.off_ym);
  float* dtaps = at.fp(p.off_taps);
  float* denc = at.fp(p.off_denc);
  float* slab = at.fp(p.off_slab);
  int ns = 0;

  // ---- decoder (convtasnet.py:92-97): d taps, d D[n][k] = sum over (row, s) ym[row][512 s + n] dtaps[row][s][k]
  {
    const int64_t n = M * 4 * CT_L;
    hipLaunchKernelGGL(cttrain_dtaps_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_s1, d_s2, F, M, p.Lout, dtaps);
    HANDLE_LAUNCH_CHECK(c, "cttrain dtaps");
    if (int rc = launch_wgrad<CT_N, 2 * CT_L>(c, st, 2 * M, ALoadDense{ym, 2 * M, CT_N, 32}, ALoadDense{dtaps, 2 * M, 2 * CT_L, 32},
                                              slab, &ns))
      return rc;
    if (int rc = launch_reduce(c, st, slab, ns, (int64_t)CT_N * 2 * CT_L, CT_N, 2 * CT_L, G[DEC], 2 * CT_L)) return rc;
  }

  // ---- Separator (convtasnet.py:55-83): mask head from the taps gradient, 24 blocks, bottleneck, GlobalNorm -> d enc
  if (int rc = launch_separator_backward<HEAD_TAPS>(c, st, W.data() + SEP, G.data() + SEP, dtaps, W[DEC], B, F, M, p, ws))
    return rc;

  // ---- encoder weight (convtasnet.py:12-15): d W[n][k] = sum_rows d enc[row][n] xpad[16 f + k]
  if (int rc = launch_wgrad<CT_N, 2 * CT_L>(c, st, M, ALoadDense{denc, M, CT_N, 32}, ALoadPatches{mix, T, M, F}, slab, &ns))
    return rc;
  return launch_reduce(c, st, slab, ns, (int64_t)CT_N * 2 * CT_L, CT_N, 2 * CT_L, G[0], 2 * CT_L);
}

size_t cttrain_clip_scratch_bytes(cttrain_handle) { return CLIP_PARTS * sizeof(double); }

int cttrain_grad_clip(cttrain_handle h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                      float* norm_out, void* stream) {
  return h ? train_grad_clip(h, flat_grad, n_flat, max_norm, scratch, scratch_bytes, norm_out, stream) : CTTRAIN_ERR_INVALID;
}

int cttrain_adamw_step(cttrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                       double beta1, double beta2, double eps, double weight_decay, int step, void* stream) {
  return h ? train_adamw_step(h, flat_grad, exp_avg, exp_avg_sq, n_flat, lr, beta1, beta2, eps, weight_decay, step, stream)
           : CTTRAIN_ERR_INVALID;
}

double cttrain_flops_per_mixture(cttrain_handle, int64_t T) {
  // forward MACs (ctasnet_flops_per_mixture) x 3: the backward is one data-gradient and one weight-gradient product per
  // forward product
  return 3.0 * 2.0 * convtasnet_macs() * (double)frames_of(T);
}

}  // extern "C"
