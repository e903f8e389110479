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

namespace {

thread_local std::string g_create_error;

struct Plan : SepTrainPlan {
  int64_t F, M, Lout;
  size_t total;
};

}  // namespace

struct cttrain_ctx : CtHandle {
  std::vector<float*> g;
  bool gbound = false;
};

namespace {

int make_plan(cttrain_ctx* c, int B, int64_t T, Plan& p) {
  if (int rc = check_batch(c, B, T)) return rc;
  p.F = frames_of(T);
  p.M = (int64_t)B * p.F;
  if (p.M * 2 * CT_N > (int64_t)INT32_MAX)
    return c->fail(CTTRAIN_ERR_INVALID, "B*F*1024 = %lld exceeds 32-bit indexing (B=%d, T=%lld)", (long long)(p.M * 2 * CT_N), B,
                   (long long)T);
  p.Lout = CT_L * (T / CT_L);
  size_t o = 0;
  plan_separator_train(p, o, B, (size_t)p.M);
  p.total = o;
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
  if (!h) return CTTRAIN_ERR_INVALID;
  if (int rc = check_table_ptrs(h, reinterpret_cast<const void* const*>(dev_ptrs), n, "gradient", 4)) return rc;
  h->g.assign(dev_ptrs, dev_ptrs + n);
  h->gbound = true;
  return CTTRAIN_OK;
}

int64_t cttrain_flat_offset(cttrain_handle h, int slot) {
  if (!h || slot < 0 || slot > (int)h->numels.size()) return -1;
  int64_t o = 0;
  for (int i = 0; i < slot; ++i) o += (int64_t)align64f((size_t)h->numels[i]);
  return o;
}

int64_t cttrain_flat_numel(cttrain_handle h) { return h ? cttrain_flat_offset(h, (int)h->numels.size()) : -1; }

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
  const size_t M = (size_t)p.M;
  if (which == CTTRAIN_TAPE_SKIP) return block == 0 ? (int64_t)p.off_skip : -1;
  if (block < 0 || block >= CT_BLOCKS) {
    h->fail(CTTRAIN_ERR_INVALID, "block %d out of range", block);
    return -1;
  }
  if (which == CTTRAIN_TAPE_V1) return (int64_t)(p.off_v1 + (size_t)block * M * CT_H * 4);
  if (which == CTTRAIN_TAPE_U) return (int64_t)(p.off_u + (size_t)block * M * CT_H * 4);
  h->fail(CTTRAIN_ERR_INVALID, "unknown tape tensor %d", which);
  return -1;
}

int cttrain_train_forward(cttrain_handle h, const float* mix, int B, int64_t T, float* s1_pred, float* s2_pred, void* ws,
                          size_t ws_bytes, void* stream) {
  if (!h) return CTTRAIN_ERR_INVALID;
  cttrain_ctx* c = h;
  if (!c->bound) return c->fail(CTTRAIN_ERR_WEIGHTS, "weights not bound (cttrain_bind_weights)");
  if (!mix || !s1_pred || !s2_pred) return c->fail(CTTRAIN_ERR_INVALID, "mix / s1_pred / s2_pred must not be NULL");
  Plan p;
  if (int rc = make_plan(c, B, T, p)) return rc;
  if (int rc = check_workspace(c, p.total, ws, ws_bytes)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  auto fp = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  auto f2 = [&](size_t off) { return reinterpret_cast<float2*>(base + off); };
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  float* enc = fp(p.off_enc);
  float2* part = f2(p.off_part);
  float* ym = fp(p.off_ym);
  float* taps = fp(p.off_taps);
  const SepBuffers sb{fp(p.off_x), fp(p.off_skip), fp(p.off_v1), fp(p.off_u), part, f2(p.off_stats0), f2(p.off_st1),
                      f2(p.off_st2), ym, fp(p.off_mk)};
  const unsigned row_wgs = (unsigned)((M + CT_ROWS_PER_WG - 1) / CT_ROWS_PER_WG);

  // as ctasnet_forward, on the tape: encoder (convtasnet.py:12-15), Separator (:55-83), decoder taps and overlap-add (:92-97)
  hipLaunchKernelGGL(ctasnet_encoder_kernel<false>, dim3(row_wgs), dim3(256), 0, st, mix, T, F, M, W[0], nullptr, enc, part);
  CT_LAUNCH_CHECK(c, "cttrain encoder");
  if (int rc = launch_separator<true>(c, st, W.data() + 1, enc, 2, 256.0f, B, F, M, sb)) return rc;
  if (int rc = launch_taps(c, st, ym, W[1 + CT_SEP_W], M, taps)) return rc;
  return launch_overlap_add<false>(c, st, taps, nullptr, B, F, p.Lout, s1_pred, s2_pred);
}

int cttrain_train_backward(cttrain_handle h, const float* mix, int B, int64_t T, const float* d_s1, const float* d_s2, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!h) return CTTRAIN_ERR_INVALID;
  cttrain_ctx* c = h;
  if (!c->bound) return c->fail(CTTRAIN_ERR_WEIGHTS, "weights not bound (cttrain_bind_weights)");
  if (!c->gbound) return c->fail(CTTRAIN_ERR_WEIGHTS, "gradients not bound (cttrain_bind_grads)");
  if (!mix || !d_s1 || !d_s2) return c->fail(CTTRAIN_ERR_INVALID, "mix / d_s1 / d_s2 must not be NULL");
  Plan p;
  if (int rc = make_plan(c, B, T, p)) return rc;
  if (int rc = check_workspace(c, p.total, ws, ws_bytes)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  auto fp = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  const auto& G = c->g;
  const int SEP = 1, DEC = 1 + CT_SEP_W;
  float* ym = fp(p.off_ym);
  float* dtaps = fp(p.off_taps);
  float* denc = fp(p.off_denc);
  float* slab = fp(p.off_slab);
  int ns = 0;

  // ---- decoder (convtasnet.py:92-97): d taps, d D[n][k] = sum over (row, s) ym[row][512 s + n] dtaps[row][s][k]
  {
    const int64_t n = M * 4 * CT_L;
    hipLaunchKernelGGL(cttrain_dtaps_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_s1, d_s2, F, M, p.Lout, dtaps);
    CT_LAUNCH_CHECK(c, "cttrain dtaps");
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
  if (!h) return CTTRAIN_ERR_INVALID;
  if (!flat_grad || !norm_out || n_flat < 4 || (n_flat & 3) || ((uintptr_t)flat_grad & 15))
    return h->fail(CTTRAIN_ERR_INVALID, "grad_clip: flat gradient must be 16-byte aligned with a multiple of 4 floats");
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < CLIP_PARTS * sizeof(double))
    return h->fail(CTTRAIN_ERR_WORKSPACE, "grad_clip: scratch too small / misaligned");
  hipStream_t st = (hipStream_t)stream;
  double* partials = (double*)scratch;
  hipLaunchKernelGGL(sumsq_partials_kernel, dim3(CLIP_PARTS), dim3(256), 0, st, flat_grad, n_flat / 4, partials);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(h->num_cus * 2), dim3(256), 0, st, flat_grad, n_flat / 4, partials, CLIP_PARTS,
                     max_norm, norm_out);
  CT_LAUNCH_CHECK(h, "cttrain grad_clip");
  return CTTRAIN_OK;
}

int cttrain_adamw_step(cttrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                       double beta1, double beta2, double eps, double weight_decay, int step, void* stream) {
  if (!h) return CTTRAIN_ERR_INVALID;
  if (!h->bound) return h->fail(CTTRAIN_ERR_WEIGHTS, "adamw_step: weights not bound (the step updates the bound parameters in place)");
  if (!flat_grad || !exp_avg || !exp_avg_sq || n_flat != cttrain_flat_numel(h) || step < 1)
    return h->fail(CTTRAIN_ERR_INVALID, "adamw_step: bad argument (flat buffers must hold %lld floats, step >= 1)",
                   (long long)cttrain_flat_numel(h));
  // constants formed in double and rounded once, as torch does (dptnav_adamw_step)
  const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
  const float step_size = (float)(lr / bc1), inv_sqrt_bc2 = (float)(1.0 / std::sqrt(bc2));
  const float decay = (float)(1.0 - lr * weight_decay);
  const int n = (int)h->names.size();
  int64_t off = 0;
  for (int lo = 0; lo < n; lo += ADAMW_MAX) {
    AdamwArgs a{};
    const int cnt = std::min(ADAMW_MAX, n - lo);
    for (int e = 0; e < cnt; ++e) {
      a.param[e] = const_cast<float*>(h->w[lo + e]);
      a.off[e] = off;
      a.n[e] = (int)h->numels[lo + e];
      off += (int64_t)align64f((size_t)h->numels[lo + e]);
    }
    hipLaunchKernelGGL(adamw_kernel, dim3(cnt, ADAMW_YBLOCKS), dim3(256), 0, (hipStream_t)stream, a, flat_grad, exp_avg,
                       exp_avg_sq, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, decay,
                       step_size, inv_sqrt_bc2);
    CT_LAUNCH_CHECK(h, "cttrain adamw_step");
  }
  return CTTRAIN_OK;
}

double cttrain_flops_per_mixture(cttrain_handle, int64_t T) {
  // forward MACs (ctasnet_flops_per_mixture) x 3: the backward is one data-gradient and one weight-gradient product per
  // forward product
  return 3.0 * 2.0 * convtasnet_macs() * (double)frames_of(T);
}

}  // extern "C"
