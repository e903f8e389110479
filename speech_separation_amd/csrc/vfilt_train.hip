// vfilt_train.hip -- the VoiceFilter training step (src/model/voicefilter.py:108-145 in training mode and its backward) for
// gfx950: handle and the extern "C" boundary declared in include/vfilt_train.h; the kernels are in vfilt_train_kernels.h,
// vfilt_kernels.h and lipfe_kernels.h, clip and AdamW in train_tail.h.
//
// train_forward, all on the caller's stream (F = input_size, q = speaker * B + item, pos = B F W):
//   CNN          per layer: the raw Z = conv + bias (layers 2..7 on lipfe_conv_kernel with scale 1 / shift bias), the batch
//                mean and variance by a two-stage reduction over chunks of 1024 positions (mean first, then the squares of
//                the differences), then a normalise (+ ReLU) pass of its own -> A.  Z and A of every layer stay on the tape.
//   d-vector     as vfilt.hip, on one concatenated copy of the two speakers' embeddings; the GRU kernels store r, z, n and
//                W_hn h + b_hn of every step
//   LSTM         one launch per step; the step stores its four gate activations, c and h of the step before
//   tail         ReLU, Linear(400, 600), ReLU -> Y1; frame dropout -> Yd; Linear(600, F), sigmoid -> S; S x mixture
// train_backward walks the same graph in reverse; every dense product (weight gradients included) is vfilt_gemm_kernel, the
// weight gradient of layers 2..7 is vftrain_wgrad_kernel + vftrain_wgrad_sum_kernel, their data gradient lipfe_conv_kernel on
// the flipped pack.  Column sums, BatchNorm sums and partial tiles are added in an order the shape alone decides.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vfilt_train.h"
#include "vfilt_train_kernels.h"
#include "train_tail.h"

HANDLE_ASSERT_CODES(VFTRAIN);

namespace {
thread_local std::string g_vft_create_error;

const int VFT_KH[6] = {7, 5, 5, 5, 5, 5};
const int VFT_KW[6] = {1, 5, 5, 5, 5, 5};
const int VFT_DIL[6] = {1, 1, 2, 4, 8, 16};
const int VFT_CONV_IDX[VF_LAYERS] = {1, 5, 9, 13, 17, 21, 25, 28};
const int VFT_BN_IDX[VF_LAYERS] = {2, 6, 10, 14, 18, 22, 26, 29};

struct VftPlan {
  int nseq;
  long long pos;
  int nchunk, nwchunk;    // chunks of 1024 / 4096 positions
  // tape
  size_t off_fold, off_pack, off_Z[VF_LAYERS], off_A[7], off_flat, off_stat, off_block, off_cat, off_gi0, off_y0, off_gi1, off_y1,
      off_gi1b, off_whht, off_tape0, off_tape1, off_tape1b, off_dvec, off_D, off_G, off_H, off_hprev, off_gates, off_cell, off_y1fc,
      off_keep, off_yd, off_S;
  // scratch of the backward
  size_t off_packT, off_dP, off_dY, off_dH, off_dgates, off_dcst, off_lwhht, off_dGsum, off_dGt, off_viewT, off_dflat, off_ddvec,
      off_dglast, off_dgi1, off_dgh1, off_hp1, off_dgi1b, off_dgh1b, off_dy0, off_tmp2f, off_dgi0, off_dgh0, off_hp0, off_dZ8,
      off_dA, off_dZ, off_coef, off_parts, total;
};
}  // namespace

struct vftrain_ctx : Handle {
  int F = 0, E = 0;
  int gru[2][2];
  int fcd;
  int conv[VF_LAYERS];
  int bn[VF_LAYERS];
  int lstm;
  int fc1, fc2;
  int64_t pack_off[6], pack_floats = 0;
  std::vector<float*> g;
  std::vector<char> no_grad;     // per slot: the running statistics
  bool gbound = false;
  // the tape the last train_forward left
  const void* tape_ws = nullptr;
  int tape_B = 0, tape_W = 0, tape_Tv = 0;
  float tape_inv_keep = 1.f;
};

namespace {
// vfilt.hip's table: the reference's state_dict() order without num_batches_tracked
void vft_build_table(vftrain_ctx* c) {
  const int64_t F = c->F, E = c->E;
  for (int l = 0; l < 2; ++l)
    for (int d = 0; d < 2; ++d) {
      const std::string s = "_l" + std::to_string(l) + (d ? "_reverse" : "");
      c->gru[l][d] = c->add("gru.weight_ih" + s, 3 * F * (l == 0 ? E : 2 * F));
      c->add("gru.weight_hh" + s, 3 * F * F);
      c->add("gru.bias_ih" + s, 3 * F);
      c->add("gru.bias_hh" + s, 3 * F);
    }
  c->fcd = c->add("fc_dvector.weight", F * 2 * F);
  c->add("fc_dvector.bias", F);
  for (int l = 0; l < VF_LAYERS; ++l) {
    const int cout = l == 7 ? VF_C8 : VF_C;
    const int64_t per_out = l == 0 ? 7 : l == 7 ? VF_C : (int64_t)VF_C * VFT_KH[l - 1] * VFT_KW[l - 1];
    const std::string pc = "cnn_layers." + std::to_string(VFT_CONV_IDX[l]) + ".";
    const std::string pb = "cnn_layers." + std::to_string(VFT_BN_IDX[l]) + ".";
    c->conv[l] = c->add(pc + "weight", cout * per_out);
    c->add(pc + "bias", cout);
    c->bn[l] = c->add(pb + "weight", cout);
    c->add(pb + "bias", cout);  c->add(pb + "running_mean", cout);  c->add(pb + "running_var", cout);
    if (l >= 1 && l <= 6) { c->pack_off[l - 1] = c->pack_floats;  c->pack_floats += cout * per_out; }
  }
  c->lstm = c->add("lstm.weight_ih_l0", (int64_t)VF_G * 9 * F);
  c->add("lstm.weight_hh_l0", (int64_t)VF_G * VF_H);
  c->add("lstm.bias_ih_l0", VF_G);
  c->add("lstm.bias_hh_l0", VF_G);
  c->fc1 = c->add("fc.1.weight", (int64_t)VF_FC * VF_H);
  c->add("fc.1.bias", VF_FC);
  c->fc2 = c->add("fc.4.weight", F * VF_FC);
  c->add("fc.4.bias", F);
  c->w.assign(c->names.size(), nullptr);
  c->no_grad.assign(c->names.size(), 0);
  for (int l = 0; l < VF_LAYERS; ++l) c->no_grad[c->bn[l] + 2] = c->no_grad[c->bn[l] + 3] = 1;
}

const char* vft_check_shape(int F, int B, int W, int Tv) {
  if (B < 1) return "B must be >= 1";
  if (W < 1) return "W must be >= 1";
  if (Tv < 1) return "Tv must be >= 1";
  if ((double)B * F * W < 2.0) return "batch statistics need B * input_size * W >= 2";
  if ((double)B * F * W * VF_C >= 2147483648.0) return "B * input_size * W * 64 must stay below 2^31";
  if (2.0 * B * (W > Tv ? W : Tv) * VF_G >= 2147483648.0) return "2 * B * max(W, Tv) * 1600 must stay below 2^31";
  return nullptr;
}

int vft_make_plan(vftrain_ctx* c, int B, int W, int Tv, VftPlan& p) {
  if (const char* why = vft_check_shape(c->F, B, W, Tv))
    return c->fail(VFTRAIN_ERR_INVALID, "%s (got B=%d W=%d Tv=%d, input_size=%d)", why, B, W, Tv, c->F);
  const size_t F = c->F, E = c->E, nseq = 2 * (size_t)B;
  const size_t pos = (size_t)B * F * W, rows = nseq * W, vrows = nseq * Tv;
  p.nseq = (int)nseq;
  p.pos = (long long)pos;
  p.nchunk = (int)((pos + VFT_CHUNK - 1) / VFT_CHUNK);
  p.nwchunk = (int)((pos + VFT_WG_CHUNK - 1) / VFT_WG_CHUNK);
  ByteCursor cur;
  auto take = [&](size_t floats) { return cur.take(floats * 4); };
  p.off_fold = take(128 * (VF_LAYERS + 1));
  p.off_pack = take((size_t)c->pack_floats);
  for (int l = 0; l < 7; ++l) p.off_Z[l] = take(pos * VF_C);
  p.off_Z[7] = take(pos * VF_C8);
  for (int l = 0; l < 7; ++l) p.off_A[l] = take(pos * VF_C);
  p.off_flat = take(pos * VF_C8);
  p.off_stat = take((size_t)VF_LAYERS * VFT_STAT);
  p.off_block = take((size_t)VF_LAYERS * 128);
  p.off_cat = take(vrows * E);
  p.off_gi0 = take(2 * vrows * 3 * F);
  p.off_y0 = take(vrows * 2 * F);
  p.off_gi1 = take(vrows * 3 * F);
  p.off_y1 = take(vrows * 2 * F);
  p.off_gi1b = take(nseq * 3 * F);
  p.off_whht = take(3 * 3 * F * F);
  p.off_tape0 = take(2 * vrows * 4 * F);
  p.off_tape1 = take(vrows * 4 * F);
  p.off_tape1b = take(nseq * 4 * F);
  p.off_dvec = take(nseq * F);
  p.off_D = take(nseq * VF_G);
  p.off_G = take((size_t)B * W * VF_G);
  p.off_H = take(rows * VF_H);
  p.off_hprev = take(rows * VF_H);
  p.off_gates = take(rows * VF_G);
  p.off_cell = take(rows * VF_H);
  p.off_y1fc = take(rows * VF_FC);
  p.off_keep = take(rows);
  p.off_yd = take(rows * VF_FC);
  p.off_S = take(rows * F);
  // backward
  p.off_packT = take((size_t)c->pack_floats);
  p.off_dP = take(rows * F);
  p.off_dY = take(rows * VF_FC);
  p.off_dH = take(rows * VF_H);
  p.off_dgates = take(rows * VF_G);
  p.off_dcst = take(nseq * VF_H);
  p.off_lwhht = take((size_t)VF_G * VF_H);
  p.off_dGsum = take((size_t)B * W * VF_G);
  p.off_dGt = take(nseq * VF_G);
  p.off_viewT = take((size_t)B * W * 8 * F);
  p.off_dflat = take(pos * VF_C8);
  p.off_ddvec = take(nseq * F);
  p.off_dglast = take(nseq * 2 * F);
  p.off_dgi1 = take(vrows * 3 * F);
  p.off_dgh1 = take(vrows * 3 * F);
  p.off_hp1 = take(vrows * F);
  p.off_dgi1b = take(nseq * 3 * F);
  p.off_dgh1b = take(nseq * 3 * F);
  p.off_dy0 = take(vrows * 2 * F);
  p.off_tmp2f = take(nseq * 2 * F);
  p.off_dgi0 = take(2 * vrows * 3 * F);
  p.off_dgh0 = take(2 * vrows * 3 * F);
  p.off_hp0 = take(2 * vrows * F);
  p.off_dZ8 = take(pos * VF_C8);
  p.off_dA = take(pos * VF_C);
  p.off_dZ = take(pos * VF_C);
  p.off_coef = take(VFT_COEF);
  size_t parts = (size_t)p.nchunk * 8 * 64;                                  // every VALU first stage fits 8 x 64 floats per chunk
  const size_t wparts = (size_t)p.nwchunk * 25 * 64 * 64;
  if (wparts > parts) parts = wparts;
  p.off_parts = take(parts);
  p.total = cur.o;
  return VFTRAIN_OK;
}

VfGemmArgs vft_gemm_args(const float* A, long long sam, long long sak, const float* Bw, long long sbn, long long sbk,
                         const float* bias, float* C, long long scm, long long scn, int M, int N, int K) {
  VfGemmArgs a;
  a.A = A;  a.sam = sam;  a.sak = sak;  a.sab = 0;
  a.Bw = Bw;  a.sbn = sbn;  a.sbk = sbk;
  a.bias = bias;  a.bias2 = nullptr;  a.mul = nullptr;
  a.C = C;  a.scm = scm;  a.scn = scn;  a.scb = 0;
  a.M = M;  a.N = N;  a.K = K;  a.mtiles = (M + LF_BM - 1) / LF_BM;
  a.relu_a = 0;  a.act = VF_ACT_NONE;
  return a;
}

int vft_launch_gemm(vftrain_ctx* c, hipStream_t st, const VfGemmArgs& a, int batches, const char* what) {
  const dim3 grid((unsigned)((long long)a.mtiles * batches), (unsigned)((a.N + LF_BN - 1) / LF_BN));
  hipLaunchKernelGGL(vfilt_gemm_kernel, grid, dim3(256), 0, st, a);
  HANDLE_LAUNCH_CHECK(c, what);
  return VFTRAIN_OK;
}

// C [M][N] (row stride ldc) = A^T B with A [K][M], B [K][N] (row stride ldb), both row-major: a weight gradient
int vft_gemm_tn(vftrain_ctx* c, hipStream_t st, const float* A, int M, const float* Bm, long long ldb, int N, int K, float* C,
                long long ldc, const char* what) {
  return vft_launch_gemm(c, st, vft_gemm_args(A, 1, M, Bm, 1, ldb, nullptr, C, ldc, 1, M, N, K), 1, what);
}

// C [M][N] = A B with A [M][K] row-major, B [K][N] with row stride ldb: a data gradient through y = x W^T (B = W)
int vft_gemm_nn(vftrain_ctx* c, hipStream_t st, const float* A, int M, int K, const float* Bm, long long ldb, int N, float* C,
                const char* what) {
  return vft_launch_gemm(c, st, vft_gemm_args(A, K, 1, Bm, 1, ldb, nullptr, C, N, 1, M, N, K), 1, what);
}

int vft_colsum(vftrain_ctx* c, hipStream_t st, const float* X, int rows, int C, int batches, float* out, float* out2) {
  hipLaunchKernelGGL(vftrain_colsum_kernel, dim3((C + 63) / 64, batches), dim3(256), 0, st, X, rows, C, (long long)rows * C, out, out2);
  HANDLE_LAUNCH_CHECK(c, "vftrain colsum");
  return VFTRAIN_OK;
}

unsigned vft_blocks(long long n) { return (unsigned)((n + 255) / 256); }

// batch statistics of X [n][C] -> stat (mean, invstd), block (mean, unbiased variance)
template <int C>
int vft_stats(vftrain_ctx* c, hipStream_t st, const float* X, long long n, float* parts, float* stat, float* block) {
  const int np = (int)((n + VFT_CHUNK - 1) / VFT_CHUNK);
  double* dparts = reinterpret_cast<double*>(parts);
  hipLaunchKernelGGL((vftrain_stat_part_kernel<C, false>), dim3(np), dim3(256), 0, st, X, n, (const float*)nullptr, dparts);
  hipLaunchKernelGGL(vftrain_stat_mean_kernel, dim3(1), dim3(64), 0, st, (const double*)dparts, np, C, n, stat);
  hipLaunchKernelGGL((vftrain_stat_part_kernel<C, true>), dim3(np), dim3(256), 0, st, X, n, (const float*)stat, dparts);
  hipLaunchKernelGGL(vftrain_stat_var_kernel, dim3(1), dim3(64), 0, st, (const double*)dparts, np, C, n, stat, block);
  HANDLE_LAUNCH_CHECK(c, "vftrain batch statistics");
  return VFTRAIN_OK;
}

// BatchNorm backward of X [n][C]: dA (masked where A <= 0 when A is given) -> dZ; d gamma, d beta, d conv bias
template <int C>
int vft_bn_bwd(vftrain_ctx* c, hipStream_t st, const float* dA, const float* A, const float* Z, const float* stat, long long n,
               const float* gamma, float* parts, float* coef, float* dZ, float* dgamma, float* dbeta, float* dbias) {
  const int np = (int)((n + VFT_CHUNK - 1) / VFT_CHUNK);
  double* dparts = reinterpret_cast<double*>(parts);
  hipLaunchKernelGGL(vftrain_bn_bwd_part_kernel<C>, dim3(np), dim3(256), 0, st, dA, A, Z, stat, n, dparts);
  hipLaunchKernelGGL(vftrain_bn_bwd_final_kernel, dim3(1), dim3(64), 0, st, (const double*)dparts, np, C, n, gamma, stat, coef, dgamma, dbeta, dbias);
  hipLaunchKernelGGL(vftrain_bn_bwd_apply_kernel<C>, dim3(vft_blocks(n * C / 4)), dim3(256), 0, st, dA, A, Z, stat, coef, dZ, n * C / 4);
  HANDLE_LAUNCH_CHECK(c, "vftrain BatchNorm backward");
  return VFTRAIN_OK;
}

double vft_macs(int F, int E, int W, int Tv) {
  const double f = F, pos = f * W;
  double conv = 64.0 * 7 + 64.0 * 64 * 7 + 5.0 * 64 * 64 * 25 + 64.0 * 8;
  double m = pos * conv;
  m += (double)W * 8 * f * VF_G;
  m += 2.0 * (f * VF_G + (double)W * VF_G * VF_H);
  m += 2.0 * W * ((double)VF_H * VF_FC + (double)VF_FC * f);
  m += 2.0 * (Tv * (2.0 * 3 * f * (E + f) + 3 * f * (2 * f + f)) + 3 * f * 2 * f + f * 2 * f);
  return m;
}

int vft_prologue(vftrain_ctx* c, bool backward, const void* mix, const void* e1, const void* e2, const void* o1, const void* o2,
                 int B, int W, int Tv, void* ws, size_t ws_bytes, VftPlan& p) {
  if (!c->bound) return c->fail(VFTRAIN_ERR_WEIGHTS, "weights not bound (vftrain_bind_weights)");
  if (backward && !c->gbound) return c->fail(VFTRAIN_ERR_WEIGHTS, "gradients not bound (vftrain_bind_grads)");
  if (!mix || !e1 || !e2 || !o1 || !o2)
    return c->fail(VFTRAIN_ERR_INVALID, "mix_magnitude / emb1 / emb2 / %s must not be NULL", backward ? "d_out1 / d_out2" : "out1 / out2");
  if (int rc = vft_make_plan(c, B, W, Tv, p)) return rc;
  return check_workspace(c, p.total, ws, ws_bytes);
}
}  // namespace

extern "C" {

int vftrain_abi_version(void) { return VFTRAIN_ABI_VERSION; }

int vftrain_create(vftrain_handle* out, int input_size, int embed_size) {
  if (out && (input_size < 1 || input_size > VF_FMAX))
    return refuse_create(out, g_vft_create_error, "input_size must be in [1, 257] (got " + std::to_string(input_size) + ")");
  if (out && embed_size != 512 && embed_size != 1024)
    return refuse_create(out, g_vft_create_error, "embed_size must be 512 or 1024 (got " + std::to_string(embed_size) + ")");
  if (int rc = create(out, "VoiceFilter training step", g_vft_create_error)) return rc;
  (*out)->F = input_size;
  (*out)->E = embed_size;
  vft_build_table(*out);
  return VFTRAIN_OK;
}

void vftrain_destroy(vftrain_handle h) { delete h; }

const char* vftrain_last_error(vftrain_handle h) { return h ? h->err.c_str() : g_vft_create_error.c_str(); }

int vftrain_num_weights(vftrain_handle h) { return h ? (int)h->names.size() : 0; }

const char* vftrain_weight_name(vftrain_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t vftrain_weight_numel(vftrain_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int vftrain_bind_weights(vftrain_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n, 4) : VFTRAIN_ERR_INVALID;
}

int vftrain_bind_grads(vftrain_handle h, float* const* dev_ptrs, int n) {
  if (!h) return VFTRAIN_ERR_INVALID;
  if (int rc = check_table_ptrs(h, reinterpret_cast<const void* const*>(dev_ptrs), n, "gradient", 4)) return rc;
  h->g.assign(dev_ptrs, dev_ptrs + n);
  h->gbound = true;
  return VFTRAIN_OK;
}

int64_t vftrain_flat_offset(vftrain_handle h, int slot) {
  if (!h || slot < 0 || slot > (int)h->numels.size()) return -1;
  int64_t o = 0;
  for (int i = 0; i < slot; ++i) o += (h->numels[i] + 63) & ~(int64_t)63;
  return o;
}

int64_t vftrain_flat_numel(vftrain_handle h) { return h ? vftrain_flat_offset(h, (int)h->numels.size()) : -1; }

size_t vftrain_workspace_bytes(vftrain_handle h, int B, int W, int Tv) {
  if (!h) return 0;
  VftPlan p;
  if (vft_make_plan(h, B, W, Tv, p)) return 0;
  return p.total;
}

int64_t vftrain_tape_offset(vftrain_handle h, int B, int W, int Tv, int which, int index) {
  if (!h) return -1;
  VftPlan p;
  if (vft_make_plan(h, B, W, Tv, p)) return -1;
  switch (which) {
    case VFTRAIN_TAPE_Z: if (index >= 0 && index < VF_LAYERS) return (int64_t)p.off_Z[index];  break;
    case VFTRAIN_TAPE_ACT: if (index >= 0 && index < 7) return (int64_t)p.off_A[index];  break;
    case VFTRAIN_TAPE_LSTM_H: return (int64_t)p.off_H;
    case VFTRAIN_TAPE_FC1: return (int64_t)p.off_y1fc;
    case VFTRAIN_TAPE_DROP: return (int64_t)p.off_keep;
    case VFTRAIN_TAPE_GATES: return (int64_t)p.off_gates;
    case VFTRAIN_TAPE_STATS: return (int64_t)p.off_block;
    case VFTRAIN_TAPE_CELL: return (int64_t)p.off_cell;
    default: h->fail(VFTRAIN_ERR_INVALID, "unknown tape tensor %d", which);  return -1;
  }
  h->fail(VFTRAIN_ERR_INVALID, "tape tensor %d: index %d out of range", which, index);
  return -1;
}

int vftrain_train_forward(vftrain_handle h, const float* mix, const float* emb1, const float* emb2, int B, int W, int Tv,
                          int dropout_ppm, uint32_t dropout_seed, float* out1, float* out2, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return VFTRAIN_ERR_INVALID;
  vftrain_ctx* c = h;
  VftPlan p;
  if (int rc = vft_prologue(c, false, mix, emb1, emb2, out1, out2, B, W, Tv, ws, ws_bytes, p)) return rc;
  if (dropout_ppm < 0 || dropout_ppm >= 1000000)
    return c->fail(VFTRAIN_ERR_INVALID, "dropout_ppm must be in [0, 999999] (got %d)", dropout_ppm);
  c->tape_ws = nullptr;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  const auto& Wt = c->w;
  const int F = c->F, E = c->E, nseq = p.nseq;
  const long long pos = p.pos;
  float* fold = at(p.off_fold);
  float* pack = at(p.off_pack);
  float* parts = at(p.off_parts);
  float* stat = at(p.off_stat);
  float* block = at(p.off_block);

  VftBiasSrc bs;
  for (int l = 0; l < VF_LAYERS; ++l) { bs.cb[l] = Wt[c->conv[l] + 1];  bs.C[l] = l == 7 ? VF_C8 : VF_C; }
  hipLaunchKernelGGL(vftrain_bias_fold_kernel, dim3(VF_LAYERS + 1), dim3(64), 0, st, bs, fold);
  HANDLE_LAUNCH_CHECK(c, "vftrain fold");
  LfPackSrc ps;
  for (int i = 0; i < 6; ++i) {
    ps.w[i] = Wt[c->conv[i + 1]];  ps.cin[i] = VF_C;  ps.cout[i] = VF_C;  ps.taps[i] = VFT_KH[i] * VFT_KW[i];
    ps.off[i] = c->pack_off[i];
  }
  hipLaunchKernelGGL(lipfe_pack_kernel, dim3(100, 6), dim3(256), 0, st, ps, pack);
  HANDLE_LAUNCH_CHECK(c, "vftrain pack");

  // CNN
  hipLaunchKernelGGL(vftrain_conv1_kernel, dim3(vft_blocks(pos * 64)), dim3(256), 0, st, mix, Wt[c->conv[0]], Wt[c->conv[0] + 1],
                     at(p.off_Z[0]), pos * 64, W);
  HANDLE_LAUNCH_CHECK(c, "vftrain conv1");
  for (int l = 0; l < 7; ++l) {
    if (l > 0) {
      const int i = l - 1;
      LfConvArgs a;
      a.in = at(p.off_A[l - 1]);  a.wpk = pack + c->pack_off[i];  a.scale = fold + 128 * l;  a.slope = nullptr;  a.res = nullptr;
      a.out = at(p.off_Z[l]);
      a.M = pos;
      a.Hi = F;  a.Wi = W;  a.Ho = F;  a.Wo = W;  a.Cin = VF_C;  a.Cout = VF_C;  a.stride = 1;  a.act = LF_ACT_NONE;
      a.dil = VFT_DIL[i];
      const dim3 grid((unsigned)((pos + LF_BM - 1) / LF_BM), 1);
      if (i == 0) hipLaunchKernelGGL((lipfe_conv_kernel<7, 1>), grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL((lipfe_conv_kernel<5, 5>), grid, dim3(256), 0, st, a);
      HANDLE_LAUNCH_CHECK(c, "vftrain conv");
    }
    if (int rc = vft_stats<64>(c, st, at(p.off_Z[l]), pos, parts, stat + l * VFT_STAT, block + l * 128)) return rc;
    hipLaunchKernelGGL(vftrain_norm_kernel<64>, dim3(vft_blocks(pos * 16)), dim3(256), 0, st, at(p.off_Z[l]), stat + l * VFT_STAT,
                       Wt[c->bn[l]], Wt[c->bn[l] + 1], at(p.off_A[l]), pos * 16, 1);
    HANDLE_LAUNCH_CHECK(c, "vftrain normalise");
  }
  hipLaunchKernelGGL(vfilt_conv8_kernel, dim3(vft_blocks(pos * 8)), dim3(256), 0, st, at(p.off_A[6]), Wt[c->conv[7]], fold + 128 * 7,
                     at(p.off_Z[7]), pos * 8, F, W);
  HANDLE_LAUNCH_CHECK(c, "vftrain conv8");
  if (int rc = vft_stats<8>(c, st, at(p.off_Z[7]), pos, parts, stat + 7 * VFT_STAT, block + 7 * 128)) return rc;
  float* flat = at(p.off_flat);
  hipLaunchKernelGGL(vftrain_norm_kernel<8>, dim3(vft_blocks(pos * 2)), dim3(256), 0, st, at(p.off_Z[7]), stat + 7 * VFT_STAT,
                     Wt[c->bn[7]], Wt[c->bn[7] + 1], flat, pos * 2, 0);
  HANDLE_LAUNCH_CHECK(c, "vftrain normalise 8");

  // d-vector
  const long long vrows = (long long)nseq * Tv;
  float* cat = at(p.off_cat);
  float* gi0 = at(p.off_gi0);
  float* y0 = at(p.off_y0);
  float* gi1 = at(p.off_gi1);
  float* y1 = at(p.off_y1);
  float* gi1b = at(p.off_gi1b);
  float* whht = at(p.off_whht);
  float* dvec = at(p.off_dvec);
  hipLaunchKernelGGL(vftrain_cat_kernel, dim3(vft_blocks(vrows * E)), dim3(256), 0, st, emb1, emb2, cat, (long long)B * Tv * E);
  HANDLE_LAUNCH_CHECK(c, "vftrain cat");
  for (int d = 0; d < 2; ++d) {
    const int g = c->gru[0][d];
    VfGemmArgs a = vft_gemm_args(cat, E, 1, Wt[g], E, 1, Wt[g + 2], gi0 + (long long)d * vrows * 3 * F, 3 * F, 1, (int)vrows, 3 * F, E);
    if (int rc = vft_launch_gemm(c, st, a, 1, "vftrain gru input 1")) return rc;
  }
  VfTransposeSrc ts;
  ts.w[0] = Wt[c->gru[0][0] + 1];  ts.w[1] = Wt[c->gru[0][1] + 1];  ts.w[2] = Wt[c->gru[1][0] + 1];
  hipLaunchKernelGGL(vfilt_transpose_kernel, dim3((3 * F * F + 255) / 256, 3), dim3(256), 0, st, ts, whht, F);
  HANDLE_LAUNCH_CHECK(c, "vftrain gru transpose");
  VftGruArgs ga;
  for (int d = 0; d < 2; ++d) {
    ga.g.gi[d] = gi0 + (long long)d * vrows * 3 * F;  ga.g.whht[d] = whht + (long long)d * 3 * F * F;  ga.g.bhh[d] = Wt[c->gru[0][d] + 3];
    ga.tape[d] = at(p.off_tape0) + (long long)d * vrows * 4 * F;
  }
  ga.g.y = y0;  ga.g.ldy = 2 * F;  ga.g.Tv = Tv;  ga.g.F = F;
  hipLaunchKernelGGL(vftrain_gru_kernel, dim3(nseq, 2), dim3(1024), 0, st, ga);
  HANDLE_LAUNCH_CHECK(c, "vftrain gru 1");
  {
    const int g = c->gru[1][0];
    VfGemmArgs a = vft_gemm_args(y0, 2 * F, 1, Wt[g], 2 * F, 1, Wt[g + 2], gi1, 3 * F, 1, (int)vrows, 3 * F, 2 * F);
    if (int rc = vft_launch_gemm(c, st, a, 1, "vftrain gru input 2")) return rc;
    ga.g.gi[0] = ga.g.gi[1] = gi1;  ga.g.whht[0] = ga.g.whht[1] = whht + (long long)2 * 3 * F * F;  ga.g.bhh[0] = ga.g.bhh[1] = Wt[g + 3];
    ga.tape[0] = ga.tape[1] = at(p.off_tape1);
    ga.g.y = y1;
    hipLaunchKernelGGL(vftrain_gru_kernel, dim3(nseq, 1), dim3(1024), 0, st, ga);
    HANDLE_LAUNCH_CHECK(c, "vftrain gru 2");
    const int gb = c->gru[1][1];
    const long long last = (long long)(Tv - 1) * 2 * F;
    a = vft_gemm_args(y0 + last, (long long)Tv * 2 * F, 1, Wt[gb], 2 * F, 1, Wt[gb + 2], gi1b, 3 * F, 1, nseq, 3 * F, 2 * F);
    if (int rc = vft_launch_gemm(c, st, a, 1, "vftrain gru input 2 reverse")) return rc;
    hipLaunchKernelGGL(vftrain_gru_first_step_kernel, dim3(nseq), dim3(320), 0, st, gi1b, Wt[gb + 3], y1 + last + F,
                       (long long)Tv * 2 * F, at(p.off_tape1b), F);
    HANDLE_LAUNCH_CHECK(c, "vftrain gru 2 reverse");
    a = vft_gemm_args(y1 + last, (long long)Tv * 2 * F, 1, Wt[c->fcd], 2 * F, 1, Wt[c->fcd + 1], dvec, F, 1, nseq, F, 2 * F);
    if (int rc = vft_launch_gemm(c, st, a, 1, "vftrain fc_dvector")) return rc;
  }

  // LSTM
  float* D = at(p.off_D);
  float* G = at(p.off_G);
  float* Hb = at(p.off_H);
  {
    const float* wih = Wt[c->lstm];
    VfGemmArgs a = vft_gemm_args(dvec, F, 1, wih + 8 * F, 9 * F, 1, Wt[c->lstm + 2], D, VF_G, 1, nseq, VF_G, F);
    a.bias2 = Wt[c->lstm + 3];
    if (int rc = vft_launch_gemm(c, st, a, 1, "vftrain lstm d-vector")) return rc;
    a = vft_gemm_args(flat, 1, W, wih, 9 * F, 1, nullptr, G, VF_G, 1, W, VF_G, 8 * F);
    a.sab = (long long)8 * F * W;  a.scb = (long long)W * VF_G;
    if (int rc = vft_launch_gemm(c, st, a, B, "vftrain lstm projection")) return rc;
  }
  VftLstmArgs la;
  la.l.G = G;  la.l.D = D;  la.l.whh = Wt[c->lstm + 1];  la.l.Hb = Hb;  la.l.cst = nullptr;  la.l.B = B;  la.l.W = W;  la.l.nseq = nseq;
  la.gates = at(p.off_gates);  la.cell = at(p.off_cell);  la.hprev = at(p.off_hprev);
  for (int t = 0; t < W; ++t) {
    la.l.t = t;
    if (nseq == 2) hipLaunchKernelGGL(vftrain_lstm_step_kernel<2>, dim3(VF_H / 4, 1), dim3(256), 0, st, la);
    else hipLaunchKernelGGL(vftrain_lstm_step_kernel<8>, dim3(VF_H / 4, (nseq + 7) / 8), dim3(256), 0, st, la);
    HANDLE_LAUNCH_CHECK(c, "vftrain lstm step");
  }

  // FC tail
  const long long rows = (long long)nseq * W;
  const double pdrop = dropout_ppm * 1e-6;
  const uint32_t thresh = (uint32_t)(pdrop * 16777216.0);
  const float inv_keep = (float)(1.0 / (1.0 - pdrop));
  {
    float* y1fc = at(p.off_y1fc);
    float* keep = at(p.off_keep);
    float* yd = at(p.off_yd);
    float* S = at(p.off_S);
    VfGemmArgs a = vft_gemm_args(Hb, VF_H, 1, Wt[c->fc1], VF_H, 1, Wt[c->fc1 + 1], y1fc, VF_FC, 1, (int)rows, VF_FC, VF_H);
    a.relu_a = 1;  a.act = VF_ACT_RELU;
    if (int rc = vft_launch_gemm(c, st, a, 1, "vftrain fc 1")) return rc;
    hipLaunchKernelGGL(vftrain_drop_mask_kernel, dim3(vft_blocks(rows)), dim3(256), 0, st, keep, (int)rows, dropout_seed, thresh);
    hipLaunchKernelGGL(vftrain_drop_apply_kernel, dim3(vft_blocks(rows * VF_FC)), dim3(256), 0, st, y1fc, keep, inv_keep, yd,
                       rows * VF_FC, VF_FC);
    HANDLE_LAUNCH_CHECK(c, "vftrain dropout");
    a = vft_gemm_args(yd, VF_FC, 1, Wt[c->fc2], VF_FC, 1, Wt[c->fc2 + 1], S, F, 1, (int)rows, F, VF_FC);
    a.act = VF_ACT_SIGMOID;
    if (int rc = vft_launch_gemm(c, st, a, 1, "vftrain fc 2")) return rc;
    hipLaunchKernelGGL(vftrain_out_kernel, dim3(vft_blocks(2 * pos)), dim3(256), 0, st, S, mix, out1, out2, pos, F, W);
    HANDLE_LAUNCH_CHECK(c, "vftrain output");
  }
  c->tape_ws = ws;  c->tape_B = B;  c->tape_W = W;  c->tape_Tv = Tv;  c->tape_inv_keep = inv_keep;
  return VFTRAIN_OK;
}

int vftrain_train_backward(vftrain_handle h, const float* mix, const float* emb1, const float* emb2, int B, int W, int Tv,
                           const float* d_out1, const float* d_out2, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return VFTRAIN_ERR_INVALID;
  vftrain_ctx* c = h;
  VftPlan p;
  if (int rc = vft_prologue(c, true, mix, emb1, emb2, d_out1, d_out2, B, W, Tv, ws, ws_bytes, p)) return rc;
  if (c->tape_ws != ws || c->tape_B != B || c->tape_W != W || c->tape_Tv != Tv)
    return c->fail(VFTRAIN_ERR_INVALID, "train_backward: no tape of vftrain_train_forward(B=%d, W=%d, Tv=%d) on this workspace", B, W, Tv);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  const auto& Wt = c->w;
  const auto& Gr = c->g;
  const int F = c->F, E = c->E, nseq = p.nseq;
  const long long pos = p.pos, rows = (long long)nseq * W, vrows = (long long)nseq * Tv;
  float* parts = at(p.off_parts);
  float* stat = at(p.off_stat);
  float* coef = at(p.off_coef);
  const float inv_keep = c->tape_inv_keep;

  // ---- FC tail
  float* dP = at(p.off_dP);
  float* dY = at(p.off_dY);
  float* dH = at(p.off_dH);
  float* Hb = at(p.off_H);
  hipLaunchKernelGGL(vftrain_dsig_kernel, dim3(vft_blocks(2 * pos)), dim3(256), 0, st, d_out1, d_out2, mix, at(p.off_S), dP, pos, F, W);
  HANDLE_LAUNCH_CHECK(c, "vftrain sigmoid backward");
  if (int rc = vft_gemm_tn(c, st, dP, F, at(p.off_yd), VF_FC, VF_FC, (int)rows, Gr[c->fc2], VF_FC, "vftrain fc 2 wgrad")) return rc;
  if (int rc = vft_colsum(c, st, dP, (int)rows, F, 1, Gr[c->fc2 + 1], nullptr)) return rc;
  if (int rc = vft_gemm_nn(c, st, dP, (int)rows, F, Wt[c->fc2], VF_FC, VF_FC, dY, "vftrain fc 2 dgrad")) return rc;
  hipLaunchKernelGGL(vftrain_drelu_drop_kernel, dim3(vft_blocks(rows * VF_FC)), dim3(256), 0, st, dY, at(p.off_y1fc), at(p.off_keep),
                     inv_keep, rows * VF_FC, VF_FC);
  HANDLE_LAUNCH_CHECK(c, "vftrain dropout backward");
  {
    // d fc.1.weight [600][400] = dY^T relu(H): computed transposed, so that the ReLU rides on the GEMM's A loader
    VfGemmArgs a = vft_gemm_args(Hb, 1, VF_H, dY, 1, VF_FC, nullptr, Gr[c->fc1], 1, VF_H, VF_H, VF_FC, (int)rows);
    a.relu_a = 1;
    if (int rc = vft_launch_gemm(c, st, a, 1, "vftrain fc 1 wgrad")) return rc;
  }
  if (int rc = vft_colsum(c, st, dY, (int)rows, VF_FC, 1, Gr[c->fc1 + 1], nullptr)) return rc;
  if (int rc = vft_gemm_nn(c, st, dY, (int)rows, VF_FC, Wt[c->fc1], VF_H, VF_H, dH, "vftrain fc 1 dgrad")) return rc;

  // ---- LSTM
  float* dgates = at(p.off_dgates);
  float* lwhht = at(p.off_lwhht);
  hipLaunchKernelGGL(vftrain_transpose_kernel, dim3(vft_blocks((long long)VF_G * VF_H)), dim3(256), 0, st, Wt[c->lstm + 1], lwhht, VF_G, VF_H);
  HANDLE_LAUNCH_CHECK(c, "vftrain lstm transpose");
  VftLstmBwdArgs lb;
  lb.dH = dH;  lb.Hb = Hb;  lb.gates = at(p.off_gates);  lb.cell = at(p.off_cell);  lb.whht = lwhht;  lb.dgates = dgates;
  lb.dcst = at(p.off_dcst);  lb.W = W;  lb.nseq = nseq;
  for (int t = W - 1; t >= 0; --t) {
    lb.t = t;
    if (nseq == 2) hipLaunchKernelGGL(vftrain_lstm_bwd_step_kernel<2>, dim3(VF_H / 4, 1), dim3(256), 0, st, lb);
    else hipLaunchKernelGGL(vftrain_lstm_bwd_step_kernel<8>, dim3(VF_H / 4, (nseq + 7) / 8), dim3(256), 0, st, lb);
    HANDLE_LAUNCH_CHECK(c, "vftrain lstm backward step");
  }
  float* dGsum = at(p.off_dGsum);
  float* dGt = at(p.off_dGt);
  float* viewT = at(p.off_viewT);
  float* dflat = at(p.off_dflat);
  float* ddvec = at(p.off_ddvec);
  const float* wih = Wt[c->lstm];
  float* dwih = Gr[c->lstm];
  if (int rc = vft_gemm_tn(c, st, dgates, VF_G, at(p.off_hprev), VF_H, VF_H, (int)rows, Gr[c->lstm + 1], VF_H, "vftrain lstm W_hh wgrad")) return rc;
  hipLaunchKernelGGL(vftrain_add_kernel, dim3(vft_blocks((long long)B * W * VF_G)), dim3(256), 0, st, dgates, dgates + (long long)B * W * VF_G,
                     dGsum, (long long)B * W * VF_G);
  hipLaunchKernelGGL(vftrain_view_t_kernel, dim3((W + 31) / 32, (8 * F + 31) / 32, B), dim3(256), 0, st, at(p.off_flat), viewT, 8 * F, W);
  HANDLE_LAUNCH_CHECK(c, "vftrain view transpose");
  if (int rc = vft_gemm_tn(c, st, dGsum, VF_G, viewT, 8 * F, 8 * F, B * W, dwih, 9 * F, "vftrain lstm W_ih wgrad (map)")) return rc;
  if (int rc = vft_colsum(c, st, dgates, W, VF_G, nseq, dGt, nullptr)) return rc;
  if (int rc = vft_gemm_tn(c, st, dGt, VF_G, at(p.off_dvec), F, F, nseq, dwih + 8 * F, 9 * F, "vftrain lstm W_ih wgrad (d-vector)")) return rc;
  if (int rc = vft_colsum(c, st, dGt, nseq, VF_G, 1, Gr[c->lstm + 2], Gr[c->lstm + 3])) return rc;
  {
    // d view, in the map's own memory order: dflat[b][c W + t] = sum_j dGsum[b][t][j] W_ih[j][c]
    VfGemmArgs a = vft_gemm_args(dGsum, VF_G, 1, wih, 1, 9 * F, nullptr, dflat, 1, W, W, 8 * F, VF_G);
    a.sab = (long long)W * VF_G;  a.scb = (long long)8 * F * W;
    if (int rc = vft_launch_gemm(c, st, a, B, "vftrain d view")) return rc;
  }
  if (int rc = vft_gemm_nn(c, st, dGt, nseq, VF_G, wih + 8 * F, 9 * F, F, ddvec, "vftrain d dvector")) return rc;

  // ---- d-vector: fc_dvector, GRU layer 2 (forward in full, reverse at its first step), GRU layer 1
  {
    float* y0 = at(p.off_y0);
    float* y1 = at(p.off_y1);
    float* dglast = at(p.off_dglast);
    float* dy0 = at(p.off_dy0);
    const long long last = (long long)(Tv - 1) * 2 * F;
    if (int rc = vft_gemm_tn(c, st, ddvec, F, y1 + last, (long long)Tv * 2 * F, 2 * F, nseq, Gr[c->fcd], 2 * F, "vftrain fc_dvector wgrad")) return rc;
    if (int rc = vft_colsum(c, st, ddvec, nseq, F, 1, Gr[c->fcd + 1], nullptr)) return rc;
    if (int rc = vft_gemm_nn(c, st, ddvec, nseq, F, Wt[c->fcd], 2 * F, 2 * F, dglast, "vftrain fc_dvector dgrad")) return rc;

    VftGruBwdArgs gb;
    const int g10 = c->gru[1][0], g11 = c->gru[1][1];
    float* dgi1 = at(p.off_dgi1);
    float* dgh1 = at(p.off_dgh1);
    float* hp1 = at(p.off_hp1);
    gb.tape[0] = gb.tape[1] = at(p.off_tape1);
    gb.y = y1;  gb.dy = dglast;  gb.dy_sq = 2 * F;  gb.dy_st = 0;  gb.only_t = Tv - 1;
    gb.whh[0] = gb.whh[1] = Wt[g10 + 1];
    gb.dgi[0] = gb.dgi[1] = dgi1;  gb.dgh[0] = gb.dgh[1] = dgh1;  gb.hprev[0] = gb.hprev[1] = hp1;
    gb.ldy = 2 * F;  gb.Tv = Tv;  gb.F = F;
    hipLaunchKernelGGL(vftrain_gru_bwd_kernel, dim3(nseq, 1), dim3(1024), 0, st, gb);
    HANDLE_LAUNCH_CHECK(c, "vftrain gru 2 backward");
    if (int rc = vft_gemm_tn(c, st, dgi1, 3 * F, y0, 2 * F, 2 * F, (int)vrows, Gr[g10], 2 * F, "vftrain gru 2 W_ih wgrad")) return rc;
    if (int rc = vft_gemm_tn(c, st, dgh1, 3 * F, hp1, F, F, (int)vrows, Gr[g10 + 1], F, "vftrain gru 2 W_hh wgrad")) return rc;
    if (int rc = vft_colsum(c, st, dgi1, (int)vrows, 3 * F, 1, Gr[g10 + 2], nullptr)) return rc;
    if (int rc = vft_colsum(c, st, dgh1, (int)vrows, 3 * F, 1, Gr[g10 + 3], nullptr)) return rc;
    if (int rc = vft_gemm_nn(c, st, dgi1, (int)vrows, 3 * F, Wt[g10], 2 * F, 2 * F, dy0, "vftrain gru 2 dgrad")) return rc;

    // reverse direction of layer 2: one step from h = 0, so W_hh sees zeros: its gradient is exactly zero
    float* dgi1b = at(p.off_dgi1b);
    float* dgh1b = at(p.off_dgh1b);
    float* tmp = at(p.off_tmp2f);
    hipLaunchKernelGGL(vftrain_gru_first_step_bwd_kernel, dim3(nseq), dim3(320), 0, st, at(p.off_tape1b), dglast + F, (long long)2 * F,
                       dgi1b, dgh1b, F);
    HANDLE_LAUNCH_CHECK(c, "vftrain gru 2 reverse backward");
    if (int rc = vft_gemm_tn(c, st, dgi1b, 3 * F, y0 + last, (long long)Tv * 2 * F, 2 * F, nseq, Gr[g11], 2 * F, "vftrain gru 2 reverse W_ih wgrad")) return rc;
    if (hipMemsetAsync(Gr[g11 + 1], 0, (size_t)3 * F * F * 4, st) != hipSuccess)
      return c->fail(VFTRAIN_ERR_HIP, "vftrain gru 2 reverse W_hh: memset failed");
    if (int rc = vft_colsum(c, st, dgi1b, nseq, 3 * F, 1, Gr[g11 + 2], nullptr)) return rc;
    if (int rc = vft_colsum(c, st, dgh1b, nseq, 3 * F, 1, Gr[g11 + 3], nullptr)) return rc;
    if (int rc = vft_gemm_nn(c, st, dgi1b, nseq, 3 * F, Wt[g11], 2 * F, 2 * F, tmp, "vftrain gru 2 reverse dgrad")) return rc;
    hipLaunchKernelGGL(vftrain_add_rows_kernel, dim3(vft_blocks((long long)nseq * 2 * F)), dim3(256), 0, st, dy0 + last, (long long)Tv * 2 * F,
                       tmp, nseq, 2 * F);
    HANDLE_LAUNCH_CHECK(c, "vftrain gru 2 reverse add");

    // layer 1, both directions
    float* cat = at(p.off_cat);
    for (int d = 0; d < 2; ++d) {
      gb.tape[d] = at(p.off_tape0) + (long long)d * vrows * 4 * F;
      gb.whh[d] = Wt[c->gru[0][d] + 1];
      gb.dgi[d] = at(p.off_dgi0) + (long long)d * vrows * 3 * F;
      gb.dgh[d] = at(p.off_dgh0) + (long long)d * vrows * 3 * F;
      gb.hprev[d] = at(p.off_hp0) + (long long)d * vrows * F;
    }
    gb.y = y0;  gb.dy = dy0;  gb.dy_sq = (long long)Tv * 2 * F;  gb.dy_st = 2 * F;  gb.only_t = -1;
    hipLaunchKernelGGL(vftrain_gru_bwd_kernel, dim3(nseq, 2), dim3(1024), 0, st, gb);
    HANDLE_LAUNCH_CHECK(c, "vftrain gru 1 backward");
    for (int d = 0; d < 2; ++d) {
      const int g = c->gru[0][d];
      if (int rc = vft_gemm_tn(c, st, gb.dgi[d], 3 * F, cat, E, E, (int)vrows, Gr[g], E, "vftrain gru 1 W_ih wgrad")) return rc;
      if (int rc = vft_gemm_tn(c, st, gb.dgh[d], 3 * F, gb.hprev[d], F, F, (int)vrows, Gr[g + 1], F, "vftrain gru 1 W_hh wgrad")) return rc;
      if (int rc = vft_colsum(c, st, gb.dgi[d], (int)vrows, 3 * F, 1, Gr[g + 2], nullptr)) return rc;
      if (int rc = vft_colsum(c, st, gb.dgh[d], (int)vrows, 3 * F, 1, Gr[g + 3], nullptr)) return rc;
    }
  }

  // ---- CNN
  float* dA = at(p.off_dA);
  float* dZ = at(p.off_dZ);
  float* dZ8 = at(p.off_dZ8);
  float* packT = at(p.off_packT);
  float* fold = at(p.off_fold);
  LfPackSrc ps;
  for (int i = 0; i < 6; ++i) {
    ps.w[i] = Wt[c->conv[i + 1]];  ps.cin[i] = VF_C;  ps.cout[i] = VF_C;  ps.taps[i] = VFT_KH[i] * VFT_KW[i];
    ps.off[i] = c->pack_off[i];
  }
  hipLaunchKernelGGL(vftrain_pack_flip_kernel, dim3(100, 6), dim3(256), 0, st, ps, packT);
  HANDLE_LAUNCH_CHECK(c, "vftrain pack flip");
  // layer 8
  if (int rc = vft_bn_bwd<8>(c, st, dflat, nullptr, at(p.off_Z[7]), stat + 7 * VFT_STAT, pos, Wt[c->bn[7]], parts, coef, dZ8,
                             Gr[c->bn[7]], Gr[c->bn[7] + 1], Gr[c->conv[7] + 1]))
    return rc;
  hipLaunchKernelGGL(vftrain_conv8_wgrad_kernel, dim3(p.nchunk), dim3(256), 0, st, dZ8, at(p.off_A[6]), parts, pos, F, W);
  hipLaunchKernelGGL(vftrain_parts_sum_kernel, dim3(2), dim3(256), 0, st, parts, p.nchunk, 8, Gr[c->conv[7]], 1, 64);
  hipLaunchKernelGGL(vftrain_conv8_dgrad_kernel, dim3(vft_blocks(pos * 16)), dim3(256), 0, st, dZ8, Wt[c->conv[7]], dA, pos * 16, F, W);
  HANDLE_LAUNCH_CHECK(c, "vftrain conv8 backward");
  // layers 7..2
  for (int l = 6; l >= 1; --l) {
    const int i = l - 1, taps = VFT_KH[i] * VFT_KW[i];
    if (int rc = vft_bn_bwd<64>(c, st, dA, at(p.off_A[l]), at(p.off_Z[l]), stat + l * VFT_STAT, pos, Wt[c->bn[l]], parts, coef, dZ,
                                Gr[c->bn[l]], Gr[c->bn[l] + 1], Gr[c->conv[l] + 1]))
      return rc;
    VftWgradArgs wa;
    wa.X = at(p.off_A[l - 1]);  wa.dZ = dZ;  wa.parts = parts;  wa.npos = pos;  wa.F = F;  wa.W = W;
    wa.KH = VFT_KH[i];  wa.KW = VFT_KW[i];  wa.dil = VFT_DIL[i];
    hipLaunchKernelGGL(vftrain_wgrad_kernel, dim3(p.nwchunk, taps), dim3(256), 0, st, wa);
    hipLaunchKernelGGL(vftrain_wgrad_sum_kernel, dim3(vft_blocks((long long)taps * 4096)), dim3(256), 0, st, parts, p.nwchunk, taps,
                       Gr[c->conv[l]]);
    HANDLE_LAUNCH_CHECK(c, "vftrain conv wgrad");
    LfConvArgs a;
    a.in = dZ;  a.wpk = packT + c->pack_off[i];  a.scale = fold + 128 * VF_LAYERS;  a.slope = nullptr;  a.res = nullptr;
    a.out = dA;
    a.M = pos;
    a.Hi = F;  a.Wi = W;  a.Ho = F;  a.Wo = W;  a.Cin = VF_C;  a.Cout = VF_C;  a.stride = 1;  a.act = LF_ACT_NONE;
    a.dil = VFT_DIL[i];
    const dim3 grid((unsigned)((pos + LF_BM - 1) / LF_BM), 1);
    if (i == 0) hipLaunchKernelGGL((lipfe_conv_kernel<7, 1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((lipfe_conv_kernel<5, 5>), grid, dim3(256), 0, st, a);
    HANDLE_LAUNCH_CHECK(c, "vftrain conv dgrad");
  }
  // layer 1
  if (int rc = vft_bn_bwd<64>(c, st, dA, at(p.off_A[0]), at(p.off_Z[0]), stat, pos, Wt[c->bn[0]], parts, coef, dZ, Gr[c->bn[0]],
                              Gr[c->bn[0] + 1], Gr[c->conv[0] + 1]))
    return rc;
  hipLaunchKernelGGL(vftrain_conv1_wgrad_kernel, dim3(p.nchunk), dim3(256), 0, st, dZ, mix, parts, pos, W);
  hipLaunchKernelGGL(vftrain_parts_sum_kernel, dim3(2), dim3(256), 0, st, parts, p.nchunk, 7, Gr[c->conv[0]], 7, 1);
  HANDLE_LAUNCH_CHECK(c, "vftrain conv1 wgrad");
  return VFTRAIN_OK;
}

size_t vftrain_clip_scratch_bytes(vftrain_handle) { return CLIP_PARTS * sizeof(double); }

int vftrain_grad_clip(vftrain_handle h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                      float* norm_out, void* stream) {
  if (!h) return VFTRAIN_ERR_INVALID;
  if (!flat_grad || !norm_out || n_flat < 4 || (n_flat & 3) || ((uintptr_t)flat_grad & 15))
    return h->fail(VFTRAIN_ERR_INVALID, "grad_clip: flat gradient must be 16-byte aligned with a multiple of 4 floats");
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < CLIP_PARTS * sizeof(double))
    return h->fail(VFTRAIN_ERR_WORKSPACE, "grad_clip: scratch too small / misaligned");
  // the second launch's grid only spreads an elementwise scale: no sum depends on it
  launch_grad_clip((hipStream_t)stream, 256, flat_grad, n_flat, max_norm, (double*)scratch, norm_out);
  HANDLE_LAUNCH_CHECK(h, "vftrain grad_clip");
  return VFTRAIN_OK;
}

int vftrain_adamw_step(vftrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                       double beta1, double beta2, double eps, double weight_decay, int step, void* stream) {
  if (!h) return VFTRAIN_ERR_INVALID;
  if (!h->bound) return h->fail(VFTRAIN_ERR_WEIGHTS, "adamw_step: weights not bound (the step updates the bound parameters in place)");
  if (!flat_grad || !exp_avg || !exp_avg_sq || n_flat != vftrain_flat_numel(h) || step < 1)
    return h->fail(VFTRAIN_ERR_INVALID, "adamw_step: bad argument (flat buffers must hold %lld floats, step >= 1)",
                   (long long)vftrain_flat_numel(h));
  // launch_adamw skips one slot; here sixteen (the running statistics) keep their place in the flat layout and take no
  // step, so the trainable runs between them go out one by one, each at its own offset
  const int n = (int)h->names.size();
  int i = 0;
  while (i < n) {
    if (h->no_grad[i]) { ++i;  continue; }
    int j = i;
    while (j < n && !h->no_grad[j]) ++j;
    const int64_t off = vftrain_flat_offset(h, i);
    launch_adamw((hipStream_t)stream, h->w.data() + i, h->numels.data() + i, j - i, -1, 64, flat_grad + off, exp_avg + off,
                 exp_avg_sq + off, lr, beta1, beta2, eps, weight_decay, step);
    i = j;
  }
  HANDLE_LAUNCH_CHECK(h, "vftrain adamw_step");
  return VFTRAIN_OK;
}

double vftrain_flops_per_item(vftrain_handle h, int W, int Tv) {
  if (!h || vft_check_shape(h->F, 1, W, Tv)) return 0.0;
  return 3.0 * 2.0 * vft_macs(h->F, h->E, W, Tv);
}

}  // extern "C"
