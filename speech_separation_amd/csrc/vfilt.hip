// vfilt.hip -- the VoiceFilter separator (src/model/voicefilter.py:108-145 in eval mode: lip embeddings -> d-vector, the
// mixture's magnitude -> dilated CNN -> LSTM -> FC -> sigmoid mask) for gfx950: handle and the extern "C" boundary declared
// in include/vfilt.h; the kernels are in vfilt_kernels.h and lipfe_kernels.h, the handle's scaffolding in handle.h.
//
// One forward, all on the caller's stream (F = input_size, q = speaker * B + item: the 2B sequences run together):
//   fold, pack   the 8 eval-mode BatchNorms with the conv biases -> scale / shift; the six 64 -> 64 conv weights -> K-major
//   CNN          layer 1 (1 -> 64, 1 x 7) on VALU; layers 2..7 (7 x 1, then 5 x 5 with row dilation 1, 2, 4, 8, 16) on
//                lipfe_conv_kernel, channel-last [B][F][W][64], padding as an index guard; layer 8 (64 -> 8) on VALU writes
//                [B][W][F][8], the buffer the reference then VIEWS as [B][8F][W]
//   d-vector     W_hh of the three full recurrences transposed (a derived copy, as fold and pack); GRU layer 1 in both
//                directions, layer 2 forward, layer 2 backward for the one step that is read, fc_dvector
//   projection   G[item][t][:] = W_ih[:, :8F] x view[:, t], one GEMM per item that reads the view K-major in place;
//                D[q][:] = W_ih[:, 8F:] x dvector + b_ih + b_hh, once: the concatenation is never built
//   LSTM         one launch per time step, the 400 hidden units spread over 100 workgroups (see vfilt_lstm_step_kernel)
//   tail         ReLU, Linear(400, 600), ReLU, Linear(600, F), sigmoid, x mixture, written transposed as [B][F][W]
// The derived copies (fold, pack) are made in every forward, into the workspace: a copy made at bind time would go stale
// when load_state_dict copies into the same storages.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vfilt.h"
#include "vfilt_kernels.h"

HANDLE_ASSERT_CODES(VFILT);

namespace {
thread_local std::string g_vf_create_error;

// kernel rows / columns and row dilation of layers 2..7 (the 64 -> 64 convolutions)
const int VF_KH[6] = {7, 5, 5, 5, 5, 5};
const int VF_KW[6] = {1, 5, 5, 5, 5, 5};
const int VF_DIL[6] = {1, 1, 2, 4, 8, 16};
// index of each Conv2d / BatchNorm2d in the reference's nn.Sequential (ZeroPad2d and ReLU take the others)
const int VF_CONV_IDX[VF_LAYERS] = {1, 5, 9, 13, 17, 21, 25, 28};
const int VF_BN_IDX[VF_LAYERS] = {2, 6, 10, 14, 18, 22, 26, 29};

struct VfPlan {
  int nseq;
  size_t off_fold, off_pack, off_act[2], off_flat, off_G, off_gi0, off_y0, off_gi1, off_y1, off_gi1b, off_whht, off_dvec, off_D, off_H,
      off_c, off_fc, total;
};
}  // namespace

struct vfilt_ctx : Handle {
  int F = 0, E = 0;
  int gru[2][2];                 // [layer][direction]: weight_ih (weight_hh, bias_ih, bias_hh follow)
  int fcd;                       // fc_dvector.weight (bias follows)
  int conv[VF_LAYERS];           // conv weight (bias follows)
  int bn[VF_LAYERS];             // bn weight (bias, running_mean, running_var follow)
  int lstm;                      // weight_ih (weight_hh, bias_ih, bias_hh follow)
  int fc1, fc2;                  // weight (bias follows)
  int64_t pack_off[6], pack_floats = 0;
};

namespace {
// the reference's state_dict() order without num_batches_tracked
void vf_build_table(vfilt_ctx* c) {
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
    const int64_t per_out = l == 0 ? 7 : l == 7 ? VF_C : (int64_t)VF_C * VF_KH[l - 1] * VF_KW[l - 1];
    const std::string pc = "cnn_layers." + std::to_string(VF_CONV_IDX[l]) + ".";
    const std::string pb = "cnn_layers." + std::to_string(VF_BN_IDX[l]) + ".";
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
}

const char* vf_check_shape(int F, int B, int W, int Tv) {
  if (B < 1) return "B must be >= 1";
  if (W < 1) return "W must be >= 1";
  if (Tv < 1) return "Tv must be >= 1";
  if ((double)B * F * W * VF_C >= 2147483648.0) return "B * input_size * W * 64 must stay below 2^31";
  if (2.0 * B * (W > Tv ? W : Tv) * VF_G >= 2147483648.0) return "2 * B * max(W, Tv) * 1600 must stay below 2^31";
  return nullptr;
}

int vf_make_plan(vfilt_ctx* c, int B, int W, int Tv, VfPlan& p) {
  if (const char* why = vf_check_shape(c->F, B, W, Tv))
    return c->fail(VFILT_ERR_INVALID, "%s (got B=%d W=%d Tv=%d, input_size=%d)", why, B, W, Tv, c->F);
  const size_t F = c->F, nseq = 2 * (size_t)B;
  p.nseq = (int)nseq;
  ByteCursor cur;
  auto take = [&](size_t floats) { return cur.take(floats * 4); };
  p.off_fold = take(128 * VF_LAYERS);
  p.off_pack = take((size_t)c->pack_floats);
  p.off_act[0] = take((size_t)B * F * W * VF_C);
  p.off_act[1] = take((size_t)B * F * W * VF_C);
  p.off_flat = take((size_t)B * W * F * VF_C8);
  p.off_G = take((size_t)B * W * VF_G);
  p.off_gi0 = take(2 * nseq * Tv * 3 * F);
  p.off_y0 = take(nseq * Tv * 2 * F);
  p.off_gi1 = take(nseq * Tv * 3 * F);
  p.off_y1 = take(nseq * Tv * 2 * F);
  p.off_gi1b = take(nseq * 3 * F);
  p.off_whht = take(3 * 3 * F * F);
  p.off_dvec = take(nseq * F);
  p.off_D = take(nseq * VF_G);
  p.off_H = take(nseq * W * VF_H);
  p.off_c = take(nseq * VF_H);
  p.off_fc = take(nseq * W * VF_FC);
  p.total = cur.o;
  return VFILT_OK;
}

VfGemmArgs vf_gemm_args(const float* A, long long sam, long long sak, const float* Bw, long long sbn, long long sbk,
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

int vf_launch_gemm(vfilt_ctx* c, hipStream_t st, const VfGemmArgs& a, int batches, const char* what) {
  const dim3 grid((unsigned)((long long)a.mtiles * batches), (unsigned)((a.N + LF_BN - 1) / LF_BN));
  hipLaunchKernelGGL(vfilt_gemm_kernel, grid, dim3(256), 0, st, a);
  HANDLE_LAUNCH_CHECK(c, what);
  return VFILT_OK;
}

// multiply-accumulates of one item (both speakers)
double vf_macs(int F, int E, int W, int Tv) {
  const double f = F, pos = f * W;
  double conv = 64.0 * 7 + 64.0 * 64 * 7 + 5.0 * 64 * 64 * 25 + 64.0 * 8;
  double m = pos * conv;
  m += (double)W * 8 * f * VF_G;                                           // projection, shared by the speakers
  m += 2.0 * (f * VF_G + (double)W * VF_G * VF_H);                         // d-vector's part, recurrence
  m += 2.0 * W * ((double)VF_H * VF_FC + (double)VF_FC * f);               // FC tail
  m += 2.0 * (Tv * (2.0 * 3 * f * (E + f) + 3 * f * (2 * f + f)) + 3 * f * 2 * f + f * 2 * f);   // GRU + fc_dvector
  return m;
}
}  // namespace

extern "C" {

int vfilt_abi_version(void) { return VFILT_ABI_VERSION; }

int vfilt_create(vfilt_handle* out, int input_size, int embed_size) {
  if (out && (input_size < 1 || input_size > VF_FMAX))
    return refuse_create(out, g_vf_create_error, "input_size must be in [1, 257] (got " + std::to_string(input_size) + ")");
  if (out && embed_size != 512 && embed_size != 1024)
    return refuse_create(out, g_vf_create_error, "embed_size must be 512 or 1024 (got " + std::to_string(embed_size) + ")");
  if (int rc = create(out, "VoiceFilter", g_vf_create_error)) return rc;
  (*out)->F = input_size;
  (*out)->E = embed_size;
  vf_build_table(*out);
  return VFILT_OK;
}

void vfilt_destroy(vfilt_handle h) { delete h; }

const char* vfilt_last_error(vfilt_handle h) { return h ? h->err.c_str() : g_vf_create_error.c_str(); }

int vfilt_num_weights(vfilt_handle h) { return h ? (int)h->names.size() : 0; }

const char* vfilt_weight_name(vfilt_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t vfilt_weight_numel(vfilt_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int vfilt_bind_weights(vfilt_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n, 4) : VFILT_ERR_INVALID;
}

size_t vfilt_workspace_bytes(vfilt_handle h, int B, int W, int Tv) {
  if (!h) return 0;
  VfPlan p;
  if (vf_make_plan(h, B, W, Tv, p)) return 0;
  return p.total;
}

int vfilt_forward(vfilt_handle h, const float* mix, const float* emb1, const float* emb2, int B, int W, int Tv, float* out1,
                  float* out2, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return VFILT_ERR_INVALID;
  vfilt_ctx* c = h;
  if (!c->bound) return c->fail(VFILT_ERR_WEIGHTS, "weights not bound (vfilt_bind_weights)");
  if (!mix || !emb1 || !emb2 || !out1 || !out2)
    return c->fail(VFILT_ERR_INVALID, "mix_magnitude / emb1 / emb2 / out1 / out2 must not be NULL");
  VfPlan p;
  if (int rc = vf_make_plan(c, B, W, Tv, p)) return rc;
  if (int rc = check_workspace(c, p.total, ws, ws_bytes)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  float* fold = at(p.off_fold);
  float* pack = at(p.off_pack);
  float* act[2] = {at(p.off_act[0]), at(p.off_act[1])};
  float* flat = at(p.off_flat);
  float* G = at(p.off_G);
  float* gi0 = at(p.off_gi0);
  float* y0 = at(p.off_y0);
  float* gi1 = at(p.off_gi1);
  float* y1 = at(p.off_y1);
  float* gi1b = at(p.off_gi1b);
  float* whht = at(p.off_whht);
  float* dvec = at(p.off_dvec);
  float* D = at(p.off_D);
  float* Hb = at(p.off_H);
  float* cst = at(p.off_c);
  float* fcb = at(p.off_fc);
  const auto& Wt = c->w;
  const int F = c->F, E = c->E, nseq = p.nseq;
  const long long pos = (long long)B * F * W;

  // derived copies of this forward
  VfFoldSrc fs;
  for (int l = 0; l < VF_LAYERS; ++l) {
    fs.cb[l] = Wt[c->conv[l] + 1];
    fs.w[l] = Wt[c->bn[l]];  fs.b[l] = Wt[c->bn[l] + 1];  fs.m[l] = Wt[c->bn[l] + 2];  fs.v[l] = Wt[c->bn[l] + 3];
    fs.C[l] = l == 7 ? VF_C8 : VF_C;
  }
  hipLaunchKernelGGL(vfilt_fold_kernel, dim3(VF_LAYERS), dim3(64), 0, st, fs, fold);
  HANDLE_LAUNCH_CHECK(c, "vfilt fold");
  LfPackSrc ps;
  for (int i = 0; i < 6; ++i) {
    ps.w[i] = Wt[c->conv[i + 1]];  ps.cin[i] = VF_C;  ps.cout[i] = VF_C;  ps.taps[i] = VF_KH[i] * VF_KW[i];
    ps.off[i] = c->pack_off[i];
  }
  hipLaunchKernelGGL(lipfe_pack_kernel, dim3(100, 6), dim3(256), 0, st, ps, pack);
  HANDLE_LAUNCH_CHECK(c, "vfilt pack");

  // CNN
  hipLaunchKernelGGL(vfilt_conv1_kernel, dim3((unsigned)((pos * 64 + 255) / 256)), dim3(256), 0, st, mix, Wt[c->conv[0]], fold,
                     act[0], pos * 64, W);
  HANDLE_LAUNCH_CHECK(c, "vfilt conv1");
  int cur = 0;
  for (int i = 0; i < 6; ++i) {
    LfConvArgs a;
    a.in = act[cur];  a.wpk = pack + c->pack_off[i];  a.scale = fold + 128 * (i + 1);  a.slope = nullptr;  a.res = nullptr;
    a.out = act[cur ^ 1];
    a.M = pos;
    a.Hi = F;  a.Wi = W;  a.Ho = F;  a.Wo = W;  a.Cin = VF_C;  a.Cout = VF_C;  a.stride = 1;  a.act = LF_ACT_RELU;
    a.dil = VF_DIL[i];
    const dim3 grid((unsigned)((pos + LF_BM - 1) / LF_BM), 1);
    if (i == 0) hipLaunchKernelGGL((lipfe_conv_kernel<7, 1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((lipfe_conv_kernel<5, 5>), grid, dim3(256), 0, st, a);
    HANDLE_LAUNCH_CHECK(c, "vfilt conv");
    cur ^= 1;
  }
  hipLaunchKernelGGL(vfilt_conv8_kernel, dim3((unsigned)((pos * 8 + 255) / 256)), dim3(256), 0, st, act[cur], Wt[c->conv[7]],
                     fold + 128 * 7, flat, pos * 8, F, W);
  HANDLE_LAUNCH_CHECK(c, "vfilt conv8");

  // d-vector: GRU layer 1 in both directions over the 2B sequences
  const long long rows = (long long)B * Tv;          // rows of one speaker's embeddings
  for (int d = 0; d < 2; ++d)
    for (int s = 0; s < 2; ++s) {
      const int g = c->gru[0][d];
      VfGemmArgs a = vf_gemm_args(s ? emb2 : emb1, E, 1, Wt[g], E, 1, Wt[g + 2],
                                  gi0 + ((long long)d * nseq * Tv + s * rows) * 3 * F, 3 * F, 1, (int)rows, 3 * F, E);
      if (int rc = vf_launch_gemm(c, st, a, 1, "vfilt gru input 1")) return rc;
    }
  VfTransposeSrc ts;
  ts.w[0] = Wt[c->gru[0][0] + 1];  ts.w[1] = Wt[c->gru[0][1] + 1];  ts.w[2] = Wt[c->gru[1][0] + 1];
  hipLaunchKernelGGL(vfilt_transpose_kernel, dim3((3 * F * F + 255) / 256, 3), dim3(256), 0, st, ts, whht, F);
  HANDLE_LAUNCH_CHECK(c, "vfilt gru transpose");
  VfGruArgs ga;
  for (int d = 0; d < 2; ++d) {
    ga.gi[d] = gi0 + (long long)d * nseq * Tv * 3 * F;  ga.whht[d] = whht + (long long)d * 3 * F * F;  ga.bhh[d] = Wt[c->gru[0][d] + 3];
  }
  ga.y = y0;  ga.ldy = 2 * F;  ga.Tv = Tv;  ga.F = F;
  hipLaunchKernelGGL(vfilt_gru_kernel, dim3(nseq, 2), dim3(1024), 0, st, ga);
  HANDLE_LAUNCH_CHECK(c, "vfilt gru 1");
  // layer 2 forward in full; its backward direction only at the last position, where it starts
  {
    const int g = c->gru[1][0];
    VfGemmArgs a = vf_gemm_args(y0, 2 * F, 1, Wt[g], 2 * F, 1, Wt[g + 2], gi1, 3 * F, 1, (int)(2 * rows), 3 * F, 2 * F);
    if (int rc = vf_launch_gemm(c, st, a, 1, "vfilt gru input 2")) return rc;
    ga.gi[0] = ga.gi[1] = gi1;  ga.whht[0] = ga.whht[1] = whht + (long long)2 * 3 * F * F;  ga.bhh[0] = ga.bhh[1] = Wt[g + 3];
    ga.y = y1;
    hipLaunchKernelGGL(vfilt_gru_kernel, dim3(nseq, 1), dim3(1024), 0, st, ga);
    HANDLE_LAUNCH_CHECK(c, "vfilt gru 2");
    const int gb = c->gru[1][1];
    const long long last = (long long)(Tv - 1) * 2 * F;
    a = vf_gemm_args(y0 + last, (long long)Tv * 2 * F, 1, Wt[gb], 2 * F, 1, Wt[gb + 2], gi1b, 3 * F, 1, nseq, 3 * F, 2 * F);
    if (int rc = vf_launch_gemm(c, st, a, 1, "vfilt gru input 2 reverse")) return rc;
    hipLaunchKernelGGL(vfilt_gru_first_step_kernel, dim3(nseq), dim3(320), 0, st, gi1b, Wt[gb + 3], y1 + last + F,
                       (long long)Tv * 2 * F, F);
    HANDLE_LAUNCH_CHECK(c, "vfilt gru 2 reverse");
    a = vf_gemm_args(y1 + last, (long long)Tv * 2 * F, 1, Wt[c->fcd], 2 * F, 1, Wt[c->fcd + 1], dvec, F, 1, nseq, F, 2 * F);
    if (int rc = vf_launch_gemm(c, st, a, 1, "vfilt fc_dvector")) return rc;
  }

  // LSTM input: the d-vector's columns of W_ih with both biases, then the map's columns, one GEMM per item
  {
    const float* wih = Wt[c->lstm];
    VfGemmArgs a = vf_gemm_args(dvec, F, 1, wih + 8 * F, 9 * F, 1, Wt[c->lstm + 2], D, VF_G, 1, nseq, VF_G, F);
    a.bias2 = Wt[c->lstm + 3];
    if (int rc = vf_launch_gemm(c, st, a, 1, "vfilt lstm d-vector")) return rc;
    a = vf_gemm_args(flat, 1, W, wih, 9 * F, 1, nullptr, G, VF_G, 1, W, VF_G, 8 * F);
    a.sab = (long long)8 * F * W;  a.scb = (long long)W * VF_G;
    if (int rc = vf_launch_gemm(c, st, a, B, "vfilt lstm projection")) return rc;
  }
  VfLstmArgs la;
  la.G = G;  la.D = D;  la.whh = Wt[c->lstm + 1];  la.Hb = Hb;  la.cst = cst;  la.B = B;  la.W = W;  la.nseq = nseq;
  for (int t = 0; t < W; ++t) {
    la.t = t;
    if (nseq == 2) hipLaunchKernelGGL(vfilt_lstm_step_kernel<2>, dim3(VF_H / 4, 1), dim3(256), 0, st, la);
    else hipLaunchKernelGGL(vfilt_lstm_step_kernel<8>, dim3(VF_H / 4, (nseq + 7) / 8), dim3(256), 0, st, la);
    HANDLE_LAUNCH_CHECK(c, "vfilt lstm step");
  }

  // FC tail
  {
    VfGemmArgs a = vf_gemm_args(Hb, VF_H, 1, Wt[c->fc1], VF_H, 1, Wt[c->fc1 + 1], fcb, VF_FC, 1, nseq * W, VF_FC, VF_H);
    a.relu_a = 1;  a.act = VF_ACT_RELU;
    if (int rc = vf_launch_gemm(c, st, a, 1, "vfilt fc 1")) return rc;
    for (int s = 0; s < 2; ++s) {
      a = vf_gemm_args(fcb + (long long)s * B * W * VF_FC, VF_FC, 1, Wt[c->fc2], VF_FC, 1, Wt[c->fc2 + 1], s ? out2 : out1, 1, W,
                       W, F, VF_FC);
      a.sab = (long long)W * VF_FC;  a.scb = (long long)F * W;
      a.act = VF_ACT_SIGMOID;  a.mul = mix;
      if (int rc = vf_launch_gemm(c, st, a, B, "vfilt fc 2")) return rc;
    }
  }
  return VFILT_OK;
}

double vfilt_flops_per_item(vfilt_handle h, int W, int Tv) {
  if (!h || vf_check_shape(h->F, 1, W, Tv)) return 0.0;
  return 2.0 * vf_macs(h->F, h->E, W, Tv);
}

double vfilt_min_bytes_per_item(vfilt_handle h, int W, int Tv) {
  if (!h || vf_check_shape(h->F, 1, W, Tv)) return 0.0;
  const double f = h->F, e = h->E, pos = f * W;
  double fl = pos + pos * 64;                                    // layer 1
  fl += 6.0 * 2 * pos * 64;                                      // layers 2..7
  fl += pos * 64 + pos * 8;                                      // layer 8
  fl += pos * 8 + (double)W * VF_G + (double)VF_G * 8 * f;       // projection
  fl += (double)W * (VF_G * (double)VF_H + 2.0 * (VF_G + 2 * VF_H + 2 * VF_G));   // recurrence: W_hh, h, G, D per step
  fl += 2.0 * W * (VF_H + 2.0 * VF_FC + 2 * f) + f * W;          // FC tail, mixture
  fl += 2.0 * Tv * (e + 2 * 3 * f * 2 + 2 * 2 * f + 3 * f + 2 * f) + 2.0 * 3 * f * (2 * e + 2 * 2 * f)
        + (double)Tv * 3 * 3 * f * f;                            // GRU: embeddings, gates, outputs, weights (W_hh per step)
  return 4.0 * fl;
}

}  // extern "C"
