// deepctasnet_train.hip -- DeepConvTasNet training step (src/model/deepconvtasnet.py forward + its autograd backward) for
// gfx950: handle and the extern "C" boundary declared in include/dctasnet_train.h.
//
// Training forward: the launch sequence of deepctasnet.hip in its TAPE mode (deepctasnet_kernels.h, ctasnet_kernels.h: one
// text for both), so the predictions are bitwise those of dctasnet_forward.  On top of the Separator's tape
// (ctasnet_train_kernels.h) the tape keeps the first conv's output c0 [M][512] and, for each of the eight dense k = 3
// layers, its pre-activation z (encoder [M][512], decoder [2M][512], rows (b, f, speaker)): the slopes may be 0, 1 or
// negative, so the sign of z cannot be recovered from PReLU(z).  Only z is stored; the next layer's A loader applies the
// PReLU.  The two activations that plain-row kernels read -- the encoder output enc (the Separator's tape has it) and the
// last decoder activation (the taps kernel; scratch, not tape) -- are stored as well.
//
// Backward, last layer to first: output head (taps gradient, d bias, d W from PReLU(z_3) and the taps gradient, d y_3 =
// d taps W^T), four ConvTranspose layers, mask head in its d ym form + launch_separator_backward, four Conv1d layers,
// first conv.  Per dense layer: PReLU backward in place (slope partials), bias column sums, three taps x four 128-column
// slices of the MFMA weight-gradient kernel (backward.h wgrad_kernel<512, 128>, static tile schedule) through tap-shifted
// loaders, and the data gradient as three accumulating passes of the engine on the weights packed in the other
// orientation (a Conv1d's data gradient is the ConvTranspose form and vice versa) with the shifts negated.  The pack runs
// at the start of every backward from the weights as they are then.  No atomics: every partial goes to a slab and is
// summed in a fixed order, so two backward calls on one tape give bitwise-identical gradients.
// decoder.deconv.weight is never read by the reference's forward: its gradient buffer is never written and
// dcttrain_adamw_step leaves the weight alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dctasnet_train.h"
#include "ctasnet_train_kernels.h"
#include "deepctasnet_kernels.h"

static_assert(DCTTRAIN_OK == CTASNET_OK && DCTTRAIN_ERR_INVALID == CTASNET_ERR_INVALID &&
                  DCTTRAIN_ERR_WORKSPACE == CTASNET_ERR_WORKSPACE && DCTTRAIN_ERR_WEIGHTS == CTASNET_ERR_WEIGHTS &&
                  DCTTRAIN_ERR_HIP == CTASNET_ERR_HIP,
              "the shared Conv-TasNet code returns CTASNET_* codes");

namespace {

constexpr int DCT_G_W = 256;                        // workgroups of a dense weight-gradient launch (at most): one per CU
constexpr int DCT_WN = CT_N, DCT_WK = 128;          // its tile: dW[512][128 columns of one tap]
constexpr int DCT_UNUSED = DC_DEC0 + 14;            // decoder.deconv.weight

thread_local std::string g_create_error;

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// d bias of the output head: the sum of d_s1 and d_s2 over all cropped samples; per-workgroup partials -> aslab
__global__ __launch_bounds__(256) void dcttrain_outsum_kernel(const float* __restrict__ d1, const float* __restrict__ d2,
                                                              int64_t n, float* __restrict__ aslab) {
  __shared__ float red[256];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += d1[i] + d2[i];
  const float t = block_sum256(s, red);
  if (threadIdx.x == 0) aslab[blockIdx.x] = t;
}

// Sum of wgrad_kernel's partial tiles (fragment order, see slab_reduce_frag_kernel in backward.h: same association
// order) into a strided destination: element (row, col) of the [32 RB * 4][32 CB] tile goes to out[row * ldo + col * cs].
// One tap's 128-column slice of a dense layer's weight gradient lands in weight[.][.][k] this way (ldo = 1536, cs = 3).
template <int RB, int CB>
__global__ __launch_bounds__(256) void dcttrain_reduce_frag_kernel(const float* __restrict__ slab, int nslabs, int64_t stride,
                                                                   float* __restrict__ out, int ldo, int cs) {
  __shared__ float4 red[8][32];
  const int e = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int f = blockIdx.x * 32 + e;                 // < RB * CB * 1024
  const float4* src = reinterpret_cast<const float4*>(slab) + f;
  const int64_t st4 = stride / 4;
  auto add = [](float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; };
  float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
  int k = sl;
  for (; k + 24 < nslabs; k += 32) {
    add(s0, src[(int64_t)k * st4]);
    add(s1, src[(int64_t)(k + 8) * st4]);
    add(s2, src[(int64_t)(k + 16) * st4]);
    add(s3, src[(int64_t)(k + 24) * st4]);
  }
  for (; k < nslabs; k += 8) add(s0, src[(int64_t)k * st4]);
  add(s0, s1);
  add(s2, s3);
  add(s0, s2);
  red[sl][e] = s0;
  __syncthreads();
  if (sl == 0) {
    float4 s = red[0][e];
#pragma unroll
    for (int j = 1; j < 8; ++j) add(s, red[j][e]);
    const int lane = f & 63, g4 = (f >> 6) & 3, t = f >> 8;          // t = (w * RB + i) * CB + j
    const int j = t % CB, wi = t / CB, i = wi % RB, w = wi / RB;
    const int row = (w + 4 * i) * 32 + 8 * g4 + 4 * (lane >> 5), col = j * 32 + (lane & 31);
    float* dst = out + (size_t)row * ldo + (size_t)col * cs;
    dst[0] = s.x;
    dst[ldo] = s.y;
    dst[2 * (size_t)ldo] = s.z;
    dst[3 * (size_t)ldo] = s.w;
  }
}

// operand of a dense layer's weight gradient: columns [col0, col0 + 4 * k4max) of row r + shift * 2^lg of a [M][512]
// tensor when frame (r >> lg) % F + shift lies in the sequence, else zeros; rows beyond M are zeros.
// PRE: the rows hold pre-activations, PReLU with *slope on load (the forward's own operation).
template <bool PRE>
struct ALoadTapCols {
  const float* A;
  const float* slope;
  int M, F, lg, shift, col0;
  DEV float4 load4(int tile, int row, int k4) const {
    const int r = tile * 32 + row;
    if (r >= M) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int f = (r >> lg) % F + shift;
    if (f < 0 || f >= F) return make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = *reinterpret_cast<const float4*>(A + (int64_t)(r + shift * (1 << lg)) * CT_N + col0 + 4 * k4);
    if constexpr (PRE) {
      const float a = *slope;
      v = make_float4(prelu(v.x, a), prelu(v.y, a), prelu(v.z, a), prelu(v.w, a));
    }
    return v;
  }
};

struct Plan : TrainPlanBase {
  size_t off_wpk, off_c0, off_ez, off_dz, off_ga, off_gb;
};

}  // namespace

static_assert(DCTTRAIN_TAPE_V1 == SEP_TAPE_V1 && DCTTRAIN_TAPE_U == SEP_TAPE_U && DCTTRAIN_TAPE_SKIP == SEP_TAPE_SKIP,
              "sep_tape_offset takes the header's tape kinds");

struct dcttrain_ctx : CtTrainHandle {
  dcttrain_ctx() : CtTrainHandle("dcttrain", DCT_UNUSED) {}
};

namespace {

int make_plan(CtHandle* c, int B, int64_t T, Plan& p) {
  // the decoder runs on 2*B*F rows of 512 (32-bit row indexing in the tap-shifted loaders)
  if (int rc = plan_train_head(c, B, T, "2*B*F*512", p)) return rc;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t r = o; o += align256(bytes); return r; };
  const size_t M = (size_t)p.M;
  plan_separator_train(p, o, B, M, (size_t)DCT_G_W * DCT_WN * DCT_WK);
  p.off_wpk = take((size_t)DC_LAYERS * 3 * DC_TAP_FLOATS * 4);   // forward pack, then the backward's
  p.off_c0 = take(M * CT_N * 4);                                  // tape: first conv output
  p.off_ez = take(4 * M * CT_N * 4);                              // tape: encoder pre-activations
  p.off_dz = take(4 * 2 * M * CT_N * 4);                          // tape: decoder pre-activations
  p.off_ga = take(2 * M * CT_N * 4);                              // backward ping-pong
  p.off_gb = take(2 * M * CT_N * 4);
  p.total = o;
  return DCTTRAIN_OK;
}

void pack_sources(const std::vector<const float*>& W, PackSrc& ps) {
  for (int l = 0; l < 4; ++l) {
    ps.w[l] = W[2 + 3 * l];                   // encoder.sequential.{1,3,5,7}.weight
    ps.w[4 + l] = W[DC_DEC0 + 3 * l];         // decoder.sequential.{0,2,4,6}.weight
  }
}

// one tap's 128-column slice of a dense weight gradient: partial tiles of wgrad_kernel (static schedule), then the sum
// into out[row * 1536 + col * 3]
template <class YL, class XL>
int launch_dense_wgrad(dcttrain_ctx* c, hipStream_t st, int64_t rows, const YL& yl, const XL& xl, float* slab, float* out) {
  auto kern = wgrad_kernel<DCT_WN, DCT_WK, YL, XL, false>;
  const size_t lds = WgradShape<DCT_WN, DCT_WK>::lds_bytes();
  static PerDeviceOnce once;
  if (int rc = ensure_lds(c, once, kern, lds, "dcttrain dense wgrad")) return rc;
  const int ntiles = (int)((rows + 31) / 32);
  const int g = std::min(ntiles, DCT_G_W);
  hipLaunchKernelGGL(kern, dim3(g), dim3(256), lds, st, ntiles, (unsigned*)nullptr, yl, xl, slab, (float*)nullptr);
  CT_LAUNCH_CHECK(c, "dcttrain dense wgrad");
  constexpr int RB = DCT_WN / 128, CB = DCT_WK / 32;
  hipLaunchKernelGGL((dcttrain_reduce_frag_kernel<RB, CB>), dim3(RB * CB * 32), dim3(256), 0, st, slab, g,
                     (int64_t)DCT_WN * DCT_WK, out, 3 * CT_N, 3);
  CT_LAUNCH_CHECK(c, "dcttrain dense wgrad reduce");
  return DCTTRAIN_OK;
}

struct DenseBwd {
  bool transposed;      // ConvTranspose1d (decoder) or Conv1d (encoder)
  int dil, lg;
  int64_t rows;
  int F;
  float* dy;            // [rows][512] gradient of the layer's output; becomes dz in place
  const float* z;       // tape: pre-activation
  const float* x;       // the layer's input rows: pre-activations of the layer before when xslope is not null
  const float* xslope;
  const float* slope;
  const float* wpk;     // this layer's three taps, packed in the other orientation
  float* dx;            // [rows][512] out
  float* gw;
  float* gb;
  float* ga;
};

template <bool PRE>
int dense_wgrads(dcttrain_ctx* c, hipStream_t st, const DenseBwd& d, float* slab) {
  const int rows = (int)d.rows;
  for (int k = 0; k < 3; ++k) {
    const int shift = d.transposed ? (1 - k) * d.dil : (k - 1) * d.dil;
    for (int q = 0; q < CT_N / DCT_WK; ++q) {
      float* out = d.gw + (size_t)DCT_WK * q * 3 + k;
      int rc;
      if (d.transposed)     // weight (in, out, k): rows of dW are input channels
        rc = launch_dense_wgrad(c, st, d.rows, ALoadTapCols<PRE>{d.x, d.xslope, rows, d.F, d.lg, shift, 0},
                                ALoadTapCols<false>{d.dy, nullptr, rows, d.F, d.lg, 0, DCT_WK * q}, slab, out);
      else                  // weight (out, in, k): rows of dW are output channels
        rc = launch_dense_wgrad(c, st, d.rows, ALoadTapCols<false>{d.dy, nullptr, rows, d.F, d.lg, 0, 0},
                                ALoadTapCols<PRE>{d.x, d.xslope, rows, d.F, d.lg, shift, DCT_WK * q}, slab, out);
      if (rc) return rc;
    }
  }
  return DCTTRAIN_OK;
}

// backward of one dense k = 3 layer + PReLU
int dense_backward(dcttrain_ctx* c, hipStream_t st, const DenseBwd& d, float* slab, float* cslab, float* aslab) {
  // PReLU: dz = dy (z > 0 ? 1 : a) in place, d a = sum dy z over z <= 0
  hipLaunchKernelGGL(cttrain_prelu_bwd_kernel, dim3(CTT_G_ROW), dim3(256), 0, st, d.dy, d.z, d.slope, d.rows * CT_N, aslab);
  CT_LAUNCH_CHECK(c, "dcttrain dense prelu backward");
  if (int rc = launch_reduce(c, st, aslab, CTT_G_ROW, 1, 1, 1, d.ga, 1)) return rc;
  if (int rc = launch_colsum<CT_N>(c, st, d.dy, d.rows, CT_N, 0, cslab, d.gb)) return rc;
  if (int rc = d.xslope ? dense_wgrads<true>(c, st, d, slab) : dense_wgrads<false>(c, st, d, slab)) return rc;
  // data gradient: dx[r] = sum_k V_k dz[r - s_k], zero where frame(r) - s_k leaves the sequence
  for (int k = 0; k < 3; ++k) {
    const int shift = d.transposed ? (1 - k) * d.dil : (k - 1) * d.dil;
    if (int rc = launch_gemm<CT_N>(c, st, "dcttrain dense dgrad", d.wpk + k * DC_TAP_FLOATS, nullptr, d.rows, CT_N / 128,
                                   ALoadTapShiftT<false>{d.dy, nullptr, (int)d.rows, d.F, d.lg, -shift},
                                   EpiStoreAdd{d.dx, d.rows, CT_N, k > 0}, 0))
      return rc;
  }
  return DCTTRAIN_OK;
}

}  // namespace

extern "C" {

int dcttrain_abi_version(void) { return DCTTRAIN_ABI_VERSION; }

int dcttrain_create(dcttrain_handle* out, int av) {
  if (av != 0) {
    if (out) *out = nullptr;
    g_create_error = "the audio-visual training step (DeepAVConvTasNet) is not built: dcttrain_create takes av = 0";
    return DCTTRAIN_ERR_INVALID;
  }
  if (int rc = ct_create(out, "deep Conv-TasNet training step", g_create_error)) return rc;
  dcttrain_ctx* c = *out;
  add_deepconvtasnet_names(c, false);
  c->w.assign(c->names.size(), nullptr);
  c->g.assign(c->names.size(), nullptr);
  return DCTTRAIN_OK;
}

void dcttrain_destroy(dcttrain_handle h) { delete h; }

const char* dcttrain_last_error(dcttrain_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int dcttrain_num_weights(dcttrain_handle h) { return h ? (int)h->names.size() : 0; }

const char* dcttrain_weight_name(dcttrain_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t dcttrain_weight_numel(dcttrain_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int dcttrain_bind_weights(dcttrain_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n) : DCTTRAIN_ERR_INVALID;
}

int dcttrain_bind_grads(dcttrain_handle h, float* const* dev_ptrs, int n) {
  return h ? bind_grads(h, dev_ptrs, n) : DCTTRAIN_ERR_INVALID;
}

int64_t dcttrain_flat_offset(dcttrain_handle h, int slot) { return h ? flat_offset(h, slot) : -1; }

int64_t dcttrain_flat_numel(dcttrain_handle h) { return h ? flat_numel(h) : -1; }

int64_t dcttrain_frames(int64_t T) { return frames_of(T); }

int64_t dcttrain_out_len(int64_t T) { return out_len_of(T); }

size_t dcttrain_workspace_bytes(dcttrain_handle h, int B, int64_t T) {
  if (!h) return 0;
  Plan p;
  if (make_plan(h, B, T, p)) return 0;
  return p.total;
}

int64_t dcttrain_tape_offset(dcttrain_handle h, int B, int64_t T, int which, int block) {
  if (!h) return -1;
  Plan p;
  if (make_plan(h, B, T, p)) return -1;
  const size_t M = (size_t)p.M;
  if (which == DCTTRAIN_TAPE_ENC_Z || which == DCTTRAIN_TAPE_DEC_Z) {
    if (block < 0 || block >= 4) {
      h->fail(DCTTRAIN_ERR_INVALID, "dense layer %d out of range", block);
      return -1;
    }
    return which == DCTTRAIN_TAPE_ENC_Z ? (int64_t)(p.off_ez + (size_t)block * M * CT_N * 4)
                                        : (int64_t)(p.off_dz + (size_t)block * 2 * M * CT_N * 4);
  }
  return sep_tape_offset(h, p, which, block);
}

int dcttrain_train_forward(dcttrain_handle h, const float* mix, int B, int64_t T, float* s1_pred, float* s2_pred, void* ws,
                           size_t ws_bytes, void* stream) {
  dcttrain_ctx* c = h;
  Plan p;
  WsPtr at;
  if (int rc = train_prologue(c, make_plan, false, mix, s1_pred, s2_pred, B, T, ws, ws_bytes, p, at)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  float* wpk = at.fp(p.off_wpk);
  float* enc = at.fp(p.off_enc);
  float* c0 = at.fp(p.off_c0);
  float* ym = at.fp(p.off_ym);
  float* ydec = at.fp(p.off_dv);          // the last decoder activation [2M][512]: scratch until the backward's head kernel
  float* taps = at.fp(p.off_taps);
  const SepBuffers sb = sep_tape_buffers(p, ws);

  // weights of the eight dense convs -> fragment order, this forward's copy
  PackSrc ps;
  pack_sources(W, ps);
  ps.tmask = 0xF0u;
  hipLaunchKernelGGL(dctasnet_pack_kernel, dim3((unsigned)(DC_TAP_FLOATS / 4 / 256), DC_LAYERS), dim3(256), 0, st, ps, wpk);
  CT_LAUNCH_CHECK(c, "dcttrain weight pack");

  // deep encoder (deepconvtasnet.py:7-26): first conv -> c0; layer l reads c0 / PReLU(z_{l-1}) and writes z_l; the last one
  // also writes enc = PReLU(z_3) and the GlobalNorm partials
  const unsigned row_wgs = (unsigned)((M + CT_ROWS_PER_WG - 1) / CT_ROWS_PER_WG);
  hipLaunchKernelGGL(ctasnet_encoder_kernel<true>, dim3(row_wgs), dim3(256), 0, st, mix, T, F, M, W[0], W[1], c0, nullptr);
  CT_LAUNCH_CHECK(c, "dcttrain encoder");
  for (int l = 0; l < 4; ++l) {
    float* z = at.fp(p.off_ez) + (size_t)l * M * CT_N;
    const float* x = l == 0 ? c0 : z - (size_t)M * CT_N;
    if (int rc = launch_dense<true>(c, st, wpk + (int64_t)l * 3 * DC_TAP_FLOATS, false, 1 << l, x, l == 0 ? nullptr : W[1 + 3 * l],
                                    z, l == 3 ? enc : nullptr, M, F, 0, W[3 + 3 * l], W[4 + 3 * l], nullptr,
                                    l == 3 ? sb.part : nullptr))
      return rc;
  }

  // Separator on its tape: masks times the encoder output -> ym [M][1024]
  if (int rc = launch_separator<true>(c, st, W.data() + DC_SEP0, enc, 4, 128.0f, B, F, M, sb)) return rc;

  // deep decoder (deepconvtasnet.py:96-120) on 2M rows (b, f, speaker), then the output head as taps + overlap-add
  for (int l = 0; l < 4; ++l) {
    float* z = at.fp(p.off_dz) + (size_t)l * 2 * M * CT_N;
    const float* x = l == 0 ? ym : z - (size_t)2 * M * CT_N;
    if (int rc = launch_dense<true>(c, st, wpk + (int64_t)(4 + l) * 3 * DC_TAP_FLOATS, true, 8 >> l, x,
                                    l == 0 ? nullptr : W[DC_DEC0 + 3 * l - 1], z, l == 3 ? ydec : nullptr, 2 * M, F, 1,
                                    W[DC_DEC0 + 1 + 3 * l], W[DC_DEC0 + 2 + 3 * l], nullptr, nullptr))
      return rc;
  }
  if (int rc = launch_taps(c, st, ydec, W[DC_DEC0 + 12], M, taps)) return rc;
  return launch_overlap_add<true>(c, st, taps, W[DC_DEC0 + 13], B, F, p.Lout, s1_pred, s2_pred);
}

int dcttrain_train_backward(dcttrain_handle h, const float* mix, int B, int64_t T, const float* d_s1, const float* d_s2, void* ws,
                            size_t ws_bytes, void* stream) {
  dcttrain_ctx* c = h;
  Plan p;
  WsPtr at;
  if (int rc = train_prologue(c, make_plan, true, mix, d_s1, d_s2, B, T, ws, ws_bytes, p, at)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  const auto& G = c->g;
  float* wpk = at.fp(p.off_wpk);
  float* dtaps = at.fp(p.off_taps);
  float* denc = at.fp(p.off_denc);
  float* slab = at.fp(p.off_slab);
  float* cslab = at.fp(p.off_cslab);
  float* aslab = at.fp(p.off_aslab);
  float* ga = at.fp(p.off_ga);
  float* gb = at.fp(p.off_gb);
  int ns = 0;

  // the eight layers' weights for the data gradients, from the weights as they are now: the other orientation
  PackSrc ps;
  pack_sources(W, ps);
  ps.tmask = 0x0Fu;
  hipLaunchKernelGGL(dctasnet_pack_kernel, dim3((unsigned)(DC_TAP_FLOATS / 4 / 256), DC_LAYERS), dim3(256), 0, st, ps, wpk);
  CT_LAUNCH_CHECK(c, "dcttrain backward weight pack");

  // ---- output head (decoder.sequential.8, ConvTranspose1d(512, 1, 32, 16) + bias, cropped): d taps, d bias, d W, d y_3
  {
    const int64_t n = M * 4 * CT_L;
    hipLaunchKernelGGL(cttrain_dtaps_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_s1, d_s2, F, M, p.Lout, dtaps);
    CT_LAUNCH_CHECK(c, "dcttrain dtaps");
    hipLaunchKernelGGL(dcttrain_outsum_kernel, dim3(CTT_G_ROW), dim3(256), 0, st, d_s1, d_s2, (int64_t)B * p.Lout, aslab);
    CT_LAUNCH_CHECK(c, "dcttrain output bias");
    if (int rc = launch_reduce(c, st, aslab, CTT_G_ROW, 1, 1, 1, G[DC_DEC0 + 13], 1)) return rc;
    const float* z3 = at.fp(p.off_dz) + (size_t)3 * 2 * M * CT_N;
    if (int rc = launch_wgrad<CT_N, 2 * CT_L>(c, st, 2 * M, ALoadDensePReLU{z3, W[DC_DEC0 + 11], 2 * M, CT_N, 32},
                                              ALoadDense{dtaps, 2 * M, 2 * CT_L, 32}, slab, &ns))
      return rc;
    if (int rc = launch_reduce(c, st, slab, ns, (int64_t)CT_N * 2 * CT_L, CT_N, 2 * CT_L, G[DC_DEC0 + 12], 2 * CT_L)) return rc;
    static PerDeviceOnce once;
    if (int rc = ensure_lds(c, once, cttrain_head_bwd_kernel<HEAD_DYM_OUT>, CTT_HEAD_LDS, "dcttrain head dgrad")) return rc;
    const unsigned g = (unsigned)std::min<int64_t>(M, 2048);
    hipLaunchKernelGGL(cttrain_head_bwd_kernel<HEAD_DYM_OUT>, dim3(g), dim3(256), CTT_HEAD_LDS, st, dtaps, W[DC_DEC0 + 12], nullptr,
                       nullptr, M, ga, nullptr);
    CT_LAUNCH_CHECK(c, "dcttrain head dgrad");
  }

  // ---- deep decoder, layers 3..0 (d = 1, 2, 4, 8) on 2M rows: ga -> gb -> ga -> gb -> ga = d ym
  float* dy = ga;
  float* dx = gb;
  for (int l = 3; l >= 0; --l) {
    const float* z = at.fp(p.off_dz) + (size_t)l * 2 * M * CT_N;
    const DenseBwd d{true, 8 >> l, 1, 2 * M, F, dy, z, l == 0 ? at.fp(p.off_ym) : z - (size_t)2 * M * CT_N,
                     l == 0 ? nullptr : W[DC_DEC0 + 3 * l - 1], W[DC_DEC0 + 2 + 3 * l], wpk + (int64_t)(4 + l) * 3 * DC_TAP_FLOATS,
                     dx, G[DC_DEC0 + 3 * l], G[DC_DEC0 + 1 + 3 * l], G[DC_DEC0 + 2 + 3 * l]};
    if (int rc = dense_backward(c, st, d, slab, cslab, aslab)) return rc;
    std::swap(dy, dx);
  }

  // ---- Separator (convtasnet.py:55-83): mask head from d ym, 24 blocks, bottleneck, GlobalNorm -> d enc
  if (int rc = launch_separator_backward<HEAD_DYM>(c, st, W.data() + DC_SEP0, G.data() + DC_SEP0, dy, nullptr, B, F, M, p, ws))
    return rc;

  // ---- deep encoder, layers 3..0 (d = 8, 4, 2, 1) on M rows: denc -> ga -> gb -> ga -> gb = d c0
  dy = denc;
  dx = ga;
  for (int l = 3; l >= 0; --l) {
    const float* z = at.fp(p.off_ez) + (size_t)l * M * CT_N;
    const DenseBwd d{false, 1 << l, 0, M, F, dy, z, l == 0 ? at.fp(p.off_c0) : z - (size_t)M * CT_N,
                     l == 0 ? nullptr : W[1 + 3 * l], W[4 + 3 * l], wpk + (int64_t)l * 3 * DC_TAP_FLOATS, dx, G[2 + 3 * l],
                     G[3 + 3 * l], G[4 + 3 * l]};
    if (int rc = dense_backward(c, st, d, slab, cslab, aslab)) return rc;
    dy = dx;
    dx = dy == ga ? gb : ga;
  }

  // ---- first conv (encoder.sequential.0, Conv1d(1, 512, 32, 16) + bias): d W[n][k] = sum_rows d c0[row][n] xpad[16 f + k]
  if (int rc = launch_wgrad<CT_N, 2 * CT_L>(c, st, M, ALoadDense{dy, M, CT_N, 32}, ALoadPatches{mix, T, M, F}, slab, &ns))
    return rc;
  if (int rc = launch_reduce(c, st, slab, ns, (int64_t)CT_N * 2 * CT_L, CT_N, 2 * CT_L, G[0], 2 * CT_L)) return rc;
  return launch_colsum<CT_N>(c, st, dy, M, CT_N, 0, cslab, G[1]);
}

size_t dcttrain_clip_scratch_bytes(dcttrain_handle) { return CLIP_PARTS * sizeof(double); }

int dcttrain_grad_clip(dcttrain_handle h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                       float* norm_out, void* stream) {
  return h ? train_grad_clip(h, flat_grad, n_flat, max_norm, scratch, scratch_bytes, norm_out, stream) : DCTTRAIN_ERR_INVALID;
}

// decoder.deconv.weight (no_grad_slot) takes no step and no decay: what torch.optim.AdamW does with .grad None
int dcttrain_adamw_step(dcttrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                        double beta1, double beta2, double eps, double weight_decay, int step, void* stream) {
  return h ? train_adamw_step(h, flat_grad, exp_avg, exp_avg_sq, n_flat, lr, beta1, beta2, eps, weight_decay, step, stream)
           : DCTTRAIN_ERR_INVALID;
}

double dcttrain_flops_per_mixture(dcttrain_handle, int64_t T) {
  // forward MACs (dctasnet_flops_per_mixture) x 3: the backward is one data-gradient and one weight-gradient product per
  // forward product
  return 3.0 * 2.0 * deepconvtasnet_macs() * (double)frames_of(T);
}

}  // extern "C"
