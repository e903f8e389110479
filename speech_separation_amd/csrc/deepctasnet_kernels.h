// deepctasnet_kernels.h -- what the deep Conv-TasNet units share (deepctasnet.hip: DeepConvTasNet / DeepAVConvTasNet
// forward, deepctasnet_train.hip: TrainableDeepConvTasNet / TrainableDeepAVConvTasNet): the weight table, the fragment-order
// pack of the eight dense k = 3 convs, their engine hooks and launch_dense, and the two kernels of the audio-visual head.  Everything sits in an anonymous namespace, so each including unit
// compiles its own copy.
//
// TAPE (the training forward): a dense conv stores its pre-activation z (the input of its PReLU) where the inference mode
// stores PReLU(z), and the next layer's A loader applies the PReLU while it loads, with the same float operations -- the
// pattern of the Separator's tape (ctasnet_kernels.h).  The last layer of the encoder and of the decoder feed kernels
// that read plain rows, so they store PReLU(z) as well (`act`).
#pragma once
#include "ctasnet_handle.h"

namespace {

constexpr int DC_ENC_W = 14;                                   // encoder.sequential.{0..8}
constexpr int DC_DEC_W = 14;                                   // decoder.sequential.{0..8}
constexpr int DC_NW_AUDIO = DC_ENC_W + CT_SEP_W + DC_DEC_W + 1;   // + decoder.deconv.weight (unused)
constexpr int DC_NW_AV = DC_NW_AUDIO + 4;                      // + visual_compression.{weight,bias}, video_ln.{weight,bias}
constexpr int DC_SEP0 = DC_ENC_W, DC_DEC0 = DC_ENC_W + CT_SEP_W, DC_AV0 = DC_NW_AUDIO;
constexpr int DC_LAYERS = 8;                                   // dense k = 3 convs: 4 encoder + 4 decoder
constexpr int64_t DC_TAP_FLOATS = (int64_t)CT_N * CT_N;        // one tap of one layer, fragment order
constexpr int DC_HV = 256;                                     // hidden_video / 2
constexpr int DC_VT = 8;                                       // video frames per workgroup of the linear kernel

// ------------------------------------------------------------------------------------------------
// weights -> fragment order (gemm_ws.h, ldw == 0): dst[(layer*3 + k)][cb 16][m 64][lane 64][4] = W_k[32 cb + (lane & 31)]
// [8 m + 4 (lane >> 5) ..+3], W_k[o][i] the tap-k matrix.  Conv1d weight (o, i, k): the 12 floats of (o, i..i+3, 0..2) are
// contiguous.  ConvTranspose1d weight (i, o, k): W_k[o][i] = weight[i][o][k]; lanes with consecutive o read consecutive
// 12-byte groups.
// ------------------------------------------------------------------------------------------------
struct PackSrc {
  const float* w[DC_LAYERS];
  unsigned tmask;    // bit l: layer l is packed from the (in, out, k) layout.  Forward: the four decoder layers (0xF0); a
                     // Conv1d's data gradient is the ConvTranspose form and vice versa, so the backward packs with 0x0F
};

__global__ __launch_bounds__(256) void dctasnet_pack_kernel(PackSrc src, float* __restrict__ dst) {
  const int layer = blockIdx.y;
  const int f = blockIdx.x * 256 + threadIdx.x;                // < 512 * 512 / 4
  const int lane = f & 63, m = (f >> 6) & 63, cb = f >> 12;
  const int o = 32 * cb + (lane & 31), i0 = 8 * m + 4 * (lane >> 5);
  const float* W = src.w[layer];
  float v[4][3];
  if (!((src.tmask >> layer) & 1u)) {
    const float4* p = reinterpret_cast<const float4*>(W + (int64_t)o * 3 * CT_N + 3 * i0);
    const float4 a = p[0], b = p[1], c = p[2];
    const float t[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) v[i][k] = t[3 * i + k];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) v[i][k] = W[((int64_t)(i0 + i) * CT_N + o) * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    *reinterpret_cast<float4*>(dst + (layer * 3 + k) * DC_TAP_FLOATS + 4 * (int64_t)f) =
        make_float4(v[0][k], v[1][k], v[2][k], v[3][k]);
}

// ------------------------------------------------------------------------------------------------
// engine hooks of the dense conv
// ------------------------------------------------------------------------------------------------
// row r of a pass reads row r + shift * 2^lg when frame (r >> lg) % F + shift lies in the sequence, else zeros
// PRE: the rows hold pre-activations; PReLU with *slope on load (slope is not read otherwise)
template <bool PRE>
struct ALoadTapShiftT {
  const float* A;    // rows of 512
  const float* slope;
  int M;             // rows (M * 512 < 2^31: dctasnet's plan)
  int F;             // frames per sequence
  int lg;            // log2(rows per frame): 0 encoder, 1 decoder (two speakers per frame)
  int shift;         // tap offset in frames
  DEV float4 load4(int tile, int row, int k4) const {
    const int r = tile * CT_BM + row;
    if (r >= M) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int f = (r >> lg) % F + shift;
    if (f < 0 || f >= F) return make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = *reinterpret_cast<const float4*>(A + (int64_t)(r + shift * (1 << lg)) * CT_N + 4 * k4);
    if constexpr (PRE) {
      const float a = *slope;
      v = make_float4(prelu(v.x, a), prelu(v.y, a), prelu(v.z, a), prelu(v.w, a));
    }
    return v;
  }
};

// tap 0: out = v + bias; tap 1: out += v; tap 2: out = PReLU(out + v), then (last encoder conv) + the video row and the
// row partials (n = 128 per column group) of the result for the GlobalNorm that follows.
// TAPE: tap 2 stores z = out + v to `out` and, where act is not null, PReLU(z) (+ video, partials) to act [M][512]
template <bool TAPE>
struct EpiTapConvT {
  static constexpr bool DIRECT = false;
  static constexpr bool HAS_FINISH = false;
  float* out;          // [M][512]
  float* act;          // TAPE: [M][512] or null
  const float* bias;
  const float* slope;
  const float* vid;    // [M][512] or null
  float2* part;        // [M][4] or null
  int64_t M;
  int tap;
  struct Cols { float4 b; float a; };
  DEV Cols cols(int colgroup, int c4) const {
    return Cols{*reinterpret_cast<const float4*>(bias + colgroup * 128 + 4 * c4), *slope};
  }
  // the partial sum of the earlier taps: independent of the product (blockIdx.y is the engine's column group)
  DEV float4 prefetch(int tile, int row, int c4) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    if (tap == 0 || r >= M) return make_float4(0.f, 0.f, 0.f, 0.f);
    return *reinterpret_cast<const float4*>(out + r * CT_N + blockIdx.y * 128 + 4 * c4);
  }
  DEV void row(int tile, int row, int colgroup, int c4, float4 v, float4 prev, const Cols& k) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    const int col = colgroup * 128 + 4 * c4;
    if (tap == 0) {
      v = make_float4(v.x + k.b.x, v.y + k.b.y, v.z + k.b.z, v.w + k.b.w);
    } else {
      v = make_float4(prev.x + v.x, prev.y + v.y, prev.z + v.z, prev.w + v.w);
    }
    if (tap == 2) {
      if constexpr (TAPE) {
        if (r < M) *reinterpret_cast<float4*>(out + r * CT_N + col) = v;
        if (act == nullptr) return;    // uniform across the launch
      }
      v = make_float4(prelu(v.x, k.a), prelu(v.y, k.a), prelu(v.z, k.a), prelu(v.w, k.a));
      if (vid != nullptr && r < M) {
        const float4 e = *reinterpret_cast<const float4*>(vid + r * CT_N + col);
        v = make_float4(v.x + e.x, v.y + e.y, v.z + e.z, v.w + e.w);
      }
      if (part != nullptr) {       // uniform across the launch: every lane of the 32-lane group takes part
        const float s = group_sum<32>((v.x + v.y) + (v.z + v.w));
        const float mu = s * (1.0f / 128.0f);
        const float dx = v.x - mu, dy = v.y - mu, dz = v.z - mu, dw = v.w - mu;
        const float q = group_sum<32>((dx * dx + dy * dy) + (dz * dz + dw * dw));
        if (r < M && c4 == 0) part[r * 4 + colgroup] = make_float2(s, q);
      }
    }
    if (r >= M) return;
    *reinterpret_cast<float4*>((TAPE && tap == 2 ? act : out) + r * CT_N + col) = v;
  }
};

// ------------------------------------------------------------------------------------------------
// video head (deepavconvtasnet.py:140-151)
// (1) vcat[b*Tv + t][s*256 + j] = bias[j] + sum_k Wvc[j][k] e_s[b][k][t]: one workgroup per (b, 8 frames), both speakers'
//     embedding columns staged in LDS, thread j owns output column j
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dctasnet_video_linear_kernel(const float* __restrict__ e1, const float* __restrict__ e2,
                                                                    const float* __restrict__ Wvc, const float* __restrict__ bvc,
                                                                    int Tv, float* __restrict__ vcat) {
  __shared__ __attribute__((aligned(16))) float es[2][DC_VT][CT_N];
  const int b = blockIdx.y, t0 = blockIdx.x * DC_VT, tid = threadIdx.x;
  for (int i = tid; i < 2 * DC_VT * CT_N; i += 256) {          // t fastest: coalesced along the embedding's time axis
    const int tt = i % DC_VT, k = (i / DC_VT) % CT_N, s = i / (DC_VT * CT_N);
    const float* e = s ? e2 : e1;
    es[s][tt][k] = t0 + tt < Tv ? e[((int64_t)b * CT_N + k) * Tv + t0 + tt] : 0.f;
  }
  __syncthreads();
  const int j = tid;
  const float bj = bvc[j];
  float acc[2][DC_VT];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int tt = 0; tt < DC_VT; ++tt) acc[s][tt] = bj;
  const float* wr = Wvc + (int64_t)j * CT_N;
  for (int k4 = 0; k4 < CT_N / 4; ++k4) {
    const float4 w = *reinterpret_cast<const float4*>(wr + 4 * k4);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int tt = 0; tt < DC_VT; ++tt) {
        const float4 x = *reinterpret_cast<const float4*>(&es[s][tt][4 * k4]);
        acc[s][tt] = fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, fmaf(w.x, x.x, acc[s][tt]))));
      }
  }
#pragma unroll
  for (int tt = 0; tt < DC_VT; ++tt)
    if (t0 + tt < Tv) {
#pragma unroll
      for (int s = 0; s < 2; ++s) vcat[((int64_t)b * Tv + t0 + tt) * CT_N + s * DC_HV + j] = acc[s][tt];
    }
}

// frame f of F reads rows i0, i1 of the Tv video rows with weights 1 - lam, lam (F.interpolate, linear, align_corners=False).
// One text for the forward and for the backward's recomputation (deepctasnet_train.hip): the same float operations.
struct VideoSrc { int i0, i1; float lam; };
DEV VideoSrc video_src(int f, int F, int Tv) {
  const float scale = (float)Tv / (float)F;
  float src = ((float)f + 0.5f) * scale - 0.5f;
  src = src < 0.f ? 0.f : src;
  const int i0 = (int)floorf(src);
  const int i1 = i0 + 1 < Tv ? i0 + 1 : Tv - 1;
  return VideoSrc{i0, i1, src - (float)i0};
}

// (2) vid[b*F + f] = LayerNorm_512(interpolate(vcat[b], Tv -> F, linear, align_corners=False)[f]): one wave per frame,
//     lane: channels 4 lane .. +3 and 256 + 4 lane .. +3.  Interpolation arithmetic as the DPTN-AV head (headtail.h).
__global__ __launch_bounds__(256) void dctasnet_video_frames_kernel(const float* __restrict__ vcat, const float* __restrict__ g,
                                                                    const float* __restrict__ be, int F, int Tv, int64_t M,
                                                                    float* __restrict__ vid) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= M) return;                                          // wave-uniform
  const int64_t b = r / F;
  const int f = (int)(r - b * F);
  const VideoSrc vs = video_src(f, F, Tv);
  const int i0 = vs.i0, i1 = vs.i1;
  const float lam = vs.lam;
  float u[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int ch = h * 256 + 4 * lane;
    const float4 a = *reinterpret_cast<const float4*>(vcat + (b * Tv + i0) * CT_N + ch);
    const float4 c = *reinterpret_cast<const float4*>(vcat + (b * Tv + i1) * CT_N + ch);
    u[4 * h + 0] = a.x * (1.f - lam) + c.x * lam;
    u[4 * h + 1] = a.y * (1.f - lam) + c.y * lam;
    u[4 * h + 2] = a.z * (1.f - lam) + c.z * lam;
    u[4 * h + 3] = a.w * (1.f - lam) + c.w * lam;
  }
  const float mu = wave_sum(((u[0] + u[1]) + (u[2] + u[3])) + ((u[4] + u[5]) + (u[6] + u[7]))) * (1.0f / CT_N);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    u[i] -= mu;
    q += u[i] * u[i];
  }
  const float rstd = rsqrtf(wave_sum(q) * (1.0f / CT_N) + 1e-5f);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int ch = h * 256 + 4 * lane;
    const float4 ga = *reinterpret_cast<const float4*>(g + ch), bb = *reinterpret_cast<const float4*>(be + ch);
    *reinterpret_cast<float4*>(vid + r * CT_N + ch) =
        make_float4(u[4 * h] * rstd * ga.x + bb.x, u[4 * h + 1] * rstd * ga.y + bb.y, u[4 * h + 2] * rstd * ga.z + bb.z,
                    u[4 * h + 3] * rstd * ga.w + bb.w);
  }
}

// the audio-only table (deepconvtasnet.py), then the audio-visual head's four tensors (deepavconvtasnet.py) if av
inline void add_deepconvtasnet_names(CtHandle* c, bool av) {
  auto add = [&](const std::string& n, int64_t numel) { c->add(n, numel); };
  const int64_t dense = (int64_t)CT_N * CT_N * 3;
  add("encoder.sequential.0.weight", (int64_t)CT_N * 2 * CT_L);
  add("encoder.sequential.0.bias", CT_N);
  for (int i = 1; i <= 7; i += 2) {
    const std::string p = "encoder.sequential.";
    add(p + std::to_string(i) + ".weight", dense);
    add(p + std::to_string(i) + ".bias", CT_N);
    add(p + std::to_string(i + 1) + ".weight", 1);
  }
  add_separator_names(c);
  for (int i = 0; i <= 6; i += 2) {
    const std::string p = "decoder.sequential.";
    add(p + std::to_string(i) + ".weight", dense);
    add(p + std::to_string(i) + ".bias", CT_N);
    add(p + std::to_string(i + 1) + ".weight", 1);
  }
  add("decoder.sequential.8.weight", (int64_t)CT_N * 2 * CT_L);
  add("decoder.sequential.8.bias", 1);
  add("decoder.deconv.weight", (int64_t)CT_N * 2 * CT_L);
  if (av) {
    add("visual_compression.weight", (int64_t)DC_HV * CT_N);
    add("visual_compression.bias", DC_HV);
    add("video_ln.weight", CT_N);
    add("video_ln.bias", CT_N);
  }
}

// multiply-accumulates per frame of the audio path (*_flops_per_mixture): first conv, 4 dense encoder layers, Separator,
// 4 dense decoder layers on two speakers, output head on two speakers
inline double deepconvtasnet_macs() {
  const double dense = 3.0 * CT_N * CT_N;
  return (double)CT_N * 2 * CT_L + 4.0 * dense + separator_macs() + 2.0 * 4.0 * dense + 2.0 * CT_N * 2 * CT_L;
}

// one dense k = 3 conv: three passes of the engine on the fragment-order taps wpk[3][512 * 512].  TAPE: x holds
// pre-activations when xslope is not null (PReLU on load); y gets z and act (or null) PReLU(z).
template <bool TAPE, class Ctx>
int launch_dense(Ctx* c, hipStream_t st, const float* wpk, bool transposed, int dil, const float* x, const float* xslope,
                 float* y, float* act, int64_t rows, int F, int lg, const float* bias, const float* slope, const float* vid,
                 float2* part) {
  for (int k = 0; k < 3; ++k) {
    const int shift = transposed ? (1 - k) * dil : (k - 1) * dil;
    const EpiTapConvT<TAPE> ep{y, act, bias, slope, k == 2 ? vid : nullptr, k == 2 ? part : nullptr, rows, k};
    if constexpr (TAPE) {
      if (xslope != nullptr) {
        if (int rc = launch_gemm<CT_N>(c, st, "dctasnet dense conv", wpk + k * DC_TAP_FLOATS, nullptr, rows, CT_N / 128,
                                       ALoadTapShiftT<true>{x, xslope, (int)rows, F, lg, shift}, ep, 0))
          return rc;
        continue;
      }
    }
    if (int rc = launch_gemm<CT_N>(c, st, "dctasnet dense conv", wpk + k * DC_TAP_FLOATS, nullptr, rows, CT_N / 128,
                                   ALoadTapShiftT<false>{x, nullptr, (int)rows, F, lg, shift}, ep, 0))
      return rc;
  }
  return CTASNET_OK;
}

}  // namespace
