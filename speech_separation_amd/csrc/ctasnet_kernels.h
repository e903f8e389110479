// ctasnet_kernels.h -- the Conv-TasNet kernels, engine hooks and launch helpers that ctasnet.hip (ConvTasNet) and
// deepctasnet.hip (DeepConvTasNet / DeepAVConvTasNet) share: the encoder Conv1d(1, 512, 32, stride 16), the per-mixture
// statistics, the 24-block separator (src/model/convtasnet.py:18-83, used unchanged by the deep variants), the mask GEMM and
// the decoder's taps.  Everything sits in an anonymous namespace, so each including unit compiles its own copy.
// ctasnet_train.hip runs the same separator with TAPE = true: every block writes into its own slice of a tape and two
// pre-activations are stored instead of the post-PReLU tensors (v1 = conv1d(x) + b instead of c = PReLU_1(v1), u =
// dconv(...) + b instead of w = PReLU_2(u)); their consumers apply the PReLU while they load, with the same float
// operations, so the predictions are bitwise those of the inference mode.
//
// Layout: frame-major, channel-last [row = b*F + f][channel], so every 1x1 conv is a row GEMM with M = B*F on the
// weights-stationary engine (gemm_ws.h) and the depthwise conv reads rows f +- dil coalesced along channels.
// Global / group norms need statistics of a whole mixture, so they sit on launch boundaries: the kernel that produces a
// tensor also writes per-row partial statistics (sum and centred sum of squares of a fixed group of columns), and
// ctasnet_stats_kernel reduces one mixture's partials in a fixed order into (mean, 1/sqrt(var + eps)), with
// var = (sum_i M2_i + sum_i n (m_i - mean)^2) / count -- never E[x^2] - E[x]^2.  Per block (convtasnet.py:46-53):
//   (a) GEMM 128->512, epilogue: bias, PReLU_1, store c, row partials          ctasnet gemm (4 column groups)
//       stats(c)                                                              ctasnet_stats_kernel
//   (b) norm_1 on the fly, dilated depthwise conv (zero padding of the NORMALISED signal), PReLU_2, store w, partials
//       stats(w)                                                              ctasnet_stats_kernel
//   (c) GEMM 512->256 (conv | conv_sc via the engine's second weight tensor), prologue norm_2, epilogue x += res,
//       skip += sc in place
// Every reduction runs in a fixed order and no atomics are used (the engine runs with its static tile schedule), so a
// forward is bitwise reproducible and a mixture's result does not depend on the rest of the batch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>

#include "../../include/ctasnet.h"
#include "common.h"
#include "gemm_ws.h"
#include "handle.h"

namespace {

constexpr int CT_N = 512, CT_B = 128, CT_H = 512, CT_X = 8, CT_P = 3, CT_R = 3, CT_L = 16;
constexpr int CT_BLOCKS = CT_P * CT_X;
constexpr int CT_BLOCK_W = 14;                             // tensors per Conv1D_Block in the state_dict
constexpr int CT_SEP_W = 4 + CT_BLOCKS * CT_BLOCK_W + 3;   // tensors of the Separator (norm_1.gamma .. seq.1.bias)
constexpr int CT_BM = 32;                         // GEMM row tile (engine shape <KIN, 1, 1, 4>: 32 rows x 128 columns)

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
DEV float prelu(float v, float a) { return v >= 0.f ? v : a * v; }

// sum over the 64 lanes of a wave, identical in every lane (xor butterfly: both partners add the same two numbers)
DEV float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// partial statistics of 4 values per lane over a wave (n = 256): (sum, sum of squares about the wave's mean)
DEV float2 wave_partial(float4 v) {
  const float s = wave_sum((v.x + v.y) + (v.z + v.w));
  const float mu = s * (1.0f / 256.0f);
  const float dx = v.x - mu, dy = v.y - mu, dz = v.z - mu, dw = v.w - mu;
  return make_float2(s, wave_sum((dx * dx + dy * dy) + (dz * dz + dw * dw)));
}

// ------------------------------------------------------------------------------------------------
// encoder: enc[b*F + f][n] = sum_k W[n][k] xpad[16 f + k], xpad = mix padded by (16, 32) (convtasnet.py:12-15)
// 256 threads = 4 waves; wave w: row slot w >> 1, channels 256 (w & 1) + 4 lane .. +3; rows of the workgroup strided by 2.
// Row partials: (sum, M2) per half row (n = 256), part[row][2].
// DEEP (deepconvtasnet.py:12): the first conv of the deep encoder has a bias and feeds another conv, so it starts from
// the bias and writes no partials (benc is read, part is not).
// ------------------------------------------------------------------------------------------------
constexpr int CT_ROWS_PER_WG = 8;

template <bool DEEP>
__global__ __launch_bounds__(256) void ctasnet_encoder_kernel(const float* __restrict__ mix, int64_t T, int F, int64_t M,
                                                              const float* __restrict__ Wenc, const float* __restrict__ benc,
                                                              float* __restrict__ enc, float2* __restrict__ part) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = wave & 1, rsub = wave >> 1;
  const int ch = half * 256 + 4 * lane;
  float w[4][2 * CT_L];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k4 = 0; k4 < 2 * CT_L / 4; ++k4) {
      const float4 v = *reinterpret_cast<const float4*>(Wenc + (int64_t)(ch + j) * (2 * CT_L) + 4 * k4);
      w[j][4 * k4] = v.x; w[j][4 * k4 + 1] = v.y; w[j][4 * k4 + 2] = v.z; w[j][4 * k4 + 3] = v.w;
    }
  float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (DEEP) acc0 = *reinterpret_cast<const float4*>(benc + ch);
  for (int i = 0; i < CT_ROWS_PER_WG / 2; ++i) {
    const int64_t r = (int64_t)blockIdx.x * CT_ROWS_PER_WG + 2 * i + rsub;
    if (r >= M) break;                              // wave-uniform
    const int64_t b = r / F, f = r - b * F;
    const float* x = mix + b * T;
    float4 acc = acc0;
#pragma unroll
    for (int k = 0; k < 2 * CT_L; ++k) {
      const int64_t j = CT_L * f + k - CT_L;        // sample index in the unpadded mixture
      const float xv = (j >= 0 && j < T) ? x[j] : 0.f;
      acc.x = fmaf(w[0][k], xv, acc.x);
      acc.y = fmaf(w[1][k], xv, acc.y);
      acc.z = fmaf(w[2][k], xv, acc.z);
      acc.w = fmaf(w[3][k], xv, acc.w);
    }
    *reinterpret_cast<float4*>(enc + r * CT_N + ch) = acc;
    if constexpr (!DEEP) {
      const float2 p = wave_partial(acc);
      if (lane == 0) part[r * 2 + half] = p;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// per-mixture statistics from row partials: part[(b*F + f) * P + j] = (sum, M2) of n_part values.
// One workgroup per mixture; thread t takes entries t, t + 256, ... (fixed), then a fixed LDS tree.
// stats[b] = (mean, 1 / sqrt(var + eps)).
// ------------------------------------------------------------------------------------------------
DEV float block_sum256(float v, float* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void ctasnet_stats_kernel(const float2* __restrict__ part, int F, int P, float n_part,
                                                            float eps, float2* __restrict__ stats) {
  __shared__ float red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t n = (int64_t)F * P;
  const float2* pb = part + (int64_t)b * n;
  float s = 0.f;
  for (int64_t i = tid; i < n; i += 256) s += pb[i].x;
  const float count = (float)n * n_part;
  const float mean = block_sum256(s, red) / count;
  float q = 0.f;
  for (int64_t i = tid; i < n; i += 256) {
    const float2 v = pb[i];
    const float d = v.x / n_part - mean;
    q += v.y + n_part * d * d;
  }
  const float var = block_sum256(q, red) / count;
  if (tid == 0) stats[b] = make_float2(mean, 1.0f / sqrtf(var + eps));
}

// ------------------------------------------------------------------------------------------------
// (b) depthwise dilated conv of the normalised c (convtasnet.py:49-51): w = PReLU_2(dconv(norm_1(c)))
// Same thread map as the encoder; the zero padding applies to norm_1(c), so out-of-range taps contribute nothing.
// TAPE: c holds v1 (PReLU_1 with slope1 on load; slope1 is not read otherwise) and w gets u, the pre-activation of PReLU_2.
// ------------------------------------------------------------------------------------------------
template <bool TAPE>
__global__ __launch_bounds__(256) void ctasnet_dconv_kernel(const float* __restrict__ c, const float* __restrict__ slope1,
                                                            const float2* __restrict__ stats, const float* __restrict__ g1,
                                                            const float* __restrict__ b1, const float* __restrict__ wd,
                                                            const float* __restrict__ bd, const float* __restrict__ slope2,
                                                            int dil, int F, int64_t M, float* __restrict__ w,
                                                            float2* __restrict__ part) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = wave & 1, rsub = wave >> 1;
  const int ch = half * 256 + 4 * lane;
  const float4 ga = *reinterpret_cast<const float4*>(g1 + ch), be = *reinterpret_cast<const float4*>(b1 + ch);
  const float4 bias = *reinterpret_cast<const float4*>(bd + ch);
  float tap[4][CT_R];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < CT_R; ++k) tap[j][k] = wd[(ch + j) * CT_R + k];
  const float a1 = TAPE ? *slope1 : 0.f, a2 = *slope2;
  for (int i = 0; i < CT_ROWS_PER_WG / 2; ++i) {
    const int64_t r = (int64_t)blockIdx.x * CT_ROWS_PER_WG + 2 * i + rsub;
    if (r >= M) break;                              // wave-uniform
    const int64_t b = r / F, f = r - b * F;
    const float2 st = stats[b];
    float4 acc = bias;
#pragma unroll
    for (int k = 0; k < CT_R; ++k) {
      const int64_t fk = f + (int64_t)(k - 1) * dil;
      if (fk < 0 || fk >= F) continue;              // wave-uniform
      float4 v = *reinterpret_cast<const float4*>(c + (b * F + fk) * CT_H + ch);
      if constexpr (TAPE) v = make_float4(prelu(v.x, a1), prelu(v.y, a1), prelu(v.z, a1), prelu(v.w, a1));
      acc.x = fmaf(tap[0][k], (v.x - st.x) * st.y * ga.x + be.x, acc.x);
      acc.y = fmaf(tap[1][k], (v.y - st.x) * st.y * ga.y + be.y, acc.y);
      acc.z = fmaf(tap[2][k], (v.z - st.x) * st.y * ga.z + be.z, acc.z);
      acc.w = fmaf(tap[3][k], (v.w - st.x) * st.y * ga.w + be.w, acc.w);
    }
    if constexpr (TAPE) *reinterpret_cast<float4*>(w + r * CT_H + ch) = acc;
    acc = make_float4(prelu(acc.x, a2), prelu(acc.y, a2), prelu(acc.z, a2), prelu(acc.w, a2));
    if constexpr (!TAPE) *reinterpret_cast<float4*>(w + r * CT_H + ch) = acc;
    const float2 p = wave_partial(acc);
    if (lane == 0) part[r * 2 + half] = p;
  }
}

// ------------------------------------------------------------------------------------------------
// GEMM engine hooks
// ------------------------------------------------------------------------------------------------
// A rows normalised on the fly with their mixture's statistics: gamma[k] (a - mean) rstd + beta[k]
// (GlobalNorm convtasnet.py:25-29 in front of the bottleneck conv; norm_2 in front of conv / conv_sc)
// PRE: a = PReLU(A row) with *slope first (the tape holds u, not w); slope is not read otherwise
template <bool PRE>
struct ALoadNormRows {
  const float* A;
  const float* slope;
  const float2* stats;
  const float* gamma;
  const float* beta;
  int64_t M;
  int F;
  int lda;
  DEV float4 load4(int tile, int row, int k4) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    if (r >= M) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float2 st = stats[r / F];
    float4 v = *reinterpret_cast<const float4*>(A + r * lda + 4 * k4);
    if constexpr (PRE) {
      const float a = *slope;
      v = make_float4(prelu(v.x, a), prelu(v.y, a), prelu(v.z, a), prelu(v.w, a));
    }
    const float4 g = *reinterpret_cast<const float4*>(gamma + 4 * k4), bb = *reinterpret_cast<const float4*>(beta + 4 * k4);
    return make_float4((v.x - st.x) * st.y * g.x + bb.x, (v.y - st.x) * st.y * g.y + bb.y,
                       (v.z - st.x) * st.y * g.z + bb.z, (v.w - st.x) * st.y * g.w + bb.w);
  }
};

// (a) c = PReLU_1(v + bias) -> out[row][128 colgroup + 4 c4 ..]; row partials (n = 128) -> part[row][colgroup]
// TAPE: out gets v1 = v + bias (PReLU_1 is applied by the consumers); the partials are those of PReLU_1(v1) either way
template <bool TAPE>
struct EpiPReLUStats {
  static constexpr bool DIRECT = false;
  static constexpr bool HAS_FINISH = false;
  float* out;
  float2* part;
  const float* bias;
  const float* slope;
  int64_t M;
  struct Cols { float4 b; float a; };
  DEV Cols cols(int colgroup, int c4) const {
    return Cols{*reinterpret_cast<const float4*>(bias + colgroup * 128 + 4 * c4), *slope};
  }
  DEV float4 prefetch(int, int, int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
  DEV void row(int tile, int row, int colgroup, int c4, float4 v, float4, const Cols& k) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    const float4 pre = make_float4(v.x + k.b.x, v.y + k.b.y, v.z + k.b.z, v.w + k.b.w);
    v = make_float4(prelu(pre.x, k.a), prelu(pre.y, k.a), prelu(pre.z, k.a), prelu(pre.w, k.a));
    const float s = group_sum<32>((v.x + v.y) + (v.z + v.w));
    const float mu = s * (1.0f / 128.0f);
    const float dx = v.x - mu, dy = v.y - mu, dz = v.z - mu, dw = v.w - mu;
    const float q = group_sum<32>((dx * dx + dy * dy) + (dz * dz + dw * dw));
    if (r >= M) return;
    *reinterpret_cast<float4*>(out + r * CT_H + colgroup * 128 + 4 * c4) = TAPE ? pre : v;
    if (c4 == 0) part[r * 4 + colgroup] = make_float2(s, q);
  }
};

// (c) colgroup 0: x += conv(w) + bias (residual); colgroup 1: skip (+)= conv_sc(w) + bias_sc (convtasnet.py:71-74)
struct EpiResSkip {
  static constexpr bool DIRECT = false;
  static constexpr bool HAS_FINISH = false;
  float* x;
  float* skip;
  const float* bias_res;
  const float* bias_sc;
  int64_t M;
  int first;          // first block: skip = 0.0 + score
  struct Cols { float4 b; };
  DEV Cols cols(int colgroup, int c4) const {
    return Cols{*reinterpret_cast<const float4*>((colgroup ? bias_sc : bias_res) + 4 * c4)};
  }
  DEV float4 prefetch(int, int, int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
  DEV void row(int tile, int row, int colgroup, int c4, float4 v, float4, const Cols& k) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    if (r >= M) return;
    v.x += k.b.x; v.y += k.b.y; v.z += k.b.z; v.w += k.b.w;
    float* dst = (colgroup ? skip : x) + r * CT_B + 4 * c4;
    if (colgroup == 0 || !first) {
      const float4 o = *reinterpret_cast<const float4*>(dst);
      v.x = o.x + v.x; v.y = o.y + v.y; v.z = o.z + v.z; v.w = o.w + v.w;
    }
    *reinterpret_cast<float4*>(dst) = v;
  }
};

// head (convtasnet.py:76-80): ym[row][j] = sigmoid(v + bias) * enc[row][j mod 512], j = 128 colgroup + 4 c4 ..
// TAPE: the sigmoid masks go to mk [M][1024] as well (mk is not written otherwise)
template <bool TAPE>
struct EpiMask {
  static constexpr bool DIRECT = false;
  static constexpr bool HAS_FINISH = false;
  float* ym;
  float* mk;
  const float* enc;
  const float* bias;
  int64_t M;
  struct Cols { float4 b; };
  DEV Cols cols(int colgroup, int c4) const { return Cols{*reinterpret_cast<const float4*>(bias + colgroup * 128 + 4 * c4)}; }
  DEV float4 prefetch(int, int, int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
  DEV void row(int tile, int row, int colgroup, int c4, float4 v, float4, const Cols& k) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    if (r >= M) return;
    const int j = colgroup * 128 + 4 * c4;
    const float4 e = *reinterpret_cast<const float4*>(enc + r * CT_N + (j & (CT_N - 1)));
    const float4 m = make_float4(1.0f / (1.0f + expf(-(v.x + k.b.x))), 1.0f / (1.0f + expf(-(v.y + k.b.y))),
                                 1.0f / (1.0f + expf(-(v.z + k.b.z))), 1.0f / (1.0f + expf(-(v.w + k.b.w))));
    *reinterpret_cast<float4*>(ym + r * (2 * CT_N) + j) = make_float4(e.x * m.x, e.y * m.y, e.z * m.z, e.w * m.w);
    if constexpr (TAPE) *reinterpret_cast<float4*>(mk + r * (2 * CT_N) + j) = m;
  }
};

// ------------------------------------------------------------------------------------------------
// decoder (convtasnet.py:92-97)
// taps[row][s][k] = sum_n ym[row][512 s + n] D[n][k]  (k < 32): 16 rows per workgroup, rows and D staged in LDS
// ------------------------------------------------------------------------------------------------
constexpr int CT_TAP_ROWS = 16, CT_YM_LD = 2 * CT_N + 4;
constexpr size_t CT_TAPS_LDS = sizeof(float) * (CT_N * 2 * CT_L + CT_TAP_ROWS * CT_YM_LD);

__global__ __launch_bounds__(256) void ctasnet_taps_kernel(const float* __restrict__ ym, const float* __restrict__ D,
                                                           int64_t M, float* __restrict__ taps) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Ds = lds;                                  // [512][32]
  float* Ys = lds + CT_N * 2 * CT_L;                // [16][CT_YM_LD]
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * CT_TAP_ROWS;
  for (int i = tid; i < CT_N * 2 * CT_L / 4; i += 256)
    reinterpret_cast<float4*>(Ds)[i] = reinterpret_cast<const float4*>(D)[i];
  for (int i = tid; i < CT_TAP_ROWS * (2 * CT_N / 4); i += 256) {
    const int rr = i / (2 * CT_N / 4), c4 = i % (2 * CT_N / 4);
    const int64_t r = r0 + rr < M ? r0 + rr : M - 1;    // rows beyond M: a valid copy, never stored
    *reinterpret_cast<float4*>(Ys + rr * CT_YM_LD + 4 * c4) = *reinterpret_cast<const float4*>(ym + r * (2 * CT_N) + 4 * c4);
  }
  __syncthreads();
  const int rr = tid >> 4, q = tid & 15, s = q >> 3, k0 = (q & 7) * 4;
  const float* y = Ys + rr * CT_YM_LD + s * CT_N;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int n = 0; n < CT_N; ++n) {
    const float a = y[n];
    const float4 d = *reinterpret_cast<const float4*>(Ds + n * 2 * CT_L + k0);
    acc.x = fmaf(a, d.x, acc.x); acc.y = fmaf(a, d.y, acc.y); acc.z = fmaf(a, d.z, acc.z); acc.w = fmaf(a, d.w, acc.w);
  }
  if (r0 + rr < M) *reinterpret_cast<float4*>(taps + (r0 + rr) * (4 * CT_L) + s * 2 * CT_L + k0) = acc;
}

// overlap-add and crop: out_s[b][t] = taps[b F + f][s][k] + taps[b F + f - 1][s][k + 16], t + 16 = 16 f + k
// BIAS: + *bias, the deep decoder's output bias (deepconvtasnet.py:110, :116-118); bias is not read otherwise
template <bool BIAS>
__global__ __launch_bounds__(256) void ctasnet_overlap_add_kernel(const float* __restrict__ taps, const float* __restrict__ bias,
                                                                  int B, int F, int64_t Lout, float* __restrict__ s1,
                                                                  float* __restrict__ s2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * (int64_t)B * Lout) return;
  const int64_t bs = i / Lout, t = i - bs * Lout;
  const int64_t b = bs >> 1;
  const int s = (int)(bs & 1);
  const int64_t j = t + CT_L, f = j / CT_L, k = j - f * CT_L;
  const float* tp = taps + (b * F + f) * (4 * CT_L) + s * 2 * CT_L;
  const float v = tp[k] + tp[k + CT_L - 4 * CT_L];   // previous frame's taps k + 16
  (s ? s2 : s1)[b * Lout + t] = BIAS ? v + *bias : v;
}

// ------------------------------------------------------------------------------------------------
// host side: launch helpers for a handle type with fail(code, fmt, ...), device_id and num_cus
// ------------------------------------------------------------------------------------------------
template <class Ctx, class Kern>
int set_lds(Ctx* c, Kern kern, size_t bytes, const char* what) {
  if (bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return c->fail(CTASNET_ERR_HIP, "%s: set LDS %zu: %s", what, bytes, hipGetErrorString(e));
  }
  return CTASNET_OK;
}

// The engine with its static tile schedule (no ticket queue): workgroup g takes tiles g, g + grid, ...  The grid is what
// is co-resident (occupancy query once per instantiation and device, at most two workgroups per CU).
// ldw: row stride of W, or 0 for a copy in the engine's fragment order (gemm_ws.h).
// WT: the engine in its transposed-weight form, out[m][j] = sum_k A[m][k] W[k][j] with W row-major [KIN][ldw].
template <int KIN, bool WT = false, class Ctx, class AL, class EP>
int launch_gemm(Ctx* c, hipStream_t st, const char* what, const float* W, const float* Walt, int64_t M, int colgroups,
                const AL& al, const EP& ep, int ldw = KIN) {
  auto kern = gemm_ws_kernel<KIN, 1, 1, 4, AL, EP, WT>;
  const size_t lds = GemmShape<KIN, 1, 1, 4>::lds_bytes(EP::DIRECT);
  static std::atomic<int> resident_dev[64];
  int resident = resident_dev[c->device_id & 63].load(std::memory_order_acquire);
  if (resident == 0) {
    if (int rc = set_lds(c, kern, lds, what)) return rc;
    int per_cu = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds);
    if (e != hipSuccess || per_cu < 1) return c->fail(CTASNET_ERR_HIP, "%s: occupancy query: %s", what, hipGetErrorString(e));
    resident = std::min(per_cu, 2) * c->num_cus;
    resident_dev[c->device_id & 63].store(resident, std::memory_order_release);
  }
  const int64_t ntiles = (M + CT_BM - 1) / CT_BM;
  int gx = resident / colgroups;
  if (gx < 1) gx = 1;
  if (ntiles < gx) gx = (int)ntiles;
  hipLaunchKernelGGL(kern, dim3(gx, colgroups), dim3(256), lds, st, W, Walt, ldw, (int)ntiles, nullptr, al, ep, NoRider{});
  HANDLE_LAUNCH_CHECK(c, what);
  return CTASNET_OK;
}

template <class Ctx>
int launch_stats(Ctx* c, hipStream_t st, const float2* part, int B, int F, int P, float n_part, float eps, float2* stats) {
  hipLaunchKernelGGL(ctasnet_stats_kernel, dim3(B), dim3(256), 0, st, part, F, P, n_part, eps, stats);
  HANDLE_LAUNCH_CHECK(c, "ctasnet stats");
  return CTASNET_OK;
}

template <class Ctx>
int launch_taps(Ctx* c, hipStream_t st, const float* ym, const float* D, int64_t M, float* taps) {
  static PerDeviceOnce ready;
  if (!ready.done(c->device_id)) {
    if (int rc = set_lds(c, ctasnet_taps_kernel, CT_TAPS_LDS, "ctasnet taps")) return rc;
    ready.set(c->device_id);
  }
  hipLaunchKernelGGL(ctasnet_taps_kernel, dim3((unsigned)((M + CT_TAP_ROWS - 1) / CT_TAP_ROWS)), dim3(256), CT_TAPS_LDS, st, ym,
                     D, M, taps);
  HANDLE_LAUNCH_CHECK(c, "ctasnet taps");
  return CTASNET_OK;
}

template <bool BIAS, class Ctx>
int launch_overlap_add(Ctx* c, hipStream_t st, const float* taps, const float* bias, int B, int F, int64_t Lout, float* s1,
                       float* s2) {
  const int64_t n_out = 2 * (int64_t)B * Lout;
  hipLaunchKernelGGL(ctasnet_overlap_add_kernel<BIAS>, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, taps, bias, B, F,
                     Lout, s1, s2);
  HANDLE_LAUNCH_CHECK(c, "ctasnet overlap-add");
  return CTASNET_OK;
}

// The Separator (convtasnet.py:55-83) on the encoder output `enc` [M][512], whose row partials (P per row of n_part values
// each) are in s.part: GlobalNorm statistics, bottleneck 1x1, 24 blocks, masks.
// sw: the Separator's CT_SEP_W weights in state_dict order (separator.norm_1.gamma first).
// Without a tape every block reuses the same buffers and ym may lie over c and w (contiguous).  TAPE: block i works on
// slice i of x, c (v1), w (u), stats1 and stats2, and x_{i+1} = x_i + res is formed in a copy, so x_i stays.
struct SepBuffers {
  float* x;        // [M][128]; TAPE: CT_BLOCKS + 1 of them
  float* skip;     // [M][128]
  float* c;        // [M][512]; TAPE: CT_BLOCKS of them (v1)
  float* w;        // [M][512]; TAPE: CT_BLOCKS of them (u)
  float2* part;    // [M][4]
  float2* stats0;  // [B] GlobalNorm statistics (may be stats1 without a tape)
  float2* stats1;  // [B]; TAPE: CT_BLOCKS of them
  float2* stats2;  // [B]; TAPE: CT_BLOCKS of them
  float* ym;       // [M][1024] = enc * masks
  float* mk;       // TAPE: [M][1024] sigmoid masks
};

template <bool TAPE, class Ctx>
int launch_separator(Ctx* c, hipStream_t st, const float* const* sw, const float* enc, int P, float n_part, int B, int F,
                     int64_t M, const SepBuffers& s) {
  const unsigned row_wgs = (unsigned)((M + CT_ROWS_PER_WG - 1) / CT_ROWS_PER_WG);
  // GlobalNorm statistics + bottleneck 1x1 (convtasnet.py:25-29, :67-68)
  if (int rc = launch_stats(c, st, s.part, B, F, P, n_part, 5e-6f, s.stats0)) return rc;
  if (int rc = launch_gemm<CT_N>(c, st, "ctasnet bottleneck gemm", sw[2], nullptr, M, 1,
                                 ALoadNormRows<false>{enc, nullptr, s.stats0, sw[0], sw[1], M, F, CT_N},
                                 EpiBiasStore{s.x, sw[3], M, CT_B, CT_BM, 128}))
    return rc;

  for (int i = 0; i < CT_BLOCKS; ++i) {       // Conv1D_Block i (convtasnet.py:46-53), dilation 2^(i mod 8)
    const float* const* bw = sw + 4 + i * CT_BLOCK_W;
    const int dil = 1 << (i % CT_X);
    const size_t slice = TAPE ? (size_t)i : 0;
    float* xi = s.x + slice * M * CT_B;
    float* ci = s.c + slice * M * CT_H;
    float* wi = s.w + slice * M * CT_H;
    float2* st1 = s.stats1 + slice * B;
    float2* st2 = s.stats2 + slice * B;
    if (int rc = launch_gemm<CT_B>(c, st, "ctasnet block 1x1 gemm", bw[0], nullptr, M, CT_H / 128,
                                   ALoadDense{xi, M, CT_B, CT_BM}, EpiPReLUStats<TAPE>{ci, s.part, bw[1], bw[2], M}))
      return rc;
    if (int rc = launch_stats(c, st, s.part, B, F, 4, 128.0f, 1e-10f, st1)) return rc;
    hipLaunchKernelGGL(ctasnet_dconv_kernel<TAPE>, dim3(row_wgs), dim3(256), 0, st, ci, bw[2], st1, bw[3], bw[4], bw[5], bw[6],
                       bw[7], dil, F, M, wi, s.part);
    HANDLE_LAUNCH_CHECK(c, "ctasnet dconv");
    if (int rc = launch_stats(c, st, s.part, B, F, 2, 256.0f, 1e-10f, st2)) return rc;
    float* xn = xi;                           // the residual is added in place ...
    if constexpr (TAPE) {                     // ... into a copy, so x_i stays on the tape
      xn = xi + (size_t)M * CT_B;
      if (hipMemcpyAsync(xn, xi, (size_t)M * CT_B * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return c->fail(CTASNET_ERR_HIP, "ctasnet: residual copy failed");
    }
    if (int rc = launch_gemm<CT_H>(c, st, "ctasnet block res|skip gemm", bw[10], bw[12], M, 2,
                                   ALoadNormRows<TAPE>{wi, bw[7], st2, bw[8], bw[9], M, F, CT_H},
                                   EpiResSkip{xn, s.skip, bw[11], bw[13], M, i == 0}))
      return rc;
  }

  // masks (convtasnet.py:76-81)
  const float* const* hw = sw + 4 + CT_BLOCKS * CT_BLOCK_W;
  return launch_gemm<CT_B>(c, st, "ctasnet mask gemm", hw[1], nullptr, M, 2 * CT_N / 128,
                           ALoadDensePReLU{s.skip, hw[0], M, CT_B, CT_BM}, EpiMask<TAPE>{s.ym, s.mk, enc, hw[2], M});
}

}  // namespace
