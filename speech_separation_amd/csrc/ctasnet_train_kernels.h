// ctasnet_train_kernels.h -- what the Conv-TasNet training units share (ctasnet_train.hip: TrainableConvTasNet,
// deepctasnet_train.hip: TrainableDeepConvTasNet): the backward kernels of the Separator and of the mask head, the engine
// hooks of the weight / data gradients, the slab launch helpers, the Separator's part of the workspace plan,
// launch_separator_backward -- the counterpart of launch_separator (ctasnet_kernels.h), which serves the forwards -- and
// the training handle with the bodies of the entry points that do not depend on the model (CtTrainHandle, at the end).
// Everything sits in an anonymous namespace, so each including unit compiles its own copy.
//
// Data gradients run on the weights-stationary engine in its transposed-weight form (gemm_ws.h, WT = true: the forward
// weights are read as they are at launch, nothing is cached); the res|skip weights are gathered into one [256][512]
// operand inside each step.  Weight gradients are wgrad_generic_kernel (backward.h) partial tiles per workgroup; bias
// gradients colsum_kernel partials; the norms' and PReLUs' parameter gradients per-workgroup partials of the row kernels
// below.  Every partial is summed by cttrain_reduce_kernel in slab order: no atomics, fixed grids, so repeated backward
// calls are bitwise identical.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "backward.h"
#include "train_tail.h"
#include "ctasnet_handle.h"

namespace {

constexpr int CTT_G_ROW = 512;   // workgroups of the row kernels (grid-stride): fixed, so partials are summed in a fixed order
constexpr int CTT_G_W = 128;     // workgroups of a weight-gradient launch (at most)
constexpr int CTT_G_C = 256;     // workgroups of a column-sum launch
constexpr int CTT_ROW_SLAB = 6 * CT_H;   // per-workgroup column partials of the dconv backward (3 taps, bias, gamma, beta)

// ------------------------------------------------------------------------------------------------
// backward kernels
// ------------------------------------------------------------------------------------------------
// decoder: every tap (f, s, k) of the transposed conv lands on sample t = 16 f + k - 16 of the cropped output, so
// dtaps[b F + f][s][k] = d_out_s[b][16 f + k - 16] where 0 <= t < Lout, else 0
__global__ __launch_bounds__(256) void cttrain_dtaps_kernel(const float* __restrict__ d1, const float* __restrict__ d2, int F,
                                                            int64_t M, int64_t Lout, float* __restrict__ dtaps) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * 4 * CT_L) return;
  const int64_t r = i / (4 * CT_L);
  const int q = (int)(i - r * 4 * CT_L), s = q / (2 * CT_L), k = q % (2 * CT_L);
  const int64_t b = r / F, f = r - b * F;
  const int64_t t = CT_L * f + k - CT_L;
  dtaps[i] = (t >= 0 && t < Lout) ? (s ? d2 : d1)[b * Lout + t] : 0.f;
}

// mask head: dv = dym enc m (1 - m);  d enc = sum_s dym_s m_s (the head's contribution; the GlobalNorm one is added
// later), with dym [M][1024] the gradient of the masked tensor ym.  One text, three forms:
//   HEAD_TAPS  (Conv-TasNet)  dym[r][512 s + n] = sum_k dtaps[r][s][k] D[n][k] formed here from the decoder's taps gradient
//   HEAD_DYM   (deep)         dym = `in`, already computed (the deep decoder's data gradient); D and the LDS are not used
//   HEAD_DYM_OUT (deep)       only the product of HEAD_TAPS, stored to dv [M][1024]: the gradient of the deep decoder's last
//                             activation from its output head's taps gradient; mk, enc, denc are not used
// Grid-stride over rows; thread = channels n, n + 256.
enum HeadForm { HEAD_TAPS = 0, HEAD_DYM = 1, HEAD_DYM_OUT = 2 };
constexpr size_t CTT_HEAD_LDS = sizeof(float) * (CT_N * 2 * CT_L + 4 * CT_L);
template <int FORM>
__global__ __launch_bounds__(256) void cttrain_head_bwd_kernel(const float* __restrict__ in, const float* __restrict__ D,
                                                               const float* __restrict__ mk, const float* __restrict__ enc,
                                                               int64_t M, float* __restrict__ dv, float* __restrict__ denc) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Ds = lds;                       // [512][32]
  float* ts = lds + CT_N * 2 * CT_L;     // [64]
  const int tid = threadIdx.x;
  if constexpr (FORM != HEAD_DYM)
    for (int i = tid; i < CT_N * 2 * CT_L / 4; i += 256)
      reinterpret_cast<float4*>(Ds)[i] = reinterpret_cast<const float4*>(D)[i];
  for (int64_t r = blockIdx.x; r < M; r += gridDim.x) {
    if constexpr (FORM != HEAD_DYM) {
      __syncthreads();
      if (tid < 4 * CT_L) ts[tid] = in[r * 4 * CT_L + tid];
      __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int n = tid + 256 * h;
      float y0 = 0.f, y1 = 0.f;
      if constexpr (FORM == HEAD_DYM) {
        y0 = in[r * 2 * CT_N + n];
        y1 = in[r * 2 * CT_N + CT_N + n];
      } else {
#pragma unroll
        for (int k = 0; k < 2 * CT_L; ++k) {
          const float d = Ds[n * 2 * CT_L + k];
          y0 = fmaf(ts[k], d, y0);
          y1 = fmaf(ts[2 * CT_L + k], d, y1);
        }
      }
      if constexpr (FORM == HEAD_DYM_OUT) {
        dv[r * 2 * CT_N + n] = y0;
        dv[r * 2 * CT_N + CT_N + n] = y1;
      } else {
        const float e = enc[r * CT_N + n];
        const float m0 = mk[r * 2 * CT_N + n], m1 = mk[r * 2 * CT_N + CT_N + n];
        dv[r * 2 * CT_N + n] = y0 * e * (m0 * (1.f - m0));
        dv[r * 2 * CT_N + CT_N + n] = y1 * e * (m1 * (1.f - m1));
        denc[r * CT_N + n] = y0 * m0 + y1 * m1;
      }
    }
  }
}

// PReLU backward in place over [M][128]: g = g * (x > 0 ? 1 : a); partial d a = sum g x (x <= 0) per workgroup -> aslab
__global__ __launch_bounds__(256) void cttrain_prelu_bwd_kernel(float* __restrict__ g, const float* __restrict__ x,
                                                                const float* __restrict__ slope, int64_t n,
                                                                float* __restrict__ aslab) {
  __shared__ float red[256];
  const float a = *slope;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float xv = x[i], gv = g[i];
    if (xv > 0.f) continue;
    s += gv * xv;
    g[i] = a * gv;
  }
  const float t = block_sum256(s, red);
  if (threadIdx.x == 0) aslab[blockIdx.x] = t;
}

// Row kernels share the thread map of ctasnet_dconv_kernel (wave: half = channels 256 half + 4 lane .. +3, rsub = row of a
// pair) over a grid-stride loop of row pairs.  Column partials: rsub 0 and 1 combined in that order per workgroup.
DEV void colpart_store(float4 v, float* red4, float* dst, int tid) {
  // red4: 256 float4 of LDS; dst: the workgroup's 512 floats
  reinterpret_cast<float4*>(red4)[tid] = v;
  __syncthreads();
  if (tid < 128) {
    const float4 a = reinterpret_cast<float4*>(red4)[tid], b = reinterpret_cast<float4*>(red4)[tid + 128];
    // tid < 128: waves 0, 1 (rsub 0); tid + 128: waves 2, 3 (rsub 1), same channels
    reinterpret_cast<float4*>(dst)[tid] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
  __syncthreads();
}

// norm backward, pass 1: g = dn gamma, xhat = (X - mean) rstd (X = PReLU(src) if PRE else src); row partials
// (sum g, sum g xhat) -> part[r][half]; column partials (sum dn xhat | sum dn) -> colslab[wg][1024]
template <bool PRE>
__global__ __launch_bounds__(256) void cttrain_normstat_kernel(const float* __restrict__ dn, const float* __restrict__ src,
                                                               const float* __restrict__ slope, const float2* __restrict__ stats,
                                                               const float* __restrict__ gamma, int F, int64_t M,
                                                               float2* __restrict__ part, float* __restrict__ colslab) {
  __shared__ float4 red4[256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = wave & 1, rsub = wave >> 1;
  const int ch = half * 256 + 4 * lane;
  const float4 ga = *reinterpret_cast<const float4*>(gamma + ch);
  const float a = PRE ? *slope : 0.f;
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sb = sg;
  for (int64_t rp = blockIdx.x; 2 * rp < M; rp += gridDim.x) {
    const int64_t r = 2 * rp + rsub;
    if (r >= M) continue;                            // wave-uniform
    const float2 st = stats[r / F];
    float4 x = *reinterpret_cast<const float4*>(src + r * CT_H + ch);
    if (PRE) x = make_float4(prelu(x.x, a), prelu(x.y, a), prelu(x.z, a), prelu(x.w, a));
    const float4 d = *reinterpret_cast<const float4*>(dn + r * CT_H + ch);
    const float4 xh = make_float4((x.x - st.x) * st.y, (x.y - st.x) * st.y, (x.z - st.x) * st.y, (x.w - st.x) * st.y);
    const float4 g = make_float4(d.x * ga.x, d.y * ga.y, d.z * ga.z, d.w * ga.w);
    const float s1 = wave_sum((g.x + g.y) + (g.z + g.w));
    const float s2 = wave_sum((g.x * xh.x + g.y * xh.y) + (g.z * xh.z + g.w * xh.w));
    if (lane == 0) part[r * 2 + half] = make_float2(s1, s2);
    sg.x += d.x * xh.x; sg.y += d.y * xh.y; sg.z += d.z * xh.z; sg.w += d.w * xh.w;
    sb.x += d.x; sb.y += d.y; sb.z += d.z; sb.w += d.w;
  }
  float* dst = colslab + (size_t)blockIdx.x * 2 * CT_H;
  // column partials: thread (half, lane) owns channels ch; store order [rsub][half][lane] -> channel-major per rsub
  colpart_store(sg, reinterpret_cast<float*>(red4), dst, tid);
  colpart_store(sb, reinterpret_cast<float*>(red4), dst + CT_H, tid);
}

// per-mixture sums of row partials part[(b F + f) * 2 + j] in a fixed order -> S[b]
__global__ __launch_bounds__(256) void cttrain_mixsum_kernel(const float2* __restrict__ part, int F, float2* __restrict__ S) {
  __shared__ float red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t n = (int64_t)F * 2;
  const float2* pb = part + (int64_t)b * n;
  float s1 = 0.f, s2 = 0.f;
  for (int64_t i = tid; i < n; i += 256) { s1 += pb[i].x; s2 += pb[i].y; }
  const float t1 = block_sum256(s1, red);
  const float t2 = block_sum256(s2, red);
  if (tid == 0) S[b] = make_float2(t1, t2);
}

// norm backward, pass 2: dX = rstd (g - S1 / N - xhat S2 / N), N = F * 512.
// PRE: X = PReLU(src) and the result continues through the PReLU: dn <- dX (src > 0 ? 1 : a), partial d a = sum dX src
//      (src <= 0) per workgroup -> aslab[wg].   !PRE: out += dX.
template <bool PRE>
__global__ __launch_bounds__(256) void cttrain_normapply_kernel(float* __restrict__ dn, const float* __restrict__ src,
                                                                const float* __restrict__ slope,
                                                                const float2* __restrict__ stats, const float* __restrict__ gamma,
                                                                const float2* __restrict__ S, int F, int64_t M,
                                                                float* __restrict__ out, float* __restrict__ aslab) {
  __shared__ float red[256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = wave & 1, rsub = wave >> 1;
  const int ch = half * 256 + 4 * lane;
  const float4 ga = *reinterpret_cast<const float4*>(gamma + ch);
  const float a = PRE ? *slope : 0.f;
  const float invN = 1.0f / ((float)F * (float)CT_H);
  float sa = 0.f;
  for (int64_t rp = blockIdx.x; 2 * rp < M; rp += gridDim.x) {
    const int64_t r = 2 * rp + rsub;
    if (r >= M) continue;
    const float2 st = stats[r / F];
    const float2 s = S[r / F];
    const float m1 = s.x * invN, m2 = s.y * invN;
    const float4 x0 = *reinterpret_cast<const float4*>(src + r * CT_H + ch);
    float4 x = x0;
    if (PRE) x = make_float4(prelu(x.x, a), prelu(x.y, a), prelu(x.z, a), prelu(x.w, a));
    const float4 d = *reinterpret_cast<const float4*>(dn + r * CT_H + ch);
    float dX[4];
    const float xs[4] = {x.x, x.y, x.z, x.w}, ds[4] = {d.x, d.y, d.z, d.w}, gs[4] = {ga.x, ga.y, ga.z, ga.w};
    const float us[4] = {x0.x, x0.y, x0.z, x0.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xh = (xs[j] - st.x) * st.y;
      dX[j] = st.y * (ds[j] * gs[j] - m1 - xh * m2);
      if (PRE && !(us[j] > 0.f)) {
        sa += dX[j] * us[j];
        dX[j] *= a;
      }
    }
    if (PRE) {
      *reinterpret_cast<float4*>(dn + r * CT_H + ch) = make_float4(dX[0], dX[1], dX[2], dX[3]);
    } else {
      float4 o = *reinterpret_cast<const float4*>(out + r * CT_H + ch);
      o.x += dX[0]; o.y += dX[1]; o.z += dX[2]; o.w += dX[3];
      *reinterpret_cast<float4*>(out + r * CT_H + ch) = o;
    }
  }
  if (PRE) {
    const float t = block_sum256(sa, red);
    if (tid == 0) aslab[blockIdx.x] = t;
  }
}

// depthwise dilated conv backward (u[f] = bd + sum_k tap_k n1[f + (k - 1) dil], n1 zero outside [0, F)):
//   dn1[f] = sum_k tap_k du[f - (k - 1) dil];  d tap_k = sum_f du[f] n1[f + (k - 1) dil];  d bd = sum_f du[f]
// n1 = norm_1(PReLU_1(v1)) is recomputed from the tape.  The norm_1 backward's pass-1 sums ride along:
// row partials (sum g1, sum g1 xhat1), g1 = dn1 gamma1, and column partials d gamma1 = sum dn1 xhat1, d beta1 = sum dn1.
// colslab[wg] = [512][3] taps | [512] bias | [512] gamma1 | [512] beta1
__global__ __launch_bounds__(256) void cttrain_dconv_bwd_kernel(const float* __restrict__ du, const float* __restrict__ v1,
                                                                const float* __restrict__ slope1, const float2* __restrict__ stats,
                                                                const float* __restrict__ g1, const float* __restrict__ b1,
                                                                const float* __restrict__ wd, int dil, int F, int64_t M,
                                                                float* __restrict__ dn1, float2* __restrict__ part,
                                                                float* __restrict__ colslab) {
  __shared__ float4 red4[256];
  __shared__ float stg[CT_R * CT_H];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = wave & 1, rsub = wave >> 1;
  const int ch = half * 256 + 4 * lane;
  const float4 ga = *reinterpret_cast<const float4*>(g1 + ch), be = *reinterpret_cast<const float4*>(b1 + ch);
  float tap[4][CT_R];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < CT_R; ++k) tap[j][k] = wd[(ch + j) * CT_R + k];
  const float a1 = *slope1;
  float4 st[CT_R], sbias = make_float4(0.f, 0.f, 0.f, 0.f), sg = sbias, sb = sbias;
#pragma unroll
  for (int k = 0; k < CT_R; ++k) st[k] = sbias;
  for (int64_t rp = blockIdx.x; 2 * rp < M; rp += gridDim.x) {
    const int64_t r = 2 * rp + rsub;
    if (r >= M) continue;                            // wave-uniform
    const int64_t b = r / F, f = r - b * F;
    const float2 s = stats[b];
    const float4 dur = *reinterpret_cast<const float4*>(du + r * CT_H + ch);
    sbias.x += dur.x; sbias.y += dur.y; sbias.z += dur.z; sbias.w += dur.w;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xh_own = acc;
#pragma unroll
    for (int k = 0; k < CT_R; ++k) {
      // data gradient: du at f - (k - 1) dil
      const int64_t fd = f - (int64_t)(k - 1) * dil;
      if (fd >= 0 && fd < F) {
        const float4 g = *reinterpret_cast<const float4*>(du + (b * F + fd) * CT_H + ch);
        acc.x = fmaf(tap[0][k], g.x, acc.x);
        acc.y = fmaf(tap[1][k], g.y, acc.y);
        acc.z = fmaf(tap[2][k], g.z, acc.z);
        acc.w = fmaf(tap[3][k], g.w, acc.w);
      }
      // tap gradient: n1 at f + (k - 1) dil
      const int64_t fk = f + (int64_t)(k - 1) * dil;
      if (fk >= 0 && fk < F) {
        float4 v = *reinterpret_cast<const float4*>(v1 + (b * F + fk) * CT_H + ch);
        v = make_float4(prelu(v.x, a1), prelu(v.y, a1), prelu(v.z, a1), prelu(v.w, a1));
        const float4 xh = make_float4((v.x - s.x) * s.y, (v.y - s.x) * s.y, (v.z - s.x) * s.y, (v.w - s.x) * s.y);
        if (k == 1) xh_own = xh;
        st[k].x += dur.x * (xh.x * ga.x + be.x);
        st[k].y += dur.y * (xh.y * ga.y + be.y);
        st[k].z += dur.z * (xh.z * ga.z + be.z);
        st[k].w += dur.w * (xh.w * ga.w + be.w);
      }
    }
    *reinterpret_cast<float4*>(dn1 + r * CT_H + ch) = acc;
    const float4 g = make_float4(acc.x * ga.x, acc.y * ga.y, acc.z * ga.z, acc.w * ga.w);
    const float s1 = wave_sum((g.x + g.y) + (g.z + g.w));
    const float s2 = wave_sum((g.x * xh_own.x + g.y * xh_own.y) + (g.z * xh_own.z + g.w * xh_own.w));
    if (lane == 0) part[r * 2 + half] = make_float2(s1, s2);
    sg.x += acc.x * xh_own.x; sg.y += acc.y * xh_own.y; sg.z += acc.z * xh_own.z; sg.w += acc.w * xh_own.w;
    sb.x += acc.x; sb.y += acc.y; sb.z += acc.z; sb.w += acc.w;
  }
  float* dst = colslab + (size_t)blockIdx.x * CTT_ROW_SLAB;
  float* red = reinterpret_cast<float*>(red4);
  // tap partials staged [k][512] in LDS, written [channel][3] (the layout of dconv1d.weight)
#pragma unroll
  for (int k = 0; k < CT_R; ++k) colpart_store(st[k], red, stg + k * CT_H, tid);
  for (int i = tid; i < CT_R * CT_H; i += 256) dst[i] = stg[(i % CT_R) * CT_H + i / CT_R];
  colpart_store(sbias, red, dst + 3 * CT_H, tid);
  colpart_store(sg, red, dst + 4 * CT_H, tid);
  colpart_store(sb, red, dst + 5 * CT_H, tid);
}

// out[n * ldo + k] = sum_s slab[s * stride + n * cols + k] in a FIXED association order (slab_reduce_kernel's scheme with
// a strided destination): a workgroup owns 32 consecutive elements; its 8 slab-lanes sum the slabs s = lane, lane + 8, ...
// with four loads in flight, then the lanes are combined in lane order.
__global__ __launch_bounds__(256) void cttrain_reduce_kernel(const float* __restrict__ slab, int nslabs, int64_t stride, int rows,
                                                             int cols, float* __restrict__ out, int ldo) {
  __shared__ float red[8][32];
  const int e = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t i = (int64_t)blockIdx.x * 32 + e;
  const int64_t count = (int64_t)rows * cols;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < count) {
    const float* p = slab + i;
    int k = sl;
    for (; k + 24 < nslabs; k += 32) {
      s0 += p[(int64_t)k * stride];
      s1 += p[(int64_t)(k + 8) * stride];
      s2 += p[(int64_t)(k + 16) * stride];
      s3 += p[(int64_t)(k + 24) * stride];
    }
    for (; k < nslabs; k += 8) s0 += p[(int64_t)k * stride];
  }
  red[sl][e] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (sl == 0 && i < count) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += red[j][e];
    const int n = (int)(i / cols), k = (int)(i - (int64_t)n * cols);
    out[(int64_t)n * ldo + k] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// engine hooks of the backward
// ------------------------------------------------------------------------------------------------
// A = [dx | dskip] (K = 256): the upstream gradients of conv (residual) and conv_sc (skip)
struct ALoadCat {
  const float* A0;
  const float* A1;
  int64_t M;
  DEV float4 load4(int tile, int row, int k4) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    if (r >= M) return make_float4(0.f, 0.f, 0.f, 0.f);
    return k4 < CT_B / 4 ? *reinterpret_cast<const float4*>(A0 + r * CT_B + 4 * k4)
                         : *reinterpret_cast<const float4*>(A1 + r * CT_B + 4 * (k4 - CT_B / 4));
  }
};

// normalised rows (PReLU first if PRE), columns [col0, col0 + 128): the X operand of a weight gradient
template <bool PRE>
struct ALoadNormCols {
  const float* A;
  const float* slope;
  const float2* stats;
  const float* gamma;
  const float* beta;
  int64_t M;
  int F;
  int col0;
  DEV float4 load4(int tile, int row, int k4) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    if (r >= M) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float2 st = stats[r / F];
    const int c = col0 + 4 * k4;
    float4 v = *reinterpret_cast<const float4*>(A + r * CT_H + c);
    if (PRE) {
      const float a = *slope;
      v = make_float4(prelu(v.x, a), prelu(v.y, a), prelu(v.z, a), prelu(v.w, a));
    }
    const float4 g = *reinterpret_cast<const float4*>(gamma + c), bb = *reinterpret_cast<const float4*>(beta + c);
    return make_float4((v.x - st.x) * st.y * g.x + bb.x, (v.y - st.x) * st.y * g.y + bb.y,
                       (v.z - st.x) * st.y * g.z + bb.z, (v.w - st.x) * st.y * g.w + bb.w);
  }
};

// encoder patches: row r = (b, f), column k = sample 16 f + k - 16 of mixture b (zero outside [0, T))
struct ALoadPatches {
  const float* mix;
  int64_t T;
  int64_t M;
  int F;
  DEV float4 load4(int tile, int row, int k4) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    if (r >= M) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t b = r / F, f = r - b * F;
    const float* x = mix + b * T;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t j = CT_L * f + 4 * k4 + i - CT_L;
      v[i] = (j >= 0 && j < T) ? x[j] : 0.f;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
  }
};

// out[row][128 colgroup + 4 c4 ..] = v, or += v (ADD)
struct EpiStoreAdd {
  static constexpr bool DIRECT = false;
  static constexpr bool HAS_FINISH = false;
  float* out;
  int64_t M;
  int ldo;
  int add;
  DEV float4 prefetch(int, int, int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
  DEV void row(int tile, int row, int colgroup, int c4, float4 v, float4) const {
    const int64_t r = (int64_t)tile * CT_BM + row;
    if (r >= M) return;
    float* dst = out + r * ldo + colgroup * 128 + 4 * c4;
    if (add) {
      const float4 o = *reinterpret_cast<const float4*>(dst);
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    *reinterpret_cast<float4*>(dst) = v;
  }
};

// ------------------------------------------------------------------------------------------------
// host side: launch helpers for a handle type derived from CtHandle
// ------------------------------------------------------------------------------------------------
inline size_t align64f(size_t n) { return (n + 63) & ~(size_t)63; }

template <class Ctx, class Kern>
int ensure_lds(Ctx* c, PerDeviceOnce& once, Kern kern, size_t bytes, const char* what) {
  if (!once.done(c->device_id)) {
    if (int rc = set_lds(c, kern, bytes, what)) return rc;
    once.set(c->device_id);
  }
  return CTASNET_OK;
}

template <class Ctx>
int launch_reduce(Ctx* c, hipStream_t st, const float* slab, int nslabs, int64_t stride, int rows, int cols, float* out,
                  int ldo) {
  const int64_t n = (int64_t)rows * cols;
  hipLaunchKernelGGL(cttrain_reduce_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st, slab, nslabs, stride, rows, cols,
                     out, ldo);
  HANDLE_LAUNCH_CHECK(c, "cttrain reduce");
  return CTASNET_OK;
}

// dW[NN][KK] partials of wgrad_generic_kernel -> slab [grid][NN][KK]; returns the grid (number of slabs)
template <int NN, int KK, class Ctx, class YL, class XL>
int launch_wgrad(Ctx* c, hipStream_t st, int64_t rows, const YL& yl, const XL& xl, float* slab, int* nslabs) {
  auto kern = wgrad_generic_kernel<NN, KK, YL, XL>;
  const size_t lds = sizeof(float) * 32 * ((size_t)(NN + 4) + (KK + 4));
  static PerDeviceOnce once;
  if (int rc = ensure_lds(c, once, kern, lds, "cttrain wgrad")) return rc;
  const int ntiles = (int)((rows + 31) / 32);
  const int g = std::min(ntiles, CTT_G_W);
  hipLaunchKernelGGL(kern, dim3(g), dim3(256), lds, st, ntiles, yl, xl, slab);
  HANDLE_LAUNCH_CHECK(c, "cttrain wgrad");
  *nslabs = g;
  return CTASNET_OK;
}

// bias gradient: column sums of Y[M][ld] columns [col0, col0 + C) -> out[C]
template <int C, class Ctx>
int launch_colsum(Ctx* c, hipStream_t st, const float* Y, int64_t M, int ld, int col0, float* cslab, float* out) {
  hipLaunchKernelGGL(colsum_kernel<C>, dim3(CTT_G_C), dim3(256), 0, st, Y, M, ld, col0, cslab);
  HANDLE_LAUNCH_CHECK(c, "cttrain colsum");
  return launch_reduce(c, st, cslab, CTT_G_C, C, 1, C, out, C);
}

// The Separator's part of a training workspace, as byte offsets: its tape (what launch_separator<true> leaves) and the
// scratch of launch_separator_backward.  taps holds the decoder's taps in the forward and their gradient in the backward.
struct SepTrainPlan {
  // tape
  size_t off_enc, off_stats0, off_x, off_skip, off_v1, off_u, off_st1, off_st2, off_ym, off_mk;
  // scratch
  size_t off_taps, off_part, off_dv, off_denc, off_dx, off_dskip, off_bufa, off_bufb, off_S, off_wrs, off_slab, off_cslab,
      off_aslab;
};

// slab_floats: the unit's largest weight-gradient slab beyond the Separator's own
inline void plan_separator_train(SepTrainPlan& p, ByteCursor& cur, int B, size_t M, size_t slab_floats = 0) {
  p.off_enc = cur.take(M * CT_N * 4);
  p.off_stats0 = cur.take((size_t)B * sizeof(float2));
  p.off_x = cur.take((size_t)(CT_BLOCKS + 1) * M * CT_B * 4);
  p.off_skip = cur.take(M * CT_B * 4);
  p.off_v1 = cur.take((size_t)CT_BLOCKS * M * CT_H * 4);
  p.off_u = cur.take((size_t)CT_BLOCKS * M * CT_H * 4);
  p.off_st1 = cur.take((size_t)CT_BLOCKS * B * sizeof(float2));
  p.off_st2 = cur.take((size_t)CT_BLOCKS * B * sizeof(float2));
  p.off_ym = cur.take(M * 2 * CT_N * 4);
  p.off_mk = cur.take(M * 2 * CT_N * 4);
  p.off_taps = cur.take(M * 4 * CT_L * 4);
  p.off_part = cur.take(M * 4 * sizeof(float2));
  p.off_dv = cur.take(M * 2 * CT_N * 4);
  p.off_denc = cur.take(M * CT_N * 4);
  p.off_dx = cur.take(M * CT_B * 4);
  p.off_dskip = cur.take(M * CT_B * 4);
  p.off_bufa = cur.take(M * CT_H * 4);
  p.off_bufb = cur.take(M * CT_H * 4);
  p.off_S = cur.take((size_t)B * sizeof(float2));
  p.off_wrs = cur.take((size_t)2 * CT_B * CT_H * 4);
  const size_t slab = std::max({(size_t)CTT_G_W * 256 * 128, (size_t)CTT_G_W * CT_N * 2 * CT_L,
                                (size_t)CTT_G_ROW * CTT_ROW_SLAB, slab_floats});
  p.off_slab = cur.take(slab * 4);
  p.off_cslab = cur.take((size_t)CTT_G_C * 2 * CT_N * 4);
  p.off_aslab = cur.take((size_t)CTT_G_ROW * 4);
}

inline SepBuffers sep_tape_buffers(const SepTrainPlan& p, void* ws) {
  char* base = static_cast<char*>(ws);
  auto fp = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  auto f2 = [&](size_t off) { return reinterpret_cast<float2*>(base + off); };
  return SepBuffers{fp(p.off_x), fp(p.off_skip), fp(p.off_v1), fp(p.off_u), f2(p.off_part), f2(p.off_stats0), f2(p.off_st1),
                    f2(p.off_st2), fp(p.off_ym), fp(p.off_mk)};
}

// Backward of launch_separator<true> (convtasnet.py:55-83), from the mask head to the GlobalNorm: given the gradient of
// the masked tensor ym -- FORM HEAD_TAPS: `head_in` = the decoder's taps gradient [M][2][32] and D its weight; HEAD_DYM:
// `head_in` = d ym [M][1024] -- it writes every Separator gradient (sg: CT_SEP_W buffers in state_dict order, sw the
// weights) and leaves the complete d enc [M][512] (head + GlobalNorm contributions) in the plan's denc.
template <int FORM, class Ctx>
int launch_separator_backward(Ctx* c, hipStream_t st, const float* const* sw, float* const* sg, const float* head_in,
                              const float* D, int B, int F, int64_t M, const SepTrainPlan& p, void* ws) {
  char* base = static_cast<char*>(ws);
  auto fp = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  auto f2 = [&](size_t off) { return reinterpret_cast<float2*>(base + off); };
  const int HEAD = 4 + CT_BLOCKS * CT_BLOCK_W;
  float* enc = fp(p.off_enc);
  float* skip = fp(p.off_skip);
  float* dv = fp(p.off_dv);
  float* denc = fp(p.off_denc);
  float* dx = fp(p.off_dx);
  float* dskip = fp(p.off_dskip);
  float* bufa = fp(p.off_bufa);
  float* bufb = fp(p.off_bufb);
  float* wrs = fp(p.off_wrs);
  float* slab = fp(p.off_slab);
  float* cslab = fp(p.off_cslab);
  float* aslab = fp(p.off_aslab);
  float2* part = f2(p.off_part);
  float2* S = f2(p.off_S);
  int ns = 0;

  // ---- mask head (convtasnet.py:76-80): dv, the head's d enc, seq.1 weight / bias, d skip through PReLU seq.0
  {
    static PerDeviceOnce once;
    if (int rc = ensure_lds(c, once, cttrain_head_bwd_kernel<FORM>, CTT_HEAD_LDS, "cttrain head backward")) return rc;
    const unsigned g = (unsigned)std::min<int64_t>(M, 2048);
    hipLaunchKernelGGL(cttrain_head_bwd_kernel<FORM>, dim3(g), dim3(256), CTT_HEAD_LDS, st, head_in, D, fp(p.off_mk), enc, M, dv,
                       denc);
    HANDLE_LAUNCH_CHECK(c, "cttrain head backward");
    if (int rc = launch_colsum<2 * CT_N>(c, st, dv, M, 2 * CT_N, 0, cslab, sg[HEAD + 2])) return rc;
    for (int q = 0; q < 4; ++q) {
      if (int rc = launch_wgrad<256, CT_B>(c, st, M, ALoadColsT<false>{dv, M, 2 * CT_N, 256 * q, 32},
                                           ALoadDensePReLU{skip, sw[HEAD], M, CT_B, 32}, slab, &ns))
        return rc;
      if (int rc = launch_reduce(c, st, slab, ns, 256 * CT_B, 256, CT_B, sg[HEAD + 1] + (size_t)256 * q * CT_B, CT_B)) return rc;
    }
    for (int q = 0; q < 2; ++q)
      if (int rc = launch_gemm<CT_N, true>(c, st, "cttrain head dgrad", sw[HEAD + 1] + (size_t)q * CT_N * CT_B, nullptr, M, 1,
                                           ALoadColsT<false>{dv, M, 2 * CT_N, CT_N * q, CT_BM}, EpiStoreAdd{dskip, M, CT_B, q},
                                           CT_B))
        return rc;
    hipLaunchKernelGGL(cttrain_prelu_bwd_kernel, dim3(CTT_G_ROW), dim3(256), 0, st, dskip, skip, sw[HEAD], M * CT_B, aslab);
    HANDLE_LAUNCH_CHECK(c, "cttrain head prelu backward");
    if (int rc = launch_reduce(c, st, aslab, CTT_G_ROW, 1, 1, 1, sg[HEAD], 1)) return rc;
  }

  // ---- blocks, last to first (convtasnet.py:46-53, :69-74); dx = d x_{i+1} (zero after the last block), dskip fixed
  if (hipMemsetAsync(dx, 0, (size_t)M * CT_B * 4, st) != hipSuccess) return c->fail(CTASNET_ERR_HIP, "cttrain: memset failed");
  for (int i = CT_BLOCKS - 1; i >= 0; --i) {
    const int wi = 4 + i * CT_BLOCK_W;         // index of this block's conv1d.weight
    const float* const* bw = sw + wi;
    float* const* bg = sg + wi;
    const int dil = 1 << (i % CT_X);
    const float* xi = fp(p.off_x) + (size_t)i * M * CT_B;
    const float* v1 = fp(p.off_v1) + (size_t)i * M * CT_H;
    const float* u = fp(p.off_u) + (size_t)i * M * CT_H;
    const float2* st1 = f2(p.off_st1) + (size_t)i * B;
    const float2* st2 = f2(p.off_st2) + (size_t)i * B;

    // res | skip 1x1: d n2 = [dx | dskip] [Wr ; Ws]  (operand gathered in this step), weight and bias gradients
    if (hipMemcpyAsync(wrs, bw[10], (size_t)CT_B * CT_H * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(wrs + (size_t)CT_B * CT_H, bw[12], (size_t)CT_B * CT_H * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return c->fail(CTASNET_ERR_HIP, "cttrain: weight gather failed");
    if (int rc = launch_gemm<2 * CT_B, true>(c, st, "cttrain res|skip dgrad", wrs, nullptr, M, CT_H / 128,
                                             ALoadCat{dx, dskip, M}, EpiStoreAdd{bufa, M, CT_H, 0}, CT_H))
      return rc;
    for (int q = 0; q < CT_H / 128; ++q) {
      if (int rc = launch_wgrad<2 * CT_B, 128>(c, st, M, ALoadCat{dx, dskip, M},
                                               ALoadNormCols<true>{u, bw[7], st2, bw[8], bw[9], M, F, 128 * q}, slab, &ns))
        return rc;
      if (int rc = launch_reduce(c, st, slab, ns, 2 * CT_B * 128, CT_B, 128, bg[10] + 128 * q, CT_H)) return rc;
      if (int rc = launch_reduce(c, st, slab + CT_B * 128, ns, 2 * CT_B * 128, CT_B, 128, bg[12] + 128 * q, CT_H)) return rc;
    }
    if (int rc = launch_colsum<CT_B>(c, st, dx, M, CT_B, 0, cslab, bg[11])) return rc;
    if (int rc = launch_colsum<CT_B>(c, st, dskip, M, CT_B, 0, cslab, bg[13])) return rc;

    // norm_2 (GroupNorm(1), eps 1e-10) and PReLU_2: bufa = d n2 -> d u in place
    hipLaunchKernelGGL(cttrain_normstat_kernel<true>, dim3(CTT_G_ROW), dim3(256), 0, st, bufa, u, bw[7], st2, bw[8], F, M, part,
                       slab);
    HANDLE_LAUNCH_CHECK(c, "cttrain norm_2 stats");
    if (int rc = launch_reduce(c, st, slab, CTT_G_ROW, 2 * CT_H, 1, CT_H, bg[8], CT_H)) return rc;
    if (int rc = launch_reduce(c, st, slab + CT_H, CTT_G_ROW, 2 * CT_H, 1, CT_H, bg[9], CT_H)) return rc;
    hipLaunchKernelGGL(cttrain_mixsum_kernel, dim3(B), dim3(256), 0, st, part, F, S);
    HANDLE_LAUNCH_CHECK(c, "cttrain mixsum");
    hipLaunchKernelGGL(cttrain_normapply_kernel<true>, dim3(CTT_G_ROW), dim3(256), 0, st, bufa, u, bw[7], st2, bw[8], S, F, M,
                       nullptr, aslab);
    HANDLE_LAUNCH_CHECK(c, "cttrain norm_2 backward");
    if (int rc = launch_reduce(c, st, aslab, CTT_G_ROW, 1, 1, 1, bg[7], 1)) return rc;

    // depthwise conv (taps, bias) and norm_1's pass 1: bufb = d n1
    hipLaunchKernelGGL(cttrain_dconv_bwd_kernel, dim3(CTT_G_ROW), dim3(256), 0, st, bufa, v1, bw[2], st1, bw[3], bw[4], bw[5], dil,
                       F, M, bufb, part, slab);
    HANDLE_LAUNCH_CHECK(c, "cttrain dconv backward");
    if (int rc = launch_reduce(c, st, slab, CTT_G_ROW, CTT_ROW_SLAB, 1, CT_R * CT_H, bg[5], CT_R * CT_H)) return rc;
    if (int rc = launch_reduce(c, st, slab + 3 * CT_H, CTT_G_ROW, CTT_ROW_SLAB, 1, CT_H, bg[6], CT_H)) return rc;
    if (int rc = launch_reduce(c, st, slab + 4 * CT_H, CTT_G_ROW, CTT_ROW_SLAB, 1, CT_H, bg[3], CT_H)) return rc;
    if (int rc = launch_reduce(c, st, slab + 5 * CT_H, CTT_G_ROW, CTT_ROW_SLAB, 1, CT_H, bg[4], CT_H)) return rc;
    hipLaunchKernelGGL(cttrain_mixsum_kernel, dim3(B), dim3(256), 0, st, part, F, S);
    HANDLE_LAUNCH_CHECK(c, "cttrain mixsum");
    // norm_1 (GroupNorm(1), eps 1e-10) and PReLU_1: bufb = d n1 -> d v1 in place
    hipLaunchKernelGGL(cttrain_normapply_kernel<true>, dim3(CTT_G_ROW), dim3(256), 0, st, bufb, v1, bw[2], st1, bw[3], S, F, M,
                       nullptr, aslab);
    HANDLE_LAUNCH_CHECK(c, "cttrain norm_1 backward");
    if (int rc = launch_reduce(c, st, aslab, CTT_G_ROW, 1, 1, 1, bg[2], 1)) return rc;

    // 128 -> 512 1x1: weight / bias gradients from d v1 and x_i, then d x_i = d x_{i+1} + d v1 W1 (residual) in place
    for (int q = 0; q < 2; ++q) {
      if (int rc = launch_wgrad<256, CT_B>(c, st, M, ALoadColsT<false>{bufb, M, CT_H, 256 * q, 32}, ALoadDense{xi, M, CT_B, 32},
                                           slab, &ns))
        return rc;
      if (int rc = launch_reduce(c, st, slab, ns, 256 * CT_B, 256, CT_B, bg[0] + (size_t)256 * q * CT_B, CT_B)) return rc;
    }
    if (int rc = launch_colsum<CT_H>(c, st, bufb, M, CT_H, 0, cslab, bg[1])) return rc;
    if (int rc = launch_gemm<CT_H, true>(c, st, "cttrain block 1x1 dgrad", bw[0], nullptr, M, 1,
                                         ALoadDense{bufb, M, CT_H, CT_BM}, EpiStoreAdd{dx, M, CT_B, 1}, CT_B))
      return rc;
  }

  // ---- bottleneck 1x1 (convtasnet.py:67-68) and GlobalNorm (eps 5e-6, :25-29): the second d enc contribution
  {
    const float2* stats0 = f2(p.off_stats0);
    for (int q = 0; q < CT_N / 128; ++q) {
      if (int rc = launch_wgrad<CT_B, 128>(c, st, M, ALoadDense{dx, M, CT_B, 32},
                                           ALoadNormCols<false>{enc, nullptr, stats0, sw[0], sw[1], M, F, 128 * q}, slab, &ns))
        return rc;
      if (int rc = launch_reduce(c, st, slab, ns, CT_B * 128, CT_B, 128, sg[2] + 128 * q, CT_N)) return rc;
    }
    if (int rc = launch_colsum<CT_B>(c, st, dx, M, CT_B, 0, cslab, sg[3])) return rc;
    if (int rc = launch_gemm<CT_B, true>(c, st, "cttrain bottleneck dgrad", sw[2], nullptr, M, CT_N / 128,
                                         ALoadDense{dx, M, CT_B, CT_BM}, EpiStoreAdd{bufa, M, CT_N, 0}, CT_N))
      return rc;
    hipLaunchKernelGGL(cttrain_normstat_kernel<false>, dim3(CTT_G_ROW), dim3(256), 0, st, bufa, enc, nullptr, stats0, sw[0], F, M,
                       part, slab);
    HANDLE_LAUNCH_CHECK(c, "cttrain GlobalNorm stats");
    if (int rc = launch_reduce(c, st, slab, CTT_G_ROW, 2 * CT_N, 1, CT_N, sg[0], CT_N)) return rc;
    if (int rc = launch_reduce(c, st, slab + CT_N, CTT_G_ROW, 2 * CT_N, 1, CT_N, sg[1], CT_N)) return rc;
    hipLaunchKernelGGL(cttrain_mixsum_kernel, dim3(B), dim3(256), 0, st, part, F, S);
    HANDLE_LAUNCH_CHECK(c, "cttrain mixsum");
    hipLaunchKernelGGL(cttrain_normapply_kernel<false>, dim3(CTT_G_ROW), dim3(256), 0, st, bufa, enc, nullptr, stats0, sw[0], S, F,
                       M, denc, nullptr);
    HANDLE_LAUNCH_CHECK(c, "cttrain GlobalNorm backward");
  }
  return CTASNET_OK;
}

// ------------------------------------------------------------------------------------------------
// the training handle and what the extern "C" entry points of the training units share (idiom of ctasnet_handle.h)
// ------------------------------------------------------------------------------------------------
struct CtTrainHandle : CtHandle {
  const char* const prefix;    // of the unit's entry points, for messages: "cttrain" / "dcttrain"
  const int no_grad_slot;      // a parameter the forward never reads: no gradient, no AdamW step; -1 when there is none
  std::vector<float*> g;
  bool gbound = false;
  CtTrainHandle(const char* prefix_, int no_grad_slot_) : prefix(prefix_), no_grad_slot(no_grad_slot_) {}
};

inline int bind_grads(CtTrainHandle* h, float* const* dev_ptrs, int n) {
  if (int rc = check_table_ptrs(h, reinterpret_cast<const void* const*>(dev_ptrs), n, "gradient", 4)) return rc;
  h->g.assign(dev_ptrs, dev_ptrs + n);
  h->gbound = true;
  return CTASNET_OK;
}

// the flat layout of gradient / exp_avg / exp_avg_sq: every slot rounded up to 64 floats
inline int64_t flat_offset(const CtHandle* h, int slot) {
  if (slot < 0 || slot > (int)h->numels.size()) return -1;
  int64_t o = 0;
  for (int i = 0; i < slot; ++i) o += (int64_t)align64f((size_t)h->numels[i]);
  return o;
}
inline int64_t flat_numel(const CtHandle* h) { return flat_offset(h, (int)h->numels.size()); }

inline int train_grad_clip(CtTrainHandle* h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                           float* norm_out, void* stream) {
  if (!flat_grad || !norm_out || n_flat < 4 || (n_flat & 3) || ((uintptr_t)flat_grad & 15))
    return h->fail(CTASNET_ERR_INVALID, "grad_clip: flat gradient must be 16-byte aligned with a multiple of 4 floats");
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < CLIP_PARTS * sizeof(double))
    return h->fail(CTASNET_ERR_WORKSPACE, "grad_clip: scratch too small / misaligned");
  launch_grad_clip((hipStream_t)stream, h->num_cus, flat_grad, n_flat, max_norm, (double*)scratch, norm_out);
  if (hipError_t e = hipGetLastError()) return h->fail(CTASNET_ERR_HIP, "%s grad_clip: %s", h->prefix, hipGetErrorString(e));
  return CTASNET_OK;
}

inline int train_adamw_step(CtTrainHandle* h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                            double beta1, double beta2, double eps, double weight_decay, int step, void* stream) {
  if (!h->bound) return h->fail(CTASNET_ERR_WEIGHTS, "adamw_step: weights not bound (the step updates the bound parameters in place)");
  if (!flat_grad || !exp_avg || !exp_avg_sq || n_flat != flat_numel(h) || step < 1)
    return h->fail(CTASNET_ERR_INVALID, "adamw_step: bad argument (flat buffers must hold %lld floats, step >= 1)",
                   (long long)flat_numel(h));
  launch_adamw((hipStream_t)stream, h->w.data(), h->numels.data(), (int)h->names.size(), h->no_grad_slot, 64, flat_grad, exp_avg,
               exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step);
  if (hipError_t e = hipGetLastError()) return h->fail(CTASNET_ERR_HIP, "%s adamw_step: %s", h->prefix, hipGetErrorString(e));
  return CTASNET_OK;
}

// what every training plan starts with; `rows` is the unit's spelling of B*F*1024 in the message
struct TrainPlanBase : SepTrainPlan {
  int64_t F, M, Lout;
  size_t total;
};

inline int plan_train_head(CtHandle* c, int B, int64_t T, const char* rows, TrainPlanBase& p) {
  if (int rc = check_batch(c, B, T)) return rc;
  p.F = frames_of(T);
  p.M = (int64_t)B * p.F;
  if (p.M * 2 * CT_N > (int64_t)INT32_MAX)      // 32-bit row indexing of the loaders
    return c->fail(CTASNET_ERR_INVALID, "%s = %lld exceeds 32-bit indexing (B=%d, T=%lld)", rows, (long long)(p.M * 2 * CT_N), B,
                   (long long)T);
  p.Lout = CT_L * (T / CT_L);
  return CTASNET_OK;
}

// *_tape_offset of the Separator's tensors (*_TAPE_V1 / _U / _SKIP in the headers); any other kind is refused
enum { SEP_TAPE_V1 = 0, SEP_TAPE_U = 1, SEP_TAPE_SKIP = 2 };
inline int64_t sep_tape_offset(CtHandle* h, const TrainPlanBase& p, int which, int block) {
  if (which == SEP_TAPE_SKIP) return block == 0 ? (int64_t)p.off_skip : -1;
  if (block < 0 || block >= CT_BLOCKS) {
    h->fail(CTASNET_ERR_INVALID, "block %d out of range", block);
    return -1;
  }
  if (which == SEP_TAPE_V1) return (int64_t)(p.off_v1 + (size_t)block * p.M * CT_H * 4);
  if (which == SEP_TAPE_U) return (int64_t)(p.off_u + (size_t)block * p.M * CT_H * 4);
  h->fail(CTASNET_ERR_INVALID, "unknown tape tensor %d", which);
  return -1;
}

// typed pointers into a workspace
struct WsPtr {
  char* base;
  float* fp(size_t off) const { return reinterpret_cast<float*>(base + off); }
  float2* f2(size_t off) const { return reinterpret_cast<float2*>(base + off); }
};

// What *_train_forward (o1, o2: the predictions) and *_train_backward (their gradients; needs the gradients bound) start
// with: the checks, the unit's plan and the workspace behind it.
// make_plan(c, B, T, p): the unit's plan (a function, or a callable that carries what else the plan depends on).
template <class Plan, class MakePlan>
int train_prologue(CtTrainHandle* c, MakePlan make_plan, bool backward, const void* mix,
                   const void* o1, const void* o2, int B, int64_t T, void* ws, size_t ws_bytes, Plan& p, WsPtr& at) {
  if (!c) return CTASNET_ERR_INVALID;
  if (!c->bound) return c->fail(CTASNET_ERR_WEIGHTS, "weights not bound (%s_bind_weights)", c->prefix);
  if (backward && !c->gbound) return c->fail(CTASNET_ERR_WEIGHTS, "gradients not bound (%s_bind_grads)", c->prefix);
  if (!mix || !o1 || !o2) return c->fail(CTASNET_ERR_INVALID, "mix / %s must not be NULL", backward ? "d_s1 / d_s2" : "s1_pred / s2_pred");
  if (int rc = make_plan(c, B, T, p)) return rc;
  if (int rc = check_workspace(c, p.total, ws, ws_bytes)) return rc;
  at.base = static_cast<char*>(ws);
  return CTASNET_OK;
}

}  // namespace
