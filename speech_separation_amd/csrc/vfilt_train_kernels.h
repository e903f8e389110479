// vfilt_train_kernels.h -- device code of the VoiceFilter training step (vfilt_train.hip) that is its own: batch-statistics
// BatchNorm (fixed-order two-stage reductions, normalise, backward), the weight gradient of the 64 -> 64 convolutions on
// fp32 MFMA, the thin ends of the CNN's backward on VALU, the LSTM's forward step with a tape and its backward step, the
// GRU's forward with a tape and its backward, dropout and the pointwise pieces of the FC tail.  The 64 -> 64 convolutions
// (forward and data gradient) run on lipfe_kernels.h's implicit-GEMM kernel, every dense product on vfilt_kernels.h's GEMM.
//
// Every reduction has a fixed order that depends on the shape alone: positions are cut into chunks of a fixed size, a
// workgroup sums one chunk, a second launch adds the chunks in order.  No atomics; no workgroup waits for another one.
#pragma once
#include "vfilt_kernels.h"

namespace {

constexpr int VFT_CHUNK = 1024;      // rows per partial of a column reduction
constexpr int VFT_WG_CHUNK = 4096;   // positions per partial tile of the MFMA weight gradient (128 K steps)
constexpr int VFT_STAT = 2 * 64;     // floats per layer: mean, invstd
constexpr int VFT_COEF = 3 * 64;     // floats of a BatchNorm backward's coefficients: gamma * invstd, mean(dy), mean(dy xhat)

// the 256 threads of a block are R = 256 / C rows x C columns; v[i] of the R rows are added in row order -> dst[i * C + c]
template <int C, int NV, class T>
DEV void vft_block_combine(const T (&v)[NV], T* __restrict__ dst) {
  constexpr int R = 256 / C;
  __shared__ T red[NV][R][C];
  const int c = threadIdx.x % C, r = threadIdx.x / C;
#pragma unroll
  for (int i = 0; i < NV; ++i) red[i][r][c] = v[i];
  __syncthreads();
  if (r == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      T s = 0;
#pragma unroll
      for (int rr = 0; rr < R; ++rr) s += red[i][rr][c];
      dst[i * C + c] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// conv bias as a fold (scale 1, shift bias): lipfe_conv_kernel / vfilt_conv8_kernel then write the raw Z = conv + bias
// ------------------------------------------------------------------------------------------------
struct VftBiasSrc {
  const float* cb[VF_LAYERS];
  int C[VF_LAYERS];
};
// grid (9), block 64: fold[l] = ones[64] then bias[64] at float 128 l; entry 8 is (1, 0): the data gradient's epilogue
__global__ void __launch_bounds__(64) vftrain_bias_fold_kernel(VftBiasSrc s, float* __restrict__ fold) {
  const int l = blockIdx.x, c = threadIdx.x;
  fold[128 * l + c] = 1.f;
  fold[128 * l + 64 + c] = (l < VF_LAYERS && c < s.C[l]) ? s.cb[l][c] : 0.f;
}

// layer 1 without BatchNorm and ReLU: mix [B][F][W] -> Z [B][F][W][64] = conv + bias (the taps in vfilt_conv1_kernel's order)
__global__ void __launch_bounds__(256) vftrain_conv1_kernel(const float* __restrict__ mix, const float* __restrict__ w1,
                                                            const float* __restrict__ bias, float* __restrict__ out,
                                                            long long total, int W) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i & 63);
  const long long pos = i >> 6;
  const int x = (int)(pos % W);
  const float* row = mix + (pos - x);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int ix = x + k - 3;
    if (ix >= 0 && ix < W) s = fmaf(row[ix], w1[c * 7 + k], s);
  }
  out[i] = s + bias[c];
}

// ------------------------------------------------------------------------------------------------
// BatchNorm with batch statistics over X [n][C]
// ------------------------------------------------------------------------------------------------
// grid (ceil(n / 1024)), block 256: parts[chunk][C] = sum over the chunk's rows of x - m (m = mean or NULL) or its square.
// The sums of the statistics run in double from the first addition on: the mean and the variance then carry the rounding
// of their own fp32 result and nothing else (the pass is bound by its loads, not by the additions).
template <int C, bool SQUARE>
__global__ void __launch_bounds__(256) vftrain_stat_part_kernel(const float* __restrict__ X, long long n, const float* __restrict__ mean,
                                                                double* __restrict__ parts) {
  constexpr int R = 256 / C;
  const int c = threadIdx.x % C, r = threadIdx.x / C;
  const long long r0 = (long long)blockIdx.x * VFT_CHUNK;
  const double m = mean ? (double)mean[c] : 0.0;
  double v[1] = {0.0};
  const int rows = (int)(n - r0 < VFT_CHUNK ? n - r0 : (long long)VFT_CHUNK);      // no guard inside: the loads of an unrolled body go out together
#pragma unroll 8
  for (int j = r; j < rows; j += R) {
    const double d = (double)X[(r0 + j) * C + c] - m;
    v[0] += SQUARE ? d * d : d;
  }
  vft_block_combine<C, 1, double>(v, parts + (long long)blockIdx.x * C);
}

// grid (1), block 64: the chunks in order, in double.  mean -> stat[0][c]
__global__ void __launch_bounds__(64) vftrain_stat_mean_kernel(const double* __restrict__ parts, int nparts, int C, long long n,
                                                               float* __restrict__ stat) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += parts[(long long)p * C + c];
  stat[c] = (float)(s / (double)n);
}

// grid (1), block 64: biased variance -> invstd = 1 / sqrt(var + eps) at stat[64 + c]; the batch mean and the UNBIASED
// variance -> block[c], block[64 + c] (what the running buffers are updated with)
__global__ void __launch_bounds__(64) vftrain_stat_var_kernel(const double* __restrict__ parts, int nparts, int C, long long n,
                                                              float* __restrict__ stat, float* __restrict__ block) {
  const int c = threadIdx.x;
  if (c >= C) {
    block[c] = 0.f;
    block[64 + c] = 0.f;
    return;
  }
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += parts[(long long)p * C + c];
  stat[64 + c] = (float)(1.0 / sqrt(s / (double)n + (double)LF_BN_EPS));
  block[c] = stat[c];
  block[64 + c] = (float)(s / (double)(n - 1));
}

// out = act(((z - mean) * invstd) * gamma + beta), four channels per thread; total4 = n * C / 4
template <int C>
__global__ void __launch_bounds__(256) vftrain_norm_kernel(const float* __restrict__ Z, const float* __restrict__ stat,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ out, long long total4, int relu) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)((i * 4) % C);
  const float4 z = ldg4(Z + 4 * i);
  const float zz[4] = {z.x, z.y, z.z, z.w};
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v = fmaf((zz[j] - stat[c + j]) * stat[64 + c + j], gamma[c + j], beta[c + j]);
    o[j] = relu ? fmaxf(v, 0.f) : v;
  }
  *reinterpret_cast<float4*>(out + 4 * i) = make_float4(o[0], o[1], o[2], o[3]);
}

// grid (ceil(n / 1024)), block 256: parts[chunk][2][C] = sum dy, sum dy xhat with dy = dA where A > 0 (A == NULL: everywhere)
template <int C>
__global__ void __launch_bounds__(256) vftrain_bn_bwd_part_kernel(const float* __restrict__ dA, const float* __restrict__ A,
                                                                  const float* __restrict__ Z, const float* __restrict__ stat,
                                                                  long long n, double* __restrict__ parts) {
  constexpr int R = 256 / C;
  const int c = threadIdx.x % C, r = threadIdx.x / C;
  const long long r0 = (long long)blockIdx.x * VFT_CHUNK;
  const float m = stat[c], is = stat[64 + c];
  double v[2] = {0.0, 0.0};
  const int rows = (int)(n - r0 < VFT_CHUNK ? n - r0 : (long long)VFT_CHUNK);
#pragma unroll 4
  for (int j = r; j < rows; j += R) {
    const long long o = (r0 + j) * C + c;
    float dy = dA[o];
    if (A && !(A[o] > 0.f)) dy = 0.f;
    v[0] += (double)dy;
    v[1] += (double)dy * (double)((Z[o] - m) * is);
  }
  vft_block_combine<C, 2, double>(v, parts + (long long)blockIdx.x * 2 * C);
}

// grid (1), block 64: d gamma = sum dy xhat, d beta = sum dy, d conv bias = 0 exactly (a shift in front of batch
// statistics has no effect); coef = gamma invstd, mean(dy), mean(dy xhat)
__global__ void __launch_bounds__(64) vftrain_bn_bwd_final_kernel(const double* __restrict__ parts, int nparts, int C, long long n,
                                                                  const float* __restrict__ gamma, const float* __restrict__ stat,
                                                                  float* __restrict__ coef, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, float* __restrict__ dbias) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int p = 0; p < nparts; ++p) {
    s1 += parts[((long long)p * 2) * C + c];
    s2 += parts[((long long)p * 2 + 1) * C + c];
  }
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
  dbias[c] = 0.f;
  coef[c] = gamma[c] * stat[64 + c];
  coef[64 + c] = (float)(s1 / (double)n);
  coef[128 + c] = (float)(s2 / (double)n);
}

// dz = gamma invstd (dy - mean(dy) - xhat mean(dy xhat)), four channels per thread
template <int C>
__global__ void __launch_bounds__(256) vftrain_bn_bwd_apply_kernel(const float* __restrict__ dA, const float* __restrict__ A,
                                                                   const float* __restrict__ Z, const float* __restrict__ stat,
                                                                   const float* __restrict__ coef, float* __restrict__ dZ,
                                                                   long long total4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)((i * 4) % C);
  const float4 d4 = ldg4(dA + 4 * i), z4 = ldg4(Z + 4 * i);
  float4 a4 = make_float4(1.f, 1.f, 1.f, 1.f);
  if (A) a4 = ldg4(A + 4 * i);
  const float d[4] = {d4.x, d4.y, d4.z, d4.w}, z[4] = {z4.x, z4.y, z4.z, z4.w}, a[4] = {a4.x, a4.y, a4.z, a4.w};
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float dy = a[j] > 0.f ? d[j] : 0.f;
    const float xh = (z[j] - stat[c + j]) * stat[64 + c + j];
    o[j] = coef[c + j] * ((dy - coef[64 + c + j]) - xh * coef[128 + c + j]);
  }
  *reinterpret_cast<float4*>(dZ + 4 * i) = make_float4(o[0], o[1], o[2], o[3]);
}

// ------------------------------------------------------------------------------------------------
// the thin ends of the CNN's backward (VALU)
// ------------------------------------------------------------------------------------------------
// layer 8's data gradient: dA [B][F][W][64] = dZ8 [B][W][F][8] x W8 [8][64]; one thread per (position, four channels)
__global__ void __launch_bounds__(256) vftrain_conv8_dgrad_kernel(const float* __restrict__ dZ8, const float* __restrict__ w8,
                                                                  float* __restrict__ dA, long long total4, int F, int W) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)(i & 15) * 4;
  long long pos = i >> 4;
  const int x = (int)(pos % W);  pos /= W;
  const int f = (int)(pos % F);
  const long long b = pos / F;
  const float* g = dZ8 + ((b * W + x) * F + f) * 8;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int co = 0; co < 8; ++co) {
    const float gv = g[co];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaf(gv, w8[co * 64 + c + j], o[j]);
  }
  *reinterpret_cast<float4*>(dA + 4 * i) = make_float4(o[0], o[1], o[2], o[3]);
}

// layer 8's weight gradient, first stage: grid (ceil(pos / 1024)), block 256: parts[chunk][8][64] = sum dZ8[co] A[ci]
__global__ void __launch_bounds__(256) vftrain_conv8_wgrad_kernel(const float* __restrict__ dZ8, const float* __restrict__ A,
                                                                  float* __restrict__ parts, long long npos, int F, int W) {
  const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * VFT_CHUNK;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = r; j < VFT_CHUNK; j += 4) {
    long long pos = r0 + j;
    if (pos < npos) {
      const float a = A[pos * 64 + c];
      const int x = (int)(pos % W);  pos /= W;
      const int f = (int)(pos % F);
      const long long b = pos / F;
      const float* g = dZ8 + ((b * W + x) * F + f) * 8;
#pragma unroll
      for (int co = 0; co < 8; ++co) v[co] = fmaf(g[co], a, v[co]);
    }
  }
  vft_block_combine<64, 8, float>(v, parts + (long long)blockIdx.x * 8 * 64);
}

// layer 1's weight gradient, first stage: parts[chunk][7][64] = sum dZ1[pos][c] mix[row][x + k - 3]
__global__ void __launch_bounds__(256) vftrain_conv1_wgrad_kernel(const float* __restrict__ dZ1, const float* __restrict__ mix,
                                                                  float* __restrict__ parts, long long npos, int W) {
  const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * VFT_CHUNK;
  float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = r; j < VFT_CHUNK; j += 4) {
    const long long pos = r0 + j;
    if (pos < npos) {
      const float g = dZ1[pos * 64 + c];
      const int x = (int)(pos % W);
      const float* row = mix + (pos - x);
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const int ix = x + k - 3;
        if (ix >= 0 && ix < W) v[k] = fmaf(g, row[ix], v[k]);
      }
    }
  }
  vft_block_combine<64, 7, float>(v, parts + (long long)blockIdx.x * 7 * 64);
}

// second stage of both: the chunks in order, in double.  parts[chunk][NV][64] -> out[c * ld_c + i * ld_i]
__global__ void __launch_bounds__(256) vftrain_parts_sum_kernel(const float* __restrict__ parts, int nparts, int NV,
                                                                float* __restrict__ out, int ld_c, int ld_i) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= NV * 64) return;
  const int i = e >> 6, c = e & 63;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += (double)parts[(long long)p * NV * 64 + e];
  out[c * ld_c + i * ld_i] = (float)s;
}

// ------------------------------------------------------------------------------------------------
// the data gradient's weights: dst[(tap' * 64 + co) * 64 + ci] = w[(co * 64 + ci) * taps + (taps - 1 - tap')]: the taps
// flipped, Cin and Cout exchanged, in lipfe_conv_kernel's [tap][Cin][Cout] order.  grid (x, 6), block 256
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vftrain_pack_flip_kernel(LfPackSrc s, float* __restrict__ pack) {
  const int i = blockIdx.y, taps = s.taps[i];
  const float* __restrict__ src = s.w[i];
  float* __restrict__ dst = pack + s.off[i];
  const int n = taps * 64 * 64;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const int ci = e & 63, co = (e >> 6) & 63, tp = e >> 12;
    dst[e] = src[(co * 64 + ci) * taps + (taps - 1 - tp)];
  }
}

// ------------------------------------------------------------------------------------------------
// weight gradient of a 64 -> 64 convolution on fp32 MFMA: dW[tap][ci][co] = sum_pos X[pos + off(tap)][ci] dZ[pos][co]
// ------------------------------------------------------------------------------------------------
struct VftWgradArgs {
  const float* X;      // [B][F][W][64]: the layer's input
  const float* dZ;     // [B][F][W][64]: gradient of its raw output
  float* parts;        // [chunk][tap][64 ci][64 co]
  long long npos;
  int F, W, KH, KW, dil;
};

// grid (chunks, taps), block 256: a 64 (ci) x 64 (co) tile, wave w owns the 32 x 32 sub-tile (w & 1, w >> 1), as
// lipfe_conv_kernel; K is the chunk's 4096 positions in steps of 32.  Both operands are channel-last, so a step is 32 rows
// of 64 floats each, read 16 bytes per lane and stored to LDS as they are: [k = position][m = channel].  The padding is the
// index guard of X's loader.  A step's 32 products are summed on their own, then added to the running total.
__global__ void __launch_bounds__(256) vftrain_wgrad_kernel(VftWgradArgs p) {
  __shared__ __attribute__((aligned(16))) float As[LF_KC][LF_BM];
  __shared__ __attribute__((aligned(16))) float Bs[LF_KC][LF_BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 31, hh = lane >> 5, wm = wave & 1, wn = wave >> 1;
  const int tap = blockIdx.y;
  const int ky = tap / p.KW, kx = tap - ky * p.KW;
  const int dy = (ky - p.KH / 2) * p.dil, dx = kx - p.KW / 2;
  const long long p0 = (long long)blockIdx.x * VFT_WG_CHUNK;
  long long rem = p.npos - p0;
  const int nsteps = (int)((rem < VFT_WG_CHUNK ? rem : (long long)VFT_WG_CHUNK) + LF_KC - 1) / LF_KC;
  // loader: thread -> rows lr + 16 j (j < 2) of the step, channels 4 lq .. 4 lq + 3
  const int lr = tid >> 4, lq = tid & 15;
  float4 ra[2], rb[2];
  auto fetch = [&](int step) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long long pos = p0 + (long long)step * LF_KC + lr + 16 * j;
      ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      rb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pos < p.npos) {
        rb[j] = ldg4(p.dZ + pos * 64 + 4 * lq);
        const int x = (int)(pos % p.W);
        const int f = (int)((pos / p.W) % p.F);
        const int fy = f + dy, xx = x + dx;
        if (fy >= 0 && fy < p.F && xx >= 0 && xx < p.W) ra[j] = ldg4(p.X + (pos + (long long)dy * p.W + dx) * 64 + 4 * lq);
      }
    }
  };

  f32x16 acc = zero16();
  fetch(0);
  for (int step = 0; step < nsteps; ++step) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<float4*>(&As[lr + 16 * j][4 * lq]) = ra[j];
      *reinterpret_cast<float4*>(&Bs[lr + 16 * j][4 * lq]) = rb[j];
    }
    __syncthreads();
    if (step + 1 < nsteps) fetch(step + 1);
    f32x16 part = zero16();
#pragma unroll
    for (int kk = 0; kk < LF_KC / 2; ++kk)
      part = mfma32(As[2 * kk + hh][32 * wm + c], Bs[2 * kk + hh][32 * wn + c], part);
    acc += part;
    __syncthreads();
  }
  float* __restrict__ out = p.parts + ((long long)blockIdx.x * gridDim.y + tap) * 64 * 64;
  const int co = 32 * wn + c;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[(32 * wm + ROW32(r, hh)) * 64 + co] = acc[r];
}

// second launch: the chunks in order -> the reference's layout dW[co][ci][tap].  One thread per (tap, ci, co)
__global__ void __launch_bounds__(256) vftrain_wgrad_sum_kernel(const float* __restrict__ parts, int nchunks, int taps,
                                                                float* __restrict__ dW) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int n = taps * 64 * 64;
  if (e >= n) return;
  float s = 0.f;
  for (int k = 0; k < nchunks; ++k) s += parts[(long long)k * n + e];
  const int co = e & 63, ci = (e >> 6) & 63, tap = e >> 12;
  dW[(co * 64 + ci) * taps + tap] = s;
}

// ------------------------------------------------------------------------------------------------
// column sums of X [batch][rows][C] -> out [batch][C] (+ out2), the rows in a fixed order
// grid (ceil(C / 64), batches), block 256 = 4 row groups x 64 columns
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vftrain_colsum_kernel(const float* __restrict__ X, int rows, int C, long long batch_stride,
                                                             float* __restrict__ out, float* __restrict__ out2) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const float* __restrict__ x = X + (long long)blockIdx.y * batch_stride;
  float s = 0.f;
  if (c < C)
    for (int j = r; j < rows; j += 4) s += x[(long long)j * C + c];
  red[r][cl] = s;
  __syncthreads();
  if (r == 0 && c < C) {
    const float t = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
    out[(long long)blockIdx.y * C + c] = t;
    if (out2) out2[(long long)blockIdx.y * C + c] = t;
  }
}

// ------------------------------------------------------------------------------------------------
// pointwise pieces
// ------------------------------------------------------------------------------------------------
// Dropout2d on [2B][W][600] zeroes whole frames: keep[q][t] = 1 where rand >= thresh, one draw per (sequence, frame) with
// the counter q W + t; thresh = 0 keeps everything
__global__ void __launch_bounds__(256) vftrain_drop_mask_kernel(float* __restrict__ keep, int total, uint32_t seed, uint32_t thresh) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  keep[i] = drop_rand_q(drop_qseed(seed, (uint32_t)i), 0u) >= thresh ? 1.f : 0.f;
}

// y[row][:] = x[row][:] * keep[row] * inv_keep (the ReLU behind the dropout commutes with the non-negative scale)
__global__ void __launch_bounds__(256) vftrain_drop_apply_kernel(const float* __restrict__ x, const float* __restrict__ keep,
                                                                 float inv_keep, float* __restrict__ y, long long total, int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  y[i] = x[i] * (keep[i / C] * inv_keep);
}

// out[s][b][f][t] = S[q = s B + b][t][f] * mix[b][f][t]
__global__ void __launch_bounds__(256) vftrain_out_kernel(const float* __restrict__ S, const float* __restrict__ mix,
                                                          float* __restrict__ out1, float* __restrict__ out2, long long per_spk,
                                                          int F, int W) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * per_spk) return;
  const int s = i >= per_spk;
  const long long o = i - s * per_spk;             // (b, f, t)
  const int t = (int)(o % W);
  const int f = (int)((o / W) % F);
  const long long b = o / ((long long)W * F);
  const float v = S[((s * (per_spk / ((long long)W * F)) + b) * W + t) * F + f] * mix[o];
  (s ? out2 : out1)[o] = v;
}

// dP[q][t][f] = d_out[s][b][f][t] * mix[b][f][t] * S (1 - S)
__global__ void __launch_bounds__(256) vftrain_dsig_kernel(const float* __restrict__ d1, const float* __restrict__ d2,
                                                           const float* __restrict__ mix, const float* __restrict__ S,
                                                           float* __restrict__ dP, long long per_spk, int F, int W) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;     // index into dP / S: (q, t, f)
  if (i >= 2 * per_spk) return;
  const int f = (int)(i % F);
  const int t = (int)((i / F) % W);
  const long long q = i / ((long long)F * W);
  const long long B = per_spk / ((long long)W * F);
  const int s = q >= B;
  const long long b = q - s * B;
  const long long o = (b * F + f) * W + t;
  const float sg = S[i];
  dP[i] = (s ? d2 : d1)[o] * mix[o] * (sg * (1.f - sg));
}

// through the ReLU behind fc.1 and the dropout: d[row][:] *= keep[row] * inv_keep where y1[row][:] > 0, else 0
__global__ void __launch_bounds__(256) vftrain_drelu_drop_kernel(float* __restrict__ d, const float* __restrict__ y1,
                                                                 const float* __restrict__ keep, float inv_keep, long long total,
                                                                 int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  d[i] = y1[i] > 0.f ? d[i] * (keep[i / C] * inv_keep) : 0.f;
}

// out[i] = a[i] + b[i] (speaker 1, then speaker 2)
__global__ void __launch_bounds__(256) vftrain_add_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ out, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) out[i] = a[i] + b[i];
}

// dst[row * ld + col0 + c] += src[row * C + c]
__global__ void __launch_bounds__(256) vftrain_add_rows_kernel(float* __restrict__ dst, long long ld, const float* __restrict__ src,
                                                               int rows, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C) return;
  const int row = i / C, c = i - row * C;
  dst[(long long)row * ld + c] += src[i];
}

// viewT[(b W + t) * K8 + c] = flat[b K8 W + c W + t]: the view [B][8F][W] with its rows K-major, through a 32 x 32 LDS tile
// grid (ceil(W / 32), ceil(K8 / 32), B), block 256
__global__ void __launch_bounds__(256) vftrain_view_t_kernel(const float* __restrict__ flat, float* __restrict__ viewT, int K8, int W) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const long long b = blockIdx.z;
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, t = t0 + tx;
    tile[j][tx] = (c < K8 && t < W) ? flat[b * K8 * W + (long long)c * W + t] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int t = t0 + j, c = c0 + tx;
    if (t < W && c < K8) viewT[(b * W + t) * K8 + c] = tile[tx][j];
  }
}

// the two speakers' embeddings one behind the other: cat[s][b][t][e]
__global__ void __launch_bounds__(256) vftrain_cat_kernel(const float* __restrict__ e1, const float* __restrict__ e2,
                                                          float* __restrict__ cat, long long per_spk) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * per_spk) return;
  cat[i] = i < per_spk ? e1[i] : e2[i - per_spk];
}

// dst[j][k] = src[k][j] of a [rows][cols] matrix (W_hh of the LSTM for its backward step)
__global__ void __launch_bounds__(256) vftrain_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cols) return;
  const int k = i / rows, j = i - k * rows;     // dst index (k, j): k < cols, j < rows
  dst[i] = src[j * cols + k];
}

// ------------------------------------------------------------------------------------------------
// GRU with a tape: vfilt_gru_kernel that also stores r, z, n and W_hn h + b_hn of every step, [sequence][t][4F] per direction
// ------------------------------------------------------------------------------------------------
struct VftGruArgs {
  VfGruArgs g;
  float* tape[2];
};

__global__ void __launch_bounds__(1024) vftrain_gru_kernel(VftGruArgs a) {
  __shared__ float hs[VF_FMAX + 3];
  __shared__ float gh[3 * VF_FMAX + 1];
  const VfGruArgs& p = a.g;
  const int tid = threadIdx.x;
  const int q = blockIdx.x, d = blockIdx.y, F = p.F, G3 = 3 * p.F;
  const float* __restrict__ wt = p.whht[d] + tid;
  const float bh = tid < G3 ? p.bhh[d][tid] : 0.f;
  if (tid < F) hs[tid] = 0.f;
  __syncthreads();
  for (int s = 0; s < p.Tv; ++s) {
    const int t = d ? p.Tv - 1 - s : s;
    if (tid < G3) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int k = 0;
      for (; k + 4 <= F; k += 4) {
        a0 = fmaf(wt[(k + 0) * G3], hs[k + 0], a0);
        a1 = fmaf(wt[(k + 1) * G3], hs[k + 1], a1);
        a2 = fmaf(wt[(k + 2) * G3], hs[k + 2], a2);
        a3 = fmaf(wt[(k + 3) * G3], hs[k + 3], a3);
      }
      if (k < F) a0 = fmaf(wt[k * G3], hs[k], a0);
      if (k + 1 < F) a1 = fmaf(wt[(k + 1) * G3], hs[k + 1], a1);
      if (k + 2 < F) a2 = fmaf(wt[(k + 2) * G3], hs[k + 2], a2);
      gh[tid] = ((a0 + a1) + (a2 + a3)) + bh;
    }
    __syncthreads();
    if (tid < F) {
      const float* gi = p.gi[d] + ((long long)q * p.Tv + t) * G3;
      const float r = vf_sigmoid(gi[tid] + gh[tid]);
      const float zg = vf_sigmoid(gi[F + tid] + gh[F + tid]);
      const float ghn = gh[2 * F + tid];
      const float ng = tanhf(fmaf(r, ghn, gi[2 * F + tid]));
      const float h = fmaf(zg, hs[tid] - ng, ng);
      p.y[((long long)q * p.Tv + t) * p.ldy + d * F + tid] = h;
      float* tp = a.tape[d] + ((long long)q * p.Tv + t) * 4 * F + tid;
      tp[0] = r;  tp[F] = zg;  tp[2 * F] = ng;  tp[3 * F] = ghn;
      hs[tid] = h;
    }
    __syncthreads();
  }
}

// vfilt_gru_first_step_kernel with the tape [sequence][4F]
__global__ void __launch_bounds__(320) vftrain_gru_first_step_kernel(const float* __restrict__ gi, const float* __restrict__ bhh,
                                                                     float* __restrict__ y, long long y_stride, float* __restrict__ tape,
                                                                     int F) {
  const int u = threadIdx.x, q = blockIdx.x;
  if (u >= F) return;
  const float* g = gi + (long long)q * 3 * F;
  const float r = vf_sigmoid(g[u] + bhh[u]);
  const float zg = vf_sigmoid(g[F + u] + bhh[F + u]);
  const float ng = tanhf(fmaf(r, bhh[2 * F + u], g[2 * F + u]));
  y[q * y_stride + u] = ng - zg * ng;
  float* tp = tape + (long long)q * 4 * F + u;
  tp[0] = r;  tp[F] = zg;  tp[2 * F] = ng;  tp[3 * F] = bhh[2 * F + u];
}

// BPTT through one GRU recurrence: grid (sequences, directions), block 1024, one workgroup per (sequence, direction) as
// the forward.  Per step, in the reverse of the forward's order: dh = dy[t] + what came back from the step after it;
// d gi = (d a_r, d a_z, d a_n), d gh = (d a_r, d a_z, d a_n r), h_prev -> [sequence][t][3F], [3F], [F];
// dh for the step before = dh z + W_hh^T d gh (thread k walks column k of W_hh [3F][F]: coalesced as it is).
struct VftGruBwdArgs {
  const float* tape[2];   // [sequence][t][4F]
  const float* y;         // the forward's outputs, [sequence][t][ldy], direction d at column d F
  const float* dy;        // gradient of the outputs, [sequence][...]: element (q, t, d F + k) at dy[q * dy_sq + t * dy_st + d F + k]
  long long dy_sq, dy_st;
  int only_t;             // >= 0: dy is given for that step alone (dy_st unused), the others get none
  const float* whh[2];    // [3F][F]
  float* dgi[2];          // [sequence][t][3F]
  float* dgh[2];
  float* hprev[2];        // [sequence][t][F]
  int ldy, Tv, F;
};

__global__ void __launch_bounds__(1024) vftrain_gru_bwd_kernel(VftGruBwdArgs p) {
  __shared__ float dg[3 * VF_FMAX + 1];
  const int tid = threadIdx.x;
  const int q = blockIdx.x, d = blockIdx.y, F = p.F, G3 = 3 * p.F;
  const float* __restrict__ w = p.whh[d];
  float dhrec = 0.f;
  for (int s = p.Tv - 1; s >= 0; --s) {
    const int t = d ? p.Tv - 1 - s : s;
    const long long row = (long long)q * p.Tv + t;
    if (tid < F) {
      const float* tp = p.tape[d] + row * 4 * F + tid;
      const float r = tp[0], zg = tp[F], ng = tp[2 * F], ghn = tp[3 * F];
      const int tprev = d ? t + 1 : t - 1;
      const float hp = s > 0 ? p.y[((long long)q * p.Tv + tprev) * p.ldy + d * F + tid] : 0.f;
      float dh = dhrec;
      if (p.only_t < 0) dh += p.dy[q * p.dy_sq + t * p.dy_st + d * F + tid];
      else if (t == p.only_t) dh += p.dy[q * p.dy_sq + d * F + tid];
      const float dan = dh * (1.f - zg) * (1.f - ng * ng);
      const float daz = dh * (hp - ng) * (zg * (1.f - zg));
      const float dar = dan * ghn * (r * (1.f - r));
      float* gi = p.dgi[d] + row * G3 + tid;
      gi[0] = dar;  gi[F] = daz;  gi[2 * F] = dan;
      float* gh = p.dgh[d] + row * G3 + tid;
      gh[0] = dar;  gh[F] = daz;  gh[2 * F] = dan * r;
      p.hprev[d][row * F + tid] = hp;
      dg[tid] = dar;  dg[F + tid] = daz;  dg[2 * F + tid] = dan * r;
      dhrec = dh * zg;
    }
    __syncthreads();
    if (tid < F && s > 0) {
      float a0 = 0.f, a1 = 0.f;
      int j = 0;
      for (; j + 2 <= G3; j += 2) {
        a0 = fmaf(w[(long long)j * F + tid], dg[j], a0);
        a1 = fmaf(w[(long long)(j + 1) * F + tid], dg[j + 1], a1);
      }
      if (j < G3) a0 = fmaf(w[(long long)j * F + tid], dg[j], a0);
      dhrec += a0 + a1;
    }
    __syncthreads();
  }
}

// the backward of vftrain_gru_first_step_kernel (h_prev = 0): dh [sequence][ld] -> d gi, d gh [sequence][3F]
__global__ void __launch_bounds__(320) vftrain_gru_first_step_bwd_kernel(const float* __restrict__ tape, const float* __restrict__ dh,
                                                                         long long ld, float* __restrict__ dgi, float* __restrict__ dgh,
                                                                         int F) {
  const int u = threadIdx.x, q = blockIdx.x;
  if (u >= F) return;
  const float* tp = tape + (long long)q * 4 * F + u;
  const float r = tp[0], zg = tp[F], ng = tp[2 * F], ghn = tp[3 * F];
  const float d = dh[q * ld + u];
  const float dan = d * (1.f - zg) * (1.f - ng * ng);
  const float daz = d * (0.f - ng) * (zg * (1.f - zg));
  const float dar = dan * ghn * (r * (1.f - r));
  float* gi = dgi + (long long)q * 3 * F + u;
  gi[0] = dar;  gi[F] = daz;  gi[2 * F] = dan;
  float* gh = dgh + (long long)q * 3 * F + u;
  gh[0] = dar;  gh[F] = daz;  gh[2 * F] = dan * r;
}

// ------------------------------------------------------------------------------------------------
// the mask LSTM: vfilt_lstm_step_kernel that also stores the four gate activations and c of the step
// ------------------------------------------------------------------------------------------------
struct VftLstmArgs {
  VfLstmArgs l;
  float* gates;    // [sequence][t][1600]: i, f, g, o after their activations
  float* cell;     // [sequence][t][400]
  float* hprev;    // [sequence][t][400]: h of step t - 1 (zeros at t = 0), the operand of W_hh's gradient
};

template <int NQ>
__global__ void __launch_bounds__(256) vftrain_lstm_step_kernel(VftLstmArgs a) {
  __shared__ float hs[NQ][VF_H];
  const VfLstmArgs& p = a.l;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * NQ;
  for (int i = tid; i < NQ * VF_H; i += 256) {
    const int q = i / VF_H, k = i - q * VF_H;
    float v = 0.f;
    if (p.t > 0 && q0 + q < p.nseq) v = p.Hb[((long long)(q0 + q) * p.W + (p.t - 1)) * VF_H + k];
    hs[q][k] = v;
  }
  __syncthreads();
  const int u = blockIdx.x * 4 + wave;
  float acc[4][NQ];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[g][q] = 0.f;
  for (int k = lane; k < VF_H; k += 64) {
    float w[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) w[g] = p.whh[(long long)(g * VF_H + u) * VF_H + k];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float h = hs[q][k];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g][q] = fmaf(w[g], h, acc[g][q]);
    }
  }
  float mine[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float s = vf_wave_sum(acc[g][q]);
      if (lane == q) mine[g] = s;
    }
  const int qq = q0 + lane;
  if (lane >= NQ || qq >= p.nseq) return;
  const int item = qq % p.B;
  const float* G = p.G + ((long long)item * p.W + p.t) * VF_G + u;
  const float* D = p.D + (long long)qq * VF_G + u;
  const float gi = vf_sigmoid(mine[0] + G[0] + D[0]);
  const float gf = vf_sigmoid(mine[1] + G[VF_H] + D[VF_H]);
  const float gg = tanhf(mine[2] + G[2 * VF_H] + D[2 * VF_H]);
  const float go = vf_sigmoid(mine[3] + G[3 * VF_H] + D[3 * VF_H]);
  const long long row = (long long)qq * p.W + p.t;
  const float cprev = p.t > 0 ? a.cell[(row - 1) * VF_H + u] : 0.f;
  const float cn = fmaf(gf, cprev, gi * gg);
  a.cell[row * VF_H + u] = cn;
  float* gt = a.gates + row * VF_G + u;
  gt[0] = gi;  gt[VF_H] = gf;  gt[2 * VF_H] = gg;  gt[3 * VF_H] = go;
  a.hprev[row * VF_H + u] = hs[lane][u];
  p.Hb[row * VF_H + u] = go * tanhf(cn);
}

// One step of the LSTM's backward for all sequences, launched for t = W - 1 .. 0: grid (100, ceil(nseq / NQ)), block 256,
// a wave owns one hidden unit as in the forward.  dh_t = dH[t] where H[t] > 0 (the ReLU behind the LSTM) + W_hh^T dgates[t + 1]
// (row u of the transposed copy, the 1600 products spread over the lanes), then the cell's pointwise backward -> the
// pre-activation gate gradients dgates[q][t][1600]; dc lives in dcst [sequence][400], owned by the unit's wave.
struct VftLstmBwdArgs {
  const float* dH;      // [sequence][t][400]: the FC tail's data gradient
  const float* Hb;      // [sequence][t][400]
  const float* gates;   // [sequence][t][1600]
  const float* cell;    // [sequence][t][400]
  const float* whht;    // [400][1600]
  float* dgates;        // [sequence][t][1600]
  float* dcst;          // [sequence][400]
  int W, t, nseq;
};

template <int NQ>
__global__ void __launch_bounds__(256) vftrain_lstm_bwd_step_kernel(VftLstmBwdArgs p) {
  __shared__ float ds[NQ][VF_G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * NQ;
  const bool last = p.t == p.W - 1;
  if (!last) {
    for (int i = tid; i < NQ * VF_G; i += 256) {
      const int q = i / VF_G, j = i - q * VF_G;
      ds[q][j] = q0 + q < p.nseq ? p.dgates[((long long)(q0 + q) * p.W + (p.t + 1)) * VF_G + j] : 0.f;
    }
  }
  __syncthreads();
  const int u = blockIdx.x * 4 + wave;
  float mine = 0.f;
  if (!last) {
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
    const float* __restrict__ wr = p.whht + (long long)u * VF_G;
    for (int j = lane; j < VF_G; j += 64) {
      const float w = wr[j];
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = fmaf(w, ds[q][j], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float s = vf_wave_sum(acc[q]);
      if (lane == q) mine = s;
    }
  }
  const int qq = q0 + lane;
  if (lane >= NQ || qq >= p.nseq) return;
  const long long row = (long long)qq * p.W + p.t;
  const float h = p.Hb[row * VF_H + u];
  const float dh = (h > 0.f ? p.dH[row * VF_H + u] : 0.f) + mine;
  const float* gt = p.gates + row * VF_G + u;
  const float gi = gt[0], gf = gt[VF_H], gg = gt[2 * VF_H], go = gt[3 * VF_H];
  const float cn = p.cell[row * VF_H + u];
  const float cprev = p.t > 0 ? p.cell[(row - 1) * VF_H + u] : 0.f;
  const float tc = tanhf(cn);
  const float dc = (last ? 0.f : p.dcst[(long long)qq * VF_H + u]) + dh * go * (1.f - tc * tc);
  float* dg = p.dgates + row * VF_G + u;
  dg[0] = dc * gg * (gi * (1.f - gi));
  dg[VF_H] = dc * cprev * (gf * (1.f - gf));
  dg[2 * VF_H] = dc * gi * (1.f - gg * gg);
  dg[3 * VF_H] = dh * tc * (go * (1.f - go));
  p.dcst[(long long)qq * VF_H + u] = dc * gf;
}

}  // namespace
