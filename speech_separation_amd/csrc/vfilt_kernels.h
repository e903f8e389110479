// vfilt_kernels.h -- device code of the VoiceFilter separator (vfilt.hip) that is its own: BatchNorm folding with the conv
// bias, the two thin ends of the CNN (1 -> 64 and 64 -> 8) on plain VALU, a strided GEMM on fp32 MFMA for every dense
// product (GRU and LSTM input projections, d-vector, FC tail), the GRU recurrence and the LSTM step.  The 64 -> 64
// convolutions run on lipfe_kernels.h's implicit-GEMM kernel.
//
// Every output element is one fixed-order sum that depends on its own item only: no atomics, no split-K.  No workgroup
// waits for another one inside a kernel: the LSTM's time steps are separate launches.
#pragma once
#include "lipfe_kernels.h"

namespace {

constexpr int VF_LAYERS = 8;      // Conv2d + BatchNorm2d pairs
constexpr int VF_C = 64;          // channels of the CNN's trunk
constexpr int VF_C8 = 8;          // channels of its last layer
constexpr int VF_H = 400;         // LSTM hidden size
constexpr int VF_G = 4 * VF_H;    // LSTM gate rows
constexpr int VF_FC = 600;        // width of the FC tail
constexpr int VF_FMAX = 257;      // largest input_size

DEV float vf_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// sum over the 64 lanes of a wave, the same value in every lane; all lanes must be active
DEV float vf_wave_sum(float v) { return half_sum(group_sum<32>(v)); }

// ------------------------------------------------------------------------------------------------
// eval-mode BatchNorm with the conv bias folded in: y = conv * scale + shift
// ------------------------------------------------------------------------------------------------
struct VfFoldSrc {
  const float* cb[VF_LAYERS];   // conv bias
  const float* w[VF_LAYERS];    // bn weight, bias, running_mean, running_var
  const float* b[VF_LAYERS];
  const float* m[VF_LAYERS];
  const float* v[VF_LAYERS];
  int C[VF_LAYERS];
};

// grid (8), block 64: fold[l] = scale[64] then shift[64] at float 128 l
__global__ void __launch_bounds__(64) vfilt_fold_kernel(VfFoldSrc s, float* __restrict__ fold) {
  const int l = blockIdx.x, c = threadIdx.x;
  if (c >= s.C[l]) return;
  const float sc = s.w[l][c] / sqrtf(s.v[l][c] + LF_BN_EPS);
  fold[128 * l + c] = sc;
  fold[128 * l + 64 + c] = fmaf(s.cb[l][c] - s.m[l][c], sc, s.b[l][c]);
}

// ------------------------------------------------------------------------------------------------
// layer 1: Conv2d(1, 64, (1, 7)), zero padding 3 along W, + BN + ReLU: mix [B][F][W] -> [B][F][W][64]
// one thread per (position, channel); the 7 taps are summed in order
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vfilt_conv1_kernel(const float* __restrict__ mix, const float* __restrict__ w1,
                                                          const float* __restrict__ fold, float* __restrict__ out, long long total,
                                                          int W) {
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
  out[i] = fmaxf(fmaf(s, fold[c], fold[64 + c]), 0.f);
}

// ------------------------------------------------------------------------------------------------
// layer 8: Conv2d(64, 8, 1) + BN, written as the reference's permute(0, 3, 2, 1).contiguous(): [B][F][W][64] -> [B][W][F][8]
// one thread per (position, output channel); the 64 inputs are summed in order
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vfilt_conv8_kernel(const float* __restrict__ in, const float* __restrict__ w8,
                                                          const float* __restrict__ fold, float* __restrict__ flat, long long total,
                                                          int F, int W) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i & 7);
  long long pos = i >> 3;
  const float* src = in + pos * 64;
  const int x = (int)(pos % W);  pos /= W;
  const int f = (int)(pos % F);
  const long long b = pos / F;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float4 v = ldg4(src + 4 * q);
    const float* wr = w8 + c * 64 + 4 * q;
    s = fmaf(v.x, wr[0], s);  s = fmaf(v.y, wr[1], s);  s = fmaf(v.z, wr[2], s);  s = fmaf(v.w, wr[3], s);
  }
  flat[((b * W + x) * F + f) * 8 + c] = fmaf(s, fold[c], fold[64 + c]);
}

// ------------------------------------------------------------------------------------------------
// strided, batched GEMM on fp32 MFMA: C(m, n) = act(sum_k A(m, k) B(k, n) + bias[n] + bias2[n]) * mul(m, n)
// ------------------------------------------------------------------------------------------------
constexpr int VF_ACT_NONE = 0, VF_ACT_RELU = 1, VF_ACT_SIGMOID = 2;

struct VfGemmArgs {
  const float* A;  long long sam, sak, sab;    // A(m, k) of batch z: A[z * sab + m * sam + k * sak]
  const float* Bw; long long sbn, sbk;         // B(k, n): Bw[n * sbn + k * sbk], shared by the batches
  const float* bias;                           // per n, or NULL
  const float* bias2;                          // per n, or NULL
  const float* mul;                            // indexed as C, or NULL
  float* C;        long long scm, scn, scb;    // C[z * scb + m * scm + n * scn]
  int M, N, K, mtiles;
  int relu_a;                                  // ReLU on A's elements as they are loaded
  int act;
};

// grid (mtiles * batches, ceil(N / 64)), block 256: wave w owns the 32 x 32 sub-tile (w & 1, w >> 1) of a 64 x 64 tile, as
// lipfe_conv_kernel, with the same LDS layout and the same two-level sum (32 products on their own, then the total).
// Neither operand needs an alignment or a multiple of anything: every load is one guarded scalar, and the thread ->
// element map follows whichever index is contiguous in memory.
__global__ void __launch_bounds__(256) vfilt_gemm_kernel(VfGemmArgs p) {
  __shared__ float As[LF_KC][LF_LDA];
  __shared__ float Bs[LF_KC][LF_LDA];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 31, hh = lane >> 5, wm = wave & 1, wn = wave >> 1;
  const long long z = blockIdx.x / p.mtiles;
  const int m0 = (int)(blockIdx.x % p.mtiles) * LF_BM, n0 = blockIdx.y * LF_BN;
  const float* __restrict__ A = p.A + z * p.sab;
  const bool a_kfast = p.sak == 1, b_kfast = p.sbk == 1;
  // element j of a thread: k fastest -> (k = tid & 31, row = (tid >> 5) + 8 j); row fastest -> (row = tid & 63, k = (tid >> 6) + 4 j)
  const int ak = a_kfast ? (tid & 31) : (tid >> 6), am = a_kfast ? (tid >> 5) : (tid & 63);
  const int adk = a_kfast ? 0 : 4, adm = a_kfast ? 8 : 0;
  const int bk = b_kfast ? (tid & 31) : (tid >> 6), bn = b_kfast ? (tid >> 5) : (tid & 63);
  const int bdk = b_kfast ? 0 : 4, bdn = b_kfast ? 8 : 0;

  const int nsteps = (p.K + LF_KC - 1) / LF_KC;
  float ra[8], rb[8];
  auto fetch = [&](int step) {
    const int k0 = step * LF_KC;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + ak + adk * j, m = m0 + am + adm * j;
      float v = 0.f;
      if (k < p.K && m < p.M) v = A[m * p.sam + k * p.sak];
      ra[j] = p.relu_a ? fmaxf(v, 0.f) : v;
      const int kb = k0 + bk + bdk * j, n = n0 + bn + bdn * j;
      rb[j] = (kb < p.K && n < p.N) ? p.Bw[n * p.sbn + kb * p.sbk] : 0.f;
    }
  };

  f32x16 acc = zero16();
  fetch(0);
  for (int step = 0; step < nsteps; ++step) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      As[ak + adk * j][am + adm * j] = ra[j];
      Bs[bk + bdk * j][bn + bdn * j] = rb[j];
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

  const int n = n0 + 32 * wn + c;
  if (n >= p.N) return;
  float add = 0.f;
  if (p.bias) add = p.bias[n];
  if (p.bias2) add += p.bias2[n];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + 32 * wm + ROW32(r, hh);
    if (m < p.M) {
      float v = acc[r] + add;
      if (p.act == VF_ACT_RELU) v = fmaxf(v, 0.f);
      else if (p.act == VF_ACT_SIGMOID) v = vf_sigmoid(v);
      const long long o = z * p.scb + m * p.scm + n * p.scn;
      if (p.mul) v *= p.mul[o];
      p.C[o] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// GRU recurrence (gate order r, z, n; b_hn inside the r term), one workgroup per (sequence, direction), zero initial state
// ------------------------------------------------------------------------------------------------
struct VfGruArgs {
  const float* gi[2];    // per direction: x W_ih^T + b_ih, [sequence][t][3F]
  const float* whht[2];  // W_hh transposed, [F][3F] (vfilt_transpose_kernel)
  const float* bhh[2];   // [3F]
  float* y;              // [sequence][t][ldy]: direction d writes columns d F .. d F + F - 1
  int ldy, Tv, F;
};

struct VfTransposeSrc {
  const float* w[3];     // [3F][F]
};

// grid (ceil(3F F / 256), 3), block 256: dst[i][k][j] = w[i][j][k].  Made in every forward, as the other derived copies.
__global__ void __launch_bounds__(256) vfilt_transpose_kernel(VfTransposeSrc s, float* __restrict__ dst, int F) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = 3 * F * F;
  if (i >= n) return;
  const int k = i / (3 * F), j = i - k * 3 * F;
  dst[(long long)blockIdx.y * n + i] = s.w[blockIdx.y][j * F + k];
}

// grid (sequences, directions), block 1024; direction 1 walks t = Tv - 1 .. 0.  Thread j owns gate row j (3F <= 771): it
// walks the F products of its row with h broadcast from LDS and the transposed weights read coalesced, four independent
// partial sums (k mod 4) that are added at the end: the loads do not wait for one another, and the order is fixed.
__global__ void __launch_bounds__(1024) vfilt_gru_kernel(VfGruArgs p) {
  __shared__ float hs[VF_FMAX + 3];
  __shared__ float gh[3 * VF_FMAX + 1];
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
      const float ng = tanhf(fmaf(r, gh[2 * F + tid], gi[2 * F + tid]));
      const float h = fmaf(zg, hs[tid] - ng, ng);          // (1 - z) n + z h
      p.y[((long long)q * p.Tv + t) * p.ldy + d * F + tid] = h;
      hs[tid] = h;                                          // read by this thread alone until the barrier below
    }
    __syncthreads();
  }
}

// One GRU step from the zero state (the backward direction of layer 2 at the last position, the only one that
// gru_out[:, -1, :] reads): W_hh meets zeros, so only b_hh remains.  grid (sequences), block 320
__global__ void __launch_bounds__(320) vfilt_gru_first_step_kernel(const float* __restrict__ gi, const float* __restrict__ bhh,
                                                                   float* __restrict__ y, long long y_stride, int F) {
  const int u = threadIdx.x, q = blockIdx.x;
  if (u >= F) return;
  const float* g = gi + (long long)q * 3 * F;
  const float r = vf_sigmoid(g[u] + bhh[u]);
  const float zg = vf_sigmoid(g[F + u] + bhh[F + u]);
  const float ng = tanhf(fmaf(r, bhh[2 * F + u], g[2 * F + u]));
  y[q * y_stride + u] = ng - zg * ng;
}

// ------------------------------------------------------------------------------------------------
// one time step of the mask LSTM (gate order i, f, g, o) for all sequences
// ------------------------------------------------------------------------------------------------
struct VfLstmArgs {
  const float* G;      // [item][t][1600]: the map's part of x W_ih^T, shared by the item's two speakers
  const float* D;      // [sequence][1600]: the d-vector's part + b_ih + b_hh, constant over time
  const float* whh;    // [1600][400]
  float* Hb;           // [sequence][t][400]: h of every step; step t reads row t - 1
  float* cst;          // [sequence][400]
  int B, W, t, nseq;   // sequence = speaker * B + item
};

// grid (100, ceil(nseq / NQ)), block 256: a wave owns one hidden unit (its four gate rows) for NQ sequences.  The 64 lanes
// stride over the 400 products of a row, the partial sums are added across the wave, and lane q finishes sequence q.
template <int NQ>
__global__ void __launch_bounds__(256) vfilt_lstm_step_kernel(VfLstmArgs p) {
  __shared__ float hs[NQ][VF_H];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * NQ;
  for (int i = tid; i < NQ * VF_H; i += 256) {
    const int q = i / VF_H, k = i - q * VF_H;
    float v = 0.f;
    if (p.t > 0 && q0 + q < p.nseq) v = p.Hb[((long long)(q0 + q) * p.W + (p.t - 1)) * VF_H + k];
    hs[q][k] = v;
  }
  __syncthreads();
  const int u = blockIdx.x * 4 + wave;     // < 400: the grid is exactly 100 x 4 units
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
  const float cprev = p.t > 0 ? p.cst[(long long)qq * VF_H + u] : 0.f;
  const float cn = fmaf(gf, cprev, gi * gg);
  p.cst[(long long)qq * VF_H + u] = cn;
  p.Hb[((long long)qq * p.W + p.t) * VF_H + u] = go * tanhf(cn);
}

}  // namespace
