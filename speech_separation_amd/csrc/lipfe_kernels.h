// lipfe_kernels.h -- device code of the lip-reading front end (lipfe.hip): the ResNet-18 trunk's 3x3 / 1x1 convolutions as
// implicit GEMMs on fp32 MFMA, the average pool, the per-forward copy of the weights in K-major order, and the 64-channel
// instantiations of lipfront.h's BatchNorm fold, Conv3d stem and max-pool.
//
// Activations are channel-last: [frame n = s*T + t][y][x][C].  Every output element is one fixed-order sum that depends on
// its own stream only: no atomics, no split-K, so results do not depend on the batch a stream runs in.
#pragma once
#include "lipfront.h"

namespace {

constexpr int LF_MAX_CONVS = 20;   // 16 block convs, 3 downsample convs, the stem

// ------------------------------------------------------------------------------------------------
// derived copies, made in every forward
// ------------------------------------------------------------------------------------------------
// grid (n_bn), block 256
__global__ void __launch_bounds__(256) lipfe_fold_kernel(LfFoldSrc s, float* __restrict__ fold) { lf_fold(s, fold); }

struct LfPackSrc {
  const float* w[LF_MAX_CONVS];   // [Cout][Cin][taps]
  int cin[LF_MAX_CONVS], cout[LF_MAX_CONVS], taps[LF_MAX_CONVS];
  long long off[LF_MAX_CONVS];    // floats into the pack buffer: [tap][Cin][Cout]
};

// grid (x, n_conv), block 256: dst[(tap*Cin + ci)*Cout + co] = src[(co*Cin + ci)*taps + tap].  A 32 (k) x 32 (co) tile goes
// through LDS so that both sides move whole rows.
__global__ void __launch_bounds__(256) lipfe_pack_kernel(LfPackSrc s, float* __restrict__ pack) {
  __shared__ float tile[32][33];
  const int i = blockIdx.y;
  const int cin = s.cin[i], cout = s.cout[i], taps = s.taps[i];
  const int R = cin * taps;                        // row length of the source
  const float* __restrict__ src = s.w[i];
  float* __restrict__ dst = pack + s.off[i];
  const int tr = (R + 31) / 32, tc = cout / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int t = blockIdx.x; t < tr * tc; t += gridDim.x) {
    const int r0 = (t % tr) * 32, co0 = (t / tr) * 32;
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
      const int r = r0 + tx;
      tile[j][tx] = r < R ? src[(long long)(co0 + j) * R + r] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
      const int r = r0 + j;          // source column r = ci*taps + tap
      if (r < R) {
        const int ci = r / taps, tap = r - ci * taps;
        dst[((long long)tap * cin + ci) * cout + co0 + tx] = tile[tx][j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// stem Conv3d(1 -> 64) + BN + activation -> pre [N][Hs][Ws][64] and the max-pool behind it: lipfront.h's bodies for 64 channels,
// lane c of a wave one output channel at 16 x positions; wpk is [245][64]
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lipfe_stem_kernel(LfStemArgs p) { lf_stem<64, 64>(p); }

__global__ void __launch_bounds__(256) lipfe_maxpool_kernel(const float* __restrict__ pre, float* __restrict__ out, long long total4,
                                                            int Hs, int Ws, int Hp, int Wp) {
  lf_maxpool<64>(pre, out, total4, Hs, Ws, Hp, Wp);
}

// ------------------------------------------------------------------------------------------------
// trunk convolution as an implicit GEMM: M = (frame, oy, ox), N = Cout, K = taps x Cin
// ------------------------------------------------------------------------------------------------
constexpr int LF_BM = 64, LF_BN = 64, LF_KC = 32;
constexpr int LF_LDA = LF_BM + 2;    // A is held K-major in LDS ([k][m]); + 2: a 32-lane group's scalar stores meet at most two to a bank

struct LfConvArgs {
  const float* in;       // [N][Hi][Wi][Cin]
  const float* wpk;      // [taps][Cin][Cout]
  const float* scale;    // folded BN: scale[Cout], shift[Cout] behind it
  const float* slope;    // PReLU slopes or NULL
  const float* res;      // residual [M][Cout] or NULL
  float* out;            // [M][Cout]
  long long M;
  int Hi, Wi, Ho, Wo, Cin, Cout, stride, act;
  int dil;               // row dilation (the taps of a column are dil rows apart); columns are never dilated
};

// KH x KW taps, zero padding (KH / 2) * dil rows and KW / 2 columns: 3 x 3 and 1 x 1 here, 7 x 1 and dilated 5 x 5 in
// vfilt.hip.  grid (ceil(M / 64), Cout / 64), block 256: wave w owns the 32 x 32 sub-tile (w & 1, w >> 1).
// One K step is 32 input channels of one tap: the next step's global loads are in flight while this one's MFMAs run.
// Each step's 32 products are summed on their own and then added to the running total: with K up to 4608 one running
// fp32 sum would carry about sqrt(K / 24) ulp of rounding error, the two levels about a quarter of that.
template <int KH, int KW>
__global__ void __launch_bounds__(256) lipfe_conv_kernel(LfConvArgs p) {
  __shared__ float As[LF_KC][LF_LDA];
  __shared__ __attribute__((aligned(16))) float Bs[LF_KC][LF_BN];
  constexpr int PADY = KH / 2, PADX = KW / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 31, hh = lane >> 5, wm = wave & 1, wn = wave >> 1;
  const long long m0 = (long long)blockIdx.x * LF_BM;
  const int n0 = blockIdx.y * LF_BN;

  // A loader: thread -> positions ap + 32 j (j < 2), channels 4 aq .. 4 aq + 3 of the step's 32
  const int ap = tid >> 3, aq = tid & 7;
  long long a_base[2];   // element offset of (frame, 0, 0, 0)
  int a_y[2], a_x[2];    // top-left input coordinate of the window; a_y = INT_MIN/2 for rows past M
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    long long m = m0 + ap + 32 * j;
    if (m < p.M) {
      const int ox = (int)(m % p.Wo);  m /= p.Wo;
      const int oy = (int)(m % p.Ho);  m /= p.Ho;
      a_base[j] = m * p.Hi * p.Wi * p.Cin;
      a_y[j] = oy * p.stride - PADY * p.dil;
      a_x[j] = ox * p.stride - PADX;
    } else {
      a_base[j] = 0;
      a_y[j] = -(1 << 20);
      a_x[j] = 0;
    }
  }
  // B loader: thread -> rows bk + 16 j, columns 4 bq .. 4 bq + 3
  const int bk = tid >> 4, bq = tid & 15;

  const int csteps = p.Cin / LF_KC, nsteps = KH * KW * csteps;
  float4 ra[2], rb[2];
  auto fetch = [&](int step) {
    const int tap = step / csteps, c0 = (step - tap * csteps) * LF_KC;
    const int ky = tap / KW, kx = tap - ky * KW;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int iy = a_y[j] + ky * p.dil, ix = a_x[j] + kx;
      ra[j] = (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi)
                  ? ldg4(p.in + a_base[j] + ((long long)iy * p.Wi + ix) * p.Cin + c0 + 4 * aq)
                  : make_float4(0.f, 0.f, 0.f, 0.f);
      rb[j] = ldg4(p.wpk + ((long long)tap * p.Cin + c0 + bk + 16 * j) * p.Cout + n0 + 4 * bq);
    }
  };

  f32x16 acc = zero16();
  fetch(0);
  for (int step = 0; step < nsteps; ++step) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      As[4 * aq + 0][ap + 32 * j] = ra[j].x;
      As[4 * aq + 1][ap + 32 * j] = ra[j].y;
      As[4 * aq + 2][ap + 32 * j] = ra[j].z;
      As[4 * aq + 3][ap + 32 * j] = ra[j].w;
      *reinterpret_cast<float4*>(&Bs[bk + 16 * j][4 * bq]) = rb[j];
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

  const int col = n0 + 32 * wn + c;
  const float sc = p.scale[col], sh = p.scale[p.Cout + col], sl = p.slope ? p.slope[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long m = m0 + 32 * wm + ROW32(r, hh);
    if (m < p.M) {
      float v = fmaf(acc[r], sc, sh);
      if (p.res) v += p.res[m * p.Cout + col];
      p.out[m * p.Cout + col] = lf_act(v, p.act, sl);
    }
  }
}

// AdaptiveAvgPool2d(1): [N][P][512] -> [N][512], one thread per (frame, channel), positions summed in order
__global__ void __launch_bounds__(256) lipfe_avgpool_kernel(const float* __restrict__ in, float* __restrict__ out, long long total, int P) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long n = i >> 9;
  const int ch = (int)(i & 511);
  const float* src = in + n * P * 512 + ch;
  float s = 0.f;
  for (int q = 0; q < P; ++q) s += src[(long long)q * 512];
  out[i] = s / (float)P;
}

}  // namespace
