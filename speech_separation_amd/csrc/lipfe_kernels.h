// lipfe_kernels.h -- device code of the lip-reading front end (lipfe.hip): Conv3d stem, max-pool, the ResNet-18 trunk's
// 3x3 / 1x1 convolutions as implicit GEMMs on fp32 MFMA, the average pool, and the per-forward derived copies (weights in
// K-major order, eval-mode BatchNorm folded to scale / shift).
//
// Activations are channel-last: [frame n = s*T + t][y][x][C].  Every output element is one fixed-order sum that depends on
// its own stream only: no atomics, no split-K, so results do not depend on the batch a stream runs in.
#pragma once
#include "common.h"

namespace {

constexpr int LF_ACT_NONE = -1, LF_ACT_RELU = 0, LF_ACT_PRELU = 1, LF_ACT_SWISH = 2;
constexpr int LF_MAX_CONVS = 20;   // 16 block convs, 3 downsample convs, the stem
constexpr int LF_MAX_BNS = 20;
constexpr float LF_BN_EPS = 1e-5f;

DEV float lf_act(float v, int act, float slope) {
  if (act == LF_ACT_RELU) return fmaxf(v, 0.f);
  if (act == LF_ACT_PRELU) return v >= 0.f ? v : slope * v;
  if (act == LF_ACT_SWISH) return v * (1.0f / (1.0f + expf(-v)));
  return v;
}

// ------------------------------------------------------------------------------------------------
// derived copies, made in every forward
// ------------------------------------------------------------------------------------------------
struct LfFoldSrc {
  const float* w[LF_MAX_BNS];   // weight, bias, running_mean, running_var
  const float* b[LF_MAX_BNS];
  const float* m[LF_MAX_BNS];
  const float* v[LF_MAX_BNS];
  int C[LF_MAX_BNS];
  int off[LF_MAX_BNS];          // floats into the fold buffer: scale[C] then shift[C]
};

// grid (n_bn), block 256
__global__ void __launch_bounds__(256) lipfe_fold_kernel(LfFoldSrc s, float* __restrict__ fold) {
  const int i = blockIdx.x, C = s.C[i];
  float* scale = fold + s.off[i];
  float* shift = scale + C;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float sc = s.w[i][c] / sqrtf(s.v[i][c] + LF_BN_EPS);
    scale[c] = sc;
    shift[c] = s.b[i][c] - s.m[i][c] * sc;
  }
}

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
// stem: Conv3d(1 -> 64, (5,7,7), stride (1,2,2), pad (2,3,3)) + BN + activation  ->  pre [N][Hs][Ws][64]
// ------------------------------------------------------------------------------------------------
constexpr int LF_STX = 16, LF_STY = 4;                  // output tile of one workgroup
constexpr int LF_PR = 2 * LF_STY + 5, LF_PC = 40;       // input patch rows, padded row length (37 used)

struct LfStemArgs {
  const float* x;        // [S][T][Hin][Win]
  const float* wpk;      // [245][64]
  const float* scale;    // folded BN: scale[64], shift[64] behind it
  const float* slope;    // PReLU slopes or NULL
  float* pre;
  int T, Hin, Win, y0, x0, H, W, Hs, Ws, tiles_x, tiles_y, act;
  float a, b;
};

// grid (tiles_x * tiles_y * N), block 256: wave g computes row g of the tile, lane c one output channel at 16 x positions.
__global__ void __launch_bounds__(256) lipfe_stem_kernel(LfStemArgs p) {
  __shared__ __attribute__((aligned(16))) float patch[5][LF_PR][LF_PC];
  __shared__ float ws[49][64];
  const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
  long long wg = blockIdx.x;
  const int tx = (int)(wg % p.tiles_x);  wg /= p.tiles_x;
  const int ty = (int)(wg % p.tiles_y);  wg /= p.tiles_y;
  const long long n = wg;                  // frame s*T + t
  const int t = (int)(n % p.T);
  const int oy0 = ty * LF_STY, ox0 = tx * LF_STX;
  const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
  for (int i = tid; i < 5 * LF_PR * LF_PC; i += 256) {
    const int col = i % LF_PC, r = (i / LF_PC) % LF_PR, kt = i / (LF_PC * LF_PR);
    const int tt = t + kt - 2, iy = iy0 + r, ix = ix0 + col;
    float v = 0.f;     // padding is zero in the normalised domain
    if (col < 37 && tt >= 0 && tt < p.T && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
      v = fmaf(p.a, p.x[((n + (kt - 2)) * p.Hin + (p.y0 + iy)) * p.Win + (p.x0 + ix)], p.b);
    patch[kt][r][col] = v;
  }
  float tot[LF_STX], acc[LF_STX];     // the 49 taps of a frame are summed on their own, then the five frames
#pragma unroll
  for (int i = 0; i < LF_STX; ++i) tot[i] = 0.f;
  for (int kt = 0; kt < 5; ++kt) {
    __syncthreads();
    for (int i = tid; i < 49 * 64; i += 256) ws[i >> 6][i & 63] = p.wpk[kt * 49 * 64 + i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LF_STX; ++i) acc[i] = 0.f;
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
      float row[LF_PC];
      const float4* src = reinterpret_cast<const float4*>(&patch[kt][2 * g + ky][0]);
#pragma unroll
      for (int i = 0; i < LF_PC / 4; ++i) {
        const float4 q = src[i];
        row[4 * i] = q.x;  row[4 * i + 1] = q.y;  row[4 * i + 2] = q.z;  row[4 * i + 3] = q.w;
      }
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const float w = ws[ky * 7 + kx][c];
#pragma unroll
        for (int i = 0; i < LF_STX; ++i) acc[i] = fmaf(row[2 * i + kx], w, acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < LF_STX; ++i) tot[i] += acc[i];
  }
  const int oy = oy0 + g;
  if (oy >= p.Hs) return;
  const float sc = p.scale[c], sh = p.scale[64 + c], sl = p.slope ? p.slope[c] : 0.f;
  float* out = p.pre + ((n * p.Hs + oy) * p.Ws + ox0) * 64 + c;
#pragma unroll
  for (int i = 0; i < LF_STX; ++i)
    if (ox0 + i < p.Ws) out[(long long)i * 64] = lf_act(fmaf(tot[i], sc, sh), p.act, sl);
}

// MaxPool (3,3) stride 2 pad 1 over [N][Hs][Ws][64] -> [N][Hp][Wp][64]; the padding is -inf, i.e. left out of the maximum.
// One thread per 4 channels of an output position.
__global__ void __launch_bounds__(256) lipfe_maxpool_kernel(const float* __restrict__ pre, float* __restrict__ out, long long total4,
                                                            int Hs, int Ws, int Hp, int Wp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c4 = (int)(i & 15);
  long long pos = i >> 4;
  const int px = (int)(pos % Wp);  pos /= Wp;
  const int py = (int)(pos % Hp);
  const long long n = pos / Hp;
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  for (int dy = -1; dy <= 1; ++dy) {
    const int y = 2 * py + dy;
    if (y < 0 || y >= Hs) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int x = 2 * px + dx;
      if (x < 0 || x >= Ws) continue;
      const float4 v = ldg4(pre + ((n * Hs + y) * Ws + x) * 64 + 4 * c4);
      m.x = fmaxf(m.x, v.x);  m.y = fmaxf(m.y, v.y);  m.z = fmaxf(m.z, v.z);  m.w = fmaxf(m.w, v.w);
    }
  }
  *reinterpret_cast<float4*>(out + i * 4) = m;
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
