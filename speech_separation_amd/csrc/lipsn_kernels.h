// lipsn_kernels.h -- device code of the ShuffleNet-v2 lip reader (lipsn.hip): one fused kernel per InvertedResidual block
// (pointwise -> depthwise 3 x 3 -> pointwise with the block's intermediates in LDS, concat + channel shuffle as a store
// index), conv_last + ReLU + AvgPool2d(3) in one kernel, the per-forward copy of the weights (K-major, zero-padded), and the
// 24-channel instantiations of lipfront.h's BatchNorm fold, Conv3d stem and max-pool.
//
// Activations are channel-last: [frame n = s*T + t][y][x][C].  Every output element is one fixed-order sum over its own
// frame's values: no atomics, no split-K.  Frames that share an MFMA tile occupy different ROWS of it, and a row's sum reads
// nothing of the other rows, so a stream's result does not depend on its batch.
#pragma once
#include "lipfe_kernels.h"

namespace {

constexpr int SN_STEM_C = 24, SN_STEM_CP = 32;   // stem channels, padded to the lane group that computes them
constexpr int SN_MAX_PACKS = 64;                 // 13 x 3 + 3 x 5 block convs, conv_last, the stem

// ------------------------------------------------------------------------------------------------
// derived copies, made in every forward
// ------------------------------------------------------------------------------------------------
// grid (n_bn), block 256
__global__ void __launch_bounds__(256) lipsn_fold_kernel(LfFoldSrc s, float* __restrict__ fold) { lf_fold(s, fold); }

struct SnPackSrc {
  const float* w[SN_MAX_PACKS];   // [Cout][K]: pointwise K = Cin, depthwise K = 9, stem K = 245
  int K[SN_MAX_PACKS], cout[SN_MAX_PACKS], np[SN_MAX_PACKS];
  int off[SN_MAX_PACKS];          // floats into the pack buffer: [K][np], columns cout .. np - 1 zero
};

// grid (x, n_pack), block 256: dst[k * np + co] = co < cout ? src[co * K + k] : 0
__global__ void __launch_bounds__(256) lipsn_pack_kernel(SnPackSrc s, float* __restrict__ pack) {
  const int j = blockIdx.y, K = s.K[j], cout = s.cout[j], np = s.np[j];
  const float* __restrict__ src = s.w[j];
  float* __restrict__ dst = pack + s.off[j];
  const int total = K * np;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int k = i / np, co = i - k * np;
    dst[i] = co < cout ? src[co * K + k] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// stem Conv3d(1 -> 24) + BN + activation -> pre [N][Hs][Ws][24] and the max-pool behind it: lipfront.h's bodies for 24 channels
// on groups of 32 lanes, thread = (channel of 32, x half, row), 8 x positions each; wpk is [245][32]
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lipsn_stem_kernel(LfStemArgs p) { lf_stem<SN_STEM_C, SN_STEM_CP>(p); }

__global__ void __launch_bounds__(256) lipsn_maxpool_kernel(const float* __restrict__ pre, float* __restrict__ out, long long total4,
                                                            int Hs, int Ws, int Hp, int Wp) {
  lf_maxpool<SN_STEM_C>(pre, out, total4, Hs, Ws, Hp, Wp);
}

// ------------------------------------------------------------------------------------------------
// pointwise convolution of P positions held in LDS: A [P][ks] (row = position, ks odd: the 32 lanes of a ds_read_b32 group
// hit 32 banks) times W [K][Np] from memory (K even, Np a multiple of 32, zero columns behind the real ones).  Wave w takes
// the 32 x 32 tiles w, w + 4, ..., two at a time; tile rows past P re-read row P - 1 and are not handed to the epilogue.
// Each run of 32 k is summed on its own and then added to the running total, as lipfe_conv_kernel does.
// epi(row, col, value) for row < P, col < Np.
// ------------------------------------------------------------------------------------------------
template <class Epi>
DEV void sn_pointwise(const float* A, int ks, int P, const float* __restrict__ W, int K, int Np, int wave, int lane, Epi&& epi) {
  const int c = lane & 31, hh = lane >> 5;
  const int mt_n = (P + 31) >> 5, tiles = mt_n * (Np >> 5);
  // a wave runs two tiles (t, t + 4) through one K loop: their operand loads are in flight together, which halves the chain
  // of load latencies a workgroup walks.  Without a second tile the first is computed twice and handed over once.
  for (int t = wave; t < tiles; t += 8) {
    const bool two = t + 4 < tiles;
    const int t1 = two ? t + 4 : t;
    const int mt0 = t % mt_n, nt0 = t / mt_n, mt1 = t1 % mt_n, nt1 = t1 / mt_n;
    const float* a0 = A + min(32 * mt0 + c, P - 1) * ks + hh;
    const float* a1 = A + min(32 * mt1 + c, P - 1) * ks + hh;
    const float* __restrict__ b0 = W + hh * Np + 32 * nt0 + c;
    const float* __restrict__ b1 = W + hh * Np + 32 * nt1 + c;
    f32x16 acc0 = zero16(), acc1 = zero16();
    int k0 = 0;
    for (; k0 + 32 <= K; k0 += 32) {
      f32x16 part0 = zero16(), part1 = zero16();
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        part0 = mfma32(a0[k0 + 2 * kk], b0[(k0 + 2 * kk) * Np], part0);
        part1 = mfma32(a1[k0 + 2 * kk], b1[(k0 + 2 * kk) * Np], part1);
      }
      acc0 += part0;
      acc1 += part1;
    }
    if (k0 < K) {
      f32x16 part0 = zero16(), part1 = zero16();
      for (int k = k0; k < K; k += 2) {
        part0 = mfma32(a0[k], b0[k * Np], part0);
        part1 = mfma32(a1[k], b1[k * Np], part1);
      }
      acc0 += part0;
      acc1 += part1;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = 32 * mt0 + ROW32(r, hh);
      if (rr < P) epi(rr, 32 * nt0 + c, acc0[r]);
    }
    if (two) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = 32 * mt1 + ROW32(r, hh);
        if (rr < P) epi(rr, 32 * nt1 + c, acc1[r]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// one InvertedResidual block
// ------------------------------------------------------------------------------------------------
struct SnBlockArgs {
  const float* in;     // [N][Hi][Wi][Cin]
  float* out;          // [N][Ho][Wo][2 Ch]
  const float* w1;     // banch2 pointwise 1 [K1][Np]: K1 = Ch (channels Ch .. 2 Ch - 1 of the input) at stride 1, Cin at stride 2
  const float* f1;     // its folded BN: scale[Ch], shift[Ch]
  const float* wd;     // banch2 depthwise [9][Ch]
  const float* fd;
  const float* w2;     // banch2 pointwise 2 [Ch][Np]
  const float* f2;
  const float* wd1;    // stride 2 only, banch1: depthwise [9][Cin], pointwise [Cin][Np]
  const float* fd1;
  const float* wp1;
  const float* fp1;
  int N, Hi, Wi, Ho, Wo, Cin, Ch, Np, stride;
  int band, bands, G;  // a workgroup owns `band` output rows of one frame, or (bands == 1) G whole frames
  int ksx, ksm, ksd;   // LDS row lengths of X, mid and D (odd)
  int offM, offD;      // floats into LDS; X is at 0.  Stride 1: D lies over X, which is dead by then
};

// depthwise 3 x 3 (pad 1) + BN of the tile's Q output positions: src [g][RI rows from iy_lo][Wi][kss] -> dst [Q][ksd].
// Padding taps are left out; the nine taps are added in (ky, kx) order.
DEV void sn_depthwise(const float* src, int kss, float* dst, int ksd, const float* __restrict__ wd, const float* __restrict__ f,
                      int C, int Q, int BR, int oy0, int iy_lo, int RI, int Hi, int Wi, int Wo, int stride, int tid) {
  for (int i = tid; i < Q * C; i += 256) {
    const int c = i % C, q = i / C;
    const int ox = q % Wo, t = q / Wo;
    const int oy = oy0 + t % BR, g = t / BR;
    float s = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * stride - 1 + ky;
      if (iy < 0 || iy >= Hi) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * stride - 1 + kx;
        if (ix < 0 || ix >= Wi) continue;
        s = fmaf(src[((g * RI + iy - iy_lo) * Wi + ix) * kss + c], wd[(ky * 3 + kx) * C + c], s);
      }
    }
    dst[q * ksd + c] = fmaf(s, f[c], f[C + c]);
  }
}

// grid (ceil(N / G) * bands), block 256, dynamic LDS.
//   stride 1: out[2 j] = in[j] (j < Ch); out[2 j + 1] = banch2(in[Ch ..])[j]
//   stride 2: out[2 j] = banch1(in)[j];  out[2 j + 1] = banch2(in)[j]
// which is cat + channel_shuffle(., 2) of the reference.  banch2's first pointwise runs on the tile's input rows (the output
// rows' 3 x 3 windows, clipped to the image), so neighbouring bands compute their shared rows twice.
__global__ void __launch_bounds__(256) lipsn_block_kernel(SnBlockArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sn_lds[];
  float* Xs = sn_lds;
  float* Ms = sn_lds + p.offM;
  float* Ds = sn_lds + p.offD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bi = blockIdx.x % p.bands;
  const int n0 = (blockIdx.x / p.bands) * p.G;
  const int ng = min(p.G, p.N - n0);
  const int oy0 = bi * p.band, oy1 = min(p.Ho, oy0 + p.band), BR = oy1 - oy0;
  const int iy_lo = max(0, oy0 * p.stride - 1), iy_hi = min(p.Hi, (oy1 - 1) * p.stride + 2), RI = iy_hi - iy_lo;
  const int Pin = ng * RI * p.Wi, Q = ng * BR * p.Wo;     // with ng > 1: bands == 1, RI == Hi, BR == Ho
  const int Ch = p.Ch, C2 = 2 * Ch;
  const int K1 = p.stride == 1 ? Ch : p.Cin, koff = p.stride == 1 ? Ch : 0;
  const long long in_pos0 = ((long long)n0 * p.Hi + iy_lo) * p.Wi;
  const long long out_pos0 = ((long long)n0 * p.Ho + oy0) * p.Wo;

  for (int i = tid; i < Pin * K1; i += 256) {
    const int q = i / K1, k = i - q * K1;
    Xs[q * p.ksx + k] = p.in[(in_pos0 + q) * p.Cin + koff + k];
  }
  __syncthreads();
  sn_pointwise(Xs, p.ksx, Pin, p.w1, K1, p.Np, wave, lane, [&](int row, int col, float v) {
    if (col < Ch) Ms[row * p.ksm + col] = fmaxf(fmaf(v, p.f1[col], p.f1[Ch + col]), 0.f);
  });
  if (p.stride == 1) {
    for (int i = tid; i < Q * Ch; i += 256) {
      const int q = i / Ch, j = i - q * Ch;
      p.out[(out_pos0 + q) * C2 + 2 * j] = p.in[(out_pos0 + q) * p.Cin + j];
    }
  } else {
    sn_depthwise(Xs, p.ksx, Ds, p.ksd, p.wd1, p.fd1, p.Cin, Q, BR, oy0, iy_lo, RI, p.Hi, p.Wi, p.Wo, 2, tid);
    __syncthreads();
    sn_pointwise(Ds, p.ksd, Q, p.wp1, p.Cin, p.Np, wave, lane, [&](int row, int col, float v) {
      if (col < Ch) p.out[(out_pos0 + row) * C2 + 2 * col] = fmaxf(fmaf(v, p.fp1[col], p.fp1[Ch + col]), 0.f);
    });
  }
  __syncthreads();
  sn_depthwise(Ms, p.ksm, Ds, p.ksd, p.wd, p.fd, Ch, Q, BR, oy0, iy_lo, RI, p.Hi, p.Wi, p.Wo, p.stride, tid);
  __syncthreads();
  sn_pointwise(Ds, p.ksd, Q, p.w2, Ch, p.Np, wave, lane, [&](int row, int col, float v) {
    if (col < Ch) p.out[(out_pos0 + row) * C2 + 2 * col + 1] = fmaxf(fmaf(v, p.f2[col], p.f2[Ch + col]), 0.f);
  });
}

// ------------------------------------------------------------------------------------------------
// conv_last (1 x 1, C -> 1024) + BN + ReLU + AvgPool2d(3): the mean of rows / columns 0..2 of the final map
// ------------------------------------------------------------------------------------------------
constexpr int SN_LAST_G = 3, SN_LAST_N = 1024;   // frames per workgroup: 27 of a tile's 32 rows

// grid (ceil(N / 3)), block 256, dynamic LDS: X [27][ks] + per wave [27][33].  in [N][h][w][C] -> out [N][1024]
__global__ void __launch_bounds__(256) lipsn_last_kernel(const float* __restrict__ in, const float* __restrict__ wpk,
                                                         const float* __restrict__ f, float* __restrict__ out, int N, int h, int w,
                                                         int C, int ks) {
  extern __shared__ __attribute__((aligned(16))) float sn_lds[];
  float* Xs = sn_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, hh = lane >> 5;
  float* scr = sn_lds + 9 * SN_LAST_G * ks + wave * (9 * SN_LAST_G * 33);
  const int n0 = blockIdx.x * SN_LAST_G, ng = min(SN_LAST_G, N - n0), P = 9 * ng;
  for (int i = tid; i < P * C; i += 256) {
    const int row = i / C, k = i - row * C;
    const int g = row / 9, r9 = row - 9 * g, y = r9 / 3, x = r9 - 3 * y;
    Xs[row * ks + k] = in[(((long long)(n0 + g) * h + y) * w + x) * C + k];
  }
  __syncthreads();
  const int row = min(c, P - 1);
  for (int it = 0; it < SN_LAST_N / 128; ++it) {
    const int col = 32 * (wave + 4 * it) + c;
    const float* a = Xs + row * ks + hh;
    const float* __restrict__ b = wpk + hh * SN_LAST_N + col;
    f32x16 acc = zero16();
    int k0 = 0;
    for (; k0 + 32 <= C; k0 += 32) {
      f32x16 part = zero16();
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) part = mfma32(a[k0 + 2 * kk], b[(k0 + 2 * kk) * SN_LAST_N], part);
      acc += part;
    }
    if (k0 < C) {
      f32x16 part = zero16();
      for (int k = k0; k < C; k += 2) part = mfma32(a[k], b[k * SN_LAST_N], part);
      acc += part;
    }
    const float sc = f[col], sh = f[SN_LAST_N + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = ROW32(r, hh);
      if (rr < P) scr[rr * 33 + c] = fmaxf(fmaf(acc[r], sc, sh), 0.f);
    }
    __syncthreads();
    for (int g = hh; g < ng; g += 2) {
      float s = 0.f;
      for (int r = 0; r < 9; ++r) s += scr[(9 * g + r) * 33 + c];
      out[(long long)(n0 + g) * SN_LAST_N + col] = s / 9.0f;
    }
    __syncthreads();
  }
}

}  // namespace
