// mask_tail.hip -- forward and backward of the masked tail of DPTNEncDec (mask_tail.h states the math).
//
// One workgroup of 256 threads walks frame tiles of TF = 16 * (256 / N) rows (64 at N = 64, 32 at N = 128) with a
// grid-stride loop, so that the packed [W_out; W_gate] is staged into LDS once per workgroup (32 KiB at N = 64,
// 128 KiB at N = 128: one workgroup per CU there).  Per tile:
//   1. gather u (the overlap-added Z rows of the tile) into LDS: the branch-free two-chunk gather of taps_fold_kernel;
//   2. thread (o = tid % N, frame group tid / N) forms a_out[o], a_gate[o] of 16 frames: plain fp32 FMAs, weights from
//      LDS (lane-consecutive, conflict-free), u rows broadcast to the wave;
//   3. epilogue tanh / sigmoid / product / ReLU / * E, the result row back into LDS;
//   4. the <= 8-tap decoder contraction per frame, stored as the D table decoder_gather_kernel reads.
// The backward recomputes 1-3 from Z and E (nothing is kept on the tape) and writes d q * m, d a and the decoder
// weight-gradient partials (fixed summation order, no atomics: bit-reproducible for a given grid).
// fp32 VALU rather than MFMA: at N = 64 the 2N x N product is ~2.8 GFMA per B = 16 forward against ~275 MB of
// gathers, so the kernel is bound by the gather / LDS traffic, not by the multiply.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mask_tail.h"

namespace {

constexpr int MT_THREADS = 256;

// floor(n / d) for 0 <= n < 2^23, d >= 1: the float estimate is within +-1, fixed by one correction step each way
DEV int mt_div(int n, int d, float inv_d) {
  if (n >= (1 << 23)) return n / d;
  int q = (int)((float)n * inv_d);
  const int r = n - q * d;
  q += r >= d ? 1 : 0;
  q -= r < 0 ? 1 : 0;
  return q;
}

template <int N>
struct MtShape {
  static constexpr int FG = MT_THREADS / N;   // frame groups (threads per output channel)
  static constexpr int FPT = 16;              // frames per thread
  static constexpr int TF = FG * FPT;         // frames per tile
  static constexpr int LDU = N + 4;           // LDS row pitch: the tap loop's 8 frame rows per wave land 4 banks apart
  static constexpr int K4 = N / 4;
  static constexpr int NI = TF * K4 / MT_THREADS;   // float4 gather slots per thread
  static_assert(TF * K4 % MT_THREADS == 0, "gather slots");
};

// u rows [r0, r0 + TF) of the (2, B, L) frame list into Us[TF][LDU] (zero rows outside [left, left + ola) and past the end)
template <int N>
DEV void gather_u(const MaskTailGeom& g, int r0, float* Us, int tid) {
  using Sh = MtShape<N>;
  const int BL = g.B * g.L, rows = 2 * BL;
  const float invL = 1.0f / (float)g.L, invP = 1.0f / (float)g.P;
  if (g.K <= 2 * g.P) {
    // at most two chunks cover a frame: every slot requests exactly two rows (clamped addresses) and masks what does not
    // count, so that all 2 x NI loads of a thread are in flight together
    float4 z0[Sh::NI], z1[Sh::NI];
    bool ok0[Sh::NI], ok1[Sh::NI];
#pragma unroll
    for (int i = 0; i < Sh::NI; ++i) {
      const int idx = i * MT_THREADS + tid;
      const int row = idx / Sh::K4, k4 = idx - row * Sh::K4;
      const int r = r0 + row;
      const bool inr = r < rows;
      const int rc = inr ? r : rows - 1;
      const int spk = rc >= BL ? 1 : 0;
      const int rem = rc - spk * BL;
      const int b = mt_div(rem, g.L, invL);
      const int t = rem - b * g.L - g.left;
      const bool tin = t >= 0 && t < g.ola;
      const int tc = tin ? t : 0;
      int s_hi = mt_div(tc, g.P, invP);
      if (s_hi > g.S - 1) s_hi = g.S - 1;
      const int s1 = s_hi - 1;
      const int k0 = tc - g.P * s_hi, k1 = tc - g.P * s1;
      const bool v0 = tin && k0 < g.K, v1 = tin && s1 >= 0 && k1 < g.K;
      const int64_t zo0 = (((int64_t)b * g.S + s_hi) * g.K + (v0 ? k0 : 0)) * (2 * N) + spk * N + 4 * k4;
      const int64_t zo1 = (((int64_t)b * g.S + (v1 ? s1 : s_hi)) * g.K + (v1 ? k1 : 0)) * (2 * N) + spk * N + 4 * k4;
      z0[i] = *reinterpret_cast<const float4*>(g.Z + zo0);
      z1[i] = *reinterpret_cast<const float4*>(g.Z + zo1);
      ok0[i] = inr && v0;
      ok1[i] = inr && v1;
    }
#pragma unroll
    for (int i = 0; i < Sh::NI; ++i) {
      const int idx = i * MT_THREADS + tid;
      const int row = idx / Sh::K4, k4 = idx - row * Sh::K4;
      const float4 m0 = mask4(z0[i], ok0[i]), m1 = mask4(z1[i], ok1[i]);
      *reinterpret_cast<float4*>(&Us[row * Sh::LDU + 4 * k4]) = make_float4(m0.x + m1.x, m0.y + m1.y, m0.z + m1.z, m0.w + m1.w);
    }
  } else {
#pragma unroll
    for (int i = 0; i < Sh::NI; ++i) {
      const int idx = i * MT_THREADS + tid;
      const int row = idx / Sh::K4, k4 = idx - row * Sh::K4;
      const int r = r0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) {
        const int spk = r >= BL ? 1 : 0;
        const int rem = r - spk * BL;
        const int b = mt_div(rem, g.L, invL);
        const int t = rem - b * g.L - g.left;
        if (t >= 0 && t < g.ola) {
          int s_hi = mt_div(t, g.P, invP);
          if (s_hi > g.S - 1) s_hi = g.S - 1;
          for (int s = s_hi; s >= 0 && t - g.P * s < g.K; --s) {
            const float4 z = *reinterpret_cast<const float4*>(g.Z + (((int64_t)b * g.S + s) * g.K + (t - g.P * s)) * (2 * N) + spk * N + 4 * k4);
            v.x += z.x; v.y += z.y; v.z += z.z; v.w += z.w;
          }
        }
      }
      *reinterpret_cast<float4*>(&Us[row * Sh::LDU + 4 * k4]) = v;
    }
  }
}

// Ws[k][2N] = Wp[o][k] (transposed: the product loop reads one k row, lanes = output channels), bs = biases
template <int N>
DEV void stage_weights(const float* __restrict__ Wp, float* Ws, float* bs, int tid) {
  for (int i = tid; i < 2 * N * N; i += MT_THREADS) {
    const int k = i / (2 * N), o = i - k * (2 * N);
    Ws[i] = Wp[o * N + k];
  }
  for (int i = tid; i < 2 * N; i += MT_THREADS) bs[i] = Wp[2 * N * N + i];
}

// a_out / a_gate of the thread's 16 frames (output channel o, frame group grp) from the staged tile
template <int N>
DEV void tile_product(const float* Ws, const float* bs, const float* Us, int o, int grp, float (&ao)[16], float (&ag)[16]) {
  using Sh = MtShape<N>;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    ao[i] = bs[o];
    ag[i] = bs[N + o];
  }
  const float* u = Us + grp * 16 * Sh::LDU;
#pragma unroll 2
  for (int k = 0; k < N; k += 4) {
    const float wo0 = Ws[(k + 0) * 2 * N + o], wo1 = Ws[(k + 1) * 2 * N + o], wo2 = Ws[(k + 2) * 2 * N + o],
                wo3 = Ws[(k + 3) * 2 * N + o];
    const float wg0 = Ws[(k + 0) * 2 * N + N + o], wg1 = Ws[(k + 1) * 2 * N + N + o], wg2 = Ws[(k + 2) * 2 * N + N + o],
                wg3 = Ws[(k + 3) * 2 * N + N + o];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 x = *reinterpret_cast<const float4*>(u + i * Sh::LDU + k);
      ao[i] = fmaf(x.w, wo3, fmaf(x.z, wo2, fmaf(x.y, wo1, fmaf(x.x, wo0, ao[i]))));
      ag[i] = fmaf(x.w, wg3, fmaf(x.z, wg2, fmaf(x.y, wg1, fmaf(x.x, wg0, ag[i]))));
    }
  }
}

// accurate fp32 forms: tanhf, and 1 / (1 + e^-x) saturates to 0 / 1 without a NaN for any finite x
DEV float mt_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int N>
__global__ __launch_bounds__(MT_THREADS) void mask_tail_fwd_kernel(MaskTailGeom g, const float* __restrict__ Wp,
                                                                   const float* __restrict__ wdec, float* __restrict__ D) {
  using Sh = MtShape<N>;
  __shared__ __attribute__((aligned(16))) float Ws[2 * N * N];
  __shared__ __attribute__((aligned(16))) float Us[Sh::TF * Sh::LDU];
  __shared__ __attribute__((aligned(16))) float Wd[8 * Sh::LDU];
  __shared__ float bs[2 * N];
  const int tid = threadIdx.x, o = tid % N, grp = tid / N;
  const int BL = g.B * g.L, rows = 2 * BL;
  const int ntiles = (rows + Sh::TF - 1) / Sh::TF;
  stage_weights<N>(Wp, Ws, bs, tid);
  for (int i = tid; i < 8 * N; i += MT_THREADS) {
    const int j = i / N, c = i - j * N;
    Wd[j * Sh::LDU + c] = j < g.kenc ? wdec[c * g.kenc + j] : 0.f;
  }
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r0 = tile * Sh::TF;
    gather_u<N>(g, r0, Us, tid);
    __syncthreads();                                   // (the first pass: also the staged weights)
    float ao[16], ag[16];
    tile_product<N>(Ws, bs, Us, o, grp, ao, ag);
    __syncthreads();                                   // every wave is done with u: the rows are overwritten with q
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int f = grp * 16 + i, r = r0 + f;
      float q = 0.f;
      if (r < rows) {
        const int rem = r >= BL ? r - BL : r;
        const float m = fmaxf(tanhf(ao[i]) * mt_sigmoid(ag[i]), 0.f);
        q = m * g.E[(int64_t)rem * N + o];
      }
      Us[f * Sh::LDU + o] = q;
    }
    __syncthreads();
    for (int p = tid; p < Sh::TF * 8; p += MT_THREADS) {
      const int f = p >> 3, j = p & 7;
      const float* qr = Us + f * Sh::LDU;
      const float* wr = Wd + j * Sh::LDU;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
      for (int c = 0; c < N; c += 4) {
        const float4 x = *reinterpret_cast<const float4*>(qr + c), y = *reinterpret_cast<const float4*>(wr + c);
        a0 = fmaf(x.x, y.x, a0); a1 = fmaf(x.y, y.y, a1); a2 = fmaf(x.z, y.z, a2); a3 = fmaf(x.w, y.w, a3);
      }
      if (r0 + f < rows) D[(int64_t)(r0 + f) * 8 + j] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();                                   // before the next tile's gather overwrites the rows
  }
}

template <int N>
__global__ __launch_bounds__(MT_THREADS) void mask_tail_bwd_kernel(MaskTailGeom g, const float* __restrict__ Wp,
                                                                   const float* __restrict__ wdec, const float* __restrict__ dy1,
                                                                   const float* __restrict__ dy2, int64_t T, int stride,
                                                                   int pad_left, float* __restrict__ DQ, float* __restrict__ DA,
                                                                   float* __restrict__ partials) {
  using Sh = MtShape<N>;
  static_assert(Sh::FG * N * 8 <= Sh::TF * Sh::LDU, "partials reduction fits the tile buffer");
  __shared__ __attribute__((aligned(16))) float Ws[2 * N * N];
  __shared__ __attribute__((aligned(16))) float Us[Sh::TF * Sh::LDU];
  __shared__ __attribute__((aligned(16))) float dDs[Sh::TF * 8];
  __shared__ float bs[2 * N];
  const int tid = threadIdx.x, o = tid % N, grp = tid / N;
  const int BL = g.B * g.L, rows = 2 * BL;
  const int ntiles = (rows + Sh::TF - 1) / Sh::TF;
  const float invL = 1.0f / (float)g.L;
  stage_weights<N>(Wp, Ws, bs, tid);
  float wd[8], wacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    wd[j] = j < g.kenc ? wdec[o * g.kenc + j] : 0.f;
    wacc[j] = 0.f;
  }
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r0 = tile * Sh::TF;
    gather_u<N>(g, r0, Us, tid);
    // d D[r][j] = d y[pad_left + stride * l + j] (the transposed conv's gather, read back)
    for (int p = tid; p < Sh::TF * 8; p += MT_THREADS) {
      const int f = p >> 3, j = p & 7, r = r0 + f;
      float d = 0.f;
      if (r < rows && j < g.kenc) {
        const int spk = r >= BL ? 1 : 0;
        const int rem = r - spk * BL;
        const int b = mt_div(rem, g.L, invL);
        const int l = rem - b * g.L;
        const int64_t n = (int64_t)pad_left + (int64_t)stride * l + j;
        if (n >= 0 && n < T) d = (spk ? dy2 : dy1)[(int64_t)b * T + n];
      }
      dDs[p] = d;
    }
    __syncthreads();
    float ao[16], ag[16];
    tile_product<N>(Ws, bs, Us, o, grp, ao, ag);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int f = grp * 16 + i, r = r0 + f;
      if (r < rows) {
        const int rem = r >= BL ? r - BL : r;
        const float e = g.E[(int64_t)rem * N + o];
        const float t = tanhf(ao[i]), s = mt_sigmoid(ag[i]), ts = t * s;
        const float m = fmaxf(ts, 0.f), q = m * e;
        float dq = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = dDs[f * 8 + j];
          dq = fmaf(d, wd[j], dq);
          wacc[j] = fmaf(q, d, wacc[j]);
        }
        DQ[(int64_t)r * N + o] = dq * m;
        const float dpre = ts > 0.f ? dq * e : 0.f;
        DA[(int64_t)r * (2 * N) + o] = dpre * s * (1.f - t * t);
        DA[(int64_t)r * (2 * N) + N + o] = dpre * t * (s * (1.f - s));
      }
    }
    __syncthreads();                                   // before the next tile's gather overwrites u and d D
  }
  // the frame groups' decoder partials, summed in group order: partials[blockIdx.x][c][j]
  float* red = Us;
#pragma unroll
  for (int j = 0; j < 8; ++j) red[(grp * N + o) * 8 + j] = wacc[j];
  __syncthreads();
  for (int p = tid; p < N * 8; p += MT_THREADS) {
    float s = 0.f;
    for (int q = 0; q < Sh::FG; ++q) s += red[q * N * 8 + p];
    partials[(size_t)blockIdx.x * (N * 8) + p] = s;
  }
}

__global__ __launch_bounds__(256) void mask_tail_pack_kernel(int N, const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                             const float* __restrict__ w_gate, const float* __restrict__ b_gate,
                                                             float* __restrict__ Wp) {
  const int nn = N * N;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * nn + 2 * N; i += gridDim.x * 256) {
    float v;
    if (i < nn) v = w_out[i];
    else if (i < 2 * nn) v = w_gate[i - nn];
    else if (i < 2 * nn + N) v = b_out[i - 2 * nn];
    else v = b_gate[i - 2 * nn - N];
    Wp[i] = v;
  }
}

__global__ __launch_bounds__(256) void mask_tail_grad_scatter_kernel(int N, const float* __restrict__ gw, const float* __restrict__ gb,
                                                                     float* __restrict__ g_wout, float* __restrict__ g_bout,
                                                                     float* __restrict__ g_wgate, float* __restrict__ g_bgate) {
  const int nn = N * N;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * nn + 2 * N; i += gridDim.x * 256) {
    if (i < nn) g_wout[i] = gw[i];
    else if (i < 2 * nn) g_wgate[i - nn] = gw[i];
    else if (i < 2 * nn + N) g_bout[i - 2 * nn] = gb[i - 2 * nn];
    else g_bgate[i - 2 * nn - N] = gb[i - 2 * nn];
  }
}

// co-resident workgroups per CU of a kernel (LDS-bound here), queried once per kernel
template <class Kern>
int resident_per_cu(Kern kern, int* cache) {
  if (*cache == 0) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), MT_THREADS, 0) != hipSuccess ||
        per_cu < 1)
      per_cu = 1;
    *cache = per_cu;
  }
  return *cache;
}

template <int N>
int fwd_launch(hipStream_t st, const MaskTailGeom& g, const float* Wp, const float* wdec, float* D, int num_cus) {
  static int per_cu = 0;
  const int64_t rows = (int64_t)2 * g.B * g.L, ntiles = (rows + MtShape<N>::TF - 1) / MtShape<N>::TF;
  const int64_t cap = (int64_t)resident_per_cu(mask_tail_fwd_kernel<N>, &per_cu) * num_cus;
  const int grid = (int)(ntiles < cap ? ntiles : cap);
  hipLaunchKernelGGL(mask_tail_fwd_kernel<N>, dim3(grid), dim3(MT_THREADS), 0, st, g, Wp, wdec, D);
  return (int)hipGetLastError();
}

template <int N>
int bwd_launch(hipStream_t st, const MaskTailGeom& g, const float* Wp, const float* wdec, const float* dy1, const float* dy2,
               int64_t T, int stride, int pad_left, float* DQ, float* DA, float* partials, int max_wgs, int num_cus,
               int* grid_used) {
  static int per_cu = 0;
  const int64_t rows = (int64_t)2 * g.B * g.L, ntiles = (rows + MtShape<N>::TF - 1) / MtShape<N>::TF;
  int64_t cap = (int64_t)resident_per_cu(mask_tail_bwd_kernel<N>, &per_cu) * num_cus;
  if (cap > max_wgs) cap = max_wgs;
  const int grid = (int)(ntiles < cap ? ntiles : cap);
  *grid_used = grid;
  hipLaunchKernelGGL(mask_tail_bwd_kernel<N>, dim3(grid), dim3(MT_THREADS), 0, st, g, Wp, wdec, dy1, dy2, T, stride,
                     pad_left, DQ, DA, partials);
  return (int)hipGetLastError();
}

}  // namespace

int mask_tail_pack_launch(void* stream, int N, const float* w_out, const float* b_out, const float* w_gate,
                          const float* b_gate, float* Wp) {
  const int n = 2 * N * N + 2 * N;
  hipLaunchKernelGGL(mask_tail_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, w_out, b_out,
                     w_gate, b_gate, Wp);
  return (int)hipGetLastError();
}

int mask_tail_fwd_launch(void* stream, int N, const MaskTailGeom& g, const float* Wp, const float* wdec, float* D,
                         int num_cus) {
  if (N == 64) return fwd_launch<64>((hipStream_t)stream, g, Wp, wdec, D, num_cus);
  if (N == 128) return fwd_launch<128>((hipStream_t)stream, g, Wp, wdec, D, num_cus);
  return (int)hipErrorInvalidValue;
}

int mask_tail_bwd_launch(void* stream, int N, const MaskTailGeom& g, const float* Wp, const float* wdec,
                         const float* dy1, const float* dy2, int64_t T, int stride, int pad_left, float* DQ, float* DA,
                         float* partials, int max_wgs, int num_cus, int* grid_used) {
  if (N == 64)
    return bwd_launch<64>((hipStream_t)stream, g, Wp, wdec, dy1, dy2, T, stride, pad_left, DQ, DA, partials, max_wgs, num_cus,
                          grid_used);
  if (N == 128)
    return bwd_launch<128>((hipStream_t)stream, g, Wp, wdec, dy1, dy2, T, stride, pad_left, DQ, DA, partials, max_wgs,
                           num_cus, grid_used);
  return (int)hipErrorInvalidValue;
}

int mask_tail_grad_scatter_launch(void* stream, int N, const float* gw, const float* gb, float* g_wout, float* g_bout,
                                  float* g_wgate, float* g_bgate) {
  const int n = 2 * N * N + 2 * N;
  hipLaunchKernelGGL(mask_tail_grad_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, gw, gb,
                     g_wout, g_bout, g_wgate, g_bgate);
  return (int)hipGetLastError();
}
