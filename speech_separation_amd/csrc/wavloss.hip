// wavloss.hip -- the waveform criteria on the device (include/wavloss.h): MAE / MSE / SI-SNR under batch-level or
// utterance-level PIT, forward and backward in two launches, no host synchronisation.
//
//   BaseSSLoss (batch-level PIT)   src/loss/ss_losses.py:21-26
//   MAEWavLoss, MSEWavLoss         src/loss/ss_losses.py:65-93    (nn.L1Loss / nn.MSELoss, reduction "mean")
//   SiSNRLoss                      src/loss/ss_losses.py:100-114
//   SiSNRWavLoss                   src/loss/ss_losses.py:117-130
//
// The reference runs a few dozen small PyTorch kernels and a tensor -> bool conversion (`if loss_perm_2 < loss_perm_1`).
// Here launch 1 leaves the four per-item terms l_i(p1,s1) l_i(p1,s2) l_i(p2,s1) l_i(p2,s2) in scratch, launch 2 resolves
// the permutation in every workgroup from those terms (same fixed-order sum everywhere) and writes d loss / d prediction.
// Sums are double precision in a fixed order (no atomics): repeated calls are bit-identical.  Rows start at T * 4-byte
// strides, so nothing may assume more than float alignment: every load and store is one float (coalesced dwords).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wavloss.h"

namespace {

constexpr int WL_STAT = 8;             // doubles per (item, pair): loss term, mx, my, D, G, Nn, pad, pad
constexpr int WL_STATS_THREADS = 1024; // one workgroup per (item, pair): 16 waves walk the row
constexpr int WL_GRAD_THREADS = 256;
constexpr int WL_GRAD_SPAN = 1024;     // samples per workgroup of the gradient launch

// Sum over the workgroup's NW waves, result in every thread; the order is fixed.
template <int NW>
__device__ __forceinline__ double wl_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) s += red[w];
  return s;
}

// Launch 1.  Workgroup (item b, pair): pairs = (p1,s1) (p1,s2) (p2,s1) (p2,s2).  SI-SNR takes two passes over the 2 x T
// samples (the second one hits L2): the noise energy |p~ - a s~|^2 is summed directly, not as a difference of energies.
template <int KIND>
__global__ __launch_bounds__(WL_STATS_THREADS) void wavloss_stats_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                                         const float* __restrict__ s1, const float* __restrict__ s2,
                                                                         int64_t T, double* __restrict__ stats) {
  constexpr int NW = WL_STATS_THREADS / 64;
  __shared__ double red[NW];
  const int64_t b = blockIdx.x >> 2;
  const int pair = blockIdx.x & 3;
  const float* x = (pair < 2 ? p1 : p2) + b * T;
  const float* y = ((pair & 1) ? s2 : s1) + b * T;
  double* o = stats + (int64_t)blockIdx.x * WL_STAT;
  if (KIND != WAVLOSS_SISNR) {
    double acc = 0;
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < T; i += WL_STATS_THREADS) {
      const double d = (double)x[i] - (double)y[i];        // exact
      acc += KIND == WAVLOSS_MAE ? fabs(d) : d * d;
    }
    acc = wl_block_sum<NW>(acc, red);
    if (threadIdx.x == 0) o[0] = acc / (double)T;          // nn.L1Loss / nn.MSELoss on item b, ss_losses.py:67,82
    return;
  }
  double sx = 0, sy = 0, sxy = 0, syy = 0;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < T; i += WL_STATS_THREADS) {
    const double xv = x[i], yv = y[i];
    sx += xv; sy += yv; sxy += xv * yv; syy += yv * yv;
  }
  sx = wl_block_sum<NW>(sx, red); sy = wl_block_sum<NW>(sy, red);
  sxy = wl_block_sum<NW>(sxy, red); syy = wl_block_sum<NW>(syy, red);
  const double mx = sx / (double)T, my = sy / (double)T;   // ss_losses.py:101-102
  const double D = sxy - (double)T * mx * my;              // <p~, s~>   :104
  const double G = syy - (double)T * my * my;              // |s~|^2     :105
  const double a = D / G;                                  // :106 (0/0 for a silent target, as there)
  double nn = 0;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < T; i += WL_STATS_THREADS) {
    const double e = ((double)x[i] - mx) - a * ((double)y[i] - my);   // :110
    nn += e * e;
  }
  nn = wl_block_sum<NW>(nn, red);
  if (threadIdx.x == 0) {
    o[0] = -20.0 * log10((a * a * G) / nn);                // :111-114
    o[1] = mx; o[2] = my; o[3] = D; o[4] = G; o[5] = nn;
  }
}

// Launch 2.  Workgroup = (chunk of WL_GRAD_SPAN samples, item b, prediction z), flattened into grid.x.  Batch level: every
// workgroup sums the 4 B terms in the same fixed order and takes the batch's permutation (ss_losses.py:21-25); utterance
// level: it reads its item's own four terms.  Workgroup 0 also writes loss_out and perm_out.
template <int KIND>
__global__ __launch_bounds__(WL_GRAD_THREADS) void wavloss_grad_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                                       const float* __restrict__ s1, const float* __restrict__ s2, int B,
                                                                       int64_t T, unsigned nchunk, int level,
                                                                       const double* __restrict__ stats, float grad_scale,
                                                                       float* __restrict__ d1, float* __restrict__ d2,
                                                                       float* __restrict__ loss_out, int32_t* __restrict__ perm_out) {
  __shared__ double red[WL_GRAD_THREADS / 64];
  const unsigned chunk = blockIdx.x % nchunk, rest = blockIdx.x / nchunk;
  const int z = rest & 1;
  const int64_t b = rest >> 1;
  const bool lead = blockIdx.x == 0;
  bool swap = false;
  if (level == WAVLOSS_PIT_BATCH || lead) {                // uniform over the workgroup
    double a0 = 0, a1 = 0, au = 0, cnt = 0;
    for (int i = threadIdx.x; i < B; i += WL_GRAD_THREADS) {
      const double* s = stats + (int64_t)i * 4 * WL_STAT;
      const double t0 = s[0] + s[3 * WL_STAT];             // permutation 0: (p1,s1) + (p2,s2)
      const double t1 = s[WL_STAT] + s[2 * WL_STAT];       // permutation 1: (p1,s2) + (p2,s1)
      a0 += t0; a1 += t1;
      const bool sw = t1 * 0.5 < t0 * 0.5;
      au += (sw ? t1 : t0) * 0.5;
      cnt += sw ? 1.0 : 0.0;
      if (lead && level == WAVLOSS_PIT_UTTERANCE) perm_out[i] = sw ? 1 : 0;
    }
    a0 = wl_block_sum<WL_GRAD_THREADS / 64>(a0, red);
    a1 = wl_block_sum<WL_GRAD_THREADS / 64>(a1, red);
    const double l0 = a0 / (2.0 * B), l1 = a1 / (2.0 * B);
    swap = l1 < l0;                                        // ss_losses.py:23-25
    if (lead) {
      if (level == WAVLOSS_PIT_UTTERANCE) {
        au = wl_block_sum<WL_GRAD_THREADS / 64>(au, red);
        cnt = wl_block_sum<WL_GRAD_THREADS / 64>(cnt, red);
      } else {
        for (int i = threadIdx.x; i < B; i += WL_GRAD_THREADS) perm_out[i] = swap ? 1 : 0;
      }
      if (threadIdx.x == 0) {
        loss_out[0] = level == WAVLOSS_PIT_UTTERANCE ? (float)(au / (double)B) : (float)(swap ? l1 : l0);
        loss_out[1] = level == WAVLOSS_PIT_UTTERANCE ? (float)cnt : (swap ? (float)B : 0.f);
        loss_out[2] = (float)l0;
        loss_out[3] = (float)l1;
      }
    }
  }
  const double* sb = stats + b * 4 * WL_STAT;
  if (level == WAVLOSS_PIT_UTTERANCE)
    swap = (sb[WL_STAT] + sb[2 * WL_STAT]) * 0.5 < (sb[0] + sb[3 * WL_STAT]) * 0.5;
  const int pair = swap ? (z == 0 ? 1 : 2) : (z == 0 ? 0 : 3);
  const float* x = (z == 0 ? p1 : p2) + b * T;
  const float* y = ((pair & 1) ? s2 : s1) + b * T;
  float* d = (z == 0 ? d1 : d2) + b * T;
  const int64_t i0 = (int64_t)chunk * WL_GRAD_SPAN + threadIdx.x;
  if (KIND == WAVLOSS_MAE) {
    const float w = (float)((double)grad_scale / (2.0 * (double)B * (double)T));
#pragma unroll
    for (int j = 0; j < WL_GRAD_SPAN / WL_GRAD_THREADS; ++j) {
      const int64_t i = i0 + j * WL_GRAD_THREADS;
      if (i < T) {
        const float e = x[i] - y[i];                       // the sign of an fp32 difference is exact
        d[i] = e > 0.f ? w : (e < 0.f ? -w : 0.f);         // sign(0) = 0: torch's L1 backward
      }
    }
  } else if (KIND == WAVLOSS_MSE) {
    const float w2 = (float)((double)grad_scale / ((double)B * (double)T));   // 2 / (2 B T)
#pragma unroll
    for (int j = 0; j < WL_GRAD_SPAN / WL_GRAD_THREADS; ++j) {
      const int64_t i = i0 + j * WL_GRAD_THREADS;
      if (i < T) d[i] = w2 * (x[i] - y[i]);
    }
  } else {
    // loss = w sum_items -20 log10(|a s~|^2 / |e|^2), w = grad_scale / (2 B)
    // d / d p = w (-20 / ln 10) (2 s~ / D - 2 e / |e|^2)      (s~ and e are zero-mean: the mean subtraction drops out)
    const double* s = sb + pair * WL_STAT;
    const double mx = s[1], my = s[2], D = s[3], G = s[4], nn = s[5];
    const double c = (double)grad_scale / (2.0 * B) * (-20.0 / 2.302585092994046);
    const double cg = c * 2.0 / D, ce = c * 2.0 / nn, al = D / G;
#pragma unroll
    for (int j = 0; j < WL_GRAD_SPAN / WL_GRAD_THREADS; ++j) {
      const int64_t i = i0 + j * WL_GRAD_THREADS;
      if (i < T) {
        const double g = (double)y[i] - my, e = ((double)x[i] - mx) - al * g;
        d[i] = (float)(cg * g - ce * e);
      }
    }
  }
}

template <int KIND>
void launch(hipStream_t st, const float* p1, const float* p2, const float* s1, const float* s2, int B, int64_t T, unsigned nchunk,
            int level, double* stats, float grad_scale, float* d1, float* d2, float* loss_out, int32_t* perm_out) {
  hipLaunchKernelGGL(wavloss_stats_kernel<KIND>, dim3((unsigned)B * 4u), dim3(WL_STATS_THREADS), 0, st, p1, p2, s1, s2, T, stats);
  hipLaunchKernelGGL(wavloss_grad_kernel<KIND>, dim3(nchunk * (unsigned)B * 2u), dim3(WL_GRAD_THREADS), 0, st, p1, p2, s1, s2, B, T,
                     nchunk, level, stats, grad_scale, d1, d2, loss_out, perm_out);
}

}  // namespace

extern "C" {

int wavloss_abi_version(void) { return WAVLOSS_ABI_VERSION; }

const char* wavloss_strerror(int code) {
  switch (code) {
    case WAVLOSS_OK: return "ok";
    case WAVLOSS_ERR_INVALID: return "wavloss: bad argument (shape, null pointer, kind, level, or scratch too small / misaligned)";
    case WAVLOSS_ERR_SCRATCH: return "wavloss: scratch too small / misaligned";
    case WAVLOSS_ERR_HIP: return "wavloss: a launch failed (no HIP device? libdptnav has no CPU path)";
    default: return "wavloss: unknown error code";
  }
}

size_t wavloss_scratch_bytes(int B) { return B < 1 ? 0 : (size_t)B * 4 * WL_STAT * sizeof(double); }

int wavloss_pit_loss(int kind, int level, const float* s1_pred, const float* s2_pred, const float* s1, const float* s2, int B,
                     int64_t T, float grad_scale, float* d_s1_pred, float* d_s2_pred, float* loss_out, int32_t* perm_out,
                     void* scratch, size_t scratch_bytes, void* stream) {
  if (kind != WAVLOSS_MAE && kind != WAVLOSS_MSE && kind != WAVLOSS_SISNR) return WAVLOSS_ERR_INVALID;
  if (level != WAVLOSS_PIT_BATCH && level != WAVLOSS_PIT_UTTERANCE) return WAVLOSS_ERR_INVALID;
  if (!s1_pred || !s2_pred || !s1 || !s2 || !d_s1_pred || !d_s2_pred || !loss_out || !perm_out) return WAVLOSS_ERR_INVALID;
  if (B < 1 || T < 1 || (kind == WAVLOSS_SISNR && T < 2)) return WAVLOSS_ERR_INVALID;
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < wavloss_scratch_bytes(B)) return WAVLOSS_ERR_INVALID;
  // one launch may carry 2^32 - 1 threads: B * 4 workgroups of 1024 and chunks * B * 2 workgroups of 256
  const int64_t nchunk = (T + WL_GRAD_SPAN - 1) / WL_GRAD_SPAN;
  if (B >= (1 << 20) || nchunk * B * 2 >= ((int64_t)1 << 24)) return WAVLOSS_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  double* stats = (double*)scratch;
  if (kind == WAVLOSS_MAE)
    launch<WAVLOSS_MAE>(st, s1_pred, s2_pred, s1, s2, B, T, (unsigned)nchunk, level, stats, grad_scale, d_s1_pred, d_s2_pred, loss_out,
                        perm_out);
  else if (kind == WAVLOSS_MSE)
    launch<WAVLOSS_MSE>(st, s1_pred, s2_pred, s1, s2, B, T, (unsigned)nchunk, level, stats, grad_scale, d_s1_pred, d_s2_pred, loss_out,
                        perm_out);
  else
    launch<WAVLOSS_SISNR>(st, s1_pred, s2_pred, s1, s2, B, T, (unsigned)nchunk, level, stats, grad_scale, d_s1_pred, d_s2_pred, loss_out,
                          perm_out);
  return hipGetLastError() == hipSuccess ? WAVLOSS_OK : WAVLOSS_ERR_HIP;
}

}  // extern "C"
