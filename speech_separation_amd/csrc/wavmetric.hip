// wavmetric.hip -- evaluation metrics on the device (include/wavmetric.h): SI-SDR and STOI / ESTOI of the four
// (prediction, target) pairs of a two-speaker batch.
//
//   SISDRMetric   src/metrics/si_sdr.py   (torchmetrics ScaleInvariantSignalDistortionRatio, defaults)
//   STOIMetric    src/metrics/stoi.py     (torchmetrics -> pystoi on the host, one utterance at a time)
//
// STOI in three or four launches, all sized by B and T alone (the number of kept frames never reaches the host):
//   1 resample   fs -> 10 kHz, polyphase FIR, the four signals of every item                 (skipped at fs = 10000)
//   2 mask       per (item, target): frame energies, the 40 dB rule, prefix sum -> list of kept frames + count
//   3 spectra    per (item, target, {clean, prediction 1, prediction 2}) and tile of 64 compacted frames: the
//                overlap-added signal is gathered through the list, windowed, and multiplied with the [256 x 2 x 212]
//                twiddle matrix on v_mfma_f32_32x32x2_f32 (exact fp32); |.|^2, band sums, square roots -> [frames][15]
//                launched for "all frames kept", workgroups past the device-side count leave at once
//   4 measure    per (item, pair): one wave per segment of 30 frames (a lane owns a frame), double sum in a fixed order
// Six spectra per item, not eight: a target's mask and spectrum serve both predictions.  Rows of the inputs start at
// T * 4-byte strides, so every load of a signal is one float.  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/wavmetric.h"

namespace {

constexpr int WM_FS = 10000;
constexpr int WM_FRAME = 256;
constexpr int WM_HOP = 128;
constexpr int WM_NFFT = 512;
constexpr int WM_BANDS = 15;
constexpr int WM_BAND_STRIDE = 16;       // floats per frame of a band spectrum (15 + one zero)
constexpr int WM_SEG = 30;
constexpr float WM_EPS = 2.220446049250313e-16f;       // 2^-52, the double epsilon, exactly representable
constexpr float WM_DYN_RANGE = 40.f;
constexpr float WM_CLIP = 6.623413251903491f;          // 1 + 10^(15 / 20)
constexpr float WM_SHORT = 1e-5f;
constexpr int WM_MAX_TAPS = 592;         // 2 L + 1 = 581 at 16 kHz, 365 at 8 kHz
constexpr int WM_COLS = 224;             // twiddle columns: the 212 bins 7..218, zero-padded to 7 tiles of 32
constexpr int WM_TILES = WM_COLS / 32;
constexpr int WM_ROWS = 64;              // compacted frames per workgroup of the spectra launch
constexpr int WM_A_STRIDE = 129;         // LDS row stride of the frame tile, 128 samples at a time (odd: fragment reads spread over the banks)
constexpr int WM_P_STRIDE = 225;         // LDS row stride of the power tile
constexpr int WM_MEASURE_THREADS = 1024;
constexpr int WM_SDR_THREADS = 1024;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Handle {
  int fs, extended, p, q, L, ntaps;
  int bin_lo;                            // first bin any band reads (7)
  void* dev;                             // one allocation: taps | window | cos | sin | band edges
  const float *taps, *win, *cosT, *sinT;
  const int* edges;                      // [16]: band b is bins [edges[b], edges[b + 1]) relative to bin_lo
};

// The four signals of item b at 10 kHz: the resampled copies in scratch, or the inputs themselves at fs = 10000.
struct Signals {
  const float* s[4];                     // s1_pred, s2_pred, s1, s2
  int64_t stride;                        // floats between items
};

struct Layout {
  int64_t Tr, nF;                        // samples at 10 kHz, frames
  size_t off_r, off_energy, off_src, off_count, off_bands, total;
};

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

Layout layout(const Handle* h, int B, int64_t T) {
  Layout l;
  l.Tr = h->fs == WM_FS ? T : (T * h->p + h->q - 1) / h->q;
  l.nF = l.Tr >= WM_FRAME ? (l.Tr - WM_FRAME) / WM_HOP + 1 : 0;
  size_t o = 0;
  l.off_r = o;      o += up16(h->fs == WM_FS ? 0 : (size_t)B * 4 * l.Tr * sizeof(float));
  l.off_energy = o; o += up16((size_t)B * 2 * l.nF * sizeof(float));
  l.off_src = o;    o += up16((size_t)B * 2 * l.nF * sizeof(int32_t));
  l.off_count = o;  o += up16((size_t)B * 2 * sizeof(int32_t));
  l.off_bands = o;  o += up16((size_t)B * 6 * l.nF * WM_BAND_STRIDE * sizeof(float));
  l.total = o;
  return l;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Launch 1.  Workgroup = 256 outputs of one signal of one item; y[m] = sum_j g[L + m q - j p] x[j].
__global__ __launch_bounds__(256) void wavmetric_resample_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                                 const float* __restrict__ s1, const float* __restrict__ s2,
                                                                 int64_t T, int64_t Tr, unsigned nchunk, const float* __restrict__ taps,
                                                                 int ntaps, int L, int p, int q, float* __restrict__ r) {
  __shared__ float g[WM_MAX_TAPS];
  for (int i = threadIdx.x; i < ntaps; i += 256) g[i] = taps[i];
  __syncthreads();
  const unsigned chunk = blockIdx.x % nchunk, rest = blockIdx.x / nchunk;
  const int which = rest & 3;
  const int64_t b = rest >> 2;
  const float* x = (which == 0 ? p1 : which == 1 ? p2 : which == 2 ? s1 : s2) + b * T;
  const int64_t m = (int64_t)chunk * 256 + threadIdx.x;
  if (m >= Tr) return;
  const int64_t top = L + m * q;                               // tap index that meets x[0]
  const int64_t lowest = top - 2 * (int64_t)L;                 // j p >= lowest
  int64_t jlo = lowest > 0 ? (lowest + p - 1) / p : 0;
  int64_t jhi = top / p;
  if (jhi > T - 1) jhi = T - 1;
  float acc = 0.f;
  for (int64_t j = jlo; j <= jhi; ++j) acc = fmaf(g[top - j * p], x[j], acc);
  r[(b * 4 + which) * Tr + m] = acc;
}

// Launch 2.  Workgroup = (item b, target j): e_k = 20 log10(|w x_k| + EPS) of every frame of the clean signal, keep
// frame k iff e_k > max e - 40; src[0 .. count) lists the kept frames in order.
__global__ __launch_bounds__(256) void wavmetric_mask_kernel(Signals sig, int64_t nF, const float* __restrict__ win,
                                                             float* __restrict__ energy, int32_t* __restrict__ src,
                                                             int32_t* __restrict__ count, int32_t* __restrict__ kept) {
  __shared__ float w[WM_FRAME];
  __shared__ float wmax[4];
  __shared__ int wtot[4];
  const int64_t b = blockIdx.x >> 1;
  const int j = blockIdx.x & 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = sig.s[2 + j] + b * sig.stride;
  float* e = energy + (int64_t)blockIdx.x * nF;
  int32_t* list = src + (int64_t)blockIdx.x * nF;
  w[threadIdx.x] = win[threadIdx.x];
  __syncthreads();
  float emax = -INFINITY;
  for (int64_t k = wave; k < nF; k += 4) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < WM_FRAME / 64; ++i) {
      const int t = lane + 64 * i;
      const float v = w[t] * x[k * WM_HOP + t];
      s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    const float ek = 20.f * log10f(sqrtf(s) + WM_EPS);
    if (lane == 0) e[k] = ek;
    emax = fmaxf(emax, ek);
  }
  if (lane == 0) wmax[wave] = emax;
  __syncthreads();                                             // the energies in global memory are visible to the workgroup
  const float thr = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])) - WM_DYN_RANGE;
  int carry = 0;                                               // kept frames before this round, uniform
  for (int64_t base = 0; base < nF; base += 256) {
    const int64_t k = base + threadIdx.x;
    const bool keep = k < nF && e[k] > thr;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wtot[wave] = __popcll(m);
    __syncthreads();
    int at = carry + __popcll(m & ((1ull << lane) - 1ull));
    for (int v = 0; v < wave; ++v) at += wtot[v];
    if (keep) list[at] = (int32_t)k;
    carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    count[blockIdx.x] = carry;
    kept[blockIdx.x] = carry;
  }
}

// Launch 3.  Workgroup = (tile of 64 compacted frames, item b, target j, signal s of {clean, prediction 1, prediction 2}).
// Compacted signal z = overlap-add of the kept windowed frames at hop 128: sample 128 m + t lies in kept frames m and
// m - 1 (t < 128) or m and m + 1 (t >= 128).  STFT frame m of z is w[t] z[128 m + t]; it goes to LDS as row m of the A
// tile, one half of the 256 samples at a time (the whole tile would not leave room for the power tile in 64 KiB).  Wave v takes the 32-bin column tiles v, v + 4 of the cos and the sin matrix for both 32-row halves: re and im of
// a (frame, bin) land in the same lane and register.
__global__ __launch_bounds__(256) void wavmetric_spectra_kernel(Signals sig, int64_t nF, unsigned ntile, const float* __restrict__ win,
                                                                const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                                const int* __restrict__ edges, const int32_t* __restrict__ src,
                                                                const int32_t* __restrict__ count, float* __restrict__ bands) {
  __shared__ float tile[WM_ROWS * WM_P_STRIDE];                // half an A tile at a time, then the power tile
  __shared__ float w[WM_FRAME];
  __shared__ int edge[WM_BANDS + 1];
  const unsigned mt = blockIdx.x % ntile, rest = blockIdx.x / ntile;     // rest = (b * 2 + j) * 3 + s
  const unsigned bj = rest / 3, s = rest % 3;
  const int64_t b = bj >> 1;
  const int j = bj & 1;
  const int M = count[bj];
  const int m0 = (int)mt * WM_ROWS;
  if (m0 >= M) return;                                         // uniform: launched for "all kept"
  const float* x = sig.s[s == 0 ? 2 + j : (int)s - 1] + b * sig.stride;
  const int32_t* list = src + (int64_t)bj * nF;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  w[threadIdx.x] = win[threadIdx.x];
  if (threadIdx.x <= WM_BANDS) edge[threadIdx.x] = edges[threadIdx.x];
  __syncthreads();
  // lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31] of v_mfma_f32_32x32x2_f32
  const int frag_row = lane & 31, half = lane >> 5;
  f32x16 re[2][2], im[2][2];                                   // [column tile of the wave][32-row half]
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 16; ++i) re[c][h][i] = im[c][h][i] = 0.f;
  const bool two = wave + 4 < WM_TILES;                        // wave 3 has one column tile
  const float* a0 = tile + frag_row * WM_A_STRIDE + half;
  const float* a1 = a0 + 32 * WM_A_STRIDE;
  const int64_t col = wave * 32 + frag_row;
  for (int kh = 0; kh < WM_FRAME; kh += WM_HOP) {              // samples kh .. kh + 127 of every frame
    if (kh) __syncthreads();                                   // every wave has read the first half
    for (int row = wave; row < WM_ROWS; row += 4) {
      const int m = m0 + row;
      int64_t at = 0, other = -1;                              // the frame itself and the kept frame that overlaps this half
      if (m < M) {
        at = (int64_t)list[m] * WM_HOP;
        if (kh == 0 && m >= 1) other = (int64_t)list[m - 1] * WM_HOP + WM_HOP;
        if (kh != 0 && m + 1 < M) other = (int64_t)list[m + 1] * WM_HOP - WM_HOP;
      }
      const int shift = kh == 0 ? WM_HOP : -WM_HOP;
#pragma unroll
      for (int i = 0; i < WM_HOP / 64; ++i) {
        const int t = kh + lane + 64 * i;
        float z = 0.f;
        if (m < M) {
          z = w[t] * x[at + t];
          if (other >= 0) z += w[t + shift] * x[other + t];
          z *= w[t];
        }
        tile[row * WM_A_STRIDE + t - kh] = z;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < WM_HOP; k += 2) {
      const float x0 = a0[k], x1 = a1[k];
      const int64_t o = (int64_t)(kh + k + half) * WM_COLS + col;
      const float c0 = cosT[o], s0 = sinT[o];
      re[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, c0, re[0][0], 0, 0, 0);
      im[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, s0, im[0][0], 0, 0, 0);
      re[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, c0, re[0][1], 0, 0, 0);
      im[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, s0, im[0][1], 0, 0, 0);
      if (two) {
        const float c1 = cosT[o + 128], s1 = sinT[o + 128];
        re[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, c1, re[1][0], 0, 0, 0);
        im[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, s1, im[1][0], 0, 0, 0);
        re[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, c1, re[1][1], 0, 0, 0);
        im[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, s1, im[1][1], 0, 0, 0);
      }
    }
  }
  __syncthreads();                                             // every wave has read its last A fragment
  // D register i of lane l: row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    if (c == 1 && !two) break;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = 32 * h + (i & 3) + 8 * (i >> 2) + 4 * half;
        const float a = re[c][h][i], d = im[c][h][i];
        tile[row * WM_P_STRIDE + (wave + 4 * c) * 32 + frag_row] = fmaf(a, a, d * d);
      }
  }
  __syncthreads();
  float* out = bands + ((int64_t)rest * nF + m0) * WM_BAND_STRIDE;
#pragma unroll
  for (int i = 0; i < WM_ROWS * WM_BAND_STRIDE / 256; ++i) {
    const int id = threadIdx.x + 256 * i;
    const int row = id & (WM_ROWS - 1), band = id / WM_ROWS;   // a wave shares its band: no divergence
    if (m0 + row >= M) continue;
    float sum = 0.f;
    if (band < WM_BANDS) {
      for (int k = edge[band]; k < edge[band + 1]; ++k) sum += tile[row * WM_P_STRIDE + k];
      sum = sqrtf(sum);
    }
    out[row * WM_BAND_STRIDE + band] = sum;                    // column 15 is zero
  }
}

// Launch 4.  Workgroup = (item b, pair (prediction i, target j)); a wave takes the segments v, v + 16, ...; lane l < 30
// owns frame l of the segment and its 15 band values of the clean (x) and the processed (y) signal.
template <bool EXTENDED>
__global__ __launch_bounds__(WM_MEASURE_THREADS) void wavmetric_measure_kernel(int64_t nF, const float* __restrict__ bands,
                                                                               const int32_t* __restrict__ count,
                                                                               float* __restrict__ out) {
  constexpr int NW = WM_MEASURE_THREADS / 64;
  __shared__ double red[NW];
  const int64_t b = blockIdx.x >> 2;
  const int pi = (blockIdx.x >> 1) & 1, j = blockIdx.x & 1;
  const int M = count[b * 2 + j];
  if (M < WM_SEG) {                                            // uniform
    if (threadIdx.x == 0) out[blockIdx.x] = WM_SHORT;
    return;
  }
  const float* X = bands + ((b * 2 + j) * 3 + 0) * nF * WM_BAND_STRIDE;
  const float* Y = bands + ((b * 2 + j) * 3 + 1 + pi) * nF * WM_BAND_STRIDE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = lane < WM_SEG;
  const int J = M - WM_SEG + 1;
  const float n = (float)WM_SEG;
  double acc = 0;
  for (int seg = wave; seg < J; seg += NW) {
    float x[WM_BAND_STRIDE], y[WM_BAND_STRIDE];
#pragma unroll
    for (int q4 = 0; q4 < WM_BAND_STRIDE / 4; ++q4) {
      float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vy = vx;
      if (live) {
        vx = *(const float4*)(X + (int64_t)(seg + lane) * WM_BAND_STRIDE + 4 * q4);
        vy = *(const float4*)(Y + (int64_t)(seg + lane) * WM_BAND_STRIDE + 4 * q4);
      }
      x[4 * q4] = vx.x; x[4 * q4 + 1] = vx.y; x[4 * q4 + 2] = vx.z; x[4 * q4 + 3] = vx.w;
      y[4 * q4] = vy.x; y[4 * q4 + 1] = vy.y; y[4 * q4 + 2] = vy.z; y[4 * q4 + 3] = vy.w;
    }
    float d = 0.f;
    if (!EXTENDED) {
#pragma unroll
      for (int k = 0; k < WM_BANDS; ++k) {
        const float c = sqrtf(wave_sum(x[k] * x[k])) / (sqrtf(wave_sum(y[k] * y[k])) + WM_EPS);
        const float yp = fminf(y[k] * c, x[k] * WM_CLIP);
        const float mx = wave_sum(x[k]) / n, my = wave_sum(yp) / n;      // every lane takes part in a wave sum
        const float xc = live ? x[k] - mx : 0.f;
        const float yc = live ? yp - my : 0.f;
        const float xn = xc / (sqrtf(wave_sum(xc * xc)) + WM_EPS);
        const float yn = yc / (sqrtf(wave_sum(yc * yc)) + WM_EPS);
        d += wave_sum(xn * yn);
      }
    } else {
      float sx = 0.f, sy = 0.f;
#pragma unroll
      for (int k = 0; k < WM_BANDS; ++k) {                     // rows: every band over the 30 frames
        const float rx = wave_sum(x[k]) / n, ry = wave_sum(y[k]) / n;    // every lane takes part in a wave sum
        const float xc = live ? x[k] - rx : 0.f;
        const float yc = live ? y[k] - ry : 0.f;
        x[k] = xc / (sqrtf(wave_sum(xc * xc)) + WM_EPS);
        y[k] = yc / (sqrtf(wave_sum(yc * yc)) + WM_EPS);
        sx += x[k];
        sy += y[k];
      }
      const float mx = sx / WM_BANDS, my = sy / WM_BANDS;      // columns: every frame over the 15 bands, lane-local
      float nx = 0.f, ny = 0.f;
#pragma unroll
      for (int k = 0; k < WM_BANDS; ++k) {
        x[k] -= mx;
        y[k] -= my;
        nx = fmaf(x[k], x[k], nx);
        ny = fmaf(y[k], y[k], ny);
      }
      nx = sqrtf(nx) + WM_EPS;
      ny = sqrtf(ny) + WM_EPS;
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < WM_BANDS; ++k) dot = fmaf(x[k] / nx, y[k] / ny, dot);
      d = wave_sum(live ? dot : 0.f);
    }
    acc += (double)d;
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int v = 0; v < NW; ++v) s += red[v];
    out[blockIdx.x] = (float)(EXTENDED ? s / WM_SEG / (double)J : s / ((double)J * WM_BANDS));
  }
}

// SI-SDR.  Workgroup = (item b, pair): <p, t> and <t, t>, then |a t|^2 and |a t - p|^2 summed directly, all in double.
__global__ __launch_bounds__(WM_SDR_THREADS) void wavmetric_sisdr_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                                         const float* __restrict__ s1, const float* __restrict__ s2,
                                                                         int64_t T, float* __restrict__ out) {
  constexpr int NW = WM_SDR_THREADS / 64;
  __shared__ double red[4][NW];
  __shared__ double total[4];
  const int64_t b = blockIdx.x >> 2;
  const int pair = blockIdx.x & 3;
  const float* p = (pair < 2 ? p1 : p2) + b * T;
  const float* t = ((pair & 1) ? s2 : s1) + b * T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto block_sum2 = [&](double u, double v, int slot) {        // fixed order; totals in total[slot], total[slot + 1]
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      u += __shfl_xor(u, o);
      v += __shfl_xor(v, o);
    }
    if (lane == 0) {
      red[slot][wave] = u;
      red[slot + 1][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      double s = 0;
      for (int i = 0; i < NW; ++i) s += red[slot + threadIdx.x][i];
      total[slot + threadIdx.x] = s;
    }
    __syncthreads();
  };
  double pt = 0, tt = 0;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < T; i += WM_SDR_THREADS) {
    const double pv = p[i], tv = t[i];
    pt += pv * tv;
    tt += tv * tv;
  }
  block_sum2(pt, tt, 0);
  const double eps = (double)FLT_EPSILON;
  const double a = (total[0] + eps) / (total[1] + eps);
  double ss = 0, nn = 0;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < T; i += WM_SDR_THREADS) {
    const double ts = a * (double)t[i], e = ts - (double)p[i];
    ss += ts * ts;
    nn += e * e;
  }
  block_sum2(ss, nn, 2);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(10.0 * log10((total[2] + eps) / (total[3] + eps)));
}

int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

double bessel_i0(double x) {             // power series: converges to double rounding for the |x| <= 6 used here
  double sum = 1, term = 1;
  for (int k = 1; k < 64; ++k) {
    term *= (x / (2.0 * k)) * (x / (2.0 * k));
    sum += term;
    if (term < 1e-20 * sum) break;
  }
  return sum;
}

}  // namespace

extern "C" {

int wavmetric_abi_version(void) { return WAVMETRIC_ABI_VERSION; }

const char* wavmetric_strerror(int code) {
  switch (code) {
    case WAVMETRIC_OK: return "ok";
    case WAVMETRIC_ERR_INVALID:
      return "wavmetric: bad argument (shape, null pointer or handle, sampling rate not 8000 / 10000 / 16000, or scratch too small / "
             "misaligned)";
    case WAVMETRIC_ERR_HIP: return "wavmetric: an allocation, copy or launch failed (no HIP device? libdptnav has no CPU path)";
    default: return "wavmetric: unknown error code";
  }
}

int wavmetric_sisdr_pairs(const float* s1_pred, const float* s2_pred, const float* s1, const float* s2, int B, int64_t T, float* out,
                          void* stream) {
  if (!s1_pred || !s2_pred || !s1 || !s2 || !out) return WAVMETRIC_ERR_INVALID;
  if (B < 1 || B >= (1 << 20) || T < 1) return WAVMETRIC_ERR_INVALID;
  hipLaunchKernelGGL(wavmetric_sisdr_kernel, dim3((unsigned)B * 4u), dim3(WM_SDR_THREADS), 0, (hipStream_t)stream, s1_pred, s2_pred, s1,
                     s2, T, out);
  return hipGetLastError() == hipSuccess ? WAVMETRIC_OK : WAVMETRIC_ERR_HIP;
}

int wavmetric_stoi_create(int fs, int extended, void** handle) {
  if (!handle || (fs != 8000 && fs != 10000 && fs != 16000)) return WAVMETRIC_ERR_INVALID;
  const double pi = 3.14159265358979323846;
  Handle* h = new Handle();
  h->fs = fs;
  h->extended = extended != 0;
  const int d = gcd(WM_FS, fs);
  h->p = WM_FS / d;
  h->q = fs / d;
  // resampling taps (include/wavmetric.h): Kaiser-windowed sinc, beta = 0.1102 * 51.3, normalised to a DC gain of p
  const double fc = 1.0 / (2.0 * (h->p > h->q ? h->p : h->q));
  h->L = (int)ceil(52.0 / (28.714 * fc / 10.0));
  h->ntaps = 2 * h->L + 1;
  std::vector<float> taps(WM_MAX_TAPS, 0.f), win(WM_FRAME), cs((size_t)WM_FRAME * WM_COLS, 0.f), sn((size_t)WM_FRAME * WM_COLS, 0.f);
  if (h->ntaps > WM_MAX_TAPS) {
    delete h;
    return WAVMETRIC_ERR_INVALID;
  }
  {
    const double beta = 0.1102 * 51.3;
    std::vector<double> hh(h->ntaps);
    double sum = 0;
    for (int i = 0; i < h->ntaps; ++i) {
      const double t = i - h->L, r = t / h->L;
      const double kaiser = bessel_i0(beta * sqrt(1.0 - r * r)) / bessel_i0(beta);
      const double arg = pi * 2.0 * fc * t;
      const double sinc = t == 0 ? 1.0 : sin(arg) / arg;
      hh[i] = kaiser * 2.0 * h->p * fc * sinc;
      sum += hh[i];
    }
    for (int i = 0; i < h->ntaps; ++i) taps[i] = (float)(h->p * hh[i] / sum);
  }
  // hanning(258)[1:-1]
  for (int t = 0; t < WM_FRAME; ++t) win[t] = (float)(0.5 - 0.5 * cos(2.0 * pi * (t + 1) / (WM_FRAME + 1)));
  // one-third octave bands, pystoi's rule: the bin nearest to each band's lower / upper edge frequency
  int edges[WM_BANDS + 1], lo[WM_BANDS], hi[WM_BANDS];
  for (int b = 0; b < WM_BANDS; ++b) {
    const double fl = 150.0 * pow(2.0, (2.0 * b - 1.0) / 6.0), fh = 150.0 * pow(2.0, (2.0 * b + 1.0) / 6.0);
    double bl = 1e300, bh = 1e300;
    lo[b] = hi[b] = 0;
    for (int k = 0; k <= WM_NFFT / 2; ++k) {
      const double f = (double)WM_FS * k / WM_NFFT;
      if ((f - fl) * (f - fl) < bl) { bl = (f - fl) * (f - fl); lo[b] = k; }
      if ((f - fh) * (f - fh) < bh) { bh = (f - fh) * (f - fh); hi[b] = k; }
    }
  }
  bool contiguous = hi[WM_BANDS - 1] - lo[0] <= WM_COLS;
  for (int b = 0; b + 1 < WM_BANDS; ++b) contiguous = contiguous && hi[b] == lo[b + 1];
  if (!contiguous) {                     // cannot happen at 10 kHz / 512: the kernels rely on touching bands
    delete h;
    return WAVMETRIC_ERR_INVALID;
  }
  h->bin_lo = lo[0];
  for (int b = 0; b < WM_BANDS; ++b) edges[b] = lo[b] - h->bin_lo;
  edges[WM_BANDS] = hi[WM_BANDS - 1] - h->bin_lo;
  // DFT twiddles of the bins any band reads; the angle is reduced in integers first
  for (int t = 0; t < WM_FRAME; ++t)
    for (int c = 0; c < edges[WM_BANDS]; ++c) {
      const double ang = 2.0 * pi * (double)((t * (h->bin_lo + c)) % WM_NFFT) / WM_NFFT;
      cs[(size_t)t * WM_COLS + c] = (float)cos(ang);
      sn[(size_t)t * WM_COLS + c] = (float)sin(ang);
    }
  const size_t n_taps = WM_MAX_TAPS * sizeof(float), n_win = WM_FRAME * sizeof(float), n_tw = cs.size() * sizeof(float);
  const size_t n_edges = sizeof(edges);
  char* dev = nullptr;
  if (hipMalloc((void**)&dev, n_taps + n_win + 2 * n_tw + n_edges) != hipSuccess) {
    (void)hipGetLastError();
    delete h;
    return WAVMETRIC_ERR_HIP;
  }
  bool ok = hipMemcpy(dev, taps.data(), n_taps, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(dev + n_taps, win.data(), n_win, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(dev + n_taps + n_win, cs.data(), n_tw, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(dev + n_taps + n_win + n_tw, sn.data(), n_tw, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(dev + n_taps + n_win + 2 * n_tw, edges, n_edges, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    (void)hipFree(dev);
    delete h;
    return WAVMETRIC_ERR_HIP;
  }
  h->dev = dev;
  h->taps = (const float*)dev;
  h->win = (const float*)(dev + n_taps);
  h->cosT = (const float*)(dev + n_taps + n_win);
  h->sinT = (const float*)(dev + n_taps + n_win + n_tw);
  h->edges = (const int*)(dev + n_taps + n_win + 2 * n_tw);
  *handle = h;
  return WAVMETRIC_OK;
}

void wavmetric_stoi_destroy(void* handle) {
  Handle* h = (Handle*)handle;
  if (!h) return;
  (void)hipFree(h->dev);
  delete h;
}

size_t wavmetric_stoi_scratch_bytes(void* handle, int B, int64_t T) {
  if (!handle || B < 1 || T < 1 || B >= (1 << 20) || T >= ((int64_t)1 << 27)) return 0;
  return layout((const Handle*)handle, B, T).total;
}

int wavmetric_stoi_pairs(void* handle, const float* s1_pred, const float* s2_pred, const float* s1, const float* s2, int B, int64_t T,
                         float* out, int32_t* kept, void* scratch, size_t scratch_bytes, void* stream) {
  const Handle* h = (const Handle*)handle;
  if (!h || !s1_pred || !s2_pred || !s1 || !s2 || !out || !kept) return WAVMETRIC_ERR_INVALID;
  if (B < 1 || B >= (1 << 20) || T < 1 || T >= ((int64_t)1 << 27)) return WAVMETRIC_ERR_INVALID;
  const Layout l = layout(h, B, T);
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < l.total) return WAVMETRIC_ERR_INVALID;
  const int64_t nchunk = (l.Tr + 255) / 256, ntile = (l.nF + WM_ROWS - 1) / WM_ROWS;
  if (nchunk * B * 4 >= ((int64_t)1 << 31) || ntile * B * 6 >= ((int64_t)1 << 31)) return WAVMETRIC_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  float* energy = (float*)(base + l.off_energy);
  int32_t* src = (int32_t*)(base + l.off_src);
  int32_t* count = (int32_t*)(base + l.off_count);
  float* bands = (float*)(base + l.off_bands);
  Signals sig;
  if (h->fs == WM_FS) {
    sig.s[0] = s1_pred; sig.s[1] = s2_pred; sig.s[2] = s1; sig.s[3] = s2;
    sig.stride = T;
  } else {
    float* r = (float*)(base + l.off_r);
    hipLaunchKernelGGL(wavmetric_resample_kernel, dim3((unsigned)(nchunk * B * 4)), dim3(256), 0, st, s1_pred, s2_pred, s1, s2, T, l.Tr,
                       (unsigned)nchunk, h->taps, h->ntaps, h->L, h->p, h->q, r);
    for (int i = 0; i < 4; ++i) sig.s[i] = r + i * l.Tr;
    sig.stride = 4 * l.Tr;
  }
  hipLaunchKernelGGL(wavmetric_mask_kernel, dim3((unsigned)B * 2u), dim3(256), 0, st, sig, l.nF, h->win, energy, src, count, kept);
  if (ntile > 0)
    hipLaunchKernelGGL(wavmetric_spectra_kernel, dim3((unsigned)(ntile * B * 6)), dim3(256), 0, st, sig, l.nF, (unsigned)ntile, h->win,
                       h->cosT, h->sinT, h->edges, src, count, bands);
  if (h->extended)
    hipLaunchKernelGGL(wavmetric_measure_kernel<true>, dim3((unsigned)B * 4u), dim3(WM_MEASURE_THREADS), 0, st, l.nF, bands, count, out);
  else
    hipLaunchKernelGGL(wavmetric_measure_kernel<false>, dim3((unsigned)B * 4u), dim3(WM_MEASURE_THREADS), 0, st, l.nF, bands, count, out);
  return hipGetLastError() == hipSuccess ? WAVMETRIC_OK : WAVMETRIC_ERR_HIP;
}

}  // extern "C"
