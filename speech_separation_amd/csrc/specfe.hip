// specfe.hip -- the spectral front end on the device (include/specfe.h): STFT, inverse STFT, their adjoints, log-mel; and
// VoiceFilter's two waveform ends on the same transform (include/vfwave.h).
//
//   STFT.stft            src/encoders/stft.py:25-38                  (torch.stft, then stack / transpose / contiguous)
//   torch.istft          src/model/rtfsnet.py:843-849                (AudioDecoder)
//   get_spectrogram      src/datasets/base_dataset.py:115-123,165    (torchaudio MelSpectrogram, clamp, log; on loader threads)
//
// Three kernels, one launch per call, no scratch:
//   dft     analysis: frames x twiddles as a GEMM on v_mfma_f32_32x32x2_f32 (exact fp32).  Workgroup = 32 frames of one
//           item.  The A tile is built in LDS 128 samples at a time straight from the signal: framing, reflect indexing and
//           the window happen in that load, no padded signal and no frame matrix ever exist in HBM.  Wave v takes the 32-bin
//           column tiles v, v + 4, v + 8 of the cos and the -sin table: re and im of a (frame, bin) land in the same lane
//           and register.  Four modes share the loop:
//             STFT        A = w[t] xp[m H + t]; the epilogue writes [B][2][M][F] directly
//             LOGMEL      same A; the epilogue squares into an LDS power tile, multiplies with the sparse mel filterbank,
//                         clamps, takes the log and writes [B][n_mels][M]
//             ISTFT_BWD   A = w[t] gy[m H + t - N / 2] / env; the epilogue scales by c_k / N and zeroes Im of bins 0, N / 2
//                         (the adjoint of the synthesis IS an analysis of the enveloped gradient)
//             VF          same A, but the MFMA operands change places: the table fragment is the A operand and the frames the
//                         B operand, so the accumulators hold the TRANSPOSED tile, a lane owns one frame and its registers
//                         run over the bins.  The epilogue turns (Re, Im) into VoiceFilter's normalised dB magnitude and the
//                         unit phasor and stores both as [B][F][W] straight from the registers: the 32 lanes of a half wave
//                         write 32 consecutive frames of one bin, no pass through LDS
//   gather  synthesis: one thread per output sample walks the frames that overlap it in ascending order and sums the
//           N-term inverse DFT of each from one period of cos / sin in LDS.  Two modes:
//             ISTFT       y[j] = z[N / 2 + j] / (N env[N / 2 + j])
//             STFT_BWD    gx[j] = g(j) + g(-j) + g(2 (T - 1) - j): the padded gradient and the two reflected ends, in that
//                         order (the adjoint of the analysis IS a synthesis without the envelope)
//           Plain VALU: at 2 frames x 256 terms per sample the synthesis of a [16][32000] batch is 0.26 GFLOP and the kernel
//           needs no intermediate frame matrix.
//   synth   vfwave_synthesis: the ISTFT gather on X = 10^(5 clamp(p, 0, 1) - 4) (phasor[0] + i phasor[1]).  A workgroup of
//           256 output samples stages the complex rows of the frames its samples overlap in LDS, VF_FRAMES at a time,
//           denormalising every (frame, bin) ONCE while it does; the threads then gather from LDS, frames ascending.
// env is summed in double from the fp32 window.  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/specfe.h"
#include "../../include/vfwave.h"

namespace {

constexpr int SF_MAX_N = 512;
constexpr int SF_ROWS = 32;              // frames per workgroup of the dft kernel
constexpr int SF_KC = 128;               // samples of every frame in LDS at a time
constexpr int SF_A_STRIDE = SF_KC + 1;   // odd: fragment reads spread over the banks
constexpr int SF_MAX_FP = 288;           // F = 257 bins rounded up to column tiles of 32
constexpr int SF_P_STRIDE = SF_MAX_FP + 1;
constexpr int SF_TILES = 3;              // column tiles per wave: ceil(9 / 4)
constexpr int SF_KB = 8;                 // MFMA steps (of 2 samples) whose table fragments are in flight together
constexpr int SF_MAX_MELS = 256;
constexpr float SF_CLAMP = 1e-5f;
constexpr float SF_LOG_CLAMP = -11.512925464970229f;       // log(1e-5) rounded once: what a clamped band gets, whatever logf's last bits are

constexpr int VF_FRAMES = 16;            // frames of the denormalised spectrum in LDS at a time (vfwave_synthesis)
constexpr float VF_FLOOR = 1e-5f;        // get_magnitude's clamp of |S|

enum { MODE_STFT = 0, MODE_LOGMEL = 1, MODE_ISTFT_BWD = 2, MODE_VF = 3 };

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Handle {
  int N, H, F, Fp, n_mels, sr;
  void* dev;                             // one allocation: window | cos | -sin | cos period | sin period | filterbank | ranges
  const float *win, *cosT, *sinT, *cos1, *sin1, *fb;
  const int* rng;                        // [n_mels][2]: band j is non-zero on bins [rng[2 j], rng[2 j + 1])
};

struct DftArgs {
  const float* src;                      // x [B][T], or gy [B][L]
  float* out;
  int64_t T;                             // samples per item of src
  int64_t M;
  unsigned ntile;
  int N, H, F, Fp, n_mels;
  const float *win, *cosT, *sinT, *fb;
  const int* rng;
  float* out2;                           // MODE_VF: the phasor [B][2][F][M] (out is spec [B][F][M])
};

// env[n] = sum of w[n - m H]^2 over the frames 0 <= m < M that contain n, ascending m, in double
__device__ __forceinline__ double env_at(const float* w, int64_t n, int N, int H, int64_t M) {
  int64_t lo = n >= N ? (n - N) / H + 1 : 0, hi = n / H;
  if (hi > M - 1) hi = M - 1;
  double e = 0;
  for (int64_t m = lo; m <= hi; ++m) {
    const double v = (double)w[n - m * H];
    e += v * v;
  }
  return e;
}

template <int MODE>
__global__ __launch_bounds__(256) void specfe_dft_kernel(DftArgs a) {
  __shared__ float tile[SF_ROWS * SF_P_STRIDE];                // the A tile, 128 samples at a time; then the power tile
  __shared__ float w[SF_MAX_N];
  const int N = a.N, H = a.H, F = a.F, Fp = a.Fp;
  const int64_t M = a.M, T = a.T;
  const int64_t b = blockIdx.x / a.ntile;
  const int64_t m0 = (int64_t)(blockIdx.x % a.ntile) * SF_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = threadIdx.x; t < N; t += 256) w[t] = a.win[t];
  __syncthreads();
  const float* src = a.src + b * T;
  // lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31] of v_mfma_f32_32x32x2_f32
  const int frag_row = lane & 31, half = lane >> 5;
  const int nb = Fp / 32;
  f32x16 re[SF_TILES], im[SF_TILES];
#pragma unroll
  for (int c = 0; c < SF_TILES; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) re[c][i] = im[c][i] = 0.f;
  const float* afrag = tile + frag_row * SF_A_STRIDE + half;
  for (int kh = 0; kh < N; kh += SF_KC) {
    const int kc = N - kh < SF_KC ? N - kh : SF_KC;            // even: N is a multiple of 16
    if (kh) __syncthreads();                                   // every wave has read the previous chunk
    for (int row = wave; row < SF_ROWS; row += 4) {
      const int64_t m = m0 + row;
      for (int t0 = lane; t0 < kc; t0 += 64) {
        const int t = kh + t0;
        float v = 0.f;
        if (m < M) {
          if (MODE == MODE_ISTFT_BWD) {
            const int64_t n = m * H + t, j = n - N / 2;
            if (j >= 0 && j < T) {
              const double e = env_at(w, n, N, H, M);
              if (e > 0) v = w[t] * (float)((double)src[j] / e);
            }
          } else {
            int64_t i = m * H + t - N / 2;                     // reflect: one fold is enough for T > N / 2
            if (i < 0) i = -i;
            if (i >= T) i = 2 * (T - 1) - i;
            if (i >= 0 && i < T) v = w[t] * src[i];
          }
        }
        tile[row * SF_A_STRIDE + t0] = v;
      }
    }
    __syncthreads();
    // The table fragments of SF_KB MFMA steps are requested together, then consumed: one round trip to L2 per 16 samples
    // instead of one per step (a workgroup's time is this chain of latencies, not its arithmetic).  kc is a multiple of 16.
    for (int k0 = 0; k0 < kc; k0 += 2 * SF_KB) {
      float cv[SF_KB][SF_TILES], sv[SF_KB][SF_TILES];
#pragma unroll
      for (int u = 0; u < SF_KB; ++u) {
        const int o = (kh + k0 + 2 * u + half) * Fp + frag_row;
#pragma unroll
        for (int c = 0; c < SF_TILES; ++c) {
          const int ct = wave + 4 * c;
          const bool on = ct < nb;                             // uniform over the wave
          cv[u][c] = on ? a.cosT[o + ct * 32] : 0.f;
          sv[u][c] = on ? a.sinT[o + ct * 32] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < SF_KB; ++u) {
        const float x0 = afrag[k0 + 2 * u];
#pragma unroll
        for (int c = 0; c < SF_TILES; ++c) {
          if (wave + 4 * c < nb) {
            if (MODE == MODE_VF) {                             // D^T = table^T frames^T: the same products, bins down the registers
              re[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(cv[u][c], x0, re[c], 0, 0, 0);
              im[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[u][c], x0, im[c], 0, 0, 0);
            } else {
              re[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, cv[u][c], re[c], 0, 0, 0);
              im[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, sv[u][c], im[c], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  // D register i of lane l: row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31
  if (MODE == MODE_VF) {                                       // rows are bins, columns frames: lane l owns frame m0 + (l & 31)
    const int64_t m = m0 + frag_row;
    float* spec = a.out + b * F * M;
    float* ph = a.out2 + b * 2 * F * M;
#pragma unroll
    for (int c = 0; c < SF_TILES; ++c) {
      const int ct = wave + 4 * c;
      if (ct >= nb) continue;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = ct * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
        if (k >= F || m >= M) continue;
        const float p = re[c][i], q = im[c][i];
        const float mag = sqrtf(fmaf(p, p, q * q));
        const float db = (20.f * log10f(fmaxf(mag, VF_FLOOR)) - 20.f) / 100.f;
        spec[k * M + m] = mag >= 10.f ? 1.f : fminf(fmaxf(db, -1.f), 0.f) + 1.f;   // |S| >= 10 is 1 whatever log10f's last bit is
        ph[k * M + m] = mag > 0.f ? p / mag : 1.f;                                  // angle(0) = 0
        ph[(F + k) * M + m] = mag > 0.f ? q / mag : 0.f;
      }
    }
  } else if (MODE != MODE_LOGMEL) {
    float* out = a.out + b * 2 * M * F;
#pragma unroll
    for (int c = 0; c < SF_TILES; ++c) {
      const int k = (wave + 4 * c) * 32 + frag_row;
      if (k >= F) continue;
      float sr = 1.f, si = 1.f;
      if (MODE == MODE_ISTFT_BWD) {
        const bool edge = k == 0 || k == N / 2;
        sr = (float)((edge ? 1.0 : 2.0) / N);
        si = edge ? 0.f : sr;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t m = m0 + (i & 3) + 8 * (i >> 2) + 4 * half;
        if (m >= M) continue;
        out[m * F + k] = MODE == MODE_ISTFT_BWD ? re[c][i] * sr : re[c][i];
        out[(M + m) * F + k] = MODE == MODE_ISTFT_BWD ? (si == 0.f ? 0.f : im[c][i] * si) : im[c][i];
      }
    }
  } else {
    __syncthreads();                                           // every wave has read its last A fragment
#pragma unroll
    for (int c = 0; c < SF_TILES; ++c) {
      const int ct = wave + 4 * c;
      if (ct >= nb) continue;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * half;
        const float p = re[c][i], q = im[c][i];
        tile[row * SF_P_STRIDE + ct * 32 + frag_row] = fmaf(p, p, q * q);
      }
    }
    __syncthreads();
    const int n_mels = a.n_mels;
    float* out = a.out + b * n_mels * M;
    for (int id = threadIdx.x; id < SF_ROWS * n_mels; id += 256) {
      const int row = id & (SF_ROWS - 1), mel = id / SF_ROWS;
      const int64_t m = m0 + row;
      if (m >= M) continue;
      const float* f = a.fb + (int64_t)mel * Fp;
      const int hi = a.rng[2 * mel + 1];
      float s = 0.f;
      for (int k = a.rng[2 * mel]; k < hi; ++k) s = fmaf(f[k], tile[row * SF_P_STRIDE + k], s);
      out[(int64_t)mel * M + m] = s <= SF_CLAMP ? SF_LOG_CLAMP : logf(s);      // a NaN goes through logf, as torch's clamp lets it
    }
  }
}

// sum over the frames m that contain the padded sample n (ascending) of w[t] [Re X_m,0 + (-1)^t Re X_m,N/2 +
// C sum_{0<k<N/2} (Re X_m,k cos(2 pi k t / N) - Im X_m,k sin(2 pi k t / N))], t = n - m H.  0 where no frame reaches.
template <int C>
__device__ __forceinline__ float gather_at(const float* __restrict__ Xb, int64_t n, int N, int H, int F, int64_t M, const float* w,
                                           const float* cs, const float* sn) {
  int64_t lo = n >= N ? (n - N) / H + 1 : 0, hi = n / H;
  if (hi > M - 1) hi = M - 1;
  float s = 0.f;
  for (int64_t m = lo; m <= hi; ++m) {
    const int t = (int)(n - m * H);
    const float* re = Xb + m * F;
    const float* im = Xb + (M + m) * F;
    const float edge = (t & 1) ? re[0] - re[N / 2] : re[0] + re[N / 2];
    float acc = 0.f;
    int idx = 0;                                               // k t mod N
    for (int k = 1; k < N / 2; ++k) {
      idx += t;
      if (idx >= N) idx -= N;
      acc = fmaf(re[k], cs[idx], acc);
      acc = fmaf(-im[k], sn[idx], acc);
    }
    s = fmaf(w[t], fmaf((float)C, acc, edge), s);
  }
  return s;
}

// ISTFT: X [B][2][M][F] -> y [B][L].  STFT_BWD (INV == false): gX [B][2][M][F] -> gx [B][L], L = T.
template <bool INV>
__global__ __launch_bounds__(256) void specfe_gather_kernel(const float* __restrict__ X, int64_t M, int64_t L, unsigned nchunk, int N, int H,
                                                            int F, const float* __restrict__ win, const float* __restrict__ cos1,
                                                            const float* __restrict__ sin1, float* __restrict__ out) {
  __shared__ float w[SF_MAX_N], cs[SF_MAX_N], sn[SF_MAX_N];
  for (int t = threadIdx.x; t < N; t += 256) {
    w[t] = win[t];
    cs[t] = cos1[t];
    sn[t] = sin1[t];
  }
  __syncthreads();
  const int64_t b = blockIdx.x / nchunk;
  const int64_t j = (int64_t)(blockIdx.x % nchunk) * 256 + threadIdx.x;
  if (j >= L) return;
  const float* Xb = X + b * 2 * M * F;
  float v;
  if (INV) {
    const int64_t n = j + N / 2;
    const double e = env_at(w, n, N, H, M);
    v = e > 0 ? (float)((double)gather_at<2>(Xb, n, N, H, F, M, w, cs, sn) / ((double)N * e)) : 0.f;
  } else {
    const int64_t T = L;
    v = gather_at<1>(Xb, j + N / 2, N, H, F, M, w, cs, sn);
    if (j >= 1 && j <= N / 2) v += gather_at<1>(Xb, N / 2 - j, N, H, F, M, w, cs, sn);                       // left reflection
    if (j >= T - 1 - N / 2 && j <= T - 2) v += gather_at<1>(Xb, 2 * (T - 1) - j + N / 2, N, H, F, M, w, cs, sn);   // right reflection
  }
  out[b * L + j] = v;
}

// pred [S][B][F][M], phasor [B][2][F][M] -> y [S][B][L]: specfe_gather_kernel<true> on the denormalised, rotated spectrum.
// blockIdx.x = (source s, item b, chunk of 256 samples).  The frames m_lo .. m_hi that the chunk's samples overlap are staged
// VF_FRAMES at a time as rows xr / xi [frame][F]; a thread adds its own frames of every group in ascending order, so the
// order of its sum does not depend on the grouping.
__global__ __launch_bounds__(256) void vfwave_synth_kernel(const float* __restrict__ pred, const float* __restrict__ phasor, int B,
                                                           int64_t M, int64_t L, unsigned nchunk, int N, int H, int F,
                                                           const float* __restrict__ win, const float* __restrict__ cos1,
                                                           const float* __restrict__ sin1, float* __restrict__ out) {
  __shared__ float w[SF_MAX_N], cs[SF_MAX_N], sn[SF_MAX_N];
  __shared__ float xr[VF_FRAMES * (SF_MAX_N / 2 + 1)], xi[VF_FRAMES * (SF_MAX_N / 2 + 1)];
  for (int t = threadIdx.x; t < N; t += 256) {
    w[t] = win[t];
    cs[t] = cos1[t];
    sn[t] = sin1[t];
  }
  __syncthreads();
  const int64_t sb = blockIdx.x / nchunk, b = sb % B;
  const int64_t j0 = (int64_t)(blockIdx.x % nchunk) * 256, j = j0 + threadIdx.x;
  const bool active = j < L;
  const int64_t n_first = j0 + N / 2, n_last = (j0 + 255 < L ? j0 + 255 : L - 1) + N / 2, n = j + N / 2;
  const int64_t m_lo = n_first >= N ? (n_first - N) / H + 1 : 0;
  const int64_t m_hi = n_last / H < M - 1 ? n_last / H : M - 1;
  const int64_t lo = n >= N ? (n - N) / H + 1 : 0, hi = n / H < M - 1 ? n / H : M - 1;
  const float* ps = pred + sb * F * M;
  const float* p0 = phasor + b * 2 * F * M;
  const float* p1 = p0 + (int64_t)F * M;
  float s = 0.f;
  for (int64_t ma = m_lo; ma <= m_hi; ma += VF_FRAMES) {
    const int nf = m_hi - ma + 1 < VF_FRAMES ? (int)(m_hi - ma + 1) : VF_FRAMES;
    if (ma != m_lo) __syncthreads();                           // every thread is done with the last group
    for (int id = threadIdx.x; id < nf * F; id += 256) {       // frames fastest: odd row stride F, no bank conflict
      const int k = id / nf, g = id - k * nf;
      const int64_t at = k * M + ma + g;
      const float mag = exp10f(fmaf(5.f, fminf(fmaxf(ps[at], 0.f), 1.f), -4.f));
      xr[g * F + k] = mag * p0[at];
      xi[g * F + k] = mag * p1[at];
    }
    __syncthreads();
    if (active) {
      const int64_t a = lo > ma ? lo : ma, e = hi < ma + nf - 1 ? hi : ma + nf - 1;
      for (int64_t m = a; m <= e; ++m) {
        const int t = (int)(n - m * H);
        const float* re = xr + (int)(m - ma) * F;              // gather_at<2>'s term of one frame, its operands in LDS
        const float* im = xi + (int)(m - ma) * F;
        const float edge = (t & 1) ? re[0] - re[N / 2] : re[0] + re[N / 2];
        float acc = 0.f;
        int idx = 0;                                           // k t mod N
        for (int k = 1; k < N / 2; ++k) {                      // im[0] and im[N / 2] are never read
          idx += t;
          if (idx >= N) idx -= N;
          acc = fmaf(re[k], cs[idx], acc);
          acc = fmaf(-im[k], sn[idx], acc);
        }
        s = fmaf(w[t], fmaf(2.f, acc, edge), s);
      }
    }
  }
  if (!active) return;
  const double e = env_at(w, n, N, H, M);
  out[sb * L + j] = e > 0 ? (float)((double)s / ((double)N * e)) : 0.f;
}

// cos and sin of 2 pi idx / N, exact on the axes
void twiddle(int idx, int N, double* c, double* s) {
  const double pi = 3.14159265358979323846;
  if (idx == 0) { *c = 1; *s = 0; }
  else if (2 * idx == N) { *c = -1; *s = 0; }
  else if (4 * idx == N) { *c = 0; *s = 1; }
  else if (4 * idx == 3 * N) { *c = 0; *s = -1; }
  else { *c = cos(2.0 * pi * idx / N); *s = sin(2.0 * pi * idx / N); }
}

bool size_ok(int B, int64_t len) { return B >= 1 && B < (1 << 20) && len >= 1 && len < ((int64_t)1 << 27); }

int create(int n_fft, int hop, int sample_rate, int n_mels, bool mel, void** handle) {
  if (!handle || n_fft < 32 || n_fft > SF_MAX_N || n_fft % 16 || hop < 1 || hop > n_fft / 2) return SPECFE_ERR_INVALID;
  if (mel && (sample_rate < 2 || n_mels < 1 || n_mels > SF_MAX_MELS)) return SPECFE_ERR_INVALID;
  const double pi = 3.14159265358979323846;
  const int N = n_fft, F = N / 2 + 1, Fp = (F + 31) / 32 * 32;
  if (!mel) n_mels = 0;
  std::vector<float> win(N), cs((size_t)N * Fp, 0.f), sn((size_t)N * Fp, 0.f), c1(N), s1(N), fb((size_t)n_mels * Fp, 0.f);
  std::vector<int> rng((size_t)2 * n_mels, 0);
  for (int t = 0; t < N; ++t) {
    win[t] = (float)(0.5 - 0.5 * cos(2.0 * pi * t / N));
    double c, s;
    twiddle(t, N, &c, &s);
    c1[t] = (float)c;
    s1[t] = (float)s;
    for (int k = 0; k < F; ++k) {                              // the angle is reduced in integers first
      twiddle((int)(((int64_t)t * k) % N), N, &c, &s);
      cs[(size_t)t * Fp + k] = (float)c;
      sn[(size_t)t * Fp + k] = (float)(-s);
    }
  }
  if (mel) {                                                   // include/specfe.h: HTK scale, f_min 0, f_max sr / 2, no norm
    const double top = 2595.0 * log10(1.0 + 0.5 * sample_rate / 700.0);
    std::vector<double> f(n_mels + 2);
    for (int j = 0; j < n_mels + 2; ++j) f[j] = 700.0 * (pow(10.0, top * j / (n_mels + 1) / 2595.0) - 1.0);
    for (int j = 0; j < n_mels; ++j) {
      int lo = F, hi = 0;
      for (int k = 0; k < F; ++k) {
        const double g = 0.5 * sample_rate * k / (F - 1);
        const double down = (g - f[j]) / (f[j + 1] - f[j]), up = (f[j + 2] - g) / (f[j + 2] - f[j + 1]);
        const double v = fmax(0.0, fmin(down, up));
        fb[(size_t)j * Fp + k] = (float)v;
        if ((float)v != 0.f) {
          if (k < lo) lo = k;
          hi = k + 1;
        }
      }
      rng[2 * j] = lo < hi ? lo : 0;
      rng[2 * j + 1] = hi;
    }
  }
  const size_t n_win = (size_t)N * sizeof(float), n_tw = cs.size() * sizeof(float), n_fb = fb.size() * sizeof(float);
  const size_t n_rng = rng.size() * sizeof(int);
  char* dev = nullptr;
  if (hipMalloc((void**)&dev, 3 * n_win + 2 * n_tw + n_fb + n_rng + 16) != hipSuccess) {
    (void)hipGetLastError();
    return SPECFE_ERR_HIP;
  }
  char* at = dev;
  const void* srcs[7] = {win.data(), cs.data(), sn.data(), c1.data(), s1.data(), fb.data(), rng.data()};
  const size_t lens[7] = {n_win, n_tw, n_tw, n_win, n_win, n_fb, n_rng};
  char* where[7];
  bool ok = true;
  for (int i = 0; i < 7; ++i) {
    where[i] = at;
    if (lens[i]) ok = ok && hipMemcpy(at, srcs[i], lens[i], hipMemcpyHostToDevice) == hipSuccess;
    at += lens[i];
  }
  if (!ok) {
    (void)hipGetLastError();
    (void)hipFree(dev);
    return SPECFE_ERR_HIP;
  }
  Handle* h = new Handle();
  h->N = N; h->H = hop; h->F = F; h->Fp = Fp; h->n_mels = n_mels; h->sr = mel ? sample_rate : 0;
  h->dev = dev;
  h->win = (const float*)where[0];
  h->cosT = (const float*)where[1];
  h->sinT = (const float*)where[2];
  h->cos1 = (const float*)where[3];
  h->sin1 = (const float*)where[4];
  h->fb = (const float*)where[5];
  h->rng = (const int*)where[6];
  *handle = h;
  return SPECFE_OK;
}

template <int MODE>
int launch_dft(const Handle* h, const float* src, int B, int64_t T, int64_t M, float* out, void* stream, float* out2 = nullptr) {
  const int64_t ntile = (M + SF_ROWS - 1) / SF_ROWS;
  if (ntile * B >= ((int64_t)1 << 31)) return SPECFE_ERR_INVALID;
  DftArgs a;
  a.src = src; a.out = out; a.out2 = out2; a.T = T; a.M = M; a.ntile = (unsigned)ntile;
  a.N = h->N; a.H = h->H; a.F = h->F; a.Fp = h->Fp; a.n_mels = h->n_mels;
  a.win = h->win; a.cosT = h->cosT; a.sinT = h->sinT; a.fb = h->fb; a.rng = h->rng;
  hipLaunchKernelGGL(specfe_dft_kernel<MODE>, dim3((unsigned)(ntile * B)), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? SPECFE_OK : SPECFE_ERR_HIP;
}

template <bool INV>
int launch_gather(const Handle* h, const float* X, int B, int64_t M, int64_t L, float* out, void* stream) {
  const int64_t nchunk = (L + 255) / 256;
  if (nchunk * B >= ((int64_t)1 << 31)) return SPECFE_ERR_INVALID;
  hipLaunchKernelGGL(specfe_gather_kernel<INV>, dim3((unsigned)(nchunk * B)), dim3(256), 0, (hipStream_t)stream, X, M, L, (unsigned)nchunk,
                     h->N, h->H, h->F, h->win, h->cos1, h->sin1, out);
  return hipGetLastError() == hipSuccess ? SPECFE_OK : SPECFE_ERR_HIP;
}

// the output length of the inverse, or 0 when the arguments are out of range
int64_t inverse_length(const Handle* h, int B, int64_t M, int64_t length) {
  if (!h || !size_ok(B, M)) return 0;
  const int64_t L = length > 0 ? length : (M - 1) * h->H;
  return size_ok(B, L) && (M - 1) * h->H + h->N < ((int64_t)1 << 27) ? L : 0;
}

}  // namespace

extern "C" {

int specfe_abi_version(void) { return SPECFE_ABI_VERSION; }

const char* specfe_strerror(int code) {
  switch (code) {
    case SPECFE_OK: return "ok";
    case SPECFE_ERR_INVALID:
      return "specfe: bad argument (null pointer or handle, n_fft not a multiple of 16 in [32, 512], hop not in [1, n_fft / 2], "
             "a signal no longer than n_fft / 2, a size out of range, or a log-mel call on a handle without a filterbank)";
    case SPECFE_ERR_HIP: return "specfe: an allocation, copy or launch failed (no HIP device? libdptnav has no CPU path)";
    default: return "specfe: unknown error code";
  }
}

int specfe_create(int n_fft, int hop, void** handle) { return create(n_fft, hop, 0, 0, false, handle); }

int specfe_create_mel(int n_fft, int hop, int sample_rate, int n_mels, void** handle) {
  return create(n_fft, hop, sample_rate, n_mels, true, handle);
}

void specfe_destroy(void* handle) {
  Handle* h = (Handle*)handle;
  if (!h) return;
  (void)hipFree(h->dev);
  delete h;
}

int specfe_stft(void* handle, const float* x, int B, int64_t T, float* X, void* stream) {
  const Handle* h = (const Handle*)handle;
  if (!h || !x || !X || !size_ok(B, T) || T <= h->N / 2) return SPECFE_ERR_INVALID;
  return launch_dft<MODE_STFT>(h, x, B, T, 1 + T / h->H, X, stream);
}

int specfe_logmel(void* handle, const float* x, int B, int64_t T, float* S, void* stream) {
  const Handle* h = (const Handle*)handle;
  if (!h || !x || !S || h->n_mels < 1 || !size_ok(B, T) || T <= h->N / 2) return SPECFE_ERR_INVALID;
  return launch_dft<MODE_LOGMEL>(h, x, B, T, 1 + T / h->H, S, stream);
}

int specfe_stft_backward(void* handle, const float* gX, int B, int64_t T, float* gx, void* stream) {
  const Handle* h = (const Handle*)handle;
  if (!h || !gX || !gx || !size_ok(B, T) || T <= h->N / 2) return SPECFE_ERR_INVALID;
  return launch_gather<false>(h, gX, B, 1 + T / h->H, T, gx, stream);
}

int specfe_istft(void* handle, const float* X, int B, int64_t M, int64_t length, float* y, void* stream) {
  const Handle* h = (const Handle*)handle;
  const int64_t L = inverse_length(h, B, M, length);
  if (!X || !y || L < 1) return SPECFE_ERR_INVALID;
  return launch_gather<true>(h, X, B, M, L, y, stream);
}

int specfe_istft_backward(void* handle, const float* gy, int B, int64_t M, int64_t length, float* gX, void* stream) {
  const Handle* h = (const Handle*)handle;
  const int64_t L = inverse_length(h, B, M, length);
  if (!gy || !gX || L < 1) return SPECFE_ERR_INVALID;
  return launch_dft<MODE_ISTFT_BWD>(h, gy, B, L, M, gX, stream);
}

int vfwave_abi_version(void) { return VFWAVE_ABI_VERSION; }

const char* vfwave_strerror(int code) {
  switch (code) {
    case VFWAVE_OK: return "ok";
    case VFWAVE_ERR_INVALID:
      return "vfwave: bad argument (null pointer or handle, a signal no longer than n_fft / 2, n_src not in [1, 4], or a size out "
             "of range)";
    case VFWAVE_ERR_HIP: return "vfwave: the launch failed (no HIP device? libdptnav has no CPU path)";
    default: return "vfwave: unknown error code";
  }
}

int vfwave_analysis(void* handle, const float* x, int B, int64_t T, float* spec, float* phasor, void* stream) {
  const Handle* h = (const Handle*)handle;
  if (!h || !x || !spec || !phasor || !size_ok(B, T) || T <= h->N / 2) return VFWAVE_ERR_INVALID;
  return launch_dft<MODE_VF>(h, x, B, T, 1 + T / h->H, spec, stream, phasor);
}

int vfwave_synthesis(void* handle, const float* pred, const float* phasor, int n_src, int B, int64_t W, int64_t length, float* y,
                     void* stream) {
  const Handle* h = (const Handle*)handle;
  const int64_t L = inverse_length(h, B, W, length);
  if (!pred || !phasor || !y || L < 1 || n_src < 1 || n_src > VFWAVE_MAX_SRC) return VFWAVE_ERR_INVALID;
  const int64_t nchunk = (L + 255) / 256;
  if (nchunk * B * n_src >= ((int64_t)1 << 31)) return VFWAVE_ERR_INVALID;
  hipLaunchKernelGGL(vfwave_synth_kernel, dim3((unsigned)(nchunk * B * n_src)), dim3(256), 0, (hipStream_t)stream, pred, phasor, B, W, L,
                     (unsigned)nchunk, h->N, h->H, h->F, h->win, h->cos1, h->sin1, y);
  return hipGetLastError() == hipSuccess ? VFWAVE_OK : VFWAVE_ERR_HIP;
}

}  // extern "C"
