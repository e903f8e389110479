// deepctasnet_train.hip -- DeepConvTasNet and DeepAVConvTasNet training steps (src/model/deepconvtasnet.py,
// src/model/deepavconvtasnet.py: forward + autograd backward) for gfx950: handles and the extern "C" boundaries declared in
// include/dctasnet_train.h (dcttrain_*, audio only) and include/davctasnet_train.h (davtrain_*, audio-visual).  One plan, one
// forward body and one backward body serve both; the audio-visual handle takes the `av` branches.
//
// Training forward: the launch sequence of deepctasnet.hip in its TAPE mode (deepctasnet_kernels.h, ctasnet_kernels.h: one
// text for both), so the predictions are bitwise those of dctasnet_forward.  On top of the Separator's tape
// (ctasnet_train_kernels.h) the tape keeps the first conv's output c0 [M][512] and, for each of the eight dense k = 3
// layers, its pre-activation z (encoder [M][512], decoder [2M][512], rows (b, f, speaker)): the slopes may be 0, 1 or
// negative, so the sign of z cannot be recovered from PReLU(z).  Only z is stored; the next layer's A loader applies the
// PReLU.  The two activations that plain-row kernels read -- the encoder output enc (the Separator's tape has it) and the
// last decoder activation (the taps kernel; scratch, not tape) -- are stored as well.
//
// Backward, last layer to first: output head (taps gradient, d bias, d W from PReLU(z_3) and the taps gradient, d y_3 =
// d taps W^T), four ConvTranspose layers, mask head in its d ym form + launch_separator_backward, four Conv1d layers,
// first conv.  Per dense layer: PReLU backward in place (slope partials), bias column sums, three taps x four 128-column
// slices of the MFMA weight-gradient kernel (backward.h wgrad_kernel<512, 128>, static tile schedule) through tap-shifted
// loaders, and the data gradient as three accumulating passes of the engine on the weights packed in the other
// orientation (a Conv1d's data gradient is the ConvTranspose form and vice versa) with the shifts negated.  The pack runs
// at the start of every backward from the weights as they are then.  No atomics: every partial goes to a slab and is
// summed in a fixed order, so two backward calls on one tape give bitwise-identical gradients.
// decoder.deconv.weight is never read by the reference's forward: its gradient buffer is never written and
// *_adamw_step leaves the weight alone.
//
// Audio-visual head (deepavconvtasnet.py:140-155).  Forward: the two video launches of deepctasnet.hip run before the
// encoder, vcat [B Tv][512] stays on the tape and the video rows sit in scratch until the last dense encoder pass adds
// them in its epilogue and writes the GlobalNorm partials of the fused tensor; the tape's enc is the fused tensor.
// Backward: d fused = the Separator backward's d enc is also d vid.  The encoder's PReLU backward works in place, so the
// video backward runs between launch_separator_backward and encoder layer 3 and reads d fused before it is overwritten:
// (1) one workgroup per (b, t) walks the frames that interpolate from video row t in ascending f, recomputes the
// interpolated row, mu and rstd from vcat with the forward's float operations, forms the LayerNorm's data gradient and
// gathers its weighted sum into d vcat[b, t] (no scatter); the frames whose i0 is t also give the workgroup's partial of
// d gamma, d beta (each frame has one such t), summed afterwards in (b, t) order; (2) the Linear's d W, d b as register
// tiles over fixed row chunks of d vcat, the embeddings staged through LDS along their time axis, partials summed in chunk
// order.  Nothing of size [M][512] is written for the head; the embeddings get no gradient.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/davctasnet_train.h"
#include "../../include/dctasnet_train.h"
#include "ctasnet_train_kernels.h"
#include "deepctasnet_kernels.h"

static_assert(DCTTRAIN_OK == CTASNET_OK && DCTTRAIN_ERR_INVALID == CTASNET_ERR_INVALID &&
                  DCTTRAIN_ERR_WORKSPACE == CTASNET_ERR_WORKSPACE && DCTTRAIN_ERR_WEIGHTS == CTASNET_ERR_WEIGHTS &&
                  DCTTRAIN_ERR_HIP == CTASNET_ERR_HIP,
              "the shared Conv-TasNet code returns CTASNET_* codes");
static_assert(DAVTRAIN_OK == CTASNET_OK && DAVTRAIN_ERR_INVALID == CTASNET_ERR_INVALID &&
                  DAVTRAIN_ERR_WORKSPACE == CTASNET_ERR_WORKSPACE && DAVTRAIN_ERR_WEIGHTS == CTASNET_ERR_WEIGHTS &&
                  DAVTRAIN_ERR_HIP == CTASNET_ERR_HIP,
              "the shared Conv-TasNet code returns CTASNET_* codes");

namespace {

constexpr int DCT_G_W = 256;                        // workgroups of a dense weight-gradient launch (at most): one per CU
constexpr int DCT_WN = CT_N, DCT_WK = 128;          // its tile: dW[512][128 columns of one tap]
constexpr int DCT_UNUSED = DC_DEC0 + 14;            // decoder.deconv.weight
constexpr int DAV_KT = 32;                          // video Linear backward: input channels (columns of dW) per workgroup
constexpr int DAV_TT = 64;                          // video frames of one mixture per row chunk
constexpr int DAV_LD = DAV_KT + 4;                  // LDS row stride of the staged embeddings (float4 reads stay aligned)
constexpr int DAV_G_R = 64;                         // row-chunk workgroups (at most): one partial dW [256][512] each
static_assert((size_t)DAV_G_R * DC_HV * CT_N <= (size_t)DCT_G_W * DCT_WN * DCT_WK, "the dense wgrad slab holds the Linear's partials");
static_assert(DAV_G_R * DC_HV <= CTT_G_C * 2 * CT_N, "the column-sum slab holds the Linear's bias partials");

thread_local std::string g_create_error;

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// d bias of the output head: the sum of d_s1 and d_s2 over all cropped samples; per-workgroup partials -> aslab
__global__ __launch_bounds__(256) void dcttrain_outsum_kernel(const float* __restrict__ d1, const float* __restrict__ d2,
                                                              int64_t n, float* __restrict__ aslab) {
  __shared__ float red[256];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += d1[i] + d2[i];
  const float t = block_sum256(s, red);
  if (threadIdx.x == 0) aslab[blockIdx.x] = t;
}

// Sum of wgrad_kernel's partial tiles (fragment order, see slab_reduce_frag_kernel in backward.h: same association
// order) into a strided destination: element (row, col) of the [32 RB * 4][32 CB] tile goes to out[row * ldo + col * cs].
// One tap's 128-column slice of a dense layer's weight gradient lands in weight[.][.][k] this way (ldo = 1536, cs = 3).
template <int RB, int CB>
__global__ __launch_bounds__(256) void dcttrain_reduce_frag_kernel(const float* __restrict__ slab, int nslabs, int64_t stride,
                                                                   float* __restrict__ out, int ldo, int cs) {
  __shared__ float4 red[8][32];
  const int e = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int f = blockIdx.x * 32 + e;                 // < RB * CB * 1024
  const float4* src = reinterpret_cast<const float4*>(slab) + f;
  const int64_t st4 = stride / 4;
  auto add = [](float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; };
  float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
  int k = sl;
  for (; k + 24 < nslabs; k += 32) {
    add(s0, src[(int64_t)k * st4]);
    add(s1, src[(int64_t)(k + 8) * st4]);
    add(s2, src[(int64_t)(k + 16) * st4]);
    add(s3, src[(int64_t)(k + 24) * st4]);
  }
  for (; k < nslabs; k += 8) add(s0, src[(int64_t)k * st4]);
  add(s0, s1);
  add(s2, s3);
  add(s0, s2);
  red[sl][e] = s0;
  __syncthreads();
  if (sl == 0) {
    float4 s = red[0][e];
#pragma unroll
    for (int j = 1; j < 8; ++j) add(s, red[j][e]);
    const int lane = f & 63, g4 = (f >> 6) & 3, t = f >> 8;          // t = (w * RB + i) * CB + j
    const int j = t % CB, wi = t / CB, i = wi % RB, w = wi / RB;
    const int row = (w + 4 * i) * 32 + 8 * g4 + 4 * (lane >> 5), col = j * 32 + (lane & 31);
    float* dst = out + (size_t)row * ldo + (size_t)col * cs;
    dst[0] = s.x;
    dst[ldo] = s.y;
    dst[2 * (size_t)ldo] = s.z;
    dst[3 * (size_t)ldo] = s.w;
  }
}

// operand of a dense layer's weight gradient: columns [col0, col0 + 4 * k4max) of row r + shift * 2^lg of a [M][512]
// tensor when frame (r >> lg) % F + shift lies in the sequence, else zeros; rows beyond M are zeros.
// PRE: the rows hold pre-activations, PReLU with *slope on load (the forward's own operation).
template <bool PRE>
struct ALoadTapCols {
  const float* A;
  const float* slope;
  int M, F, lg, shift, col0;
  DEV float4 load4(int tile, int row, int k4) const {
    const int r = tile * 32 + row;
    if (r >= M) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int f = (r >> lg) % F + shift;
    if (f < 0 || f >= F) return make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = *reinterpret_cast<const float4*>(A + (int64_t)(r + shift * (1 << lg)) * CT_N + col0 + 4 * k4);
    if constexpr (PRE) {
      const float a = *slope;
      v = make_float4(prelu(v.x, a), prelu(v.y, a), prelu(v.z, a), prelu(v.w, a));
    }
    return v;
  }
};

// ------------------------------------------------------------------------------------------------
// audio-visual head, backward
// ------------------------------------------------------------------------------------------------
// first frame f of [0, F) whose i0 is >= t, F if there is none: video_src's i0 does not decrease with f
DEV int video_first_frame(int t, int F, int Tv) {
  int lo = 0, hi = F;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (video_src(mid, F, Tv).i0 >= t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// LayerNorm(512) and interpolation backward.  Workgroup (t, b): the frames with i0 in {t - 1, t} are the ones that read
// video row t (i1 = min(i0 + 1, Tv - 1)), one contiguous range.  Wave w takes frames f_lo + w, f_lo + w + 4, ... in
// ascending order (lane: channels 4 lane .. +3 and 256 + 4 lane .. +3, as dctasnet_video_frames_kernel, whose operations
// give u, mu, rstd again); the four waves are then summed in wave order.  With dy = dfused[b F + f], g = dy gamma,
// xhat = (u - mu) rstd:  du = rstd (g - mean(g) - xhat mean(g xhat)),  dvcat[b Tv + t] = sum_f ((1 - lam)[i0 = t] +
// lam [i1 = t]) du,  vslab[b Tv + t] = (sum dy xhat | sum dy) over the frames with i0 = t.  An empty range writes zeros.
__global__ __launch_bounds__(256) void davtrain_video_ln_bwd_kernel(const float* __restrict__ dfused, const float* __restrict__ vcat,
                                                                    const float* __restrict__ g, int F, int Tv,
                                                                    float* __restrict__ dvcat, float* __restrict__ vslab) {
  __shared__ __attribute__((aligned(16))) float red[4][3][CT_N];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int t = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int f_lo = video_first_frame(t - 1, F, Tv), f_hi = video_first_frame(t + 1, F, Tv);
  float4 ga[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) ga[h] = *reinterpret_cast<const float4*>(g + h * 256 + 4 * lane);
  const float gam[8] = {ga[0].x, ga[0].y, ga[0].z, ga[0].w, ga[1].x, ga[1].y, ga[1].z, ga[1].w};
  float acc[8], sg[8], sb[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = sg[i] = sb[i] = 0.f;
  for (int f = f_lo + wave; f < f_hi; f += 4) {              // wave-uniform
    const VideoSrc vs = video_src(f, F, Tv);
    const int i0 = vs.i0, i1 = vs.i1;
    const float lam = vs.lam;
    float u[8], dy[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ch = h * 256 + 4 * lane;
      const float4 a = *reinterpret_cast<const float4*>(vcat + (b * Tv + i0) * CT_N + ch);
      const float4 c = *reinterpret_cast<const float4*>(vcat + (b * Tv + i1) * CT_N + ch);
      const float4 d = *reinterpret_cast<const float4*>(dfused + (b * F + f) * CT_N + ch);
      u[4 * h + 0] = a.x * (1.f - lam) + c.x * lam;
      u[4 * h + 1] = a.y * (1.f - lam) + c.y * lam;
      u[4 * h + 2] = a.z * (1.f - lam) + c.z * lam;
      u[4 * h + 3] = a.w * (1.f - lam) + c.w * lam;
      dy[4 * h + 0] = d.x; dy[4 * h + 1] = d.y; dy[4 * h + 2] = d.z; dy[4 * h + 3] = d.w;
    }
    const float mu = wave_sum(((u[0] + u[1]) + (u[2] + u[3])) + ((u[4] + u[5]) + (u[6] + u[7]))) * (1.0f / CT_N);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      u[i] -= mu;
      q += u[i] * u[i];
    }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / CT_N) + 1e-5f);
    float gg[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      u[i] *= rstd;                                          // xhat
      gg[i] = dy[i] * gam[i];
      s1 += gg[i];
      s2 = fmaf(gg[i], u[i], s2);
    }
    const float m1 = wave_sum(s1) * (1.0f / CT_N), m2 = wave_sum(s2) * (1.0f / CT_N);
    const float w0 = i0 == t ? 1.f - lam : 0.f, w1 = i1 == t ? lam : 0.f;
    const bool own = i0 == t;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float du = rstd * (gg[i] - m1 - u[i] * m2);
      acc[i] = fmaf(w1, du, fmaf(w0, du, acc[i]));
      if (own) {
        sg[i] = fmaf(dy[i], u[i], sg[i]);
        sb[i] += dy[i];
      }
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int ch = h * 256 + 4 * lane;
    *reinterpret_cast<float4*>(&red[wave][0][ch]) = make_float4(acc[4 * h], acc[4 * h + 1], acc[4 * h + 2], acc[4 * h + 3]);
    *reinterpret_cast<float4*>(&red[wave][1][ch]) = make_float4(sg[4 * h], sg[4 * h + 1], sg[4 * h + 2], sg[4 * h + 3]);
    *reinterpret_cast<float4*>(&red[wave][2][ch]) = make_float4(sb[4 * h], sb[4 * h + 1], sb[4 * h + 2], sb[4 * h + 3]);
  }
  __syncthreads();
  const int64_t row = b * Tv + t;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = tid + 256 * h;
    float s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = ((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c];
    dvcat[row * CT_N + c] = s[0];
    vslab[row * 2 * CT_N + c] = s[1];
    vslab[row * 2 * CT_N + CT_N + c] = s[2];
  }
}

// Linear(512 -> 256) backward, shared by the two speakers: dW[j][k] = sum_{s, b, t} dvcat[b Tv + t][256 s + j] e_s[b][k][t],
// d b[j] = sum_{s, b, t} dvcat[b Tv + t][256 s + j].  Workgroup (x, y): columns k0 = 32 x .. +31 of dW over the row chunks
// (b, 64 frames) y, y + gridDim.y, ... in that order; thread j owns row j.  Both speakers' embedding tile is staged in LDS
// with t fastest on the global side (coalesced along the embedding's time axis, as dctasnet_video_linear_kernel).
// Partials: slab[y][256][512] and, from the x = 0 workgroups, bslab[y][256].
__global__ __launch_bounds__(256) void davtrain_video_linear_bwd_kernel(const float* __restrict__ e1, const float* __restrict__ e2,
                                                                        const float* __restrict__ dvcat, int B, int Tv, int nchunk,
                                                                        float* __restrict__ slab, float* __restrict__ bslab) {
  __shared__ __attribute__((aligned(16))) float es[2][DAV_TT][DAV_LD];
  const int j = threadIdx.x, k0 = blockIdx.x * DAV_KT;
  float acc[DAV_KT];
#pragma unroll
  for (int i = 0; i < DAV_KT; ++i) acc[i] = 0.f;
  float bs = 0.f;
  for (int rc = blockIdx.y; rc < B * nchunk; rc += gridDim.y) {
    const int64_t b = rc / nchunk;
    const int t0 = (rc % nchunk) * DAV_TT;
    __syncthreads();
    for (int i = j; i < 2 * DAV_KT * DAV_TT; i += 256) {
      const int tt = i % DAV_TT, k = (i / DAV_TT) % DAV_KT, s = i / (DAV_TT * DAV_KT);
      const float* e = s ? e2 : e1;
      es[s][tt][k] = t0 + tt < Tv ? e[(b * CT_N + k0 + k) * Tv + t0 + tt] : 0.f;
    }
    __syncthreads();
    const int nt = Tv - t0 < DAV_TT ? Tv - t0 : DAV_TT;
    for (int tt = 0; tt < nt; ++tt) {
      const float* d = dvcat + (b * Tv + t0 + tt) * CT_N;
      const float d0 = d[j], d1 = d[DC_HV + j];
      bs += d0 + d1;
#pragma unroll
      for (int k4 = 0; k4 < DAV_KT / 4; ++k4) {
        const float4 x0 = *reinterpret_cast<const float4*>(&es[0][tt][4 * k4]);
        const float4 x1 = *reinterpret_cast<const float4*>(&es[1][tt][4 * k4]);
        acc[4 * k4 + 0] = fmaf(d1, x1.x, fmaf(d0, x0.x, acc[4 * k4 + 0]));
        acc[4 * k4 + 1] = fmaf(d1, x1.y, fmaf(d0, x0.y, acc[4 * k4 + 1]));
        acc[4 * k4 + 2] = fmaf(d1, x1.z, fmaf(d0, x0.z, acc[4 * k4 + 2]));
        acc[4 * k4 + 3] = fmaf(d1, x1.w, fmaf(d0, x0.w, acc[4 * k4 + 3]));
      }
    }
  }
  float* out = slab + ((size_t)blockIdx.y * DC_HV + j) * CT_N + k0;
#pragma unroll
  for (int k4 = 0; k4 < DAV_KT / 4; ++k4)
    *reinterpret_cast<float4*>(out + 4 * k4) = make_float4(acc[4 * k4], acc[4 * k4 + 1], acc[4 * k4 + 2], acc[4 * k4 + 3]);
  if (blockIdx.x == 0) bslab[(size_t)blockIdx.y * DC_HV + j] = bs;
}

struct Plan : TrainPlanBase {
  size_t off_wpk, off_c0, off_ez, off_dz, off_ga, off_gb;
  size_t off_dvcat, off_vslab, off_vcat;      // audio-visual only (empty otherwise)
};

}  // namespace

static_assert(DCTTRAIN_TAPE_V1 == SEP_TAPE_V1 && DCTTRAIN_TAPE_U == SEP_TAPE_U && DCTTRAIN_TAPE_SKIP == SEP_TAPE_SKIP,
              "sep_tape_offset takes the header's tape kinds");

static_assert(DAVTRAIN_TAPE_V1 == SEP_TAPE_V1 && DAVTRAIN_TAPE_U == SEP_TAPE_U && DAVTRAIN_TAPE_SKIP == SEP_TAPE_SKIP &&
                  DAVTRAIN_TAPE_ENC_Z == DCTTRAIN_TAPE_ENC_Z && DAVTRAIN_TAPE_DEC_Z == DCTTRAIN_TAPE_DEC_Z,
              "one tape_offset body serves both headers");

namespace {
// what the two handles share: the audio-visual one takes the `av` branches of the plan, the forward and the backward
struct DctCtx : CtTrainHandle {
  const bool av;
  DctCtx(const char* prefix_, bool av_) : CtTrainHandle(prefix_, DCT_UNUSED), av(av_) {}
};
}  // namespace

struct dcttrain_ctx : DctCtx {
  dcttrain_ctx() : DctCtx("dcttrain", false) {}
};

struct davtrain_ctx : DctCtx {
  davtrain_ctx() : DctCtx("davtrain", true) {}
};

namespace {

// Tv: video frames (audio-visual handle; the audio-only entry points pass 0)
int make_plan(CtHandle* h, int B, int64_t T, int Tv, Plan& p) {
  const bool av = static_cast<DctCtx*>(h)->av;
  CtHandle* c = h;
  // the decoder runs on 2*B*F rows of 512 (32-bit row indexing in the tap-shifted loaders)
  if (int rc = plan_train_head(c, B, T, "2*B*F*512", p)) return rc;
  if (av && Tv < 1) return c->fail(CTASNET_ERR_INVALID, "Tv must be >= 1 (got %d)", Tv);
  if (av && (int64_t)B * Tv * CT_N > (int64_t)INT32_MAX)
    return c->fail(CTASNET_ERR_INVALID, "B*Tv*512 = %lld exceeds 32-bit indexing (B=%d, Tv=%d)", (long long)B * Tv * CT_N, B, Tv);
  ByteCursor cur;
  const size_t M = (size_t)p.M;
  plan_separator_train(p, cur, B, M, (size_t)DCT_G_W * DCT_WN * DCT_WK);
  p.off_wpk = cur.take((size_t)DC_LAYERS * 3 * DC_TAP_FLOATS * 4);   // forward pack, then the backward's
  p.off_c0 = cur.take(M * CT_N * 4);                                  // tape: first conv output
  p.off_ez = cur.take(4 * M * CT_N * 4);                              // tape: encoder pre-activations
  p.off_dz = cur.take(4 * 2 * M * CT_N * 4);                          // tape: decoder pre-activations
  p.off_ga = cur.take(2 * M * CT_N * 4);                              // backward ping-pong
  p.off_gb = cur.take(2 * M * CT_N * 4);
  const size_t rows_v = av ? (size_t)B * Tv : 0;
  p.off_dvcat = cur.take(rows_v * CT_N * 4);                         // d vcat
  p.off_vslab = cur.take(rows_v * 2 * CT_N * 4);                     // per-(b, t) partials of d video_ln.weight | bias
  p.off_vcat = cur.take(rows_v * CT_N * 4);                          // tape: compressed embeddings; the workspace ends with it
  p.total = cur.o;
  return DCTTRAIN_OK;
}

void pack_sources(const std::vector<const float*>& W, PackSrc& ps) {
  for (int l = 0; l < 4; ++l) {
    ps.w[l] = W[2 + 3 * l];                   // encoder.sequential.{1,3,5,7}.weight
    ps.w[4 + l] = W[DC_DEC0 + 3 * l];         // decoder.sequential.{0,2,4,6}.weight
  }
}

// one tap's 128-column slice of a dense weight gradient: partial tiles of wgrad_kernel (static schedule), then the sum
// into out[row * 1536 + col * 3]
template <class YL, class XL>
int launch_dense_wgrad(DctCtx* c, hipStream_t st, int64_t rows, const YL& yl, const XL& xl, float* slab, float* out) {
  auto kern = wgrad_kernel<DCT_WN, DCT_WK, YL, XL, false>;
  const size_t lds = WgradShape<DCT_WN, DCT_WK>::lds_bytes();
  static PerDeviceOnce once;
  if (int rc = ensure_lds(c, once, kern, lds, "dcttrain dense wgrad")) return rc;
  const int ntiles = (int)((rows + 31) / 32);
  const int g = std::min(ntiles, DCT_G_W);
  hipLaunchKernelGGL(kern, dim3(g), dim3(256), lds, st, ntiles, (unsigned*)nullptr, yl, xl, slab, (float*)nullptr);
  HANDLE_LAUNCH_CHECK(c, "dcttrain dense wgrad");
  constexpr int RB = DCT_WN / 128, CB = DCT_WK / 32;
  hipLaunchKernelGGL((dcttrain_reduce_frag_kernel<RB, CB>), dim3(RB * CB * 32), dim3(256), 0, st, slab, g,
                     (int64_t)DCT_WN * DCT_WK, out, 3 * CT_N, 3);
  HANDLE_LAUNCH_CHECK(c, "dcttrain dense wgrad reduce");
  return DCTTRAIN_OK;
}

struct DenseBwd {
  bool transposed;      // ConvTranspose1d (decoder) or Conv1d (encoder)
  int dil, lg;
  int64_t rows;
  int F;
  float* dy;            // [rows][512] gradient of the layer's output; becomes dz in place
  const float* z;       // tape: pre-activation
  const float* x;       // the layer's input rows: pre-activations of the layer before when xslope is not null
  const float* xslope;
  const float* slope;
  const float* wpk;     // this layer's three taps, packed in the other orientation
  float* dx;            // [rows][512] out
  float* gw;
  float* gb;
  float* ga;
};

template <bool PRE>
int dense_wgrads(DctCtx* c, hipStream_t st, const DenseBwd& d, float* slab) {
  const int rows = (int)d.rows;
  for (int k = 0; k < 3; ++k) {
    const int shift = d.transposed ? (1 - k) * d.dil : (k - 1) * d.dil;
    for (int q = 0; q < CT_N / DCT_WK; ++q) {
      float* out = d.gw + (size_t)DCT_WK * q * 3 + k;
      int rc;
      if (d.transposed)     // weight (in, out, k): rows of dW are input channels
        rc = launch_dense_wgrad(c, st, d.rows, ALoadTapCols<PRE>{d.x, d.xslope, rows, d.F, d.lg, shift, 0},
                                ALoadTapCols<false>{d.dy, nullptr, rows, d.F, d.lg, 0, DCT_WK * q}, slab, out);
      else                  // weight (out, in, k): rows of dW are output channels
        rc = launch_dense_wgrad(c, st, d.rows, ALoadTapCols<false>{d.dy, nullptr, rows, d.F, d.lg, 0, 0},
                                ALoadTapCols<PRE>{d.x, d.xslope, rows, d.F, d.lg, shift, DCT_WK * q}, slab, out);
      if (rc) return rc;
    }
  }
  return DCTTRAIN_OK;
}

// backward of one dense k = 3 layer + PReLU
int dense_backward(DctCtx* c, hipStream_t st, const DenseBwd& d, float* slab, float* cslab, float* aslab) {
  // PReLU: dz = dy (z > 0 ? 1 : a) in place, d a = sum dy z over z <= 0
  hipLaunchKernelGGL(cttrain_prelu_bwd_kernel, dim3(CTT_G_ROW), dim3(256), 0, st, d.dy, d.z, d.slope, d.rows * CT_N, aslab);
  HANDLE_LAUNCH_CHECK(c, "dcttrain dense prelu backward");
  if (int rc = launch_reduce(c, st, aslab, CTT_G_ROW, 1, 1, 1, d.ga, 1)) return rc;
  if (int rc = launch_colsum<CT_N>(c, st, d.dy, d.rows, CT_N, 0, cslab, d.gb)) return rc;
  if (int rc = d.xslope ? dense_wgrads<true>(c, st, d, slab) : dense_wgrads<false>(c, st, d, slab)) return rc;
  // data gradient: dx[r] = sum_k V_k dz[r - s_k], zero where frame(r) - s_k leaves the sequence
  for (int k = 0; k < 3; ++k) {
    const int shift = d.transposed ? (1 - k) * d.dil : (k - 1) * d.dil;
    if (int rc = launch_gemm<CT_N>(c, st, "dcttrain dense dgrad", d.wpk + k * DC_TAP_FLOATS, nullptr, d.rows, CT_N / 128,
                                   ALoadTapShiftT<false>{d.dy, nullptr, (int)d.rows, d.F, d.lg, -shift},
                                   EpiStoreAdd{d.dx, d.rows, CT_N, k > 0}, 0))
      return rc;
  }
  return DCTTRAIN_OK;
}

int64_t dct_tape_offset(DctCtx* h, int B, int64_t T, int Tv, int which, int block) {
  if (!h) return -1;
  Plan p;
  if (make_plan(h, B, T, Tv, p)) return -1;
  if (h->av && which == DAVTRAIN_TAPE_VCAT) return (int64_t)p.off_vcat;
  const size_t M = (size_t)p.M;
  if (which == DCTTRAIN_TAPE_ENC_Z || which == DCTTRAIN_TAPE_DEC_Z) {
    if (block < 0 || block >= 4) {
      h->fail(DCTTRAIN_ERR_INVALID, "dense layer %d out of range", block);
      return -1;
    }
    return which == DCTTRAIN_TAPE_ENC_Z ? (int64_t)(p.off_ez + (size_t)block * M * CT_N * 4)
                                        : (int64_t)(p.off_dz + (size_t)block * 2 * M * CT_N * 4);
  }
  return sep_tape_offset(h, p, which, block);
}

// the audio-visual handle needs both embeddings (Tv is checked by the plan)
int check_embeddings(DctCtx* c, const float* e1, const float* e2) {
  if (c && c->av && (!e1 || !e2))
    return c->fail(CTASNET_ERR_INVALID, "the audio-visual model needs both speaker embeddings (e1 / e2 must not be NULL)");
  return CTASNET_OK;
}

// *_train_forward of both handles; e1, e2, Tv: the audio-visual one's
int dct_train_forward(DctCtx* c, const float* mix, const float* e1, const float* e2, int B, int64_t T, int Tv, float* s1_pred,
                      float* s2_pred, void* ws, size_t ws_bytes, void* stream) {
  Plan p;
  WsPtr at;
  if (int rc = check_embeddings(c, e1, e2)) return rc;
  auto plan = [Tv](CtHandle* h, int b, int64_t t, Plan& q) { return make_plan(h, b, t, Tv, q); };
  if (int rc = train_prologue(c, plan, false, mix, s1_pred, s2_pred, B, T, ws, ws_bytes, p, at)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  float* wpk = at.fp(p.off_wpk);
  float* enc = at.fp(p.off_enc);
  float* c0 = at.fp(p.off_c0);
  float* ym = at.fp(p.off_ym);
  float* ydec = at.fp(p.off_dv);          // the last decoder activation [2M][512]: scratch until the backward's head kernel
  float* taps = at.fp(p.off_taps);
  const SepBuffers sb = sep_tape_buffers(p, ws);

  // weights of the eight dense convs -> fragment order, this forward's copy
  PackSrc ps;
  pack_sources(W, ps);
  ps.tmask = 0xF0u;
  hipLaunchKernelGGL(dctasnet_pack_kernel, dim3((unsigned)(DC_TAP_FLOATS / 4 / 256), DC_LAYERS), dim3(256), 0, st, ps, wpk);
  HANDLE_LAUNCH_CHECK(c, "dcttrain weight pack");

  // video rows (deepavconvtasnet.py:140-151), the launches of dctasnet_forward: vcat stays on the tape; vid waits in the
  // scratch that holds the last decoder activation later on
  float* vid = nullptr;
  if (c->av) {
    float* vcat = at.fp(p.off_vcat);
    hipLaunchKernelGGL(dctasnet_video_linear_kernel, dim3((unsigned)((Tv + DC_VT - 1) / DC_VT), B), dim3(256), 0, st, e1, e2,
                       W[DC_AV0], W[DC_AV0 + 1], Tv, vcat);
    HANDLE_LAUNCH_CHECK(c, "davtrain video linear");
    vid = ydec;
    hipLaunchKernelGGL(dctasnet_video_frames_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, vcat, W[DC_AV0 + 2],
                       W[DC_AV0 + 3], F, Tv, M, vid);
    HANDLE_LAUNCH_CHECK(c, "davtrain video frames");
  }

  // deep encoder (deepconvtasnet.py:7-26): first conv -> c0; layer l reads c0 / PReLU(z_{l-1}) and writes z_l; the last one
  // also writes enc = PReLU(z_3) (+ the video rows: the fused tensor) and the GlobalNorm partials of enc
  const unsigned row_wgs = (unsigned)((M + CT_ROWS_PER_WG - 1) / CT_ROWS_PER_WG);
  hipLaunchKernelGGL(ctasnet_encoder_kernel<true>, dim3(row_wgs), dim3(256), 0, st, mix, T, F, M, W[0], W[1], c0, nullptr);
  HANDLE_LAUNCH_CHECK(c, "dcttrain encoder");
  for (int l = 0; l < 4; ++l) {
    float* z = at.fp(p.off_ez) + (size_t)l * M * CT_N;
    const float* x = l == 0 ? c0 : z - (size_t)M * CT_N;
    if (int rc = launch_dense<true>(c, st, wpk + (int64_t)l * 3 * DC_TAP_FLOATS, false, 1 << l, x, l == 0 ? nullptr : W[1 + 3 * l],
                                    z, l == 3 ? enc : nullptr, M, F, 0, W[3 + 3 * l], W[4 + 3 * l], l == 3 ? vid : nullptr,
                                    l == 3 ? sb.part : nullptr))
      return rc;
  }

  // Separator on its tape: masks times the encoder output -> ym [M][1024]
  if (int rc = launch_separator<true>(c, st, W.data() + DC_SEP0, enc, 4, 128.0f, B, F, M, sb)) return rc;

  // deep decoder (deepconvtasnet.py:96-120) on 2M rows (b, f, speaker), then the output head as taps + overlap-add
  for (int l = 0; l < 4; ++l) {
    float* z = at.fp(p.off_dz) + (size_t)l * 2 * M * CT_N;
    const float* x = l == 0 ? ym : z - (size_t)2 * M * CT_N;
    if (int rc = launch_dense<true>(c, st, wpk + (int64_t)(4 + l) * 3 * DC_TAP_FLOATS, true, 8 >> l, x,
                                    l == 0 ? nullptr : W[DC_DEC0 + 3 * l - 1], z, l == 3 ? ydec : nullptr, 2 * M, F, 1,
                                    W[DC_DEC0 + 1 + 3 * l], W[DC_DEC0 + 2 + 3 * l], nullptr, nullptr))
      return rc;
  }
  if (int rc = launch_taps(c, st, ydec, W[DC_DEC0 + 12], M, taps)) return rc;
  return launch_overlap_add<true>(c, st, taps, W[DC_DEC0 + 13], B, F, p.Lout, s1_pred, s2_pred);
}

// *_train_backward of both handles
int dct_train_backward(DctCtx* c, const float* mix, const float* e1, const float* e2, int B, int64_t T, int Tv, const float* d_s1,
                       const float* d_s2, void* ws, size_t ws_bytes, void* stream) {
  Plan p;
  WsPtr at;
  if (int rc = check_embeddings(c, e1, e2)) return rc;
  auto plan = [Tv](CtHandle* h, int b, int64_t t, Plan& q) { return make_plan(h, b, t, Tv, q); };
  if (int rc = train_prologue(c, plan, true, mix, d_s1, d_s2, B, T, ws, ws_bytes, p, at)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  const auto& G = c->g;
  float* wpk = at.fp(p.off_wpk);
  float* dtaps = at.fp(p.off_taps);
  float* denc = at.fp(p.off_denc);
  float* slab = at.fp(p.off_slab);
  float* cslab = at.fp(p.off_cslab);
  float* aslab = at.fp(p.off_aslab);
  float* ga = at.fp(p.off_ga);
  float* gb = at.fp(p.off_gb);
  int ns = 0;

  // the eight layers' weights for the data gradients, from the weights as they are now: the other orientation
  PackSrc ps;
  pack_sources(W, ps);
  ps.tmask = 0x0Fu;
  hipLaunchKernelGGL(dctasnet_pack_kernel, dim3((unsigned)(DC_TAP_FLOATS / 4 / 256), DC_LAYERS), dim3(256), 0, st, ps, wpk);
  HANDLE_LAUNCH_CHECK(c, "dcttrain backward weight pack");

  // ---- output head (decoder.sequential.8, ConvTranspose1d(512, 1, 32, 16) + bias, cropped): d taps, d bias, d W, d y_3
  {
    const int64_t n = M * 4 * CT_L;
    hipLaunchKernelGGL(cttrain_dtaps_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_s1, d_s2, F, M, p.Lout, dtaps);
    HANDLE_LAUNCH_CHECK(c, "dcttrain dtaps");
    hipLaunchKernelGGL(dcttrain_outsum_kernel, dim3(CTT_G_ROW), dim3(256), 0, st, d_s1, d_s2, (int64_t)B * p.Lout, aslab);
    HANDLE_LAUNCH_CHECK(c, "dcttrain output bias");
    if (int rc = launch_reduce(c, st, aslab, CTT_G_ROW, 1, 1, 1, G[DC_DEC0 + 13], 1)) return rc;
    const float* z3 = at.fp(p.off_dz) + (size_t)3 * 2 * M * CT_N;
    if (int rc = launch_wgrad<CT_N, 2 * CT_L>(c, st, 2 * M, ALoadDensePReLU{z3, W[DC_DEC0 + 11], 2 * M, CT_N, 32},
                                              ALoadDense{dtaps, 2 * M, 2 * CT_L, 32}, slab, &ns))
      return rc;
    if (int rc = launch_reduce(c, st, slab, ns, (int64_t)CT_N * 2 * CT_L, CT_N, 2 * CT_L, G[DC_DEC0 + 12], 2 * CT_L)) return rc;
    static PerDeviceOnce once;
    if (int rc = ensure_lds(c, once, cttrain_head_bwd_kernel<HEAD_DYM_OUT>, CTT_HEAD_LDS, "dcttrain head dgrad")) return rc;
    const unsigned g = (unsigned)std::min<int64_t>(M, 2048);
    hipLaunchKernelGGL(cttrain_head_bwd_kernel<HEAD_DYM_OUT>, dim3(g), dim3(256), CTT_HEAD_LDS, st, dtaps, W[DC_DEC0 + 12], nullptr,
                       nullptr, M, ga, nullptr);
    HANDLE_LAUNCH_CHECK(c, "dcttrain head dgrad");
  }

  // ---- deep decoder, layers 3..0 (d = 1, 2, 4, 8) on 2M rows: ga -> gb -> ga -> gb -> ga = d ym
  float* dy = ga;
  float* dx = gb;
  for (int l = 3; l >= 0; --l) {
    const float* z = at.fp(p.off_dz) + (size_t)l * 2 * M * CT_N;
    const DenseBwd d{true, 8 >> l, 1, 2 * M, F, dy, z, l == 0 ? at.fp(p.off_ym) : z - (size_t)2 * M * CT_N,
                     l == 0 ? nullptr : W[DC_DEC0 + 3 * l - 1], W[DC_DEC0 + 2 + 3 * l], wpk + (int64_t)(4 + l) * 3 * DC_TAP_FLOATS,
                     dx, G[DC_DEC0 + 3 * l], G[DC_DEC0 + 1 + 3 * l], G[DC_DEC0 + 2 + 3 * l]};
    if (int rc = dense_backward(c, st, d, slab, cslab, aslab)) return rc;
    std::swap(dy, dx);
  }

  // ---- Separator (convtasnet.py:55-83): mask head from d ym, 24 blocks, bottleneck, GlobalNorm -> d enc
  if (int rc = launch_separator_backward<HEAD_DYM>(c, st, W.data() + DC_SEP0, G.data() + DC_SEP0, dy, nullptr, B, F, M, p, ws))
    return rc;

  // ---- video head (deepavconvtasnet.py:140-153): d fused is also d vid; read here, before encoder layer 3's PReLU
  // backward overwrites denc in place
  if (c->av) {
    float* dvcat = at.fp(p.off_dvcat);
    float* vslab = at.fp(p.off_vslab);
    const int rows_v = B * Tv;
    hipLaunchKernelGGL(davtrain_video_ln_bwd_kernel, dim3(Tv, B), dim3(256), 0, st, denc, at.fp(p.off_vcat), W[DC_AV0 + 2], F, Tv,
                       dvcat, vslab);
    HANDLE_LAUNCH_CHECK(c, "davtrain video LayerNorm backward");
    if (int rc = launch_reduce(c, st, vslab, rows_v, 2 * CT_N, 1, CT_N, G[DC_AV0 + 2], CT_N)) return rc;
    if (int rc = launch_reduce(c, st, vslab + CT_N, rows_v, 2 * CT_N, 1, CT_N, G[DC_AV0 + 3], CT_N)) return rc;
    const int nchunk = (Tv + DAV_TT - 1) / DAV_TT;
    const int gr = (int)std::min<int64_t>((int64_t)B * nchunk, DAV_G_R);
    hipLaunchKernelGGL(davtrain_video_linear_bwd_kernel, dim3(CT_N / DAV_KT, gr), dim3(256), 0, st, e1, e2, dvcat, B, Tv, nchunk,
                       slab, cslab);
    HANDLE_LAUNCH_CHECK(c, "davtrain video linear backward");
    if (int rc = launch_reduce(c, st, slab, gr, (int64_t)DC_HV * CT_N, DC_HV, CT_N, G[DC_AV0], CT_N)) return rc;
    if (int rc = launch_reduce(c, st, cslab, gr, DC_HV, 1, DC_HV, G[DC_AV0 + 1], DC_HV)) return rc;
  }

  // ---- deep encoder, layers 3..0 (d = 8, 4, 2, 1) on M rows: denc -> ga -> gb -> ga -> gb = d c0
  dy = denc;
  dx = ga;
  for (int l = 3; l >= 0; --l) {
    const float* z = at.fp(p.off_ez) + (size_t)l * M * CT_N;
    const DenseBwd d{false, 1 << l, 0, M, F, dy, z, l == 0 ? at.fp(p.off_c0) : z - (size_t)M * CT_N,
                     l == 0 ? nullptr : W[1 + 3 * l], W[4 + 3 * l], wpk + (int64_t)l * 3 * DC_TAP_FLOATS, dx, G[2 + 3 * l],
                     G[3 + 3 * l], G[4 + 3 * l]};
    if (int rc = dense_backward(c, st, d, slab, cslab, aslab)) return rc;
    dy = dx;
    dx = dy == ga ? gb : ga;
  }

  // ---- first conv (encoder.sequential.0, Conv1d(1, 512, 32, 16) + bias): d W[n][k] = sum_rows d c0[row][n] xpad[16 f + k]
  if (int rc = launch_wgrad<CT_N, 2 * CT_L>(c, st, M, ALoadDense{dy, M, CT_N, 32}, ALoadPatches{mix, T, M, F}, slab, &ns))
    return rc;
  if (int rc = launch_reduce(c, st, slab, ns, (int64_t)CT_N * 2 * CT_L, CT_N, 2 * CT_L, G[0], 2 * CT_L)) return rc;
  return launch_colsum<CT_N>(c, st, dy, M, CT_N, 0, cslab, G[1]);
}

}  // namespace

extern "C" {

int dcttrain_abi_version(void) { return DCTTRAIN_ABI_VERSION; }

int dcttrain_create(dcttrain_handle* out, int av) {
  if (av != 0) {
    if (out) *out = nullptr;
    g_create_error = "the audio-visual training step (DeepAVConvTasNet) is not built: dcttrain_create takes av = 0";
    return DCTTRAIN_ERR_INVALID;
  }
  if (int rc = ct_create(out, "deep Conv-TasNet training step", g_create_error)) return rc;
  dcttrain_ctx* c = *out;
  add_deepconvtasnet_names(c, false);
  c->w.assign(c->names.size(), nullptr);
  c->g.assign(c->names.size(), nullptr);
  return DCTTRAIN_OK;
}

void dcttrain_destroy(dcttrain_handle h) { delete h; }

const char* dcttrain_last_error(dcttrain_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int dcttrain_num_weights(dcttrain_handle h) { return h ? (int)h->names.size() : 0; }

const char* dcttrain_weight_name(dcttrain_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t dcttrain_weight_numel(dcttrain_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int dcttrain_bind_weights(dcttrain_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n) : DCTTRAIN_ERR_INVALID;
}

int dcttrain_bind_grads(dcttrain_handle h, float* const* dev_ptrs, int n) {
  return h ? bind_grads(h, dev_ptrs, n) : DCTTRAIN_ERR_INVALID;
}

int64_t dcttrain_flat_offset(dcttrain_handle h, int slot) { return h ? flat_offset(h, slot) : -1; }

int64_t dcttrain_flat_numel(dcttrain_handle h) { return h ? flat_numel(h) : -1; }

int64_t dcttrain_frames(int64_t T) { return frames_of(T); }

int64_t dcttrain_out_len(int64_t T) { return out_len_of(T); }

size_t dcttrain_workspace_bytes(dcttrain_handle h, int B, int64_t T) {
  if (!h) return 0;
  Plan p;
  if (make_plan(h, B, T, 0, p)) return 0;
  return p.total;
}

int64_t dcttrain_tape_offset(dcttrain_handle h, int B, int64_t T, int which, int block) {
  return dct_tape_offset(h, B, T, 0, which, block);
}

int dcttrain_train_forward(dcttrain_handle h, const float* mix, int B, int64_t T, float* s1_pred, float* s2_pred, void* ws,
                           size_t ws_bytes, void* stream) {
  return dct_train_forward(h, mix, nullptr, nullptr, B, T, 0, s1_pred, s2_pred, ws, ws_bytes, stream);
}

int dcttrain_train_backward(dcttrain_handle h, const float* mix, int B, int64_t T, const float* d_s1, const float* d_s2, void* ws,
                            size_t ws_bytes, void* stream) {
  return dct_train_backward(h, mix, nullptr, nullptr, B, T, 0, d_s1, d_s2, ws, ws_bytes, stream);
}

size_t dcttrain_clip_scratch_bytes(dcttrain_handle) { return CLIP_PARTS * sizeof(double); }

int dcttrain_grad_clip(dcttrain_handle h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                       float* norm_out, void* stream) {
  return h ? train_grad_clip(h, flat_grad, n_flat, max_norm, scratch, scratch_bytes, norm_out, stream) : DCTTRAIN_ERR_INVALID;
}

// decoder.deconv.weight (no_grad_slot) takes no step and no decay: what torch.optim.AdamW does with .grad None
int dcttrain_adamw_step(dcttrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                        double beta1, double beta2, double eps, double weight_decay, int step, void* stream) {
  return h ? train_adamw_step(h, flat_grad, exp_avg, exp_avg_sq, n_flat, lr, beta1, beta2, eps, weight_decay, step, stream)
           : DCTTRAIN_ERR_INVALID;
}

double dcttrain_flops_per_mixture(dcttrain_handle, int64_t T) {
  // forward MACs (dctasnet_flops_per_mixture) x 3: the backward is one data-gradient and one weight-gradient product per
  // forward product
  return 3.0 * 2.0 * deepconvtasnet_macs() * (double)frames_of(T);
}

// ---- davtrain_*: the same bodies on the audio-visual handle (include/davctasnet_train.h)
int davtrain_abi_version(void) { return DAVTRAIN_ABI_VERSION; }

int davtrain_create(davtrain_handle* out) {
  if (int rc = ct_create(out, "deep audio-visual Conv-TasNet training step", g_create_error)) return rc;
  davtrain_ctx* c = *out;
  add_deepconvtasnet_names(c, true);
  c->w.assign(c->names.size(), nullptr);
  c->g.assign(c->names.size(), nullptr);
  return DAVTRAIN_OK;
}

void davtrain_destroy(davtrain_handle h) { delete h; }

const char* davtrain_last_error(davtrain_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int davtrain_num_weights(davtrain_handle h) { return h ? (int)h->names.size() : 0; }

const char* davtrain_weight_name(davtrain_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t davtrain_weight_numel(davtrain_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int davtrain_bind_weights(davtrain_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n) : DAVTRAIN_ERR_INVALID;
}

int davtrain_bind_grads(davtrain_handle h, float* const* dev_ptrs, int n) {
  return h ? bind_grads(h, dev_ptrs, n) : DAVTRAIN_ERR_INVALID;
}

int64_t davtrain_flat_offset(davtrain_handle h, int slot) { return h ? flat_offset(h, slot) : -1; }

int64_t davtrain_flat_numel(davtrain_handle h) { return h ? flat_numel(h) : -1; }

int64_t davtrain_frames(int64_t T) { return frames_of(T); }

int64_t davtrain_out_len(int64_t T) { return out_len_of(T); }

size_t davtrain_workspace_bytes(davtrain_handle h, int B, int64_t T, int Tv) {
  if (!h) return 0;
  Plan p;
  if (make_plan(h, B, T, Tv, p)) return 0;
  return p.total;
}

int64_t davtrain_tape_offset(davtrain_handle h, int B, int64_t T, int Tv, int which, int block) {
  return dct_tape_offset(h, B, T, Tv, which, block);
}

int davtrain_train_forward(davtrain_handle h, const float* mix, const float* e1, const float* e2, int B, int64_t T, int Tv,
                           float* s1_pred, float* s2_pred, void* ws, size_t ws_bytes, void* stream) {
  return dct_train_forward(h, mix, e1, e2, B, T, Tv, s1_pred, s2_pred, ws, ws_bytes, stream);
}

int davtrain_train_backward(davtrain_handle h, const float* mix, const float* e1, const float* e2, int B, int64_t T, int Tv,
                            const float* d_s1, const float* d_s2, void* ws, size_t ws_bytes, void* stream) {
  return dct_train_backward(h, mix, e1, e2, B, T, Tv, d_s1, d_s2, ws, ws_bytes, stream);
}

size_t davtrain_clip_scratch_bytes(davtrain_handle) { return CLIP_PARTS * sizeof(double); }

int davtrain_grad_clip(davtrain_handle h, float* flat_grad, int64_t n_flat, float max_norm, void* scratch, size_t scratch_bytes,
                       float* norm_out, void* stream) {
  return h ? train_grad_clip(h, flat_grad, n_flat, max_norm, scratch, scratch_bytes, norm_out, stream) : DAVTRAIN_ERR_INVALID;
}

int davtrain_adamw_step(davtrain_handle h, const float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat, double lr,
                        double beta1, double beta2, double eps, double weight_decay, int step, void* stream) {
  return h ? train_adamw_step(h, flat_grad, exp_avg, exp_avg_sq, n_flat, lr, beta1, beta2, eps, weight_decay, step, stream)
           : DAVTRAIN_ERR_INVALID;
}

// the video head is left out of the cost model, as in dctasnet_flops_per_mixture
double davtrain_flops_per_mixture(davtrain_handle, int64_t T) { return 3.0 * 2.0 * deepconvtasnet_macs() * (double)frames_of(T); }

}  // extern "C"
