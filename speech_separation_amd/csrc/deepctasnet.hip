// deepctasnet.hip -- DeepConvTasNet / DeepAVConvTasNet inference forward (src/model/deepconvtasnet.py,
// src/model/deepavconvtasnet.py) for gfx950: handle and the extern "C" boundary declared in include/dctasnet.h; the kernels
// are in deepctasnet_kernels.h, shared with the training step.
//
// The Separator is Conv-TasNet's, unchanged (ctasnet_kernels.h).  New here are the deep encoder / decoder -- eight dense
// dilated k = 3 convs 512 -> 512, about 65 % of the FLOPs -- and the audio-visual head.
//
// Dense k = 3 conv: out[f] = bias + sum_k W_k x[f + s_k], with s_k = (k - 1) d for the Conv1d and s_k = (1 - k) d, W_k =
// weight[:, :, k]^T for the stride-1 ConvTranspose1d (weight stored (in, out, k)).  It runs as three accumulating passes of
// the weights-stationary engine, one per tap, each a KIN = 512 contraction: the A loader reads row f + s_k of the same
// sequence (zero outside [0, F)), the epilogue stores bias + v (tap 0), adds v (tap 1), adds v and applies the PReLU (tap 2).
// A K = 1536 slice does not fit the engine (its 128-column x 512 slice already holds 256 registers per lane).
// The weights are repacked in every forward, into the workspace, in the engine's fragment order: one launch for the three
// taps of all eight layers.  A copy made at bind time would go stale when load_state_dict copies into the same storages.
//
// Rows: the encoder runs on M = B*F rows [b*F + f][512].  The decoder runs on 2*B*F rows in (b, f, speaker) order: the
// masked separator output ym[b*F + f][speaker*512 + n] read as rows of 512, so a frame step is two rows.  This keeps
// Conv-TasNet's mask epilogue, decoder taps and overlap-add layout unchanged.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/dctasnet.h"
#include "deepctasnet_kernels.h"

static_assert(DCTASNET_OK == CTASNET_OK && DCTASNET_ERR_INVALID == CTASNET_ERR_INVALID &&
                  DCTASNET_ERR_WORKSPACE == CTASNET_ERR_WORKSPACE && DCTASNET_ERR_WEIGHTS == CTASNET_ERR_WEIGHTS &&
                  DCTASNET_ERR_HIP == CTASNET_ERR_HIP,
              "the shared Conv-TasNet code returns CTASNET_* codes");

namespace {
thread_local std::string g_create_error;

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct Plan {
  int64_t F, M, Lout;
  size_t off_wpk, off_enc, off_x, off_skip, off_c, off_dec, off_taps, off_part, off_stats, off_vcat, total;
};

}  // namespace

struct dctasnet_ctx : CtHandle {
  bool av = false;
};

namespace {
int make_plan(dctasnet_ctx* c, int B, int64_t T, int Tv, Plan& p) {
  if (int rc = check_batch(c, B, T)) return rc;
  if (c->av && Tv < 1) return c->fail(DCTASNET_ERR_INVALID, "Tv must be >= 1 for the audio-visual model (got %d)", Tv);
  p.F = frames_of(T);
  p.M = (int64_t)B * p.F;
  // the decoder runs on 2*B*F rows of 512
  if (2 * p.M * CT_N > (int64_t)INT32_MAX)
    return c->fail(DCTASNET_ERR_INVALID, "2*B*F*512 = %lld exceeds 32-bit indexing (B=%d, T=%lld)", (long long)(2 * p.M * CT_N),
                   B, (long long)T);
  if (c->av && (int64_t)B * Tv * CT_N > (int64_t)INT32_MAX)
    return c->fail(DCTASNET_ERR_INVALID, "B*Tv*512 = %lld exceeds 32-bit indexing (B=%d, Tv=%d)", (long long)B * Tv * CT_N, B, Tv);
  p.Lout = CT_L * (T / CT_L);
  ByteCursor cur;
  const size_t M = (size_t)p.M;
  p.off_wpk = cur.take((size_t)DC_LAYERS * 3 * DC_TAP_FLOATS * 4);
  p.off_enc = cur.take(M * CT_N * 4);       // encoder output (AV: fused with the video rows); the mask epilogue reads it
  p.off_x = cur.take(M * CT_B * 4);
  p.off_skip = cur.take(M * CT_B * 4);
  p.off_c = cur.take(M * 2 * CT_N * 4);     // separator c | w, then ym [M][1024]; encoder ping-pong buffer before that
  p.off_dec = cur.take(M * 2 * CT_N * 4);   // decoder ping-pong buffer; the video rows [M][512] before that
  p.off_taps = cur.take(M * 4 * CT_L * 4);
  p.off_part = cur.take(M * 4 * sizeof(float2));
  p.off_stats = cur.take((size_t)B * 2 * sizeof(float2));
  p.off_vcat = cur.take(c->av ? (size_t)B * Tv * CT_N * 4 : 0);
  p.total = cur.o;
  return DCTASNET_OK;
}
}  // namespace

extern "C" {

int dctasnet_abi_version(void) { return DCTASNET_ABI_VERSION; }

int dctasnet_create(dctasnet_handle* out, int av) {
  if (int rc = ct_create(out, "deep Conv-TasNet", g_create_error)) return rc;
  dctasnet_ctx* c = *out;
  c->av = av != 0;  add_deepconvtasnet_names(c, c->av);
  c->w.assign(c->names.size(), nullptr);
  return DCTASNET_OK;
}

void dctasnet_destroy(dctasnet_handle h) { delete h; }

const char* dctasnet_last_error(dctasnet_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int dctasnet_num_weights(dctasnet_handle h) { return h ? (int)h->names.size() : 0; }

const char* dctasnet_weight_name(dctasnet_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t dctasnet_weight_numel(dctasnet_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int dctasnet_bind_weights(dctasnet_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n) : DCTASNET_ERR_INVALID;
}

int64_t dctasnet_frames(int64_t T) { return frames_of(T); }

int64_t dctasnet_out_len(int64_t T) { return out_len_of(T); }

size_t dctasnet_workspace_bytes(dctasnet_handle h, int B, int64_t T, int Tv) {
  if (!h) return 0;
  Plan p;
  if (make_plan(h, B, T, Tv, p)) return 0;
  return p.total;
}

int dctasnet_forward(dctasnet_handle h, const float* mix, const float* e1, const float* e2, int B, int64_t T, int Tv,
                     float* s1_pred, float* s2_pred, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return DCTASNET_ERR_INVALID;
  dctasnet_ctx* c = h;
  if (!c->bound) return c->fail(DCTASNET_ERR_WEIGHTS, "weights not bound (dctasnet_bind_weights)");
  if (!mix || !s1_pred || !s2_pred) return c->fail(DCTASNET_ERR_INVALID, "mix / s1_pred / s2_pred must not be NULL");
  if (c->av && (!e1 || !e2)) return c->fail(DCTASNET_ERR_INVALID, "the audio-visual model needs both speaker embeddings");
  if (!c->av && (e1 || e2)) return c->fail(DCTASNET_ERR_INVALID, "the audio-only model takes no embeddings (pass NULL)");
  Plan p;
  if (int rc = make_plan(c, B, T, Tv, p)) return rc;
  if (int rc = check_workspace(c, p.total, ws, ws_bytes)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  float* wpk = reinterpret_cast<float*>(base + p.off_wpk);
  float* enc = reinterpret_cast<float*>(base + p.off_enc);
  float* cbuf = reinterpret_cast<float*>(base + p.off_c);
  float* dec = reinterpret_cast<float*>(base + p.off_dec);
  float* taps = reinterpret_cast<float*>(base + p.off_taps);
  float2* part = reinterpret_cast<float2*>(base + p.off_part);
  float2* stats1 = reinterpret_cast<float2*>(base + p.off_stats);
  const SepBuffers sb{reinterpret_cast<float*>(base + p.off_x), reinterpret_cast<float*>(base + p.off_skip), cbuf,
                      cbuf + p.M * CT_N, part, stats1, stats1, stats1 + B, cbuf, nullptr};
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;

  // weights of the eight dense convs -> fragment order, this forward's copy
  PackSrc ps;
  ps.tmask = 0xF0u;
  for (int l = 0; l < 4; ++l) {
    ps.w[l] = W[2 + 3 * l];                   // encoder.sequential.{1,3,5,7}.weight
    ps.w[4 + l] = W[DC_DEC0 + 3 * l];         // decoder.sequential.{0,2,4,6}.weight
  }
  hipLaunchKernelGGL(dctasnet_pack_kernel, dim3((unsigned)(DC_TAP_FLOATS / 4 / 256), DC_LAYERS), dim3(256), 0, st, ps, wpk);
  HANDLE_LAUNCH_CHECK(c, "dctasnet weight pack");

  // video rows (deepavconvtasnet.py:140-151), kept in the decoder's buffer until the encoder is done
  float* vid = nullptr;
  if (c->av) {
    float* vcat = reinterpret_cast<float*>(base + p.off_vcat);
    hipLaunchKernelGGL(dctasnet_video_linear_kernel, dim3((unsigned)((Tv + DC_VT - 1) / DC_VT), B), dim3(256), 0, st, e1, e2,
                       W[DC_AV0], W[DC_AV0 + 1], Tv, vcat);
    HANDLE_LAUNCH_CHECK(c, "dctasnet video linear");
    vid = dec;
    hipLaunchKernelGGL(dctasnet_video_frames_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, vcat, W[DC_AV0 + 2],
                       W[DC_AV0 + 3], F, Tv, M, vid);
    HANDLE_LAUNCH_CHECK(c, "dctasnet video frames");
  }

  // deep encoder (deepconvtasnet.py:7-26): Conv1d(1, 512, 32, 16) + bias, then 4 x [dense conv d, PReLU], d = 1, 2, 4, 8.
  // Ping-pong enc <-> c; the last conv lands in enc, adds the video rows and writes the GlobalNorm partials.
  const unsigned row_wgs = (unsigned)((M + CT_ROWS_PER_WG - 1) / CT_ROWS_PER_WG);
  hipLaunchKernelGGL(ctasnet_encoder_kernel<true>, dim3(row_wgs), dim3(256), 0, st, mix, T, F, M, W[0], W[1], enc, nullptr);
  HANDLE_LAUNCH_CHECK(c, "dctasnet encoder");
  for (int l = 0; l < 4; ++l) {
    const float* x = (l & 1) ? cbuf : enc;
    float* y = (l & 1) ? enc : cbuf;
    if (int rc = launch_dense<false>(c, st, wpk + (int64_t)l * 3 * DC_TAP_FLOATS, false, 1 << l, x, nullptr, y, nullptr, M, F, 0,
                                     W[3 + 3 * l], W[4 + 3 * l], l == 3 ? vid : nullptr, l == 3 ? part : nullptr))
      return rc;
  }

  // Separator: masks times the (fused) encoder output -> ym [M][1024] in c
  if (int rc = launch_separator<false>(c, st, W.data() + DC_SEP0, enc, 4, 128.0f, B, F, M, sb)) return rc;

  // deep decoder (deepconvtasnet.py:96-120) on 2M rows (b, f, speaker): 4 x [dense ConvTranspose d, PReLU], d = 8, 4, 2, 1,
  // ping-pong c <-> dec, ending in c; then ConvTranspose1d(512, 1, 32, 16) + bias as taps + overlap-add
  for (int l = 0; l < 4; ++l) {
    const float* x = (l & 1) ? dec : cbuf;
    float* y = (l & 1) ? cbuf : dec;
    if (int rc = launch_dense<false>(c, st, wpk + (int64_t)(4 + l) * 3 * DC_TAP_FLOATS, true, 8 >> l, x, nullptr, y, nullptr, 2 * M,
                                     F, 1, W[DC_DEC0 + 1 + 3 * l], W[DC_DEC0 + 2 + 3 * l], nullptr, nullptr))
      return rc;
  }
  if (int rc = launch_taps(c, st, cbuf, W[DC_DEC0 + 12], M, taps)) return rc;
  return launch_overlap_add<true>(c, st, taps, W[DC_DEC0 + 13], B, F, p.Lout, s1_pred, s2_pred);
}

double dctasnet_flops_per_mixture(dctasnet_handle, int64_t T) {
  return 2.0 * deepconvtasnet_macs() * (double)frames_of(T);
}

double dctasnet_min_bytes_per_mixture(dctasnet_handle h, int64_t T) {
  // floats per frame that the launches read + write once each (row partials and per-mixture statistics are ~1 % and left out)
  const double F = (double)frames_of(T);
  const double dense = 3.0 * CT_N + 5.0 * CT_N;              // per row: 3 taps' A rows; out written, then twice read + written
  const double enc = CT_N + 4.0 * dense + (h && h->av ? 2.0 * CT_N : 0.0);   // first conv; 4 dense; video rows out + in
  const double sep = (CT_N + CT_B)                           // bottleneck: enc in, x out
                     + CT_BLOCKS * ((CT_B + CT_H) + (CT_R * CT_H + CT_H) + (CT_H + 4.0 * CT_B))
                     + (CT_B + CT_N + 2 * CT_N);               // mask GEMM: skip, enc in; ym out
  const double dec = 2.0 * 4.0 * dense + (2 * CT_N + 4 * CT_L) + (4 * CT_L + 2 * CT_L);
  return 4.0 * F * (enc + sep + dec) + 4.0 * (double)T;
}

size_t dctasnet_weight_pack_bytes(dctasnet_handle) { return (size_t)2 * DC_LAYERS * 3 * DC_TAP_FLOATS * 4; }

}  // extern "C"
