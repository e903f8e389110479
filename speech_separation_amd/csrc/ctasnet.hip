// ctasnet.hip -- Conv-TasNet inference forward (src/model/convtasnet.py) for gfx950: handle and the extern "C" boundary
// declared in include/ctasnet.h.  The kernels, engine hooks and the separator's launch sequence live in ctasnet_kernels.h,
// the handle's scaffolding in ctasnet_handle.h (both shared with deepctasnet.hip and ctasnet_train.hip); the layout and the
// statistics scheme are described in the former.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/ctasnet.h"
#include "ctasnet_handle.h"

namespace {

thread_local std::string g_create_error;

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct Plan {
  int64_t F, M, Lout;
  size_t off_enc, off_x, off_skip, off_c, off_w, off_taps, off_part, off_stats, total;
};

}  // namespace

struct ctasnet_ctx : CtHandle {};

namespace {

int make_plan(ctasnet_ctx* c, int B, int64_t T, Plan& p) {
  if (int rc = check_batch(c, B, T)) return rc;
  p.F = frames_of(T);
  p.M = (int64_t)B * p.F;
  if (p.M * CT_H > (int64_t)INT32_MAX)
    return c->fail(CTASNET_ERR_INVALID, "B*F*512 = %lld exceeds 32-bit indexing (B=%d, T=%lld)", (long long)(p.M * CT_H), B,
                   (long long)T);
  p.Lout = CT_L * (T / CT_L);
  ByteCursor cur;
  const size_t M = (size_t)p.M;
  p.off_enc = cur.take(M * CT_N * 4);
  p.off_x = cur.take(M * CT_B * 4);
  p.off_skip = cur.take(M * CT_B * 4);
  p.off_c = cur.take(M * CT_H * 4);        // c and w are contiguous: the head's masked rows [M][1024] reuse both
  p.off_w = cur.take(M * CT_H * 4);
  p.off_taps = cur.take(M * 4 * CT_L * 4);
  p.off_part = cur.take(M * 4 * sizeof(float2));
  p.off_stats = cur.take((size_t)B * 2 * sizeof(float2));
  p.total = cur.o;
  return CTASNET_OK;
}

}  // namespace

extern "C" {

int ctasnet_abi_version(void) { return CTASNET_ABI_VERSION; }

int ctasnet_create(ctasnet_handle* out) {
  if (int rc = ct_create(out, "Conv-TasNet", g_create_error)) return rc;
  add_convtasnet_names(*out);
  (*out)->w.assign((*out)->names.size(), nullptr);
  return CTASNET_OK;
}

void ctasnet_destroy(ctasnet_handle h) { delete h; }

const char* ctasnet_last_error(ctasnet_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ctasnet_num_weights(ctasnet_handle h) { return h ? (int)h->names.size() : 0; }

const char* ctasnet_weight_name(ctasnet_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t ctasnet_weight_numel(ctasnet_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int ctasnet_bind_weights(ctasnet_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n) : CTASNET_ERR_INVALID;
}

int64_t ctasnet_frames(int64_t T) { return frames_of(T); }

int64_t ctasnet_out_len(int64_t T) { return out_len_of(T); }

size_t ctasnet_workspace_bytes(ctasnet_handle h, int B, int64_t T) {
  if (!h) return 0;
  Plan p;
  if (make_plan(h, B, T, p)) return 0;
  return p.total;
}

int ctasnet_forward(ctasnet_handle h, const float* mix, int B, int64_t T, float* s1_pred, float* s2_pred, void* ws,
                    size_t ws_bytes, void* stream) {
  if (!h) return CTASNET_ERR_INVALID;
  ctasnet_ctx* c = h;
  if (!c->bound) return c->fail(CTASNET_ERR_WEIGHTS, "weights not bound (ctasnet_bind_weights)");
  if (!mix || !s1_pred || !s2_pred) return c->fail(CTASNET_ERR_INVALID, "mix / s1_pred / s2_pred must not be NULL");
  Plan p;
  if (int rc = make_plan(c, B, T, p)) return rc;
  if (int rc = check_workspace(c, p.total, ws, ws_bytes)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  float* enc = reinterpret_cast<float*>(base + p.off_enc);
  float* cbuf = reinterpret_cast<float*>(base + p.off_c);
  float* taps = reinterpret_cast<float*>(base + p.off_taps);
  float2* part = reinterpret_cast<float2*>(base + p.off_part);
  float2* stats1 = reinterpret_cast<float2*>(base + p.off_stats);
  const SepBuffers sb{reinterpret_cast<float*>(base + p.off_x), reinterpret_cast<float*>(base + p.off_skip), cbuf,
                      reinterpret_cast<float*>(base + p.off_w), part, stats1, stats1, stats1 + B, cbuf, nullptr};
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  const unsigned row_wgs = (unsigned)((M + CT_ROWS_PER_WG - 1) / CT_ROWS_PER_WG);

  // encoder (convtasnet.py:12-15), then the Separator on its output (convtasnet.py:55-83)
  hipLaunchKernelGGL(ctasnet_encoder_kernel<false>, dim3(row_wgs), dim3(256), 0, st, mix, T, F, M, W[0], nullptr, enc, part);
  HANDLE_LAUNCH_CHECK(c, "ctasnet encoder");
  if (int rc = launch_separator<false>(c, st, W.data() + 1, enc, 2, 256.0f, B, F, M, sb)) return rc;

  // decoder taps, overlap-add (convtasnet.py:92-97)
  if (int rc = launch_taps(c, st, cbuf, W[1 + CT_SEP_W], M, taps)) return rc;
  return launch_overlap_add<false>(c, st, taps, nullptr, B, F, p.Lout, s1_pred, s2_pred);
}

double ctasnet_flops_per_mixture(ctasnet_handle, int64_t T) {
  return 2.0 * convtasnet_macs() * (double)frames_of(T);
}

double ctasnet_min_bytes_per_mixture(ctasnet_handle, int64_t T) {
  // floats per frame that the launches read + write once each (row partials and per-mixture statistics are ~1 % and left out)
  const double F = (double)frames_of(T);
  const double enc = CT_N + 1.0 * CT_N;                        // encoder writes enc; the bottleneck GEMM reads it
  const double bottleneck = CT_B;                              // ... and writes x
  const double block = (CT_B + CT_H)                           // (a) reads x, writes c
                       + (CT_R * CT_H + CT_H)                  // (b) reads 3 rows of c (dilated taps), writes w
                       + (CT_H + 2.0 * CT_B + 2.0 * CT_B);     // (c) reads w, x, skip; writes x, skip
  const double tail = (CT_B + CT_N + 2 * CT_N)                 // mask GEMM: skip, enc in; ym out
                      + (2 * CT_N + 4 * CT_L)                  // taps
                      + (4 * CT_L + 2 * CT_L);                 // overlap-add
  return 4.0 * F * (enc + bottleneck + CT_BLOCKS * block + tail) + 4.0 * (double)T;
}

}  // extern "C"
