// ctasnet.hip -- Conv-TasNet inference forward (src/model/convtasnet.py) for gfx950: handle and the extern "C" boundary
// declared in include/ctasnet.h.  The kernels, engine hooks and the separator's launch sequence live in ctasnet_kernels.h
// (shared with deepctasnet.hip); the layout and the statistics scheme are described there.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ctasnet.h"
#include "common.h"
// gemm_ws.h also defines the (non-template) weight-packing kernel that dptnav.hip launches; this unit does not use it, and
// renaming its copy here keeps the two objects from defining the same symbol without touching the engine header.
#define gemm_pack_rows_kernel ctasnet_unused_gemm_pack_rows_kernel
#include "gemm_ws.h"
#undef gemm_pack_rows_kernel
#include "ctasnet_kernels.h"

namespace {

constexpr int CT_NW = 5 + CT_BLOCKS * CT_BLOCK_W + 4;

thread_local std::string g_create_error;

// overlap-add and crop: out_s[b][t] = taps[b F + f][s][k] + taps[b F + f - 1][s][k + 16], t + 16 = 16 f + k
__global__ __launch_bounds__(256) void ctasnet_overlap_add_kernel(const float* __restrict__ taps, int B, int F,
                                                                  int64_t Lout, float* __restrict__ s1,
                                                                  float* __restrict__ s2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * (int64_t)B * Lout) return;
  const int64_t bs = i / Lout, t = i - bs * Lout;
  const int64_t b = bs >> 1;
  const int s = (int)(bs & 1);
  const int64_t j = t + CT_L, f = j / CT_L, k = j - f * CT_L;
  const float* tp = taps + (b * F + f) * (4 * CT_L) + s * 2 * CT_L;
  const float v = tp[k] + tp[k + CT_L - 4 * CT_L];   // previous frame's taps k + 16
  (s ? s2 : s1)[b * Lout + t] = v;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct Plan {
  int64_t F, M, Lout;
  size_t off_enc, off_x, off_skip, off_c, off_w, off_taps, off_part, off_stats, total;
};

}  // namespace

struct ctasnet_ctx {
  std::string err;
  std::vector<std::string> names;
  std::vector<int64_t> numels;
  std::vector<const float*> w;
  bool bound = false;
  int device_id = 0;
  int num_cus = 256;
  int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
};

namespace {

void build_names(ctasnet_ctx* c) {
  auto add = [&](const std::string& n, int64_t numel) { c->names.push_back(n); c->numels.push_back(numel); };
  add("encoder.conv1d.weight", (int64_t)CT_N * 2 * CT_L);
  add("separator.norm_1.gamma", CT_N);
  add("separator.norm_1.beta", CT_N);
  add("separator.conv1d.weight", (int64_t)CT_B * CT_N);
  add("separator.conv1d.bias", CT_B);
  for (int i = 0; i < CT_BLOCKS; ++i) {
    const std::string p = "separator.separator." + std::to_string(i) + ".";
    add(p + "conv1d.weight", (int64_t)CT_H * CT_B);
    add(p + "conv1d.bias", CT_H);
    add(p + "PReLU_1.weight", 1);
    add(p + "norm_1.weight", CT_H);
    add(p + "norm_1.bias", CT_H);
    add(p + "dconv1d.weight", (int64_t)CT_H * CT_R);
    add(p + "dconv1d.bias", CT_H);
    add(p + "PReLU_2.weight", 1);
    add(p + "norm_2.weight", CT_H);
    add(p + "norm_2.bias", CT_H);
    add(p + "conv.weight", (int64_t)CT_B * CT_H);
    add(p + "conv.bias", CT_B);
    add(p + "conv_sc.weight", (int64_t)CT_B * CT_H);
    add(p + "conv_sc.bias", CT_B);
  }
  add("separator.seq.0.weight", 1);
  add("separator.seq.1.weight", (int64_t)2 * CT_N * CT_B);
  add("separator.seq.1.bias", 2 * CT_N);
  add("decoder.deconv.weight", (int64_t)CT_N * 2 * CT_L);
}

int64_t frames_of(int64_t T) { return T < CT_L ? 0 : (T + CT_L) / CT_L + 1; }

int make_plan(ctasnet_ctx* c, int B, int64_t T, Plan& p) {
  if (B <= 0) return c->fail(CTASNET_ERR_INVALID, "B must be >= 1 (got %d)", B);
  if (T < CT_L) return c->fail(CTASNET_ERR_INVALID, "T must be >= %d samples (got %lld): the output would be empty", CT_L,
                               (long long)T);
  p.F = frames_of(T);
  p.M = (int64_t)B * p.F;
  if (p.M * CT_H > (int64_t)INT32_MAX)
    return c->fail(CTASNET_ERR_INVALID, "B*F*512 = %lld exceeds 32-bit indexing (B=%d, T=%lld)", (long long)(p.M * CT_H), B,
                   (long long)T);
  p.Lout = CT_L * (T / CT_L);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t r = o; o += align256(bytes); return r; };
  const size_t M = (size_t)p.M;
  p.off_enc = take(M * CT_N * 4);
  p.off_x = take(M * CT_B * 4);
  p.off_skip = take(M * CT_B * 4);
  p.off_c = take(M * CT_H * 4);        // c and w are contiguous: the head's masked rows [M][1024] reuse both
  p.off_w = take(M * CT_H * 4);
  p.off_taps = take(M * 4 * CT_L * 4);
  p.off_part = take(M * 4 * sizeof(float2));
  p.off_stats = take((size_t)B * 2 * sizeof(float2));
  p.total = o;
  return CTASNET_OK;
}

}  // namespace

extern "C" {

int ctasnet_abi_version(void) { return CTASNET_ABI_VERSION; }

int ctasnet_create(ctasnet_handle* out) {
  if (!out) {
    g_create_error = "out must not be NULL";
    return CTASNET_ERR_INVALID;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    g_create_error = "no HIP device visible: libdptnav's Conv-TasNet has no CPU path";
    return CTASNET_ERR_INVALID;
  }
  ctasnet_ctx* c = new ctasnet_ctx();
  int devid = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&devid) == hipSuccess) c->device_id = devid;
  if (hipGetDeviceProperties(&prop, devid) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
  build_names(c);
  c->w.assign(c->names.size(), nullptr);
  *out = c;
  return CTASNET_OK;
}

void ctasnet_destroy(ctasnet_handle h) { delete h; }

const char* ctasnet_last_error(ctasnet_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ctasnet_num_weights(ctasnet_handle h) { return h ? (int)h->names.size() : 0; }

const char* ctasnet_weight_name(ctasnet_handle h, int i) {
  return (h && i >= 0 && i < (int)h->names.size()) ? h->names[i].c_str() : nullptr;
}

int64_t ctasnet_weight_numel(ctasnet_handle h, int i) {
  return (h && i >= 0 && i < (int)h->numels.size()) ? h->numels[i] : -1;
}

int ctasnet_bind_weights(ctasnet_handle h, const float* const* dev_ptrs, int n) {
  if (!h) return CTASNET_ERR_INVALID;
  if (n != CT_NW || !dev_ptrs) return h->fail(CTASNET_ERR_WEIGHTS, "expected %d weight pointers, got %d", CT_NW, n);
  for (int i = 0; i < n; ++i) {
    if (!dev_ptrs[i]) return h->fail(CTASNET_ERR_WEIGHTS, "weight %d (%s) is NULL", i, h->names[i].c_str());
    if (reinterpret_cast<uintptr_t>(dev_ptrs[i]) % 16)
      return h->fail(CTASNET_ERR_WEIGHTS, "weight %d (%s) is not 16-byte aligned", i, h->names[i].c_str());
  }
  h->w.assign(dev_ptrs, dev_ptrs + n);
  h->bound = true;
  return CTASNET_OK;
}

int64_t ctasnet_frames(int64_t T) { return frames_of(T); }

int64_t ctasnet_out_len(int64_t T) { return T < CT_L ? 0 : CT_L * (T / CT_L); }

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
  if (!ws || ws_bytes < p.total || reinterpret_cast<uintptr_t>(ws) % 256)
    return c->fail(CTASNET_ERR_WORKSPACE, "workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", p.total, ws_bytes, ws);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  float* enc = reinterpret_cast<float*>(base + p.off_enc);
  float* cbuf = reinterpret_cast<float*>(base + p.off_c);
  float* taps = reinterpret_cast<float*>(base + p.off_taps);
  float2* part = reinterpret_cast<float2*>(base + p.off_part);
  float2* stats1 = reinterpret_cast<float2*>(base + p.off_stats);
  const SepBuffers sb{reinterpret_cast<float*>(base + p.off_x), reinterpret_cast<float*>(base + p.off_skip), cbuf,
                      reinterpret_cast<float*>(base + p.off_w), part, stats1, stats1 + B};
  const int F = (int)p.F;
  const int64_t M = p.M;
  const auto& W = c->w;
  const unsigned row_wgs = (unsigned)((M + CT_ROWS_PER_WG - 1) / CT_ROWS_PER_WG);

  // encoder (convtasnet.py:12-15), then the Separator on its output (convtasnet.py:55-83)
  hipLaunchKernelGGL(ctasnet_encoder_kernel<false>, dim3(row_wgs), dim3(256), 0, st, mix, T, F, M, W[0], nullptr, enc, part);
  CT_LAUNCH_CHECK(c, "ctasnet encoder");
  if (int rc = launch_separator(c, st, W.data() + 1, enc, 2, 256.0f, B, F, M, sb)) return rc;

  // decoder taps, overlap-add (convtasnet.py:92-97)
  if (int rc = launch_taps(c, st, cbuf, W[1 + CT_SEP_W], M, taps)) return rc;
  const int64_t n_out = 2 * (int64_t)B * p.Lout;
  hipLaunchKernelGGL(ctasnet_overlap_add_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, taps, B, F, p.Lout,
                     s1_pred, s2_pred);
  CT_LAUNCH_CHECK(c, "ctasnet overlap-add");
  return CTASNET_OK;
}

double ctasnet_flops_per_mixture(ctasnet_handle, int64_t T) {
  const double F = (double)frames_of(T);
  const double per_block = (double)CT_B * CT_H + (double)CT_H * CT_R + 2.0 * CT_H * CT_B;
  const double mac = (double)CT_N * 2 * CT_L + (double)CT_N * CT_B + CT_BLOCKS * per_block + (double)CT_B * 2 * CT_N +
                     2.0 * CT_N * 2 * CT_L;
  return 2.0 * mac * F;
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
