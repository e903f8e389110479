// ctasnet_handle.h -- the host-side scaffolding the three Conv-TasNet handles share (ctasnet.hip, deepctasnet.hip,
// ctasnet_train.hip): the context base, the frame arithmetic, the Separator's weight table and the argument checks of
// the extern "C" entry points.  The three headers under include/ give their error codes the same values (deepctasnet.hip
// and ctasnet_train.hip assert it), so the shared code returns CTASNET_* codes, as ctasnet_kernels.h does.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "ctasnet_kernels.h"

namespace {

struct CtHandle {
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
  void add(const std::string& n, int64_t numel) {
    names.push_back(n);
    numels.push_back(numel);
  }
  const char* weight_name(int i) const { return (i >= 0 && i < (int)names.size()) ? names[i].c_str() : nullptr; }
  int64_t weight_numel(int i) const { return (i >= 0 && i < (int)numels.size()) ? numels[i] : -1; }
};

// *_create: a new Ctx on the current device, or the reason in create_error (what *_last_error(NULL) returns).
// `model` completes "libdptnav's ... has no CPU path".  The caller fills in the weight table.
template <class Ctx>
int ct_create(Ctx** out, const char* model, std::string& create_error) {
  if (!out) {
    create_error = "out must not be NULL";
    return CTASNET_ERR_INVALID;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    create_error = std::string("no HIP device visible: libdptnav's ") + model + " has no CPU path";
    return CTASNET_ERR_INVALID;
  }
  Ctx* c = new Ctx();
  int devid = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&devid) == hipSuccess) c->device_id = devid;
  if (hipGetDeviceProperties(&prop, devid) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
  *out = c;
  return CTASNET_OK;
}

inline int64_t frames_of(int64_t T) { return T < CT_L ? 0 : (T + CT_L) / CT_L + 1; }
inline int64_t out_len_of(int64_t T) { return T < CT_L ? 0 : CT_L * (T / CT_L); }

// the Separator's CT_SEP_W entries (src/model/convtasnet.py:55-83), state_dict order
inline void add_separator_names(CtHandle* c) {
  c->add("separator.norm_1.gamma", CT_N);
  c->add("separator.norm_1.beta", CT_N);
  c->add("separator.conv1d.weight", (int64_t)CT_B * CT_N);
  c->add("separator.conv1d.bias", CT_B);
  for (int i = 0; i < CT_BLOCKS; ++i) {
    const std::string p = "separator.separator." + std::to_string(i) + ".";
    c->add(p + "conv1d.weight", (int64_t)CT_H * CT_B);
    c->add(p + "conv1d.bias", CT_H);
    c->add(p + "PReLU_1.weight", 1);
    c->add(p + "norm_1.weight", CT_H);
    c->add(p + "norm_1.bias", CT_H);
    c->add(p + "dconv1d.weight", (int64_t)CT_H * CT_R);
    c->add(p + "dconv1d.bias", CT_H);
    c->add(p + "PReLU_2.weight", 1);
    c->add(p + "norm_2.weight", CT_H);
    c->add(p + "norm_2.bias", CT_H);
    c->add(p + "conv.weight", (int64_t)CT_B * CT_H);
    c->add(p + "conv.bias", CT_B);
    c->add(p + "conv_sc.weight", (int64_t)CT_B * CT_H);
    c->add(p + "conv_sc.bias", CT_B);
  }
  c->add("separator.seq.0.weight", 1);
  c->add("separator.seq.1.weight", (int64_t)2 * CT_N * CT_B);
  c->add("separator.seq.1.bias", 2 * CT_N);
}

// Conv-TasNet's own table: encoder, Separator, decoder (ConvTasNet and its training step)
inline void add_convtasnet_names(CtHandle* c) {
  c->add("encoder.conv1d.weight", (int64_t)CT_N * 2 * CT_L);
  add_separator_names(c);
  c->add("decoder.deconv.weight", (int64_t)CT_N * 2 * CT_L);
}

// multiply-accumulates per frame of the Separator and of the whole Conv-TasNet (*_flops_per_mixture)
inline double separator_macs() {
  const double per_block = (double)CT_B * CT_H + (double)CT_H * CT_R + 2.0 * CT_H * CT_B;
  return (double)CT_N * CT_B + CT_BLOCKS * per_block + (double)CT_B * 2 * CT_N;
}
inline double convtasnet_macs() { return (double)CT_N * 2 * CT_L + separator_macs() + 2.0 * CT_N * 2 * CT_L; }

// one device pointer per table entry, none NULL, each `align`-byte aligned; kind = "weight" / "gradient"
inline int check_table_ptrs(CtHandle* h, const void* const* ptrs, int n, const char* kind, unsigned align) {
  const int nw = (int)h->names.size();
  if (n != nw || !ptrs) return h->fail(CTASNET_ERR_WEIGHTS, "expected %d %s pointers, got %d", nw, kind, n);
  for (int i = 0; i < n; ++i) {
    if (!ptrs[i]) return h->fail(CTASNET_ERR_WEIGHTS, "%s %d (%s) is NULL", kind, i, h->names[i].c_str());
    if (reinterpret_cast<uintptr_t>(ptrs[i]) % align)
      return h->fail(CTASNET_ERR_WEIGHTS, "%s %d (%s) is not %u-byte aligned", kind, i, h->names[i].c_str(), align);
  }
  return CTASNET_OK;
}

inline int bind_weights(CtHandle* h, const float* const* dev_ptrs, int n) {
  if (int rc = check_table_ptrs(h, reinterpret_cast<const void* const*>(dev_ptrs), n, "weight", 16)) return rc;
  h->w.assign(dev_ptrs, dev_ptrs + n);
  h->bound = true;
  return CTASNET_OK;
}

// the checks every plan starts with
inline int check_batch(CtHandle* c, int B, int64_t T) {
  if (B <= 0) return c->fail(CTASNET_ERR_INVALID, "B must be >= 1 (got %d)", B);
  if (T < CT_L) return c->fail(CTASNET_ERR_INVALID, "T must be >= %d samples (got %lld): the output would be empty", CT_L,
                               (long long)T);
  return CTASNET_OK;
}

inline int check_workspace(CtHandle* c, size_t need, const void* ws, size_t ws_bytes) {
  if (!ws || ws_bytes < need || reinterpret_cast<uintptr_t>(ws) % 256)
    return c->fail(CTASNET_ERR_WORKSPACE, "workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", need, ws_bytes, ws);
  return CTASNET_OK;
}

}  // namespace
