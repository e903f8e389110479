// handle.h -- the model-neutral part of a handle behind an extern "C" boundary: the context base (last error, weight table,
// bound pointers), *_create's preamble, the pointer-table and workspace checks, the launch check and the byte cursor a
// workspace plan is laid out with.  Users: the Conv-TasNet family (ctasnet_handle.h), lipfe.hip, lipsn.hip, vfilt.hip.
// The public headers under include/ give their five codes the same values, so the shared code returns H_*; every user
// asserts it for its own header (HANDLE_ASSERT_CODES).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace {

enum { H_OK = 0, H_ERR_INVALID = 1, H_ERR_WORKSPACE = 2, H_ERR_WEIGHTS = 3, H_ERR_HIP = 4 };

#define HANDLE_ASSERT_CODES(P)                                                                                        \
  static_assert(P##_OK == H_OK && P##_ERR_INVALID == H_ERR_INVALID && P##_ERR_WORKSPACE == H_ERR_WORKSPACE &&         \
                    P##_ERR_WEIGHTS == H_ERR_WEIGHTS && P##_ERR_HIP == H_ERR_HIP,                                     \
                "handle.h returns its own codes through this header's entry points")

struct Handle {
  std::string err;
  std::vector<std::string> names;
  std::vector<int64_t> numels;
  std::vector<const float*> w;
  bool bound = false;
  int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
  int add(const std::string& n, int64_t numel) {   // returns the entry's index
    names.push_back(n);
    numels.push_back(numel);
    return (int)names.size() - 1;
  }
  const char* weight_name(int i) const { return (i >= 0 && i < (int)names.size()) ? names[i].c_str() : nullptr; }
  int64_t weight_numel(int i) const { return (i >= 0 && i < (int)numels.size()) ? numels[i] : -1; }
};

// *_create refuses: no handle, the reason in create_error (what *_last_error(NULL) returns)
template <class Ctx>
int refuse_create(Ctx** out, std::string& create_error, const std::string& why) {
  if (out) *out = nullptr;
  create_error = why;
  return H_ERR_INVALID;
}

// *_create: a new Ctx, or the reason in create_error.  `what` completes "libdptnav's ... has no CPU path".  The caller
// fills in the weight table.
template <class Ctx>
int create(Ctx** out, const char* what, std::string& create_error) {
  if (!out) return refuse_create(out, create_error, "out must not be NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return refuse_create(out, create_error, std::string("no HIP device visible: libdptnav's ") + what + " has no CPU path");
  *out = new Ctx();
  return H_OK;
}

// one device pointer per table entry, none NULL, each `align`-byte aligned; kind = "weight" / "gradient"
inline int check_table_ptrs(Handle* h, const void* const* ptrs, int n, const char* kind, unsigned align) {
  const int nw = (int)h->names.size();
  if (n != nw || !ptrs) return h->fail(H_ERR_WEIGHTS, "expected %d %s pointers, got %d", nw, kind, n);
  for (int i = 0; i < n; ++i) {
    if (!ptrs[i]) return h->fail(H_ERR_WEIGHTS, "%s %d (%s) is NULL", kind, i, h->names[i].c_str());
    if (reinterpret_cast<uintptr_t>(ptrs[i]) % align)
      return h->fail(H_ERR_WEIGHTS, "%s %d (%s) is not %u-byte aligned", kind, i, h->names[i].c_str(), align);
  }
  return H_OK;
}

inline int bind_weights(Handle* h, const float* const* dev_ptrs, int n, unsigned align) {
  if (int rc = check_table_ptrs(h, reinterpret_cast<const void* const*>(dev_ptrs), n, "weight", align)) return rc;
  h->w.assign(dev_ptrs, dev_ptrs + n);
  h->bound = true;
  return H_OK;
}

inline int check_workspace(Handle* c, size_t need, const void* ws, size_t ws_bytes) {
  if (!ws || ws_bytes < need || reinterpret_cast<uintptr_t>(ws) % 256)
    return c->fail(H_ERR_WORKSPACE, "workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", need, ws_bytes, ws);
  return H_OK;
}

#define HANDLE_LAUNCH_CHECK(c, what)                                                         \
  do {                                                                                       \
    hipError_t e_ = hipGetLastError();                                                       \
    if (e_ != hipSuccess) return (c)->fail(H_ERR_HIP, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// a workspace plan is laid out with it: take(bytes) is the offset of the next piece, pieces start 256-byte aligned
struct ByteCursor {
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t r = o;
    o += align256(bytes);
    return r;
  }
};

}  // namespace
