// ctasnet_handle.h -- what the Conv-TasNet handles (ctasnet.hip, deepctasnet.hip, ctasnet_train.hip, deepctasnet_train.hip)
// share on the host beyond handle.h's model-neutral scaffolding: the context base with its device, the frame arithmetic, the
// Separator's weight table, the MAC counts and the batch check.  The family's headers under include/ give their error codes
// the same values (the units assert it against CTASNET_*), which are handle.h's.
#pragma once
#include "ctasnet_kernels.h"

HANDLE_ASSERT_CODES(CTASNET);

namespace {

struct CtHandle : Handle {
  int device_id = 0;
  int num_cus = 256;
};

// *_create: handle.h's create on the current device.  `model` completes "libdptnav's ... has no CPU path".
template <class Ctx>
int ct_create(Ctx** out, const char* model, std::string& create_error) {
  if (int rc = create(out, model, create_error)) return rc;
  Ctx* c = *out;
  int devid = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&devid) == hipSuccess) c->device_id = devid;
  if (hipGetDeviceProperties(&prop, devid) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
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

// the family binds 16-byte aligned weights: its loaders read them four floats at a time
inline int bind_weights(CtHandle* h, const float* const* dev_ptrs, int n) { return bind_weights(h, dev_ptrs, n, 16); }

// the checks every plan starts with
inline int check_batch(CtHandle* c, int B, int64_t T) {
  if (B <= 0) return c->fail(CTASNET_ERR_INVALID, "B must be >= 1 (got %d)", B);
  if (T < CT_L) return c->fail(CTASNET_ERR_INVALID, "T must be >= %d samples (got %lld): the output would be empty", CT_L,
                               (long long)T);
  return CTASNET_OK;
}

}  // namespace
