// lipsn.hip -- the ShuffleNet-v2 lip reader (src/lipreader/lipreading/model.py:141-273 with backbone_type = "shufflenet" and
// extract_feats = True: 24-channel Conv3d stem + ShuffleNetV2.features + conv_last + AvgPool2d(3), mouth video -> 1024-wide
// embeddings per frame) for gfx950: handle and the extern "C" boundary declared in include/lipsn.h; the kernels are in
// lipsn_kernels.h.  The handle's scaffolding is handle.h's; everything up to the trunk (argument checks, the head of the
// workspace plan, fold, stem, max-pool) is lipfront.h's, shared with lipfe.hip.
//
// One forward is 21 launches, all on the caller's stream:
//   fold      the 56 eval-mode BatchNorms -> scale = w / sqrt(var + eps), shift = b - mean * scale         (1 launch)
//   pack      the 56 conv weights [Cout][K] -> [K][Cout padded to 32 with zero columns]                     (1 launch)
//   stem      Conv3d + BN + act on plain VALU, window and affine applied on load; then the max-pool        (2 launches)
//   blocks    one launch per InvertedResidual: pointwise (MFMA) -> depthwise (VALU) -> pointwise (MFMA) with the
//             intermediates in LDS; concat + channel shuffle are the store index                           (16 launches)
//   last      conv_last + BN + ReLU + the mean over rows / columns 0..2 of the final map                   (1 launch)
// The derived copies (fold, pack) are made in every forward, into the workspace: a copy made at bind time would go stale
// when load_state_dict copies into the same storages.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lipsn.h"
#include "lipsn_kernels.h"

HANDLE_ASSERT_CODES(LIPSN);
static_assert(LIPSN_RELU == LF_ACT_RELU && LIPSN_PRELU == LF_ACT_PRELU && LIPSN_SWISH == LF_ACT_SWISH, "relu_type is LF_ACT_*");

namespace {
thread_local std::string g_sn_create_error;

constexpr int SN_BLOCK_LDS_FLOATS = 16384;   // 64 KiB per workgroup of the block kernel: two of them fit a CU's 160 KiB
constexpr int SN_LAUNCHES = 21;
const int SN_REPEATS[3] = {4, 8, 4};
const int SN_STAGES[2][3] = {{48, 96, 192}, {116, 232, 464}};   // width_x2 = 1, 2

struct SnConv {
  int w, bn;            // weight-table indices: conv weight, bn.weight (bias, mean, var follow)
  int K, cout, np;      // source [cout][K] -> pack [K][np]
  int pack_off, fold_off;
};

struct SnBlock {
  int stride, cin, ch;
  SnConv pw1, dw, pw2;  // banch2
  SnConv dw1, pwb1;     // banch1 (stride 2)
};

struct SnBlockPlan {
  int band, bands, G, ksx, ksm, ksd, offM, offD, lds_floats;
};

struct SnPlan : LfPlan {
  size_t off_act[2];
};

const LfModel LIPSN_MODEL = {"lipsn", SN_STEM_C, INT32_MAX / 4, "the supported 2^29 positions", lipsn_fold_kernel, lipsn_stem_kernel,
                             lipsn_maxpool_kernel};

inline int pad32(int n) { return (n + 31) & ~31; }

// LDS floats of a tile of `band` output rows of G frames; fills the offsets
int sn_block_lds(int stride, int Hi, int Wi, int Wo, int cin, int ch, int band, int G, SnBlockPlan& b) {
  const int RI = std::min(Hi, (band - 1) * stride + 3);
  const int Pin = G * RI * Wi, Q = G * band * Wo;
  b.ksx = (stride == 1 ? ch : cin) | 1;
  b.ksm = ch | 1;
  b.ksd = stride == 1 ? b.ksx : (std::max(cin, ch) | 1);
  const int X = Pin * b.ksx, M = Pin * b.ksm, D = Q * b.ksd;
  if (stride == 1) { b.offD = 0;  b.offM = std::max(X, D);  b.lds_floats = b.offM + M; }
  else { b.offM = X;  b.offD = X + M;  b.lds_floats = X + M + D; }
  return b.lds_floats;
}

// the largest band of output rows whose tile fits the LDS budget; where a whole frame fits, as many frames as fit, up to 64
// output positions (two MFMA row tiles)
SnBlockPlan sn_plan_block(int stride, int Hi, int Wi, int Ho, int Wo, int cin, int ch) {
  SnBlockPlan b;
  int band = Ho;
  while (band > 1 && sn_block_lds(stride, Hi, Wi, Wo, cin, ch, band, 1, b) > SN_BLOCK_LDS_FLOATS) --band;
  int G = 1;
  if (band == Ho)
    while ((G + 1) * Ho * Wo <= 64 && sn_block_lds(stride, Hi, Wi, Wo, cin, ch, band, G + 1, b) <= SN_BLOCK_LDS_FLOATS) ++G;
  sn_block_lds(stride, Hi, Wi, Wo, cin, ch, band, G, b);
  b.band = band;  b.bands = (Ho + band - 1) / band;  b.G = G;
  return b;
}
}  // namespace

struct lipsn_ctx : LfCtx {
  int width_x2 = 2;
  SnBlock blocks[16];
  SnConv last, stem;
  std::vector<SnConv*> convs;   // every conv, in table order: the pack jobs
  lipsn_ctx() { model = &LIPSN_MODEL; }
  // conv `p0`.weight [cout][K] followed by the BatchNorm `p1`*
  void conv(SnConv& d, const std::string& p0, const std::string& p1, int cout, int K, int np) {
    d.w = add(p0 + "weight", (int64_t)cout * K);
    d.bn = add_bn(p1, cout, d.fold_off);
    d.K = K;  d.cout = cout;  d.np = np;
    d.pack_off = (int)pack_floats;  pack_floats += K * np;
    convs.push_back(&d);
  }
};

namespace {
// the reference's state_dict() order without tcn.* and num_batches_tracked: the trunk is registered before the stem
void sn_build_table(lipsn_ctx* c) {
  const int* stages = SN_STAGES[c->width_x2 - 1];
  int inp = SN_STEM_C, bi = 0;
  for (int s = 0; s < 3; ++s) {
    const int ch = stages[s] / 2, np = pad32(ch);
    for (int r = 0; r < SN_REPEATS[s]; ++r, ++bi) {
      SnBlock& b = c->blocks[bi];
      const std::string p = "trunk.0." + std::to_string(bi) + ".";
      b.stride = r == 0 ? 2 : 1;  b.cin = inp;  b.ch = ch;
      if (r == 0) {
        c->conv(b.dw1, p + "banch1.0.", p + "banch1.1.", inp, 9, inp);
        c->conv(b.pwb1, p + "banch1.2.", p + "banch1.3.", ch, inp, np);
      }
      c->conv(b.pw1, p + "banch2.0.", p + "banch2.1.", ch, r == 0 ? inp : ch, np);
      c->conv(b.dw, p + "banch2.3.", p + "banch2.4.", ch, 9, ch);
      c->conv(b.pw2, p + "banch2.5.", p + "banch2.6.", ch, ch, np);
      inp = stages[s];
    }
  }
  c->conv(c->last, "trunk.1.0.", "trunk.1.1.", SN_LAST_N, inp, SN_LAST_N);
  c->conv(c->stem, "frontend3D.0.", "frontend3D.1.", SN_STEM_C, 245, SN_STEM_CP);
  if (c->act == LIPSN_PRELU) c->stem_slope = c->add("frontend3D.2.weight", SN_STEM_C);
  c->stem_pack_off = c->stem.pack_off;  c->stem_fold_off = c->stem.fold_off;
  c->w.assign(c->names.size(), nullptr);
}

const char* sn_check_shape(int S, int T, int H, int W) {
  if (S < 1) return "S must be >= 1";
  if (T < 1) return "T must be >= 1";
  if (H < LIPSN_MIN_HW || H > LIPSN_MAX_HW || W < LIPSN_MIN_HW || W > LIPSN_MAX_HW)
    return "H and W must be in [65, 160] (where the reference's AvgPool2d(3) yields one position)";
  return nullptr;
}

int sn_make_plan(lipsn_ctx* c, int S, int T, int H, int W, SnPlan& p) {
  ByteCursor cur;
  if (int rc = lf_plan_head(c, sn_check_shape(S, T, H, W), S, T, H, W, p, cur)) return rc;
  const int* stages = SN_STAGES[c->width_x2 - 1];
  size_t act = (size_t)p.z.h[0] * p.z.w[0] * SN_STEM_C;
  for (int l = 1; l < 4; ++l) act = std::max(act, (size_t)p.z.h[l] * p.z.w[l] * stages[l - 1]);
  for (int i = 0; i < 2; ++i) p.off_act[i] = cur.take((size_t)p.N * act * 4);
  p.total = cur.o;
  return LIPSN_OK;
}

size_t sn_last_lds_bytes(int C) { return (size_t)(9 * SN_LAST_G * ((C | 1) + 4 * 33)) * 4; }

double sn_macs_per_frame(int width_x2, int H, int W) {
  const LfSizes z = sizes_of(H, W);
  const int* stages = SN_STAGES[width_x2 - 1];
  double macs = (double)z.Hs * z.Ws * SN_STEM_C * 245;
  int inp = SN_STEM_C;
  for (int s = 0; s < 3; ++s) {
    const double ch = stages[s] / 2, pin = (double)z.h[s] * z.w[s], pout = (double)z.h[s + 1] * z.w[s + 1];
    macs += pout * inp * 9 + pout * inp * ch;                     // banch1 of the stride-2 block
    macs += pin * inp * ch + pout * ch * 9 + pout * ch * ch;      // its banch2
    macs += (SN_REPEATS[s] - 1) * pout * (2 * ch * ch + 9 * ch);  // the stride-1 blocks
    inp = stages[s];
  }
  return macs + (double)z.h[3] * z.w[3] * inp * SN_LAST_N;
}
}  // namespace

extern "C" {

int lipsn_abi_version(void) { return LIPSN_ABI_VERSION; }

int lipsn_create(lipsn_handle* out, int relu_type, int width_x2) {
  if (out && relu_type != LIPSN_RELU && relu_type != LIPSN_PRELU && relu_type != LIPSN_SWISH)
    return refuse_create(out, g_sn_create_error,
                         "relu_type must be LIPSN_RELU, LIPSN_PRELU or LIPSN_SWISH (got " + std::to_string(relu_type) + ")");
  if (out && width_x2 != 1 && width_x2 != 2)
    return refuse_create(out, g_sn_create_error,
                         "width_x2 must be 1 (width_mult 0.5) or 2 (width_mult 1.0): width_mult 1.5 and 2.0 are not built (got " +
                             std::to_string(width_x2) + ")");
  if (int rc = create(out, "ShuffleNet lip reader", g_sn_create_error)) return rc;
  lipsn_ctx* c = *out;
  // both kernels take more dynamic LDS than the default limit
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lipsn_block_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     SN_BLOCK_LDS_FLOATS * 4);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(lipsn_last_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)sn_last_lds_bytes(SN_STAGES[1][2]));
  if (e != hipSuccess) {
    delete c;
    refuse_create(out, g_sn_create_error, std::string("hipFuncSetAttribute (dynamic LDS): ") + hipGetErrorString(e));
    return LIPSN_ERR_HIP;
  }
  c->act = relu_type;
  c->width_x2 = width_x2;
  sn_build_table(c);
  return LIPSN_OK;
}

void lipsn_destroy(lipsn_handle h) { delete h; }

const char* lipsn_last_error(lipsn_handle h) { return h ? h->err.c_str() : g_sn_create_error.c_str(); }

int lipsn_num_weights(lipsn_handle h) { return h ? (int)h->names.size() : 0; }

const char* lipsn_weight_name(lipsn_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t lipsn_weight_numel(lipsn_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int lipsn_bind_weights(lipsn_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n, 4) : LIPSN_ERR_INVALID;
}

size_t lipsn_workspace_bytes(lipsn_handle h, int S, int T, int H, int W) {
  if (!h) return 0;
  SnPlan p;
  if (sn_make_plan(h, S, T, H, W, p)) return 0;
  return p.total;
}

int lipsn_forward(lipsn_handle h, const float* x, int S, int T, int Hin, int Win, int y0, int x0, int H, int W, float a, float b,
                  float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return LIPSN_ERR_INVALID;
  lipsn_ctx* c = h;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SnPlan p;
  // the front: act[0] = [N][h0][w0][24]; the pack (a derived copy of this forward, as the fold) is this reader's own
  auto pack_weights = [&](float* pack) {
    SnPackSrc ps;
    const int nb = (int)c->convs.size();
    for (int i = 0; i < nb; ++i) {
      const SnConv& d = *c->convs[i];
      ps.w[i] = c->w[d.w];  ps.K[i] = d.K;  ps.cout[i] = d.cout;  ps.np[i] = d.np;  ps.off[i] = d.pack_off;
    }
    hipLaunchKernelGGL(lipsn_pack_kernel, dim3(64, nb), dim3(256), 0, st, ps, pack);
    HANDLE_LAUNCH_CHECK(c, "lipsn pack");
    return LIPSN_OK;
  };
  if (int rc = lf_front(c, LfVideo{x, S, T, Hin, Win, y0, x0, H, W, a, b}, out, p,
                        [&](SnPlan& q) { return sn_make_plan(c, S, T, H, W, q); }, ws, ws_bytes, st, pack_weights))
    return rc;
  char* base = static_cast<char*>(ws);
  const float* fold = reinterpret_cast<float*>(base + p.off_fold);
  const float* pack = reinterpret_cast<float*>(base + p.off_pack);
  float* act[2] = {reinterpret_cast<float*>(base + p.off_act[0]), reinterpret_cast<float*>(base + p.off_act[1])};
  const LfSizes& z = p.z;
  const int64_t N = p.N;

  // trunk: block i reads act[i & 1] and writes the other
  int bi = 0;
  for (int s = 0; s < 3; ++s) {
    for (int r = 0; r < SN_REPEATS[s]; ++r, ++bi) {
      const SnBlock& B = c->blocks[bi];
      SnBlockArgs ba;
      ba.in = act[bi & 1];  ba.out = act[(bi + 1) & 1];
      ba.w1 = pack + B.pw1.pack_off;  ba.f1 = fold + B.pw1.fold_off;
      ba.wd = pack + B.dw.pack_off;  ba.fd = fold + B.dw.fold_off;
      ba.w2 = pack + B.pw2.pack_off;  ba.f2 = fold + B.pw2.fold_off;
      ba.wd1 = ba.fd1 = ba.wp1 = ba.fp1 = nullptr;
      if (B.stride == 2) {
        ba.wd1 = pack + B.dw1.pack_off;  ba.fd1 = fold + B.dw1.fold_off;
        ba.wp1 = pack + B.pwb1.pack_off;  ba.fp1 = fold + B.pwb1.fold_off;
      }
      ba.N = (int)N;
      ba.Hi = B.stride == 2 ? z.h[s] : z.h[s + 1];  ba.Wi = B.stride == 2 ? z.w[s] : z.w[s + 1];
      ba.Ho = z.h[s + 1];  ba.Wo = z.w[s + 1];
      ba.Cin = B.cin;  ba.Ch = B.ch;  ba.Np = B.pw2.np;  ba.stride = B.stride;
      const SnBlockPlan bp = sn_plan_block(B.stride, ba.Hi, ba.Wi, ba.Ho, ba.Wo, B.cin, B.ch);
      ba.band = bp.band;  ba.bands = bp.bands;  ba.G = bp.G;
      ba.ksx = bp.ksx;  ba.ksm = bp.ksm;  ba.ksd = bp.ksd;  ba.offM = bp.offM;  ba.offD = bp.offD;
      if (bp.lds_floats > SN_BLOCK_LDS_FLOATS)
        return c->fail(LIPSN_ERR_INVALID, "block %d: a one-row tile needs %d floats of LDS", bi, bp.lds_floats);
      const int64_t wgs = (N + bp.G - 1) / bp.G * bp.bands;
      hipLaunchKernelGGL(lipsn_block_kernel, dim3((unsigned)wgs), dim3(256), (size_t)bp.lds_floats * 4, st, ba);
      HANDLE_LAUNCH_CHECK(c, "lipsn block");
    }
  }
  const int Cl = c->last.K;
  hipLaunchKernelGGL(lipsn_last_kernel, dim3((unsigned)((N + SN_LAST_G - 1) / SN_LAST_G)), dim3(256), sn_last_lds_bytes(Cl), st,
                     (const float*)act[bi & 1], (const float*)(pack + c->last.pack_off), (const float*)(fold + c->last.fold_off), out,
                     (int)N, z.h[3], z.w[3], Cl, Cl | 1);
  HANDLE_LAUNCH_CHECK(c, "lipsn conv_last");
  return LIPSN_OK;
}

int lipsn_launches_per_forward(void) { return SN_LAUNCHES; }

double lipsn_flops_per_stream(int width_x2, int T, int H, int W) {
  if ((width_x2 != 1 && width_x2 != 2) || sn_check_shape(1, T, H, W)) return 0.0;
  return 2.0 * T * sn_macs_per_frame(width_x2, H, W);
}

double lipsn_min_bytes_per_stream(int width_x2, int T, int H, int W) {
  if ((width_x2 != 1 && width_x2 != 2) || sn_check_shape(1, T, H, W)) return 0.0;
  // floats per frame that the launches read + write once each when nothing stays cached between them
  const LfSizes z = sizes_of(H, W);
  const int* stages = SN_STAGES[width_x2 - 1];
  double f = (double)H * W + 2.0 * z.Hs * z.Ws * SN_STEM_C + (double)z.h[0] * z.w[0] * SN_STEM_C;   // stem in, pre out + in, pool out
  int inp = SN_STEM_C;
  for (int s = 0; s < 3; ++s) {
    const double o = (double)z.h[s + 1] * z.w[s + 1] * stages[s];
    f += (double)z.h[s] * z.w[s] * inp + o + (SN_REPEATS[s] - 1) * 2.0 * o;
    inp = stages[s];
  }
  f += 9.0 * inp + SN_LAST_N;   // conv_last reads rows / columns 0..2
  return 4.0 * T * f;
}

size_t lipsn_weight_pack_bytes(lipsn_handle h) {
  if (!h) return 0;
  size_t src = 0;
  for (const SnConv* d : h->convs) src += (size_t)d->cout * d->K + 4 * (size_t)d->cout;
  return (src + (size_t)h->pack_floats + h->fold_floats) * 4;
}

}  // extern "C"
