// lipfe.hip -- the lip-reading front end (src/lipreader/lipreading/model.py:141-273 with extract_feats = True: Conv3d stem
// + ResNet-18 trunk, mouth video -> 512-wide embeddings per frame) for gfx950: handle and the extern "C" boundary declared
// in include/lipfe.h; the kernels are in lipfe_kernels.h.  The handle's scaffolding is handle.h's; everything up to the trunk
// (argument checks, the head of the workspace plan, fold, stem, max-pool) is lipfront.h's, shared with lipsn.hip.
//
// One forward is 24 launches, all on the caller's stream:
//   fold      the 20 eval-mode BatchNorms -> scale = w / sqrt(var + eps), shift = b - mean * scale        (1 launch)
//   pack      the 20 conv weights [Cout][Cin][taps] -> [tap][Cin][Cout], the order the GEMM's B loader reads (1 launch)
//   stem      Conv3d + BN + act on plain VALU (Cin = 1: K = 245 is no MFMA shape), window and affine applied on load
//   maxpool   3 x 3 / 2, -inf padding.  Stem and pool are TWO launches: the pre-pool map [N][Hs][Ws][64] makes one round
//             trip through memory (49.6 MB written and read at S = 2, T = 50, 88 x 88)
//   trunk     8 BasicBlocks = 16 3x3 convs + 3 1x1 stride-2 downsample convs, each one launch of the implicit-GEMM kernel
//             with BN, residual add and activation in its epilogue                                          (19 launches)
//   avgpool   mean over the final map                                                                      (1 launch)
// The derived copies (fold, pack) are made in every forward, into the workspace: a copy made at bind time would go stale
// when load_state_dict copies into the same storages.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lipfe.h"
#include "lipfe_kernels.h"

HANDLE_ASSERT_CODES(LIPFE);
static_assert(LIPFE_RELU == LF_ACT_RELU && LIPFE_PRELU == LF_ACT_PRELU && LIPFE_SWISH == LF_ACT_SWISH, "relu_type is LF_ACT_*");

namespace {
thread_local std::string g_create_error;

struct ConvDesc {
  int w, bn, slope;                 // weight-table indices: conv weight, bn.weight (bias, mean, var follow), slope or -1
  int cin, cout, taps, stride;
  int64_t pack_off;                 // floats into the pack buffer
  int fold_off;                     // floats into the fold buffer
};

const int PLANES[4] = {64, 128, 256, 512};

struct Plan : LfPlan {
  size_t off_act[4];
};

const LfModel LIPFE_MODEL = {"lipfe", 64, INT32_MAX, "32-bit indexing", lipfe_fold_kernel, lipfe_stem_kernel, lipfe_maxpool_kernel};
}  // namespace

struct lipfe_ctx : LfCtx {
  ConvDesc stem;
  ConvDesc conv1[8], conv2[8], down[4];   // down[l]: first block of layer l (l >= 1)
  lipfe_ctx() { model = &LIPFE_MODEL; }
  // conv `d`'s BatchNorm `p`* and its place in the pack buffer
  void place(ConvDesc& d, const std::string& p) {
    d.bn = add_bn(p, d.cout, d.fold_off);
    d.pack_off = pack_floats;  pack_floats += (int64_t)d.cout * d.cin * d.taps;
  }
};

namespace {
// the reference's state_dict() order without tcn.* and num_batches_tracked: the trunk is registered before the stem
void build_table(lipfe_ctx* c) {
  const bool prelu = c->act == LIPFE_PRELU;
  int inp = 64;
  for (int l = 0; l < 4; ++l) {
    const int P = PLANES[l];
    for (int b = 0; b < 2; ++b) {
      const std::string p = "trunk.layer" + std::to_string(l + 1) + "." + std::to_string(b) + ".";
      const int cin = b == 0 ? inp : P;
      const bool ds = b == 0 && l > 0;
      ConvDesc& c1 = c->conv1[2 * l + b];
      ConvDesc& c2 = c->conv2[2 * l + b];
      c1 = ConvDesc{c->add(p + "conv1.weight", (int64_t)P * cin * 9), 0, -1, cin, P, 9, ds ? 2 : 1, 0, 0};
      c->place(c1, p + "bn1.");
      int s1 = -1, s2 = -1;
      if (prelu) { s1 = c->add(p + "relu1.weight", P);  s2 = c->add(p + "relu2.weight", P); }
      c1.slope = s1;
      c2 = ConvDesc{c->add(p + "conv2.weight", (int64_t)P * P * 9), 0, s2, P, P, 9, 1, 0, 0};
      c->place(c2, p + "bn2.");
      if (ds) {
        ConvDesc& d = c->down[l];
        d = ConvDesc{c->add(p + "downsample.0.weight", (int64_t)P * cin), 0, -1, cin, P, 1, 2, 0, 0};
        c->place(d, p + "downsample.1.");
      }
    }
    inp = P;
  }
  c->stem = ConvDesc{c->add("frontend3D.0.weight", 64 * 245), 0, -1, 1, 64, 245, 2, 0, 0};
  c->place(c->stem, "frontend3D.1.");
  if (prelu) c->stem.slope = c->add("frontend3D.2.weight", 64);
  c->stem_pack_off = c->stem.pack_off;  c->stem_fold_off = c->stem.fold_off;  c->stem_slope = c->stem.slope;
  c->w.assign(c->names.size(), nullptr);
}

template <class F>
void for_each_conv(lipfe_ctx* c, F&& f) {
  for (int i = 0; i < 8; ++i) {
    f(c->conv1[i]);  f(c->conv2[i]);
    if ((i & 1) == 0 && i > 0) f(c->down[i / 2]);
  }
  f(c->stem);
}

const char* check_shape(int S, int T, int H, int W) {
  if (S < 1) return "S must be >= 1";
  if (T < 1) return "T must be >= 1";
  if (H < 8 || H > 256 || W < 8 || W > 256) return "H and W must be in [8, 256]";
  return nullptr;
}

int make_plan(lipfe_ctx* c, int S, int T, int H, int W, Plan& p) {
  ByteCursor cur;
  if (int rc = lf_plan_head(c, check_shape(S, T, H, W), S, T, H, W, p, cur)) return rc;
  size_t act = 0;
  for (int l = 0; l < 4; ++l) {
    const size_t a = (size_t)p.z.h[l] * p.z.w[l] * PLANES[l];
    if (a > act) act = a;
  }
  for (int i = 0; i < 4; ++i) p.off_act[i] = cur.take((size_t)p.N * act * 4);
  p.total = cur.o;
  return LIPFE_OK;
}

int launch_conv(lipfe_ctx* c, hipStream_t st, const ConvDesc& d, const float* fold, const float* pack, const float* in,
                const float* res, float* out, int64_t N, int Hi, int Wi, int Ho, int Wo, int act) {
  LfConvArgs a;
  a.in = in;  a.wpk = pack + d.pack_off;  a.scale = fold + d.fold_off;
  a.slope = d.slope >= 0 ? c->w[d.slope] : nullptr;
  a.res = res;  a.out = out;
  a.M = N * Ho * Wo;
  a.Hi = Hi;  a.Wi = Wi;  a.Ho = Ho;  a.Wo = Wo;  a.Cin = d.cin;  a.Cout = d.cout;  a.stride = d.stride;  a.act = act;  a.dil = 1;
  const dim3 grid((unsigned)((a.M + LF_BM - 1) / LF_BM), (unsigned)(d.cout / LF_BN));
  if (d.taps == 9) hipLaunchKernelGGL((lipfe_conv_kernel<3, 3>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((lipfe_conv_kernel<1, 1>), grid, dim3(256), 0, st, a);
  HANDLE_LAUNCH_CHECK(c, "lipfe conv");
  return LIPFE_OK;
}

double conv_macs_per_frame(int H, int W) {
  const LfSizes z = sizes_of(H, W);
  double macs = (double)z.Hs * z.Ws * 64 * 245;
  int inp = 64;
  for (int l = 0; l < 4; ++l) {
    const double pos = (double)z.h[l] * z.w[l];
    if (l > 0) macs += pos * PLANES[l] * inp;
    macs += pos * PLANES[l] * 9.0 * (inp + 3.0 * PLANES[l]);
    inp = PLANES[l];
  }
  return macs;
}
}  // namespace

extern "C" {

int lipfe_abi_version(void) { return LIPFE_ABI_VERSION; }

int lipfe_create(lipfe_handle* out, int relu_type) {
  if (out && relu_type != LIPFE_RELU && relu_type != LIPFE_PRELU && relu_type != LIPFE_SWISH)
    return refuse_create(out, g_create_error,
                         "relu_type must be LIPFE_RELU, LIPFE_PRELU or LIPFE_SWISH (got " + std::to_string(relu_type) + ")");
  if (int rc = create(out, "lip-reading front end", g_create_error)) return rc;
  (*out)->act = relu_type;
  build_table(*out);
  return LIPFE_OK;
}

void lipfe_destroy(lipfe_handle h) { delete h; }

const char* lipfe_last_error(lipfe_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int lipfe_num_weights(lipfe_handle h) { return h ? (int)h->names.size() : 0; }

const char* lipfe_weight_name(lipfe_handle h, int i) { return h ? h->weight_name(i) : nullptr; }

int64_t lipfe_weight_numel(lipfe_handle h, int i) { return h ? h->weight_numel(i) : -1; }

int lipfe_bind_weights(lipfe_handle h, const float* const* dev_ptrs, int n) {
  return h ? bind_weights(h, dev_ptrs, n, 4) : LIPFE_ERR_INVALID;
}

size_t lipfe_workspace_bytes(lipfe_handle h, int S, int T, int H, int W) {
  if (!h) return 0;
  Plan p;
  if (make_plan(h, S, T, H, W, p)) return 0;
  return p.total;
}

int lipfe_forward(lipfe_handle h, const float* x, int S, int T, int Hin, int Win, int y0, int x0, int H, int W, float a, float b,
                  float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return LIPFE_ERR_INVALID;
  lipfe_ctx* c = h;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Plan p;
  // the front: act[0] = [N][h0][w0][64]; the pack (a derived copy of this forward, as the fold) is this reader's own
  auto pack_weights = [&](float* pack) {
    LfPackSrc ps;
    int nb = 0;
    for_each_conv(c, [&](const ConvDesc& d) {
      ps.w[nb] = c->w[d.w];  ps.cin[nb] = d.cin;  ps.cout[nb] = d.cout;  ps.taps[nb] = d.taps;  ps.off[nb] = d.pack_off;
      ++nb;
    });
    hipLaunchKernelGGL(lipfe_pack_kernel, dim3(512, nb), dim3(256), 0, st, ps, pack);
    HANDLE_LAUNCH_CHECK(c, "lipfe pack");
    return LIPFE_OK;
  };
  if (int rc = lf_front(c, LfVideo{x, S, T, Hin, Win, y0, x0, H, W, a, b}, out, p,
                        [&](Plan& q) { return make_plan(c, S, T, H, W, q); }, ws, ws_bytes, st, pack_weights))
    return rc;
  char* base = static_cast<char*>(ws);
  const float* fold = reinterpret_cast<float*>(base + p.off_fold);
  const float* pack = reinterpret_cast<float*>(base + p.off_pack);
  float* act[4];
  for (int i = 0; i < 4; ++i) act[i] = reinterpret_cast<float*>(base + p.off_act[i]);
  const LfSizes& z = p.z;
  const int64_t N = p.N;

  // trunk: the block's input is act[cur]; mid, the downsampled residual and the output take the other three buffers
  int cur = 0;
  for (int i = 0; i < 8; ++i) {
    const int l = i / 2;
    const bool ds = (i & 1) == 0 && l > 0;
    const int Hi = ds ? z.h[l - 1] : z.h[l], Wi = ds ? z.w[l - 1] : z.w[l];
    float* in = act[cur];
    float* mid = act[(cur + 1) & 3];
    float* resb = act[(cur + 2) & 3];
    float* outb = act[(cur + 3) & 3];
    if (int rc = launch_conv(c, st, c->conv1[i], fold, pack, in, nullptr, mid, N, Hi, Wi, z.h[l], z.w[l], c->act)) return rc;
    const float* res = in;
    if (ds) {
      if (int rc = launch_conv(c, st, c->down[l], fold, pack, in, nullptr, resb, N, Hi, Wi, z.h[l], z.w[l], LF_ACT_NONE)) return rc;
      res = resb;
    }
    if (int rc = launch_conv(c, st, c->conv2[i], fold, pack, mid, res, outb, N, z.h[l], z.w[l], z.h[l], z.w[l], c->act)) return rc;
    cur = (cur + 3) & 3;
  }
  const int64_t total = N * 512;
  hipLaunchKernelGGL(lipfe_avgpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, act[cur], out, (long long)total,
                     z.h[3] * z.w[3]);
  HANDLE_LAUNCH_CHECK(c, "lipfe avgpool");
  return LIPFE_OK;
}

double lipfe_flops_per_stream(int T, int H, int W) {
  if (check_shape(1, T, H, W)) return 0.0;
  return 2.0 * T * conv_macs_per_frame(H, W);
}

double lipfe_min_bytes_per_stream(int T, int H, int W) {
  if (check_shape(1, T, H, W)) return 0.0;
  // floats per frame that the launches read + write once each when nothing stays cached between them
  const LfSizes z = sizes_of(H, W);
  double f = (double)H * W + 2.0 * z.Hs * z.Ws * 64 + (double)z.h[0] * z.w[0] * 64;   // stem in, pre out + in, pool out
  int inp = 64;
  for (int l = 0; l < 4; ++l) {
    const double o = (double)z.h[l] * z.w[l] * PLANES[l];
    const double i = l > 0 ? (double)z.h[l - 1] * z.w[l - 1] * inp : o;
    f += (i + o) + (l > 0 ? i + o : 0.0) + 3.0 * o;   // block 0: conv1, downsample, conv2 (mid + residual in, out)
    f += 2.0 * o + 3.0 * o;                           // block 1
    inp = PLANES[l];
  }
  f += (double)z.h[3] * z.w[3] * 512 + 512;           // avgpool
  return 4.0 * T * f;
}

size_t lipfe_weight_pack_bytes(lipfe_handle h) { return h ? (size_t)2 * ((size_t)h->pack_floats + h->fold_floats) * 4 : 0; }

}  // extern "C"
