// lipfront.h -- what the two lip readers (lipfe.hip: ResNet-18, lipsn.hip: ShuffleNet-v2) share: the front of the network up
// to the trunk.  Device side: eval-mode BatchNorm folded to scale / shift, the Conv3d stem for C channels and the max-pool
// behind it; the __global__ instantiations are in lipfe_kernels.h (C = 64) and lipsn_kernels.h (C = 24).  Host side: the
// context base, the map sizes, the head of the workspace plan (fold | pack | pre) and lf_front, which checks a forward's
// arguments and runs fold, the reader's own weight pack, stem and max-pool.
//
// Activations are channel-last: [frame n = s*T + t][y][x][C].
#pragma once
#include "common.h"
#include "handle.h"

namespace {

constexpr int LF_ACT_NONE = -1, LF_ACT_RELU = 0, LF_ACT_PRELU = 1, LF_ACT_SWISH = 2;
constexpr int LF_MAX_BNS = 64;     // lipfe folds 20 BatchNorms, lipsn 56
constexpr float LF_BN_EPS = 1e-5f;

DEV float lf_act(float v, int act, float slope) {
  if (act == LF_ACT_RELU) return fmaxf(v, 0.f);
  if (act == LF_ACT_PRELU) return v >= 0.f ? v : slope * v;
  if (act == LF_ACT_SWISH) return v * (1.0f / (1.0f + expf(-v)));
  return v;
}

// ------------------------------------------------------------------------------------------------
// eval-mode BatchNorm -> scale = w / sqrt(var + eps), shift = b - mean * scale; a derived copy, made in every forward
// ------------------------------------------------------------------------------------------------
struct LfFoldSrc {
  const float* w[LF_MAX_BNS];   // weight, bias, running_mean, running_var
  const float* b[LF_MAX_BNS];
  const float* m[LF_MAX_BNS];
  const float* v[LF_MAX_BNS];
  int C[LF_MAX_BNS];
  int off[LF_MAX_BNS];          // floats into the fold buffer: scale[C] then shift[C]
};

// grid (n_bn), block 256
DEV void lf_fold(const LfFoldSrc& s, float* __restrict__ fold) {
  const int i = blockIdx.x, C = s.C[i];
  float* scale = fold + s.off[i];
  float* shift = scale + C;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float sc = s.w[i][c] / sqrtf(s.v[i][c] + LF_BN_EPS);
    scale[c] = sc;
    shift[c] = s.b[i][c] - s.m[i][c] * sc;
  }
}

// ------------------------------------------------------------------------------------------------
// stem: Conv3d(1 -> C, (5,7,7), stride (1,2,2), pad (2,3,3)) + BN + activation  ->  pre [N][Hs][Ws][C]
// ------------------------------------------------------------------------------------------------
constexpr int LF_STX = 16, LF_STY = 4;                  // output tile of one workgroup
constexpr int LF_PR = 2 * LF_STY + 5, LF_PC = 40;       // input patch rows, padded row length (37 used)

struct LfStemArgs {
  const float* x;        // [S][T][Hin][Win]
  const float* wpk;      // [245][CP]
  const float* scale;    // folded BN: scale[C], shift[C] behind it
  const float* slope;    // PReLU slopes or NULL
  float* pre;
  int T, Hin, Win, y0, x0, H, W, Hs, Ws, tiles_x, tiles_y, act;
  float a, b;
};

// grid (tiles_x * tiles_y * N), block 256: wave g computes row g of the tile.  A group of CP lanes (a power of two, C <= CP
// <= 64) takes the channels, the wave's XH = 64 / CP groups split the row's 16 x positions: thread = (channel, x part, row),
// NX positions each.  Lanes C .. CP - 1 of a group compute on the zero columns of wpk and store nothing.
template <int C, int CP>
DEV void lf_stem(const LfStemArgs p) {
  constexpr int XH = 64 / CP, NX = LF_STX / XH, RW = (2 * NX + 5 + 3) & ~3;   // RW: the patch columns a thread reads
  constexpr int LOG_CP = CP == 64 ? 6 : 5;
  static_assert(CP == 1 << LOG_CP && C <= CP && 2 * NX * (XH - 1) + RW <= LF_PC, "lane group / row slice");
  __shared__ __attribute__((aligned(16))) float patch[5][LF_PR][LF_PC];
  __shared__ float ws[49][CP];
  const int tid = threadIdx.x, c = tid & (CP - 1), xh = XH == 1 ? 0 : (tid >> LOG_CP) & (XH - 1), g = tid >> 6;
  long long wg = blockIdx.x;
  const int tx = (int)(wg % p.tiles_x);  wg /= p.tiles_x;
  const int ty = (int)(wg % p.tiles_y);  wg /= p.tiles_y;
  const long long n = wg;                  // frame s*T + t
  const int t = (int)(n % p.T);
  const int oy0 = ty * LF_STY, ox0 = tx * LF_STX;
  const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
  for (int i = tid; i < 5 * LF_PR * LF_PC; i += 256) {
    const int col = i % LF_PC, r = (i / LF_PC) % LF_PR, kt = i / (LF_PC * LF_PR);
    const int tt = t + kt - 2, iy = iy0 + r, ix = ix0 + col;
    float v = 0.f;     // padding is zero in the normalised domain
    if (col < 37 && tt >= 0 && tt < p.T && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
      v = fmaf(p.a, p.x[((n + (kt - 2)) * p.Hin + (p.y0 + iy)) * p.Win + (p.x0 + ix)], p.b);
    patch[kt][r][col] = v;
  }
  float tot[NX], acc[NX];             // the 49 taps of a frame are summed on their own, then the five frames
#pragma unroll
  for (int i = 0; i < NX; ++i) tot[i] = 0.f;
  for (int kt = 0; kt < 5; ++kt) {
    __syncthreads();
    for (int i = tid; i < 49 * CP; i += 256) ws[i >> LOG_CP][i & (CP - 1)] = p.wpk[kt * 49 * CP + i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NX; ++i) acc[i] = 0.f;
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
      float row[RW];
      const float4* src = reinterpret_cast<const float4*>(&patch[kt][2 * g + ky][2 * NX * xh]);
#pragma unroll
      for (int i = 0; i < RW / 4; ++i) {
        const float4 q = src[i];
        row[4 * i] = q.x;  row[4 * i + 1] = q.y;  row[4 * i + 2] = q.z;  row[4 * i + 3] = q.w;
      }
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const float w = ws[ky * 7 + kx][c];
#pragma unroll
        for (int i = 0; i < NX; ++i) acc[i] = fmaf(row[2 * i + kx], w, acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) tot[i] += acc[i];
  }
  const int oy = oy0 + g;
  if (oy >= p.Hs) return;
  if constexpr (C < CP) { if (c >= C) return; }
  const float sc = p.scale[c], sh = p.scale[C + c], sl = p.slope ? p.slope[c] : 0.f;
  const int oxb = ox0 + NX * xh;
  float* out = p.pre + ((n * p.Hs + oy) * p.Ws + oxb) * C + c;
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (oxb + i < p.Ws) out[(long long)i * C] = lf_act(fmaf(tot[i], sc, sh), p.act, sl);
}

// MaxPool (3,3) stride 2 pad 1 over [N][Hs][Ws][C] -> [N][Hp][Wp][C]; the padding is -inf, i.e. left out of the maximum.
// One thread per 4 channels of an output position: total4 = N * Hp * Wp * C / 4, block 256.
template <int C>
DEV void lf_maxpool(const float* __restrict__ pre, float* __restrict__ out, long long total4, int Hs, int Ws, int Hp, int Wp) {
  constexpr int C4 = C / 4;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c4 = (int)(i % C4);
  long long pos = i / C4;
  const int px = (int)(pos % Wp);  pos /= Wp;
  const int py = (int)(pos % Hp);
  const long long n = pos / Hp;
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  for (int dy = -1; dy <= 1; ++dy) {
    const int y = 2 * py + dy;
    if (y < 0 || y >= Hs) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int x = 2 * px + dx;
      if (x < 0 || x >= Ws) continue;
      const float4 v = ldg4(pre + ((n * Hs + y) * Ws + x) * C + 4 * c4);
      m.x = fmaxf(m.x, v.x);  m.y = fmaxf(m.y, v.y);  m.z = fmaxf(m.z, v.z);  m.w = fmaxf(m.w, v.w);
    }
  }
  *reinterpret_cast<float4*>(out + i * 4) = m;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct LfSizes {
  int Hs, Ws, h[4], w[4];           // after the stem conv; after the pool and in the trunk's three later stages
};

inline LfSizes sizes_of(int H, int W) {
  LfSizes z;
  z.Hs = (H - 1) / 2 + 1;  z.Ws = (W - 1) / 2 + 1;
  z.h[0] = (z.Hs - 1) / 2 + 1;  z.w[0] = (z.Ws - 1) / 2 + 1;
  for (int l = 1; l < 4; ++l) { z.h[l] = (z.h[l - 1] - 1) / 2 + 1;  z.w[l] = (z.w[l - 1] - 1) / 2 + 1; }
  return z;
}

// what differs between the two readers' fronts
struct LfModel {
  const char* name;        // "lipfe" / "lipsn": in front of the launch names, and names *_bind_weights
  int C;                   // stem channels
  int64_t max_pos;         // the largest S*T*Hs*Ws its kernels' index arithmetic holds ...
  const char* limit;       // ... and what the refusal calls it
  void (*fold)(LfFoldSrc, float*);
  void (*stem)(LfStemArgs);
  void (*maxpool)(const float*, float*, long long, int, int, int, int);
};

struct LfCtx : Handle {
  const LfModel* model = nullptr;
  int act = LF_ACT_SWISH;           // the public headers' *_RELU / *_PRELU / *_SWISH are LF_ACT_*
  struct Bn { int bn, C, off; };    // table index of bn.weight, channels, floats into the fold buffer
  std::vector<Bn> bns;              // every BatchNorm: the fold jobs
  int64_t pack_floats = 0;
  int fold_floats = 0;
  int64_t stem_pack_off = 0;        // the stem's weights in the pack buffer, its BatchNorm in the fold buffer, its PReLU
  int stem_fold_off = 0, stem_slope = -1;   // slopes' table index or -1: set by the reader's table builder
  // the BatchNorm `p`* of C channels: four table entries and a fold job.  Returns the index of p.weight.
  int add_bn(const std::string& p, int C, int& fold_off) {
    const int i = add(p + "weight", C);
    add(p + "bias", C);  add(p + "running_mean", C);  add(p + "running_var", C);
    fold_off = fold_floats;  fold_floats += 2 * C;
    bns.push_back(Bn{i, C, fold_off});
    return i;
  }
};

struct LfPlan {
  LfSizes z;
  int64_t N;
  size_t off_fold, off_pack, off_pre, total;
};

// the head of both plans.  `why`: the reader's own verdict on S, T, H, W (NULL: supported); the reader takes its activation
// buffers from `cur` next.
inline int lf_plan_head(LfCtx* c, const char* why, int S, int T, int H, int W, LfPlan& p, ByteCursor& cur) {
  if (why) return c->fail(H_ERR_INVALID, "%s (got S=%d T=%d H=%d W=%d)", why, S, T, H, W);
  p.z = sizes_of(H, W);
  p.N = (int64_t)S * T;
  const int64_t pos = p.N * p.z.Hs * p.z.Ws;
  if (pos > c->model->max_pos)
    return c->fail(H_ERR_INVALID, "S*T*Hs*Ws = %lld exceeds %s (S=%d T=%d H=%d W=%d)", (long long)pos, c->model->limit, S, T, H, W);
  p.off_fold = cur.take((size_t)c->fold_floats * 4);
  p.off_pack = cur.take((size_t)c->pack_floats * 4);
  p.off_pre = cur.take((size_t)pos * c->model->C * 4);
  return H_OK;
}

struct LfVideo {            // *_forward's view of the input: the H x W window at (y0, x0) of [S][T][Hin][Win], a * x + b on load
  const float* x;
  int S, T, Hin, Win, y0, x0, H, W;
  float a, b;
};

// The front of *_forward: refuses what cannot run (in the order bound, NULL, shape, window, workspace), then launches fold,
// the reader's pack(pack buffer) and stem + max-pool -> act0 = [N][h0][w0][C].  make_plan(p) is the reader's own plan.
template <class Plan, class MakePlan, class Pack>
int lf_front(LfCtx* c, const LfVideo& v, const float* out, Plan& p, MakePlan&& make_plan, void* ws, size_t ws_bytes,
             hipStream_t st, Pack&& pack) {
  const LfModel& m = *c->model;
  if (!c->bound) return c->fail(H_ERR_WEIGHTS, "weights not bound (%s_bind_weights)", m.name);
  if (!v.x || !out) return c->fail(H_ERR_INVALID, "x / out must not be NULL");
  if (int rc = make_plan(p)) return rc;
  if (v.y0 < 0 || v.x0 < 0 || (int64_t)v.y0 + v.H > v.Hin || (int64_t)v.x0 + v.W > v.Win)
    return c->fail(H_ERR_INVALID, "window %d x %d at (%d, %d) does not lie inside the %d x %d frame", v.H, v.W, v.y0, v.x0, v.Hin,
                   v.Win);
  if (int rc = check_workspace(c, p.total, ws, ws_bytes)) return rc;
  char* base = static_cast<char*>(ws);
  float* fold = reinterpret_cast<float*>(base + p.off_fold);
  float* packed = reinterpret_cast<float*>(base + p.off_pack);
  float* pre = reinterpret_cast<float*>(base + p.off_pre);
  float* act0 = reinterpret_cast<float*>(base + p.off_act[0]);
  const auto& Wt = c->w;
  const LfSizes& z = p.z;

  LfFoldSrc fs;
  const int nb = (int)c->bns.size();
  for (int i = 0; i < nb; ++i) {
    const LfCtx::Bn& d = c->bns[i];
    fs.w[i] = Wt[d.bn];  fs.b[i] = Wt[d.bn + 1];  fs.m[i] = Wt[d.bn + 2];  fs.v[i] = Wt[d.bn + 3];
    fs.C[i] = d.C;  fs.off[i] = d.off;
  }
  hipLaunchKernelGGL(m.fold, dim3(nb), dim3(256), 0, st, fs, fold);
  HANDLE_LAUNCH_CHECK(c, (std::string(m.name) + " fold").c_str());
  if (int rc = pack(packed)) return rc;

  LfStemArgs sa;
  sa.x = v.x;  sa.wpk = packed + c->stem_pack_off;  sa.scale = fold + c->stem_fold_off;
  sa.slope = c->stem_slope >= 0 ? Wt[c->stem_slope] : nullptr;
  sa.pre = pre;
  sa.T = v.T;  sa.Hin = v.Hin;  sa.Win = v.Win;  sa.y0 = v.y0;  sa.x0 = v.x0;  sa.H = v.H;  sa.W = v.W;  sa.Hs = z.Hs;  sa.Ws = z.Ws;
  sa.tiles_x = (z.Ws + LF_STX - 1) / LF_STX;  sa.tiles_y = (z.Hs + LF_STY - 1) / LF_STY;
  sa.act = c->act;  sa.a = v.a;  sa.b = v.b;
  const int64_t stem_wgs = p.N * sa.tiles_x * sa.tiles_y;   // <= N * Hs * Ws <= max_pos <= INT32_MAX
  hipLaunchKernelGGL(m.stem, dim3((unsigned)stem_wgs), dim3(256), 0, st, sa);
  HANDLE_LAUNCH_CHECK(c, (std::string(m.name) + " stem").c_str());
  const int64_t pool4 = p.N * z.h[0] * z.w[0] * (m.C / 4);
  hipLaunchKernelGGL(m.maxpool, dim3((unsigned)((pool4 + 255) / 256)), dim3(256), 0, st, (const float*)pre, act0, (long long)pool4,
                     z.Hs, z.Ws, z.h[0], z.w[0]);
  HANDLE_LAUNCH_CHECK(c, (std::string(m.name) + " maxpool").c_str());
  return H_OK;
}

}  // namespace
