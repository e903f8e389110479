// lstm16x.hip -- LSTM recurrence on 16-sequence tiles WITH the input projection inside (num_features = 64), gfx950.
//
// Reference semantics: torch.nn.LSTM(batch_first=True), gate order i, f, g, o (src/model/dptn.py:22-30,
// src/model/dprnn.py:24-47):   gates_t = x_t W_ih^T + b_ih + h_{t-1} W_hh^T + b_hh.
//
// lstm16.hip takes `x_t W_ih^T + b` from HBM (PRE16, written by the K4 GEMM): 2 KiB per token and direction written and
// read again -- for 64 features an 8x expansion of the 256-byte input row, and 80 % of a forward's HBM traffic.  Here the
// pre-activations never exist in memory: one workgroup = one direction x 16 sequences x all positions keeps
//   * W_hh (512 x 128) in the AGPR half of its register file, as lstm16.hip does, and
//   * W_ih (512 x 64 = 128 KiB) in LDS, in MFMA B-fragment order (each wave its own 32 KiB: 8 blocks x 4 k-chunks),
// reads the step's 16 x 64 input rows (4 KiB, one float4 per thread, requested three steps ahead) and accumulates
//   acc = b + x_t W_ih^T  (128 MFMAs per wave, issued at the END of the previous step: they do not depend on h_{t-1})
//   acc += h_{t-1} W_hh^T (256 MFMAs per wave)
// in one chain.  The recurrence gets 50 % more matrix work per step; the K4 launch (as many FLOPs, plus 4 KiB of stores per
// token) disappears.  Fragment maps, cell update and the h exchange are lstm16.hip's (v_mfma_f32_16x16x4_f32:
// lane l: i16 = l & 15, ks = l >> 4; A[i16][ks], B[ks][i16], D reg r = (row 4ks + r, col i16); MFMA step 4m+t uses true
// k = 16m + 4ks + t).  Compiled with -mllvm -amdgpu-mfma-vgpr-form (build.py).
#include <hip/hip_runtime.h>

#include "lstm16.h"
#include "vmem_asm.h"

namespace {

template <int NIN>
struct X16 {
  static constexpr int MK = NIN / 16;                   // k-chunks of the input projection
  static constexpr int LDX = NIN + 8;                   // input rows in LDS: conflict-free ds_read_b128 for the 16x16x4 A map
  static constexpr int WL_FLOATS = 4 * MK * 8 * 256;    // [wave][m][block][lane][4]
  static constexpr int XS_FLOATS = 2 * 16 * LDX;        // two steps of input rows
  static constexpr int NXL = (16 * NIN / 4) / 256;      // float4 of an input tile per thread
  static constexpr size_t LDS_BYTES = sizeof(float) * (WL_FLOATS + L16_HS_FLOATS + XS_FLOATS);
  static_assert((16 * NIN / 4) % 256 == 0 && NIN % 16 == 0, "input tile / threads");
  static_assert(LDS_BYTES <= 160 * 1024, "W_ih must fit the LDS beside the h and x tiles");
};

// Fragment-order copy of one direction's weights, written by lstm16x_pack_kernel from the weights as they are at that moment and
// read by the PRO = 1 prologues: per wave `SETS` sets of 1 KiB ([lane 64][4 floats], one wave instruction each), every value
// already multiplied by l16_gate_scale of its gate (the multiply the PRO = 0 prologue does itself: the same bits).
//   sets [0, HH0):      W_ih set p = 8 m + b:  W_ih[row(b)][16 m + 4 ks .. + 3]      row(b) = (b >> 1) 128 + 32 wave + 16 (b & 1) + i16
//   sets [HH0, BIAS0):  W_hh set q = 8 b + m:  W_hh[row(b)][16 m + 4 ks .. + 3]
//   sets BIAS0 + j:     (b_ih + b_hh)[row(4 j + k)], k = 0..3
template <int NIN>
struct XPack {
  static constexpr int HH0 = 8 * (NIN / 16), BIAS0 = HH0 + 64, SETS = BIAS0 + 2;
  static constexpr size_t DIR_FLOATS = (size_t)4 * SETS * 256;
  static_assert(DIR_FLOATS == lstm16x_pack_floats(NIN), "lstm16.h");
};

// PRO: the prologue.  0 = every lane reads its rows of the nn.LSTM tensors with ordinary loads and scales them (the compiler
// serialises them: 44 blocking load groups, 80 in the 128-feature kernel); 1 = one burst of hand-issued 1-KiB requests from the
// packed copy, W_ih to LDS by LDS-DMA, W_hh straight into its AGPRs, one wait.  Same values in the same registers either way.
template <int NIN, bool RELU, int PRO>
DEV void lstm16x_body(const float* __restrict__ x, int ldx, const float* __restrict__ wih_f,
                      const float* __restrict__ wih_b, const float* __restrict__ bih_f,
                      const float* __restrict__ bih_b, const float* __restrict__ bhh_f,
                      const float* __restrict__ bhh_b, const float* __restrict__ whh_f,
                      const float* __restrict__ whh_b, const float* __restrict__ pk, float* __restrict__ hc, int ldh,
                      int64_t dump_row, SeqGeom g) {
  using Sh = X16<NIN>;
  constexpr int MK = Sh::MK, LDX = Sh::LDX, NXL = Sh::NXL;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Wl = smem;                               // [4][MK][8][256]
  float* Hs = smem + Sh::WL_FLOATS;               // [2][16][L16_LDH]
  float* Xs = Hs + L16_HS_FLOATS;                 // [2][16][LDX]
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, i16 = lane & 15, ks = lane >> 4;
  const int st = blockIdx.x, d = blockIdx.y;
  const float* whh = d ? whh_b : whh_f;
  const float* wih = d ? wih_b : wih_f;
  const float* bih = d ? bih_b : bih_f;
  const float* bhh = d ? bhh_b : bhh_f;

  // ---- W_hh -> AGPRs (B fragments of the recurrent product), pre-scaled for the exp2 forms of sigmoid / tanh ----------
  float wf[8][32];
  float bsc[8];                                   // (b_ih + b_hh) of the lane's column in block b, pre-scaled
  float* wl_wave = Wl + w * (MK * 8 * 256) + lane * 4;
  f32x4 wq[64], bq[2];                            // PRO = 1: W_hh set q = 8 b + m, the bias of blocks 0..3 / 4..7, in flight
  if constexpr (PRO == 0) {
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int row = (b >> 1) * L16_H + 32 * w + 16 * (b & 1) + i16;
      const float gs = l16_gate_scale(b >> 1);
      const float* wrow = whh + (int64_t)row * L16_H + 4 * ks;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const float4 v = *reinterpret_cast<const float4*>(wrow + 16 * m);
        wf[b][4 * m + 0] = v.x * gs;
        wf[b][4 * m + 1] = v.y * gs;
        wf[b][4 * m + 2] = v.z * gs;
        wf[b][4 * m + 3] = v.w * gs;
      }
      bsc[b] = (bih[row] + bhh[row]) * gs;
      // ---- W_ih -> LDS, the same fragment map (this lane writes exactly what it will read) ----------------------------------
      const float* irow = wih + (int64_t)row * NIN + 4 * ks;
#pragma unroll
      for (int m = 0; m < MK; ++m) {
        const float4 v = *reinterpret_cast<const float4*>(irow + 16 * m);
        *reinterpret_cast<float4*>(wl_wave + (m * 8 + b) * 256) = make_float4(v.x * gs, v.y * gs, v.z * gs, v.w * gs);
      }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int i = 0; i < 32; ++i) asm volatile("" : "+a"(wf[b][i]));
  } else {
    // One burst, oldest first: W_ih (this wave's 32 KiB of LDS, set by set), the bias, W_hh.  Everything the compiler counts in
    // this kernel (the input rows' loads, the h row stores) is issued behind the burst, so its own waits cover the burst as well;
    // the one wait written by hand is vmcnt(0), in front of the first barrier.
    using P = XPack<NIN>;
    const char* pw = reinterpret_cast<const char*>(pk) + (size_t)(d * 4 + w) * (P::SETS * 1024);
    const uint32_t lane16 = (uint32_t)lane * 16u;
    const uint32_t wl_lds = lds_addr(Wl + w * (MK * 8 * 256));
    static_for<8 * MK>([&](auto PP) {
      constexpr int p = decltype(PP)::value;
      dma_part<false>(pw + p * 1024, lane16, wl_lds + p * 1024);
    });
    ldg4_uncounted<0>(bq[0], pw + P::BIAS0 * 1024, lane16);
    ldg4_uncounted<1024>(bq[1], pw + P::BIAS0 * 1024, lane16);
    static_for<64>([&](auto Q) {
      constexpr int q = decltype(Q)::value;
      ldg4_uncounted_a<(q & 3) * 1024>(wq[q], pw + (P::HH0 + (q & ~3)) * 1024, lane16);
    });
  }

  const int t0 = d ? g.len - 1 : 0, tdir = d ? -1 : 1;
  const int tstride = seq_token_stride(g);
  // ---- h rows leave through the LDS tile (lstm16.hip): wave w stores tile rows 4w + 2j + (lane >> 5), 16 bytes at column
  // 4 (lane & 31).  Rows of padded sequences walk through the dump rows.  64-bit addresses: a DPRNN launch of 16 mixtures
  // x 8 s is 4 M tokens x 1 KiB.
  const int srow = 4 * w + (lane >> 5), scol = 4 * (lane & 31);
  char* hp[2];
  const int64_t hstep = (int64_t)tdir * tstride * ldh * 4;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = st * 16 + srow + 2 * j;
    const int64_t tokb = q < g.nseq ? seq_token_base(g, q) : dump_row;
    hp[j] = reinterpret_cast<char*>(hc) + ((tokb + (int64_t)t0 * tstride) * ldh + d * L16_H + scol) * 4;
  }
  // ---- input rows: thread -> (row, 16-byte chunk) of the 16 x NIN tile; padded sequences read the last real one ------------
  const char* xp[NXL];
  int xoff[NXL];                                  // float offset inside an Xs buffer
  const int64_t xstep = (int64_t)tdir * tstride * ldx * 4;
#pragma unroll
  for (int i = 0; i < NXL; ++i) {
    const int idx = i * 256 + tid, row = idx / (NIN / 4), ch = idx % (NIN / 4);
    const int q = st * 16 + row;
    const int64_t tokb = seq_token_base(g, q < g.nseq ? q : g.nseq - 1);
    xp[i] = reinterpret_cast<const char*>(x) + ((tokb + (int64_t)t0 * tstride) * ldx + 4 * ch) * 4;
    xoff[i] = row * LDX + 4 * ch;
  }
  float4 xr[NXL];
  // x_0 -> Xs[0], x_1 -> Xs[1], x_2 -> registers (positions past the end re-read the last one: never used)
  auto load_x = [&](int s) {
    const int64_t adv = (int64_t)(s < g.len ? s : g.len - 1) * xstep;
#pragma unroll
    for (int i = 0; i < NXL; ++i) xr[i] = *reinterpret_cast<const float4*>(xp[i] + adv);
  };
  auto stage_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NXL; ++i) *reinterpret_cast<float4*>(Xs + buf * 16 * LDX + xoff[i]) = xr[i];
  };
  load_x(0);
  stage_x(0);
  load_x(1);
  stage_x(1);
  load_x(2);
  for (int i = tid; i < 16 * L16_LDH; i += 256) Hs[i] = 0.f;      // h_{-1} = 0 (buffer 0)
  f32x4v cst[2] = {(f32x4v){0.f, 0.f, 0.f, 0.f}, (f32x4v){0.f, 0.f, 0.f, 0.f}};
  if constexpr (PRO == 1) {
    static_for<4>([&](auto Q) { wait_vm_a16<0>(wq + 16 * decltype(Q)::value); });      // the burst is in (W_ih: in LDS)
    wait_vm_v2<0>(bq[0], bq[1]);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      bsc[b] = bq[b >> 2][b & 3];
#pragma unroll
      for (int i = 0; i < 32; ++i) wf[b][i] = wq[8 * b + (i >> 2)][i & 3];
    }
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int i = 0; i < 32; ++i) asm volatile("" : "+a"(wf[b][i]));
  }
  __syncthreads();

  // ---- acc = b + x W_ih^T of one step, from the staged rows (all of a wave's B fragments come from its own LDS slice) -----
  f32x4v acc[8];
  auto input_part = [&](int buf) {
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[b] = (f32x4v){bsc[b], bsc[b], bsc[b], bsc[b]};
    const float* xrow = Xs + buf * 16 * LDX + i16 * LDX + 4 * ks;
    float4 xa[MK];
#pragma unroll
    for (int m = 0; m < MK; ++m) xa[m] = *reinterpret_cast<const float4*>(xrow + 16 * m);
    float4 wcur[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) wcur[b] = *reinterpret_cast<const float4*>(wl_wave + b * 256);
#pragma unroll
    for (int m = 0; m < MK; ++m) {
      float4 wnext[8];
      if (m + 1 < MK) {
#pragma unroll
        for (int b = 0; b < 8; ++b) wnext[b] = *reinterpret_cast<const float4*>(wl_wave + ((m + 1) * 8 + b) * 256);
      }
      const float av[4] = {xa[m].x, xa[m].y, xa[m].z, xa[m].w};
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const float bv[4] = {wcur[b].x, wcur[b].y, wcur[b].z, wcur[b].w};
          acc[b] = mfma16(av[tt], bv[tt], acc[b]);
        }
      }
      if (m + 1 < MK) {
#pragma unroll
        for (int b = 0; b < 8; ++b) wcur[b] = wnext[b];
      }
    }
  };
  input_part(0);
  __syncthreads();      // step 0 overwrites the buffer of x_0 with x_2

  for (int step = 0; step < g.len; ++step) {
    const float* hcur = Hs + (step & 1) * 16 * L16_LDH;
    float* hnext = Hs + ((step + 1) & 1) * 16 * L16_LDH;
    const float* arow = hcur + i16 * L16_LDH + 4 * ks;
    float4 afr[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) afr[m] = *reinterpret_cast<const float4*>(arow + 16 * m);
    float4 hs[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) hs[j] = *reinterpret_cast<const float4*>(hcur + (srow + 2 * j) * L16_LDH + scol);
#pragma unroll
    for (int b = 0; b < 8; ++b) asm volatile("" : "+v"(acc[b]));
    // step 0 stores the zeros of h_{-1} at position t0 without advancing and step 1 overwrites them
    const int64_t adv = step > 0 ? hstep : 0;

    auto cell_half = [&](int hf) {
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const LstmCell2 u = lstm_cell2((f32x2){acc[hf][r], acc[hf][r + 1]}, (f32x2){acc[2 + hf][r], acc[2 + hf][r + 1]},
                                       (f32x2){acc[4 + hf][r], acc[4 + hf][r + 1]}, (f32x2){acc[6 + hf][r], acc[6 + hf][r + 1]},
                                       (f32x2){cst[hf][r], cst[hf][r + 1]});
        cst[hf][r] = u.c.x;
        cst[hf][r + 1] = u.c.y;
        hnext[(4 * ks + r) * L16_LDH + 32 * w + 16 * hf + i16] = u.h.x;
        hnext[(4 * ks + r + 1) * L16_LDH + 32 * w + 16 * hf + i16] = u.h.y;
      }
    };

    // h_{t-1} W_hh^T, unit half by unit half (lstm16.hip); one memory instruction per MFMA group in the first groups:
    // slots 0, 1 the stores of h_{t-1}; then the input rows of step + 2 go from registers to LDS (they are read at the end of
    // step + 1, behind the barrier that closes this step) and the rows of step + 3 are requested
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const float av[4] = {afr[m].x, afr[m].y, afr[m].z, afr[m].w};
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
          for (int gt = 0; gt < 4; ++gt) acc[2 * gt + hf] = mfma16(av[tt], wf[2 * gt + hf][4 * m + tt], acc[2 * gt + hf]);
          const int slot = 4 * m + tt;
          if (hf == 0 && slot < 2) {
            asm volatile("" : "+v"(hs[slot].x), "+v"(hs[slot].y), "+v"(hs[slot].z), "+v"(hs[slot].w));
            if (RELU) hs[slot] = make_float4(relu1(hs[slot].x), relu1(hs[slot].y), relu1(hs[slot].z), relu1(hs[slot].w));
            *reinterpret_cast<float4*>(hp[slot]) = hs[slot];
            hp[slot] += adv;
            __builtin_amdgcn_sched_barrier(0);
          } else if (hf == 0 && slot == 2) {
            stage_x(step & 1);                    // x_{step+2}: buffer of x_step, last read before the previous barrier
            __builtin_amdgcn_sched_barrier(0);
          } else if (hf == 0 && slot == 3) {
            load_x(step + 3);
            __builtin_amdgcn_sched_barrier(0);
          } else if (hf == 1) {
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            __builtin_amdgcn_sched_group_barrier(0x006, 5, 0);
          }
        }
      }
      if (hf == 0) cell_half(0);
    }
    cell_half(1);
    // the next step's input part: independent of h_t, so it runs in front of the barrier the wave would otherwise wait at
    if (step + 1 < g.len) input_part((step + 1) & 1);
    __syncthreads();
  }
  // h of the last step: the barrier above published it in buffer (len & 1)
  {
    const float* hfin = Hs + (g.len & 1) * 16 * L16_LDH;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float4 v = *reinterpret_cast<const float4*>(hfin + (srow + 2 * j) * L16_LDH + scol);
      if (RELU) v = make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w));
      *reinterpret_cast<float4*>(hp[j]) = v;
    }
  }
}

#define LSTM16X_ARGS                                                                                                         \
  const float *__restrict__ x, int ldx, const float *__restrict__ wih_f, const float *__restrict__ wih_b,                    \
      const float *__restrict__ bih_f, const float *__restrict__ bih_b, const float *__restrict__ bhh_f,                     \
      const float *__restrict__ bhh_b, const float *__restrict__ whh_f, const float *__restrict__ whh_b,                     \
      const float *__restrict__ pk, float *__restrict__ hc, int ldh, int64_t dump_row, SeqGeom g
#define LSTM16X_PASS x, ldx, wih_f, wih_b, bih_f, bih_b, bhh_f, bhh_b, whh_f, whh_b, pk, hc, ldh, dump_row, g
// the kernel, and the kernel with the prologue before the packed copy (engine option lstm_prologue = 0: same-process A/B)
template <int NIN, bool RELU>
__global__ __launch_bounds__(256) void lstm16x_kernel(LSTM16X_ARGS) {
  lstm16x_body<NIN, RELU, 1>(LSTM16X_PASS);
}
template <int NIN, bool RELU>
__global__ __launch_bounds__(256) void lstm16x_pro0_kernel(LSTM16X_ARGS) {
  lstm16x_body<NIN, RELU, 0>(LSTM16X_PASS);
}

// =====================================================================================================================
// num_features = 128: W_ih (512 x 128) is as large as W_hh and the two do not fit one CU's registers together -- W_hh fills
// the AGPR half (256 registers per lane), the LDS has room for 31 of the wave's 64 W_ih fragment sets (k-chunk m, block b)
// beside the h and x tiles, and the other 33 sets (132 registers) live in the architectural VGPRs.  That leaves ~120
// registers for everything else, so the step is written for short live ranges: the recurrent product walks the k-chunks with
// both unit halves per chunk (one h fragment live at a time; the cell update of both halves follows the last MFMA), and the
// input part takes its LDS fragments in groups of four sets, one group ahead.
constexpr int X128_RES = 33;                                   // fragment sets p = 8 m + b < X128_RES: registers; others: LDS
constexpr int X128_WL_FLOATS = 4 * (64 - X128_RES) * 256;      // [wave][set - RES][lane][4]
constexpr int X128_XS_FLOATS = 16 * 128;                       // one step's input rows, unpadded (LDS-DMA), 16-byte chunks XOR-swizzled
constexpr size_t X128_LDS_BYTES = sizeof(float) * (X128_WL_FLOATS + L16_HS_FLOATS + 2 * X128_XS_FLOATS);
static_assert(X128_LDS_BYTES <= 160 * 1024, "LDS budget");

// lstm_cell2 (common.h) with the one contraction its source leaves open written out: c_t = fma(f, c_{t-1}, i * g).  Under
// -ffp-contract=fast `f * c + i * g` may become that or fma(i, g, f * c), which rounds differently; which one the compiler picks
// depends on the code around it (this kernel's step loop came out with the first form for every slot, and with the second form
// for accumulator rows 2, 3 once the same statement stood in a lambda).  Every step loop of lstm16x128_kernel computes the first.
DEV LstmCell2 lstm_cell2_fc(f32x2 ai, f32x2 af, f32x2 ag, f32x2 ao, f32x2 c_prev) {
  LstmCell2 r;
  r.i = rcp_2(1.0f + exp2_2(ai));
  r.f = rcp_2(1.0f + exp2_2(af));
  r.g = 2.0f * rcp_2(1.0f + exp2_2(ag)) - 1.0f;
  r.o = rcp_2(1.0f + exp2_2(ao));
  const f32x2 ig = r.i * r.g;
  r.c = (f32x2){__builtin_fmaf(r.f.x, c_prev.x, ig.x), __builtin_fmaf(r.f.y, c_prev.y, ig.y)};
  const f32x2 th = 2.0f * rcp_2(1.0f + exp2_2(r.c * -2.8853900817779268f)) - 1.0f;
  r.h = r.o * th;
  return r;
}

template <bool RELU, int SCHED, int PRO>
DEV void lstm16x128_body(LSTM16X_ARGS) {
  constexpr int NIN = 128, RES = X128_RES;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Wl = smem;                               // [4][64 - RES][256]
  float* Hs = smem + X128_WL_FLOATS;              // [2][16][L16_LDH]
  float* Xs = Hs + L16_HS_FLOATS;                 // [2][16][128], chunk c of row r stored at chunk position c ^ (r & 15)
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, i16 = lane & 15, ks = lane >> 4;
  const int st = blockIdx.x, d = blockIdx.y;
  const float* whh = d ? whh_b : whh_f;
  const float* wih = d ? wih_b : wih_f;
  const float* bih = d ? bih_b : bih_f;
  const float* bhh = d ? bhh_b : bhh_f;

  float wf[8][32];                                // W_hh fragments -> AGPRs
  float bsc[8];
  float* wl_wave = Wl + w * ((64 - RES) * 256) + lane * 4;
  float wiv[RES][4];                              // W_ih fragment sets 0 .. RES-1 -> VGPRs, the others -> LDS
  if constexpr (PRO == 0) {
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int row = (b >> 1) * L16_H + 32 * w + 16 * (b & 1) + i16;
      const float gs = l16_gate_scale(b >> 1);
      const float* wrow = whh + (int64_t)row * L16_H + 4 * ks;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const float4 v = *reinterpret_cast<const float4*>(wrow + 16 * m);
        wf[b][4 * m + 0] = v.x * gs;
        wf[b][4 * m + 1] = v.y * gs;
        wf[b][4 * m + 2] = v.z * gs;
        wf[b][4 * m + 3] = v.w * gs;
      }
      bsc[b] = (bih[row] + bhh[row]) * gs;
    }
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int i = 0; i < 32; ++i) asm volatile("" : "+a"(wf[b][i]));
#pragma unroll
    for (int p = 0; p < 64; ++p) {
      const int m = p >> 3, b = p & 7;
      const int row = (b >> 1) * L16_H + 32 * w + 16 * (b & 1) + i16;
      const float gs = l16_gate_scale(b >> 1);
      const float4 v = *reinterpret_cast<const float4*>(wih + (int64_t)row * NIN + 16 * m + 4 * ks);
      if (p < RES) {
        constexpr int dummy = 0;
        (void)dummy;
        wiv[p % RES][0] = v.x * gs;
        wiv[p % RES][1] = v.y * gs;
        wiv[p % RES][2] = v.z * gs;
        wiv[p % RES][3] = v.w * gs;
      } else {
        *reinterpret_cast<float4*>(wl_wave + (p - RES) * 256) = make_float4(v.x * gs, v.y * gs, v.z * gs, v.w * gs);
      }
    }
#pragma unroll
    for (int p = 0; p < RES; ++p)
#pragma unroll
      for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(wiv[p][i]));
  }

  const int t0 = d ? g.len - 1 : 0, tdir = d ? -1 : 1;
  const int tstride = seq_token_stride(g);
  const int srow = 4 * w + (lane >> 5), scol = 4 * (lane & 31);
  // h rows and input rows are addressed as a wave-uniform base + a 32-bit byte offset per lane (the host checks that both tensors
  // are below 4 GiB for this kernel): four registers less than 64-bit pointers, which is what keeps the step loop free of scratch
  unsigned hp[2];
  const unsigned hstep = (unsigned)(tdir * tstride * ldh * 4);      // (may be "negative": offsets are taken modulo 2^32)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = st * 16 + srow + 2 * j;
    const int64_t tokb = q < g.nseq ? seq_token_base(g, q) : dump_row;
    hp[j] = (unsigned)(((tokb + (int64_t)t0 * tstride) * ldh + d * L16_H + scol) * 4);
  }
  char* const hcb = reinterpret_cast<char*>(hc);
  // input rows: 16 x 512 bytes per step, by LDS-DMA (no registers): wave w issues two 1-KiB requests, request j = 2w + i covers
  // rows 2j and 2j + 1 -- lane L delivers 16 bytes to LDS position 16 L of the request's KiB, so it FETCHES the chunk that
  // belongs there: row 2j + (L >> 5), chunk (L & 31) ^ (row & 15) (the XOR spreads a fragment read's 16 rows over the banks).
  // Padded sequences read the last real one.
  unsigned xp[2];
  const unsigned xstep = (unsigned)(tdir * tstride * ldx * 4);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = 2 * (2 * w + i) + (lane >> 5);
    const int q = st * 16 + row;
    const int64_t tokb = seq_token_base(g, q < g.nseq ? q : g.nseq - 1);
    xp[i] = (unsigned)(((tokb + (int64_t)t0 * tstride) * ldx + 4 * ((lane & 31) ^ (row & 15))) * 4);
  }
  // Hand-issued (vmem_asm.h): through the builtin the compiler put s_waitcnt vmcnt(0) in front of the NEXT LDS access -- here the
  // a_next fragment read eleven instructions behind the request, so every step sat out the round trip of the rows it had just asked
  // for.  The one wait this traffic needs is written by hand at the end of the step.
  const uint32_t xs_lds = lds_addr(Xs);
  auto dma_x = [&](int s, int buf, int i) {        // x_s -> Xs[buf], this wave's request i
    const unsigned adv = (unsigned)(s < g.len ? s : g.len - 1) * xstep;
    const uint32_t dst = xs_lds + (uint32_t)((buf * X128_XS_FLOATS + (2 * w + i) * 256) * 4);
    dma_part<false>(x, xp[i] + adv, dst);
  };
  dma_x(0, 0, 0); dma_x(0, 0, 1);
  dma_x(1, 1, 0); dma_x(1, 1, 1);
  // PRO = 1: the weights, in one burst behind the rows of x_0 / x_1 and in the order step 0 wants them -- the bias, W_ih (sets
  // 0 .. RES-1 into their VGPRs, the others into this wave's LDS slice by LDS-DMA: no staging registers), then W_hh straight into
  // its AGPRs.  Issue order of the prologue and what each wait leaves in flight (every request is 1 KiB per wave instruction;
  // this kernel has no compiler-counted vector-memory LOAD anywhere and no store in front of the step loop):
  //     4 x rows (LDS-DMA), 2 bias, 64 W_ih, W_hh sets 0..59        130 requests
  //     wait vmcnt(60): names the bias and the resident W_ih sets     rows, bias and all of W_ih are in; 60 W_hh sets in flight
  //     W_hh sets 60..63                                               64 in flight (a wave's counter holds 63: the last one waits for the first)
  //     barrier, step 0's input part (240 MFMAs, no vector-memory instruction)
  //     wait vmcnt(0): names all 64 W_hh quads                         in front of step 0's recurrent product
  f32x4 wq[64], wiq[RES], bq[2];
  auto request_whh = [&](auto Q) {
    constexpr int q = decltype(Q)::value;
    const char* pw = reinterpret_cast<const char*>(pk) + (size_t)(d * 4 + w) * (XPack<128>::SETS * 1024);
    ldg4_uncounted_a<(q & 3) * 1024>(wq[q], pw + (XPack<128>::HH0 + (q & ~3)) * 1024, (uint32_t)lane * 16u);
  };
  // W_hh has landed: in front of the first recurrent product (nothing else of this wave is outstanding then)
  auto whh_landed = [&]() {
    if constexpr (PRO == 1) {
      static_for<4>([&](auto Q) { wait_vm_a16<0>(wq + 16 * decltype(Q)::value); });
#pragma unroll
      for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int i = 0; i < 32; ++i) wf[b][i] = wq[8 * b + (i >> 2)][i & 3];
      // (SCHED 0's loop, left to the compiler, copied quad elements to VGPRs -- 216 v_accvgpr_read and 20 scratch accesses per
      //  step -- until each fragment was pinned on its own as the PRO = 0 prologue pins it; SCHED 1's loop needs no pin)
      if constexpr (SCHED == 0) {
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
          for (int i = 0; i < 32; ++i) asm volatile("" : "+a"(wf[b][i]));
      }
    }
  };
  if constexpr (PRO == 1) {
    using P = XPack<128>;
    const char* pw = reinterpret_cast<const char*>(pk) + (size_t)(d * 4 + w) * (P::SETS * 1024);
    const uint32_t lane16 = (uint32_t)lane * 16u;
    const uint32_t wl_dma = lds_addr(Wl + w * ((64 - RES) * 256));
    ldg4_uncounted<0>(bq[0], pw + P::BIAS0 * 1024, lane16);
    ldg4_uncounted<1024>(bq[1], pw + P::BIAS0 * 1024, lane16);
    static_for<64>([&](auto PP) {
      constexpr int p = decltype(PP)::value;
      if constexpr (p < RES) ldg4_uncounted<(p & 3) * 1024>(wiq[p < RES ? p : 0], pw + (p & ~3) * 1024, lane16);
      else dma_part<false>(pw + p * 1024, lane16, wl_dma + (p - RES) * 1024);
    });
    static_for<60>(request_whh);
  }
  for (int i = tid; i < 16 * L16_LDH; i += 256) Hs[i] = 0.f;
  f32x4v cst[2] = {(f32x4v){0.f, 0.f, 0.f, 0.f}, (f32x4v){0.f, 0.f, 0.f, 0.f}};
  if constexpr (PRO == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    wait_vm_v16<60>(wiq);
    wait_vm_v16<60>(wiq + 16);
    wait_vm_v3<60>(wiq[32], bq[0], bq[1]);
    static_assert(RES == 33, "the three waits above name every resident set");
    request_whh(std::integral_constant<int, 60>{});
    request_whh(std::integral_constant<int, 61>{});
    request_whh(std::integral_constant<int, 62>{});
    request_whh(std::integral_constant<int, 63>{});
#pragma unroll
    for (int b = 0; b < 8; ++b) bsc[b] = bq[b >> 2][b & 3];
#pragma unroll
    for (int p = 0; p < RES; ++p)
#pragma unroll
      for (int i = 0; i < 4; ++i) wiv[p][i] = wiq[p][i];
  }
  __syncthreads();

  f32x4v acc[8];
  // the lane's A fragment of k-chunk m: chunk 4m + ks of row i16, at chunk position (4m + ks) ^ i16 = 4 (m ^ (i16 >> 2)) + (ks ^ (i16 & 3))
  const int xlane = i16 * 128 + 4 * (ks ^ (i16 & 3));
  const int xq = i16 >> 2;
  // acc = b + x W_ih^T: 16 groups of four fragment sets (k-chunk m = group / 2, blocks 4 (group & 1) .. + 3); the sets that live
  // in LDS are fetched ONE PAIR of sets (8 MFMAs = 256 cycles) ahead, by hand: written as ordinary loads "one group ahead" the
  // compiler -- with all 256 + 256 registers in use -- sank every one of them to the MFMA that consumes it and waited for it there:
  // a dozen exposed LDS round trips per step in the generated loop (`ds_read_b128; s_waitcnt lgkmcnt(0); 32 MFMAs`, round 5).  The
  // reads are volatile asm statements now (they stay where they are written, 16 registers for two pairs) and each pair is waited
  // for by one hand-written `s_waitcnt lgkmcnt(0)` that carries the pair's registers as operands.
  const uint32_t wl_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)wl_wave;
  // k-chunk 0 of the NEXT step's input part is held back: its x fragment is read here (x0) and its 32 MFMAs -- registers only, sets
  // 0..7 are resident -- are issued by the next step right behind the barrier, in front of the recurrent product, where they cover
  // the round trip of the first h fragment (which cannot be requested before the barrier).
  // (HALF of it: k = 0, 1 of every lane's four -- 16 MFMAs = 512 cycles cover an LDS round trip, and two registers across the
  //  barrier fit where four brought a scratch reload into the loop)
  f32x2 x0;
  auto input_chunk0 = [&](float t0v, float t1v, int tt0) {
    const float av[2] = {t0v, t1v};
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = 4 * half + j;
          acc[p & 7] = mfma16(av[tt], wiv[p][tt0 + tt], acc[p & 7]);
        }
  };
  auto input_part = [&](int buf) {
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[b] = (f32x4v){bsc[b], bsc[b], bsc[b], bsc[b]};
    const float* xrow = Xs + buf * X128_XS_FLOATS + xlane;
    {
      const float4 xc0 = *reinterpret_cast<const float4*>(xrow + 16 * (0 ^ xq));
      x0 = (f32x2){xc0.x, xc0.y};
      input_chunk0(xc0.z, xc0.w, 2);      // k = 2, 3 of chunk 0 now, k = 0, 1 behind the barrier
    }
    float4 xa = *reinterpret_cast<const float4*>(xrow + 16 * (1 ^ xq));
    static_assert(RES >= 33 && RES <= 34 && (RES & 1) == 1, "sets 0..32 resident: the first LDS pair is (32 resident, 33)");
    // ---- k-chunks 1..3: sets 8..31, all resident
#pragma unroll
    for (int m = 1; m < 4; ++m) {
      const float4 xa_next = *reinterpret_cast<const float4*>(xrow + 16 * (((m + 1) & 3) ^ xq) + 64 * ((m + 1) >> 2));
      const float av[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int p = 8 * m + 4 * half + j;
            acc[p & 7] = mfma16(av[tt], wiv[p][tt], acc[p & 7]);
          }
      xa = xa_next;
    }
    // ---- k-chunks 4..7: sets 32..63 in pairs (p0, p0 + 1); set 32 is resident, the other 31 come from LDS
    f32x4v fa[2][2];
    auto request = [](auto CH, f32x4v (&dst)[2], uint32_t base) {      // the LDS sets of pair CH
      constexpr int p0 = 32 + 2 * decltype(CH)::value;
      if constexpr (p0 >= RES)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[0]) : "v"(base), "n"((p0 - RES) * 1024));
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[1]) : "v"(base), "n"((p0 + 1 - RES) * 1024));
    };
    request(std::integral_constant<int, 0>{}, fa[0], wl_lds);
    float4 xa_next = xa;
    static_for<16>([&](auto CH) {
      constexpr int ch = decltype(CH)::value, p0 = 32 + 2 * ch, m = p0 >> 3;
      if constexpr ((p0 & 7) == 0 && m + 1 < 8) xa_next = *reinterpret_cast<const float4*>(xrow + 16 * (((m + 1) & 3) ^ xq) + 64 * ((m + 1) >> 2));
      // this pair's sets have landed (nothing else of this wave is outstanding on the LDS counter that is younger)
      if constexpr (p0 >= RES) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[ch & 1][0]), "+v"(fa[ch & 1][1]) : : "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[ch & 1][1]) : : "memory");
      if constexpr (ch + 1 < 16) request(std::integral_constant<int, ch + 1 < 16 ? ch + 1 : 0>{}, fa[(ch + 1) & 1], wl_lds);
      __builtin_amdgcn_sched_barrier(0);      // (the pair's MFMAs behind the request: arithmetic is scheduled across an asm statement otherwise)
      const float av[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const float b0 = p0 < RES ? wiv[p0 < RES ? p0 : 0][tt] : fa[ch & 1][0][tt];
        acc[p0 & 7] = mfma16(av[tt], b0, acc[p0 & 7]);
        acc[(p0 + 1) & 7] = mfma16(av[tt], fa[ch & 1][1][tt], acc[(p0 + 1) & 7]);
      }
      if constexpr ((p0 & 7) == 6) xa = xa_next;      // last pair of the k-chunk
    });
  };
  // cell update of both unit halves (lane-local), h_t -> the other LDS buffer
  auto cell_update = [&](float* hnext) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const LstmCell2 u = lstm_cell2_fc((f32x2){acc[hf][r], acc[hf][r + 1]}, (f32x2){acc[2 + hf][r], acc[2 + hf][r + 1]},
                                       (f32x2){acc[4 + hf][r], acc[4 + hf][r + 1]}, (f32x2){acc[6 + hf][r], acc[6 + hf][r + 1]},
                                       (f32x2){cst[hf][r], cst[hf][r + 1]});
        cst[hf][r] = u.c.x;
        cst[hf][r + 1] = u.c.y;
        hnext[(4 * ks + r) * L16_LDH + 32 * w + 16 * hf + i16] = u.h.x;
        hnext[(4 * ks + r + 1) * L16_LDH + 32 * w + 16 * hf + i16] = u.h.y;
      }
    }
  };
  // SCHED 0: the step loop as it was before the LDS schedule was written by hand (kept for same-process A/B, option "lstm_sched")
  if constexpr (SCHED == 0) {
    input_part(0);
    whh_landed();
    __syncthreads();      // step 0 requests x_2 into the buffer of x_0

    for (int step = 0; step < g.len; ++step) {
      const float* hcur = Hs + (step & 1) * 16 * L16_LDH;
      float* hnext = Hs + ((step + 1) & 1) * 16 * L16_LDH;
      const float* arow = hcur + i16 * L16_LDH + 4 * ks;
      // (the two h rows this lane stores: the second is read when the first has left -- one of them live at a time)
      float4 hs = *reinterpret_cast<const float4*>(hcur + srow * L16_LDH + scol);
      float4 a = *reinterpret_cast<const float4*>(arow);
#pragma unroll
      for (int b = 0; b < 8; ++b) asm volatile("" : "+v"(acc[b]));
      input_chunk0(x0.x, x0.y, 0);      // (this step's x_t, fragment read before the barrier)
      __builtin_amdgcn_sched_barrier(0);  // (these 16 MFMAs FIRST: the h row store below was scheduled in front of them, with its wait)
      const unsigned adv = step > 0 ? hstep : 0u;

      // h_{t-1} W_hh^T, k-chunk by k-chunk, all eight blocks per chunk; one memory instruction per MFMA group in the first
      // groups: the stores of h_{t-1}, the input rows of step + 2 to LDS, the requests for the rows of step + 3
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        float4 a_next = a;
        if (m + 1 < 8) a_next = *reinterpret_cast<const float4*>(arow + 16 * (m + 1));
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
          for (int b = 0; b < 8; ++b) acc[b] = mfma16(av[tt], wf[b][4 * m + tt], acc[b]);
          const int slot = 4 * m + tt;
          if (slot < 2) {
            asm volatile("" : "+v"(hs.x), "+v"(hs.y), "+v"(hs.z), "+v"(hs.w));
            if (RELU) hs = make_float4(relu1(hs.x), relu1(hs.y), relu1(hs.z), relu1(hs.w));
            *reinterpret_cast<float4*>(hcb + hp[slot]) = hs;
            hp[slot] += adv;
            if (slot == 0) hs = *reinterpret_cast<const float4*>(hcur + (srow + 2) * L16_LDH + scol);
            __builtin_amdgcn_sched_barrier(0);
          } else if (slot < 4) {
            dma_x(step + 2, step & 1, slot - 2);    // x_{step+2} -> the buffer of x_step (last read before the previous barrier)
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        a = a_next;
      }
      cell_update(hnext);
      if (step + 1 < g.len) input_part((step + 1) & 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's rows of x_{step+2} have landed (read behind the NEXT barrier)
      __syncthreads();
    }
  } else {
    // ================================================================================================================
    // SCHED 1: the step's LDS schedule, written down.  Every LDS read of the loop is issued by hand (vmem_asm.h:
    // lds_read4_uncounted) and covered by ONE hand-counted wait that names its registers (wait_lds<KEEP>); every request +
    // wait group stands between two sched_barrier(0), and so do the h row stores and the LDS-DMA requests.  The only
    // compiler-counted LDS instructions left are the cell update's stores of h_t: they are OLDER than every read issued
    // behind them, so no KEEP below has them among the instructions it leaves in flight, and the compiler's own
    // lgkmcnt(0) in front of the barrier (the fence of __syncthreads) finds them long done.
    //
    // Issue order of one step and what each wait leaves outstanding (MFMA = number of the step's 512 MFMAs issued in
    // front of the group; the LDS answers in order, so KEEP = the number of requests issued behind the wanted one):
    //
    //   MFMA  group                          requests issued               wait: registers          KEEP (left in flight)   lead
    //      0  behind the barrier             hs0, hs1, a0                  -
    //   0-15  input chunk 0, k = 0, 1 (x0: registers)
    //     16  recurrent chunk 0              a1                            hs0, hs1, a0             1 (a1)                  16
    //  24,32  (h row stores: registers have landed)  40, 48: the two LDS-DMA requests for x_{step+2} (vmcnt, not lgkmcnt)
    //  16+32m recurrent chunk m = 1..6       a(m+1)                        a(m)                     1 (a(m+1))              32
    //    240  recurrent chunk 7              x0', x1' (rows of step + 1)   a7                       2 (x0', x1')            32
    //    272  behind the last recurrent MFMA -                             x0', x1'                 0 (nothing younger)     32
    //         cell update (VALU; its stores of h_t are compiler-counted, older than everything below)
    // 272-287 input chunk 0 of step + 1, k = 2, 3 (x0')
    //    288  input chunk 1 (x1')            x2                            -
    //    320  input chunk 2                  x3                            x2                       1 (x3)                  32
    //    352  input chunk 3                  x4, w33                       x3                       2 (x4, w33)             32
    //    384  pair 0 (set 32 resident, 33)   x5, pair 1                    x4, w33                  3 (x5, pair 1)          32
    //  384+8c pair c, not first of a chunk   pair c+1                      pair c                   2 (pair c+1)             8
    //    416  pair 4 (first of chunk 5)      x6, pair 5                    x5, pair 4               3 (x6, pair 5)           8 (x5: 32)
    //    448  pair 8 (first of chunk 6)      x7, pair 9                    x6, pair 8               3 (x7, pair 9)           8 (x6: 32)
    //    480  pair 12 (first of chunk 7)     pair 13                       x7, pair 12              2 (pair 13)              8 (x7: 32)
    //    504  pair 15                        -                             pair 15                  0 (nothing younger)      8
    //    512  vmcnt(0) for the rows of x_{step+2}, barrier.  Nothing hand-issued is outstanding here.
    //
    // The LAST step (written out behind the loop, see one_step) has no input part behind it: it requests no x0' / x1', its wait
    // at 240 is KEEP 0 and it has no group at 272.
    //
    // Leads are the source's own: one k-chunk (32 MFMAs) for h and x fragments, one pair (8 MFMAs) for the W_ih sets, the
    // held-back half of chunk 0 (16 MFMAs) for the first h fragment.  Differences from SCHED 0 that are not order alone:
    // BOTH h rows a lane stores are read at the top of the step (SCHED 0 read the second behind the first store, 8 MFMAs
    // in front of its wait; the 16 registers of the W_ih pairs are free in this part of the step), x0' / x1' are read
    // under recurrent chunk 7 (their buffer was published by the barrier that opened the step) and w33, the first LDS
    // set, a k-chunk ahead.  No register forces a shorter lead anywhere.  Judge the GENERATED loop, not this table:
    // tools/lds_wait_scan.py, tests/test_lds_wait_schedule.py.
    const uint32_t hs_lds = lds_addr(Hs);
    const uint32_t a_off = (uint32_t)((i16 * L16_LDH + 4 * ks) * 4);      // the lane's A fragment of chunk m: + 64 m
    const uint32_t hrow_off = (uint32_t)((srow * L16_LDH + scol) * 4);    // the two h rows the lane stores: + 0, + 2 rows
    const uint32_t xf_off = (uint32_t)(xlane * 4);
    auto request_x = [&](auto M, int buf, f32x4v& dst) {                  // the lane's x fragment of k-chunk M
      constexpr int m = decltype(M)::value;
      lds_read4_uncounted<256 * (m >> 2)>(dst, xs_lds + (uint32_t)(buf * (X128_XS_FLOATS * 4)) + xf_off + ((uint32_t)((m & 3) ^ xq) << 6));
    };
    auto request_w = [&](auto CH, f32x4v (&dst)[2]) {                     // the LDS sets of pair CH
      constexpr int p0 = 32 + 2 * decltype(CH)::value;
      if constexpr (p0 >= RES) lds_read4_uncounted<(p0 >= RES ? p0 - RES : 0) * 1024>(dst[0], wl_lds);
      lds_read4_uncounted<(p0 + 1 - RES) * 1024>(dst[1], wl_lds);
    };
    // acc = b + x W_ih^T without the held-back half of chunk 0; xc0 / xc1 (k-chunks 0 and 1) have landed
    auto input_part1 = [&](int buf, const f32x4v& xc0, const f32x4v& xc1) {
#pragma unroll
      for (int b = 0; b < 8; ++b) acc[b] = (f32x4v){bsc[b], bsc[b], bsc[b], bsc[b]};
      x0 = (f32x2){xc0.x, xc0.y};
      input_chunk0(xc0.z, xc0.w, 2);
      f32x4v xf[8];                             // k-chunks 2..7
      f32x4v fa[2][2];
      static_for<3>([&](auto MM) {              // k-chunks 1..3: sets 8..31, all resident
        constexpr int m = decltype(MM)::value + 1;
        __builtin_amdgcn_sched_barrier(0);
        request_x(std::integral_constant<int, m + 1>{}, buf, xf[m + 1]);
        if constexpr (m == 3) request_w(std::integral_constant<int, 0>{}, fa[0]);
        if constexpr (m == 2) wait_lds<1>(xf[2]);
        if constexpr (m == 3) wait_lds<2>(xf[3]);
        __builtin_amdgcn_sched_barrier(0);
        const f32x4v xv = m == 1 ? xc1 : xf[m];
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
          for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int p = 8 * m + 4 * half + j;
              acc[p & 7] = mfma16(xv[tt], wiv[p][tt], acc[p & 7]);
            }
      });
      static_for<16>([&](auto CH) {             // k-chunks 4..7: sets 32..63 in pairs (p0, p0 + 1)
        constexpr int ch = decltype(CH)::value, p0 = 32 + 2 * ch, m = p0 >> 3;
        constexpr bool first = (p0 & 7) == 0, more_x = first && m + 1 < 8, more_w = ch + 1 < 16;
        constexpr int keep = (more_x ? 1 : 0) + (more_w ? 2 : 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (more_x) request_x(std::integral_constant<int, more_x ? m + 1 : 0>{}, buf, xf[more_x ? m + 1 : 0]);
        if constexpr (more_w) request_w(std::integral_constant<int, more_w ? ch + 1 : 1>{}, fa[(ch + 1) & 1]);
        if constexpr (ch == 0) wait_lds<keep>(xf[m], fa[0][1]);
        else if constexpr (first) wait_lds<keep>(xf[m], fa[ch & 1][0], fa[ch & 1][1]);
        else wait_lds<keep>(fa[ch & 1][0], fa[ch & 1][1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          if constexpr (p0 < RES) acc[p0 & 7] = mfma16(xf[m][tt], wiv[p0 < RES ? p0 : 0][tt], acc[p0 & 7]);
          else acc[p0 & 7] = mfma16(xf[m][tt], fa[ch & 1][0][tt], acc[p0 & 7]);
          acc[(p0 + 1) & 7] = mfma16(xf[m][tt], fa[ch & 1][1][tt], acc[(p0 + 1) & 7]);
        }
      });
    };
    f32x4v xc0, xc1;
    request_x(std::integral_constant<int, 0>{}, 0, xc0);
    request_x(std::integral_constant<int, 1>{}, 0, xc1);
    wait_lds<0>(xc0, xc1);
    input_part1(0, xc0, xc1);
    whh_landed();
    __syncthreads();      // step 0 requests x_2 into the buffer of x_0

    // The last step has no input part behind it and is written out on its own behind the loop (LAST): with the input part
    // under `if (step + 1 < g.len)` inside the loop, the x fragments requested under recurrent chunk 7 were live into a
    // conditional block, and the register allocator answered with W_hh fragments in scratch, 87 v_accvgpr_read and 110
    // v_mov in the loop.
    auto one_step = [&](int step, auto LAST) {
      constexpr bool last = decltype(LAST)::value;
      const uint32_t hcur = hs_lds + (uint32_t)((step & 1) * (16 * L16_LDH * 4));
      float* hnext = Hs + ((step + 1) & 1) * 16 * L16_LDH;
      f32x4v hsv[2], af[8];
      lds_read4_uncounted<0>(hsv[0], hcur + hrow_off);
      lds_read4_uncounted<2 * L16_LDH * 4>(hsv[1], hcur + hrow_off);
      lds_read4_uncounted<0>(af[0], hcur + a_off);
#pragma unroll
      for (int b = 0; b < 8; ++b) asm volatile("" : "+v"(acc[b]));
      input_chunk0(x0.x, x0.y, 0);      // (this step's x_t, fragment read before the barrier)
      const unsigned adv = step > 0 ? hstep : 0u;

      // h_{t-1} W_hh^T, k-chunk by k-chunk, all eight blocks per chunk; one memory instruction per MFMA group in the first
      // groups: the stores of h_{t-1}, then the requests for the input rows of step + 2
      static_for<8>([&](auto MM) {
        constexpr int m = decltype(MM)::value;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (m + 1 < 8) lds_read4_uncounted<64 * (m + 1 < 8 ? m + 1 : 0)>(af[m + 1 < 8 ? m + 1 : 0], hcur + a_off);
        if constexpr (m == 7 && !last) {
          request_x(std::integral_constant<int, 0>{}, (step + 1) & 1, xc0);
          request_x(std::integral_constant<int, 1>{}, (step + 1) & 1, xc1);
        }
        if constexpr (m == 0) wait_lds<1>(hsv[0], hsv[1], af[0]);
        else wait_lds<(m == 7 ? (last ? 0 : 2) : 1)>(af[m]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
          for (int b = 0; b < 8; ++b) acc[b] = mfma16(af[m][tt], wf[b][4 * m + tt], acc[b]);
          const int slot = 4 * m + tt;
          if (slot < 2) {
            __builtin_amdgcn_sched_barrier(0);
            f32x4v v = hsv[slot];
            if (RELU) v = (f32x4v){relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)};
            *reinterpret_cast<f32x4v*>(hcb + hp[slot]) = v;
            hp[slot] += adv;
            __builtin_amdgcn_sched_barrier(0);
          } else if (slot < 4) {
            __builtin_amdgcn_sched_barrier(0);
            dma_x(step + 2, step & 1, slot - 2);    // x_{step+2} -> the buffer of x_step (last read before the previous barrier)
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      });
      if constexpr (!last) {
        __builtin_amdgcn_sched_barrier(0);
        wait_lds<0>(xc0, xc1);
        __builtin_amdgcn_sched_barrier(0);
      }
      cell_update(hnext);
      if constexpr (!last) input_part1((step + 1) & 1, xc0, xc1);
      __builtin_amdgcn_sched_barrier(0);                 // (the last pair's MFMAs in front of the barrier, not behind it)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's rows of x_{step+2} have landed (read behind the NEXT barrier)
      __syncthreads();
    };
    for (int step = 0; step + 1 < g.len; ++step) one_step(step, std::false_type{});
    one_step(g.len - 1, std::true_type{});
  }
  {
    const float* hfin = Hs + (g.len & 1) * 16 * L16_LDH;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float4 v = *reinterpret_cast<const float4*>(hfin + (srow + 2 * j) * L16_LDH + scol);
      if (RELU) v = make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w));
      *reinterpret_cast<float4*>(hcb + hp[j]) = v;
    }
  }
}

template <bool RELU, int SCHED>
__global__ __launch_bounds__(256) void lstm16x128_kernel(LSTM16X_ARGS) {
  lstm16x128_body<RELU, SCHED, 1>(LSTM16X_PASS);
}
template <bool RELU, int SCHED>
__global__ __launch_bounds__(256) void lstm16x128_pro0_kernel(LSTM16X_ARGS) {
  lstm16x128_body<RELU, SCHED, 0>(LSTM16X_PASS);
}

// The packed copy (XPack): one block row per matrix set (a path's direction), 16 blocks each, 16 bytes per thread and turn.
struct Lstm16xPackArgs {
  const float *wih[LSTM16X_PACK_MAX], *whh[LSTM16X_PACK_MAX], *bih[LSTM16X_PACK_MAX], *bhh[LSTM16X_PACK_MAX];   // wih == nullptr: slot left untouched
};
template <int NIN>
__global__ __launch_bounds__(256) void lstm16x_pack_kernel(Lstm16xPackArgs a, float* __restrict__ dst) {
  using P = XPack<NIN>;
  const float *wih = a.wih[blockIdx.y], *whh = a.whh[blockIdx.y], *bih = a.bih[blockIdx.y], *bhh = a.bhh[blockIdx.y];
  if (wih == nullptr) return;
  float4* out = reinterpret_cast<float4*>(dst + (size_t)blockIdx.y * P::DIR_FLOATS);
  for (int f = blockIdx.x * 256 + threadIdx.x; f < 4 * P::SETS * 64; f += gridDim.x * 256) {
    const int lane = f & 63, set = (f >> 6) % P::SETS, w = (f >> 6) / P::SETS;
    const int i16 = lane & 15, ks = lane >> 4;
    float4 v;
    if (set < P::BIAS0) {
      const bool hh = set >= P::HH0;
      const int b = hh ? (set - P::HH0) >> 3 : set & 7, m = hh ? (set - P::HH0) & 7 : set >> 3;
      const int row = (b >> 1) * L16_H + 32 * w + 16 * (b & 1) + i16;
      const float gs = l16_gate_scale(b >> 1);
      const float* src = hh ? whh + (size_t)row * L16_H + 16 * m + 4 * ks : wih + (size_t)row * NIN + 16 * m + 4 * ks;
      const float4 s = *reinterpret_cast<const float4*>(src);
      v = make_float4(s.x * gs, s.y * gs, s.z * gs, s.w * gs);
    } else {
      float r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = 4 * (set - P::BIAS0) + k;
        const int row = (b >> 1) * L16_H + 32 * w + 16 * (b & 1) + i16;
        r[k] = (bih[row] + bhh[row]) * l16_gate_scale(b >> 1);
      }
      v = make_float4(r[0], r[1], r[2], r[3]);
    }
    out[f] = v;
  }
}

}  // namespace

int lstm16x_pack_launch(int nin, void* stream, const float* const* wih, const float* const* whh, const float* const* bih,
                        const float* const* bhh, int n, float* dst) {
  if ((nin != 64 && nin != 128) || n < 1 || n > LSTM16X_PACK_MAX || dst == nullptr) return (int)hipErrorInvalidValue;
  Lstm16xPackArgs a;
  for (int i = 0; i < LSTM16X_PACK_MAX; ++i) {
    a.wih[i] = i < n ? wih[i] : nullptr;
    a.whh[i] = i < n ? whh[i] : nullptr;
    a.bih[i] = i < n ? bih[i] : nullptr;
    a.bhh[i] = i < n ? bhh[i] : nullptr;
  }
  if (nin == 64) hipLaunchKernelGGL(lstm16x_pack_kernel<64>, dim3(16, n), dim3(256), 0, static_cast<hipStream_t>(stream), a, dst);
  else hipLaunchKernelGGL(lstm16x_pack_kernel<128>, dim3(16, n), dim3(256), 0, static_cast<hipStream_t>(stream), a, dst);
  return (int)hipGetLastError();
}

int lstm16x_launch(int nin, bool relu, int nst16, int ndir, void* stream, const float* x, int ldx, const float* const* wih,
                   const float* const* bih, const float* const* bhh, const float* const* whh, float* hc, int ldh,
                   int64_t dump_row, const SeqGeom& g, int sched, const float* pack) {
  if ((nin != 64 && nin != 128) || nst16 < 1 || ndir < 1 || ndir > 2 || g.len < 1) return (int)hipErrorInvalidValue;
  const bool pro = pack != nullptr;
  auto kern = nin == 64 ? (pro ? (relu ? lstm16x_kernel<64, true> : lstm16x_kernel<64, false>)
                               : (relu ? lstm16x_pro0_kernel<64, true> : lstm16x_pro0_kernel<64, false>))
              : pro    ? (sched == 0 ? (relu ? lstm16x128_kernel<true, 0> : lstm16x128_kernel<false, 0>)
                                     : (relu ? lstm16x128_kernel<true, 1> : lstm16x128_kernel<false, 1>))
                       : (sched == 0 ? (relu ? lstm16x128_pro0_kernel<true, 0> : lstm16x128_pro0_kernel<false, 0>)
                                     : (relu ? lstm16x128_pro0_kernel<true, 1> : lstm16x128_pro0_kernel<false, 1>));
  const size_t lds = nin == 64 ? X16<64>::LDS_BYTES : X128_LDS_BYTES;
  static PerDeviceOnce ready[12];
  const int dev = current_hip_device();
  const int ki = 2 * ((nin == 128 ? (sched == 0 ? 4 : 2) : 0) + (relu ? 1 : 0)) + (pro ? 1 : 0);
  if (!ready[ki].done(dev)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    ready[ki].set(dev);
  }
  const int r = ndir == 2 ? 1 : 0;
  hipLaunchKernelGGL(kern, dim3(nst16, ndir), dim3(256), lds, static_cast<hipStream_t>(stream), x, ldx, wih[0], wih[r], bih[0],
                     bih[r], bhh[0], bhh[r], whh[0], whh[r], pack, hc, ldh, dump_row, g);
  return (int)hipGetLastError();
}
