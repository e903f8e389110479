// gemm_t.hip -- a K = 128 forward projection with a wide output, transposed and weights-stationary like dgrad_t.hip (round 5):
//
//     out[M][NOUT] = A[M][128] W[NOUT][128]^T + bias           NOUT = 384: qkv = x W_in^T + b_in, the in-projection of
//                                                                nn.MultiheadAttention (dptn.py:16-21, 46) in the TRAINING forward
//
// (inference forms it inside the fused attention block).  It was a gemm_ws.h launch at 0.65 MFMA-busy (388 k cycles per launch,
// profiles/r05_train_mfma_utilisation.txt): the A tile staged through registers, the C tile through LDS with a second barrier and a
// 12-pass row epilogue.  Here: A tile by hand-counted LDS-DMA (512-byte rows: half-EXEC requests), wave w = output columns
// [NOUT/4 w, NOUT/4 (w + 1)) in NT = NOUT / 128 blocks of 32 (three accumulation chains alternate), the accumulators START from the
// bias (a per-lane constant vector read from LDS), so a tile's result is 4 NT 16-byte fragment stores and nothing else; the
// previous tile's stores and the next tile's requests sit between the MFMAs; one barrier per 32-token tile.
// Weights: the fragment-order copy gemm_pack_rows_kernel makes (gemm_ws.h: [column block 32][k-chunk 16][lane 64][4]).
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "common.h"
#include "gemm_t.h"
#include "vmem_asm.h"

namespace {

constexpr int KIN = 128, CH = KIN / 8, LDA = KIN + 4;

// Vector-memory operations of a wave inside tile i, in issue order: [ticket atomic, one lane] | rows(i + 1) x 8 [HN] | stores(i - 1)
// x NS [HP] (two slots per k-chunk: the requests first, the stores behind them) -- end of the tile: rows(i + 1) must be in -> at most
// (HP ? NS : 0) younger operations outstanding [HN]; last tile, in front of its own stores: the ticket atomic must be back -> at most
// (HP ? NS : 0), the stores(i - 1) [!HN].
template <int NOUT>
__global__ __launch_bounds__(256) void gemm_t_kernel(const float* __restrict__ A, const float* __restrict__ Wp, const float* __restrict__ bias,
                                                     float* __restrict__ out, int64_t M, int ntiles, unsigned* queue) {
  constexpr int NT = NOUT / 128, NS = 4 * NT, WCOLS = NOUT / 4;
  static_assert(8 + NS <= 2 * CH, "two request slots per k-chunk");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Bs = smem + 4;                            // [NOUT] bias, behind the [2] tile tickets
  float* As = Bs + NOUT;                           // [2][32][LDA]
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, c = lane & 31, hh = lane >> 5;
  TicketLoop tk(reinterpret_cast<int*>(smem), queue, ntiles);
  for (int i = tid; i < NOUT; i += 256) Bs[i] = bias[i];
  __syncthreads();
  int tile = tk.first_tile();
  if (tile >= ntiles) return;

  const uint32_t lane16 = (uint32_t)lane * 16u;
  const uint32_t as_lds = lds_addr(As);
  const char* const Ab = reinterpret_cast<const char*>(A);
  auto issue_req = [&](int t, int b, int r) {      // row 8 w + r of tile t -> buffer b (rows beyond M repeat the last one)
    const int row = 8 * w + r;
    int64_t grow = (int64_t)t * 32 + row;
    grow = grow < M ? grow : M - 1;
    dma_part<true>(Ab + grow * (KIN * 4), lane16, as_lds + (uint32_t)((b * 32 + row) * LDA * 4));
  };
#pragma unroll
  for (int r = 0; r < 8; ++r) issue_req(tile, 0, r);

  // W fragments (A operand): wf4[nt * 16 + m] of lane (c, hh) = W[WCOLS w + 32 nt + c][8 m + 4 hh .. + 3], straight into AGPRs
  f32x4 wf4[NT * CH];
  {
    const char* wb = reinterpret_cast<const char*>(Wp + (size_t)w * NT * CH * 256);
    static_for<NT * CH / 4>([&](auto MQ) {
      constexpr int mq = decltype(MQ)::value;
      ldg4_uncounted_a<0>(wf4[4 * mq + 0], wb + mq * 4096, lane16);
      ldg4_uncounted_a<1024>(wf4[4 * mq + 1], wb + mq * 4096, lane16);
      ldg4_uncounted_a<2048>(wf4[4 * mq + 2], wb + mq * 4096, lane16);
      ldg4_uncounted_a<3072>(wf4[4 * mq + 3], wb + mq * 4096, lane16);
    });
  }
  static_for<NT * CH / 16>([&](auto Q) { wait_vm_a16<0>(wf4 + 16 * decltype(Q)::value); });   // weights and the first tile's rows are in

  int buf = 0;
  f32x4 res[NS];             // results of the previous tile, on their way out
  char* pbase = nullptr;
  uint32_t poff = 0;
  auto store_piece = [&](char* base, uint32_t off, auto J) {      // piece j = 4 nt + jj: columns WCOLS w + 32 nt + 8 jj + 4 hh ..
    constexpr int j = decltype(J)::value;
    stg4_uncounted<(j / 4) * 128 + (j % 4) * 32>(base, off, res[j]);
  };
  auto body = [&](auto HAS_NEXT, auto HAS_PREV, int next) {
    constexpr bool HN = decltype(HAS_NEXT)::value, HP = decltype(HAS_PREV)::value;
    const int64_t tok0 = (int64_t)tile * 32;
    const int last = (int)(M - 1 - tok0 < 31 ? M - 1 - tok0 : 31);      // wave-uniform
    const uint32_t eoff = (uint32_t)(((c < last ? c : last) * NOUT + WCOLS * w + 4 * hh) * 4);
    char* const obase = reinterpret_cast<char*>(out) + tok0 * (NOUT * 4);
    // accumulators start from the bias: register 4 jj + t of block nt belongs to column WCOLS w + 32 nt + 8 jj + 4 hh + t
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float4 bv = *reinterpret_cast<const float4*>(Bs + WCOLS * w + 32 * nt + 8 * jj + 4 * hh);
        acc[nt][4 * jj] = bv.x; acc[nt][4 * jj + 1] = bv.y; acc[nt][4 * jj + 2] = bv.z; acc[nt][4 * jj + 3] = bv.w;
      }
    const float* arow = As + (buf * 32 + c) * LDA + 4 * hh;
    static_for<2>([&](auto B_) {
      constexpr int b = decltype(B_)::value;
      float4 af[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) af[m] = *reinterpret_cast<const float4*>(arow + 8 * (8 * b + m));
      static_for<8>([&](auto M_) {
        constexpr int m = decltype(M_)::value, ch = 8 * b + m;
        static_for<2>([&](auto H_) {      // half a k-chunk: 2 NT MFMAs, the NT chains alternate
          constexpr int h2 = decltype(H_)::value, slot = 2 * ch + h2;
          const float a0 = h2 == 0 ? af[m].x : af[m].z, a1 = h2 == 0 ? af[m].y : af[m].w;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma32(wf4[nt * CH + ch][2 * h2], a0, acc[nt]);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma32(wf4[nt * CH + ch][2 * h2 + 1], a1, acc[nt]);
          __builtin_amdgcn_sched_barrier(0);      // (MFMAs are scheduled across a volatile asm statement otherwise: pin the place)
          if constexpr (slot < 8) {
            if constexpr (HN) {
              issue_req(next, buf ^ 1, slot);
              __builtin_amdgcn_sched_barrier(0);
            }
          } else if constexpr (slot < 8 + NS) {
            if constexpr (HP) {
              store_piece(pbase, poff, std::integral_constant<int, slot - 8>{});
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        });
      });
    });
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
        res[4 * nt + jj] = (f32x4){acc[nt][4 * jj], acc[nt][4 * jj + 1], acc[nt][4 * jj + 2], acc[nt][4 * jj + 3]};
    pbase = obase;
    poff = eoff;
    if constexpr (!HN) {
      tk.retire<HP ? NS : 0>();      // the ticket nobody will use is back: its register stays its own until here
      static_for<NS>([&](auto J) { store_piece(pbase, poff, J); });
    }
    if constexpr (HN) tk.wait<HP ? NS : 0>();      // the next tile's rows (this wave's requests) are in
  };

  tk.run(tile, buf, body);
}

}  // namespace

int gemm_t_launch(void* stream, const GemmTArgs& a, int num_cus) {
  if (a.nout != 384 || a.M < 1 || !a.A || !a.Wpacked || !a.bias || !a.out) return (int)hipErrorInvalidValue;
  if ((a.M + 31) / 32 > 0x7fffffff / 2 || ((uintptr_t)a.A & 15) || ((uintptr_t)a.out & 15) || ((uintptr_t)a.Wpacked & 15)) return (int)hipErrorInvalidValue;
  auto kern = gemm_t_kernel<384>;
  const size_t lds = sizeof(float) * (4 + 384 + 2 * 32 * (size_t)LDA);
  const int dev = current_hip_device();
  static PerDeviceOnce ready;
  if (!ready.done(dev)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    ready.set(dev);
  }
  const int ntiles = (int)((a.M + 31) / 32);
  const int grid = ntiles < num_cus ? ntiles : num_cus;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, static_cast<hipStream_t>(stream), a.A, a.Wpacked, a.bias, a.out, a.M, ntiles, a.queue);
  return (int)hipGetLastError();
}
