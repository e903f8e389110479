// mask_tail.h -- the masked separation tail of DPTNEncDec (dptn.py:103-115,122-141,185-193): launch boundary of
// mask_tail.hip, called by run_tail / run_tail_backward (dptnav.hip) when dptnav_config.mask_tail is set.
//
// Rows r of the (2, B, L) frame list; u_r = overlap-added separated tokens of speaker r / (B L), zero outside
// [left, left + ola) (the reference pads BEFORE the two 1x1 convs, so those frames still see the biases):
//   a = [W_out; W_gate] u_r + [b_out; b_gate]          (Wp: [2N][N] rows, then the 2N biases)
//   m = ReLU(tanh(a_out) * sigmoid(a_gate)),  q = m * E_r,  D[r][j] = sum_c q[c] W_dec[c][j]
#pragma once
#include <cstdint>

struct MaskTailGeom {
  const float* Z;   // (B*S*K, 2N) separated tokens
  const float* E;   // (B*L, N) encoded latent, frame-major
  int B, L, S, K, P, left, ola, kenc;
};

// Wp[0 : 2N*N] = [W_out; W_gate] (row = output channel), Wp[2N*N : 2N*N + 2N] = [b_out; b_gate]
int mask_tail_pack_launch(void* stream, int N, const float* w_out, const float* b_out, const float* w_gate,
                          const float* b_gate, float* Wp);
// D (2*B*L, 8) decoder tap products (columns j >= kenc: 0)
int mask_tail_fwd_launch(void* stream, int N, const MaskTailGeom& g, const float* Wp, const float* wdec, float* D,
                         int num_cus);
// Recomputes the forward per frame tile and writes DQ = (d q) * m (rows x N, the gradient of E through the product),
// DA = [d a_out | d a_gate] (rows x 2N) and per-workgroup decoder weight-gradient partials [grid][N][8]
// (at most max_wgs workgroups; the grid used is returned in *grid_used).
int mask_tail_bwd_launch(void* stream, int N, const MaskTailGeom& g, const float* Wp, const float* wdec,
                         const float* dy1, const float* dy2, int64_t T, int stride, int pad_left, float* DQ, float* DA,
                         float* partials, int max_wgs, int num_cus, int* grid_used);
// [dW_out; dW_gate] (2N x N) and [db_out; db_gate] (2N) -> the four gradient slots
int mask_tail_grad_scatter_launch(void* stream, int N, const float* gw, const float* gb, float* g_wout, float* g_bout,
                                  float* g_wgate, float* g_bgate);
