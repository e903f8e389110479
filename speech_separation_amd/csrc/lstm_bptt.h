// lstm_bptt.h -- LSTM backward through time: shared declarations (kernel in lstm_bptt.hip).
#pragma once
#include "common.h"
#include "lstm.h"
#include "lstm16.h"

// d tanh-free pieces of the cell backward for TWO accumulator slots (packed fp32), shared by both tile sizes
struct Bptt2 {
  f32x2 dpi, dpf, dpg, dpo, dc_next;
};
DEV Bptt2 bptt_cell2(f32x2 dh, f32x2 dc_in, f32x2 i, f32x2 f, f32x2 g, f32x2 o, f32x2 c, f32x2 cprev) {
  // tanh(c) = 2 / (1 + 2^(-2 log2e c)) - 1
  const f32x2 e = exp2_2(c * -2.8853900817779268f);
  const f32x2 tc = 2.0f * rcp_2(1.0f + e) - 1.0f;
  const f32x2 dho = dh * o;
  const f32x2 dc = dc_in + dho * (1.0f - tc * tc);
  Bptt2 r;
  r.dpo = dh * tc * (o - o * o);
  const f32x2 dci = dc * i;
  r.dpi = dc * g * (i - i * i);
  r.dpf = dc * cprev * (f - f * f);
  r.dpg = dci - dci * g * g;
  r.dc_next = dc * f;
  return r;
}

constexpr int BPTT_LDP = 512 + 4;
constexpr size_t BPTT_LDS_BYTES = sizeof(float) * 2 * 32 * BPTT_LDP;

// One launch = both directions of one TransformerDPRNN's LSTM over `nst` tiles of 32 sequences.
//   tape_gates / tape_c : the forward's tape (lstm.h);  dh_up[tok][ldh] : upstream gradient of h (dump rows included);
//   dg_out[tok][ldg]    : dP = gradient of the gate pre-activations, token-major (feeds the W_ih / W_hh gradient GEMMs
//                         and the data gradient);  bias_partials[ndir][nst][512] : per-workgroup column sums of dP.
// Returns a hipError_t as int.
int lstm_bptt_launch(int nst, int ndir, void* stream, const float* tape_gates, const float* tape_c, const float* whh_f,
                     const float* whh_b, const float* dh_up, int ldh, float* dg_out, int ldg, int dump_row,
                     const SeqGeom& g, float* bias_partials);

// 16-sequence-tile variant (lstm_bptt16.hip): consumes the tape of lstm16.hip's training forward; bias_partials is
// [ndir][nst16][512].
constexpr int BPTT16_LDP = 512 + 8;
constexpr size_t BPTT16_LDS_BYTES = sizeof(float) * 2 * 16 * BPTT16_LDP;
int lstm_bptt16_launch(int nst16, int ndir, void* stream, const float* tape_gates, const float* tape_c, const float* whh_f,
                       const float* whh_b, const float* dh_up, int ldh, float* dg_out, int ldg, int dump_row,
                       const SeqGeom& g, float* bias_partials);
