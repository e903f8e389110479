// attn_long_train.h -- training attention for sequences of any length (option train_long_seq): streaming forward with a
// tape, and a two-launch backward on key / query tiles of fixed size.  Exact fp32 MFMA, no atomics: y, dx and dqkv are
// bitwise repeatable.
//
// The on-chip trio (attention_kernel / attention_bwd_kernel<.,.,0/1>) keeps a whole sequence in registers and LDS and stops
// at 256 positions.  These three hold one 32 x 32 block pair at a time:
//   * forward: attention_long_kernel's scheme (transposed score tiles, running (max, sum) per query in the query's lanes,
//     O^T = V^T P^T, K rows from global memory one key block ahead) plus the tape -- stats_out[(token, head)] = (row max
//     in the log2 domain, 1 / row sum) exactly as attention_kernel leaves it -- and train-mode dropout: the normaliser sums
//     every key, a dropped entry only leaves the P V accumulation, 1 / (1 - p) is folded into the final scale.
//   * backward A: a wave owns a query block and walks the key blocks; K and V rows of a key block are staged by the whole
//     workgroup (four query blocks) into one of two LDS tiles, the next block's rows are requested before the MFMAs of this
//     one and stored behind them (one barrier per block).  P is recomputed from the taped (m, 1/l); delta = <dO, O>; dQ
//     stays in registers; stats[token][head] = (m, 1/l, delta, dropout seed of the query).
//   * backward B: a wave owns a key block and walks the query blocks (Q, dO rows and the stats of A through the same two
//     LDS tiles), accumulating dK and dV in registers.
// Keep decisions are RE-HASHED (drop_rand_q) in all three, not read from the bit-mask tape: the hash is a pure function of
// (seed, token, head, key), so there is nothing to lay out or size by the block count, and the per-query seed -- the
// expensive half -- travels to phase B in the fourth stats word.
// The bodies of A and B are those of attention_bwd_kernel with the key / query block index as a run-time loop and the
// tile in LDS instead of the whole sequence; waves whose block lies beyond the sequence (the last workgroup of a sequence)
// run on zeros and store nothing, so every wave reaches every barrier.
#pragma once
#include "common.h"

DEV bool drop_keep(uint32_t qseed, uint32_t key, uint32_t thresh) { return drop_rand_q(qseed, key) >= thresh; }

template <int DH>
__global__ __launch_bounds__(256, 2) void attention_long_train_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N,
                                                                       int heads, SeqGeom g, float scale_log2e, DropCfg drop,
                                                                       float2* __restrict__ stats_out) {
  static_assert(DH == 32 || DH == 16, "head width");
  const int tid = threadIdx.x;
  const int w = tid >> 6, lane = tid & 63, c = lane & 31, hh = lane >> 5;
  const int seq = blockIdx.x, head = blockIdx.y;
  const int len = g.len;
  const int64_t tok0 = seq_token_base(g, seq);
  const int tstride = seq_token_stride(g);
  const int ld = 3 * N;
  const float* base = qkv + head * DH;
  const int nkb = (len + 31) / 32;
  const bool dcol = c < DH;                       // DH = 16: only half of the 32 V^T rows exist
  const int cd = dcol ? c : 0;
  const bool dropping = drop.thresh != 0u;        // wave-uniform

  for (int qb = w; qb < nkb; qb += 4) {
    const int pq = qb * 32 + c;
    const uint32_t qseed = drop_qseed(drop.seed, (uint32_t)(tok0 + (int64_t)pq * tstride) * (uint32_t)heads + (uint32_t)head);
    float qf[DH / 2];
    {
      const float* row = base + (tok0 + (int64_t)(pq < len ? pq : 0) * tstride) * ld + 4 * hh;
#pragma unroll
      for (int m = 0; m < DH / 8; ++m) {
        float4 v = *reinterpret_cast<const float4*>(row + 8 * m);
        if (pq >= len) v = make_float4(0.f, 0.f, 0.f, 0.f);
        qf[4 * m + 0] = v.x * scale_log2e;
        qf[4 * m + 1] = v.y * scale_log2e;
        qf[4 * m + 2] = v.z * scale_log2e;
        qf[4 * m + 3] = v.w * scale_log2e;
      }
    }
    // key-block operands as in attention_long_kernel: rows beyond len read row 0 and are masked / zeroed; element offsets
    // are 32-bit (host-checked).  K rows come one key block ahead in two statically named buffers; the V^T values of a block
    // are requested at its top and arrive behind its score MFMAs, softmax and hash (a second V buffer, as in the inference
    // kernel, put the DH = 32 kernel past 256 VGPRs with the hash beside it)
    const unsigned koff = (unsigned)(N + 4 * hh), voff = (unsigned)(2 * N + cd);
    const unsigned tbase = (unsigned)tok0, ts = (unsigned)tstride, ldu = (unsigned)ld;
    auto fetch = [&](int kb, float4 (&kf)[DH / 8]) {
      const int key = kb * 32 + c;
      const float* krow = base + (tbase + (unsigned)(key < len ? key : 0) * ts) * ldu + koff;
#pragma unroll
      for (int m = 0; m < DH / 8; ++m) kf[m] = *reinterpret_cast<const float4*>(krow + 8 * m);
    };
    auto fetch_v = [&](int kb, float (&vf)[16]) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kr = kb * 32 + ROW32(r, hh);
        const float v = base[(tbase + (unsigned)(kr < len ? kr : 0) * ts) * ldu + voff];
        vf[r] = (kr < len && dcol) ? v : 0.f;
      }
    };
    float mrun = -1e30f, lrun = 0.f;
    f32x16 o = zero16();
    auto block = [&](int kb, const float4 (&kf)[DH / 8]) {
      float vf[16];
      fetch_v(kb, vf);
      f32x16 s = zero16();
#pragma unroll
      for (int m = 0; m < DH / 8; ++m) {
        s = mfma32(kf[m].x, qf[4 * m + 0], s);
        s = mfma32(kf[m].y, qf[4 * m + 1], s);
        s = mfma32(kf[m].z, qf[4 * m + 2], s);
        s = mfma32(kf[m].w, qf[4 * m + 3], s);
      }
      if ((kb + 1) * 32 > len) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kb * 32 + ROW32(r, hh) >= len) s[r] = -1e30f;
      }
      float mx = s[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mnew = fmaxf(mrun, mx);
      const float alpha = fast_exp2(mrun - mnew);
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = fast_exp2(s[r] - mnew);
        sum += s[r];
      }
      sum += __shfl_xor(sum, 32);
      lrun = lrun * alpha + sum;      // every key, kept or not
      mrun = mnew;
      if (dropping) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = drop_keep(qseed, (uint32_t)(kb * 32 + ROW32(r, hh)), drop.thresh) ? s[r] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) o = mfma32(vf[r], s[r], o);
    };
    float4 kfa[DH / 8], kfb[DH / 8];
    fetch(0, kfa);
    for (int kb = 0; kb < nkb; kb += 2) {
      if (kb + 1 < nkb) fetch(kb + 1, kfb);
      block(kb, kfa);
      if (kb + 1 < nkb) {
        if (kb + 2 < nkb) fetch(kb + 2, kfa);
        block(kb + 1, kfb);
      }
    }
    if (pq < len) {
      const float inv = fast_rcp(lrun);
      if (stats_out != nullptr && hh == 0) stats_out[(tok0 + (int64_t)pq * tstride) * heads + head] = make_float2(mrun, inv);
      const float f = inv * drop.inv_keep;
      float* orow = out + (tok0 + (int64_t)pq * tstride) * N + head * DH;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d0 = 8 * j + 4 * hh;
        if (d0 < DH)
          *reinterpret_cast<float4*>(orow + d0) = make_float4(o[4 * j + 0] * f, o[4 * j + 1] * f, o[4 * j + 2] * f, o[4 * j + 3] * f);
      }
    }
  }
}

// LDS of the two backward launches: two buffers of two 32-row tiles (+ 32 float4 of per-query statistics in phase B)
template <int DH>
struct AttnLongBwdShape {
  static constexpr int LD = DH + 4;           // conflict-free ds_read_b128, as AttnBwdShape
  static constexpr int TILE = 32 * LD;
  static constexpr int BUF = 2 * TILE + 128;
};

// grid (sequences, heads, ceil(query blocks / 4)), 256 threads
template <int DH>
__global__ __launch_bounds__(256, 2) void attention_long_bwd_a_kernel(const float* __restrict__ qkv, const float* __restrict__ att,
                                                                       const float* __restrict__ datt, float* __restrict__ dqkv,
                                                                       float* __restrict__ stats, int heads, int N, SeqGeom g, float scale,
                                                                       DropCfg drop, const float2* __restrict__ fstats) {
  using Sh = AttnLongBwdShape<DH>;
  constexpr int LD = Sh::LD, R4 = DH / 4;
  __shared__ __attribute__((aligned(16))) float smem[2 * Sh::BUF];
  const int tid = threadIdx.x;
  const int wv = tid >> 6, lane = tid & 63, c = lane & 31, hh = lane >> 5;
  const int seq = blockIdx.x, head = blockIdx.y;
  const int len = g.len;
  const int nkb = (len + 31) / 32;
  const int64_t tok0 = seq_token_base(g, seq);
  const int tstride = seq_token_stride(g);
  const int ld3 = 3 * N;
  const float sl2e = scale * 1.4426950408889634f;
  const int qb = blockIdx.z * 4 + wv;           // may lie beyond the sequence: every p >= len then
  const int p = qb * 32 + c;
  const bool dropping = drop.thresh != 0u;

  // this thread's piece of a staged key block: row sr, float4 sf of the K and of the V row (DH = 16: threads 0..127)
  const int sr = tid / R4, sf = tid % R4;
  const bool stager = sr < 32;
  auto stage_load = [&](int kb, float4& k4, float4& v4) {
    const int key = kb * 32 + (stager ? sr : 0);
    const float* row = qkv + (tok0 + (int64_t)(key < len ? key : len - 1) * tstride) * ld3 + head * DH + 4 * sf;
    k4 = mask4(*reinterpret_cast<const float4*>(row + N), key < len);
    v4 = mask4(*reinterpret_cast<const float4*>(row + 2 * N), key < len);
  };
  auto stage_store = [&](int buf, const float4& k4, const float4& v4) {
    if (stager) {
      float* Ks = smem + buf * Sh::BUF;
      *reinterpret_cast<float4*>(&Ks[sr * LD + 4 * sf]) = k4;
      *reinterpret_cast<float4*>(&Ks[Sh::TILE + sr * LD + 4 * sf]) = v4;
    }
  };
  float4 k4, v4;
  stage_load(0, k4, v4);

  float qf[DH / 2], df[DH / 2];
  float dsum = 0.f;
  {
    const int64_t tok = tok0 + (int64_t)(p < len ? p : 0) * tstride;
    const float* qrow = qkv + tok * ld3 + head * DH + 4 * hh;
    const float* drow = datt + tok * N + head * DH + 4 * hh;
    const float* orow = att + tok * N + head * DH + 4 * hh;
#pragma unroll
    for (int m = 0; m < DH / 8; ++m) {
      float4 q4 = *reinterpret_cast<const float4*>(qrow + 8 * m);
      float4 d4 = *reinterpret_cast<const float4*>(drow + 8 * m);
      float4 o4 = *reinterpret_cast<const float4*>(orow + 8 * m);
      if (p >= len) q4 = d4 = o4 = make_float4(0.f, 0.f, 0.f, 0.f);
      qf[4 * m + 0] = q4.x * sl2e; qf[4 * m + 1] = q4.y * sl2e; qf[4 * m + 2] = q4.z * sl2e; qf[4 * m + 3] = q4.w * sl2e;
      df[4 * m + 0] = d4.x; df[4 * m + 1] = d4.y; df[4 * m + 2] = d4.z; df[4 * m + 3] = d4.w;
      dsum += d4.x * o4.x + d4.y * o4.y + d4.z * o4.z + d4.w * o4.w;
    }
  }
  const float delta = dsum + __shfl_xor(dsum, 32);
  const int64_t qtok = tok0 + (int64_t)(p < len ? p : 0) * tstride;
  float2 ms = fstats[qtok * heads + head];
  if (p >= len) ms = make_float2(0.f, 0.f);
  const float mx = ms.x, inv = ms.y;
  const uint32_t qseed = drop_qseed(drop.seed, (uint32_t)qtok * (uint32_t)heads + (uint32_t)head);
  if (hh == 0 && p < len)
    *reinterpret_cast<float4*>(stats + (qtok * heads + head) * 4) = make_float4(mx, inv, delta, __uint_as_float(qseed));

  stage_store(0, k4, v4);
  __syncthreads();
  f32x16 dq = zero16();
  for (int kb = 0; kb < nkb; ++kb) {
    if (kb + 1 < nkb) stage_load(kb + 1, k4, v4);
    const float* Ks = smem + (kb & 1) * Sh::BUF;
    const float* Vs = Ks + Sh::TILE;
    f32x16 sc = zero16(), dp = zero16();
    const float* krow = Ks + c * LD + 4 * hh;
    const float* vrow = Vs + c * LD + 4 * hh;
#pragma unroll
    for (int m = 0; m < DH / 8; ++m) {
      const float4 k = *reinterpret_cast<const float4*>(krow + 8 * m);
      const float4 v = *reinterpret_cast<const float4*>(vrow + 8 * m);
      sc = mfma32(k.x, qf[4 * m + 0], sc);
      dp = mfma32(v.x, df[4 * m + 0], dp);
      sc = mfma32(k.y, qf[4 * m + 1], sc);
      dp = mfma32(v.y, df[4 * m + 1], dp);
      sc = mfma32(k.z, qf[4 * m + 2], sc);
      dp = mfma32(v.z, df[4 * m + 2], dp);
      sc = mfma32(k.w, qf[4 * m + 3], sc);
      dp = mfma32(v.w, df[4 * m + 3], dp);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int krow_i = ROW32(r, hh);
      const int key = kb * 32 + krow_i;
      const float kval = Ks[krow_i * LD + (c < DH ? c : 0)];
      const float kk = c < DH ? kval : 0.f;
      float pr = fast_exp2(sc[r] - mx) * inv;
      pr = key < len ? pr : 0.f;
      float dpv = dp[r] * drop.inv_keep;
      if (dropping) dpv = drop_keep(qseed, (uint32_t)key, drop.thresh) ? dpv : 0.f;
      dq = mfma32(pr * (dpv - delta), kk, dq);
    }
    if (kb + 1 < nkb) stage_store((kb + 1) & 1, k4, v4);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int pq = qb * 32 + ROW32(r, hh);
    if (pq < len && c < DH) dqkv[(tok0 + (int64_t)pq * tstride) * ld3 + head * DH + c] = dq[r] * scale;
  }
}

// grid (sequences, heads, ceil(key blocks / 4)), 256 threads
template <int DH>
__global__ __launch_bounds__(256, 2) void attention_long_bwd_b_kernel(const float* __restrict__ qkv, const float* __restrict__ datt,
                                                                       float* __restrict__ dqkv, const float* __restrict__ stats, int heads,
                                                                       int N, SeqGeom g, float scale, DropCfg drop) {
  using Sh = AttnLongBwdShape<DH>;
  constexpr int LD = Sh::LD, R4 = DH / 4;
  __shared__ __attribute__((aligned(16))) float smem[2 * Sh::BUF];
  const int tid = threadIdx.x;
  const int wv = tid >> 6, lane = tid & 63, c = lane & 31, hh = lane >> 5;
  const int seq = blockIdx.x, head = blockIdx.y;
  const int len = g.len;
  const int nqb = (len + 31) / 32;
  const int64_t tok0 = seq_token_base(g, seq);
  const int tstride = seq_token_stride(g);
  const int ld3 = 3 * N;
  const float sl2e = scale * 1.4426950408889634f;
  const int kb = blockIdx.z * 4 + wv;           // may lie beyond the sequence
  const int key = kb * 32 + c;
  const bool key_ok = key < len;
  const bool dropping = drop.thresh != 0u;

  // this thread's piece of a staged query block: row sr, float4 sf of the Q and of the dO row; threads 0..31 also the stats row
  const int sr = tid / R4, sf = tid % R4;
  const bool stager = sr < 32;
  auto stage_load = [&](int qb, float4& q4, float4& d4, float4& s4) {
    const int pq = qb * 32 + (stager ? sr : 0);
    const int64_t tok = tok0 + (int64_t)(pq < len ? pq : len - 1) * tstride;
    q4 = mask4(*reinterpret_cast<const float4*>(qkv + tok * ld3 + head * DH + 4 * sf), pq < len);
    d4 = mask4(*reinterpret_cast<const float4*>(datt + tok * N + head * DH + 4 * sf), pq < len);
    const int ps = qb * 32 + (tid & 31);
    s4 = mask4(*reinterpret_cast<const float4*>(stats + ((tok0 + (int64_t)(ps < len ? ps : len - 1) * tstride) * heads + head) * 4), ps < len);
  };
  auto stage_store = [&](int buf, const float4& q4, const float4& d4, const float4& s4) {
    float* Qs = smem + buf * Sh::BUF;
    if (stager) {
      *reinterpret_cast<float4*>(&Qs[sr * LD + 4 * sf]) = q4;
      *reinterpret_cast<float4*>(&Qs[Sh::TILE + sr * LD + 4 * sf]) = d4;
    }
    if (tid < 32) *reinterpret_cast<float4*>(&Qs[2 * Sh::TILE + 4 * tid]) = s4;
  };
  float4 q4, d4, s4;
  stage_load(0, q4, d4, s4);

  float kf[DH / 2], vf[DH / 2];
  {
    const float* krow = qkv + (tok0 + (int64_t)(key_ok ? key : 0) * tstride) * ld3 + N + head * DH + 4 * hh;
#pragma unroll
    for (int m = 0; m < DH / 8; ++m) {
      float4 k4 = *reinterpret_cast<const float4*>(krow + 8 * m);
      float4 v4 = *reinterpret_cast<const float4*>(krow + N + 8 * m);
      if (!key_ok) k4 = v4 = make_float4(0.f, 0.f, 0.f, 0.f);
      kf[4 * m + 0] = k4.x; kf[4 * m + 1] = k4.y; kf[4 * m + 2] = k4.z; kf[4 * m + 3] = k4.w;
      vf[4 * m + 0] = v4.x; vf[4 * m + 1] = v4.y; vf[4 * m + 2] = v4.z; vf[4 * m + 3] = v4.w;
    }
  }
  stage_store(0, q4, d4, s4);
  __syncthreads();
  f32x16 dk = zero16(), dv = zero16();
  for (int qb = 0; qb < nqb; ++qb) {
    if (qb + 1 < nqb) stage_load(qb + 1, q4, d4, s4);
    const float* Qs = smem + (qb & 1) * Sh::BUF;
    const float* Ds = Qs + Sh::TILE;
    const float4* St = reinterpret_cast<const float4*>(Qs + 2 * Sh::TILE);
    f32x16 s2 = zero16(), dp2 = zero16();
    const float* qrow = Qs + c * LD + 4 * hh;
    const float* drow = Ds + c * LD + 4 * hh;
#pragma unroll
    for (int m = 0; m < DH / 8; ++m) {
      const float4 qq4 = *reinterpret_cast<const float4*>(qrow + 8 * m);
      const float4 dd4 = *reinterpret_cast<const float4*>(drow + 8 * m);
      s2 = mfma32(qq4.x, kf[4 * m + 0], s2);
      s2 = mfma32(qq4.y, kf[4 * m + 1], s2);
      s2 = mfma32(qq4.z, kf[4 * m + 2], s2);
      s2 = mfma32(qq4.w, kf[4 * m + 3], s2);
      dp2 = mfma32(dd4.x, vf[4 * m + 0], dp2);
      dp2 = mfma32(dd4.y, vf[4 * m + 1], dp2);
      dp2 = mfma32(dd4.z, vf[4 * m + 2], dp2);
      dp2 = mfma32(dd4.w, vf[4 * m + 3], dp2);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = ROW32(r, hh);
      const float4 st4 = St[qi];               // rows beyond len: zeros -> p2 = 0
      const float pexp = fast_exp2(s2[r] * sl2e - st4.x) * st4.y;
      const float p2 = key_ok ? pexp : 0.f;
      float keep = drop.inv_keep;
      if (dropping) keep = drop_keep(__float_as_uint(st4.w), (uint32_t)key, drop.thresh) ? keep : 0.f;
      const float pd = p2 * keep;                              // dropped P (feeds dV)
      const float ds = p2 * (dp2[r] * keep - st4.z);           // dS
      const float qv = Qs[qi * LD + (c < DH ? c : 0)], dv_ = Ds[qi * LD + (c < DH ? c : 0)];
      dv = mfma32(pd, c < DH ? dv_ : 0.f, dv);
      dk = mfma32(ds, c < DH ? qv : 0.f, dk);
    }
    if (qb + 1 < nqb) stage_store((qb + 1) & 1, q4, d4, s4);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int pk = kb * 32 + ROW32(r, hh);
    if (pk < len && c < DH) {
      float* row = dqkv + (tok0 + (int64_t)pk * tstride) * ld3 + head * DH + c;
      row[N] = dk[r] * scale;
      row[2 * N] = dv[r];
    }
  }
}
