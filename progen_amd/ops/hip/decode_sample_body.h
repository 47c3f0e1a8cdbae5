// Body of the decode-step sampler (decode_sample.hip), written once for the
// scalar kernel and for the slot kernel (decode_slots.hip).
//
// SLOTS = false: one position *pos_ptr, one seed, top_k and greedy for every
//                row; Philox counter (j / 4, w, b, 0); ``lens`` holds the
//                prime lengths. ``ctl`` and ``pos_out`` are not read.
// SLOTS = true:  row b runs at pos_ptr[b] under its own controls
//                ctl[b] = [len, limit, top_k, seed, stream]: greedy when
//                seed < 0, Philox counter (j / 4, w, stream, 0) under the key
//                seed. pos_ptr[b] < 0 is an idle row and nothing of it is
//                touched. The row also advances or retires itself:
//                pos_out[b] <- -1 once it has two pads or has written
//                position limit - 1, else w. With w >= limit (or L) on entry
//                it retires and touches nothing else. ``seed_ptr``, ``lens``,
//                ``top_k`` and ``greedy`` are not read.
#pragma once

#include <climits>

#include "common.h"
#include "decode_sample_kernels.h"

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1,
                                              unsigned c2, unsigned c3,
                                              unsigned k0, unsigned k1,
                                              unsigned* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const unsigned hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// (score, index) argmax step: the larger score, the lower index on a tie. A
// NaN never displaces anything and is never displaced.
__device__ __forceinline__ void take_better(float& s, int& i, float s2,
                                            int i2) {
  if (s2 > s || (s2 == s && i2 < i)) {
    s = s2;
    i = i2;
  }
}

template <bool BF, bool SLOTS>
__device__ __forceinline__ void dec_sample_body(
    const void* __restrict__ logits, const long long* pos_ptr,
    const long long* __restrict__ seed_ptr, long long* seq,
    const long long* __restrict__ lens, long long* pads, long long* token,
    float* __restrict__ u_out, const long long* __restrict__ ctl,
    long long* pos_out, int V, int L, int top_k, bool greedy) {
  __shared__ __attribute__((aligned(16))) float row[DEC_SAMPLE_MAX_V];
  __shared__ float red_s[4];
  __shared__ int red_i[4];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const long long pos = SLOTS ? pos_ptr[b] : *pos_ptr;
  const long long w = pos + 1;
  long long len = 0, limit = L, seed_v = 0;
  unsigned stream = (unsigned)b;
  if (SLOTS) {
    if (pos < 0) return;  // idle: uniform, before any barrier
    const long long* c = ctl + (long long)b * 5;
    len = c[0];
    limit = c[1];
    if (w >= limit || w >= L) {  // uniform: before any barrier
      // a wave that loads pos_ptr[b] (the same address) only after this
      // store sees -1 and takes the idle return above: either way it writes
      // nothing and has passed no barrier
      if (tid == 0) pos_out[b] = -1;
      return;
    }
    // above V nothing is masked, as with 0; the clamp keeps the narrowing safe
    const long long k = c[2];
    top_k = k <= 0 ? 0 : (k > V ? V + 1 : (int)k);
    seed_v = c[3];
    greedy = seed_v < 0;
    stream = (unsigned)c[4];
  } else {
    if (pos < 0 || w >= L) return;  // uniform: before any barrier
  }

  const int wave = tid >> 6, lane = tid & 63;
  const long long lrow = (long long)b * V;
  const int j0 = tid * 4;
  const float ninf = -__builtin_inff();

  float t[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    t[e] = j0 + e < V ? ld1<BF>(logits, lrow + j0 + e) : ninf;
    row[j0 + e] = t[e];
  }

  float score[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) score[e] = t[e];

  if (!greedy && j0 < V) {  // 4 * tid < V: this thread's Philox block is live
    const unsigned long long seed =
        (unsigned long long)(SLOTS ? seed_v : *seed_ptr);
    unsigned x[4];
    philox4x32_10((unsigned)tid, (unsigned)w, stream, 0u,
                  (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float u = (float)(x[e] >> 8) * 5.9604644775390625e-8f;  // 2^-24
      if (u_out != nullptr && j0 + e < V) u_out[lrow + j0 + e] = u;
      score[e] = t[e] + -logf(-logf(u + 1e-20f) + 1e-20f);
    }
  }

  if (!greedy && top_k > 0) {
    __syncthreads();  // uniform condition: one value per workgroup
    if (j0 < V) {
      int cnt[4] = {0, 0, 0, 0};
      const int nblk = (V + 3) >> 2;
      for (int i = 0; i < nblk; ++i) {
        const f32x4 r = *(const f32x4*)&row[i * 4];  // same address: broadcast
#pragma unroll
        for (int e = 0; e < 4; ++e)
          cnt[e] += (r[0] >= t[e]) + (r[1] >= t[e]) + (r[2] >= t[e]) +
                    (r[3] >= t[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (cnt[e] >= top_k) score[e] = 0.f;
    }
  }

  // ---- argmax over (score, index) -----------------------------------------
  float bs = score[0];
  int bi = j0;
#pragma unroll
  for (int e = 1; e < 4; ++e)
    if (j0 + e < V) take_better(bs, bi, score[e], j0 + e);
  if (j0 >= V) {  // no live entry: lose to every real one
    bs = ninf;
    bi = INT_MAX;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float s2 = __shfl_xor(bs, off, 64);
    const int i2 = __shfl_xor(bi, off, 64);
    take_better(bs, bi, s2, i2);
  }
  if (lane == 0) {
    red_s[wave] = bs;
    red_i[wave] = bi;
  }
  __syncthreads();

  if (tid == 0) {
#pragma unroll
    for (int v = 1; v < 4; ++v) take_better(bs, bi, red_s[v], red_i[v]);
    long long tok = bi < V ? bi : V - 1;
    long long* slot = seq + (long long)b * L + w;
    if (w >= (SLOTS ? len : lens[b])) *slot = tok;
    else tok = *slot;
    const long long np = pads[b] + (tok == 0);
    pads[b] = np;
    token[b] = tok;
    if (SLOTS) pos_out[b] = (np >= 2 || w + 1 >= limit) ? -1 : w;
  }
}
