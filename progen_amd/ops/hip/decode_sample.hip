// Decode-step sampler: picks the next token of every row on the device, so
// a captured decode step can feed itself (progen_amd/decode.py).
//
//   w = pos + 1                      the position the token is written to
//   t = logits[b] as fp32
//   greedy:  sampled = argmax_j t_j
//   else:    u_j     = Philox4x32-10(key = seed, counter = (j / 4, w, b, 0))
//                      word j % 4, top 24 bits, in [0, 1)
//            g_j     = -log(-log(u_j + 1e-20) + 1e-20)
//            sel_j   = top_k == 0 or #{i : t_i >= t_j} < top_k
//            sampled = argmax_j (sel_j ? t_j + g_j : 0), lowest j on ties
//   if w >= lens[b]: seq[b, w] <- sampled       (else the prime token stays)
//   pads[b] += (seq[b, w] == 0);  token[b] <- seq[b, w]
//
// The count form of sel is reference.select_top_k's strict "greater than the
// k-th largest value": ties at the threshold select fewer than k entries and
// k = 1 selects none. An entry that is not selected scores exactly 0, not
// -inf, so it wins whenever every selected score is negative.
//
// Grid: B workgroups of 256 threads, one row each. The row is staged in LDS
// as fp32, padded with -inf to 1024 entries; thread i owns entries 4i..4i+3,
// which are the four words of Philox block i, and counts their rank against
// the whole row with broadcast 16 B LDS reads. The generator is stateless,
// so a replayed graph needs no generator state: the position in the counter
// is what moves. Both logs are the accurate logf: the fast intrinsic has no
// relative accuracy near 1, where the largest noise values come from. A
// workgroup reads and writes only row b of every tensor. ``pos`` is read
// from device memory; with pos < 0 or w >= L the block returns before it
// touches anything else. Non-finite logits are outside the contract; the
// reduction still ends and the token stays inside [0, V).

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

template <bool BF>
__global__ __launch_bounds__(256) void dec_sample_kernel(
    const void* __restrict__ logits, const long long* __restrict__ pos_ptr,
    const long long* __restrict__ seed_ptr, long long* seq,
    const long long* __restrict__ lens, long long* pads, long long* token,
    float* __restrict__ u_out, int V, int L, int top_k, bool greedy) {
  __shared__ __attribute__((aligned(16))) float row[DEC_SAMPLE_MAX_V];
  __shared__ float red_s[4];
  __shared__ int red_i[4];

  const long long pos = *pos_ptr;
  const long long w = pos + 1;
  if (pos < 0 || w >= L) return;  // uniform: before any barrier

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
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
    const unsigned long long seed = (unsigned long long)*seed_ptr;
    unsigned x[4];
    philox4x32_10((unsigned)tid, (unsigned)w, (unsigned)b, 0u,
                  (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float u = (float)(x[e] >> 8) * 5.9604644775390625e-8f;  // 2^-24
      if (u_out != nullptr && j0 + e < V) u_out[lrow + j0 + e] = u;
      score[e] = t[e] + -logf(-logf(u + 1e-20f) + 1e-20f);
    }
  }

  if (!greedy && top_k > 0) {
    __syncthreads();  // uniform condition: greedy and top_k are arguments
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
    if (w >= lens[b]) *slot = tok;
    else tok = *slot;
    pads[b] += (tok == 0);
    token[b] = tok;
  }
}

extern "C" hipError_t dec_sample_launch(const void* logits,
                                        const long long* pos,
                                        const long long* seed, long long* seq,
                                        const long long* lens, long long* pads,
                                        long long* token, float* u_out, int B,
                                        int V, int L, int top_k, bool greedy,
                                        bool is_bf16, hipStream_t stream) {
  if (is_bf16)
    dec_sample_kernel<true><<<B, 256, 0, stream>>>(
        logits, pos, seed, seq, lens, pads, token, u_out, V, L, top_k, greedy);
  else
    dec_sample_kernel<false><<<B, 256, 0, stream>>>(
        logits, pos, seed, seq, lens, pads, token, u_out, V, L, top_k, greedy);
  return hipGetLastError();
}
