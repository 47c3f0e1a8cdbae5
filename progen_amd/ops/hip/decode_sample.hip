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
// reduction still ends and the token stays inside [0, V). The body is in
// decode_sample_body.h, shared with the slot kernel.

#include "common.h"
#include "decode_sample_body.h"
#include "decode_sample_kernels.h"

template <bool BF>
__global__ __launch_bounds__(256) void dec_sample_kernel(
    const void* __restrict__ logits, const long long* __restrict__ pos_ptr,
    const long long* __restrict__ seed_ptr, long long* seq,
    const long long* __restrict__ lens, long long* pads, long long* token,
    float* __restrict__ u_out, int V, int L, int top_k, bool greedy) {
  dec_sample_body<BF, false>(logits, pos_ptr, seed_ptr, seq, lens, pads, token,
                             u_out, nullptr, nullptr, V, L, top_k, greedy);
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
