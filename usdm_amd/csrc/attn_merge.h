// The merge of the context-split decode-attention partials (pm, pl, po of usdm_attn_decode_args), once, for its three sites:
// attn_combine_kernel and the last-arriver merge of attn_decode_kernel (llm_attn_k.hip) and the CMB prologue of gemv_kernel
// (llm_k.hip).  Split s of a head carries its score maximum m_s, its sum l_s of exp(score - m_s) and its unnormalised output o_s:
//   e_s = exp(m_s - max m),  out = sum_s o_s e_s / sum_s l_s e_s.
// The sites differ in how they load (plain loads, or agent-scope loads of partials other workgroups have just written) and in how
// many loads they keep in flight; both come in as parameters, so the three results are equal bit for bit
// (tests/test_llm_gpu.py::test_split_merges_agree_bit_for_bit).  The MRG prologue of gemv_kernel sums in another order (fma, four
// elements per thread) and is not built on this.
#pragma once
#include "common.h"

namespace {
// The weights of one head.  Called by lanes 0..63 of ONE wave; ldm(s) / ldl(s) load m_s / l_s (NS <= 64 splits).  Leaves e_s in
// w[0..63] (0 past NS) and returns 1 / sum_s l_s e_s on every lane.
template <class LDM, class LDL>
__device__ __forceinline__ float attn_merge_weights(int NS, int lane, float* w, LDM ldm, LDL ldl) {
  const float mv = lane < NS ? ldm(lane) : -1e30f;
  const float m = wave_max(mv);
  const float e = lane < NS ? __expf(mv - m) : 0.f;
  const float l = wave_sum(lane < NS ? ldl(lane) * e : 0.f);
  w[lane] = e;
  return 1.0f / l;
}

// one group of four splits: the association every site shares
__device__ __forceinline__ float attn_merge_four(float a0, float a1, float a2, float a3, const float* w) {
  return (a0 * w[0] + a1 * w[1]) + (a2 * w[2] + a3 * w[3]);
}

// The weighted sum of one output element over the NS partials, in split order: ld(s) loads o_s, w is attn_merge_weights'.  o takes one
// group of four at a time, then a scalar tail.  NF = 4: the four loads of a group are in flight together.  NF = 16 (the fused merge,
// whose agent-scope loads each pay a trip to memory): sixteen loads are requested before the first group is summed, while sixteen
// splits are left.  The association does not depend on NF.
template <int NF, class LD>
__device__ __forceinline__ float attn_merge_sum(int NS, const float* w, LD ld) {
  static_assert(NF % 4 == 0, "whole groups of four in flight");
  float o = 0.f;
  int s = 0;
  if constexpr (NF > 4) {
#pragma unroll 1   // NF in flight, not a multiple of it
    for (; s + NF <= NS; s += NF) {
      float pv[NF];
#pragma unroll
      for (int u = 0; u < NF; ++u) pv[u] = ld(s + u);
#pragma unroll
      for (int u = 0; u < NF; u += 4) o += attn_merge_four(pv[u], pv[u + 1], pv[u + 2], pv[u + 3], w + s + u);
    }
  }
  for (; s + 4 <= NS; s += 4) {
    const float a0 = ld(s), a1 = ld(s + 1), a2 = ld(s + 2), a3 = ld(s + 3);
    o += attn_merge_four(a0, a1, a2, a3, w + s);
  }
  for (; s < NS; ++s) o += ld(s) * w[s];
  return o;
}
}  // namespace
