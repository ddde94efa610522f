// The end of a pick, once, for the kernels that choose the next token (argmax_final_kernel in llm_k.hip, argmax_p2p_kernel in
// p2p.hip, sample_final_kernel in sample_k.hip, beam_merge_kernel in beam_k.hip): the (value, id) arg-max order and its reductions,
// the commit of the token to the device-side decode state, and the embedding-row copy for the next step.
#pragma once
#include "common.h"
#include "../../include/usdm_hip.h"

constexpr int PICK_NO_ID = 0x7fffffff;   // the id of "no candidate" (with value -inf): loses against every real (value, id)

// arg-max order: the larger value, among equal values the lower id (= torch.argmax).  NaN never wins
__device__ __forceinline__ bool pick_better(float v, int id, float bv, int bi) { return v > bv || (v == bv && id < bi); }

// the best pair of the wave, in every lane
__device__ __forceinline__ void pick_wave_best(float& v, int& id) {
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(id, off, 64);
    if (pick_better(ov, oi, v, id)) { v = ov; id = oi; }
  }
}

// the best pair of a workgroup of NT threads (a power of two), one pair per thread, through sv[NT] / si[NT] in LDS: the result is in
// sv[0] / si[0] behind the last barrier
template <int NT>
__device__ __forceinline__ void pick_block_best(float* sv, int* si, float v, int id) {
  const int tid = threadIdx.x;
  sv[tid] = v; si[tid] = id;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s && pick_better(sv[tid + s], si[tid + s], sv[tid], si[tid])) { sv[tid] = sv[tid + s]; si[tid] = si[tid + s]; }
    __syncthreads();
  }
}

// One thread commits token `tok` (id_offset already added) as output `step` of sequence b: the token fed to the next step, the
// output row, the counters, and the device-side EOS: eos = {count, min_new, ids...} -> done[b]
__device__ __forceinline__ void pick_commit(const usdm_decode_state& st, int b, int step, int tok) {
  st.next_token[b] = tok;
  if (step < st.max_out) st.out_tokens[(int64_t)b * st.max_out + step] = tok;
  st.step[b] = step + 1;
  if (st.advance_pos) st.pos[b] = st.pos[b] + 1;
  if (st.done && st.eos) {
    const int n = st.eos[0], mn = st.eos[1];
    bool hit = false;
    for (int i = 0; i < n && i < 6; ++i) hit |= (st.eos[2 + i] == tok);
    if (hit && step + 1 >= mn) st.done[b] = 1;
  }
}

// dst[0 : Hd] = E[tok] by the whole workgroup of NT threads, 16 bytes per thread and turn (Hd % 8 == 0): the fused nn.Embedding
// lookup of the token the next decode step consumes
template <int NT>
__device__ __forceinline__ void pick_embed_row(const bf16_t* E, int tok, int Hd, bf16_t* dst_row) {
  const u32x4* src = (const u32x4*)(E + (int64_t)tok * Hd);
  u32x4* dst = (u32x4*)dst_row;
  for (int i = threadIdx.x; i < Hd / 8; i += NT) dst[i] = src[i];
}
