// The f32 logits row of one sequence as the pick kernels (sample_k.hip, logprob_k.hip, penalty_k.hip, edit_k.hip, and through logprob_row.h
// score_k.hip and beam_k.hip) address it, plus the host-side checks of its shape.
//
// SEG = false: the row is contiguous, id i sits at row[i].  SEG = true: it is made of rank-major segments of seg_len ids, seg_stride
// elements apart (the *_seg entry points; under tensor parallelism every rank's lm_head slice is one segment); id i sits at
// (i / seg_len) * seg_stride + i % seg_len, the quotient by a multiply-high with magic = ceil(2^32 / seg_len) and one correction
// (exact for i, seg_len < 2^20).  Every kernel that reads a row through this view computes per-id quantities from the id's value only
// and sums them as integers, so both forms give bit-identical results on the same logical row.
#pragma once
#include "common.h"

__device__ __forceinline__ unsigned fkey(float x) {   // order-preserving float -> uint
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct logits_row_view {   // built inside the kernel from its three scalar parameters (all unused when SEG = false)
  int64_t seg_stride;
  int seg_len;
  unsigned seg_magic;
};

// where id i (0 <= i < V) sits (P = const float*, or float* for a kernel that writes in place)
template <bool SEG, typename P>
__device__ __forceinline__ P row_ptr(P row, int i, const logits_row_view& v) {
  if constexpr (SEG) {
    unsigned q = __umulhi((unsigned)i, v.seg_magic);
    if (q * (unsigned)v.seg_len > (unsigned)i) --q;
    return row + ((int64_t)q * v.seg_stride + (i - (int)q * v.seg_len));
  } else {
    return row + i;
  }
}

template <bool SEG>
__device__ __forceinline__ float row_at(const float* row, int i, const logits_row_view& v) { return *row_ptr<SEG>(row, i, v); }   // logit of id i

// f(i, pointer to id i) for i = tid, tid + NT, ... < V (P = const float*, or float* for a kernel that writes in place).  The segmented
// form divides once and then walks a pointer, stepping over the gap between two segments when it crosses one (seg_len >= NT: at most
// one step per iteration)
template <bool SEG, int NT, typename P, typename F>
__device__ __forceinline__ void row_each(P row, int V, int tid, const logits_row_view& v, F&& f) {
  if constexpr (SEG) {
    unsigned q = __umulhi((unsigned)tid, v.seg_magic);
    if (q * (unsigned)v.seg_len > (unsigned)tid) --q;
    int r = tid - (int)q * v.seg_len;
    P ptr = row + (int64_t)q * v.seg_stride + r;
    for (int i = tid; i < V; i += NT) {
      f(i, ptr);
      ptr += NT; r += NT;
      while (r >= v.seg_len) { r -= v.seg_len; ptr += v.seg_stride - v.seg_len; }
    }
  } else {
    for (int i = tid; i < V; i += NT) f(i, row + i);
  }
}

// ---- host side ---------------------------------------------------------------------------------
inline int logits_rows(int batch) { return batch > 1 ? batch : 1; }   // workgroups = sequences: usdm_decode_state::batch 0 means one

inline unsigned logits_seg_magic(int seg_len) { return (unsigned)((((uint64_t)1 << 32) + (uint64_t)seg_len - 1) / (uint64_t)seg_len); }

// the segments of a *_seg entry point: nseg of seg_len ids hold ids 0 .. V-1, and the nb rows (logits_bs apart) of one segment end
// before the next segment begins
inline int check_logits_seg(const char* who, int nseg, int64_t seg_stride, int seg_len, int V, int64_t logits_bs, int nb) {
  USDM_CHECK_ARG(nseg >= 1 && seg_len >= 2 && seg_len <= (1 << 20) && (int64_t)nseg * seg_len >= V,
                 "%s: nseg segments of seg_len ids must cover V", who);
  USDM_CHECK_ARG(nseg == 1 || seg_stride >= logits_bs * (nb - 1) + seg_len, "%s: segments overlap", who);
  return 0;
}
