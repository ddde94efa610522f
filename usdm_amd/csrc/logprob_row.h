// The per-row passes of the log-probability kernels, once: prompt_logprob_kernel (score_k.hip) and beam_row_kernel (beam_k.hip) call
// them on one f32 logits row, read through logits_row.h's view, with one workgroup of LPR_NT threads.  They are logprob_kernel's
// (logprob_k.hip) passes, term for term; that kernel keeps a body of its own for the reason its header gives, and a fix to this
// arithmetic is made in both files.
//
//   lpr_sum      pass 1  max, and optionally how many ids beat a target              (registers, wave reductions)
//                pass 2  sum of exp(x - max) as a 2^40 FIXED-POINT integer sum       (associative: no dependence on thread scheduling)
//   lpr_lse      -> lp(x) = x - logsumexp(x): banned ids (-inf) are zero mass
//   lpr_select   radix select, 8 bits per pass, of the K-th largest COMPOSITE key (order key of val(x)) << 24 | (2^24-1 - id): keys
//                are unique, so the selection is exact and ties need no special case.  The select stops at the first pass whose
//                boundary bin is needed whole (2 passes when the K-th value is untied, up to 7 when exact ties straddle it)
//   lpr_collect  collect the kept keys, order them by counting
// Histogram bins are replicated 32 times (lane % 32): a pass whose keys share a few bins (the exponent byte) would otherwise serialise
// 64 LDS atomics per wave instruction on one address.  Every sum is an integer sum and every per-id quantity depends on the id's
// value only, so the same logical row gives bit-identical output in every caller, contiguous or segmented.
//
// Each kernel keeps its prologue (row address, early returns, target, score) and its stores; the __shared__ block is declared in the
// kernel and passed in.  The kernel also chooses when Z is read: the log-probability kernel ranks the logit and reads Z behind the
// select's barriers, the beam row ranks score + lp(x) and needs Z (behind a barrier of its own) before its select.
#pragma once
#include "logits_row.h"

constexpr int LPR_NT = 1024, LPR_NW = LPR_NT / 64, LPR_REP = 32;

template <int KCAP>   // KCAP: capacity of the candidate array (the largest K of the kernel)
struct lpr_shared {
  unsigned hist[256 * LPR_REP];
  unsigned long long cand[KCAP];
  float sredf[LPR_NW];
  unsigned sredu[LPR_NW];
  unsigned long long s_z, s_prefix;
  unsigned s_rem, s_cnt, s_n;
};

__device__ __forceinline__ float fkey_inv(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
// composite key of (id, value): larger = better, then lower id.  -0.0 is folded into +0.0 first (equal values must tie)
__device__ __forceinline__ unsigned long long ckey(int i, float x) {
  return ((unsigned long long)fkey(x + 0.0f) << 24) | (unsigned long long)(0xFFFFFFu - (unsigned)i);
}

struct lpr_lse_t {   // the row's max and Z = sum exp(x - max) * 2^40
  float m;
  unsigned long long Z;
  double logZ;
  __device__ __forceinline__ float lp(float x) const {   // banned / empty row: -inf, never NaN; NaN only from a NaN logit
    if (x == -INFINITY || Z == 0) return -INFINITY;
    return (float)((double)(x == m ? 0.f : x - m) - logZ);
  }
};

// f(i, logit of i) for i = tid, tid + LPR_NT, ... < V
template <bool SEG, typename F>
__device__ __forceinline__ void lpr_each(const float* row, int V, const logits_row_view& rv, F&& f) {
  row_each<SEG, LPR_NT>(row, V, (int)threadIdx.x, rv, [&](int i, const float* px) { f(i, *px); });
}

// Passes 1 and 2: returns the row's max.  RANK: also count the ids whose logit is strictly greater than xt into gt (both unused
// otherwise).  Z is complete in sh behind the caller's next barrier; also zeroes the counter of lpr_collect.
template <bool SEG, bool RANK, int KCAP>
__device__ __forceinline__ float lpr_sum(const float* row, int V, const logits_row_view& rv, lpr_shared<KCAP>& sh, float xt, unsigned& gt) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // ---- pass 1: max, and how many ids beat the target
  float m = -INFINITY;
  gt = 0;
  lpr_each<SEG>(row, V, rv, [&](int, float x) {
    m = fmaxf(m, x);
    if constexpr (RANK) gt += x > xt;
  });
  m = wave_max(m);
  if constexpr (RANK)
    for (int off = 32; off > 0; off >>= 1) gt += __shfl_xor(gt, off, 64);
  if (lane == 0) {
    sh.sredf[wv] = m;
    if constexpr (RANK) sh.sredu[wv] = gt;
  }
  if (tid == 0) { sh.s_z = 0; sh.s_n = 0; }
  __syncthreads();
  m = sh.sredf[0];
  if constexpr (RANK) gt = sh.sredu[0];
  for (int w = 1; w < LPR_NW; ++w) {
    m = fmaxf(m, sh.sredf[w]);
    if constexpr (RANK) gt += sh.sredu[w];
  }

  // ---- pass 2: Z = sum exp(x - max) in 2^40 fixed point (each term <= 2^40, V <= 2^20: no overflow)
  unsigned long long z = 0;
  lpr_each<SEG>(row, V, rv, [&](int, float x) {
    const float e = x == -INFINITY ? 0.f : expf(x == m ? 0.f : x - m);
    z += e == e ? (unsigned long long)((double)e * 1099511627776.0) : 0ull;      // (a NaN logit: no conversion of NaN)
  });
  unsigned lo = (unsigned)z, hi = (unsigned)(z >> 32);
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = ((unsigned long long)__shfl_xor(hi, off, 64) << 32) | __shfl_xor(lo, off, 64);
    z += o;
    lo = (unsigned)z; hi = (unsigned)(z >> 32);
  }
  if (lane == 0) atomicAdd(&sh.s_z, z);
  return m;
}

// behind a barrier after lpr_sum
template <int KCAP>
__device__ __forceinline__ lpr_lse_t lpr_lse(const lpr_shared<KCAP>& sh, float m) {
  const unsigned long long Z = sh.s_z;
  return lpr_lse_t{m, Z, log((double)Z) - 40.0 * 0.69314718055994530942};
}

struct lpr_cut {   // kept: (key & keep) >= kth; {0, 0} keeps everything (V <= K)
  unsigned long long kth, keep;
};

// The K-th largest composite key of val(logit) over the row, 0 < K < V.  Begins and ends with barriers.
template <bool SEG, int KCAP, typename VAL>
__device__ __forceinline__ lpr_cut lpr_select(const float* row, int V, int K, const logits_row_view& rv, lpr_shared<KCAP>& sh, VAL&& val) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned long long prefix = 0, mask = 0;
  unsigned rem = (unsigned)K;
  for (int shift = 48; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256 * LPR_REP; i += LPR_NT) sh.hist[i] = 0;
    __syncthreads();
    lpr_each<SEG>(row, V, rv, [&](int i, float x) {
      const unsigned long long c = ckey(i, val(x));
      if ((c & mask) == prefix) atomicAdd(&sh.hist[(unsigned)((c >> shift) & 255) * LPR_REP + (tid & (LPR_REP - 1))], 1u);
    });
    __syncthreads();
    // thread d < 256 owns digit d: its count, then the suffix sum over the digits >= d (descending keys come first)
    unsigned tot = 0;
    if (tid < 256)
      for (int r = 0; r < LPR_REP; ++r) tot += sh.hist[tid * LPR_REP + ((r + tid) & (LPR_REP - 1))];
    unsigned incl = tot;
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned o = __shfl_down(incl, off, 64);
      if (lane + off < 64) incl += o;
    }
    if (lane == 0) sh.sredu[wv] = incl;
    __syncthreads();
    for (int w = wv + 1; w < 4; ++w) incl += sh.sredu[w];
    if (tid < 256 && incl >= rem && incl - tot < rem) {   // the K-th key has digit tid here: exactly one thread
      sh.s_prefix = prefix | ((unsigned long long)tid << shift);
      sh.s_rem = rem - (incl - tot);
      sh.s_cnt = tot;
    }
    __syncthreads();
    prefix = sh.s_prefix; rem = sh.s_rem; mask |= 255ull << shift;
    const bool whole = sh.s_cnt == rem;   // every key of the boundary bin is kept: no need to look inside it
    __syncthreads();
    if (whole) break;
  }
  return lpr_cut{prefix, mask};
}

// The keys that pass the cut (at most KCAP are held), ordered by counting: calls emit(r, id, value) for r = 0 .. n-1 in descending
// order, one thread each, and returns n = min(K, V).
template <bool SEG, int KCAP, typename VAL, typename EMIT>
__device__ __forceinline__ int lpr_collect(const float* row, int V, int K, const logits_row_view& rv, lpr_shared<KCAP>& sh, lpr_cut cut,
                                           VAL&& val, EMIT&& emit) {
  const int tid = threadIdx.x;
  lpr_each<SEG>(row, V, rv, [&](int i, float x) {
    const unsigned long long c = ckey(i, val(x));
    if ((c & cut.keep) >= cut.kth) {
      const unsigned s = atomicAdd(&sh.s_n, 1u);
      if (s < KCAP) sh.cand[s] = c;
    }
  });
  __syncthreads();
  const int n = min((int)sh.s_n, K);
  if (tid < n) {
    const unsigned long long c = sh.cand[tid];
    int r = 0;
    for (int j = 0; j < n; ++j) r += sh.cand[j] > c;   // keys are unique: a permutation of 0 .. n-1
    emit(r, (int)(0xFFFFFFu - (unsigned)(c & 0xFFFFFFu)), fkey_inv((unsigned)(c >> 24)));
  }
  return n;
}
