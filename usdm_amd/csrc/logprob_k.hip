// Per-token log-probabilities of the LLM decode step, on the device: the row the sampler just drew from never leaves the GPU and the
// step stays one hipGraph.  usdm_logprobs runs AFTER the pick (usdm_sample_final) of the same step, on the same ban-masked f32 row.
//
// Definition: lp(i) = x_i - logsumexp(x) over ids 0 .. V-1 of that row, banned ids (-inf) included as zero mass.  This is the MODEL's
// distribution over the allowed ids, BEFORE temperature, top-k and top-p: it does not depend on the request's sampling knobs (vLLM
// versions differ: "raw_logprobs" is this one, "processed_logprobs" the other).  Rank = 1 + number of ids whose logit is strictly
// greater than the picked one (vLLM's rank); the top K ids in descending log-probability, exact ties by lowest id first.
//
// One workgroup of 1024 threads per sequence, passes over the V logits (L2-resident, 168 KB at V = 42003):
//   1  max and rank count          (registers, wave reductions)
//   2  sum of exp(x - max)         as a 2^40 FIXED-POINT integer sum (associative: no dependence on thread scheduling)
//   3+ top K (K > 0, V > K)        radix select, 8 bits per pass, of the K-th largest COMPOSITE key (order key of x) << 24 | (2^24-1 - id):
//                                  keys are unique, so the selection is exact and ties need no special case.  The select stops at the
//                                  first pass whose boundary bin is needed whole (2 passes when the K-th value is untied, up to 7 when exact ties straddle it)
//   last collect the <= 20 kept keys, order them by counting, write the row
// Histogram bins are replicated 32 times (lane % 32): a pass whose keys share a few bins (the exponent byte) would otherwise
// serialise 64 LDS atomics per wave instruction on one address.  Every sum is an integer sum and every per-id quantity depends on the
// id's value only, so the same logical row gives bit-identical output run to run, single or batched, contiguous or segmented
// (logits_row.h).
//
// The row body below is this kernel's OWN: usdm_prompt_logprobs (score_k.hip) and usdm_beam_step (beam_k.hip) run the same passes
// from logprob_row.h, and a fix to this arithmetic is made there AND here.  This kernel, written over that header, has the same
// instructions in its loops, no scratch, the same LDS and 79 / 82 VGPRs (here: 82 / 82), but at K = 0 it measured 0.1 - 0.3 us
// per launch slower than this form (18.3 - 18.6 against 18.0 - 18.4 us at one row, 19.2 - 19.3 against 19.0 - 19.1 us at 16), outside
// this form's own spread, and it sits inside every captured log-probability step: profiles/pick_share.txt has the numbers.
// tests/test_score_gpu.py and tests/test_beam_gpu.py pin the shared passes to this kernel's bits.
#include "logits_row.h"
#include "../../include/usdm_hip.h"

namespace {
constexpr int NT = 1024, NW = NT / 64, REP = 32, KMAX = 20;

__device__ __forceinline__ float fkey_inv(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
// composite key of (id, logit): larger = more likely, then lower id.  -0.0 is folded into +0.0 first (equal values must tie)
__device__ __forceinline__ unsigned long long ckey(int i, float x) {
  return ((unsigned long long)fkey(x + 0.0f) << 24) | (unsigned long long)(0xFFFFFFu - (unsigned)i);
}

template <bool SEG>
__global__ __launch_bounds__(NT) void logprob_kernel(usdm_logprob_args a, usdm_decode_state st, int64_t seg_stride, int seg_len,
                                                     unsigned seg_magic) {
  __shared__ unsigned hist[256 * REP];
  __shared__ unsigned long long cand[KMAX];
  __shared__ float sredf[NW];
  __shared__ unsigned sredu[NW];
  __shared__ unsigned long long s_z, s_prefix;
  __shared__ unsigned s_rem, s_cnt, s_n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, V = a.V, K = a.K;
  const int b = blockIdx.x;
  a.logits += (int64_t)b * a.logits_bs;
  const int step = st.step[b];
  const int t = step - 1;   // the pick of this step has already advanced the counter: its row is step - 1
  // rows already written for this sequence: a replay after the device-side EOS (the pick returned early, step did not move) writes
  // nothing, while the step whose pick SET `done` still has step > count and writes its row
  if (a.count && a.count[b] >= step) return;
  if (t < 0 || t >= st.max_out) return;
  const int tok = st.next_token[b] - st.id_offset;
  const bool tok_ok = tok >= 0 && tok < V;

  const logits_row_view rv{seg_stride, seg_len, seg_magic};
  auto each = [&](auto&& f) {   // f(i, logit of i) for i = tid, tid + NT, ... < V
    row_each<SEG, NT>(a.logits, V, tid, rv, [&](int i, const float* px) { f(i, *px); });
  };

  // ---- pass 1: max, and how many ids beat the picked one
  const float xt = tok_ok ? row_at<SEG>(a.logits, tok, rv) : -INFINITY;
  float m = -INFINITY;
  unsigned gt = 0;
  each([&](int, float x) {
    m = fmaxf(m, x);
    gt += x > xt;
  });
  m = wave_max(m);
  for (int off = 32; off > 0; off >>= 1) gt += __shfl_xor(gt, off, 64);
  if (lane == 0) { sredf[wv] = m; sredu[wv] = gt; }
  if (tid == 0) { s_z = 0; s_n = 0; }
  __syncthreads();
  m = sredf[0]; gt = sredu[0];
  for (int w = 1; w < NW; ++w) { m = fmaxf(m, sredf[w]); gt += sredu[w]; }

  // ---- pass 2: Z = sum exp(x - max) in 2^40 fixed point (each term <= 2^40, V <= 2^20: no overflow)
  {
    unsigned long long z = 0;
    each([&](int, float x) {
      const float e = x == -INFINITY ? 0.f : expf(x == m ? 0.f : x - m);
      z += e == e ? (unsigned long long)((double)e * 1099511627776.0) : 0ull;      // (a NaN logit: no conversion of NaN)
    });
    unsigned lo = (unsigned)z, hi = (unsigned)(z >> 32);
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = ((unsigned long long)__shfl_xor(hi, off, 64) << 32) | __shfl_xor(lo, off, 64);
      z += o;
      lo = (unsigned)z; hi = (unsigned)(z >> 32);
    }
    if (lane == 0) atomicAdd(&s_z, z);
  }

  // ---- top K: the K-th largest composite key
  unsigned long long kth = 0, keep = 0;   // kept: (key & keep) >= kth; everything when V <= K
  if (K > 0 && V > K) {
    unsigned long long prefix = 0, mask = 0;
    unsigned rem = (unsigned)K;
    for (int shift = 48; shift >= 0; shift -= 8) {
      for (int i = tid; i < 256 * REP; i += NT) hist[i] = 0;
      __syncthreads();
      each([&](int i, float x) {
        const unsigned long long c = ckey(i, x);
        if ((c & mask) == prefix) atomicAdd(&hist[(unsigned)((c >> shift) & 255) * REP + (tid & (REP - 1))], 1u);
      });
      __syncthreads();
      // thread d < 256 owns digit d: its count, then the suffix sum over the digits >= d (descending keys come first)
      unsigned tot = 0;
      if (tid < 256)
        for (int r = 0; r < REP; ++r) tot += hist[tid * REP + ((r + tid) & (REP - 1))];
      unsigned incl = tot;
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_down(incl, off, 64);
        if (lane + off < 64) incl += o;
      }
      if (lane == 0) sredu[wv] = incl;
      __syncthreads();
      for (int w = wv + 1; w < 4; ++w) incl += sredu[w];
      if (tid < 256 && incl >= rem && incl - tot < rem) {   // the K-th key has digit tid here: exactly one thread
        s_prefix = prefix | ((unsigned long long)tid << shift);
        s_rem = rem - (incl - tot);
        s_cnt = tot;
      }
      __syncthreads();
      prefix = s_prefix; rem = s_rem; mask |= 255ull << shift;
      const bool whole = s_cnt == rem;   // every key of the boundary bin is kept: no need to look inside it
      __syncthreads();
      if (whole) break;
    }
    kth = prefix; keep = mask;
  } else {
    __syncthreads();
  }
  const unsigned long long Z = s_z;
  const double logZ = log((double)Z) - 40.0 * 0.69314718055994530942;
  auto LP = [&](float x) -> float {   // banned / empty row: -inf, never NaN; NaN only from a NaN logit
    if (x == -INFINITY || Z == 0) return -INFINITY;
    return (float)((double)(x == m ? 0.f : x - m) - logZ);
  };
  if (tid == 0) {
    a.tok_lp[(int64_t)b * a.tok_bs + t] = tok_ok ? LP(xt) : -INFINITY;
    a.tok_rank[(int64_t)b * a.tok_bs + t] = 1 + (int)gt;
    if (a.count) a.count[b] = step;
  }
  if (K > 0) {
    each([&](int i, float x) {
      const unsigned long long c = ckey(i, x);
      if ((c & keep) >= kth) {
        const unsigned s = atomicAdd(&s_n, 1u);
        if (s < KMAX) cand[s] = c;
      }
    });
    __syncthreads();
    const int n = min((int)s_n, K);
    int32_t* ids = a.top_id + (int64_t)b * a.top_bs + (int64_t)t * K;
    float* lps = a.top_lp + (int64_t)b * a.top_bs + (int64_t)t * K;
    if (tid < n) {
      const unsigned long long c = cand[tid];
      int r = 0;
      for (int j = 0; j < n; ++j) r += cand[j] > c;   // keys are unique: a permutation of 0 .. n-1
      ids[r] = (int)(0xFFFFFFu - (unsigned)(c & 0xFFFFFFu));
      lps[r] = LP(fkey_inv((unsigned)(c >> 24)));
    } else if (tid < K) {   // fewer ids than K
      ids[tid] = -1;
      lps[tid] = -INFINITY;
    }
  }
}

int check_logprobs(const usdm_logprob_args* pa, const usdm_decode_state* st, const char* who) {
  USDM_CHECK_ARG(pa && pa->logits && pa->V > 0 && pa->V <= (1 << 20), "%s: logits / V (1 .. 2^20)", who);
  USDM_CHECK_ARG(pa->K >= 0 && pa->K <= KMAX, "%s: K must be 0 .. 20", who);
  USDM_CHECK_ARG(pa->tok_lp && pa->tok_rank, "%s: tok_lp / tok_rank missing", who);
  USDM_CHECK_ARG(pa->K == 0 || (pa->top_id && pa->top_lp), "%s: top_id / top_lp missing with K > 0", who);
  USDM_CHECK_ARG(st && st->next_token && st->step && st->max_out > 0, "%s: decode state", who);
  USDM_CHECK_ARG(!st->done || pa->count, "%s: a state with a device-side `done` word needs the rows-written count", who);
  return 0;
}
}  // namespace

extern "C" int usdm_logprobs(const usdm_logprob_args* pa, const usdm_decode_state* st, usdm_stream_t stream) {
  if (int rc = check_logprobs(pa, st, "usdm_logprobs")) return rc;
  const int nb = logits_rows(st->batch);
  USDM_CHECK_ARG(nb == 1 || (pa->logits_bs >= pa->V && pa->tok_bs >= st->max_out && (pa->K == 0 || pa->top_bs >= (int64_t)st->max_out * pa->K)),
                 "usdm_logprobs: the batched form needs logits_bs >= V, tok_bs >= max_out and top_bs >= max_out * K");
  hipLaunchKernelGGL(logprob_kernel<false>, dim3(nb), dim3(NT), 0, (hipStream_t)stream, *pa, *st, (int64_t)0, 0, 0u);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_logprobs_seg(const usdm_logprob_args* pa, int32_t nseg, int64_t seg_stride, int32_t seg_len,
                                 const usdm_decode_state* st, usdm_stream_t stream) {
  if (int rc = check_logprobs(pa, st, "usdm_logprobs_seg")) return rc;
  const int nb = logits_rows(st->batch);
  if (int rc = check_logits_seg("usdm_logprobs_seg", nseg, seg_stride, seg_len, pa->V, pa->logits_bs, nb)) return rc;
  USDM_CHECK_ARG(nb == 1 || (pa->logits_bs >= seg_len && pa->tok_bs >= st->max_out && (pa->K == 0 || pa->top_bs >= (int64_t)st->max_out * pa->K)),
                 "usdm_logprobs_seg: the batched form needs logits_bs >= seg_len, tok_bs >= max_out and top_bs >= max_out * K");
  hipLaunchKernelGGL(logprob_kernel<true>, dim3(nb), dim3(NT), 0, (hipStream_t)stream, *pa, *st, seg_stride, (int)seg_len, logits_seg_magic(seg_len));
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_logprob_args(void) { return (int)sizeof(usdm_logprob_args); }
