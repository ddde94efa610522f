// Log-probabilities of tokens the caller GAVE (a prompt's rows), on the device: usdm_prompt_logprobs scores a chunk of f32 logits rows
// - row r of the chunk is prompt row row0 + r, produced by the lm_head GEMM over the prefill's hidden states - against the prompt's
// next ids: the target of row row0 + r is ids[row0 + r + 1], and every output is indexed by the TARGET's row t = row0 + r + 1.
//
// Per row exactly the quantities and the arithmetic of usdm_logprobs (logprob_k.hip): lp(i) = x_i - logsumexp(x) over ids 0 .. V-1
// (-inf ids are zero mass; here the rows are the raw model's, nothing is banned), rank = 1 + number of strictly greater logits, the
// top K ids in descending log-probability with exact ties by lowest id first.  The row body below is a COPY of logprob_kernel's: moving
// it into a shared __device__ template changed the register allocation of usdm_logprobs (profiles/score_row_share_isa_diff.txt), so
// the decode kernel stays as it is.  tests/test_score_gpu.py pins the two to the same bits on the same row and target.
//
// One workgroup of 1024 threads per row, passes over the V logits (the chunk was just written by the GEMM):
//   1  max and rank count          (registers, wave reductions)
//   2  sum of exp(x - max)         as a 2^40 FIXED-POINT integer sum (associative: no dependence on thread scheduling)
//   3+ top K (K > 0, V > K)        radix select, 8 bits per pass, of the K-th largest COMPOSITE key (order key of x) << 24 | (2^24-1 - id)
//   last collect the <= 20 kept keys, order them by counting, write the row
// Every sum is an integer sum and every per-id quantity depends on the id's value only, so the same logical row gives bit-identical
// output run to run, whatever chunk it sits in, contiguous or segmented (logits_row.h).
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
__global__ __launch_bounds__(NT) void prompt_logprob_kernel(usdm_prompt_logprob_args a, int64_t seg_stride, int seg_len, unsigned seg_magic) {
  __shared__ unsigned hist[256 * REP];
  __shared__ unsigned long long cand[KMAX];
  __shared__ float sredf[NW];
  __shared__ unsigned sredu[NW];
  __shared__ unsigned long long s_z, s_prefix;
  __shared__ unsigned s_rem, s_cnt, s_n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, V = a.V, K = a.K;
  const int r = blockIdx.x;                         // < rows (the grid)
  a.logits += (int64_t)r * a.logits_bs;
  const int64_t t = (int64_t)a.row0 + r + 1;        // the target's row: <= row0 + rows < n_ids (checked on the host)
  const int64_t id = a.ids[t];
  const bool tok_ok = id >= 0 && id < V;
  const int tok = tok_ok ? (int)id : 0;

  const logits_row_view rv{seg_stride, seg_len, seg_magic};
  auto each = [&](auto&& f) {   // f(i, logit of i) for i = tid, tid + NT, ... < V
    row_each<SEG, NT>(a.logits, V, tid, rv, [&](int i, const float* px) { f(i, *px); });
  };

  // ---- pass 1: max, and how many ids beat the target
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
        for (int q = 0; q < REP; ++q) tot += hist[tid * REP + ((q + tid) & (REP - 1))];
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
  auto LP = [&](float x) -> float {   // empty row: -inf, never NaN; NaN only from a NaN logit
    if (x == -INFINITY || Z == 0) return -INFINITY;
    return (float)((double)(x == m ? 0.f : x - m) - logZ);
  };
  if (tid == 0) {
    a.tok_lp[t] = tok_ok ? LP(xt) : -INFINITY;
    a.tok_rank[t] = 1 + (int)gt;
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
    int32_t* ids = a.top_id + t * K;
    float* lps = a.top_lp + t * K;
    if (tid < n) {
      const unsigned long long c = cand[tid];
      int p = 0;
      for (int j = 0; j < n; ++j) p += cand[j] > c;   // keys are unique: a permutation of 0 .. n-1
      ids[p] = (int)(0xFFFFFFu - (unsigned)(c & 0xFFFFFFu));
      lps[p] = LP(fkey_inv((unsigned)(c >> 24)));
    } else if (tid < K) {   // fewer ids than K
      ids[tid] = -1;
      lps[tid] = -INFINITY;
    }
  }
}

int check_prompt_logprobs(const usdm_prompt_logprob_args* pa, const char* who) {
  USDM_CHECK_ARG(pa && pa->logits && pa->V > 0 && pa->V <= (1 << 20), "%s: logits / V (1 .. 2^20)", who);
  USDM_CHECK_ARG(pa->K >= 0 && pa->K <= KMAX, "%s: K must be 0 .. 20", who);
  USDM_CHECK_ARG(pa->ids, "%s: ids missing", who);
  USDM_CHECK_ARG(pa->tok_lp && pa->tok_rank, "%s: tok_lp / tok_rank missing", who);
  USDM_CHECK_ARG(pa->K == 0 || (pa->top_id && pa->top_lp), "%s: top_id / top_lp missing with K > 0", who);
  USDM_CHECK_ARG(pa->rows >= 1 && pa->row0 >= 0 && (int64_t)pa->row0 + pa->rows + 1 <= pa->n_ids,
                 "%s: rows row0 .. row0 + rows - 1 need their targets: rows >= 1, row0 >= 0, row0 + rows + 1 <= n_ids", who);
  return 0;
}
}  // namespace

extern "C" int usdm_prompt_logprobs(const usdm_prompt_logprob_args* pa, usdm_stream_t stream) {
  if (int rc = check_prompt_logprobs(pa, "usdm_prompt_logprobs")) return rc;
  USDM_CHECK_ARG(pa->logits_bs >= pa->V, "usdm_prompt_logprobs: logits_bs >= V");
  hipLaunchKernelGGL(prompt_logprob_kernel<false>, dim3(pa->rows), dim3(NT), 0, (hipStream_t)stream, *pa, (int64_t)0, 0, 0u);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_prompt_logprobs_seg(const usdm_prompt_logprob_args* pa, int32_t nseg, int64_t seg_stride, int32_t seg_len,
                                        usdm_stream_t stream) {
  if (int rc = check_prompt_logprobs(pa, "usdm_prompt_logprobs_seg")) return rc;
  if (int rc = check_logits_seg("usdm_prompt_logprobs_seg", nseg, seg_stride, seg_len, pa->V, pa->logits_bs, pa->rows)) return rc;
  USDM_CHECK_ARG(pa->rows == 1 || pa->logits_bs >= seg_len, "usdm_prompt_logprobs_seg: logits_bs >= seg_len");
  hipLaunchKernelGGL(prompt_logprob_kernel<true>, dim3(pa->rows), dim3(NT), 0, (hipStream_t)stream, *pa, seg_stride, (int)seg_len,
                     logits_seg_magic(seg_len));
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_prompt_logprob_args(void) { return (int)sizeof(usdm_prompt_logprob_args); }
