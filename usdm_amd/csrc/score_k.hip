// Log-probabilities of tokens the caller GAVE (a prompt's rows), on the device: usdm_prompt_logprobs scores a chunk of f32 logits rows
// - row r of the chunk is prompt row row0 + r, produced by the lm_head GEMM over the prefill's hidden states - against the prompt's
// next ids: the target of row row0 + r is ids[row0 + r + 1], and every output is indexed by the TARGET's row t = row0 + r + 1.
//
// Per row exactly the quantities and the arithmetic of usdm_logprobs (logprob_k.hip): lp(i) = x_i - logsumexp(x) over ids 0 .. V-1
// (-inf ids are zero mass; here the rows are the raw model's, nothing is banned), rank = 1 + number of strictly greater logits, the
// top K ids in descending log-probability with exact ties by lowest id first.  The passes over the row are logprob_row.h's, shared
// with usdm_beam_step; logprob_kernel has the same passes in a body of its own (its header says why), and tests/test_score_gpu.py
// pins the two to the same bits on the same row and target.
//
// One workgroup of 1024 threads per row (the chunk was just written by the GEMM).  The same logical row gives bit-identical output
// run to run, whatever chunk it sits in, contiguous or segmented (logits_row.h).
#include "logprob_row.h"
#include "../../include/usdm_hip.h"

namespace {
constexpr int NT = LPR_NT, KMAX = 20;

template <bool SEG>
__global__ __launch_bounds__(NT) void prompt_logprob_kernel(usdm_prompt_logprob_args a, int64_t seg_stride, int seg_len, unsigned seg_magic) {
  __shared__ lpr_shared<KMAX> sh;
  const int tid = threadIdx.x, V = a.V, K = a.K;
  const int r = blockIdx.x;                         // < rows (the grid)
  a.logits += (int64_t)r * a.logits_bs;
  const int64_t t = (int64_t)a.row0 + r + 1;        // the target's row: <= row0 + rows < n_ids (checked on the host)
  const int64_t id = a.ids[t];
  const bool tok_ok = id >= 0 && id < V;
  const int tok = tok_ok ? (int)id : 0;

  const logits_row_view rv{seg_stride, seg_len, seg_magic};
  const float xt = tok_ok ? row_at<SEG>(a.logits, tok, rv) : -INFINITY;
  unsigned gt;   // how many ids beat the target
  const float m = lpr_sum<SEG, true>(a.logits, V, rv, sh, xt, gt);
  const auto logit = [](float x) { return x; };   // what is ranked
  lpr_cut cut{0, 0};
  if (K > 0 && V > K) cut = lpr_select<SEG>(a.logits, V, K, rv, sh, logit);
  else __syncthreads();
  const lpr_lse_t z = lpr_lse(sh, m);
  if (tid == 0) {
    a.tok_lp[t] = tok_ok ? z.lp(xt) : -INFINITY;
    a.tok_rank[t] = 1 + (int)gt;
  }
  if (K > 0) {
    int32_t* ids = a.top_id + t * K;
    float* lps = a.top_lp + t * K;
    const int n = lpr_collect<SEG>(a.logits, V, K, rv, sh, cut, logit, [&](int p, int i, float x) { ids[p] = i; lps[p] = z.lp(x); });
    if (tid >= n && tid < K) {   // fewer ids than K
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
