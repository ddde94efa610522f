// Additive logit bias and the n-gram ban of the LLM decode step, on the device: what both depend on (the request's bias list, the
// prompt, out_tokens, step) lives there, so a step with either stays one hipGraph.  usdm_logit_edit runs BEFORE usdm_penalize and
// the pick (usdm_sample_final) of the same step, in place on the ban-masked f32 row the lm_head wrote in this step.
//
// State per sequence (device memory, written by the host per request): a 16-byte block {ngram n, prompt_len P, n_bias}, the rows
// bias_id / bias_val of up to 1024 entries (one per thread) and the row prompt of the prompt's ids.  One launch, two phases:
//   1  bias: thread t < n_bias does row[bias_id[t]] = row[bias_id[t]] + bias_val[t], one f32 add (-inf stays -inf, NaN stays NaN);
//      the ids are distinct, entries outside [0, V) are ignored.
//   -- __syncthreads(): a bias read-modify-write must not overwrite the ban of the same id
//   2  n-gram ban (HF NoRepeatNGramLogitsProcessor): hist[j] = j < P ? prompt[j] : out_tokens[j - P] - id_offset, Lh = P + *step, read
//      where it lives.  With n >= 1 and Lh >= n, every j in 0 .. Lh - n whose hist[j .. j+n-2] equals the last n - 1 tokens bans
//      hist[j+n-1]: row[..] = -inf.  Threads stride over j and leave a compare at its first mismatch; several threads may store -inf
//      to one id, which is benign.
// A sequence with n_bias = 0 and n <= 0 returns before it forms its row's address; one whose `done` word is set returns at once.
//
// One workgroup of 1024 threads per sequence; the row is contiguous or segmented (logits_row.h).
#include "logits_row.h"
#include "../../include/usdm_hip.h"

namespace {
constexpr int NT = 1024;

template <bool SEG>
__global__ __launch_bounds__(NT) void logit_edit_kernel(usdm_logit_edit_args a, usdm_decode_state st, int64_t seg_stride, int seg_len,
                                                        unsigned seg_magic) {
  const int tid = threadIdx.x, V = a.V, b = blockIdx.x;
  if (st.done && st.done[b]) return;
  const usdm_logit_edit_params kn = a.dev_params[b];
  // values outside their ranges (the host never writes one) are clamped to what the rows hold
  const int nbias = min(max(kn.n_bias, 0), min(a.bias_max, NT));
  const int n = max(kn.ngram, 0);
  if (nbias == 0 && n == 0) return;   // neutral slot: every bit of the row stays, nothing of it is read
  float* row = a.logits + (int64_t)b * a.logits_bs;
  const logits_row_view rv{seg_stride, seg_len, seg_magic};
  if (tid < nbias) {
    const int id = a.bias_id[(int64_t)b * a.bias_bs + tid];
    if ((unsigned)id < (unsigned)V) {
      float* px = row_ptr<SEG>(row, id, rv);
      *px = *px + a.bias_val[(int64_t)b * a.bias_bs + tid];
    }
  }
  __syncthreads();   // (nbias and n are the same for the whole workgroup)
  if (n == 0) return;
  const int P = min(max(kn.prompt_len, 0), a.prompt_max);
  const int Lh = P + min(max(st.step[b], 0), st.max_out);
  if (Lh < n) return;
  const int32_t* prompt = a.prompt + (int64_t)b * a.prompt_bs;
  const int32_t* out = st.out_tokens + (int64_t)b * st.max_out;
  auto hist = [&](int j) -> int { return j < P ? prompt[j] : out[j - P] - st.id_offset; };
  const int tail = Lh - (n - 1);   // the last n - 1 tokens start here
  for (int j = tid; j <= Lh - n; j += NT) {
    bool same = true;
    for (int k = 0; k < n - 1; ++k)
      if (hist(j + k) != hist(tail + k)) { same = false; break; }
    if (!same) continue;
    const int id = hist(j + n - 1);
    if ((unsigned)id < (unsigned)V) *row_ptr<SEG>(row, id, rv) = -INFINITY;
  }
}

int check_logit_edit(const usdm_logit_edit_args* pa, const usdm_decode_state* st, const char* who) {
  USDM_CHECK_ARG(pa && pa->logits && pa->V > 0 && pa->V <= (1 << 20), "%s: logits / V (1 .. 2^20)", who);
  USDM_CHECK_ARG(pa->dev_params, "%s: dev_params missing", who);
  USDM_CHECK_ARG(pa->bias_max >= 0 && pa->bias_max <= NT && (pa->bias_max == 0 || (pa->bias_id && pa->bias_val)),
                 "%s: bias_max (0 .. 1024) / bias_id / bias_val", who);
  USDM_CHECK_ARG(pa->prompt_max >= 0 && (pa->prompt_max == 0 || pa->prompt), "%s: prompt_max / prompt", who);
  USDM_CHECK_ARG((uintptr_t)pa->logits % 4 == 0 && (uintptr_t)pa->bias_id % 4 == 0 && (uintptr_t)pa->bias_val % 4 == 0 &&
                 (uintptr_t)pa->prompt % 4 == 0 && (uintptr_t)pa->dev_params % 16 == 0,
                 "%s: logits / bias_id / bias_val / prompt must be 4-byte aligned, dev_params 16-byte aligned", who);
  USDM_CHECK_ARG(st && st->out_tokens && st->step && st->max_out > 0, "%s: decode state", who);
  return 0;
}
}  // namespace

extern "C" int usdm_logit_edit(const usdm_logit_edit_args* pa, const usdm_decode_state* st, usdm_stream_t stream) {
  if (int rc = check_logit_edit(pa, st, "usdm_logit_edit")) return rc;
  const int nb = logits_rows(st->batch);
  USDM_CHECK_ARG(nb == 1 || (pa->logits_bs >= pa->V && pa->bias_bs >= pa->bias_max && pa->prompt_bs >= pa->prompt_max),
                 "usdm_logit_edit: the batched form needs logits_bs >= V, bias_bs >= bias_max and prompt_bs >= prompt_max");
  hipLaunchKernelGGL(logit_edit_kernel<false>, dim3(nb), dim3(NT), 0, (hipStream_t)stream, *pa, *st, (int64_t)0, 0, 0u);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_logit_edit_seg(const usdm_logit_edit_args* pa, int32_t nseg, int64_t seg_stride, int32_t seg_len,
                                   const usdm_decode_state* st, usdm_stream_t stream) {
  if (int rc = check_logit_edit(pa, st, "usdm_logit_edit_seg")) return rc;
  const int nb = logits_rows(st->batch);
  if (int rc = check_logits_seg("usdm_logit_edit_seg", nseg, seg_stride, seg_len, pa->V, pa->logits_bs, nb)) return rc;
  USDM_CHECK_ARG(nb == 1 || (pa->logits_bs >= seg_len && pa->bias_bs >= pa->bias_max && pa->prompt_bs >= pa->prompt_max),
                 "usdm_logit_edit_seg: the batched form needs logits_bs >= seg_len, bias_bs >= bias_max and prompt_bs >= prompt_max");
  hipLaunchKernelGGL(logit_edit_kernel<true>, dim3(nb), dim3(NT), 0, (hipStream_t)stream, *pa, *st, seg_stride, (int)seg_len, logits_seg_magic(seg_len));
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_sizeof_logit_edit_args(void) { return (int)sizeof(usdm_logit_edit_args); }
extern "C" int usdm_sizeof_logit_edit_params(void) { return (int)sizeof(usdm_logit_edit_params); }
