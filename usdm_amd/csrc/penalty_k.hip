// Repetition / frequency / presence penalties of the LLM decode step, on the device: the history a penalty depends on (out_tokens,
// step) already lives there, so a penalised step stays one hipGraph.  usdm_penalize runs BEFORE the pick (usdm_sample_final) of the
// same step, in place on the ban-masked f32 row the sampler will read.
//
// State per sequence: tbl[V] int32, c(i) = how often id i was generated in this call in bits 0 .. 29, in_prompt(i) in bit 30 (seeded
// by the host per request).  One launch does both jobs of a step:
//   1  account for the token the PREVIOUS step picked: last = out_tokens[*step - 1] - id_offset.  The thread that owns id `last` adds
//      1 in registers and stores the word back: no atomics, no second launch.
//   2  penalise this step's row, every operation a separate f32 operation (the library builds with -ffp-contract=off; a numpy
//      float32 restatement is bit-identical):
//        seen = in_prompt(i) or c(i) > 0
//        x = seen ? (x < 0 ? x * r : x / r) : x        repetition_penalty r  (HF RepetitionPenaltyLogitsProcessor; prompt + output)
//        x = x - (f * float(c(i)))                     frequency_penalty f   (vLLM: output tokens only)
//        x = x - (p * (c(i) > 0 ? 1.0f : 0.0f))        presence_penalty p    (vLLM: output tokens only)
//      -inf (banned) stays -inf, NaN stays NaN.  A slot with the neutral knobs r = 1, f = 0, p = 0 only counts: its row is not read.
// Replays must not count twice: with a `count` word a token is counted only while count[b] < *step, and count[b] = *step afterwards;
// with a device-side `done` word the launch returns at once when it is set, as the decode kernels do with `skip`.  At every pick c
// is therefore exactly the histogram of out_tokens[0 .. *step - 1].
//
// One workgroup of 1024 threads per sequence (the read of `count` and its update are separated by a __syncthreads()), one pass over
// the V logits and table words (L2-resident, 2 x 168 KB at V = 42003); the row is contiguous or segmented (logits_row.h).
#include "logits_row.h"
#include "../../include/usdm_hip.h"

namespace {
constexpr int NT = 1024;
constexpr int PROMPT_BIT = 1 << 30, COUNT_MASK = PROMPT_BIT - 1;

template <bool SEG>
__global__ __launch_bounds__(NT) void penalty_kernel(usdm_penalty_args a, usdm_decode_state st, int64_t seg_stride, int seg_len,
                                                     unsigned seg_magic) {
  const int tid = threadIdx.x, V = a.V, b = blockIdx.x;
  if (st.done && st.done[b]) return;
  const int step = st.step[b];
  // the token picked by the previous step, if this launch is the first to see it (a replay at the same step counts nothing)
  int last = -1;
  if (step >= 1 && step <= st.max_out && (!a.count || a.count[b] < step)) last = st.out_tokens[(int64_t)b * st.max_out + step - 1] - st.id_offset;
  if (last >= V) last = -1;
  __syncthreads();   // every thread has read count[b]
  if (tid == 0 && a.count) a.count[b] = step;
  const usdm_penalty_params kn = a.dev_params[b];
  // a knob outside its range (the host never writes one; a zero-filled block) is taken as neutral
  const float r = (kn.repetition > 0.f && kn.repetition <= 2.f) ? kn.repetition : 1.0f;
  const float f = (kn.frequency >= -2.f && kn.frequency <= 2.f) ? kn.frequency : 0.0f;
  const float p = (kn.presence >= -2.f && kn.presence <= 2.f) ? kn.presence : 0.0f;
  int32_t* tbl = a.table + (int64_t)b * a.table_bs;
  if (r == 1.0f && f == 0.0f && p == 0.0f) {   // neutral slot: count only, every bit of the row stays
    if (tid == 0 && last >= 0) tbl[last] = tbl[last] + 1;
    return;
  }
  float* row = a.logits + (int64_t)b * a.logits_bs;
  row_each<SEG, NT>(row, V, tid, logits_row_view{seg_stride, seg_len, seg_magic}, [&](int i, float* px) {
    int t = tbl[i];
    if (i == last) {
      t += 1;
      tbl[i] = t;
    }
    const int c = t & COUNT_MASK;
    float x = *px;
    if (t != 0) x = x < 0.f ? x * r : x / r;
    x = x - (f * (float)c);
    x = x - (p * (c > 0 ? 1.0f : 0.0f));
    *px = x;
  });
}

int check_penalize(const usdm_penalty_args* pa, const usdm_decode_state* st, const char* who) {
  USDM_CHECK_ARG(pa && pa->logits && pa->V > 0 && pa->V <= (1 << 20), "%s: logits / V (1 .. 2^20)", who);
  USDM_CHECK_ARG(pa->table && pa->dev_params, "%s: table / dev_params missing", who);
  USDM_CHECK_ARG((uintptr_t)pa->logits % 4 == 0 && (uintptr_t)pa->table % 4 == 0 && (uintptr_t)pa->count % 4 == 0 &&
                 (uintptr_t)pa->dev_params % 16 == 0, "%s: logits / table / count must be 4-byte aligned, dev_params 16-byte aligned", who);
  USDM_CHECK_ARG(st && st->out_tokens && st->step && st->max_out > 0, "%s: decode state", who);
  USDM_CHECK_ARG(!st->done || pa->count, "%s: a state with a device-side `done` word needs the tokens-counted word", who);
  return 0;
}
}  // namespace

extern "C" int usdm_penalize(const usdm_penalty_args* pa, const usdm_decode_state* st, usdm_stream_t stream) {
  if (int rc = check_penalize(pa, st, "usdm_penalize")) return rc;
  const int nb = logits_rows(st->batch);
  USDM_CHECK_ARG(nb == 1 || (pa->logits_bs >= pa->V && pa->table_bs >= pa->V),
                 "usdm_penalize: the batched form needs logits_bs >= V and table_bs >= V");
  hipLaunchKernelGGL(penalty_kernel<false>, dim3(nb), dim3(NT), 0, (hipStream_t)stream, *pa, *st, (int64_t)0, 0, 0u);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_penalize_seg(const usdm_penalty_args* pa, int32_t nseg, int64_t seg_stride, int32_t seg_len,
                                 const usdm_decode_state* st, usdm_stream_t stream) {
  if (int rc = check_penalize(pa, st, "usdm_penalize_seg")) return rc;
  const int nb = logits_rows(st->batch);
  if (int rc = check_logits_seg("usdm_penalize_seg", nseg, seg_stride, seg_len, pa->V, pa->logits_bs, nb)) return rc;
  USDM_CHECK_ARG(nb == 1 || (pa->logits_bs >= seg_len && pa->table_bs >= pa->V),
                 "usdm_penalize_seg: the batched form needs logits_bs >= seg_len and table_bs >= V");
  hipLaunchKernelGGL(penalty_kernel<true>, dim3(nb), dim3(NT), 0, (hipStream_t)stream, *pa, *st, seg_stride, (int)seg_len, logits_seg_magic(seg_len));
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_penalty_params_init(usdm_penalty_params* out, float repetition, float frequency, float presence) {
  USDM_CHECK_ARG(out, "usdm_penalty_params_init: out missing");
  USDM_CHECK_ARG(repetition > 0.f && repetition <= 2.f, "usdm_penalty_params_init: repetition_penalty must be in (0, 2], got %g", (double)repetition);
  USDM_CHECK_ARG(frequency >= -2.f && frequency <= 2.f, "usdm_penalty_params_init: frequency_penalty must be in [-2, 2], got %g", (double)frequency);
  USDM_CHECK_ARG(presence >= -2.f && presence <= 2.f, "usdm_penalty_params_init: presence_penalty must be in [-2, 2], got %g", (double)presence);
  out->repetition = repetition; out->frequency = frequency; out->presence = presence; out->reserved = 0;
  return 0;
}
extern "C" int usdm_sizeof_penalty_args(void) { return (int)sizeof(usdm_penalty_args); }
extern "C" int usdm_sizeof_penalty_params(void) { return (int)sizeof(usdm_penalty_params); }
