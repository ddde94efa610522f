// usdm_spec_commit: the end of a speculative greedy step, one workgroup: the T rows' arg-max picks, the accepted run
// of drafts, the commit to the device-side decode state, the next step's n-gram drafts from the sequence's own history, and the T
// embedding rows the next step consumes.  Everything is int32 or a copy, so tests/_spec_reference.py restates it bit for bit.
#include "common.h"
#include "../../include/usdm_hip.h"
#include "pick_commit.h"

namespace {
constexpr int SP_TMAX = 8, SP_NMAX = 16;

// token j of the history: the prompt's ids (+ id_offset), then the output so far (as usdm_logit_edit reads it, in token space)
__device__ __forceinline__ int spec_hist(const usdm_spec_args& a, const usdm_decode_state& st, int P, int j) {
  return j < P ? a.prompt[j] + st.id_offset : st.out_tokens[j - P];
}

__global__ __launch_bounds__(256) void spec_commit_kernel(const usdm_spec_args a, const usdm_decode_state st, const bf16_t* E, int Hd,
                                                          bf16_t* h_out) {
#include "spec_commit_body.h"
}

// usdm_spec_commit_batch: workgroup i is usdm_spec_commit's on slot b = slot_lo + i - the arrays of ba.s and st moved on by b slots
__global__ __launch_bounds__(256) void spec_commit_batch_kernel(const usdm_spec_batch_args ba, const usdm_decode_state bst, const bf16_t* E,
                                                                int Hd, bf16_t* h_out) {
  const int b = ba.slot_lo + blockIdx.x;
  usdm_spec_args a = ba.s;
  usdm_decode_state st = bst;
  const int64_t r0 = (int64_t)b * a.T;
  if (a.part_val) { a.part_val += r0 * a.nparts; a.part_idx += r0 * a.nparts; }
  a.drafts += b * SP_TMAX;
  a.limit += b;
  if (a.prompt) a.prompt += (int64_t)b * a.prompt_max;
  a.prompt_len += b;
  if (a.script) a.script += (int64_t)b * st.max_out;
  a.counters += b * 3;
  st.next_token += b;
  st.out_tokens += (int64_t)b * st.max_out;
  st.step += b;
  st.pos += b;
  st.done += b;
  if (st.eos) st.eos += b * 8;
  h_out += r0 * Hd;
#include "spec_commit_body.h"
}

// what both launchers refuse; name: the entry point, for the message
int spec_commit_check(const char* name, const usdm_spec_args* pa, const usdm_decode_state* st, const void* embed_table, int Hd, const void* h_out) {
  USDM_CHECK_ARG(pa && st && embed_table && h_out, "%s: null args", name);
  const usdm_spec_args& a = *pa;
  USDM_CHECK_ARG(a.T >= 1 && a.T <= SP_TMAX, "%s: T = %d outside 1 .. %d", name, a.T, SP_TMAX);
  USDM_CHECK_ARG(st->next_token && st->out_tokens && st->step && st->pos && st->max_out > 0, "%s: decode state incomplete", name);
  USDM_CHECK_ARG(a.drafts && a.limit && a.prompt_len && a.params && a.counters && (a.prompt || a.prompt_max == 0) && a.prompt_max >= 0,
                 "%s: drafts, limit, prompt, prompt_len, params and counters are required", name);
  USDM_CHECK_ARG(a.propose_only || (a.part_val && a.part_idx && a.nparts > 0), "%s: arg-max partials missing", name);
  USDM_CHECK_ARG(a.V > 0 && Hd > 0 && Hd % 8 == 0, "%s: V > 0, Hd a positive multiple of 8", name);
  return 0;
}
}  // namespace

extern "C" int usdm_sizeof_spec_args(void) { return (int)sizeof(usdm_spec_args); }
extern "C" int usdm_spec_commit(const usdm_spec_args* pa, const usdm_decode_state* st, const void* embed_table, int32_t Hd, void* h_out,
                                usdm_stream_t stream) {
  if (int rc = spec_commit_check("usdm_spec_commit", pa, st, embed_table, Hd, h_out)) return rc;
  const usdm_spec_args& a = *pa;
  USDM_CHECK_ARG(st->batch <= 1, "usdm_spec_commit: one sequence only (batch = %d)", st->batch);
  hipLaunchKernelGGL(spec_commit_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, *st, (const bf16_t*)embed_table, Hd, (bf16_t*)h_out);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_sizeof_spec_batch_args(void) { return (int)sizeof(usdm_spec_batch_args); }
extern "C" int usdm_spec_commit_batch(const usdm_spec_batch_args* pb, const usdm_decode_state* st, const void* embed_table, int32_t Hd,
                                      void* h_out, usdm_stream_t stream) {
  USDM_CHECK_ARG(pb, "usdm_spec_commit_batch: null args");
  if (int rc = spec_commit_check("usdm_spec_commit_batch", &pb->s, st, embed_table, Hd, h_out)) return rc;
  USDM_CHECK_ARG(st->batch >= 1 && st->batch * pb->s.T <= SP_NMAX, "usdm_spec_commit_batch: a state of %d slots with T = %d rows each: 1 .. 16 rows",
                 st->batch, pb->s.T);
  USDM_CHECK_ARG(pb->slot_lo >= 0 && pb->n >= 1 && pb->slot_lo + pb->n <= st->batch, "usdm_spec_commit_batch: slots [%d, %d) outside the state's %d",
                 pb->slot_lo, pb->slot_lo + pb->n, st->batch);
  USDM_CHECK_ARG(st->done, "usdm_spec_commit_batch: the per-slot done words are required");
  hipLaunchKernelGGL(spec_commit_batch_kernel, dim3(pb->n), dim3(256), 0, (hipStream_t)stream, *pb, *st, (const bf16_t*)embed_table, Hd,
                     (bf16_t*)h_out);
  USDM_LAUNCH_CHECK();
  return 0;
}
