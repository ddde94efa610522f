// usdm_spec_commit: the end of a speculative greedy step, one workgroup: the T rows' arg-max picks, the accepted run
// of drafts, the commit to the device-side decode state, the next step's n-gram drafts from the sequence's own history, and the T
// embedding rows the next step consumes.  Everything is int32 or a copy, so tests/_spec_reference.py restates it bit for bit.
// The *_picks forms take the rows' picks as given - usdm_spec_sample's draws - and share everything behind them.
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
#include "spec_slot_view.h"
#include "spec_commit_body.h"
}

// usdm_spec_commit_picks: the same workgroup with the rows' picks given (usdm_spec_sample's draws) instead of arg-maxed
#define SPEC_GIVEN_PICKS
__global__ __launch_bounds__(256) void spec_commit_picks_kernel(const usdm_spec_args a, const usdm_decode_state st, const bf16_t* E, int Hd,
                                                                bf16_t* h_out, const int* picks) {
#include "spec_commit_body.h"
}

// usdm_spec_commit_batch_picks: workgroup i on slot b = slot_lo + i, its picks at b * T
__global__ __launch_bounds__(256) void spec_commit_batch_picks_kernel(const usdm_spec_batch_args ba, const usdm_decode_state bst, const bf16_t* E,
                                                                      int Hd, bf16_t* h_out, const int* picks) {
#include "spec_slot_view.h"
  if (picks) picks += r0;
#include "spec_commit_body.h"
}
#undef SPEC_GIVEN_PICKS

// what every launcher refuses; name: the entry point, for the message.  given: the picks form (picks in place of the partials)
int spec_commit_check(const char* name, const usdm_spec_args* pa, const usdm_decode_state* st, const void* embed_table, int Hd, const void* h_out,
                      bool given = false, const int32_t* picks = nullptr) {
  USDM_CHECK_ARG(pa && st && embed_table && h_out, "%s: null args", name);
  const usdm_spec_args& a = *pa;
  USDM_CHECK_ARG(a.T >= 1 && a.T <= SP_TMAX, "%s: T = %d outside 1 .. %d", name, a.T, SP_TMAX);
  USDM_CHECK_ARG(st->next_token && st->out_tokens && st->step && st->pos && st->max_out > 0, "%s: decode state incomplete", name);
  USDM_CHECK_ARG(a.drafts && a.limit && a.prompt_len && a.params && a.counters && (a.prompt || a.prompt_max == 0) && a.prompt_max >= 0,
                 "%s: drafts, limit, prompt, prompt_len, params and counters are required", name);
  if (given) {
    USDM_CHECK_ARG(a.propose_only || picks, "%s: picks missing", name);
  } else {
    USDM_CHECK_ARG(a.propose_only || (a.part_val && a.part_idx && a.nparts > 0), "%s: arg-max partials missing", name);
  }
  USDM_CHECK_ARG(a.V > 0 && Hd > 0 && Hd % 8 == 0, "%s: V > 0, Hd a positive multiple of 8", name);
  return 0;
}

// the single-sequence launch, from the partials or (given) from picks
int spec_commit_launch(const char* name, const usdm_spec_args* pa, bool given, const int32_t* picks, const usdm_decode_state* st,
                       const void* embed_table, int32_t Hd, void* h_out, usdm_stream_t stream) {
  if (int rc = spec_commit_check(name, pa, st, embed_table, Hd, h_out, given, picks)) return rc;
  USDM_CHECK_ARG(st->batch <= 1, "%s: one sequence only (batch = %d)", name, st->batch);
  if (given)
    hipLaunchKernelGGL(spec_commit_picks_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *pa, *st, (const bf16_t*)embed_table, Hd,
                       (bf16_t*)h_out, picks);
  else
    hipLaunchKernelGGL(spec_commit_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *pa, *st, (const bf16_t*)embed_table, Hd, (bf16_t*)h_out);
  USDM_LAUNCH_CHECK();
  return 0;
}

// the launch over the slots [slot_lo, slot_lo + n), likewise
int spec_commit_batch_launch(const char* name, const usdm_spec_batch_args* pb, bool given, const int32_t* picks, const usdm_decode_state* st,
                             const void* embed_table, int32_t Hd, void* h_out, usdm_stream_t stream) {
  USDM_CHECK_ARG(pb, "%s: null args", name);
  if (int rc = spec_commit_check(name, &pb->s, st, embed_table, Hd, h_out, given, picks)) return rc;
  USDM_CHECK_ARG(st->batch >= 1 && st->batch * pb->s.T <= SP_NMAX, "%s: a state of %d slots with T = %d rows each: 1 .. 16 rows", name, st->batch,
                 pb->s.T);
  USDM_CHECK_ARG(pb->slot_lo >= 0 && pb->n >= 1 && pb->slot_lo + pb->n <= st->batch, "%s: slots [%d, %d) outside the state's %d", name,
                 pb->slot_lo, pb->slot_lo + pb->n, st->batch);
  USDM_CHECK_ARG(st->done, "%s: the per-slot done words are required", name);
  if (given)
    hipLaunchKernelGGL(spec_commit_batch_picks_kernel, dim3(pb->n), dim3(256), 0, (hipStream_t)stream, *pb, *st, (const bf16_t*)embed_table, Hd,
                       (bf16_t*)h_out, picks);
  else
    hipLaunchKernelGGL(spec_commit_batch_kernel, dim3(pb->n), dim3(256), 0, (hipStream_t)stream, *pb, *st, (const bf16_t*)embed_table, Hd,
                       (bf16_t*)h_out);
  USDM_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" int usdm_sizeof_spec_args(void) { return (int)sizeof(usdm_spec_args); }
extern "C" int usdm_spec_commit(const usdm_spec_args* pa, const usdm_decode_state* st, const void* embed_table, int32_t Hd, void* h_out,
                                usdm_stream_t stream) {
  return spec_commit_launch("usdm_spec_commit", pa, false, nullptr, st, embed_table, Hd, h_out, stream);
}
extern "C" int usdm_spec_commit_picks(const usdm_spec_args* pa, const int32_t* picks, const usdm_decode_state* st, const void* embed_table,
                                      int32_t Hd, void* h_out, usdm_stream_t stream) {
  return spec_commit_launch("usdm_spec_commit_picks", pa, true, picks, st, embed_table, Hd, h_out, stream);
}

extern "C" int usdm_sizeof_spec_batch_args(void) { return (int)sizeof(usdm_spec_batch_args); }
extern "C" int usdm_spec_commit_batch(const usdm_spec_batch_args* pb, const usdm_decode_state* st, const void* embed_table, int32_t Hd,
                                      void* h_out, usdm_stream_t stream) {
  return spec_commit_batch_launch("usdm_spec_commit_batch", pb, false, nullptr, st, embed_table, Hd, h_out, stream);
}
extern "C" int usdm_spec_commit_batch_picks(const usdm_spec_batch_args* pb, const int32_t* picks, const usdm_decode_state* st,
                                            const void* embed_table, int32_t Hd, void* h_out, usdm_stream_t stream) {
  return spec_commit_batch_launch("usdm_spec_commit_batch_picks", pb, true, picks, st, embed_table, Hd, h_out, stream);
}
