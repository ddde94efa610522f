// Beam search on the device: usdm_beam_step is the pick of the batched decode step of B beams (in place of usdm_sample_final),
// usdm_kv_reorder moves the beams' KV rows to their new owners afterwards.  Both read everything that changes per step (scores,
// parents, positions, the EOS ids) from device memory, so the step stays one hipGraph.
//
// usdm_beam_step, launch 1 (beam_row_kernel): one workgroup of 1024 threads per LIVE row, the row passes of logprob_row.h over its V
// logits (L2-resident), shared with usdm_prompt_logprobs: lp(x) has usdm_logprobs' bits (tests/test_beam_gpu.py and
// tests/test_score_gpu.py pin the three kernels to each other), and the row's own best KC are selected under the composite key
// (order key of s) << 24 | (2^24-1 - id) with s = score[b] + lp(x): the key is the key of the SUM, not of the logit, because two
// logits can round to one s and the total order then goes by the id.  (s, id) go into the scratch [b][KC].
// Launch 2 (beam_merge_kernel): one workgroup ranks the nlive * KC <= 512 scratch entries by (key of s) << 32 | (2^32-1 - flat index)
// by counting, writes the first KC into the step log, walks them for the first B that are no EOS (HF's running beams of the next
// iteration), advances the counters and copies the embedding rows.  The KC best of B * V are among the rows' own best KC, and within
// a row the flat index orders like the id, so the result is the exact selection under the total order.
// Every sum is an integer sum and every per-id quantity depends on the id's value only: bit-identical run to run.
//
// usdm_kv_reorder (kv_reorder_kernel): a byte copy; one thread owns one 16-byte (or, for rows under 16 bytes, 1-byte) offset in ALL
// slots, loads the sources of every slot that changes owner and only then stores them: in place, any map, no staging copy.
#include "logprob_row.h"
#include "pick_commit.h"
#include "../../include/usdm_hip.h"

namespace {
constexpr int NT = LPR_NT, KMAX = USDM_BEAM_MAX_KC, BMAX = 16, NTM = 512, NTR = 256;

__global__ __launch_bounds__(NT) void beam_row_kernel(usdm_beam_args a, int KC) {
  __shared__ lpr_shared<KMAX> sh;
  const int b = blockIdx.x;                        // < nlive (the grid)
  a.logits += (int64_t)b * a.logits_bs;
  const float sc = a.score[b];
  const logits_row_view rv{0, 0, 0u};   // the contiguous row (beam search runs on one GPU: no segmented form)
  unsigned none;                        // (no target: no rank count)
  const float m = lpr_sum<false, false>(a.logits, a.V, rv, sh, 0.f, none);
  __syncthreads();
  const lpr_lse_t z = lpr_lse(sh, m);
  // what is ranked: the candidate's score, one f32 addition on top of usdm_logprobs' lp (banned / empty row: -inf)
  const auto S = [&](float x) { return sc + z.lp(x); };
  const lpr_cut cut = a.V > KC ? lpr_select<false>(a.logits, a.V, KC, rv, sh, S) : lpr_cut{0, 0};
  lpr_collect<false>(a.logits, a.V, KC, rv, sh, cut, S, [&](int r, int id, float s) {   // n = KC: the launcher refuses V < KC
    a.cand_index[b * KC + r] = id;
    a.cand_score[b * KC + r] = s;
  });
}

__global__ __launch_bounds__(NTM) void beam_merge_kernel(usdm_beam_args a, usdm_decode_state st, int B, int KC, const bf16_t* E, int Hd,
                                                         bf16_t* h_out) {
  __shared__ unsigned long long keys[NTM];
  __shared__ float o_s[KMAX];
  __shared__ int o_tok[KMAX], o_par[KMAX], sel_tok[BMAX];
  const int tid = threadIdx.x, n = a.nlive * KC;   // <= 16 * 32 = NTM
  const int t = st.step[0];
  if (t < 0 || t >= a.log_rows || t >= st.max_out) return;
  float s = 0.f;
  int flat = 0, id = 0, b = 0;
  unsigned long long key = 0;
  if (tid < n) {
    b = tid / KC;
    s = a.cand_score[tid];
    id = a.cand_index[tid];
    flat = b * a.V + id;                            // < 16 * 2^20
    key = ((unsigned long long)fkey(s + 0.0f) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)flat);
  }
  keys[tid] = key;
  __syncthreads();
  if (tid < n) {
    int r = 0;
    for (int j = 0; j < n; ++j) r += keys[j] > key;   // keys are unique: a permutation of 0 .. n-1
    if (r < KC) { o_s[r] = s; o_tok[r] = id + st.id_offset; o_par[r] = b; }
  }
  __syncthreads();
  if (tid < KC) {
    a.log_score[(int64_t)t * KC + tid] = o_s[tid];
    a.log_token[(int64_t)t * KC + tid] = o_tok[tid];
    a.log_parent[(int64_t)t * KC + tid] = o_par[tid];
  }
  if (tid == 0) {
    int e[3] = {0, 0, 0};
    for (int j = 0; j < a.n_eos; ++j) e[j] = a.eos[j];
    int got = 0;
    for (int r = 0; r < KC && got < B; ++r) {
      const int tok = o_tok[r];
      bool is_eos = false;
      for (int j = 0; j < a.n_eos; ++j) is_eos |= e[j] == tok;
      if (is_eos) continue;
      sel_tok[got] = tok;
      st.next_token[got] = tok;
      st.out_tokens[(int64_t)got * st.max_out + t] = tok;
      a.parent[got] = o_par[r];
      a.score[got] = o_s[r];
      ++got;
    }
    for (; got < B; ++got) sel_tok[got] = -1;      // (cannot happen: at most n_eos * nlive of the KC are EOS)
    for (int q = 0; q < B; ++q) {
      st.step[q] = t + 1;
      if (st.advance_pos) st.pos[q] = st.pos[q] + 1;
    }
  }
  __syncthreads();
  if (E) {
    for (int q = 0; q < B; ++q)
      if (sel_tok[q] >= 0) pick_embed_row<NTM>(E, sel_tok[q], Hd, h_out + (int64_t)q * Hd);
  }
}

// units of T at byte offset beg of every slot: slot b <- slot par[b], all sources loaded before the first store
template <typename T>
__device__ __forceinline__ void reorder_range(char* base, int64_t slot_bytes, int64_t beg, int64_t n_units, int B, const int* par) {
  for (int64_t u = (int64_t)blockIdx.x * NTR + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * NTR) {
    const int64_t off = beg + u * (int64_t)sizeof(T);
    T v[BMAX];
#pragma unroll
    for (int b = 0; b < BMAX; ++b)
      if (b < B && par[b] != b) v[b] = *(const T*)(base + (int64_t)par[b] * slot_bytes + off);
#pragma unroll
    for (int b = 0; b < BMAX; ++b)
      if (b < B && par[b] != b) *(T*)(base + (int64_t)b * slot_bytes + off) = v[b];
  }
}

__global__ __launch_bounds__(NTR) void kv_reorder_kernel(usdm_kv_reorder_args a) {
  __shared__ int par[BMAX];
  const int arr = blockIdx.z, k = blockIdx.y;
  if (threadIdx.x < BMAX) {
    const int b = threadIdx.x;
    const int p = b < a.B ? a.parent[b] : b;
    par[b] = (p >= 0 && p < a.B) ? p : b;
  }
  __syncthreads();
  const int lo = max(0, a.lo[0]), hi = min(a.ctx_max, a.pos[0]);
  if (lo >= hi) return;
  const int rb = a.row_bytes[arr];
  const int64_t beg = ((int64_t)k * a.ctx_max + lo) * rb, nbytes = (int64_t)(hi - lo) * rb;
  char* base = (char*)a.base[arr];
  if (rb % 16 == 0) reorder_range<u32x4>(base, a.slot_bytes[arr], beg, nbytes / 16, a.B, par);
  else reorder_range<unsigned char>(base, a.slot_bytes[arr], beg, nbytes, a.B, par);
}

int check_beam(const usdm_beam_args* pa, const usdm_decode_state* st, const void* embed_table, int32_t Hd, void* h_out, const char* who) {
  USDM_CHECK_ARG(pa && pa->logits && pa->V > 0 && pa->V <= (1 << 20), "%s: logits / V (1 .. 2^20)", who);
  USDM_CHECK_ARG(st && st->next_token && st->out_tokens && st->step && st->pos && st->max_out > 0, "%s: decode state", who);
  USDM_CHECK_ARG(st->batch >= 0 && st->batch <= BMAX, "%s: a state of 1 .. 16 beams (st->batch)", who);
  USDM_CHECK_ARG(pa->n_eos >= 0 && pa->n_eos <= 3 && (pa->n_eos == 0 || pa->eos), "%s: n_eos must be 0 .. 3 (with the device list eos)", who);
  const int B = logits_rows(st->batch), KC = (pa->n_eos + 1 > 2 ? pa->n_eos + 1 : 2) * B;
  USDM_CHECK_ARG(KC <= KMAX, "%s: KC = max(2, 1 + n_eos) * B = %d candidates, at most %d are supported", who, KC, KMAX);
  USDM_CHECK_ARG(pa->V >= KC, "%s: V = %d is smaller than the KC = %d candidates kept per step", who, pa->V, KC);
  USDM_CHECK_ARG(pa->nlive == 1 || pa->nlive == B, "%s: nlive must be 1 (first step) or B", who);
  USDM_CHECK_ARG(pa->score && pa->parent && pa->cand_score && pa->cand_index, "%s: score / parent / scratch missing", who);
  USDM_CHECK_ARG(pa->log_score && pa->log_token && pa->log_parent && pa->log_rows >= 1, "%s: step log missing", who);
  USDM_CHECK_ARG(!embed_table || (h_out && Hd > 0 && Hd % 8 == 0), "%s: embedding output missing", who);
  return 0;
}
}  // namespace

extern "C" int usdm_beam_step(const usdm_beam_args* pa, const usdm_decode_state* st, const void* embed_table, int32_t Hd, void* h_out,
                              usdm_stream_t stream) {
  if (int rc = check_beam(pa, st, embed_table, Hd, h_out, "usdm_beam_step")) return rc;
  USDM_CHECK_ARG(pa->logits_bs >= pa->V, "usdm_beam_step: logits_bs >= V");
  const int B = logits_rows(st->batch), KC = (pa->n_eos + 1 > 2 ? pa->n_eos + 1 : 2) * B;
  hipLaunchKernelGGL(beam_row_kernel, dim3(pa->nlive), dim3(NT), 0, (hipStream_t)stream, *pa, KC);
  USDM_LAUNCH_CHECK();
  hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(NTM), 0, (hipStream_t)stream, *pa, *st, B, KC, (const bf16_t*)embed_table, Hd, (bf16_t*)h_out);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_sizeof_beam_args(void) { return (int)sizeof(usdm_beam_args); }

extern "C" int usdm_kv_reorder(const usdm_kv_reorder_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->parent && pa->lo && pa->pos, "usdm_kv_reorder: parent / lo / pos missing");
  USDM_CHECK_ARG(pa->B >= 1 && pa->B <= BMAX, "usdm_kv_reorder: B must be 1 .. 16");
  USDM_CHECK_ARG(pa->n_arrays >= 1 && pa->n_arrays <= 4 && pa->nblk >= 1 && pa->nblk <= 65535 && pa->ctx_max >= 1,
                 "usdm_kv_reorder: n_arrays 1 .. 4, nblk 1 .. 65535, ctx_max >= 1");
  for (int i = 0; i < pa->n_arrays; ++i) {
    const int rb = pa->row_bytes[i];
    USDM_CHECK_ARG(pa->base[i] && rb >= 1, "usdm_kv_reorder: array %d: base / row_bytes", i);
    USDM_CHECK_ARG(rb < 16 || (rb % 16 == 0 && (uintptr_t)pa->base[i] % 16 == 0 && pa->slot_bytes[i] % 16 == 0),
                   "usdm_kv_reorder: array %d: rows of 16 bytes or more must be multiples of 16 bytes, 16-byte aligned", i);
    USDM_CHECK_ARG(pa->slot_bytes[i] >= (int64_t)pa->nblk * pa->ctx_max * rb, "usdm_kv_reorder: array %d: slots overlap", i);
  }
  hipLaunchKernelGGL(kv_reorder_kernel, dim3(8, pa->nblk, pa->n_arrays), dim3(NTR), 0, (hipStream_t)stream, *pa);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_kv_reorder_args(void) { return (int)sizeof(usdm_kv_reorder_args); }
