// Beam search on the device: usdm_beam_step is the pick of the batched decode step of B beams (in place of usdm_sample_final),
// usdm_kv_reorder moves the beams' KV rows to their new owners afterwards.  Both read everything that changes per step (scores,
// parents, positions, the EOS ids) from device memory, so the step stays one hipGraph.
//
// usdm_beam_step, launch 1 (beam_row_kernel): one workgroup of 1024 threads per LIVE row, passes over its V logits (L2-resident):
//   1  max                         (registers, wave reductions)
//   2  sum of exp(x - max)         as a 2^40 FIXED-POINT integer sum: usdm_logprobs' arithmetic, term for term (logprob_k.hip)
//   3+ the row's own best KC       radix select, 8 bits per pass, of the KC-th largest COMPOSITE key (order key of s) << 24 | (2^24-1 - id)
//                                  with s = score[b] + lp(x): the key is the key of the SUM, not of the logit, because two logits can
//                                  round to one s and the total order then goes by the id
//   last collect the kept keys, order them by counting, write (s, id) into the scratch [b][KC]
// Launch 2 (beam_merge_kernel): one workgroup ranks the nlive * KC <= 512 scratch entries by (key of s) << 32 | (2^32-1 - flat index)
// by counting, writes the first KC into the step log, walks them for the first B that are no EOS (HF's running beams of the next
// iteration), advances the counters and copies the embedding rows.  The KC best of B * V are among the rows' own best KC, and within
// a row the flat index orders like the id, so the result is the exact selection under the total order.
// Every sum is an integer sum and every per-id quantity depends on the id's value only: bit-identical run to run.
//
// usdm_kv_reorder (kv_reorder_kernel): a byte copy; one thread owns one 16-byte (or, for rows under 16 bytes, 1-byte) offset in ALL
// slots, loads the sources of every slot that changes owner and only then stores them: in place, any map, no staging copy.
#include "logits_row.h"
#include "../../include/usdm_hip.h"

namespace {
constexpr int NT = 1024, NW = NT / 64, REP = 32, KMAX = USDM_BEAM_MAX_KC, BMAX = 16, NTM = 512, NTR = 256;

// composite key of (id, s): larger = better, then lower id.  -0.0 is folded into +0.0 first (equal values must tie)
__device__ __forceinline__ unsigned long long ckey(int i, float s) {
  return ((unsigned long long)fkey(s + 0.0f) << 24) | (unsigned long long)(0xFFFFFFu - (unsigned)i);
}
__device__ __forceinline__ float fkey_inv(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ __launch_bounds__(NT) void beam_row_kernel(usdm_beam_args a, int KC) {
  __shared__ unsigned hist[256 * REP];
  __shared__ unsigned long long cand[KMAX];
  __shared__ float sredf[NW];
  __shared__ unsigned sredu[NW];
  __shared__ unsigned long long s_z, s_prefix;
  __shared__ unsigned s_rem, s_cnt, s_n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, V = a.V, K = KC;
  const int b = blockIdx.x;                        // < nlive (the grid)
  a.logits += (int64_t)b * a.logits_bs;
  const float sc = a.score[b];

  const logits_row_view rv{0, 0, 0u};   // the contiguous row (beam search runs on one GPU: no segmented form)
  auto each = [&](auto&& f) {   // f(i, logit of i) for i = tid, tid + NT, ... < V
    row_each<false, NT>(a.logits, V, tid, rv, [&](int i, const float* px) { f(i, *px); });
  };

  // ---- pass 1: max
  float m = -INFINITY;
  each([&](int, float x) { m = fmaxf(m, x); });
  m = wave_max(m);
  if (lane == 0) sredf[wv] = m;
  if (tid == 0) { s_z = 0; s_n = 0; }
  __syncthreads();
  m = sredf[0];
  for (int w = 1; w < NW; ++w) m = fmaxf(m, sredf[w]);

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
  __syncthreads();
  const unsigned long long Z = s_z;
  const double logZ = log((double)Z) - 40.0 * 0.69314718055994530942;
  auto S = [&](float x) -> float {   // the candidate's score: one f32 addition on top of usdm_logprobs' lp (banned / empty row: -inf)
    const float lp = (x == -INFINITY || Z == 0) ? -INFINITY : (float)((double)(x == m ? 0.f : x - m) - logZ);
    return sc + lp;
  };

  // ---- the row's own best K: the K-th largest composite key
  unsigned long long kth = 0, keep = 0;   // kept: (key & keep) >= kth; everything when V <= K
  if (V > K) {
    unsigned long long prefix = 0, mask = 0;
    unsigned rem = (unsigned)K;
    for (int shift = 48; shift >= 0; shift -= 8) {
      for (int i = tid; i < 256 * REP; i += NT) hist[i] = 0;
      __syncthreads();
      each([&](int i, float x) {
        const unsigned long long c = ckey(i, S(x));
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
  }
  each([&](int i, float x) {
    const unsigned long long c = ckey(i, S(x));
    if ((c & keep) >= kth) {
      const unsigned s = atomicAdd(&s_n, 1u);
      if (s < KMAX) cand[s] = c;
    }
  });
  __syncthreads();
  const int n = min((int)s_n, K);       // = K: the launcher refuses V < KC
  if (tid < n) {
    const unsigned long long c = cand[tid];
    int r = 0;
    for (int j = 0; j < n; ++j) r += cand[j] > c;   // keys are unique: a permutation of 0 .. n-1
    a.cand_index[b * K + r] = (int)(0xFFFFFFu - (unsigned)(c & 0xFFFFFFu));
    a.cand_score[b * K + r] = fkey_inv((unsigned)(c >> 24));
  }
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
    for (int q = 0; q < B; ++q) {
      if (sel_tok[q] < 0) continue;
      const u32x4* src = (const u32x4*)(E + (int64_t)sel_tok[q] * Hd);
      u32x4* dst = (u32x4*)(h_out + (int64_t)q * Hd);
      for (int i = tid; i < Hd / 8; i += NTM) dst[i] = src[i];
    }
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
