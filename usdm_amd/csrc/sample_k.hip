// Sampling head of the LLM decode step: temperature -> top-k -> top-p -> one multinomial draw, on the device, so that a
// sampled decode step is as replayable (hipGraph) as the greedy one.  Semantics follow HF transformers'
// TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper + torch.multinomial (the reference's
// model.generate(do_sample=True, top_p, top_k, temperature) at src/inference.py:63-83; the demo exposes the knobs,
// streamlit_demo.py:201-211).  What cannot be mirrored is torch's random stream: the draw uses Philox4x32-10 keyed by
// `seed` with the device-side step counter as counter, so a (seed, step) pair always gives the same token.
//
// One workgroup of 1024 threads, a handful of passes over the V logits (L2-resident, 168 KB at V = 42003):
//   top-k  : radix select (4 x 8 bits) of the k-th largest key with integer histograms; ties at the k-th rank are kept, and -0.0
//            counts as +0.0 there, as in HF's `scores < kth`;
//   top-p  : radix select over the ascending exp(x - max) keys with FIXED-POINT mass histograms (u64 LDS atomics are
//            associative, so the kept set does not depend on thread scheduling); ties are kept or dropped as a block;
//   min-p  : HF MinPLogitsWarper / vLLM: ids with p_i < min_p * p_max are dropped, by raising the top-p stage's key threshold;
//   draw   : u * kept_mass located by an exclusive scan over contiguous index ranges (index order, deterministic).
// The passes are one text, sample_body.h: the decode step's pick (sample_final_kernel) and the rows of a sampled speculative step
// (spec_sample_kernel, DESIGN.md 8k-3: row i drawn with the counter step + i, nothing committed) include it.
#include "logits_row.h"
#include "pick_commit.h"
#include "../../include/usdm_hip.h"

namespace {
constexpr int NT = 1024;

__device__ __forceinline__ void philox_round(unsigned (&c)[4], const unsigned (&k)[2]) {
  const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k[0], n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k[1], n3 = (unsigned)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

__device__ double philox_uniform(unsigned long long seed, unsigned ctr) {   // u in [0, 1), 53 bits
  unsigned c[4] = {ctr, 0u, 0u, 0u}, k[2] = {(unsigned)seed, (unsigned)(seed >> 32)};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k);
    k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
  }
  const unsigned long long hi = c[0] >> 5, lo = c[1] >> 6;   // 27 + 26 bits
  return (double)((hi << 26) | lo) * (1.0 / 9007199254740992.0);
}

__device__ float block_max(float v, float* sred) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = sred[0];
  for (int w = 1; w < NT / 64; ++w) m = fmaxf(m, sred[w]);
  __syncthreads();
  return m;
}

// SEG: the row of sequence b is contiguous (usdm_sample_final) or segmented (usdm_sample_final_seg), see logits_row.h.  Every sum
// below is an integer sum and every per-id quantity depends on the id's value only.
template <bool SEG>
__global__ __launch_bounds__(NT) void sample_final_kernel(usdm_sample_args a, usdm_decode_state st, const bf16_t* E, int Hd,
                                                           bf16_t* h_out, int64_t seg_stride, int seg_len, unsigned seg_magic,
                                                           int64_t probs_bs) {
  const int tid = threadIdx.x, V = a.V;
  // batched decode (st.batch > 1): workgroup b = sequence b, with its OWN knobs (dev_params[b]), logits row, state words and
  // Philox counter (its own step): a sequence sampled inside a continuous batch gets the tokens it would get alone
  const int b = blockIdx.x;
  a.logits += (int64_t)b * a.logits_bs;
  if (a.probs_out) a.probs_out += (int64_t)b * probs_bs;
  if (st.done && st.done[b]) return;
  constexpr int row_i = 0;
#include "sample_body.h"
  if (a.probs_out) {
    const double inv = Zk > 0 ? 1.0 / (double)Zk : 0.0;
    each([&](int i, float lg) {
      const float e = El(lg);
      a.probs_out[i] = (e > 0.f && __float_as_uint(e) >= pkey) ? (float)((double)Q(e) * inv) : 0.f;
    });
  }
  if (tid == 0) pick_commit(st, b, step, s_tok + st.id_offset);
  if (E) pick_embed_row<NT>(E, s_tok + st.id_offset, Hd, h_out + (int64_t)b * Hd);
}

// usdm_spec_sample: workgroup r = b * T + i draws the token of sequence b's row i as sample_final_kernel would draw it at step[b] + i
// from that row - the same text - and writes the local id to picks[r]: no commit, no embedding row, no state word changes.  A
// workgroup whose sequence is done, or whose row no accept run can reach (a draft in front of it is -1), returns at once.
__global__ __launch_bounds__(NT) void spec_sample_kernel(const usdm_spec_sample_args sa) {
  constexpr bool SEG = false;
  constexpr int64_t seg_stride = 0;
  constexpr int seg_len = 0;
  constexpr unsigned seg_magic = 0u;
  const int tid = threadIdx.x, V = sa.V;
  const int r = blockIdx.x, b = r / sa.T, row_i = r - b * sa.T;
  if (sa.done && sa.done[b]) return;
  for (int j = 1; j <= row_i; ++j)
    if (sa.drafts[b * 8 + j] < 0) return;
  usdm_sample_args a = {};
  a.logits = sa.logits + (int64_t)r * sa.logits_bs;
  a.dev_params = sa.dev_params;
  usdm_decode_state st = {};
  st.step = const_cast<int32_t*>(sa.step);
#include "sample_body.h"
  if (tid == 0) sa.picks[r] = s_tok;
}
}  // namespace

namespace {
int check_sample(const usdm_sample_args* pa, const usdm_decode_state* st, const void* embed_table, int32_t Hd, void* h_out,
                 const char* who) {
  USDM_CHECK_ARG(pa && pa->logits && pa->V > 0 && pa->V <= (1 << 20), "%s: logits / V", who);
  USDM_CHECK_ARG(pa->dev_params || (pa->temperature > 0.f && pa->top_p > 0.f && pa->top_p <= 1.0f && pa->top_k >= 0),
                 "%s: temperature > 0, 0 < top_p <= 1, top_k >= 0 (0 = off)", who);
  USDM_CHECK_ARG(pa->dev_params || (pa->min_p >= 0.f && pa->min_p <= 1.0f), "%s: min_p must be in [0, 1] (0 = off)", who);
  USDM_CHECK_ARG(st && st->next_token && st->out_tokens && st->step && st->pos, "%s: decode state", who);
  USDM_CHECK_ARG(!embed_table || (h_out && Hd > 0 && Hd % 8 == 0), "%s: embedding output missing", who);
  return 0;
}
}  // namespace

extern "C" int usdm_sample_final(const usdm_sample_args* pa, const usdm_decode_state* st, const void* embed_table, int32_t Hd,
                                 void* h_out, usdm_stream_t stream) {
  if (int rc = check_sample(pa, st, embed_table, Hd, h_out, "usdm_sample_final")) return rc;
  const int nb = logits_rows(st->batch);
  USDM_CHECK_ARG(nb == 1 || (pa->logits_bs >= pa->V && pa->dev_params), "usdm_sample_final: the batched form needs logits_bs >= V and dev_params[batch]");
  hipLaunchKernelGGL(sample_final_kernel<false>, dim3(nb), dim3(NT), 0, (hipStream_t)stream, *pa, *st, (const bf16_t*)embed_table, Hd,
                     (bf16_t*)h_out, (int64_t)0, 0, 0u, (int64_t)pa->V);   // probs_out is [batch][V], whatever the rows' stride
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_sample_final_seg(const usdm_sample_args* pa, int32_t nseg, int64_t seg_stride, int32_t seg_len,
                                     const usdm_decode_state* st, const void* embed_table, int32_t Hd, void* h_out,
                                     usdm_stream_t stream) {
  if (int rc = check_sample(pa, st, embed_table, Hd, h_out, "usdm_sample_final_seg")) return rc;
  const int nb = logits_rows(st->batch);
  if (int rc = check_logits_seg("usdm_sample_final_seg", nseg, seg_stride, seg_len, pa->V, pa->logits_bs, nb)) return rc;
  USDM_CHECK_ARG(nb == 1 || (pa->logits_bs >= seg_len && pa->dev_params), "usdm_sample_final_seg: the batched form needs logits_bs >= seg_len and dev_params[batch]");
  hipLaunchKernelGGL(sample_final_kernel<true>, dim3(nb), dim3(NT), 0, (hipStream_t)stream, *pa, *st, (const bf16_t*)embed_table, Hd,
                     (bf16_t*)h_out, seg_stride, (int)seg_len, logits_seg_magic(seg_len), (int64_t)pa->V);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_sample_args(void) { return (int)sizeof(usdm_sample_args); }

extern "C" int usdm_spec_sample(const usdm_spec_sample_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->logits && pa->V > 0 && pa->V <= (1 << 20), "usdm_spec_sample: logits / V");
  USDM_CHECK_ARG(pa->T >= 1 && pa->T <= 8 && pa->n >= 1 && pa->n * pa->T <= 16, "usdm_spec_sample: n = %d sequences of T = %d rows: T in 1 .. 8, 1 .. 16 rows",
                 pa->n, pa->T);
  USDM_CHECK_ARG(pa->logits_bs >= pa->V || pa->n * pa->T == 1, "usdm_spec_sample: logits_bs >= V");
  USDM_CHECK_ARG(pa->dev_params && pa->step && pa->drafts && pa->picks, "usdm_spec_sample: dev_params[n], step[n], drafts[n][8] and picks[n * T] are required");
  hipLaunchKernelGGL(spec_sample_kernel, dim3(pa->n * pa->T), dim3(NT), 0, (hipStream_t)stream, *pa);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_spec_sample_args(void) { return (int)sizeof(usdm_spec_sample_args); }
