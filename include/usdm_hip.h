/*
 * libusdm_hip.so — C-ABI of the MI355X (gfx950) hot path of USDM inference.
 *
 * The reference (ishine/usdm) has no FFI / plugin boundary: its inference path is Python calling
 * PyTorch-CUDA ops.  This header is therefore the *new* native boundary that the
 * Python drop-ins (usdm_amd/voicebox/..., usdm_amd/unit_extractor.py, usdm_amd/llm.py) bind with
 * ctypes.  Every entry point cites the reference call site whose arithmetic it replaces
 * (paths relative to the reference repo root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (a torch tensor), unless named host_*
 *   - no allocation, no synchronisation, no hidden global state; all work is enqueued on `stream`
 *   - return value: 0 = ok, 1 = HIP runtime error, 2 = bad argument; text via usdm_last_error()
 *   - dtype codes: USDM_BF16 = 0 (raw bf16 bits), USDM_F32 = 1
 */
#ifndef USDM_HIP_H_
#define USDM_HIP_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* usdm_stream_t; /* hipStream_t */

enum { USDM_BF16 = 0, USDM_F32 = 1 };
enum { USDM_ACT_NONE = 0, USDM_ACT_GELU = 1, USDM_ACT_SWIGLU = 3, USDM_ACT_TANH = 4, USDM_ACT_LOGCLAMP = 5 /* log(max(x,1e-5)) */ };
enum { USDM_EPI_PLAIN = 0, USDM_EPI_QKV_HEADS = 1 };

const char* usdm_last_error(void);
int usdm_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Universal "tap-GEMM" on the MFMA matrix cores (bf16 16x16x32 / exact-f32 16x16x4):
 *
 *   acc[m][n] = sum_{tap<taps} sum_{c<Kc} A[row(m,tap)][c + tap*a_tap_stride] * W[n][tap*Kc + c]
 *   row(m,tap) = m*a_row_mul + a_row_off + tap*a_row_step      (rows outside [0,rowsA) read as 0)
 *   v = alpha*acc + bias[n];  v = act(v);  v += residual[m][n];  store
 *
 * With channels-last activations [time][channel] this one kernel is every dense op of the path:
 *   nn.Linear / Conv1d k=1        networks.py:141-144,219-222,299,301; voicebox transformer GEMMs
 *   dilated Conv1d                vocoder/models.py:33-49 (AMPBlock1 convs), :150 (conv_pre)
 *   ConvTranspose1d (per phase)   vocoder/models.py:157-162 (ups)
 *   grouped Conv1d                networks.py:70-76 (PositionalConvEmbedding)
 *   strided Conv1d                XLS-R feature extractor (third-party)
 *   skip Linear over cat[h,skip]  networks.py:364 (two-source K via a_tap_stride)
 *   Mistral prefill projections   HF MistralAttention/MistralMLP (third-party)
 * ---------------------------------------------------------------------------------------------- */
typedef struct usdm_gemm_args {
  int32_t dtype;         /* USDM_BF16 or USDM_F32: element type of A and W                        */
  int32_t M, N;          /* output rows / columns (per group, per batch)                          */
  int32_t taps, Kc;      /* Kc: channels per tap, multiple of 32 (bf16) / 16 (f32)                */
  const void* A;
  int64_t lda;           /* elements between consecutive A rows                                   */
  int32_t rowsA;         /* number of valid A rows (per batch); others read as zero               */
  int32_t a_row_mul, a_row_off, a_row_step;
  int64_t a_tap_stride;  /* elements added to the A column base per tap (two-source K)            */
  const void* W;
  int64_t ldw;           /* elements between consecutive W rows (>= taps*Kc)                      */
  int32_t groups, batch; /* grid z = batch*groups                                                 */
  int64_t a_gstride;     /* A column offset per group (elements)                                  */
  int64_t w_gstride;     /* W element offset per group                                            */
  int64_t a_bstride;     /* A element offset per batch                                            */
  int32_t c_gcol;        /* output/bias/residual column offset per group                          */
  int64_t c_bstride;     /* output/residual ROW offset per batch (before c_row_mul)               */
  const float* bias;     /* [groups*N] or NULL                                                    */
  float alpha;
  int32_t act;           /* USDM_ACT_*                                                            */
  int32_t round_bf16;    /* 1: round acc(+bias) to bf16 before act/residual (HF bf16 semantics)   */
  const void* residual;  /* [rows][ldr] of res_dtype or NULL; indexed like the output             */
  int32_t res_dtype;
  int64_t ldr;
  void* C32;             /* optional f32 output                                                   */
  void* C16;             /* optional bf16 output                                                  */
  int64_t ldc;           /* elements between output rows (or between columns if transpose_out)    */
  int32_t c_row_mul, c_row_off; /* output row = (b*c_bstride + m)*c_row_mul + c_row_off           */
  int32_t transpose_out; /* 1: store C^T, i.e. out[n][row]                                        */
  int32_t epi;           /* USDM_EPI_*                                                            */
  /* USDM_EPI_QKV_HEADS: N = 3*H*D, rows m = b*S + s; Q,K -> [B][H][S_pad][D], V -> [B][H][D][S_pad] */
  int32_t qkv_S, qkv_Spad, qkv_H, qkv_D;
  void *qkv_q, *qkv_k, *qkv_v; /* bf16 */
  /* split-K (single-tap, plain f32 output only): grid z is multiplied by split_k; split s accumulates its share of the K
   * chunks and stores to C32 + s*c_split_stride; bias and residual are applied by split 0 only.  The consumer sums the
   * partials (e.g. usdm_norm's `res` input).  For deep-K problems whose output tiles do not fill the chip. */
  int32_t split_k; int64_t c_split_stride;
  /* LayerNorm folded into the neighbouring GEMMs (post-LN block of networks.py:236-266: h1 = LN(h + attn) is consumed by the
   * feed-forward GEMM and by the next residual add, never on its own; saves the LayerNorm launch and its 22 MB round trip).
   *   stats_out  PRODUCER (row-major plain epilogue, 128-column tiles): after bias / residual, every tile writes the sum of its
   *              128 columns of each output row and their M2 = sum (v - tile mean)^2 to stats_out[row][tiles_n][2] (f32; no
   *              atomics, so the result is run-to-run reproducible).
   *   ln_mode 1  CONSUMER, A operand = the UN-normalised rows x (bf16), W = weights with gamma folded in along K:
   *              v = rstd[m] * acc[m][n] - rstd[m] * mean[m] * ln_c[n] + bias[n]   (ln_c[n] = sum_k W[n][k]; bias already holds
   *              b[n] + sum_k W0[n][k] beta[k]), i.e. exactly LN(x) W0^T + b, then the activation.  GELU bf16-out epilogue of the
   *              ping-pong tiles only.
   *   ln_mode 2  CONSUMER, residual[m][n] is UN-normalised x (f32): the residual added is LN(x)[m][n] =
   *              (x - mean[m]) * rstd[m] * ln_gamma[n] + ln_beta[n].  Row-major plain epilogue.
   * mean / rstd come from ln_stats[row][ln_nt][2]: per 128-column tile the producer's (sum, M2 about the tile's own mean), merged
   * pairwise-exactly (Chan et al.) over the ln_nt tiles of ln_C = 128 * ln_nt columns: no sum(x^2) - mean^2 cancellation.
   *   ln_guard   optional device word (ln_mode 1 and 2): OR-ed with 1 when a row has |mean| * rstd > ln_guard_ratio.  ln_mode 1
   *              multiplies rows that were rounded to bf16 before centring, so its operand noise relative to the normalised
   *              signal is 2^-9 * sqrt(1 + (mean / sigma)^2): the caller bounds the ratio it accepts and re-runs such inputs with
   *              the separate LayerNorm kernel (usdm_amd/voicebox/model/networks.py does). */
  float* stats_out;
  const float* ln_stats; int32_t ln_nt, ln_mode, ln_C; float ln_eps;
  const float* ln_c; const float* ln_gamma; const float* ln_beta;
  int32_t* ln_guard; float ln_guard_ratio;
  /* 0: the launcher picks the tile from the shape (measured heuristics, csrc/gemm.hip gemm_select); t + 1: force tile t, a row of
   * USDM_GEMM_TILES in csrc/gemm.hip (benchmarks and the tile-equivalence tests; the Python wrapper fills it from USDM_GEMM_TILE
   * so the library itself reads no environment per launch) */
  int32_t tile_sel;
} usdm_gemm_args;

int usdm_gemm(const usdm_gemm_args* args, usdm_stream_t stream);
int usdm_gemm_tile_for(const usdm_gemm_args* args); /* the tile usdm_gemm would pick (the ping-pong rows of the table are the only ones
                                                        with the stats_out / ln_mode epilogues), < 0 for invalid arguments; launches nothing */
int usdm_gemm_tile_info(int tile, int dtype, int32_t* out); /* out[8] = BM, BN, waves, DMA, LDS stages, chunks per stage, ping-pong, 0
                                                                of row `tile`; refuses a tile that does not exist for `dtype`; host only */

/* ------------------------------------------------------------------------------------------------
 * LayerNorm / RMSNorm over channels of [rows][C] activations (one wave per row).
 *   t = x (+ res);  [premask: rows s >= valid_len[b] zeroed first];  sum32/sum16 <- t (optional)
 *   y = (t - mean) * rsqrt(var + eps) * gamma + beta     (rms: mean := 0, no beta)
 *   y = act(y);  rows s >= valid_len[b] are written as zero
 * Replaces nn.LayerNorm at networks.py:245-247,297,349; XLS-R LayerNorms; HF MistralRMSNorm.
 * round_bf16 = 1 reproduces HF's bf16 rounding points: bf16(gamma * bf16(t * rstd)), and rounds
 * t = x + res to bf16 (the bf16 residual stream of HF Mistral).
 * ---------------------------------------------------------------------------------------------- */
typedef struct usdm_norm_args {
  const void* x; int32_t x_dtype; int64_t ldx;
  const void* res; int32_t res_dtype; int64_t ldr;
  const float* gamma; const float* beta; float eps;
  int32_t rows, C;
  int32_t rms, act, round_bf16, premask;
  const int32_t* valid_len; int32_t rows_per_batch;
  void* out32; void* out16; int64_t ldo;
  void* sum32; void* sum16; int64_t lds;
  const float* res2; int32_t n_res2; int64_t res2_stride;   /* n_res2 more f32 addends [rows][ldr], res2_stride elements apart (split-K partials): x + res + res2[0] + ... */
} usdm_norm_args;

int usdm_norm(const usdm_norm_args* args, usdm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused anti-aliased SnakeBeta: Activation1d(SnakeBeta) of the reference in one pass
 * (vocoder/alias_free_torch/act.py:23-28, resample.py:25-33, filter.py:86-95,
 *  vocoder/activations.py:107-120).  x is channels-last f32 [T][ldx]; channels >= Creal are padding
 * and are written as zero (their x, alpha and beta are never used).  fup/fdn: the 12 Kaiser-sinc taps
 * of kaiser_sinc_filter1d(0.25,0.3,12) (filter.py:28-57) computed on the host.  The production taps are
 * symmetric, but the fields are not interchangeable with their reverse.  Orientation: fup[] are the
 * weights of conv_transpose1d(stride 2), fdn[] the weights of conv1d(stride 2) (a correlation):
 *   u[2m]   = 2 * sum_{i=-2..3} fup[5+2i] * x~[m-i]
 *   u[2m+1] = 2 * sum_{i=-3..2} fup[6+2i] * x~[m-i]           x~[k] = x[clamp(k, 0, T-1)]
 *   v[n]    = u[n] + 1/(b + 1e-9) * sin(u[n] * a)^2           a, b = alpha, beta (exp() of them if logscale)
 *   o[t]    = sum_{j=0..11} fdn[j] * v~[2t-5+j]               v~[n] = v[clamp(n, 0, 2T-1)]
 * L: time steps per thread (0 = choose); the result does not depend on it.
 * Alignment: the kernel moves channel pairs, so C, ldx and ldo are even, x and out32 are 8-byte aligned
 * and out16 is 4-byte aligned; anything else is refused.
 * ---------------------------------------------------------------------------------------------- */
typedef struct usdm_snake_args {
  const float* x; int64_t ldx;
  int32_t T, C, Creal, L;
  const float* alpha; const float* beta; int32_t logscale;
  float fup[12]; float fdn[12];
  float* out32; void* out16; int64_t ldo;
} usdm_snake_args;
int usdm_aa_snake(const usdm_snake_args* args, usdm_stream_t stream);

/* (a+b+c)*scale over n f32 elements (vocoder/models.py:198-204). n % 4 == 0. */
int usdm_sum3_scale(const float* a, const float* b, const float* c, float scale, int64_t n,
                    float* out32, void* out16_bf16, usdm_stream_t stream);

/* channels-first f32 [B][C][T] -> channels-last [B][T][Cpad] (f32 and/or bf16), y = x*scale+shift,
 * padded channels zero.  Mel de-normalisation + layout change (model_util.py:103-104). */
int usdm_cf_to_cl(const float* x, int32_t B, int32_t C, int32_t T, int32_t Cpad, float scale, float shift,
                  float* out32, void* out16_bf16, usdm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Flash-style attention forward (bf16 MFMA, fp32 online softmax), nothing [S,S]-sized in memory.
 *   mode 0: bidirectional, score += -slopes[h]*|i-j| (0 for key 0 if alibi_col0_zero), keys >= kv_len[b]
 *           masked  -> Voicebox Attention.forward + Transformer.forward bias (networks.py:162-210,319-341)
 *   mode 1: causal (key j visible iff j <= q_pos0 + i), GQA -> HF Mistral prefill attention
 * Layouts (bf16, element strides): q[b][h][s][dh] via q_bs/q_hs/q_rs; k likewise with Hkv heads;
 * vt = V^T [b][hk][dh][key] via v_bs/v_hs/v_ds; o[b][s][h*dh] via o_bs/o_rs.
 * K/V^T must be allocated and finite up to Skv_alloc >= roundup(Skv,64) keys.
 * ---------------------------------------------------------------------------------------------- */
typedef struct usdm_attn_args {
  int32_t mode, dh, B, Hq, Hkv, Sq, Skv, Skv_alloc, q_pos0, alibi_col0_zero;
  float scale;
  int32_t head_order;   /* mode 0, speed only: 0 = library default, 1 = steepest ALiBi heads first and last in dispatch order, -1 = flattest first */
  const void* q; int64_t q_bs, q_hs, q_rs;
  const void* k; int64_t k_bs, k_hs, k_rs;
  const void* vt; int64_t v_bs, v_hs, v_ds;
  void* o; int64_t o_bs, o_rs;
  const int32_t* kv_len;  /* [B] or NULL (= Skv) */
  const float* slopes;    /* [Hq] or NULL */
  int32_t window;         /* mode 1: > 0 = sliding window, query at position p sees keys p-window+1 .. p (HF Mistral sliding_window,
                             src/model.py:337-371 keeps W - 1 past keys + the new one = the HF eager mask; the reference's flash-attn call
                             passes window_size = (W, W), src/model.py:510,532, which admits W + 1 keys in a prefill: the two reference
                             paths themselves differ by one key beyond 4096 tokens, and this follows the first); 0 = full causal */
  int32_t variant;        /* mode 0, d = 64, speed only: 0 = 16-query waves (default), 1 = the 32-query-wave kernel (benchmarks; results agree
                             to one bf16 ulp).  The library reads no environment variable per launch. */
} usdm_attn_args;
int usdm_attention(const usdm_attn_args* args, usdm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Voicebox glue (dense math is usdm_gemm / usdm_attention / usdm_norm).
 * ---------------------------------------------------------------------------------------------- */
/* Estimator input assembly: embed(x)*sqrt(E) ++ y ++ cond, channels-last bf16 rows
 * (networks.py:305-307), with the classifier-free-guidance batch doubling of voicebox.py:60-65
 * done in place when dup == 2 (first B_in rows: null token, zero cond). */
typedef struct usdm_vb_input_args {
  const int64_t* ids;  /* [B_in][S] */
  const float* y;      /* [B_in][F][S] */
  const float* cond;   /* [B_in][F][S] */
  const void* table;   /* bf16 [n_tokens+1][E], already multiplied by sqrt(E) */
  int32_t B_in, dup, S, E, F, null_id, use_cond;
  void* out; int64_t ldo; /* [B_in*dup][S][ldo] of out_dtype */
  int32_t out_dtype;      /* USDM_BF16 (default plan: MFMA operand rows, table bf16) or USDM_F32 (exact-f32 plan: table f32) */
} usdm_vb_input_args;
int usdm_vb_build_input(const usdm_vb_input_args* args, usdm_stream_t stream);

/* Attention probabilities of the exact-f32 Voicebox plan (the reference runs fp32: networks.py:162-210): in place on the f32 score
 * matrix x[row][h*ldseg + j] = q_i.k_j (row = b*rows_per_batch + i): p = softmax_j(x - slopes[h]*|i-j|, key 0 unbiased when
 * col0_zero) over keys j < kv_len[b]; masked keys -> 0, pad columns [n, npad) -> 0 (networks.py:319-341). */
int usdm_softmax_alibi(float* x, int32_t rows, int32_t rows_per_batch, int32_t nheads, int32_t n, int32_t npad, int64_t ldrow,
                       int32_t ldseg, const float* slopes, const int32_t* kv_len, int32_t col0_zero, usdm_stream_t stream);

/* Sinusoidal time token (SinusoidalPosEmb, networks.py:13-28) into row 0 of each batch of h:
 * [sin(1000*t*freqs), cos(1000*t*freqs)], freqs[H/2] = exp(arange(H/2) * -ln(1e4)/(H/2-1)) from the host. */
int usdm_vb_time_token(const float* t, int32_t t_stride, const float* freqs, int32_t Bx, int32_t H,
                       int64_t rows_per_batch, float* h32, void* h16_bf16, usdm_stream_t stream);

/* One elementwise solver update (voicebox.py:66-72 CFG, :83-90 Euler, :112-131 Heun):
 *   v = cfg ? vc + gs*(vc - vu) : vout
 *   mode 0: v1 <- v ; zn = z + dt*v          mode 1: zn = z + dt*(v1 + v)/2
 *   if eps: zn[.., s < P] = c_eps*eps + c_cond*cond   (prompt re-noising, :115-117,:126-128)
 *   z_in <- zn (estimator input), z_commit <- zn (solver state), t_cur[0..t_count) <- t_next */
typedef struct usdm_vb_solver_args {
  const float* vout;  /* [B*(cfg?2:1)][F][S] */
  const float* z; float* v1; const float* eps; const float* cond;
  float* z_in; float* z_commit; float* t_cur;
  int32_t B, F, S, P, cfg, mode, t_count;
  float gs, dt, c_eps, c_cond, t_next;
} usdm_vb_solver_args;
int usdm_vb_solver_step(const usdm_vb_solver_args* args, usdm_stream_t stream);

/* Padding mask of ragged Voicebox batches (networks.py:330-333 and the `* y_mask` products): zero every time step
 * t >= valid_len[b] - off of x; layout 0 = [B][T][C] (channels-last), 1 = [B][C][T] (channels-first). */
int usdm_mask_time(float* x32, void* x16_bf16, int32_t B, int32_t T, int32_t C, int32_t layout, const int32_t* valid_len,
                   int32_t off, usdm_stream_t stream);

/* device-to-device async copy (graph-capturable plumbing) */
int usdm_copy_bytes(void* dst, const void* src, int64_t nbytes, usdm_stream_t stream);

/* process_unit (util/model_util.py:50-54): out[f] = mode of repeat_interleave(units, rep)[f*hop:(f+1)*hop],
 * ties -> smallest id; nframes = floor(n*rep/hop).  int64 in / int64 out. */
int usdm_process_unit(const int64_t* units, int32_t n, int32_t rep, int32_t hop, int64_t* out, int32_t nframes,
                      usdm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mistral-7B speech-text LLM (third-party arithmetic of the reference: HF transformers
 * MistralForCausalLM + GenerationMixin.generate, call sites src/inference.py:63-83, load :116-124).
 * Prefill uses usdm_gemm / usdm_norm / usdm_attention(mode 1); the kernels below are the rest.
 * ---------------------------------------------------------------------------------------------- */
/* Batch-1 GEMV y = W x over bf16 weights [N][ldw] (nn.Linear layout), HBM-streaming:
 *   norm_w != NULL : x is the raw residual stream; RMSNorm(x)*norm_w is applied first (HF rounding)
 *   act == USDM_ACT_SWIGLU : rows packed in blocks of 32 = 16 gate + 16 up; output N/2 = silu(g)*u
 *   residual       : y += residual[n] (bf16)             round_bf16 : HF bf16 rounding points
 *   part_val/idx   : lm_head mode — per-block (max, argmax) of the bf16-rounded logits with ban[n]==1
 *                    excluded (bad_words_ids of inference.py:51-53); y32 (optional) receives the logits */
typedef struct usdm_gemv_args {
  const void* W; int64_t ldw; int32_t N, K;
  const void* x;
  const float* norm_w; float eps;
  int32_t act, round_bf16;
  const void* residual;
  void* y16; float* y32;
  const uint8_t* ban; float* part_val; int32_t* part_idx;
  int32_t idx_offset; /* added to the row index stored in part_idx (vocab-parallel shards) */
  /* tensor-parallel decode: the all-reduced f32 partial sum of the previous row-parallel projection is folded in here
   * instead of a separate residual-add launch: x' = bf16(x + bf16(x_delta)) is what gets normalised / multiplied, and
   * workgroup 0 writes x' to x_out (a DIFFERENT buffer than x: other workgroups are still reading x) */
  const float* x_delta; void* x_out;
  const int32_t* skip;  /* optional: *skip != 0 -> the launch returns immediately (see usdm_decode_state.done) */
  /* tensor-parallel decode over xGMI peer-to-peer (usdm_allreduce_p2p_*, below): this launch is a ROW-parallel projection
   * whose f32 partial sums are all-reduced INSIDE its epilogue.  p2p_mode 1 (fused): the workgroup that owns output rows
   * [r0, r1) writes its partials as {epoch, f32} granules into slot[site][rank] of EVERY rank's buffer, waits (bounded) for
   * the same rows from every rank in its own buffer, sums them in rank order and stores y16[n] = bf16(residual[n] +
   * bf16(sum)): the all-reduce, the residual add and the bf16 rounding of HF's residual stream in one epilogue, no
   * collective launch.  p2p_mode 2 (split): write only; usdm_allreduce_p2p_reduce finishes.  Needs residual and y16. */
  const struct usdm_p2p_dev* p2p; int32_t p2p_site, p2p_mode;
  /* EXPERIMENTAL, off by default (measured slower: profiles/r02_decode_ablation.txt section 1; see usdm_hip_experimental.h).
   * o_proj of the decode step: x is not read from memory but MERGED here, in the x-staging prologue, from the context-split
   * partials usdm_attn_decode left (defer_merge): x[h*128+d] = bf16( sum_s po[h][s][d]*w_s / sum_s pl[h][s]*w_s ),
   * w_s = exp(pm[h][s] - max_s pm[h][s]).  Replaces the separate combine launch (the prologue runs while this launch's first
   * weight loads are in flight).  K = heads*128; mrg_ns splits per head. */
  const float* mrg_pm; const float* mrg_pl; const float* mrg_po; int32_t mrg_ns;
  /* o_proj of the decode step, hand-off form (round 3): with cmb_gran the mrg_* partials are combined ONCE per head, by the
   * first K/128 workgroups of THIS launch (the arithmetic of the combine kernel, bit for bit), and handed to all workgroups as
   * 8-byte granules {tag 1, 2 x bf16} in cmb_gran[K/2] (device memory; its tags must be zero when the launch starts:
   * usdm_attn_decode(cmb_gran) clears them).  Every workgroup requests its first weight ring BEFORE it waits for the granules,
   * so the combine runs under the weight latency instead of in a launch of its own.  The wait is bounded (cmb_timeout_ms of the
   * 100 MHz clock); on expiry the workgroup ORs 1 into *cmb_err and carries on with zeros.  N = 16 * 256 outputs only (one
   * 16-wave workgroup per CU, all co-resident): the hand-off ASSUMES that workgroups 0 .. K/128-1 are dispatched and make progress
   * while the others poll, which holds exactly because the whole grid is resident at once; a launch for which it did not hold
   * would cost one timeout per layer (and raise through *cmb_err), not hang. */
  unsigned long long* cmb_gran; int32_t* cmb_err; int32_t cmb_timeout_ms;
  /* Form of the SwiGLU launch (benchmarking / test override, as usdm_gemm_args.tile_sel; it occupies what was the struct's tail
   * padding, so sizeof and every other offset are unchanged and a zero-filled struct means what it always did).
   *   0  the launcher's choice: gate/up of the 7B (14-output tiles of 7 waves) runs RESIDENT on bf16 weights - the grid is the number
   *      of workgroups the device holds at once, workgroup b streams tiles b, b + grid, ... behind ONE prologue, and the weight ring
   *      of a tile is refilled from the next tile's rows - every other shape as before;
   *   -1 one tile per workgroup;
   *   >0 resident on at most this many workgroups.
   * A non-zero value also selects the 14-output tile at EVERY SwiGLU shape (so that both forms partition the RMSNorm sums alike at
   * the small shapes of the tests).  Both forms give identical bits; FP8 / MXFP4 weights and x_delta have the one-tile form only.
   * A plain bf16 projection with K = 14336 (no SwiGLU, norm_w, x_delta, lm_head mode, merged input or fused all-reduce; down_proj
   * of the 7B) has a straight-line form of the 16-wave one-row kernel, whose weight ring stays in flight through the K loop:
   *   0  that form where the launcher picks 16-wave workgroups anyway (N = 16 * 256);  -1 never;
   *   >0 that form at every N, one workgroup per 16 rows (the value itself means nothing more).  Identical bits again. */
  int32_t resident;
} usdm_gemv_args;
int usdm_gemv(const usdm_gemv_args* args, usdm_stream_t stream);
int usdm_gemv_nblocks(int32_t N, int32_t act); /* number of partials the lm_head mode writes */

int usdm_gemv_threads(const usdm_gemv_args* args);   /* threads per workgroup usdm_gemv would launch this projection with */
int usdm_gemv_streams(const usdm_gemv_args* args);   /* 1 where usdm_gemv runs it (bf16 weights) in the straight-line K = 14336 form */

/* Batched decode (the serving path's request lists, src/inference_vllm.py:109-125): the same projection over nb
 * input vectors, weights streamed ONCE per step.  g holds item 0's pointers; item b is at + b * stride.  Two forms:
 *   VALU (nb <= 4)          v_dot2 per sequence; per item the arithmetic of usdm_gemv, bit for bit.
 *   matrix cores (nb <= 16) the weights as the A operand of v_mfma_f32_16x16x32_bf16 (16 rows x 32 K per instruction, loaded from
 *                           HBM straight into the fragment layout), the nb activation vectors as B: the step costs what the batch-1
 *                           step costs in HBM time for any nb <= 16.  Same rounding points (RMSNorm, bf16 outputs, SwiGLU,
 *                           residual, bf16 logits), but K is summed in a different order than usdm_gemv: equal to f32 rounding of
 *                           the accumulation, not bit for bit (csrc/llm_mfma_k.hip).
 * form: 0 = VALU for nb <= 4, matrix cores above; 1 = matrix cores; -1 = VALU (nb <= 4 only); 3 = matrix cores with
 * fragment-shaped weight loads (A/B of the load pattern); 5 = matrix cores without the workgroup-level K split. */
typedef struct usdm_gemv_batch_args {
  usdm_gemv_args g;          /* x_delta / x_out must be NULL */
  int32_t nb;
  int64_t x_bs, y_bs, res_bs; /* element strides between items of x, y16 / y32, residual */
  int32_t part_bs;            /* element stride between items of part_val / part_idx (>= usdm_gemv_nblocks; the matrix-core form
                                 writes one partial per workgroup (<= 256) and fills the rest with "no candidate") */
  int32_t form;
  /* Matrix-core form, K split over workgroups (round 4; K > 4096 = down_proj): with ks_part / ks_cnt given and K %% 2048 == 0 (no
   * RMSNorm, SwiGLU or lm_head mode) workgroup (s, j) multiplies K slice s (2048 wide, its activation slice HELD in registers) of its
   * 16-row tiles; the K / 2048 partial tiles meet in ks_part (write-through stores), the workgroup that arrives last at a tile's
   * counter sums them in slice order (deterministic) and runs the epilogue.  ks_part: usdm_gemv_batch_ks_floats(N, K) floats;
   * ks_cnt: ceil(N / 16) int32, ZERO when the launch starts (every launch leaves them zero).  form 5 = do not split. */
  float* ks_part; int32_t* ks_cnt; int64_t ks_part_floats;
} usdm_gemv_batch_args;
int64_t usdm_gemv_batch_ks_floats(int32_t N, int32_t K);   /* 0: this shape is not split */
int usdm_gemv_batch(const usdm_gemv_batch_args* args, usdm_stream_t stream);

/* What the matrix-core launcher decides for a shape, asked on the host (no HIP call, no device needed): the one selection that
 * usdm_gemv_batch (forms 1 / 3 / 5), usdm_gemv_fp8_mfma and usdm_gemv_mxfp4_mfma launch from.
 * flags: bit 0 SwiGLU, bit 1 fused RMSNorm, bit 2 lm_head mode, bit 3 ks_part / ks_cnt given.  form: as usdm_gemv_batch_args.form.
 * fmt: 0 bf16, 1 FP8, 2 MXFP4.  Returns 0 and fills *out, or non-zero with usdm_last_error() for a shape the launcher refuses. */
typedef struct usdm_gemv_mfma_plan {
  int32_t hold, cpwt, trl;   /* the kernel variant: activations held in registers; K chunks per wave as a constant (0: any); row-contiguous
                                loads re-cut through LDS */
  int32_t rt;                /* rows per tile */
  int32_t ksplit;            /* K slices over workgroups (1: not split) */
  int32_t ntiles, nout;
  int32_t cpw;               /* K chunks of 32 per wave */
  int32_t grid, kwg;         /* workgroups; workgroups that share the tiles of a K slice (= grid when not split) */
  int32_t lds_bytes;
} usdm_gemv_mfma_plan;
int usdm_gemv_mfma_select(int32_t N, int32_t K, int32_t flags, int32_t form, int32_t fmt, usdm_gemv_mfma_plan* out);
int usdm_sizeof_gemv_mfma_plan(void);

/* Weight-only FP8 decode GEMV (opt-in, usdm_amd/quant.py): b.g.W holds OCP e4m3fn bytes [N][ldw] (row-major, ldw in elements =
 * bytes, a multiple of 8) and row r is scaled by 2^row_exp[r].  Every dequantized weight q * 2^e is a bf16 value, and the kernels
 * convert it exactly in registers and then run the bf16 arithmetic unchanged: the result equals usdm_gemv (nb = 1) or the VALU
 * form of usdm_gemv_batch (nb = 2..4) on the bf16 matrix W' = q * 2^e, bit for bit.  Supported: the plain single-GPU forms
 * (RMSNorm, SwiGLU, residual, lm_head mode, skip).  Not supported (error, no fall-back): nb > 4 / the matrix-core forms, p2p,
 * mrg_* / cmb_gran, x_delta / x_out. */
typedef struct usdm_gemv_fp8_args {
  usdm_gemv_batch_args b;    /* nb = 1: batch-1 kernel (strides unused); 2..4: the VALU batch kernel; form must be 0 or -1 */
  const int8_t* row_exp;     /* [N] */
} usdm_gemv_fp8_args;
int usdm_gemv_fp8(const usdm_gemv_fp8_args* args, usdm_stream_t stream);
/* The matrix-core form with FP8 weights (opt-in, 1..16 sequences): b.nb 1..16, b.form 0 (K split over workgroups where b.ks_*
 * allow it, as in usdm_gemv_batch) or 5 (no K split).  The bytes are converted exactly to bf16 in registers and the bf16
 * matrix-core arithmetic runs unchanged (same tiles, chunk order, wave merge, K split and epilogues): the result equals
 * usdm_gemv_batch(form = 1, or 5) with the same ks_* arguments on W' = q * 2^e, bit for bit (like that form, NOT bit-identical
 * with usdm_gemv / the VALU form).  W 16-byte aligned, ldw a multiple of 16, x 16-byte aligned.  Refused (error, no fall-back):
 * nb > 16, any other form, p2p, mrg_* / cmb_gran, x_delta / x_out, and every shape the bf16 matrix-core form refuses (K %% 256,
 * the fused RMSNorm with K > 4096, more than 64 tiles per workgroup). */
int usdm_gemv_fp8_mfma(const usdm_gemv_fp8_args* args, usdm_stream_t stream);
/* out[r][k] = bf16(e4m3(q[r][k]) * 2^row_exp[r]) for r < N, k < K (prefill: the bf16 operand of usdm_gemm).  K, ldq and ldo
 * multiples of 8; q 8-byte and out 16-byte aligned. */
int usdm_dequant_fp8(const void* q, const int8_t* row_exp, int32_t N, int32_t K, int64_t ldq, void* out, int64_t ldo,
                     usdm_stream_t stream);
int usdm_sizeof_gemv_fp8_args(void);

/* Weight-only MXFP4 (opt-in; usdm_amd/quant.py): OCP e2m1 codes (magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 the sign) with one
 * e8m0 scale byte (2^(byte - 127)) per block of 32 consecutive K elements of a row.  Every W'[r][k] = e2m1(code) * 2^s is exactly
 * a bf16 value.  Memory layout (private to quant.Mxfp4Weight, which is the one packer): a row is cut into groups of 2048 elements,
 * the last one padded with zero codes and scale bytes 127.  A group is 1024 code bytes = 64 pieces of 16 bytes; dword i (0..3) of
 * piece L holds elements 2048g + 512i + 8L .. +7 of the row, element 2m of a byte pair in bits 3:0 and 2m+1 in bits 7:4.  The
 * group's 64 scale bytes are 16 dwords; byte i of dword q is the scale of block 64g + 16i + q.  b.g.W points to the codes with
 * row stride b.g.ldw BYTES (a multiple of 1024, 2 * ldw >= K), scales to the scale bytes with row stride lds bytes (a multiple of
 * 64, 32 * lds >= K); W 16-byte and scales 4-byte aligned, K a multiple of 32.
 * usdm_gemv_mxfp4 converts the codes to bf16 in registers (exact) and runs the bf16 arithmetic unchanged: the result equals usdm_gemv
 * (nb = 1) / the VALU form of usdm_gemv_batch (nb = 2..4) on the bf16 matrix W', bit for bit.  Supported: RMSNorm, SwiGLU on packed
 * gate/up rows, residual, plain, skip.  Refused (error, no fall-back): nb > 4 / the matrix-core forms, the lm_head mode
 * (part_val / ban; y32 is refused too), p2p, mrg_* / cmb_gran, x_delta / x_out, misaligned pointers or strides. */
typedef struct usdm_gemv_mxfp4_args {
  usdm_gemv_batch_args b;    /* nb = 1: batch-1 kernel (strides unused); 2..4: the VALU batch kernel; form must be 0 or -1 */
  const uint8_t* scales;     /* [N][lds] */
  int64_t lds;
} usdm_gemv_mxfp4_args;
int usdm_gemv_mxfp4(const usdm_gemv_mxfp4_args* args, usdm_stream_t stream);
/* out[r][k] = W'[r][k] as bf16 for r < N, k < K (prefill: the bf16 operand of usdm_gemm).  codes / ldw / scales / lds as above;
 * K a multiple of 32, ldo a multiple of 8, out 16-byte aligned. */
int usdm_dequant_mxfp4(const void* codes, int64_t ldw, const uint8_t* scales, int64_t lds, int32_t N, int32_t K, void* out,
                       int64_t ldo, usdm_stream_t stream);
int usdm_sizeof_gemv_mxfp4_args(void);

/* The matrix-core form with MXFP4 weights (opt-in, 1..16 sequences).  It reads a SECOND image of the matrix, cut for waves that own
 * contiguous K chunks of 32 (quant.Mxfp4Weight.with_matrix_core_image is the one packer): a row is K / 2 code bytes; for every quad Q
 * of four consecutive chunks (128 elements, 64 bytes) 16-byte piece g (0..3) holds four dwords, dword j the 8 codes of elements
 * 128 Q + 32 j + 8 g .. + 7, the earlier element of a byte in bits 3:0.  Lane (row r, g) of a wave so fetches its A fragments of four
 * chunks with one 16-byte load (16 rows x 64 contiguous bytes per wave instruction), or dword j alone where a wave's share of K is
 * no whole number of quads.  scales is plain [N][K / 32] e8m0 bytes: the dword at byte 4 Q of a row holds the scales of quad Q.
 * ldc / lds: the row strides of codes / scales in bytes (ldc >= K / 2, a multiple of 16; lds >= K / 32, a multiple of 4); codes
 * 16-byte, scales 4-byte aligned.  b.g.W and b.g.ldw are not read.
 * b.nb 1..16, b.form 0 (K split over workgroups where b.ks_* allow it, as in usdm_gemv_batch) or 5 (no K split).  The codes are
 * converted exactly to bf16 in registers (one scale per row and chunk) and the bf16 matrix-core arithmetic runs unchanged: the same
 * tiles, rows per tile, K chunks per wave and their order, wave merge, K split with its slice-order merge and epilogues, so the result
 * equals usdm_gemv_batch(form = 1, or 5) with the same ks_* arguments on W', bit for bit.  Supported: RMSNorm (K <= 4096), SwiGLU on
 * packed gate/up rows, residual, plain; y16 only.  Refused (error, no fall-back): nb > 16, any other form, the lm_head mode
 * (part_val / part_idx / ban / y32), p2p, mrg_* / cmb_gran, x_delta / x_out, misaligned pointers or strides, and every shape the
 * bf16 matrix-core form refuses (K %% 256, the fused RMSNorm with K > 4096, more than 64 tiles per workgroup). */
typedef struct usdm_gemv_mxfp4_mfma_args {
  usdm_gemv_batch_args b;
  const void* codes;         /* [N][ldc] bytes, the matrix-core image */
  int64_t ldc;
  const uint8_t* scales;     /* [N][lds] */
  int64_t lds;
} usdm_gemv_mxfp4_mfma_args;
int usdm_gemv_mxfp4_mfma(const usdm_gemv_mxfp4_mfma_args* args, usdm_stream_t stream);
int usdm_sizeof_gemv_mxfp4_mfma_args(void);

/* Lossless 13-bit image of a bf16 weight matrix (default on for the 7B's down_proj; usdm_amd/wpack.py is the one packer).  The
 * exponent field of a weight matrix is almost constant, so a weight b (its 16 bits) is stored as its low byte b & 0xff, the 4-bit
 * index ((b >> 8) & 0x7f) - base of its upper seven exponent bits, and its sign: 13 bits, rebuilt exactly in registers.  base is
 * one value per matrix.  A row that holds a weight whose index is outside 0..15 (zeros, denormals, inf / NaN, ...) is marked in
 * rowflag and streamed from the bf16 matrix instead, so the result never depends on the data.
 * Layout: row r starts at planes + r * stride and is K / 2048 units of 3328 bytes; unit u covers elements 2048 u .. +2047, i.e.
 * the four K iterations 4u .. 4u + 3 of the bf16 kernels, in which lane L owns elements e(i, k) = 2048 u + 512 i + 8 L + k:
 *   bytes    0 .. 1023  low bytes: byte 16 L + 8 i + k of element e(i, k), i = 0, 1
 *   bytes 1024 .. 2047  the same for i = 2, 3
 *   bytes 2048 .. 3071  nibbles: dword 4 L + i holds in byte k (0..3) the index of e(i, k) in bits 3:0 and of e(i, k + 4) in 7:4
 *   bytes 3072 .. 3327  signs: dword L holds the sign of e(i, k) at bit 8 (k & 3) + 7 - (2 i + (k >> 2))
 * usdm_gemv_packed(args, pack) computes exactly usdm_gemv(args), bit for bit: where usdm_gemv would run the straight-line
 * K = 14336 form (see usdm_gemv_args.resident) the unmarked rows stream the image; every other call is usdm_gemv itself. */
typedef struct usdm_gemv_wpack {
  const void* planes;        /* 16-byte aligned */
  const uint8_t* rowflag;    /* [N rounded up to 4]: non-zero = the row streams from args->W (the packer's record; see marked) */
  int64_t stride;            /* bytes between rows: a multiple of 16, >= K / 2048 * 3328 */
  int32_t base;              /* 0 .. 112 */
  int32_t units;             /* K / 2048 */
  /* rowflag as bits (bit r of the array = row r is marked), the copy the kernel reads: a kernel argument, so no memory round trip
   * stands in front of the first weight load.  At most 14336 rows. */
  uint32_t marked[448];
} usdm_gemv_wpack;
int usdm_gemv_packed(const usdm_gemv_args* args, const usdm_gemv_wpack* pack, usdm_stream_t stream);
int usdm_gemv_packs(const usdm_gemv_args* args);   /* 1 where usdm_gemv_packed streams the image of this projection */
int usdm_sizeof_gemv_wpack(void);
/* The same image of an interleaved gate/up matrix (a SwiGLU call: N rows = blocks of 16 gate + 16 up rows, N / 2 outputs).  The
 * byte layout per ROW is the one above, K = 4096 = 2 units; planes, rowflag, stride, base and units mean what they mean above, with
 * rowflag still one byte per weight row.  Only `marked` differs: bit o of the array = OUTPUT o is marked, i.e. its gate row
 * 32 (o >> 4) + (o & 15) or its up row (that + 16) holds a weight outside the window; at most 14336 outputs.  A wave of the kernel
 * that owns a marked output streams its rows from the bf16 matrix.
 * usdm_gemv_packed_glu(args, pack) computes exactly usdm_gemv(args), bit for bit.  usdm_gemv_packs_glu is 1 where it streams the
 * image: where usdm_gemv would run the straight-line resident form of gate/up - a plain bf16 SwiGLU call, no x_delta, K = 4096 and
 * two tiles on every resident workgroup (see usdm_gemv_args.resident; the device is asked how many it holds, so the query needs
 * one where the rest applies).  Every other call is usdm_gemv itself.  Refused: units != 2, a stride below 2 * 3328 or no multiple
 * of 16, planes not 16-byte aligned, base outside 0..112, N / 2 > 14336. */
int usdm_gemv_packed_glu(const usdm_gemv_args* args, const usdm_gemv_wpack* pack, usdm_stream_t stream);
int usdm_gemv_packs_glu(const usdm_gemv_args* args);

/* Device-resident greedy-decode state so that a decode step is replayable as one hipGraph. */
typedef struct usdm_decode_state {
  int32_t* next_token;  /* [1] token fed to the next step                     */
  int32_t* out_tokens;  /* [max_out] generated ids                            */
  int32_t* step;        /* [1] number of generated tokens so far              */
  int32_t* pos;         /* [1] number of tokens in the KV cache               */
  int32_t max_out, id_offset, advance_pos;
  int32_t batch;        /* batched decode: 0 or 1 = single; else arrays of `batch` items: next_token[b], step[b], pos[b],
                           out_tokens[b][max_out] */
  /* device-side end of sequence (optional; all device memory so that a captured graph follows per-call settings):
   * eos = { n_eos (<= 6), min_new, id0, id1, ... }.  Once the picked token is one of the ids and at least min_new tokens
   * exist, done[b] is set; later calls with done[b] != 0 return without touching the state.  The decode kernels take
   * the same word as `skip` and return at once, so steps launched past the EOS cost launch overhead only. */
  int32_t* done; const int32_t* eos;
} usdm_decode_state;
/* arg-max over the per-block partials (ties -> lowest id = torch.argmax on the masked logits; with
 * do_sample=True, top_k=1 the reference samples among exact ties, of which this is one outcome). */
int usdm_argmax_final(const float* part_val, const int32_t* part_idx, int32_t nparts,
                      const usdm_decode_state* st, const void* embed_table_bf16, int32_t Hd, void* h_out_bf16,
                      usdm_stream_t stream);
/* The same pick over nseg SEGMENTS of nparts partials per sequence, seg_stride elements apart (sequence b's partials of segment s
 * start at s * seg_stride + b * nparts): the tensor-parallel batched decode step all-gathers the ranks' [sequences][nparts] blocks
 * into [rank][sequences][nparts] (SURVEY.md 8e + 8f-2). */
int usdm_argmax_final_seg(const float* part_val, const int32_t* part_idx, int32_t nparts, int32_t nseg, int64_t seg_stride,
                          const usdm_decode_state* st, const void* embed_table, int32_t Hd, void* h_out, usdm_stream_t stream);  /* embed_table != NULL: also h_out = table[token] (next step's input);
                                                 batched state: part_val/part_idx are [batch][nparts], h_out [batch][Hd] */

/* Sampling twin of usdm_argmax_final: temperature -> top-k -> top-p (HF TemperatureLogitsWarper, TopKLogitsWarper,
 * TopPLogitsWarper: generate(do_sample=True, top_k, top_p, temperature) of src/inference.py:63-83 with the knobs the demo
 * exposes, streamlit_demo.py:201-211) and one multinomial draw with Philox4x32-10(seed, counter = *st->step).
 * logits: f32 [V] of this step with banned ids = -inf (usdm_gemv lm_head mode writes exactly that into y32).
 * top_k = 0 and top_p = 1 switch the filters off.  Ties at a filter boundary are kept or dropped as a block (HF's
 * unstable sort picks arbitrarily).  probs_out (optional, [V]) receives the filtered, renormalised distribution.
 * If no id has positive mass (every logit banned or NaN) the arg-max of the finite logits is taken, else id 0: the
 * kernel never emits an id outside [0, V).
 * min_p (HF MinPLogitsWarper, vLLM; 0 = off): after temperature, top-k and top-p an id is dropped when p_i < min_p * p_max.  The
 * ratio p_i / p_max = exp(x_i / T - max / T) does not change under renormalisation and the maximum survives top-k and top-p, so the
 * kept set is the intersection of the top-k test, the top-p test and e_i >= min_p, e_i being the f32 softmax numerator of the other
 * stages; draw and probs_out honour it.  With top_k = 1 it changes nothing. */
typedef struct usdm_sample_params {   /* the per-request knobs (vLLM SamplingParams of inference_vllm.py:42-66) */
  float temperature; int32_t top_k; float top_p;
  float min_p;   /* in [0, 1]; zero bits = off.  A device value outside the range (NaN included) is taken as 0 */
  uint64_t seed;
} usdm_sample_params;
typedef struct usdm_sample_args {
  const float* logits; int32_t V;
  float temperature; int32_t top_k; float top_p;
  uint64_t seed;
  float* probs_out;
  /* optional DEVICE copy of the knobs: when non-NULL it overrides temperature / top_k / top_p / seed above, so that one
   * captured decode graph serves every request (the host rewrites 24 bytes instead of re-capturing per seed). */
  const usdm_sample_params* dev_params;
  /* batched decode (usdm_decode_state.batch > 1): sequence b reads logits + b * logits_bs, dev_params[b] (required), the state
   * words [b] and writes h_out + b * Hd and probs_out + b * V (contiguous [batch][V], also where logits_bs > V); its Philox
   * counter is ITS step, so its tokens equal those of the single-sequence call
   * (per-slot sampling inside a continuous batch: src/inference_vllm.py:109-123 passes one SamplingParams per request). */
  int64_t logits_bs;
  float min_p;   /* [0, 1], 0 = off (dev_params: the block's) */
} usdm_sample_args;
int usdm_sample_final(const usdm_sample_args* args, const usdm_decode_state* st, const void* embed_table_bf16, int32_t Hd,
                      void* h_out_bf16, usdm_stream_t stream);
/* The same draw over a row of nseg SEGMENTS (tensor parallelism: the ranks' lm_head shards gathered rank-major): id i (0 <= i < V)
 * of sequence b is read at logits + (i / seg_len) * seg_stride + b * logits_bs + i % seg_len.  nseg = 1, seg_len >= V is the
 * contiguous row; the batched tensor-parallel step gathers [rank][sequence][Vloc] and passes nseg = tp, seg_len = logits_bs = Vloc,
 * seg_stride = batch * Vloc.  Ids >= V are never read (the last rank's padding slots need no fill).  probs_out is contiguous
 * [batch][V].  Histograms and masses are integer sums, so token, kept set and probs_out are bit-identical with usdm_sample_final
 * on the same logical row.  Needs 2 <= seg_len <= 2^20 and nseg * seg_len >= V. */
int usdm_sample_final_seg(const usdm_sample_args* args, int32_t nseg, int64_t seg_stride, int32_t seg_len, const usdm_decode_state* st,
                          const void* embed_table_bf16, int32_t Hd, void* h_out_bf16, usdm_stream_t stream);

/* Per-token log-probabilities of the step whose token usdm_sample_final has JUST picked, from the same ban-masked f32 row (after a
 * host logits hook: the row as the hook left it).  lp(i) = x_i - logsumexp(x) over ids 0 .. V-1: the model's distribution over the
 * allowed ids BEFORE temperature, top-k and top-p, independent of the sampling knobs (vLLM's "raw" log-probabilities; its versions
 * differ on the default).  The pick has already advanced *st->step, so the row index is t = *st->step - 1, and the picked id is
 * *st->next_token - st->id_offset.  Written for that t:
 *   tok_lp[t]            lp of the picked token
 *   tok_rank[t]          1 + number of ids whose logit is strictly greater than the picked one (vLLM's rank)
 *   top_id / top_lp      [t][K]: the K most likely ids in descending log-probability, exact ties by lowest id first; 0 <= K <= 20
 *                        (K = 0: not written, may be NULL); with V < K the tail is id -1, lp -inf
 * A row with no finite logit gives -inf everywhere (never NaN); NaN appears only if the row holds one.  t >= st->max_out or t < 0
 * writes nothing.  Exact and deterministic: radix select on unique (value, id) keys, the sum behind the logsumexp is an integer
 * fixed-point sum, so the same logical row gives bit-identical output single or batched, contiguous or segmented.
 * count [batch] (device, rows written so far; the caller zeroes it with st->step): a row is written only while count[b] < *st->step,
 * and count[b] = *st->step afterwards.  REQUIRED with a device-side st->done: the pick of the final token sets `done` and still gets
 * its row, replays after it (step no longer moves) write nothing.  NULL: every launch writes row t. */
typedef struct usdm_logprob_args {
  const float* logits; int32_t V; int32_t K;
  int64_t logits_bs;        /* batched (st->batch > 1): sequence b reads logits + b * logits_bs */
  float* tok_lp; int32_t* tok_rank; int32_t* top_id; float* top_lp;
  int64_t tok_bs, top_bs;   /* batched: per-sequence strides (elements) of tok_lp / tok_rank (>= max_out) and top_id / top_lp (>= max_out * K) */
  int32_t* count;
} usdm_logprob_args;
int usdm_logprobs(const usdm_logprob_args* args, const usdm_decode_state* st, usdm_stream_t stream);
/* The same over a row of nseg segments, addressed as usdm_sample_final_seg addresses it (ids >= V never read). */
int usdm_logprobs_seg(const usdm_logprob_args* args, int32_t nseg, int64_t seg_stride, int32_t seg_len, const usdm_decode_state* st,
                      usdm_stream_t stream);
int usdm_sizeof_logprob_args(void);

/* Log-probabilities of tokens the caller SUPPLIED: a chunk of f32 logits rows of a prompt scored against the prompt's own next ids.
 * Row r (0 <= r < rows) of the chunk, at logits + r * logits_bs, is prompt row row0 + r (the lm_head over the hidden state of that
 * position); its target is ids[row0 + r + 1], and every output is indexed by the TARGET's row t = row0 + r + 1:
 *   tok_lp[t], tok_rank[t]     log p(ids[t] | ids[< t]) and its vLLM rank
 *   top_id / top_lp            [t][K], as usdm_logprobs writes them (K = 0: not written, may be NULL)
 * so the caller's buffers hold n_ids rows (n_ids * K for the top lists); rows outside row0 + 1 .. row0 + rows are not touched.
 * The quantities and the arithmetic are usdm_logprobs' (2^40 fixed-point sum, f64 log, one rounding to f32; radix select on unique
 * (value, id) keys): the same row and target give the same bits from both.  A target id outside [0, V) is reported with lp -inf
 * (and the rank of -inf); a row with no finite logit gives -inf everywhere, never NaN.  Nothing is banned or edited: the rows are
 * the raw model's distribution over all V ids (vLLM's prompt_logprobs).  One workgroup per row; no host synchronisation.
 * Refused: null pointers, K outside 0 .. 20, V outside 1 .. 2^20, rows < 1, row0 < 0, row0 + rows + 1 > n_ids, logits_bs < V. */
typedef struct usdm_prompt_logprob_args {
  const float* logits; int32_t V; int32_t K;
  int64_t logits_bs;          /* elements between two rows of the chunk */
  const int64_t* ids;         /* the prompt's ids (device) */
  int32_t n_ids;
  int32_t row0, rows;         /* first prompt row of the chunk, rows in the chunk */
  float* tok_lp; int32_t* tok_rank; int32_t* top_id; float* top_lp;
} usdm_prompt_logprob_args;
int usdm_prompt_logprobs(const usdm_prompt_logprob_args* args, usdm_stream_t stream);
/* The same over rows of nseg segments (the vocab-parallel lm_head: the ranks' [rows][seg_len] chunks gathered rank-major): id i of
 * row r is read at logits + (i / seg_len) * seg_stride + r * logits_bs + i % seg_len; ids >= V are never read.  Needs
 * 2 <= seg_len <= 2^20, nseg * seg_len >= V, logits_bs >= seg_len and seg_stride >= logits_bs * (rows - 1) + seg_len.  Bit-identical
 * with usdm_prompt_logprobs on the same logical rows. */
int usdm_prompt_logprobs_seg(const usdm_prompt_logprob_args* args, int32_t nseg, int64_t seg_stride, int32_t seg_len,
                             usdm_stream_t stream);
int usdm_sizeof_prompt_logprob_args(void);

/* Repetition / frequency / presence penalties of the step whose token usdm_sample_final is ABOUT to pick, applied in place to the
 * ban-masked f32 row it will read (before a host logits hook, which sees the penalised row).  State per sequence: table[V], one
 * int32 per id: c(i) = how often id i was generated so far in this call in bits 0 .. 29, in_prompt(i) in bit 30 (the caller zeroes
 * the table per request and sets bit 30 of every prompt id).  One launch
 *   1. counts the token picked by the previous step, out_tokens[*st->step - 1] - st->id_offset, when *st->step >= 1;
 *   2. rewrites x of every id i < V, each line one f32 operation (no contraction):
 *        seen = in_prompt(i) or c(i) > 0
 *        x = seen ? (x < 0 ? x * r : x / r) : x       repetition (HF RepetitionPenaltyLogitsProcessor; vLLM: prompt + output)
 *        x = x - (f * float(c(i)))                    frequency  (vLLM: output tokens only)
 *        x = x - (p * (c(i) > 0 ? 1.0f : 0.0f))       presence   (vLLM: output tokens only)
 *      -inf stays -inf, NaN stays NaN.  With the neutral knobs r = 1, f = 0, p = 0 the row is not touched (the token is still counted).
 * The knobs are a DEVICE block, one per sequence, rewritten by the host per request: plans and graphs never depend on the values.
 * Ranges (vLLM): r in (0, 2], f and p in [-2, 2]; usdm_penalty_params_init fills a host block and refuses anything else, NaN
 * included.  (A device block outside the ranges, such as a zero-filled one, is taken as neutral.)
 * count [batch] (device, *st->step at the last counting; the caller zeroes it with st->step): a token is counted only while
 * count[b] < *st->step, and count[b] = *st->step afterwards, so a replay at the same step counts nothing.  REQUIRED with a device-side
 * st->done, and the launch then returns at once when done[b] != 0.  NULL: every launch with *st->step >= 1 counts.
 * At every pick c is exactly the histogram of out_tokens[0 .. *st->step - 1]. */
typedef struct usdm_penalty_params { float repetition, frequency, presence; int32_t reserved; } usdm_penalty_params;
typedef struct usdm_penalty_args {
  float* logits; int32_t V;
  int64_t logits_bs;        /* batched (st->batch > 1): sequence b's row is logits + b * logits_bs */
  int32_t* table;
  int64_t table_bs;         /* batched: sequence b's table is table + b * table_bs (>= V) */
  const usdm_penalty_params* dev_params;   /* [batch], 16-byte aligned */
  int32_t* count;
} usdm_penalty_args;
int usdm_penalize(const usdm_penalty_args* args, const usdm_decode_state* st, usdm_stream_t stream);
/* The same over a row of nseg segments, addressed as usdm_sample_final_seg addresses it (ids >= V never read or written). */
int usdm_penalize_seg(const usdm_penalty_args* args, int32_t nseg, int64_t seg_stride, int32_t seg_len, const usdm_decode_state* st,
                      usdm_stream_t stream);
int usdm_penalty_params_init(usdm_penalty_params* out, float repetition, float frequency, float presence);
int usdm_sizeof_penalty_args(void);
int usdm_sizeof_penalty_params(void);

/* Additive logit bias and the n-gram ban of the step whose token usdm_sample_final is ABOUT to pick, applied in place to the
 * ban-masked f32 row it will read, in front of usdm_penalize (HF's and vLLM's order: bias, then penalties), a host logits hook and
 * the pick.  One workgroup per sequence, two phases with a barrier between them:
 *   1. bias (OpenAI / vLLM logit_bias, HF SequenceBiasLogitsProcessor with single-token keys): for t < n_bias
 *        x[bias_id[t]] = x[bias_id[t]] + bias_val[t]          one f32 add; -inf stays -inf, NaN stays NaN
 *      The ids of a sequence are distinct (the caller's duty); entries outside [0, V) are ignored.  n_bias <= bias_max <= 1024.
 *   2. n-gram ban (HF NoRepeatNGramLogitsProcessor, no_repeat_ngram_size = n >= 1): the history is the prompt followed by the tokens
 *      generated so far, hist[j] = j < P ? prompt[j] : out_tokens[j - P] - st->id_offset, of length Lh = P + *st->step, read where it
 *      lives (no copy is kept).  When Lh >= n: for every j in 0 .. Lh - n with hist[j .. j+n-2] equal to the last n - 1 tokens,
 *        x[hist[j+n-1]] = -inf
 *      (n = 1: the tail is empty and every id of the history is banned).  An id that is both biased and banned ends at -inf.  The
 *      prefill's pick has *st->step = 0: its history is the prompt.  *st->step above st->max_out counts as max_out.
 * Per-sequence state, all DEVICE memory rewritten by the host per request, so plans and graphs never depend on the values:
 * dev_params[b] = {ngram n (<= 0: off), prompt_len P (0 .. prompt_max), n_bias}, the rows bias_id / bias_val and the row prompt.
 * A sequence with n_bias = 0 and n <= 0 (a zero-filled block) neither reads nor writes its row.  With a device-side st->done the
 * launch returns at once when done[b] != 0. */
typedef struct usdm_logit_edit_params { int32_t ngram, prompt_len, n_bias, reserved; } usdm_logit_edit_params;
typedef struct usdm_logit_edit_args {
  float* logits; int32_t V;
  int64_t logits_bs;        /* batched (st->batch > 1): sequence b's row is logits + b * logits_bs */
  const usdm_logit_edit_params* dev_params;   /* [batch], 16-byte aligned */
  const int32_t* bias_id; const float* bias_val;
  int32_t bias_max;         /* entries a bias row holds, 0 .. 1024 (0: the rows may be NULL) */
  int64_t bias_bs;          /* batched: sequence b's bias rows are bias_id + b * bias_bs, bias_val + b * bias_bs (>= bias_max) */
  const int32_t* prompt;
  int32_t prompt_max;       /* ids a prompt row holds (0: the row may be NULL) */
  int64_t prompt_bs;        /* batched: sequence b's prompt row is prompt + b * prompt_bs (>= prompt_max) */
} usdm_logit_edit_args;
int usdm_logit_edit(const usdm_logit_edit_args* args, const usdm_decode_state* st, usdm_stream_t stream);
/* The same over a row of nseg segments, addressed as usdm_sample_final_seg addresses it (ids >= V never read or written). */
int usdm_logit_edit_seg(const usdm_logit_edit_args* args, int32_t nseg, int64_t seg_stride, int32_t seg_len, const usdm_decode_state* st,
                        usdm_stream_t stream);
int usdm_sizeof_logit_edit_args(void);
int usdm_sizeof_logit_edit_params(void);

/* Beam search, the pick of the batched decode step of B = st->batch beams in lockstep (1 .. 16; batch 0 counts as 1), in place of usdm_sample_final.
 * Rows b < nlive of the ban-masked f32 logits are live (nlive = 1 on the first step, where all beams are still the prompt: this
 * replaces HF's -1e9 initial scores; else nlive = B).  Per live row lp_b(i) = x_i - logsumexp(x) with exactly usdm_logprobs'
 * arithmetic (max, 2^40 fixed-point sum, f64 log, one rounding to f32; banned ids -inf) and s(b, i) = score[b] + lp_b(i), one f32
 * addition.  Selected are the KC = max(2, 1 + n_eos) * B largest s (HF's beams_to_keep) under the TOTAL order: value descending,
 * then flat index b * V + i ascending, -0.0 folded into +0.0; composite (value, index) keys are unique, so the selection is exact.
 * Written, for t = step[0] (t >= log_rows or t >= st->max_out: the launch changes nothing):
 *   log_score / log_token / log_parent [t][KC]   the candidates in that order (token = id + st->id_offset)
 *   next_token[b], parent[b], score[b], out_tokens[b][t], h_out[b] = embed_table[next_token[b]]   for b < B: the first B candidates
 *                                                whose token is none of the n_eos ids eos[0 ..] (HF's running beams of the next
 *                                                iteration; at most n_eos * nlive of the KC are EOS, so B always remain)
 *   step[b] + 1 and (st->advance_pos) pos[b] + 1 for all b < B
 * Every sum is an integer sum and every per-id quantity depends on the value only: bit-identical run to run, and two live rows with
 * equal logits and equal scores give bit-equal candidates.  Two launches: one workgroup per live row, one merging workgroup.
 * Refused: B outside 1 .. 16, n_eos outside 0 .. 3, KC > 32, V < KC or V > 2^20, nlive outside {1, B}, logits_bs < V, a missing
 * pointer, log_rows < 1. */
#define USDM_BEAM_MAX_KC 32
typedef struct usdm_beam_args {
  const float* logits; int32_t V;
  int64_t logits_bs;           /* beam b's row is logits + b * logits_bs (>= V) */
  float* score;                /* [B] running scores, read and rewritten */
  int32_t* parent;             /* [B] out: the beam each new running beam continues */
  int32_t nlive, n_eos;
  const int32_t* eos;          /* [3] device: the EOS ids (the first n_eos are read) */
  float* log_score; int32_t* log_token; int32_t* log_parent;   /* [log_rows][KC] */
  int32_t log_rows;
  float* cand_score; int32_t* cand_index;   /* scratch [B][KC]: the rows' own best KC (value, id), between the two launches */
} usdm_beam_args;
int usdm_beam_step(const usdm_beam_args* args, const usdm_decode_state* st, const void* embed_table_bf16, int32_t Hd, void* h_out_bf16,
                   usdm_stream_t stream);
int usdm_sizeof_beam_args(void);

/* Reorder of the beams' KV rows by parent, in place: for every array a < n_arrays, block k < nblk (layer x kv head) and row r in
 * [*lo, pos[0]), slot b's row becomes what slot parent[b]'s row was BEFORE the launch, for all b < B at once; parent may be any map
 * (identity, cycles, several children of one parent).  A byte copy: array a is base[a] + b * slot_bytes[a] + k * ctx_max *
 * row_bytes[a] + r * row_bytes[a], so bf16 rows (256 B), e4m3 rows (128 B) and their int8 exponents (1 B) are the same kernel.
 * One thread owns a byte offset in ALL slots: it loads the sources of every slot with parent[b] != b, then stores them, so no
 * staging copy is needed.  parent, lo and pos are read from device memory (the launch is capturable); rows outside [lo, pos),
 * slots >= B and slots with parent[b] == b or outside [0, B) are not written.  lo < 0 counts as 0, pos[0] > ctx_max as ctx_max.
 * Refused: B outside 1 .. 16, n_arrays outside 1 .. 4, a null base, row_bytes < 1, a row_bytes >= 16 that is no multiple of 16 or
 * whose base / slot_bytes are not 16-byte aligned, slot_bytes < nblk * ctx_max * row_bytes. */
typedef struct usdm_kv_reorder_args {
  void* base[4]; int64_t slot_bytes[4]; int32_t row_bytes[4];
  int32_t n_arrays, nblk, ctx_max, B;
  const int32_t* parent; const int32_t* lo; const int32_t* pos;
} usdm_kv_reorder_args;
int usdm_kv_reorder(const usdm_kv_reorder_args* args, usdm_stream_t stream);
int usdm_sizeof_kv_reorder_args(void);

/* out[r][:] = table[ids[r]][:] (bf16 rows; ids == NULL -> single row from *next_token) */
int usdm_embed_rows(const void* table, const int64_t* ids, const int32_t* next_token, int32_t n, int32_t Hd,
                    void* out, usdm_stream_t stream);

/* Prefill: HF apply_rotary_pos_emb (bf16 rounding) in place on q,k of qkv[S][(Hq+2Hkv)*128]; roped K and
 * V appended to the caches [Hkv][ctx_max][128]; V also written transposed to vt[Hkv][128][vt_ld] for
 * usdm_attention.  cos/sin: bf16 [max_pos][64] built on the host as HF's MistralRotaryEmbedding does. */
typedef struct usdm_rope_args {
  void* qkv; int64_t ld; int32_t S, pos0, Hq, Hkv, ctx_max, max_pos;
  const uint16_t* cos; const uint16_t* sin;
  void* kcache; void* vcache; void* vt; int64_t vt_ld;
} usdm_rope_args;
int usdm_rope_cache(const usdm_rope_args* args, usdm_stream_t stream);

/* Decode attention for ONE new token (GQA, head_dim 128), context split over NS workgroups per kv head
 * + combine.  Ropes q/k of qkv[(Hq+2Hkv)*128] at position *pos, appends K,V to the caches, writes
 * out[Hq*128] bf16.  Softmax in fp32, P rounded to bf16 for PV (flash-attention-2 semantics). */
typedef struct usdm_attn_decode_args {
  const void* qkv; const int32_t* pos;
  int32_t Hq, Hkv, ctx_max, NS; float scale;
  const uint16_t* cos; const uint16_t* sin;
  void* kcache; void* vcache;
  float* pm; float* pl; float* po; /* scratch [Hq][NS], [Hq][NS], [Hq][NS][128] */
  void* out;
  int32_t* counters; /* [Hkv] zero-initialised once, self-resetting: when given (NS > 1) the workgroup that finishes a
                        kv head last merges its NS partials itself and no separate combine kernel is launched */
  /* batched decode: `batch` sequences in one launch (0 or 1 = single).  Item b reads pos[b], qkv + b*qkv_bs, caches +
   * b*cache_bs, writes out + b*out_bs (element strides); scratch is [batch][Hq][NS]...; counters [batch][Hkv]. NS > 1. */
  int32_t batch; int64_t qkv_bs, out_bs, cache_bs;
  const int32_t* skip;  /* optional (single-sequence form): *skip != 0 -> return immediately */
  int32_t defer_merge;  /* NS > 1, no counters: leave the partials (pm, pl, po) for the consumer (usdm_gemv mrg_*): no combine
                           launch, `out` is not written */
  int32_t window;       /* > 0: sliding window, the token at *pos sees keys pos-window+1 .. pos only (the NS splits divide that
                           range); 0 = the whole cache */
  unsigned long long* cmb_gran;  /* optional: the Hq*64 granules of usdm_gemv's cmb_gran hand-off, cleared by this launch */
} usdm_attn_decode_args;
int usdm_attn_decode(const usdm_attn_decode_args* args, usdm_stream_t stream);

/* FP8 KV cache (opt-in, usdm_amd/quant.py quantize_kv_rows): a cache row = the 128 values of one (token, kv head) as OCP e4m3fn
 * bytes plus ONE int8 power-of-two exponent, exactly quantize_rows of the bf16 row the bf16 cache would hold.  Caches: uint8
 * [Hkv][ctx_max][128] (16-byte aligned), exponents int8 [Hkv][ctx_max] (4-byte aligned); zero-initialised = rows of 0.0.
 *
 * usdm_attn_decode_fp8: a.kcache / a.vcache are the byte caches, a.cache_bs is in bytes, everything else as usdm_attn_decode's
 * split form (batch, window, skip, counters, defer_merge, cmb_gran).  The cached rows are converted exactly to the bf16 values
 * K' / V' in registers and the bf16 arithmetic runs unchanged: out (or the partials) equal usdm_attn_decode on the dequantized
 * caches bit for bit.  The new token's own K / V are used unquantized (as the bf16 kernel takes them from LDS, not from the cache);
 * the appended row is quantize_rows of the bf16 row usdm_attn_decode appends.  Refused (error, no fall-back): NS == 1 (the
 * one-workgroup form is not built for fp8 caches), unaligned caches / exponents, and everything usdm_attn_decode refuses. */
typedef struct usdm_attn_decode_fp8_args {
  usdm_attn_decode_args a;
  int8_t* kexp; int8_t* vexp;   /* [Hkv][ctx_max] */
  int64_t exp_bs;               /* batched: item b's exponents at kexp + b * exp_bs (a multiple of 4) */
} usdm_attn_decode_fp8_args;
int usdm_attn_decode_fp8(const usdm_attn_decode_fp8_args* args, usdm_stream_t stream);
/* Prefill twin of usdm_rope_cache: q and k roped as there (q in place); the S new K / V rows are QUANTIZED into r.kcache /
 * r.vcache (+ kexp / vexp) at positions pos0 .. pos0+S-1; the bf16 roped K rows go to kscr [Hkv][kscr_ld][128] (row s = token s of
 * this call) and V^T to r.vt [Hkv][128][vt_ld] - the unquantized operands of the prompt's own usdm_attention (either may be NULL). */
typedef struct usdm_rope_fp8_args {
  usdm_rope_args r;
  int8_t* kexp; int8_t* vexp;   /* [Hkv][ctx_max] */
  void* kscr; int64_t kscr_ld;
} usdm_rope_fp8_args;
int usdm_rope_cache_fp8(const usdm_rope_fp8_args* args, usdm_stream_t stream);
int usdm_sizeof_attn_decode_fp8_args(void);
int usdm_sizeof_rope_fp8_args(void);

/* Prefix reuse where the prefill attention's V^T is per-plan scratch (batch slots, FP8 cache): rows 0 .. n-1 of ONE layer's cache
 * of ONE sequence as the bf16 operands usdm_attention (mode 1) reads, in front of the rows the rope launch adds at offset n.
 * bf16 cache (kexp = vexp = NULL): vt[h][d][r] = vcache[h][r][d]; K is read in place by the attention, kscr must be NULL.
 * FP8 cache: kscr[h][r][:] and vt[h][:][r] are the exact dequantization byte x 2^e of the row (quant.dequantize_kv_rows; the values
 * usdm_attn_decode_fp8 computes with).  Rows / columns >= n of the destinations and the caches are not written.
 * 2 x Hkv x n x 256 bytes written (bf16 cache: half of that), 256 / 129 bytes read per row and array.
 * Refused: a null kcache / vcache / vt, caches not 16-byte aligned, exponents / vt / kscr not 4-byte aligned, n < 1, n > ctx_max,
 * vt_ld < n, kscr_ld < n, kscr with a bf16 cache, an FP8 cache without kscr or with one exponent array only. */
typedef struct usdm_kv_expand_args {
  const void* kcache; const void* vcache;  /* [Hkv][ctx_max][128], bf16 or e4m3 */
  const int8_t* kexp; const int8_t* vexp;  /* FP8 cache: [Hkv][ctx_max]; NULL = bf16 cache */
  void* kscr; int64_t kscr_ld;             /* FP8 only: bf16 [Hkv][kscr_ld][128], rows 0 .. n-1 are written */
  void* vt;   int64_t vt_ld;               /* bf16 [Hkv][128][vt_ld], columns 0 .. n-1 are written */
  int32_t Hkv, ctx_max, n;
} usdm_kv_expand_args;
int usdm_kv_expand(const usdm_kv_expand_args* args, usdm_stream_t stream);
int usdm_sizeof_kv_expand_args(void);

/* Speculative greedy decoding: decode attention for T = 1 .. 8 new tokens of ONE sequence (GQA G in {1, 2, 4},
 * head_dim 128, bf16 cache).  Row i of qkv [T][qkv_ld] is the token at position *pos + i: its q and k are roped as usdm_attn_decode
 * ropes them, its K / V rows are appended at *pos + i (bit-identical with T successive usdm_attn_decode calls) and out[i][Hq*128]
 * is its attention over keys lo_i .. *pos + i (lo_i from `window` as in usdm_attn_decode); the step's own rows come from LDS as
 * the bf16 values that are appended.  Every cached row is read once per launch for all T * G query rows of its kv head; scores and
 * PV run on v_mfma_f32_16x16x32_bf16, softmax in fp32, P rounded to bf16.
 * POSITION INVARIANCE: the result for the token at absolute position p (out row and appended rows) depends on p and the keys it
 * sees only - not on T, its row index or *pos.  Splits are the FIXED key ranges [s * C, (s + 1) * C), key tiles of 64 are aligned
 * to absolute indices, masked keys carry P = 0 exactly, and row p's partials are merged over splits 0 .. p / C in ascending order
 * with the arithmetic of usdm_attn_decode's merge.  Grid (Hkv, ceil(ctx_max / C)); workgroups past the live context exit at once.
 * Rows at positions >= ctx_max are neither appended nor computed (their out rows are not written).  *skip != 0: nothing is
 * written.  Refused (error, no fall-back): T outside 1 .. 8, G outside {1, 2, 4}, a NULL pointer, caches not 16-byte aligned,
 * qkv / out not 4-byte aligned, qkv_ld < (Hq + 2 Hkv) * 128 or odd, out_ld < Hq * 128, C no multiple of 64 or outside 64 .. 256,
 * more than 64 splits, window < 0. */
typedef struct usdm_attn_verify_args {
  const void* qkv; int64_t qkv_ld;
  const int32_t* pos;
  int32_t T, Hq, Hkv, ctx_max;
  int32_t C;                /* keys per split: a plan constant, a multiple of the key tile (64) */
  int32_t window; float scale;
  const uint16_t* cos; const uint16_t* sin;
  void* kcache; void* vcache;          /* [Hkv][ctx_max][128] bf16 */
  float* pm; float* pl; float* po;     /* scratch [T][Hq][NSP], [T][Hq][NSP], [T][Hq][NSP][128], NSP = ceil(ctx_max / C) */
  void* out; int64_t out_ld;           /* bf16 [T][out_ld] */
  const int32_t* skip;
} usdm_attn_verify_args;
int usdm_attn_verify(const usdm_attn_verify_args* args, usdm_stream_t stream);
int usdm_sizeof_attn_verify_args(void);

/* The same for B slots x T rows in one launch (batched speculative decoding).  v describes slot 0 and the arrays:
 * row b * T + i of qkv [B * T][qkv_ld] is the token at position pos[b] + i of slot b, slot b's caches start cache_bs ELEMENTS behind
 * slot b - 1's (usdm_attn_decode's cache_bs), out is [B * T][out_ld], the partials [B][T][Hq][NSP] (po: x 128), pos and skip are [B]:
 * skip[b] != 0 -> slot b writes nothing.  T is the same for every slot.  Grid (Hkv, NSP, B), the merge (Hq, T, B); workgroup
 * (kh, s, b) runs usdm_attn_verify's workgroup (kh, s) on slot b's arrays - the same device function - so slot b's out rows and
 * cache equal, bit for bit, usdm_attn_verify on that slot alone, and every point of the position-invariance contract holds per slot.
 * Rows at positions >= ctx_max are neither appended nor computed: slot b's rows never reach slot b + 1's.
 * Refused (error, no fall-back): B < 1, B * T > 16, cache_bs < Hkv * ctx_max * 128 or no multiple of 8, and everything
 * usdm_attn_verify refuses. */
typedef struct usdm_attn_verify_batch_args {
  usdm_attn_verify_args v;
  int32_t B;
  int64_t cache_bs;
} usdm_attn_verify_batch_args;
int usdm_attn_verify_batch(const usdm_attn_verify_batch_args* args, usdm_stream_t stream);
int usdm_sizeof_attn_verify_batch_args(void);

/* The end of a speculative step, in place of usdm_argmax_final: pick, accept, commit, propose, embed - one launch, one workgroup.
 * Picks g_0 .. g_{T-1}: the arg-max of row i's partials part_val / part_idx [T][nparts] (ties to the lowest id, the reduction of
 * usdm_argmax_final; no candidate -> id 0), token = id + st->id_offset.  drafts[i], i = 1 .. T-1, are the tokens that were fed as
 * rows 1 .. T-1 (-1: none, never matches).  n = the number of leading i with drafts[i + 1] == g_i.
 * Commit: with s = *st->step and lim = min(*limit, st->max_out), g_0 .. g_n go to out_tokens[s ..] until lim is reached or a stop id
 * (st->eos = {count, min_new, ids}) is emitted with at least min_new tokens out; m = the number emitted.  done is set on that stop
 * id or when s + m >= lim.  *step += m, *pos += m, next_token = the last emitted token; counters += {1, drafts >= 0 among the fed,
 * m - 1}.  s >= lim on entry: done is set and nothing else changes.
 * Propose (history = the prompt's ids + id_offset followed by out_tokens[0 .. *step), as usdm_logit_edit reads it): for n from
 * params[0] (lookup_max, <= 16) down to params[1] (lookup_min, >= 1) the MOST RECENT earlier occurrence of the last n tokens
 * (start j <= Lh - n - 1); drafts[i] = the token i - 1 places behind that occurrence's end, -1 where the history ends or nothing
 * matched.  params[2] != 0 and script != NULL: drafts[i] = script[*step + i - 1] instead (tests, tools/spec_rate.py).  A draft
 * whose id is outside [0, V) is -1.
 * Finish: h_out[0] = E[next_token], h_out[i] = E[drafts[i]] (-1: the row of id 0) for the next step.
 * propose_only != 0 (after the prefill, whose pick is already committed): only propose and finish.
 * done != 0 on entry: the launch changes nothing.  Refused: T outside 1 .. 8, a batched state, a missing pointer, Hd % 8 != 0. */
typedef struct usdm_spec_args {
  const float* part_val; const int32_t* part_idx; int32_t nparts;
  int32_t T;
  int32_t* drafts;                 /* [8] device */
  const int32_t* limit;            /* [1] device: max_new of the call */
  const int32_t* prompt; const int32_t* prompt_len; int32_t prompt_max;   /* device: the prompt's ids, their count */
  const int32_t* script;           /* [st->max_out] device or NULL */
  const int32_t* params;           /* [4] device: lookup_max, lookup_min, use_script, reserved */
  int32_t V;
  int32_t* counters;               /* [3] device: steps, drafted, accepted */
  int32_t propose_only;
} usdm_spec_args;
int usdm_spec_commit(const usdm_spec_args* args, const usdm_decode_state* st, const void* embed_table_bf16, int32_t Hd,
                     void* h_out_bf16, usdm_stream_t stream);
int usdm_sizeof_spec_args(void);

/* The same for the slots [slot_lo, slot_lo + n) of a batched state, one workgroup per slot.  st->batch = B is the
 * number of slots the arrays hold (B * T <= 16): next_token / step / pos / done [B] (done is required), out_tokens [B][max_out],
 * eos [B][8] (a stop block per slot, or NULL).  s describes slot 0 and the arrays: part_val / part_idx [B * T][nparts], drafts [B][8],
 * limit [B], prompt [B][prompt_max], prompt_len [B], script [B][st->max_out] or NULL, counters [B][3]; params [4] is shared.  h_out is
 * [B * T][Hd].  Workgroup b runs usdm_spec_commit's workgroup - the same device function - on slot b's rows b * T .. b * T + T - 1
 * and words, so every buffer equals usdm_spec_commit applied slot by slot.  done[b] != 0 on entry: slot b changes nothing (idle
 * slots are kept that way).  propose_only over a range of one slot gives an admitted request its first drafts and input rows.
 * Refused: what usdm_spec_commit refuses, B < 1 or B * T > 16, a slot range outside [0, B), done == NULL. */
typedef struct usdm_spec_batch_args {
  usdm_spec_args s;
  int32_t slot_lo, n;
} usdm_spec_batch_args;
int usdm_spec_commit_batch(const usdm_spec_batch_args* args, const usdm_decode_state* st, const void* embed_table_bf16, int32_t Hd,
                           void* h_out_bf16, usdm_stream_t stream);
int usdm_sizeof_spec_batch_args(void);

/* Speculative decoding for SAMPLED requests: the picks of the n * T rows of a verify step, drawn instead of
 * arg-maxed.  One launch, one workgroup of 1024 threads per row; row r = b * T + i belongs to sequence / slot b and reads
 * logits + r * logits_bs (f32 [V], banned ids = -inf).  It draws as usdm_sample_final does - the same text - with the knobs of
 * dev_params[b] (sanitised as there) and the Philox counter (unsigned)(step[b] + i): picks[r] is the LOCAL id that
 * usdm_sample_final commits (minus id_offset) for that row, those knobs and step[b] + i, bit for bit - top_k == 1 takes the lowest
 * id among ties, a row without mass the arg-max of its finite logits, else id 0.  The token at a position is therefore a function
 * of (its logits row, the knobs, the seed, the position) and of nothing else, which is what makes "draw, accept the draft iff it
 * equals the draw" exact and independent of the drafts.
 * Nothing else is written: no commit, no embedding row, no state word.  done != NULL and done[b] != 0: sequence b's workgroups return
 * at once and its picks keep their old values.  So does row i >= 1 unless drafts[b][1 .. i] are all >= 0: the accept loop of the
 * commit stops at the first draft that is -1 and never reads such a pick.
 * Refused: T outside 1 .. 8, n < 1, n * T > 16, V outside 1 .. 2^20, logits_bs < V with more than one row, a NULL logits,
 * dev_params, step, drafts or picks. */
typedef struct usdm_spec_sample_args {
  const float* logits; int64_t logits_bs;      /* [n * T][logits_bs] */
  int32_t V, T, n;
  const usdm_sample_params* dev_params;        /* [n] device */
  const int32_t* step;                         /* [n] device: the decode state's */
  const int32_t* done;                         /* [n] device or NULL */
  const int32_t* drafts;                       /* [n][8] device: the ids fed as rows 1 .. T-1 */
  int32_t* picks;                              /* [n * T] device */
} usdm_spec_sample_args;
int usdm_spec_sample(const usdm_spec_sample_args* args, usdm_stream_t stream);
int usdm_sizeof_spec_sample_args(void);

/* usdm_spec_commit / usdm_spec_commit_batch from GIVEN picks: picks [T] (batch: [B * T], slot b's at b * T) are the rows' LOCAL ids
 * (usdm_spec_sample's), g_i = picks[i] + st->id_offset, in place of the arg-max of the partials - part_val / part_idx / nparts are
 * not read.  Everything behind the pick - accept, stop ids, min_new, the limit, the counters, the proposal, the T embedding rows,
 * propose_only, done - is the same text as the arg-max forms'.  Refused: what those refuse, and picks == NULL unless propose_only. */
int usdm_spec_commit_picks(const usdm_spec_args* args, const int32_t* picks, const usdm_decode_state* st, const void* embed_table_bf16,
                           int32_t Hd, void* h_out_bf16, usdm_stream_t stream);
int usdm_spec_commit_batch_picks(const usdm_spec_batch_args* args, const int32_t* picks, const usdm_decode_state* st,
                                 const void* embed_table_bf16, int32_t Hd, void* h_out_bf16, usdm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * One-shot peer-to-peer all-reduce for the tensor-parallel decode step (replaces the single-GPU
 * model.generate of src/inference.py:116-123 when the 7B is sharded over the 8 GPUs of a node).  Messages are 4096 f32
 * (16 KB): pure latency, so there is no ring and no collective kernel: every rank WRITES its partial rows straight into
 * every peer's buffer over xGMI (hipIpc-mapped, uncached device memory) as 8-byte granules {tag = epoch, f32 value} -
 * the data is its own flag (one aligned 8-byte system-scope store is never torn), so no fence, no counter and no
 * separate flag store are needed; the reader polls its OWN memory.
 *
 *   buffer of one rank:  [256-B header: epoch u32, err u32, arrivals u32][parity 2][site n_sites][src rank 8][max_elems] granules
 *   epoch   : device word, starts at 1, +1 per decode step (usdm_argmax_p2p, or usdm_logits_p2p when sampling), so a captured
 *             hipGraph replays correctly
 *   arrivals: local word of usdm_logits_p2p's last-arriving workgroup (zero between launches)
 *   parity  : epoch & 1 selects the half; together with the all-to-all of usdm_argmax_p2p once per token no slot is
 *             rewritten before every reader has left it
 *   waits   : every poll is BOUNDED (timeout_ms of the 100 MHz wall clock); on expiry the kernel ORs a code into the
 *             err word - its own AND every peer's (| USDM_P2P_ERR_PEER) - and carries on with zeros; once err != 0 no
 *             kernel waits again, so a protocol bug costs one timeout and surfaces on EVERY rank as
 *             usdm_allreduce_p2p_error() != 0 - never as a hang, never as silently diverging ranks
 *   order   : partials are summed in rank order 0..world-1 on every rank -> bit-identical results on all ranks
 * Host protocol: create -> export (64-byte hipIpcMemHandle) -> exchange handles by any host channel -> import each
 * peer (other process) or attach (same process, logical ranks) -> commit.  RCCL stays the prefill / validation path.
 * ---------------------------------------------------------------------------------------------- */
enum { USDM_P2P_MAX_RANKS = 8, USDM_P2P_HANDLE_BYTES = 64, USDM_P2P_HEADER_BYTES = 256 };
enum { USDM_P2P_ERR_TIMEOUT_ROWS = 1, USDM_P2P_ERR_TIMEOUT_PICK = 2, USDM_P2P_ERR_TIMEOUT_REDUCE = 4,
       USDM_P2P_ERR_PEER = 8 /* set by ANOTHER rank that timed out (with its code): results may have diverged there */,
       USDM_P2P_ERR_TIMEOUT_LOGITS = 16 };
typedef struct usdm_p2p_dev {          /* device-visible view (device memory, constant after commit) */
  uint64_t base[8];                    /* address of rank r's buffer as mapped in THIS process; base[rank] = local */
  int32_t rank, world, n_sites, max_elems;
  uint64_t timeout_ticks;              /* 100 MHz ticks */
} usdm_p2p_dev;
typedef struct usdm_p2p usdm_p2p;      /* opaque host handle */
int64_t usdm_allreduce_p2p_bytes(int32_t n_sites, int32_t max_elems);   /* buffer size of one rank (layout above) */
int usdm_allreduce_p2p_create(int32_t rank, int32_t world, int32_t n_sites, int32_t max_elems, int32_t timeout_ms,
                              usdm_p2p** out);
int usdm_allreduce_p2p_export(const usdm_p2p* c, void* handle64);                    /* host bytes out */
int usdm_allreduce_p2p_import(usdm_p2p* c, int32_t peer, const void* handle64);      /* peer lives in another process */
int usdm_allreduce_p2p_attach(usdm_p2p* c, int32_t peer, void* peer_local_base);     /* peer lives in this process */
void* usdm_allreduce_p2p_base(const usdm_p2p* c);                                    /* this rank's buffer */
int usdm_allreduce_p2p_commit(usdm_p2p* c, usdm_stream_t stream);                    /* all peers known: publish the device view */
const usdm_p2p_dev* usdm_allreduce_p2p_dev(const usdm_p2p* c);                       /* device pointer for kernel args */
int usdm_allreduce_p2p_error(const usdm_p2p* c, int32_t* host_err, int32_t* host_epoch);  /* synchronous 8-byte read */
int usdm_allreduce_p2p_destroy(usdm_p2p* c);
/* split mode, second half (and the validation form): h[n] = bf16(h[n] + bf16(sum_r slot[site][r][n])), n < n_elems */
int usdm_allreduce_p2p_reduce(const usdm_p2p_dev* dev, int32_t site, int32_t n_elems, void* h_bf16, const int32_t* skip,
                              usdm_stream_t stream);
/* Vocab-parallel token pick: arg-max over this rank's lm_head partials, the (value, id) pair exchanged with every rank
 * through `site`, global arg-max (ties -> lowest id) identical on every rank, decode state advanced as
 * usdm_argmax_final does, epoch += 1.  One launch replaces all_gather x2 + usdm_argmax_final.
 * phase 0: put + get in one launch; phase 1 / 2: the put half / the get half as separate launches (split form). */
int usdm_argmax_p2p(const float* part_val, const int32_t* part_idx, int32_t nparts, const usdm_decode_state* st,
                    const usdm_p2p_dev* dev, int32_t site, int32_t phase, const void* embed_table_bf16, int32_t Hd,
                    void* h_out_bf16, usdm_stream_t stream);
/* Logits exchange of the SAMPLED tensor-parallel step (the sampling twin of usdm_argmax_p2p): every rank puts its Vloc ban-masked f32
 * logits as tagged granules into slot [parity][site0 + j][src = rank] of every rank's buffer (element e of the shard: site
 * site0 + e / max_elems, granule e % max_elems; one shard spans ceil(Vloc / max_elems) consecutive sites), then waits (bounded) for
 * every rank's granules and unpacks them into row_out[rank * Vloc + e]: the full [world * Vloc] row in global-id order (v0 = rank *
 * Vloc), identical on every rank, on which the unchanged usdm_sample_final draws the same token everywhere (same seed, same step).
 * Epoch += 1 per call, done by the get half's last-arriving workgroup (arrivals word), after every workgroup of the launch has read
 * the epoch.  The parity argument above still holds: this is the step's one all-to-all, and a rank can only write parity p again
 * two epochs later, i.e. after it received every peer's granules of the epoch in between, which each peer puts only after its own
 * get of parity p has finished (stream order) - nothing is rewritten before every reader has left it.  st: only its done word is
 * read (a finished sequence skips the exchange on every rank alike, epoch unchanged).  phase 0: put + get in one launch (ranks on
 * different streams / GPUs); 1 / 2: the put half / the get half (split form).  Timeouts set USDM_P2P_ERR_TIMEOUT_LOGITS. */
int usdm_logits_p2p(const float* logits, int32_t Vloc, const usdm_decode_state* st, const usdm_p2p_dev* dev, int32_t site0,
                    int32_t phase, float* row_out, usdm_stream_t stream);

/* h = bf16(h + bf16(delta)) : residual add after a tensor-parallel all-reduce of f32 partial sums */
int usdm_residual_add(void* h_bf16, const float* delta, int32_t n, usdm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * XLS-R / k-means unit extractor (third-party seamless_communication UnitExtractor.predict, call sites
 * src/inference.py:59,111-113, util/model_util.py:79-80).  fp32 throughout; GEMMs are usdm_gemm(F32).
 * ---------------------------------------------------------------------------------------------- */
/* y = layer_norm(x) over all n samples (F.layer_norm(wave, wave.shape)) */
int usdm_wave_layernorm(const float* x, int32_t n, float eps, float* y, usdm_stream_t stream);
/* first conv layer fused: Conv1d(1->512,k=10,stride) + LayerNorm(512) + GELU -> channels-last [T][512] */
int usdm_w2v_conv0(const float* x, int32_t n, int32_t T, int32_t C, int32_t k, int32_t stride, const float* w,
                   const float* b, const float* ln_g, const float* ln_b, float eps, float* out, usdm_stream_t stream);
/* in-place softmax of x[row][seg*ldseg + 0..n), pad columns [n,npad) zeroed (attention probabilities) */
int usdm_softmax_segments(float* x, int32_t rows, int32_t nseg, int32_t n, int32_t npad, int64_t ldrow, int32_t ldseg,
                          usdm_stream_t stream);
/* ids[t] = argmin_n(|x_t|^2 - 2*dots[t][n] + csq[n]) (first minimum); margin[t] = runner-up - best (optional) */
int usdm_kmeans_argmin(const float* x, int32_t T, int32_t D, const float* dots, int64_t ldd, const float* csq,
                       int32_t n_units, int64_t* ids, float* margin, usdm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mel front end of the speech prompt: get_mel / mel_spectrogram (util/model_util.py:24-38,
 * vocoder/meldataset.py:55-78).  frames = Hann-windowed, reflect-padded (pad = (n_fft-hop)/2), clamped
 * signal [T][n_fft]; the DFT is usdm_gemm(F32) against a host-built [2*nbins][n_fft] cos/-sin matrix;
 * usdm_stft_mag = sqrt(re^2+im^2+eps); mel projection + log(clamp(.,1e-5)) = usdm_gemm with
 * USDM_ACT_LOGCLAMP and transpose_out.  Sample-rate conversion is a polyphase FIR, also a usdm_gemm.
 * ---------------------------------------------------------------------------------------------- */
int usdm_stft_frames(const float* x, int32_t n, int32_t n_fft, int32_t hop, int32_t pad, const float* window,
                     float* frames, int32_t T, usdm_stream_t stream);
/* frames[t][c] = x[t*hop + c - offset], zero outside the signal (im2col for the polyphase resampler GEMM) */
int usdm_frame_signal(const float* x, int32_t n, int32_t frame_len, int32_t hop, int32_t offset, float* frames, int32_t T,
                      usdm_stream_t stream);
int usdm_stft_mag(const float* re_im, int64_t ld, int32_t T, int32_t nbins, float eps, float* out, int64_t ldo,
                  int32_t nbins_pad, usdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* USDM_HIP_H_ */
