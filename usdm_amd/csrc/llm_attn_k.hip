// Mistral-7B kernels that touch the KV cache: RoPE + cache append of the prefill (bf16 and FP8 caches) and decode attention (the
// context-split form with its three merges, the one-workgroup form, and usdm_attn_verify: several new tokens of one sequence, at the
// end of the file).  The decode GEMVs and the glue kernels are in llm_k.hip.
// Rounding points follow HF transformers' bf16 Mistral as described there.
#include "common.h"
#include "../../include/usdm_hip.h"
#include "attn_merge.h"

namespace {
// ---------------------------------------------------------------------------------------------
// RoPE (HF apply_rotary_pos_emb in bf16) helpers.  cos/sin tables are bf16 [maxpos][64].
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void rope_pair(float x1, float x2, float c, float s, float& o1, float& o2) {
  // o1 = x1*cos + (-x2)*sin ; o2 = x2*cos + x1*sin ; every product and sum rounded to bf16
  o1 = round_bf(round_bf(x1 * c) + round_bf(-x2 * s));
  o2 = round_bf(round_bf(x2 * c) + round_bf(x1 * s));
}

// prefill: in-place RoPE of q,k inside qkv [S][(Hq+2Hkv)*128]; K,V appended to the caches; V^T scratch
__global__ void rope_cache_kernel(const usdm_rope_args a) {
  const int s = blockIdx.x, hh = blockIdx.y;  // hh over Hq + 2*Hkv heads
  const int d = threadIdx.x;                  // 0..63
  const int pos = a.pos0 + s;
  bf16_t* row = (bf16_t*)a.qkv + (int64_t)s * a.ld + hh * 128;
  const float c = bf2f(a.cos[(int64_t)pos * 64 + d]), sn = bf2f(a.sin[(int64_t)pos * 64 + d]);
  if (hh < a.Hq) {
    float o1, o2;
    rope_pair(bf2f(row[d]), bf2f(row[d + 64]), c, sn, o1, o2);
    row[d] = f2bf(o1); row[d + 64] = f2bf(o2);
  } else if (hh < a.Hq + a.Hkv) {
    const int kh = hh - a.Hq;
    float o1, o2;
    rope_pair(bf2f(row[d]), bf2f(row[d + 64]), c, sn, o1, o2);
    bf16_t* kc = (bf16_t*)a.kcache + ((int64_t)kh * a.ctx_max + pos) * 128;
    kc[d] = f2bf(o1); kc[d + 64] = f2bf(o2);
  } else {
    const int vh = hh - a.Hq - a.Hkv;
    bf16_t* vc = (bf16_t*)a.vcache + ((int64_t)vh * a.ctx_max + pos) * 128;
    vc[d] = row[d]; vc[d + 64] = row[d + 64];
    if (a.vt) {
      bf16_t* vt = (bf16_t*)a.vt + (int64_t)vh * 128 * a.vt_ld;
      vt[(int64_t)d * a.vt_ld + s] = row[d];
      vt[(int64_t)(d + 64) * a.vt_ld + s] = row[d + 64];
    }
  }
}

// ---- FP8 KV cache (opt-in; usdm_amd/quant.py quantize_kv_rows): the device side of quantize_rows for ONE row of 128 bf16 values.
// e = the smallest integer with amax / 2^e <= 448 = 1.75 * 2^8, clamped to [-117, 119], 0 for a zero row (quant._row_exponents):
// from amax's exponent field and a mantissa test.  (An f32 subnormal amax has field 0 and lands on the lower clamp, where it belongs.)
__device__ __forceinline__ int kv8_row_exp(float amax) {
  const unsigned b = __builtin_bit_cast(unsigned, amax);
  if ((b & 0x7fffffffu) == 0u) return 0;
  const int e = (int)((b >> 23) & 0xffu) - 127 - 8 + ((b & 0x7fffffu) > 0x600000u ? 1 : 0);
  return min(119, max(-117, e));
}
// f32 (finite) -> OCP e4m3fn byte, round to nearest even, saturating at +-448: integer arithmetic, so that the bytes do not depend
// on a conversion instruction's corner cases (torch's float8_e4m3fn cast gives the same byte for every |x| <= 448).
__device__ __forceinline__ unsigned kv8_byte(float x) {
  const unsigned sgn = (__builtin_bit_cast(unsigned, x) >> 24) & 0x80u;
  const float ax = fminf(fabsf(x), 448.0f);
  if (ax >= 0x1p-6f) {                       // e4m3 normal: keep 3 mantissa bits (ties to even), rebias 127 -> 7
    unsigned u = __builtin_bit_cast(unsigned, ax);
    u += 0x7ffffu + ((u >> 20) & 1u);
    return sgn | ((u >> 20) - (120u << 3));
  }
  return sgn | (unsigned)rintf(ax * 512.0f);  // subnormal: multiples of 2^-9 (8 = the smallest normal, the same encoding)
}
// the calling wave's 64 lanes hold the row, x0 / x1 = elements 2 * lane, 2 * lane + 1 (bf16 values): bytes to row8, exponent to *ep
__device__ __forceinline__ void kv8_store_row(float x0, float x1, int lane, uint8_t* row8, int8_t* ep) {
  // row maximum on the magnitude BITS (monotonic for finite values): independent of how v_max treats f32 subnormals
  unsigned m = max(__builtin_bit_cast(unsigned, x0) & 0x7fffffffu, __builtin_bit_cast(unsigned, x1) & 0x7fffffffu);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  const int e = kv8_row_exp(__builtin_bit_cast(float, m));
  const float inv = fp8_row_scale(-e);       // exact power-of-two scaling
  *(unsigned short*)(row8 + 2 * lane) = (unsigned short)(kv8_byte(x0 * inv) | (kv8_byte(x1 * inv) << 8));
  if (lane == 0) *ep = (int8_t)e;
}

// prefill with an FP8 KV cache: RoPE of q,k in place as rope_cache_kernel; the quantized K / V rows + exponents go to the caches,
// the bf16 K rows and V^T that the prefill attention consumes to per-plan scratch (the prompt attends to its unquantized K / V).
// One wave per (token, head); a lane owns elements 2 * lane, 2 * lane + 1 and the rotation partner comes from lane ^ 32.
__global__ __launch_bounds__(64) void rope_cache_fp8_kernel(const usdm_rope_args a, int8_t* kexp, int8_t* vexp, bf16_t* kscr, int64_t kscr_ld) {
  const int s = blockIdx.x, hh = blockIdx.y;
  const int lane = threadIdx.x;
  const int pos = a.pos0 + s;
  bf16_t* row = (bf16_t*)a.qkv + (int64_t)s * a.ld + hh * 128;
  const int d0 = 2 * lane, dd = d0 & 63;     // rope pairs (d, d + 64): this lane holds d0, d0 + 1 of one half, lane ^ 32 the other
  const unsigned raw = *(const unsigned*)(row + d0);
  const float x0 = bf2f(raw & 0xffff), x1 = bf2f(raw >> 16);
  float y0 = x0, y1 = x1;
  if (hh < a.Hq + a.Hkv) {
    const float p0 = __shfl_xor(x0, 32, 64), p1 = __shfl_xor(x1, 32, 64);
    const float c0 = bf2f(a.cos[(int64_t)pos * 64 + dd]), s0 = bf2f(a.sin[(int64_t)pos * 64 + dd]);
    const float c1 = bf2f(a.cos[(int64_t)pos * 64 + dd + 1]), s1 = bf2f(a.sin[(int64_t)pos * 64 + dd + 1]);
    float o1, o2;
    if (lane < 32) { rope_pair(x0, p0, c0, s0, o1, o2); y0 = o1; rope_pair(x1, p1, c1, s1, o1, o2); y1 = o1; }
    else { rope_pair(p0, x0, c0, s0, o1, o2); y0 = o2; rope_pair(p1, x1, c1, s1, o1, o2); y1 = o2; }
  }
  const unsigned packed = pack_bf2(y0, y1);  // exact: y0 / y1 are bf16 values
  if (hh < a.Hq) {
    *(unsigned*)(row + d0) = packed;
  } else if (hh < a.Hq + a.Hkv) {
    const int kh = hh - a.Hq;
    // (as in rope_cache_kernel, the k section of qkv itself stays unroped)
    if (kscr) *(unsigned*)(kscr + ((int64_t)kh * kscr_ld + s) * 128 + d0) = packed;
    kv8_store_row(y0, y1, lane, (uint8_t*)a.kcache + ((int64_t)kh * a.ctx_max + pos) * 128, kexp + (int64_t)kh * a.ctx_max + pos);
  } else {
    const int vh = hh - a.Hq - a.Hkv;
    kv8_store_row(x0, x1, lane, (uint8_t*)a.vcache + ((int64_t)vh * a.ctx_max + pos) * 128, vexp + (int64_t)vh * a.ctx_max + pos);
    if (a.vt) {
      bf16_t* vt = (bf16_t*)a.vt + (int64_t)vh * 128 * a.vt_ld;
      vt[(int64_t)d0 * a.vt_ld + s] = (bf16_t)(raw & 0xffff);
      vt[(int64_t)(d0 + 1) * a.vt_ld + s] = (bf16_t)(raw >> 16);
    }
  }
}

// ---- usdm_kv_expand: rows 0 .. n-1 of ONE layer's cache of ONE sequence -> the bf16 operands of the prefill attention (prefix
// reuse where V^T is per-plan scratch: batch slots, FP8 cache).  Grid (ceil(n / 64), Hkv, FP8 ? 2 : 1), 256 threads; a workgroup
// takes 64 keys x 128 d of one kv head.  z = 0: the V rows (FP8: dequantized exactly, fp8x8_to_bf16x8 with the row's 2^e, as the
// decode kernels do) go through a padded LDS tile and leave as V^T, 8 keys = 16 bytes per store; z = 1 (FP8 only): the K rows,
// dequantized likewise, go to kscr as they are.  Every global access is a 16-byte piece, except the columns of a last group of
// fewer than 8 keys and destinations that are not 16-byte aligned (element / 4-byte stores).  Rows / columns >= n are neither read
// nor written.
constexpr int KVX_KEYS = 64, KVX_LD = 65;     // tile: [64 keys][64 dwords = 128 bf16], rows padded to 65 dwords (conflict-free both ways)
__device__ __forceinline__ void kvx_store16(bf16_t* p, u32x4 v, bool al16) {
  if (al16) { *(u32x4*)p = v; return; }
#pragma unroll
  for (int w = 0; w < 4; ++w) ((unsigned*)p)[w] = v[w];
}
template <bool FP8>
__global__ __launch_bounds__(256) void kv_expand_kernel(const usdm_kv_expand_args a) {
  __shared__ unsigned tile[KVX_KEYS][KVX_LD];
  const int tid = threadIdx.x, kh = blockIdx.y;
  const int r0 = blockIdx.x * KVX_KEYS;
  const int64_t hrow = (int64_t)kh * a.ctx_max;
  if (FP8 && blockIdx.z == 1) {      // K rows: 64 rows x 8 pieces of 16 e4m3 bytes -> 2 x 16 bytes of bf16 each
    const bool al16 = ((uintptr_t)a.kscr & 15) == 0;
    for (int p = tid; p < KVX_KEYS * 8; p += 256) {
      const int r = r0 + (p >> 3), c = p & 7;
      if (r >= a.n) break;
      const u32x4 q = *(const u32x4*)((const uint8_t*)a.kcache + (hrow + r) * 128 + c * 16);
      const float s = fp8_row_scale(a.kexp[hrow + r]);
      bf16_t* dst = (bf16_t*)a.kscr + ((int64_t)kh * a.kscr_ld + r) * 128 + c * 16;
      kvx_store16(dst, fp8x8_to_bf16x8(u32x2{q[0], q[1]}, s), al16);
      kvx_store16(dst + 8, fp8x8_to_bf16x8(u32x2{q[2], q[3]}, s), al16);
    }
    return;
  }
  // V rows -> the tile (bf16 values, two per dword)
  if constexpr (FP8) {
    for (int p = tid; p < KVX_KEYS * 8; p += 256) {
      const int k = p >> 3, c = p & 7;
      if (r0 + k >= a.n) break;
      const u32x4 q = *(const u32x4*)((const uint8_t*)a.vcache + (hrow + r0 + k) * 128 + c * 16);
      const float s = fp8_row_scale(a.vexp[hrow + r0 + k]);
      const u32x4 lo = fp8x8_to_bf16x8(u32x2{q[0], q[1]}, s), hi = fp8x8_to_bf16x8(u32x2{q[2], q[3]}, s);
#pragma unroll
      for (int w = 0; w < 4; ++w) { tile[k][c * 8 + w] = lo[w]; tile[k][c * 8 + 4 + w] = hi[w]; }
    }
  } else {
    for (int p = tid; p < KVX_KEYS * 16; p += 256) {
      const int k = p >> 4, c = p & 15;
      if (r0 + k >= a.n) break;
      const u32x4 v = *(const u32x4*)((const bf16_t*)a.vcache + (hrow + r0 + k) * 128 + c * 8);
#pragma unroll
      for (int w = 0; w < 4; ++w) tile[k][c * 4 + w] = v[w];
    }
  }
  __syncthreads();
  // the tile -> V^T: an item = (pair of d, group of 8 keys) = two 16-byte pieces, one per d
  const bool al16 = ((uintptr_t)a.vt & 15) == 0 && a.vt_ld % 8 == 0;
  bf16_t* vt = (bf16_t*)a.vt + (int64_t)kh * 128 * a.vt_ld;
  for (int p = tid; p < 64 * 8; p += 256) {
    const int kg = p & 7, dp = p >> 3;
    const int kb = r0 + kg * 8;
    if (kb >= a.n) continue;
    const int nkeys = min(8, a.n - kb);
    unsigned w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = j < nkeys ? tile[kg * 8 + j][dp] : 0u;
    bf16_t* d0 = vt + (int64_t)(2 * dp) * a.vt_ld + kb;
    bf16_t* d1 = d0 + a.vt_ld;
    if (nkeys == 8 && al16) {
      u32x4 e, o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[j] = (w[2 * j] & 0xffffu) | (w[2 * j + 1] << 16);
        o[j] = (w[2 * j] >> 16) | (w[2 * j + 1] & 0xffff0000u);
      }
      *(u32x4*)d0 = e;
      *(u32x4*)d1 = o;
    } else {
      for (int j = 0; j < nkeys; ++j) { d0[j] = (bf16_t)(w[j] & 0xffffu); d1[j] = (bf16_t)(w[j] >> 16); }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The rope prologue, the scores of a key and the softmax statistics of a decode-attention step, once, for attn_decode_kernel and
// attn_decode1_kernel: one kv head with its G query heads, d = 128.  What differs between the kernels - which keys a thread takes,
// how many rows it has in flight, where the score rows live - stays in the kernels.  So does the PV step of one key (ten lines in
// each): as a shared function the compiler packed the G = 4 accumulators of attn_decode1_kernel across heads, four more moves per
// key and 0.35 us (2.6 %) per launch (profiles/attn_decode_share.txt).
// ---------------------------------------------------------------------------------------------
// rope of the new q (G heads of kv head kh) and the new k into LDS, by the NTH threads of the workgroup
template <int G, int NTH>
__device__ __forceinline__ void da_rope_qk(const bf16_t* qkv, const bf16_t* cos, const bf16_t* sin, int pos, int Hq, int kh, int tid,
                                           float (*qs)[128], float* knew) {
  for (int i = tid; i < (G + 1) * 64; i += NTH) {
    const int hsel = i >> 6, d = i & 63;
    const float c = bf2f(cos[(int64_t)pos * 64 + d]), sn = bf2f(sin[(int64_t)pos * 64 + d]);
    const bf16_t* src = hsel < G ? qkv + (kh * G + hsel) * 128 : qkv + (Hq + kh) * 128;
    float o1, o2;
    rope_pair(bf2f(src[d]), bf2f(src[d + 64]), c, sn, o1, o2);
    if (hsel < G) { qs[hsel][d] = o1; qs[hsel][d + 64] = o2; }
    else { knew[d] = o1; knew[d + 64] = o2; }
  }
}

// the scores of one key: 8 lanes per key, lane j of them holds d = 16 j .. 16 j + 15 of the K row as bf16 pairs (b0, b1) and of the
// G query rows (qr).  Key `key` == pos is the new token's: its K is not in the cache yet and comes from LDS (knew).  Head h's score
// goes to sc[h * hs + kk] (hs: the stride between the heads' score rows).
template <int G>
__device__ __forceinline__ void da_score_key(u32x4 b0, u32x4 b1, int key, int pos, const float (&qr)[G][16], const float* knew, int j, float scale,
                                             float* sc, int hs, int kk) {
  float kv[16];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    kv[2 * e] = bf2f(b0[e] & 0xffff); kv[2 * e + 1] = bf2f(b0[e] >> 16);
    kv[8 + 2 * e] = bf2f(b1[e] & 0xffff); kv[8 + 2 * e + 1] = bf2f(b1[e] >> 16);
  }
  if (key == pos) {
#pragma unroll
    for (int e = 0; e < 16; ++e) kv[e] = knew[j * 16 + e];
  }
#pragma unroll
  for (int h = 0; h < G; ++h) {
    float sdot = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) sdot = fmaf(qr[h][e], kv[e], sdot);
    sdot += __shfl_xor(sdot, 1, 64); sdot += __shfl_xor(sdot, 2, 64); sdot += __shfl_xor(sdot, 4, 64);
    if (j == 0) sc[h * hs + kk] = sdot * scale;
  }
}

// softmax statistics of one head's n scores, by one wave: the maximum m and l = sum exp(s - m) in fp32 on every lane; the row is
// left holding P rounded to bf16 for the PV product (flash-attention semantics)
__device__ __forceinline__ void da_softmax_row(float* row, int n, int lane, float& m, float& l) {
  m = -1e30f;
  for (int kk = lane; kk < n; kk += 64) m = fmaxf(m, row[kk]);
  m = wave_max(m);
  l = 0.f;
  for (int kk = lane; kk < n; kk += 64) {
    const float p = __expf(row[kk] - m);
    l += p;
    row[kk] = round_bf(p);
  }
  l = wave_sum(l);
}

// ---------------------------------------------------------------------------------------------
// Decode attention, split over the context: grid (Hkv, NS).  Each block ropes the new q (G heads of
// its kv head) and the new k itself, so no block depends on another block's cache write.
// ---------------------------------------------------------------------------------------------
constexpr int DA_KMAX = 512;  // max keys per split
// PIPE (round 4, the many-sequence step: few splits of up to 512 keys each): the K / V rows of the NEXT batch of keys are requested
// before the current batch is consumed (second register set).  The batch-1 step (NS = 32: ~20 keys per split, one batch) keeps
// the plain form.  Same keys per thread in the same order: bit-identical results (profiles/r04_decode_ablation.txt 11).
// FP8 (opt-in, usdm_attn_decode_fp8): the caches hold e4m3 rows with one power-of-two exponent per (key, kv head)
// (usdm_amd/quant.py).  A lane's 16 d of a K row are 16 bytes, a thread's 4 d of a V row 4 bytes; they are converted exactly to the
// bf16 values K' / V' in registers and the bf16 arithmetic runs unchanged on the same keys per lane in the same order, so the
// result equals the bf16 kernel's on the dequantized caches bit for bit.  Sweep depth: USDM_KV8_SWEEPS below.
// The exponents are requested with the rows.  The cache pointers of usdm_attn_decode_args are the byte caches; the exponent
// pointers come as one extra kernel argument (FP8 only: the bf16 instantiations keep their signature and code).
#ifndef USDM_KV8_SWEEPS
#define USDM_KV8_SWEEPS 4   // sweeps in flight of the FP8 instantiations.  4 = the bf16 depth, i.e. half the bytes in flight; 8 (the same
                            // bytes in flight, 200 instead of ~170 VGPRs at G = 4) measured 2-3 % SLOWER per launch (profiles/kv8_batch_rate.txt)
#endif
struct kv8_exps { int8_t* k; int8_t* v; int64_t bs; };
__device__ __forceinline__ kv8_exps kv8_get() { return kv8_exps{nullptr, nullptr, 0}; }
__device__ __forceinline__ kv8_exps kv8_get(kv8_exps e) { return e; }
template <bool FP8> struct kv_fmt { typedef u32x2 vvec; };
template <> struct kv_fmt<true> { typedef unsigned vvec; };

template <int G, bool PIPE = false, bool FP8 = false, class... FMT>
__global__ __launch_bounds__(256) void attn_decode_kernel(const usdm_attn_decode_args a, FMT... fmt) {
  static_assert(FP8 == (sizeof...(FMT) == 1), "FP8 takes the row exponents");
  typedef typename kv_fmt<FP8>::vvec vvec;
  __shared__ float qs[G][128];
  __shared__ float knew[128], vnew[128];
  __shared__ float sc[G][DA_KMAX];
  __shared__ float red[8][G][128];
  __shared__ float lsum[G], lmax[G];
  const int skipv = a.skip ? *a.skip : 0;        // tested after the K/V requests below are issued
  const int kh = blockIdx.x, sp = blockIdx.y, NS = gridDim.y;
  const int bi = blockIdx.z;                      // sequence of a batched decode step (0 when single)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pos = a.pos[bi];
  if (a.cmb_gran) {   // clear the tags of the o_proj hand-off granules (usdm_gemv cmb_gran) for the launch that follows.  BEFORE the
    // position check below: on that (caller-bug) path the o_proj launch must not find the previous token's granules still tagged
    const int gi = ((int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x) * 256 + tid;
    if (bi == 0 && gi < a.Hq * 64) a.cmb_gran[gi] = 0ull;
  }
  if ((unsigned)pos >= (unsigned)a.ctx_max) return;   // never append past the cache / rope table (a caller bug: the host bounds every sequence)
  const int ctx = pos + 1;
  const int lo = (a.window > 0 && ctx > a.window) ? ctx - a.window : 0;   // sliding window: keys lo .. pos
  const int chunk = (ctx - lo + NS - 1) / NS;
  const int k0 = lo + sp * chunk, k1 = min(ctx, k0 + chunk);
  const int nk = max(0, k1 - k0);
  const bf16_t* qkv = (const bf16_t*)a.qkv + (int64_t)bi * a.qkv_bs;
  bf16_t* kcache_b = (bf16_t*)a.kcache + (int64_t)bi * a.cache_bs;
  bf16_t* vcache_b = (bf16_t*)a.vcache + (int64_t)bi * a.cache_bs;
  const bf16_t* Kc = kcache_b + (int64_t)kh * a.ctx_max * 128;
  const bf16_t* Vc = vcache_b + (int64_t)kh * a.ctx_max * 128;
  // FP8: the same rows as bytes, and the exponents of this kv head's keys
  const kv8_exps ex = kv8_get(fmt...);
  uint8_t* k8_b = (uint8_t*)a.kcache + (int64_t)bi * a.cache_bs;
  uint8_t* v8_b = (uint8_t*)a.vcache + (int64_t)bi * a.cache_bs;
  const uint8_t* Kc8 = k8_b + (int64_t)kh * a.ctx_max * 128;
  const uint8_t* Vc8 = v8_b + (int64_t)kh * a.ctx_max * 128;
  int8_t* Ke = ex.k + (int64_t)bi * ex.bs + (int64_t)kh * a.ctx_max;
  int8_t* Ve = ex.v + (int64_t)bi * ex.bs + (int64_t)kh * a.ctx_max;
  float* pm_b = a.pm + (int64_t)bi * a.Hq * NS;
  float* pl_b = a.pl + (int64_t)bi * a.Hq * NS;
  float* po_b = a.po + (int64_t)bi * a.Hq * NS * 128;
  bf16_t* out_b = (bf16_t*)a.out + (int64_t)bi * a.out_bs;
  // ---- everything that depends only on pos is requested NOW: the first batch of K rows (scores layout) and of V rows
  // (PV layout) is in flight while q/k are roped; at ~25 keys per split that is the whole split, so the kernel pays one
  // memory latency instead of three (rope inputs -> K -> V).
  constexpr int SW = FP8 ? USDM_KV8_SWEEPS : 4, PW = FP8 ? USDM_KV8_SWEEPS : 4;
  const int j = lane & 7, gk = (wave << 3) + (lane >> 3);  // scores: 8 lanes per key, key slot within a 32-key sweep
  const int d4 = (tid & 31) * 4, kl = tid >> 5;            // PV: thread = (4 d's, key lane)
  u32x4 r0[SW], r1[FP8 ? 1 : SW];
  vvec rv[PW];
  int ek[FP8 ? SW : 1], ev[FP8 ? PW : 1];                  // FP8: the keys' exponents
  // key kk of this split -> registers: the lane's 16 d of the K row (bf16: two 16-byte loads; FP8: one + the exponent byte) ...
  auto ldk = [&](int kk, u32x4& x0, u32x4& x1, int& e) {
    if constexpr (FP8) {
      x0 = *(const u32x4*)(Kc8 + (int64_t)(k0 + kk) * 128 + j * 16);
      e = Ke[k0 + kk];
    } else {
      const bf16_t* kp = Kc + (int64_t)(k0 + kk) * 128 + j * 16;
      x0 = *(const u32x4*)kp;
      x1 = *(const u32x4*)(kp + 8);
    }
  };
  // ... and the thread's 4 d of the V row (bf16: 8 bytes; FP8: 4 + the exponent byte)
  auto ldv = [&](int kk, vvec& x, int& e) {
    if constexpr (FP8) {
      x = *(const unsigned*)(Vc8 + (int64_t)(k0 + kk) * 128 + d4);
      e = Ve[k0 + kk];
    } else {
      x = *(const u32x2*)(Vc + (int64_t)(k0 + kk) * 128 + d4);
    }
  };
  if (nk > 0) {
#pragma unroll
    for (int w = 0; w < SW; ++w) ldk(min(32 * w + gk, nk - 1), r0[w], r1[FP8 ? 0 : w], ek[FP8 ? w : 0]);
#pragma unroll
    for (int w = 0; w < PW; ++w) ldv(min(8 * w + kl, nk - 1), rv[w], ev[FP8 ? w : 0]);
  }
  if (skipv) return;   // sequence already ended (usdm_decode_state.done): nothing may be appended to the cache
  // ---- rope q (G heads) and the new k; stash v
  da_rope_qk<G, 256>(qkv, a.cos, a.sin, pos, a.Hq, kh, tid, qs, knew);
  if (tid < 128) vnew[tid] = bf2f(qkv[(a.Hq + a.Hkv + kh) * 128 + tid]);
  __syncthreads();
  if constexpr (FP8) {
    // designated writer: wave 0 quantizes the K row, wave 1 the V row (knew / vnew hold bf16 values: the row the bf16 kernel stores)
    if (sp == 0 && tid < 128) {
      const float* src = wave == 0 ? knew : vnew;
      const int64_t r = (int64_t)kh * a.ctx_max + pos;
      kv8_store_row(src[2 * lane], src[2 * lane + 1], lane, (wave == 0 ? k8_b : v8_b) + r * 128, (wave == 0 ? Ke : Ve) + pos);
    }
  } else {
  if (sp == 0 && tid < 128) {  // designated writer of the new cache row
    kcache_b[((int64_t)kh * a.ctx_max + pos) * 128 + tid] = f2bf(knew[tid]);
    vcache_b[((int64_t)kh * a.ctx_max + pos) * 128 + tid] = f2bf(vnew[tid]);
  }
  }
  // ---- scores: 8 lanes per key, 16 d each; the K rows of SW sweeps are requested before any of them is used
  {
    float qr[G][16];
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
      for (int e = 0; e < 16; ++e) qr[h][e] = qs[h][j * 16 + e];
    u32x4 n0[PIPE ? SW : 1], n1[PIPE && !FP8 ? SW : 1];      // PIPE: the next batch's rows
    int nek[PIPE && FP8 ? SW : 1];
    for (int base = 0; base < nk; base += 32 * SW) {
      if constexpr (PIPE) {
        // unconditional (clamped) requests: a branch here would make the wait-count pass drain everything at the join
#pragma unroll
        for (int w = 0; w < SW; ++w) ldk(min(base + 32 * SW + 32 * w + gk, nk - 1), n0[w], n1[FP8 ? 0 : w], nek[FP8 ? w : 0]);
      } else if (base > 0) {
#pragma unroll
        for (int w = 0; w < SW; ++w) ldk(min(base + 32 * w + gk, nk - 1), r0[w], r1[FP8 ? 0 : w], ek[FP8 ? w : 0]);
      }
#pragma unroll
      for (int w = 0; w < SW; ++w) {
        const int kk = base + 32 * w + gk;
        if (kk >= nk) continue;
        u32x4 b0, b1;                              // the 16 d as bf16 pairs
        if constexpr (FP8) {
          const float s = fp8_row_scale(ek[w]);
          b0 = fp8x8_to_bf16x8(u32x2{r0[w][0], r0[w][1]}, s);
          b1 = fp8x8_to_bf16x8(u32x2{r0[w][2], r0[w][3]}, s);
        } else {
          b0 = r0[w]; b1 = r1[w];
        }
        da_score_key<G>(b0, b1, k0 + kk, pos, qr, knew, j, a.scale, &sc[0][0], DA_KMAX, kk);
      }
      if constexpr (PIPE) {
#pragma unroll
        for (int w = 0; w < SW; ++w) {
          r0[w] = n0[w];
          if constexpr (FP8) ek[w] = nek[w];
          else r1[w] = n1[w];
        }
      }
    }
  }
  __syncthreads();
  // ---- softmax statistics per head (wave h <-> head h when G <= 4)
  for (int h = wave; h < G; h += 4) {
    float m, l;
    da_softmax_row(sc[h], nk, lane, m, l);
    if (lane == 0) { lsum[h] = l; lmax[h] = m; }
  }
  __syncthreads();
  // ---- PV: thread = (4 d's, key lane)
  {
    float acc[G][4];
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[h][e] = 0.f;
    vvec nv[PIPE ? PW : 1];
    int nev[PIPE && FP8 ? PW : 1];
    for (int base = 0; base < nk; base += 8 * PW) {
      if constexpr (PIPE) {
#pragma unroll
        for (int w = 0; w < PW; ++w) ldv(min(base + 8 * PW + 8 * w + kl, nk - 1), nv[w], nev[FP8 ? w : 0]);
      } else if (base > 0) {
#pragma unroll
        for (int w = 0; w < PW; ++w) ldv(min(base + 8 * w + kl, nk - 1), rv[w], ev[FP8 ? w : 0]);
      }
#pragma unroll
      for (int w = 0; w < PW; ++w) {
        const int kk = base + 8 * w + kl;
        if (kk >= nk) continue;
        u32x2 bv;                                  // the 4 d as bf16 pairs
        if constexpr (FP8) {
          typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_cvt;
          const float s = fp8_row_scale(ev[w]);
          bv[0] = __builtin_bit_cast(unsigned, (bf16x2_cvt)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(rv[w], s, false));
          bv[1] = __builtin_bit_cast(unsigned, (bf16x2_cvt)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(rv[w], s, true));
        } else {
          bv = rv[w];
        }
        float v[4] = {bf2f(bv[0] & 0xffff), bf2f(bv[0] >> 16), bf2f(bv[1] & 0xffff), bf2f(bv[1] >> 16)};
        if (k0 + kk == pos) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = vnew[d4 + e];
        }
#pragma unroll
        for (int h = 0; h < G; ++h) {
          const float p = sc[h][kk];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[h][e] = fmaf(p, v[e], acc[h][e]);
        }
      }
      if constexpr (PIPE) {
#pragma unroll
        for (int w = 0; w < PW; ++w) {
          rv[w] = nv[w];
          if constexpr (FP8) ev[w] = nev[w];
        }
      }
    }
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[kl][h][d4 + e] = acc[h][e];
  }
  __syncthreads();
  for (int i = tid; i < G * 128; i += 256) {
    const int h = i >> 7, d = i & 127;
    float s = 0.f;
#pragma unroll
    for (int kl2 = 0; kl2 < 8; ++kl2) s += red[kl2][h][d];
    const int hq = kh * G + h;
    // agent-scope (write-through) stores: the merging workgroup may sit on another XCD, whose L2 is not coherent with ours
    __hip_atomic_store(po_b + ((int64_t)hq * NS + sp) * 128 + d, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (d == 0) {
      __hip_atomic_store(pm_b + hq * NS + sp, nk > 0 ? lmax[h] : -1e30f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(pl_b + hq * NS + sp, nk > 0 ? lsum[h] : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (!a.counters) return;   // partials are merged by attn_combine_kernel
  // ---- fused merge: the workgroup that finishes this kv head last combines the NS partials of its G heads.
  // No agent-scope fences (an L2 write-back / invalidate per workgroup cost ~30 us per launch): the partials travel
  // as write-through stores and are read back with agent-scope loads; ordering = every thread waits for its own
  // stores to be acknowledged, workgroup barrier, then one relaxed increment of the kv head's counter.
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(a.counters + bi * a.Hkv + kh, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (old == NS - 1);
    if (old == NS - 1) __hip_atomic_store(a.counters + bi * a.Hkv + kh, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
  }
  __syncthreads();
  if (!s_last) return;
  {
    auto ald = [](const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    float* wgt = &sc[0][0];                       // [G][64] merge weights (sc is free now; DA_KMAX >= 64)
    for (int h = wave; h < G; h += 4) {           // wave per head: NS <= 64 lanes
      const int hq = kh * G + h;
      const float linv = attn_merge_weights(NS, lane, wgt + h * 64, [&](int s) { return ald(pm_b + hq * NS + s); },
                                            [&](int s) { return ald(pl_b + hq * NS + s); });
      if (lane == 0) lsum[h] = linv;
    }
    __syncthreads();
    for (int i = tid; i < G * 128; i += 256) {
      const int h = i >> 7, d = i & 127;
      const int hq = kh * G + h;
      const float* p = po_b + (int64_t)hq * NS * 128 + d;
      const float o = attn_merge_sum<16>(NS, wgt + h * 64, [&](int s) { return ald(p + s * 128); });   // 16 partials in flight per output
      out_b[hq * 128 + d] = f2bf(o * lsum[h]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Decode attention, one 16-wave workgroup per kv head (no context split, no partials, no combine launch):
// at batch 1 the phase is latency-bound, not bandwidth-bound (<= ~0.8 MB of K/V per kv head), so the fastest form is
// the one with the fewest dependent steps: rope q/k -> scores (16 waves x 8 keys per sweep) -> softmax (wave per head)
// -> PV (32 key lanes x 32 d-quads) -> in-LDS reduction -> bf16 output.  Rope, scores and softmax are the split kernel's (da_*).
// ---------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(1024) void attn_decode1_kernel(const usdm_attn_decode_args a) {
  if (a.skip && *a.skip) return;
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  float* sc = (float*)dsm;                          // [G][ctx_pad]
  const int pos = *a.pos;
  if ((unsigned)pos >= (unsigned)a.ctx_max) return;
  const int ctx = pos + 1;
  const int ctx_pad = (a.ctx_max + 3) & ~3;
  float* red = sc + G * ctx_pad;                    // [16][G][128]
  __shared__ float qs[G][128];
  __shared__ float knew[128], vnew[128];
  __shared__ float lsum[G], lmax[G];
  const int kh = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_t* qkv = (const bf16_t*)a.qkv;
  da_rope_qk<G, 1024>(qkv, a.cos, a.sin, pos, a.Hq, kh, tid, qs, knew);
  if (tid >= 512 && tid < 640) vnew[tid - 512] = bf2f(qkv[(a.Hq + a.Hkv + kh) * 128 + tid - 512]);
  __syncthreads();
  const bf16_t* Kc = (const bf16_t*)a.kcache + (int64_t)kh * a.ctx_max * 128;
  const bf16_t* Vc = (const bf16_t*)a.vcache + (int64_t)kh * a.ctx_max * 128;
  if (tid < 128) {
    ((bf16_t*)a.kcache)[((int64_t)kh * a.ctx_max + pos) * 128 + tid] = f2bf(knew[tid]);
    ((bf16_t*)a.vcache)[((int64_t)kh * a.ctx_max + pos) * 128 + tid] = f2bf(vnew[tid]);
  }
  // ---- scores
  {
    constexpr int SW = 2;
    const int j = lane & 7, gk = (wave << 3) + (lane >> 3);   // 128 keys per block sweep
    float qr[G][16];
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
      for (int e = 0; e < 16; ++e) qr[h][e] = qs[h][j * 16 + e];
    for (int base = 0; base < ctx; base += 128 * SW) {
      u32x4 r0[SW], r1[SW];
#pragma unroll
      for (int w = 0; w < SW; ++w) {
        const int kk = min(base + 128 * w + gk, ctx - 1);
        const bf16_t* kp = Kc + (int64_t)kk * 128 + j * 16;
        r0[w] = *(const u32x4*)kp;
        r1[w] = *(const u32x4*)(kp + 8);
      }
#pragma unroll
      for (int w = 0; w < SW; ++w) {
        const int kk = base + 128 * w + gk;
        if (kk >= ctx) continue;
        da_score_key<G>(r0[w], r1[w], kk, pos, qr, knew, j, a.scale, sc, ctx_pad, kk);
      }
    }
  }
  __syncthreads();
  // ---- softmax statistics: wave h <-> head h
  if (wave < G) {
    const int h = wave;
    float m, l;
    da_softmax_row(sc + h * ctx_pad, ctx, lane, m, l);
    if (lane == 0) { lsum[h] = l; lmax[h] = m; }
  }
  __syncthreads();
  // ---- PV: 32 key lanes x 32 d-quads; lanes l and l^32 of a wave share the d-quad
  {
    constexpr int PW = 4;
    const int d4 = (tid & 31) * 4, kl = tid >> 5;   // kl in [0, 32)
    float acc[G][4];
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[h][e] = 0.f;
    for (int base = 0; base < ctx; base += 32 * PW) {
      u32x2 rv[PW];
#pragma unroll
      for (int w = 0; w < PW; ++w) {
        const int kk = min(base + 32 * w + kl, ctx - 1);
        rv[w] = *(const u32x2*)(Vc + (int64_t)kk * 128 + d4);
      }
#pragma unroll
      for (int w = 0; w < PW; ++w) {
        const int kk = base + 32 * w + kl;
        if (kk >= ctx) continue;
        float v[4] = {bf2f(rv[w][0] & 0xffff), bf2f(rv[w][0] >> 16), bf2f(rv[w][1] & 0xffff), bf2f(rv[w][1] >> 16)};
        if (kk == pos) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = vnew[d4 + e];
        }
#pragma unroll
        for (int h = 0; h < G; ++h) {
          const float p = sc[h * ctx_pad + kk];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[h][e] = fmaf(p, v[e], acc[h][e]);
        }
      }
    }
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[h][e];
        v += __shfl_xor(v, 32, 64);
        if (lane < 32) red[(wave * G + h) * 128 + d4 + e] = v;
      }
  }
  __syncthreads();
  for (int i = tid; i < G * 128; i += 1024) {
    const int h = i >> 7, d = i & 127;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) s += red[(w * G + h) * 128 + d];
    ((bf16_t*)a.out)[(kh * G + h) * 128 + d] = f2bf(s / lsum[h]);
  }
}

// the merge of the split partials as a launch of its own (no counters, no defer_merge): one workgroup per query head
__global__ __launch_bounds__(128) void attn_combine_kernel(const float* pm, const float* pl, const float* po, int NS, bf16_t* out,
                                                           int64_t out_bs, const int* skip) {
  if (skip && *skip) return;
  __shared__ float w[64];
  __shared__ float linv;
  const int hq = blockIdx.x, d = threadIdx.x;  // 128 threads
  const int bi = blockIdx.y, Hq = gridDim.x;   // sequence of a batched step
  pm += (int64_t)bi * Hq * NS; pl += (int64_t)bi * Hq * NS; po += (int64_t)bi * Hq * NS * 128; out += (int64_t)bi * out_bs;
  if (d < 64) {
    const float inv = attn_merge_weights(NS, d, w, [&](int s) { return pm[hq * NS + s]; }, [&](int s) { return pl[hq * NS + s]; });
    if (d == 0) linv = inv;
  }
  __syncthreads();
  const float* p = po + (int64_t)hq * NS * 128 + d;
  const float o = attn_merge_sum<4>(NS, w, [&](int s) { return p[s * 128]; });
  out[hq * 128 + d] = f2bf(o * linv);
}

// calls f(da_ic<G>) for a supported group size G = Hq / Hkv and returns 0; any other G is the caller's error
template <int I> struct da_ic { static constexpr int value = I; };
template <class F>
static int da_dispatch_g(const char* who, int G, F&& f) {
  if (G == 4) f(da_ic<4>{});
  else if (G == 2) f(da_ic<2>{});
  else if (G == 1) f(da_ic<1>{});
  else USDM_CHECK_ARG(false, "%s: group size %d unsupported (1,2,4)", who, G);
  return 0;
}
}  // namespace

extern "C" int usdm_rope_cache(const usdm_rope_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->qkv && pa->cos && pa->sin && pa->kcache && pa->vcache, "usdm_rope_cache: null args");
  const usdm_rope_args& a = *pa;
  USDM_CHECK_ARG(a.S > 0 && a.pos0 >= 0 && a.pos0 + a.S <= a.ctx_max && a.pos0 + a.S <= a.max_pos, "usdm_rope_cache: positions exceed the cache / rope table");
  USDM_CHECK_ARG(!a.vt || a.vt_ld >= a.S, "usdm_rope_cache: vt_ld");
  hipLaunchKernelGGL(rope_cache_kernel, dim3(a.S, a.Hq + 2 * a.Hkv), dim3(64), 0, (hipStream_t)stream, a);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_rope_cache_fp8(const usdm_rope_fp8_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->r.qkv && pa->r.cos && pa->r.sin && pa->r.kcache && pa->r.vcache && pa->kexp && pa->vexp, "usdm_rope_cache_fp8: null args");
  const usdm_rope_args& a = pa->r;
  USDM_CHECK_ARG(a.S > 0 && a.pos0 >= 0 && a.pos0 + a.S <= a.ctx_max && a.pos0 + a.S <= a.max_pos, "usdm_rope_cache_fp8: positions exceed the cache / rope table");
  USDM_CHECK_ARG(a.Hq >= 0 && a.Hkv > 0 && a.ld >= (int64_t)(a.Hq + 2 * a.Hkv) * 128 && a.ld % 2 == 0 && ((uintptr_t)a.qkv & 3) == 0, "usdm_rope_cache_fp8: qkv 4-byte aligned, ld even and >= (Hq + 2 Hkv) * 128");
  USDM_CHECK_ARG(!a.vt || a.vt_ld >= a.S, "usdm_rope_cache_fp8: vt_ld");
  USDM_CHECK_ARG(!pa->kscr || (pa->kscr_ld >= a.S && ((uintptr_t)pa->kscr & 3) == 0), "usdm_rope_cache_fp8: kscr_ld >= S, kscr 4-byte aligned");
  USDM_CHECK_ARG(((uintptr_t)a.kcache & 15) == 0 && ((uintptr_t)a.vcache & 15) == 0, "usdm_rope_cache_fp8: the fp8 caches must be 16-byte aligned");
  USDM_CHECK_ARG(((uintptr_t)pa->kexp & 3) == 0 && ((uintptr_t)pa->vexp & 3) == 0, "usdm_rope_cache_fp8: the exponent arrays must be 4-byte aligned");
  hipLaunchKernelGGL(rope_cache_fp8_kernel, dim3(a.S, a.Hq + 2 * a.Hkv), dim3(64), 0, (hipStream_t)stream, a, pa->kexp, pa->vexp, (bf16_t*)pa->kscr, pa->kscr_ld);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_kv_expand(const usdm_kv_expand_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->kcache && pa->vcache && pa->vt, "usdm_kv_expand: null args");
  const usdm_kv_expand_args& a = *pa;
  const bool fp8 = a.kexp || a.vexp;
  USDM_CHECK_ARG(a.Hkv > 0 && a.ctx_max > 0 && a.n >= 1 && a.n <= a.ctx_max, "usdm_kv_expand: Hkv, ctx_max > 0 and 1 <= n <= ctx_max");
  USDM_CHECK_ARG(((uintptr_t)a.vcache & 15) == 0 && ((uintptr_t)a.kcache & 15) == 0, "usdm_kv_expand: the caches must be 16-byte aligned");
  USDM_CHECK_ARG(a.vt_ld >= a.n && ((uintptr_t)a.vt & 3) == 0, "usdm_kv_expand: vt_ld >= n, vt 4-byte aligned");
  if (fp8) {
    USDM_CHECK_ARG(a.kexp && a.vexp && a.kscr, "usdm_kv_expand: an fp8 cache comes with both exponent arrays and kscr");
    USDM_CHECK_ARG(((uintptr_t)a.kexp & 3) == 0 && ((uintptr_t)a.vexp & 3) == 0, "usdm_kv_expand: the exponent arrays must be 4-byte aligned");
    USDM_CHECK_ARG(a.kscr_ld >= a.n && ((uintptr_t)a.kscr & 3) == 0, "usdm_kv_expand: kscr_ld >= n, kscr 4-byte aligned");
  } else {
    USDM_CHECK_ARG(!a.kscr, "usdm_kv_expand: kscr belongs to the fp8 cache (the attention reads a bf16 cache's K rows in place)");
  }
  const dim3 grid((a.n + KVX_KEYS - 1) / KVX_KEYS, a.Hkv, fp8 ? 2 : 1);
  if (fp8) hipLaunchKernelGGL(kv_expand_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(kv_expand_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_kv_expand_args(void) { return (int)sizeof(usdm_kv_expand_args); }
extern "C" int usdm_sizeof_rope_args(void) { return (int)sizeof(usdm_rope_args); }
extern "C" int usdm_sizeof_rope_fp8_args(void) { return (int)sizeof(usdm_rope_fp8_args); }
extern "C" int usdm_sizeof_attn_decode_args(void) { return (int)sizeof(usdm_attn_decode_args); }
extern "C" int usdm_sizeof_attn_decode_fp8_args(void) { return (int)sizeof(usdm_attn_decode_fp8_args); }

// the split form (NS > 1), one selection for both cache formats: an FP8 launch partitions the keys exactly as the bf16 launch
template <bool FP8, class... FMT>
static int attn_decode_launch_split(const char* who, const usdm_attn_decode_args& a, int span, hipStream_t st, FMT... fmt) {
  const int G = a.Hq / a.Hkv;
  const int nbatch = a.batch > 1 ? a.batch : 1;
  dim3 grid(a.Hkv, a.NS, nbatch);
  const bool pipe = nbatch > 1 && cdiv(span, a.NS) > 64;      // long splits (the many-sequence step): next batch of keys prefetched
  if (int rc = da_dispatch_g(who, G, [&](auto GC) {
        constexpr int g = decltype(GC)::value;
        if (pipe) hipLaunchKernelGGL((attn_decode_kernel<g, true, FP8, FMT...>), grid, dim3(256), 0, st, a, fmt...);
        else hipLaunchKernelGGL((attn_decode_kernel<g, false, FP8, FMT...>), grid, dim3(256), 0, st, a, fmt...);
      }))
    return rc;
  USDM_LAUNCH_CHECK();
  if (!a.counters && !a.defer_merge) {
    hipLaunchKernelGGL(attn_combine_kernel, dim3(a.Hq, nbatch), dim3(128), 0, st, a.pm, a.pl, a.po, a.NS, (bf16_t*)a.out, a.out_bs, a.skip);
    USDM_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int usdm_attn_decode_fp8(const usdm_attn_decode_fp8_args* pf, usdm_stream_t stream) {
  USDM_CHECK_ARG(pf && pf->a.qkv && pf->a.pos && pf->a.kcache && pf->a.vcache && pf->kexp && pf->vexp && (pf->a.out || pf->a.defer_merge),
                 "usdm_attn_decode_fp8: null args");
  const usdm_attn_decode_args& a = pf->a;
  USDM_CHECK_ARG(a.NS != 1, "usdm_attn_decode_fp8: the one-workgroup form (NS == 1) is not built for an fp8 cache (use NS > 1)");
  USDM_CHECK_ARG(!a.defer_merge || (a.NS > 1 && !a.counters && a.batch <= 1), "usdm_attn_decode_fp8: defer_merge needs NS > 1, no counters, one sequence");
  USDM_CHECK_ARG(a.pm && a.pl && a.po, "usdm_attn_decode_fp8: partial buffers missing");
  USDM_CHECK_ARG(a.Hkv > 0 && a.Hq % a.Hkv == 0 && a.NS > 1 && a.NS <= 64, "usdm_attn_decode_fp8: heads / NS (2..64)");
  USDM_CHECK_ARG(a.batch <= 1 || (a.batch <= 64 && a.qkv_bs > 0 && a.out_bs > 0 && a.cache_bs > 0 && pf->exp_bs > 0),
                 "usdm_attn_decode_fp8: batched form needs the four strides");
  USDM_CHECK_ARG(a.window >= 0, "usdm_attn_decode_fp8: window >= 0");
  USDM_CHECK_ARG(a.ctx_max > 0 && ((uintptr_t)a.kcache & 15) == 0 && ((uintptr_t)a.vcache & 15) == 0 && (a.batch <= 1 || a.cache_bs % 16 == 0),
                 "usdm_attn_decode_fp8: the fp8 caches (and cache_bs) must be 16-byte aligned");
  USDM_CHECK_ARG(((uintptr_t)pf->kexp & 3) == 0 && ((uintptr_t)pf->vexp & 3) == 0 && (a.batch <= 1 || pf->exp_bs % 4 == 0),
                 "usdm_attn_decode_fp8: the exponent arrays (and exp_bs) must be 4-byte aligned");
  const int span = (a.window > 0 && a.window < a.ctx_max) ? a.window : a.ctx_max;      // most keys a step can see
  USDM_CHECK_ARG(cdiv(span, a.NS) <= DA_KMAX, "usdm_attn_decode_fp8: visible keys / NS exceeds %d keys per split", DA_KMAX);
  return attn_decode_launch_split<true>("usdm_attn_decode_fp8", a, span, (hipStream_t)stream, kv8_exps{pf->kexp, pf->vexp, a.batch > 1 ? pf->exp_bs : 0});
}

extern "C" int usdm_attn_decode(const usdm_attn_decode_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->qkv && pa->pos && pa->kcache && pa->vcache && (pa->out || pa->defer_merge), "usdm_attn_decode: null args");
  USDM_CHECK_ARG(!pa->defer_merge || (pa->NS > 1 && !pa->counters && pa->batch <= 1), "usdm_attn_decode: defer_merge needs NS > 1, no counters, one sequence");
  USDM_CHECK_ARG(pa->NS == 1 || (pa->pm && pa->pl && pa->po), "usdm_attn_decode: partial buffers missing");
  const usdm_attn_decode_args& a = *pa;
  USDM_CHECK_ARG(a.Hkv > 0 && a.Hq % a.Hkv == 0 && a.NS > 0 && a.NS <= 64, "usdm_attn_decode: heads / NS (<= 64)");
  USDM_CHECK_ARG(a.batch <= 1 || (a.NS > 1 && a.batch <= 64 && a.qkv_bs > 0 && a.out_bs > 0 && a.cache_bs > 0),
                 "usdm_attn_decode: batched form needs NS > 1 and the three strides");
  USDM_CHECK_ARG(a.window >= 0 && (a.window == 0 || a.NS > 1), "usdm_attn_decode: window >= 0, and only with the split form (NS > 1)");
  const int span = (a.window > 0 && a.window < a.ctx_max) ? a.window : a.ctx_max;      // most keys a step can see
  USDM_CHECK_ARG(a.NS == 1 || cdiv(span, a.NS) <= DA_KMAX, "usdm_attn_decode: visible keys / NS exceeds %d keys per split", DA_KMAX);
  const int G = a.Hq / a.Hkv;
  hipStream_t st = (hipStream_t)stream;
  if (a.NS == 1) {   // single-workgroup-per-kv-head form: no partials, no combine
    const int ctx_pad = (a.ctx_max + 3) & ~3;
    const size_t lds = (size_t)(G * ctx_pad + 16 * G * 128) * sizeof(float);
    USDM_CHECK_ARG(lds <= 120 * 1024, "usdm_attn_decode: ctx_max too large for the one-workgroup form (use NS > 1)");
    static bool attr_set = false;
    if (!attr_set) {   // allow > 64 KiB of dynamic LDS (gfx950 has 160 KiB per workgroup)
      for (int g : {4, 2, 1})
        da_dispatch_g("", g, [](auto GC) {
          (void)hipFuncSetAttribute((const void*)attn_decode1_kernel<decltype(GC)::value>, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
        });
      attr_set = true;
    }
    if (int rc = da_dispatch_g("usdm_attn_decode", G, [&](auto GC) {
          hipLaunchKernelGGL(attn_decode1_kernel<decltype(GC)::value>, dim3(a.Hkv), dim3(1024), lds, st, a);
        }))
      return rc;
    USDM_LAUNCH_CHECK();
    return 0;
  }
  return attn_decode_launch_split<false>("usdm_attn_decode", a, span, st);
}

// ---------------------------------------------------------------------------------------------
// usdm_attn_verify: decode attention for T = 1 .. 8 new tokens of ONE sequence (speculative decoding).  Grid
// (Hkv, ceil(ctx_max / C)): workgroup (kh, sp) takes the FIXED key range [sp * C, (sp + 1) * C) for all T * G query rows of kv head
// kh (M = 16 or 32 rows, zero-padded), in key tiles of 64 aligned to absolute indices:
//   rope (rope_pair, as da_rope_qk) of the T x G q rows and the T k rows into LDS as bf16; sp == 0 appends the T K / V rows;
//   scores  S = Q K^T on v_mfma_f32_16x16x32_bf16, a wave per 16 keys of a tile, 4 steps over d, times scale, into LDS;
//   softmax per row over the keys it sees (lo_i .. pos + i) in fp32, P rounded to bf16, masked keys P = 0 exactly;
//   PV      O = P V on the same instruction, the V tile transposed through LDS, a wave per 32 d, tiles in ascending order;
//   partials (m, l, o) per (row, head, split); attn_verify_merge_kernel merges row p's splits 0 .. p / C (attn_merge.h).
// The step's own K / V rows (keys pos .. pos + T - 1) are taken from LDS, never from the cache another workgroup is writing.
// Nothing here depends on T, the row index or *pos except through the set of visible keys: a masked key adds +0 to a sum and
// -1e30 to a maximum, a skipped tile is a tile of such keys.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr int AV_KT = 64;        // key tile
constexpr int AV_CMAX = 256;     // most keys per split
constexpr int AV_TMAX = 8;
constexpr int AV_SLD = AV_CMAX + 4;   // score row stride (floats)
constexpr int AV_PLD = AV_CMAX + 8;   // P row stride (bf16; rows stay 16-byte aligned)
constexpr int AV_VLD = 128 + 8;       // V tile / q row stride (bf16)

__device__ __forceinline__ int av_lo(int p, int window) { return (window > 0 && p + 1 > window) ? p + 1 - window : 0; }

template <int G, int MB>
__global__ __launch_bounds__(256) void attn_verify_kernel(const usdm_attn_verify_args a) {
#include "attn_verify_body.h"
}

// slot b's view of a batched launch: the arrays of ba.v moved on by b slots (NSP splits per row and head in the partials)
__device__ __forceinline__ usdm_attn_verify_args attn_verify_slot(const usdm_attn_verify_batch_args& ba, int b, int NSP) {
  usdm_attn_verify_args a = ba.v;
  const int64_t r0 = (int64_t)b * a.T, p0 = r0 * a.Hq * NSP;
  a.qkv = (const bf16_t*)a.qkv + r0 * a.qkv_ld;
  a.out = (bf16_t*)a.out + r0 * a.out_ld;
  a.pos += b;
  if (a.skip) a.skip += b;
  a.kcache = (bf16_t*)a.kcache + b * ba.cache_bs;
  a.vcache = (bf16_t*)a.vcache + b * ba.cache_bs;
  a.pm += p0;
  a.pl += p0;
  a.po += p0 * 128;
  return a;
}

// usdm_attn_verify_batch: grid (Hkv, NSP, B), workgroup (kh, sp, b) is usdm_attn_verify's workgroup (kh, sp) on slot b
template <int G, int MB>
__global__ __launch_bounds__(256) void attn_verify_batch_kernel(const usdm_attn_verify_batch_args ba) {
  const usdm_attn_verify_args a = attn_verify_slot(ba, blockIdx.z, gridDim.y);
#include "attn_verify_body.h"
}

// the merge of row i's partials over splits 0 .. p / C, p = *pos + i, in split order: attn_combine_kernel's arithmetic
__device__ __forceinline__ void attn_verify_merge_body(const usdm_attn_verify_args& a, int NSP) {
  if (a.skip && *a.skip) return;
  __shared__ float w[64];
  __shared__ float linv;
  const int hq = blockIdx.x, i = blockIdx.y, d = threadIdx.x;
  const int pos = *a.pos;
  if ((unsigned)pos >= (unsigned)a.ctx_max || pos + i >= a.ctx_max) return;
  const int ns = (pos + i) / a.C + 1;
  const float* pm = a.pm + ((int64_t)i * a.Hq + hq) * NSP;
  const float* pl = a.pl + ((int64_t)i * a.Hq + hq) * NSP;
  const float* po = a.po + ((int64_t)i * a.Hq + hq) * NSP * 128 + d;
  if (d < 64) {
    const float inv = attn_merge_weights(ns, d, w, [&](int s) { return pm[s]; }, [&](int s) { return pl[s]; });
    if (d == 0) linv = inv;
  }
  __syncthreads();
  const float o = attn_merge_sum<4>(ns, w, [&](int s) { return po[s * 128]; });
  ((bf16_t*)a.out)[(int64_t)i * a.out_ld + hq * 128 + d] = f2bf(o * linv);
}

__global__ __launch_bounds__(128) void attn_verify_merge_kernel(const usdm_attn_verify_args a, int NSP) { attn_verify_merge_body(a, NSP); }

// grid (Hq, T, B)
__global__ __launch_bounds__(128) void attn_verify_merge_batch_kernel(const usdm_attn_verify_batch_args ba, int NSP) {
  const usdm_attn_verify_args a = attn_verify_slot(ba, blockIdx.z, NSP);
  attn_verify_merge_body(a, NSP);
}

// what both launchers refuse; name: the entry point, for the message
int attn_verify_check(const char* name, const usdm_attn_verify_args* pa) {
  USDM_CHECK_ARG(pa && pa->qkv && pa->pos && pa->cos && pa->sin && pa->kcache && pa->vcache && pa->pm && pa->pl && pa->po && pa->out,
                 "%s: null args", name);
  const usdm_attn_verify_args& a = *pa;
  USDM_CHECK_ARG(a.T >= 1 && a.T <= AV_TMAX, "%s: T = %d outside 1 .. %d", name, a.T, AV_TMAX);
  USDM_CHECK_ARG(a.Hkv > 0 && a.Hq > 0 && a.Hq % a.Hkv == 0 && a.ctx_max > 0 && a.window >= 0, "%s: heads, ctx_max > 0, window >= 0", name);
  USDM_CHECK_ARG(a.C >= AV_KT && a.C <= AV_CMAX && a.C % AV_KT == 0, "%s: C = %d must be a multiple of the key tile %d in %d .. %d", name,
                 a.C, AV_KT, AV_KT, AV_CMAX);
  const int NSP = cdiv(a.ctx_max, a.C);
  USDM_CHECK_ARG(NSP <= 64, "%s: ctx_max / C = %d splits exceed 64", name, NSP);
  USDM_CHECK_ARG(((uintptr_t)a.kcache & 15) == 0 && ((uintptr_t)a.vcache & 15) == 0, "%s: the caches must be 16-byte aligned", name);
  USDM_CHECK_ARG(((uintptr_t)a.qkv & 3) == 0 && ((uintptr_t)a.out & 3) == 0 && ((uintptr_t)a.pos & 3) == 0 && ((uintptr_t)a.pm & 3) == 0 &&
                 ((uintptr_t)a.pl & 3) == 0 && ((uintptr_t)a.po & 3) == 0 && (!a.skip || ((uintptr_t)a.skip & 3) == 0),
                 "%s: qkv, out, pos, skip and the partials must be 4-byte aligned", name);
  USDM_CHECK_ARG(a.qkv_ld >= (int64_t)(a.Hq + 2 * a.Hkv) * 128 && a.qkv_ld % 2 == 0 && a.out_ld >= (int64_t)a.Hq * 128,
                 "%s: qkv_ld even and >= (Hq + 2 Hkv) * 128, out_ld >= Hq * 128", name);
  return 0;
}
}  // namespace

extern "C" int usdm_sizeof_attn_verify_args(void) { return (int)sizeof(usdm_attn_verify_args); }
extern "C" int usdm_attn_verify(const usdm_attn_verify_args* pa, usdm_stream_t stream) {
  if (int rc = attn_verify_check("usdm_attn_verify", pa)) return rc;
  const usdm_attn_verify_args& a = *pa;
  const int NSP = cdiv(a.ctx_max, a.C);
  const int G = a.Hq / a.Hkv;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a.Hkv, NSP);
  if (int rc = da_dispatch_g("usdm_attn_verify", G, [&](auto GC) {
        constexpr int g = decltype(GC)::value;
        if (a.T * g <= 16) hipLaunchKernelGGL((attn_verify_kernel<g, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((attn_verify_kernel<g, 2>), grid, dim3(256), 0, st, a);
      }))
    return rc;
  USDM_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_verify_merge_kernel, dim3(a.Hq, a.T), dim3(128), 0, st, a, NSP);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_sizeof_attn_verify_batch_args(void) { return (int)sizeof(usdm_attn_verify_batch_args); }
extern "C" int usdm_attn_verify_batch(const usdm_attn_verify_batch_args* pb, usdm_stream_t stream) {
  USDM_CHECK_ARG(pb, "usdm_attn_verify_batch: null args");
  if (int rc = attn_verify_check("usdm_attn_verify_batch", &pb->v)) return rc;
  const usdm_attn_verify_args& a = pb->v;
  USDM_CHECK_ARG(pb->B >= 1 && pb->B * a.T <= 16, "usdm_attn_verify_batch: B = %d slots of T = %d rows: B >= 1 and B * T <= 16", pb->B, a.T);
  USDM_CHECK_ARG(pb->cache_bs >=(int64_t)a.Hkv * a.ctx_max * 128,
                 "usdm_attn_verify_batch: cache_bs = %lld is smaller than one slot's cache of Hkv * ctx_max * 128 = %lld elements",
                 (long long)pb->cache_bs, (long long)a.Hkv * a.ctx_max * 128);
  USDM_CHECK_ARG(pb->cache_bs % 8 == 0, "usdm_attn_verify_batch: cache_bs must keep every slot's cache 16-byte aligned");
  const int NSP = cdiv(a.ctx_max, a.C);
  const int G = a.Hq / a.Hkv;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a.Hkv, NSP, pb->B);
  if (int rc = da_dispatch_g("usdm_attn_verify_batch", G, [&](auto GC) {
        constexpr int g = decltype(GC)::value;
        if (a.T * g <= 16) hipLaunchKernelGGL((attn_verify_batch_kernel<g, 1>), grid, dim3(256), 0, st, *pb);
        else hipLaunchKernelGGL((attn_verify_batch_kernel<g, 2>), grid, dim3(256), 0, st, *pb);
      }))
    return rc;
  USDM_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_verify_merge_batch_kernel, dim3(a.Hq, a.T, pb->B), dim3(128), 0, st, *pb, NSP);
  USDM_LAUNCH_CHECK();
  return 0;
}
