// What the weight-streaming decode GEMVs share: gemv_kernel, gemv_resident_kernel, gemv_stream_kernel (llm_k.hip),
// gemv_batch_kernel (llm_batch_k.hip), gemv_mfma_kernel (llm_mfma_k.hip: the row exponents only) and the experimental chain and
// engine kernels (llm_chain_k.hip, llm_engine_k.hip).
//   * the weight-format trait (bf16 / FP8 / MXFP4): load width, the MXFP4 argument, the ring depth;
//   * the per-item arithmetic they must share bit for bit, one text each:
//       dot8               every VALU kernel
//       gemv_sumsq8        gemv_kernel, gemv_resident_kernel, chain, engine (gemv_batch_kernel keeps the text, see there;
//                          gemv_mfma_kernel's statistic is another expression on purpose)
//       gemv_rmsnorm8      gemv_kernel, gemv_resident_kernel, gemv_batch_kernel, chain, engine (gemv_mfma_kernel keeps the text)
//       gemv_glu_row       gemv_kernel, gemv_resident_kernel, gemv_resident_wpack_kernel, gemv_batch_kernel, chain
//       gemv_swiglu_value  gemv_kernel, gemv_resident_kernel, gemv_resident_wpack_kernel, gemv_batch_kernel, chain, engine
//       gemv_plain_value   gemv_kernel, gemv_stream_kernel, gemv_stream_wpack_kernel, chain, engine (gemv_batch_kernel keeps the text)
//       gemv_wpack8        gemv_stream_wpack_kernel, gemv_resident_wpack_kernel (the rebuild of eight bf16 weights from the
//                          13-bit image)
// The structural pieces of the bf16 batch-1 kernels (hand-counted loads, the RMSNorm reduction): gemv_pieces.h.
// The launch selection and the argument checks of the launchers: gemv_launch.h.
// A new weight format plugs in here: DESIGN.md section 8f.
#pragma once
#include "common.h"
#include "../../include/usdm_hip.h"

#ifndef USDM_UNR1
#define USDM_UNR1 8   // ring depth of the one-row-per-wave variants (o_proj / down_proj)
#endif

namespace {
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// 8 bf16 weights x 8 bf16 inputs onto an f32 accumulator, element pairs in order
__device__ __forceinline__ float dot8(u32x4 w, u32x4 x, float acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned a = w[i], b = x[i];
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), acc, false);
  }
  return acc;
}

// ---- the weight-format trait.  The format is chosen by the FP8 flag and the type of the kernel's extra argument: none (bf16),
// the row exponents (FP8: const int8_t*) or gemv_mx4 (MXFP4), so the bf16 instantiations keep their exact signature.
template <bool FP8> struct gemv_fmt { typedef u32x4 wvec; };           // one load of a lane: 16 bytes (bf16: 8 weights; MXFP4: 32 codes)
template <> struct gemv_fmt<true> { typedef u32x2 wvec; };             // FP8: 8 bytes = the same 8 weights
struct gemv_mx4 { const uint8_t* scales; int64_t lds; };   // scale bytes [N][lds], lds = (row stride of the codes in bytes) / 16
template <class... FMT> struct gemv_is_mx4 { static constexpr bool value = false; };
template <> struct gemv_is_mx4<gemv_mx4> { static constexpr bool value = true; };
template <int I> struct gemv_ic { static constexpr int value = I; };
__device__ __forceinline__ const int8_t* gemv_row_exp() { return nullptr; }
__device__ __forceinline__ const int8_t* gemv_row_exp(const int8_t* e) { return e; }
__device__ __forceinline__ gemv_mx4 gemv_mx4_fmt() { return gemv_mx4{nullptr, 0}; }
__device__ __forceinline__ gemv_mx4 gemv_mx4_fmt(const int8_t*) { return gemv_mx4{nullptr, 0}; }
__device__ __forceinline__ gemv_mx4 gemv_mx4_fmt(gemv_mx4 m) { return m; }
// Ring depth of a wave that streams NR rows together: NR * depth = 15..16 16-byte loads in flight per lane.  FP8: 8-byte loads,
// twice as many for the same bytes in flight.  MXFP4: a slot is one group = 4 K iterations with its scale dword, 6..8 in flight
// (K = 4096 is two groups, so more slots would only add re-reads of the row start).
constexpr int gemv_ring_depth(int NR, bool FP8, bool MX4) {
  const int bf16_depth = NR >= 8 ? 2 : NR >= 4 ? 4 : NR == 3 ? 5 : NR == 2 ? 8 : USDM_UNR1;
  return MX4 ? (NR >= 3 ? 2 : 4) : FP8 ? 2 * bf16_depth : bf16_depth;
}

// ---- the lossless 13-bit image of a bf16 matrix (usdm_gemv_wpack in usdm_hip.h; packer: usdm_amd/wpack.py).  A weight is its
// low byte, a 4-bit index of its upper seven exponent bits above `base`, and its sign.  A row is cut into units of 2048 elements
// = four K iterations; a unit is 3328 bytes: two planes of low bytes (lane L: 16 bytes = its pieces of iterations 0, 1 / 2, 3),
// one of nibbles (lane L: one dword per iteration; byte k = element k in bits 3:0, element k + 4 in bits 7:4) and one of sign
// dwords (lane L: the sign of element k of half j = 2 * iteration + (k >= 4) at bit 8 * (k & 3) + 7 - j).
constexpr unsigned GEMV_WPACK_UNIT = 3328;
// The eight bf16 weights of K iteration P (0..3) of a unit, as the bf16 kernels load them: lo0 / lo1 the low bytes of elements
// 0..3 / 4..7, nib the iteration's nibbles, sgn the unit's signs, base4 = base in every byte
template <int P>
__device__ __forceinline__ u32x4 gemv_wpack8(unsigned lo0, unsigned lo1, unsigned nib, unsigned sgn, unsigned base4) {
  const unsigned h0 = ((nib & 0x0f0f0f0fu) + base4) | ((sgn << (2 * P)) & 0x80808080u);          // high bytes of elements 0..3
  const unsigned h1 = (((nib >> 4) & 0x0f0f0f0fu) + base4) | ((sgn << (2 * P + 1)) & 0x80808080u);   // ... of 4..7
  u32x4 w;
  w[0] = __builtin_amdgcn_perm(h0, lo0, 0x05010400u);   // (selector bytes 0..3: the low bytes, 4..7: the high bytes)
  w[1] = __builtin_amdgcn_perm(h0, lo0, 0x07030602u);
  w[2] = __builtin_amdgcn_perm(h1, lo1, 0x05010400u);
  w[3] = __builtin_amdgcn_perm(h1, lo1, 0x07030602u);
  return w;
}

// ---- per-item arithmetic that every kernel above must share bit for bit (a batched step = independent steps)
// sum of squares of 8 bf16 onto ss, element pairs in order (the RMSNorm statistic)
__device__ __forceinline__ float gemv_sumsq8(u32x4 v, float ss) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = bf2f(v[e] & 0xffff), hi = bf2f(v[e] >> 16);
    ss += lo * lo + hi * hi;
  }
  return ss;
}
// RMSNorm of 8 bf16 with their 8 f32 weights, HF rounding: bf16(bf16(x * rstd) * weight)
__device__ __forceinline__ u32x4 gemv_rmsnorm8(u32x4 v, float rstd, float4 g0, float4 g1) {
  const float gw[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = bf2f(v[e] & 0xffff), hi = bf2f(v[e] >> 16);
    o[e] = pack_bf2(round_bf(round_bf(lo * rstd) * gw[2 * e]), round_bf(round_bf(hi * rstd) * gw[2 * e + 1]));
  }
  return o;
}
// weight row of SwiGLU output o in the packed gate/up layout: blocks of 32 rows = 16 gate + 16 up
__device__ __forceinline__ int gemv_glu_row(int o, bool up) { return (o >> 4) * 32 + (o & 15) + (up ? 16 : 0); }
// SwiGLU output of a gate / up pair of f32 sums; round_bf16: HF's rounding points (the projections' bf16 outputs, silu, the product)
__device__ __forceinline__ float gemv_swiglu_value(float g, float u, bool round_bf16) {
  if (round_bf16) {
    const float gt = round_bf(g), up = round_bf(u);
    return round_bf(round_bf(gt / (1.0f + __expf(-gt))) * up);
  }
  return (g / (1.0f + __expf(-g))) * u;
}
// output of a plain projection from its f32 sum: HF rounds the Linear output and the residual add.  res(): the residual value,
// asked for only where there is one (its pointer may be null otherwise)
template <class RES>
__device__ __forceinline__ float gemv_plain_value(float acc, bool round_bf16, bool has_res, RES&& res) {
  float v = acc;
  if (round_bf16) v = round_bf(v);
  if (has_res) {
    v += res();
    if (round_bf16) v = round_bf(v);
  }
  return v;
}
}  // namespace
