// What the weight-streaming decode GEMVs share: gemv_kernel (llm_k.hip), gemv_batch_kernel (llm_batch_k.hip) and, for the row
// exponents only, gemv_mfma_kernel (llm_mfma_k.hip); the experimental kernels take dot8.
//   * the weight-format trait (bf16 / FP8 / MXFP4): load width, the MXFP4 argument, the ring depth;
//   * the per-item arithmetic the two VALU kernels must share bit for bit.
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

// ---- per-item arithmetic that gemv_kernel and gemv_batch_kernel must share bit for bit (a batched step = independent steps)
// SwiGLU output of a gate / up pair of f32 sums; round_bf16: HF's rounding points (the projections' bf16 outputs, silu, the product)
__device__ __forceinline__ float gemv_swiglu_value(float g, float u, bool round_bf16) {
  if (round_bf16) {
    const float gt = round_bf(g), up = round_bf(u);
    return round_bf(round_bf(gt / (1.0f + __expf(-gt))) * up);
  }
  return (g / (1.0f + __expf(-g))) * u;
}
}  // namespace
