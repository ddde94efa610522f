// Structural pieces of the bf16 batch-1 decode GEMVs of llm_k.hip, one text each (the arithmetic pieces: gemv_common.h).
//   * gemv_load16, gemv_early_loads: the hand-counted early loads of x and the RMSNorm weights
//       gemv_kernel, gemv_resident_kernel and gemv_resident_wpack_kernel (x + two weight pieces); gemv_stream_kernel and
//       gemv_stream_wpack_kernel (gemv_load16 twice: two pieces of x);
//   * gemv_ring_load: the hand-counted ring load of the straight-line K loops - gemv_resident_kernel, gemv_stream_kernel and the
//       marked rows of the two packed kernels;
//   * gemv_unit_load: the hand-counted ring load of a unit of the 13-bit weight image - gemv_stream_wpack_kernel,
//       gemv_resident_wpack_kernel;
//   * gemv_rms_rstd: the RMSNorm statistic over the waves of a workgroup - gemv_kernel, gemv_resident_kernel,
//       gemv_resident_wpack_kernel, the chain's stage_x.
// None of them puts a run-time branch around a load that is issued before a counted wait: the wait-count pass drains the ring at
// control-flow joins around loads (gemv_kernel's comments).
// What stays text in its kernels, because as a function it compiled to other device code in gemv_kernel (tools/isa_diff.py
// --classify against the text, profiles/gemv_shared_text.txt): the x staging loops around these pieces, the row / scale pointer
// set-up and the banned-rows tests of the lm_head mode.
#pragma once
#include "gemv_common.h"

namespace {
// ---- HAND-COUNTED loads (asm, invisible to the compiler's wait-count pass; cdna_hip_programming.md 5.7): the caller waits for them
// with an asm s_waitcnt that names how many younger loads stay in flight.
__device__ __forceinline__ void gemv_load16(u32x4& dst, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
// The thread's first piece of x (elements i0 ..) and its RMSNorm weights.  Unconditional: a clamped index, and without RMSNorm the
// two weight loads re-read the first 16 bytes of x (always there, K >= 8) and are not used.
__device__ __forceinline__ void gemv_early_loads(const usdm_gemv_args& a, int i0, int K, u32x4& x0, u32x4& ge0v, u32x4& ge1v) {
  const int ic = min(i0, K - 8);
  const float* gp0 = a.norm_w ? a.norm_w + ic : (const float*)a.x;
  const float* gp1 = a.norm_w ? gp0 + 4 : gp0;
  gemv_load16(x0, (const bf16_t*)a.x + ic);
  gemv_load16(ge0v, gp0);
  gemv_load16(ge1v, gp1);
}
// Ring load of K iteration IT (512 elements = 1024 bytes) of a bf16 row: scalar row base + lane offset (voff = lane * 16, plus 4096
// per four iterations) + immediate, non-temporal.
template <int IT>
__device__ __forceinline__ void gemv_ring_load(u32x4& dst, const char* row, unsigned voff) {
  const unsigned vo = voff + (IT >> 2) * 4096u;
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3 nt" : "=v"(dst) : "v"(vo), "s"(row), "n"((IT & 3) * 1024) : "memory");
}
// Ring load of unit U (2048 elements = four K iterations) of a row of the 13-bit image (gemv_common.h): the lane's 16 bytes of each
// of the two low-byte planes and of the nibble plane and its sign dword - four loads, in this order.  voff = lane * 16.
struct gemv_wunit { u32x4 la, lb, nib; unsigned sgn; };
template <int U>
__device__ __forceinline__ void gemv_unit_load(gemv_wunit& d, const char* row, unsigned voff) {
  const unsigned vo = voff + U * GEMV_WPACK_UNIT, vs = (voff >> 2) + U * GEMV_WPACK_UNIT;
  asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(d.la) : "v"(vo), "s"(row) : "memory");
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024 nt" : "=v"(d.lb) : "v"(vo), "s"(row) : "memory");
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:2048 nt" : "=v"(d.nib) : "v"(vo), "s"(row) : "memory");
  asm volatile("global_load_dword %0, %1, %2 offset:3072 nt" : "=v"(d.sgn) : "v"(vs), "s"(row) : "memory");
}

// ---- RMSNorm statistic of a workgroup of NWV waves: the threads' sums of squares over K elements reduced per wave, then over the
// waves in order (red[NWV] in LDS; one barrier) -> 1 / rms
template <int NWV>
__device__ __forceinline__ float gemv_rms_rstd(float ss, float* red, int K, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  ss = wave_sum(ss);
  if (lane == 0) red[wave] = ss;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < NWV; ++w) tot += red[w];
  return rsqrtf(tot / (float)K + eps);
}
}  // namespace
