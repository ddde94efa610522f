// Batched decode (several utterances decoded in lockstep): the weight-streaming GEMV with NB input
// vectors.  Same streaming structure as gemv_kernel (llm_k.hip): every weight byte is still read exactly once per STEP,
// now amortised over NB tokens; per item the arithmetic (lane partition of K, accumulation order, rounding points) is
// identical to the batch-1 kernel, so a batched step reproduces NB independent steps bit for bit.
#include "common.h"
#include "../../include/usdm_hip.h"
#include "gemv_launch.h"

namespace {
// The weight formats (FP8: the row exponents as one extra kernel argument; MXFP4: selected by the type of that argument) are those
// of gemv_kernel, where the layouts are described; the format trait (load width, MXFP4 argument, ring depth, dot8) is
// gemv_common.h's, one text for both kernels.
// (NB = 4 needs 140 VGPRs in the gate/up variant = 3 workgroups per SIMD instead of 4, i.e. a third round of workgroups for
// the 1792-workgroup launch: 57 us instead of 40.  Forcing 128 VGPRs spills and was measured slower: 898 vs 967 tok/s.)
template <int RW, bool GLU, int NWV, int NB, bool FP8 = false, class... FMT>
__global__ __launch_bounds__(NWV * 64) void gemv_batch_kernel(const usdm_gemv_batch_args ba, FMT... fmt) {
  const usdm_gemv_args& a = ba.g;
  constexpr bool MX4 = gemv_is_mx4<FMT...>::value;
  static_assert((FP8 || MX4) == (sizeof...(FMT) == 1) && !(FP8 && MX4), "FP8 takes the row exponents, MXFP4 the block scales");
  typedef typename gemv_fmt<FP8>::wvec wvec;
  constexpr int NTH = NWV * 64;
  constexpr int NR = GLU ? 2 * RW : RW;
  constexpr int UNR = gemv_ring_depth(NR, FP8, MX4);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = (bf16_t*)smem;  // [NB][Kpad] bf16, zero padded
  __shared__ float red[NB][NWV];
  __shared__ float sv[NWV];
  __shared__ int si[NWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  const int Kpad = (K + 511) & ~511;
  const int nit = Kpad >> 9;

  const int rows_per_block = NWV * RW;
  const int ob = blockIdx.x * rows_per_block + wave * RW;
  const wvec* wp[NR];
  float wsc[NR];   // FP8: the rows' scales (unused in bf16)
  const unsigned* wsp[MX4 ? NR : 1];   // MX4: the rows' scale dwords of this lane's quad
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    int r = GLU ? gemv_glu_row(ob + (j % RW), j >= RW) : ob + j;
    r = r < a.N ? r : a.N - 1;
    if constexpr (FP8) {
      wp[j] = (const wvec*)((const uint8_t*)a.W + (int64_t)r * a.ldw) + lane;
      wsc[j] = fp8_row_scale(gemv_row_exp(fmt...)[r]);
    } else if constexpr (MX4) {
      const gemv_mx4 m = gemv_mx4_fmt(fmt...);
      wp[j] = (const u32x4*)((const uint8_t*)a.W + (int64_t)r * a.ldw) + lane;
      wsp[j] = (const unsigned*)(m.scales + (int64_t)r * m.lds) + (lane >> 2);
    } else {
      wp[j] = (const u32x4*)((const bf16_t*)a.W + (int64_t)r * a.ldw) + lane;
    }
  }
  const int ngr = (nit + 3) >> 2;   // MX4: groups of four K iterations
  const bool tail_ok = ((nit - 1) << 9) + lane * 8 < K;
  // lm_head mode: rows of banned ids are not streamed (see gemv_kernel)
  bool active = true;
  if (a.part_val && a.ban) {
    const int wb = blockIdx.x * rows_per_block;
    bool wg_active = false;
    for (int r = wb; r < wb + rows_per_block && r < a.N; ++r) wg_active |= (a.ban[r] == 0);
    if (!wg_active) {
      if (tid < NB) {
        a.part_val[(int64_t)tid * ba.part_bs + blockIdx.x] = -INFINITY;
        a.part_idx[(int64_t)tid * ba.part_bs + blockIdx.x] = 0x7fffffff;
      }
      if (a.y32 && tid < rows_per_block && wb + tid < a.N)
        for (int b = 0; b < NB; ++b) a.y32[(int64_t)b * ba.y_bs + wb + tid] = -INFINITY;
      return;
    }
    active = false;
#pragma unroll
    for (int j = 0; j < NR; ++j)
      if (ob + j < a.N) active |= (a.ban[ob + j] == 0);
    active = __builtin_amdgcn_readfirstlane(active);
  }
  auto wload = [&](int j, int it) -> wvec {
    if (!active) return wvec{};
    const wvec* p = (it == nit - 1 && !tail_ok) ? wp[j] - lane : wp[j] + it * 64;
    return __builtin_nontemporal_load(p);
  };
  wvec ring[NR][UNR];
  unsigned rsc[MX4 ? NR : 1][MX4 ? UNR : 1];   // MX4: the slots' scale dwords
#pragma unroll
  for (int u = 0; u < UNR; ++u)
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      if constexpr (MX4) {   // (the padded storage holds whole groups: no tail redirect)
        if (u < ngr) {
          ring[j][u] = __builtin_nontemporal_load(wp[j] + u * 64);
          rsc[j][u] = __builtin_nontemporal_load(wsp[j] + u * 16);
        }
      } else {
        if (u < nit) ring[j][u] = wload(j, u);
      }
    }

  // ---- stage the NB input vectors (optionally RMS-normalised, HF rounding) while the first ring is in flight
  if (a.norm_w) {
    float ss[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      ss[b] = 0.f;
      const bf16_t* xg = (const bf16_t*)a.x + (int64_t)b * ba.x_bs;
      for (int i = tid * 8; i < K; i += NTH * 8) {
        const u32x4 v = *(const u32x4*)(xg + i);   // (gemv_sumsq8's text: as the function the NWV = 12 / 16 forms compiled to other branches)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = bf2f(v[e] & 0xffff), hi = bf2f(v[e] >> 16);
          ss[b] += lo * lo + hi * hi;
        }
      }
      ss[b] = wave_sum(ss[b]);
      if (lane == 0) red[b][wave] = ss[b];
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < NWV; ++w) tot += red[b][w];
      const float rstd = rsqrtf(tot / (float)K + a.eps);
      const bf16_t* xg = (const bf16_t*)a.x + (int64_t)b * ba.x_bs;
      for (int i = tid * 8; i < Kpad; i += NTH * 8) {
        u32x4 o = {0, 0, 0, 0};
        if (i < K) o = gemv_rmsnorm8(*(const u32x4*)(xg + i), rstd, *(const float4*)(a.norm_w + i), *(const float4*)(a.norm_w + i + 4));
        *(u32x4*)(xs + (int64_t)b * Kpad + i) = o;
      }
    }
  } else {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const bf16_t* xg = (const bf16_t*)a.x + (int64_t)b * ba.x_bs;
      for (int i = tid * 8; i < Kpad; i += NTH * 8) {
        u32x4 v = {0, 0, 0, 0};
        if (i < K) v = *(const u32x4*)(xg + i);
        *(u32x4*)(xs + (int64_t)b * Kpad + i) = v;
      }
    }
  }
  __syncthreads();

  float acc[NR][NB];
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[j][b] = 0.f;
  if constexpr (MX4) {
    // slot u = group g: its four K iterations in order (the bf16 kernel's accumulation order per lane), then the refill
    auto step = [&](auto I, int g, int u) {
      constexpr int i = decltype(I)::value;
      const int it = 4 * g + i;
      if (it < nit) {
        u32x4 xv[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) xv[b] = *(const u32x4*)(xs + (int64_t)b * Kpad + (it * 64 + lane) * 8);
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const u32x4 wv = mx4x8_to_bf16x8<i>(ring[j][u][i], rsc[j][u]);
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[j][b] = dot8(wv, xv[b], acc[j][b]);
        }
      }
    };
    for (int g0 = 0; g0 < ngr; g0 += UNR) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int g = g0 + u;
        if (g < ngr) {
          step(gemv_ic<0>{}, g, u); step(gemv_ic<1>{}, g, u); step(gemv_ic<2>{}, g, u); step(gemv_ic<3>{}, g, u);
          if (g + UNR < ngr) {
#pragma unroll
            for (int j = 0; j < NR; ++j) {
              ring[j][u] = __builtin_nontemporal_load(wp[j] + (g + UNR) * 64);
              rsc[j][u] = __builtin_nontemporal_load(wsp[j] + (g + UNR) * 16);
            }
          }
        }
      }
    }
  } else
  for (int it0 = 0; it0 < nit; it0 += UNR) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int it = it0 + u;
      if (it < nit) {
        u32x4 xv[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) xv[b] = *(const u32x4*)(xs + (int64_t)b * Kpad + (it * 64 + lane) * 8);
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          if constexpr (FP8) {
            const u32x4 wv = fp8x8_to_bf16x8(ring[j][u], wsc[j]);
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[j][b] = dot8(wv, xv[b], acc[j][b]);
          } else {
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[j][b] = dot8(ring[j][u], xv[b], acc[j][b]);
          }
          if (it + UNR < nit) ring[j][u] = wload(j, it + UNR);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[j][b] = wave_sum(acc[j][b]);

  if (a.part_val) {  // lm_head: bf16-rounded logits, ban mask, per-block arg-max per item (ties -> lowest id)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int n = ob + j;
        if (n < a.N && !(a.ban && a.ban[n])) {
          const float v = round_bf(acc[j][b]);
          if (a.y32 && lane == 0) a.y32[(int64_t)b * ba.y_bs + n] = v;
          if (v > bv) { bv = v; bi = n; }
        } else if (n < a.N && a.y32 && lane == 0) {
          a.y32[(int64_t)b * ba.y_bs + n] = -INFINITY;
        }
      }
      if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
      __syncthreads();
      if (tid == 0) {
        for (int w = 1; w < NWV; ++w)
          if (sv[w] > bv) { bv = sv[w]; bi = si[w]; }
        a.part_val[(int64_t)b * ba.part_bs + blockIdx.x] = bv;
        a.part_idx[(int64_t)b * ba.part_bs + blockIdx.x] = bi == 0x7fffffff ? bi : bi + a.idx_offset;
      }
      __syncthreads();
    }
    return;
  }
  if (lane != 0) return;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (GLU) {
#pragma unroll
      for (int j = 0; j < RW; ++j) {
        const int o = ob + j;
        if (2 * o >= a.N) continue;
        const float r = gemv_swiglu_value(acc[j][b], acc[j + RW][b], a.round_bf16);
        if (a.y16) ((bf16_t*)a.y16)[(int64_t)b * ba.y_bs + o] = f2bf(r);
        if (a.y32) a.y32[(int64_t)b * ba.y_bs + o] = r;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int n = ob + j;
        if (n >= a.N) continue;
        float v = acc[j][b];   // (gemv_plain_value's text: as the function these loops compiled to other device code)
        if (a.round_bf16) v = round_bf(v);
        if (a.residual) {
          v += bf2f(((const bf16_t*)a.residual)[(int64_t)b * ba.res_bs + n]);
          if (a.round_bf16) v = round_bf(v);
        }
        if (a.y16) ((bf16_t*)a.y16)[(int64_t)b * ba.y_bs + n] = f2bf(v);
        if (a.y32) a.y32[(int64_t)b * ba.y_bs + n] = v;
      }
    }
  }
}

template <int NB, bool FP8 = false, class... FMT>
int launch_nb(const usdm_gemv_batch_args& ba, hipStream_t st, FMT... fmt) {
  const size_t lds = (size_t)((ba.g.K + 511) & ~511) * 2 * NB;
  const gemv_sel s = gemv_select(ba.g, true);   // the batch-1 launcher's table, without the forms that are batch-1 only
  const bool found = gemv_dispatch<GEMV_BATCH>(s, [&](auto RW, auto GLU, auto NWV) {
    constexpr int nwv = decltype(NWV)::value;
    auto kfn = gemv_batch_kernel<decltype(RW)::value, decltype(GLU)::value != 0, nwv, NB, FP8, FMT...>;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipLaunchKernelGGL(kfn, dim3(s.grid), dim3(nwv * 64), lds, st, ba, fmt...);
  });
  if (!found) return gemv_no_instantiation(s);
  USDM_LAUNCH_CHECK();
  return 0;
}
}  // namespace

int usdm_gemv_mfma_launch(const usdm_gemv_batch_args* pa, hipStream_t st);   // llm_mfma_k.hip: the matrix-core form, 1..16 sequences

extern "C" int usdm_gemv_batch(const usdm_gemv_batch_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->g.W && pa->g.x, "usdm_gemv_batch: null args");
  const usdm_gemv_args& a = pa->g;
  USDM_CHECK_ARG(pa->g.N > 0 && pa->g.K > 0, "usdm_gemv_batch: bad N/K");
  USDM_CHECK_ARG(a.y16 || a.y32 || a.part_val, "usdm_gemv_batch: no output");
  USDM_CHECK_ARG(!a.x_delta && !a.x_out, "usdm_gemv_batch: x_delta / x_out are batch-1 (tensor-parallel) only");
  if (pa->form == 1 || pa->form == 3 || pa->form == 5 || (pa->form == 0 && pa->nb > 4)) return usdm_gemv_mfma_launch(pa, (hipStream_t)stream);
  USDM_CHECK_ARG(pa->nb >= 1 && pa->nb <= 4, "usdm_gemv_batch: the VALU form takes 1..4 sequences per step (form = 1 or nb > 4: matrix cores, <= 16)");
  if (int rc = gemv_check_shape("usdm_gemv_batch", a, "input vectors")) return rc;   // (outputs: checked above, for both forms)
  USDM_CHECK_ARG(!a.part_val || (a.part_idx && a.act != USDM_ACT_SWIGLU && pa->part_bs >= cdiv(a.N, 16)), "usdm_gemv_batch: lm_head partial buffers");
  USDM_CHECK_ARG(pa->x_bs % 8 == 0, "usdm_gemv_batch: x stride must keep 16-B alignment");
  hipStream_t st = (hipStream_t)stream;
  switch (pa->nb) {
    case 1: return launch_nb<1>(*pa, st);
    case 2: return launch_nb<2>(*pa, st);
    case 3: return launch_nb<3>(*pa, st);
    default: return launch_nb<4>(*pa, st);
  }
}
// usdm_gemv_fp8 with 2..4 sequences (llm_k.hip checks the arguments it shares with the batch-1 form)
int usdm_gemv_fp8_batch_launch(const usdm_gemv_fp8_args* pa, hipStream_t st) {
  const usdm_gemv_args& a = pa->b.g;
  USDM_CHECK_ARG(!a.part_val || pa->b.part_bs >= cdiv(a.N, 16), "usdm_gemv_fp8: lm_head partial buffers");
  USDM_CHECK_ARG(pa->b.x_bs % 8 == 0, "usdm_gemv_fp8: x stride must keep 16-B alignment");
  switch (pa->b.nb) {
    case 2: return launch_nb<2, true>(pa->b, st, pa->row_exp);
    case 3: return launch_nb<3, true>(pa->b, st, pa->row_exp);
    default: return launch_nb<4, true>(pa->b, st, pa->row_exp);
  }
}
// usdm_gemv_mxfp4 with 2..4 sequences (llm_k.hip checks the arguments it shares with the batch-1 form)
int usdm_gemv_mxfp4_batch_launch(const usdm_gemv_mxfp4_args* pa, hipStream_t st) {
  USDM_CHECK_ARG(pa->b.x_bs % 8 == 0, "usdm_gemv_mxfp4: x stride must keep 16-B alignment");
  const gemv_mx4 m{pa->scales, pa->lds};
  switch (pa->b.nb) {
    case 2: return launch_nb<2, false>(pa->b, st, m);
    case 3: return launch_nb<3, false>(pa->b, st, m);
    default: return launch_nb<4, false>(pa->b, st, m);
  }
}
extern "C" int usdm_sizeof_gemv_batch_args(void) { return (int)sizeof(usdm_gemv_batch_args); }
