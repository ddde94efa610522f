// Mistral-7B decode kernels other than the shared GEMM / flash-attention / norm kernels: the weight-streaming GEMV and the small glue
// kernels (arg-max, embedding, residual add, dequantization).  What touches the KV cache - rope + append, decode attention - is in
// llm_attn_k.hip.
//
// The decode step is HBM-bound (14.3 GB of bf16 weights per token at batch 1), so the design rule is:
// every weight byte is read exactly once, 16 B per lane, non-temporal, many loads in flight, and
// everything else (RMSNorm, residual add, SwiGLU, ban-mask + argmax) is fused into the GEMV that
// produces or consumes the vector.  Rounding points follow HF transformers' bf16 Mistral
// (third-party arithmetic of the reference): every Linear output, RMSNorm, RoPE
// product and residual add is rounded to bf16; logits are bf16 values compared in fp32.
#include "common.h"
#include <stdlib.h>
#include <utility>
#include "../../include/usdm_hip.h"
#include "gemv_launch.h"
#include "gemv_pieces.h"
#include "attn_merge.h"
#include "p2p.h"
#include "pick_commit.h"

#ifndef USDM_GEMV_DOWN_UNR
#define USDM_GEMV_DOWN_UNR 8   // ring depth of gemv_stream_kernel (12 for A/B builds: 48 of its 128 VGPRs)
#endif
#ifndef USDM_GEMV_WPACK_RU
#define USDM_GEMV_WPACK_RU 3   // units in flight per lane in gemv_stream_wpack_kernel (156 bytes; 2 and 4 for A/B builds)
#endif
#ifndef USDM_GEMV_WPACK_UB
#define USDM_GEMV_WPACK_UB 12  // ring depth of its marked (bf16) rows
#endif
#ifndef USDM_GEMV_GU_WPACK_RU
#define USDM_GEMV_GU_WPACK_RU 4   // units in flight per lane in gemv_resident_wpack_kernel (208 bytes; 5 and 6 for A/B builds)
#endif
namespace {
// ---------------------------------------------------------------------------------------------
// GEMV: y = W x, W bf16 [N][ldw] row-major (the nn.Linear layout).
//   * workgroup = 4 waves; a wave owns RW output rows (GLU: RW gate + RW up rows) and streams them
//     together, lanes striding K in 16-B pieces, non-temporal loads;
//   * a ring of UNR K-iterations per row is always in flight (NR*UNR 16-B loads per lane), and the first
//     ring is issued BEFORE x is staged / RMS-normalised into LDS, so the prologue hides under HBM latency;
//   * RW is chosen by the launcher so that the grid is a whole number of workgroups per CU.
// ---------------------------------------------------------------------------------------------
#ifdef USDM_GEMV_TRACE
// debugging aid (tools/gemv_trace.py): per-workgroup phase timestamps (100 MHz wall clock)
__device__ unsigned long long g_gemv_trace[8192 * 8];
#define GTR(i) do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_gemv_trace[blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define GTR(i) do { } while (0)
#endif

// MRG: the merged-attention input form (usdm_gemv_args.mrg_*) is a separate instantiation: its 16 partial loads per thread cost
// ~64 VGPRs, which lowered the occupancy of EVERY shape when the branch lived in the common kernel (measured: all GEMVs 20-30 %
// slower, profiles/r02_decode_ablation.txt).
// P2P: the fused peer-to-peer all-reduce epilogue (tensor-parallel decode) is likewise its own instantiation, so the single-GPU
// kernels carry none of it.
// CMB: the hand-off form of the merged-attention input (usdm_gemv_args.cmb_gran): one combine per head by the launch's first
// workgroups, granules to everyone, the wait under the first weight ring.  Its own instantiation for the same reason.
// FP8: the weight-only FP8 format (usdm_gemv_fp8): 8-byte loads of e4m3 bytes in the bf16 kernel's K-to-lane assignment, converted
// in registers with the row's power-of-two scale (exact), then the bf16 arithmetic unchanged.  The ring is twice as deep, so the
// same number of bytes is in flight per lane; only the weight load and unpack differ.  The row exponents come as one extra kernel
// argument (FP8 only: the bf16 instantiations keep their exact signature and code).
// MX4: the weight-only MXFP4 format (usdm_gemv_mxfp4; selected by the type of the extra argument, so FP8 stays a bool and the
// existing instantiations keep their names).  A row is stored in groups of 2048 elements = 1024 bytes, interleaved so that the 16
// bytes of lane L in group g are its codes of the four K iterations 4g .. 4g+3 (dword i: elements 2048g + 512i + 8L ..+7, the
// elements that lane accumulates in iteration 4g+i of the bf16 kernel); the scale bytes are interleaved the same way, so the four
// lanes that share a block read ONE dword holding their scales of the four iterations.  Rows are padded with zero codes to whole
// groups (x in LDS is zero only up to Kpad: iterations past nit are skipped, not multiplied).  A ring slot is one group.
// The format trait (load width, MXFP4 argument, ring depth, dot8) is gemv_common.h's, shared with gemv_batch_kernel.

template <int RW, bool GLU, int NWV, bool MRG = false, bool P2P = false, bool CMB = false, bool FP8 = false, class... FMT>
__global__ __launch_bounds__(NWV * 64) void gemv_kernel(const usdm_gemv_args a, FMT... fmt) {
  typedef typename gemv_fmt<FP8>::wvec wvec;
  constexpr bool MX4 = gemv_is_mx4<FMT...>::value;
  static_assert((FP8 || MX4) == (sizeof...(FMT) == 1) && !(FP8 && MX4), "FP8 takes the row exponents, MXFP4 the block scales");
  static_assert(!(FP8 || MX4) || (!MRG && !P2P && !CMB), "the FP8 / MXFP4 weight formats have the plain single-GPU forms only");
  constexpr int NTH = NWV * 64;
  constexpr int NR = GLU ? 2 * RW : RW;   // rows streamed together by one wave
  constexpr int UNR = gemv_ring_depth(NR, FP8, MX4);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = (bf16_t*)smem;  // [Kpad] bf16, zero padded
  __shared__ float red[NWV];
  __shared__ float sv[NWV];
  __shared__ int si[NWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int skipv = a.skip ? *a.skip : 0;   // requested now, tested once the first ring is in flight (no exposed latency)
  unsigned p2p_epoch = 0u;      // likewise requested now, used only in the epilogue
  bool p2p_failed = false;
  if constexpr (P2P) { p2p_epoch = p2p_load_epoch(a.p2p); p2p_failed = p2p_load_err(a.p2p) != 0u; }
  GTR(0);
  const int K = a.K;
  const int Kpad = (K + 511) & ~511;
  const int nit = Kpad >> 9;

  // ---- rows of this wave
  const int rows_per_block = NWV * RW;                    // output features per workgroup
  const int ob = blockIdx.x * rows_per_block + wave * RW; // first output feature of this wave
  const wvec* wp[NR];
  float wsc[NR];   // FP8: the rows' scales (requested here, before the hand-counted loads below; unused in bf16)
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
  const bool tail_ok = ((nit - 1) << 9) + lane * 8 < K;  // is this lane inside K on the last iteration?
  // lm_head mode: a wave whose rows are ALL banned (the reference's bad_words_ids mask whole id ranges: 76 % of the vocabulary
  // in the text->unit round, inference.py:51-53) streams nothing; its logits are -inf either way
  bool active = true;
  if (a.part_val && a.ban) {
    // whole workgroup banned: publish "no candidate" and leave before anything is staged (no barrier has been reached yet)
    const int wb = blockIdx.x * rows_per_block;
    bool wg_active = false;
    for (int r = wb; r < wb + rows_per_block && r < a.N; ++r) wg_active |= (a.ban[r] == 0);
    if (!wg_active) {
      if (tid == 0) { a.part_val[blockIdx.x] = -INFINITY; a.part_idx[blockIdx.x] = 0x7fffffff; }
      if (a.y32 && tid < rows_per_block && wb + tid < a.N) a.y32[wb + tid] = -INFINITY;
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
    // last iteration may run past K: redirect to the row start (x is zero there in LDS, contributes 0)
    const wvec* p = (it == nit - 1 && !tail_ok) ? wp[j] - lane : wp[j] + it * 64;
    return __builtin_nontemporal_load(p);
  };
  // The residual values of this wave's rows are requested HERE, at the start, not in the epilogue (round 4): there the
  // load was a full memory latency at the very end of every o_proj / down_proj launch, with nothing left to hide it.  Unconditional
  // (a predicated load is waited for at the join of its predicate): without a residual the address is the weight row, never used.
  unsigned short resraw[GLU ? 1 : NR];
  if constexpr (!GLU) {
    const bf16_t* rbase = a.residual ? (const bf16_t*)a.residual : (const bf16_t*)a.W;
#pragma unroll
    for (int j = 0; j < NR; ++j) resraw[j] = rbase[min(ob + j, a.N - 1)];
  }
  // (round 4) This thread's first piece of the input vector and its RMSNorm weights are requested BEFORE the weight ring.  Loads
  // return in order: behind the ring they landed only when the whole ring had (~2 us), and the RMSNorm prologue - sum of squares,
  // barrier, a SECOND read of x and of the weights, normalise, barrier - started after that, with no weight load of this workgroup
  // in flight.  Now the prologue runs under the ring's latency and reads nothing twice.  Unconditional loads (clamped index; a
  // dummy address without RMSNorm): a predicated load would be waited for at the join of its predicate, i.e. before the ring is
  // issued.  Not in the merged-input variants (their x is not in memory).
  constexpr bool EARLY = !CMB && !MRG;
  const int i0 = tid * 8;
  // The three loads are HAND-COUNTED (asm, invisible to the compiler; cdna_hip_programming.md 5.7): the ring below is issued under
  // run-time tests (u < nit), so the wait-count pass cannot know how many loads are younger than x0 and would wait for all but the
  // few it is sure of - the whole ring again.  The wait further down names the exact count for the full-ring case.
  u32x4 x0 = {0u, 0u, 0u, 0u}, ge0v = x0, ge1v = x0;
  if constexpr (EARLY) gemv_early_loads(a, i0, K, x0, ge0v, ge1v);
  // The first ring is ALWAYS NR x UNR loads (slots past the row's K, or of a wave whose rows are all banned, re-read the row start
  // and are never multiplied / their results never used): the wait for the early loads below can then name an exact count.
  wvec ring[NR][UNR];
  unsigned rsc[MX4 ? NR : 1][MX4 ? UNR : 1];   // MX4: the slots' scale dwords
#pragma unroll
  for (int u = 0; u < UNR; ++u)
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      if constexpr (MX4) {   // (the padded storage holds whole groups: no tail redirect; slots past the row re-read group 0)
        const int g = u < ngr ? u : 0;
        ring[j][u] = __builtin_nontemporal_load(wp[j] + g * 64);
        rsc[j][u] = __builtin_nontemporal_load(wsp[j] + g * 16);
      } else {
        const bool real = active && u < nit;
        const wvec* p = real ? ((u == nit - 1 && !tail_ok) ? wp[j] - lane : wp[j] + u * 64) : wp[j] - lane;
        ring[j][u] = __builtin_nontemporal_load(p);
      }
    }
  GTR(1);
  if constexpr (EARLY) {
    // in-order completion: "all but the NY youngest" = the three early loads have landed, the ring stays in flight.  ONE wait site on
    // every path (two sites in two branches made the compiler copy the registers of the loads at the branch - before the wait)
    constexpr int NY = (MX4 ? 2 : 1) * UNR * NR;      // (the residual loads above are older: nothing else is issued between the early loads and here)
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(x0), "+v"(ge0v), "+v"(ge1v) : "n"(NY));
  }
  if (skipv) return;   // the sequence ended in an earlier step of this host chunk (usdm_decode_state.done)
  const float4 ge0 = __builtin_bit_cast(float4, ge0v), ge1 = __builtin_bit_cast(float4, ge1v);
  // ---- stage x into LDS (optionally fused RMSNorm with HF rounding) while the first ring is in flight
  const bf16_t* xg = (const bf16_t*)a.x;
  // 8 consecutive elements of the input vector; with x_delta the pending residual add of the tensor-parallel path is applied
  // on the fly (HF rounding: bf16(h + bf16(delta))) and workgroup 0 publishes the updated residual stream
  auto with_delta = [&](u32x4 v, int i, bool publish) -> u32x4 {
    if (a.x_delta) {
      const float4 d0 = *(const float4*)(a.x_delta + i), d1 = *(const float4*)(a.x_delta + i + 4);
      const float dl[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
        v[e] = pack_bf2(bf2f(v[e] & 0xffff) + round_bf(dl[2 * e]), bf2f(v[e] >> 16) + round_bf(dl[2 * e + 1]));
      if (publish && a.x_out && blockIdx.x == 0) *(u32x4*)((bf16_t*)a.x_out + i) = v;
    }
    return v;
  };
  auto ldx = [&](int i, bool publish) -> u32x4 { return with_delta(*(const u32x4*)(xg + i), i, publish); };
  const int iloop = EARLY ? i0 + NTH * 8 : i0;               // EARLY: the first piece is x0, the loops below take the rest
  // (this staging and gemv_resident_kernel's stay two texts: as one function the x_delta tests compile to other branches here)
  if (a.norm_w) {
    float ss = 0.f;
    u32x4 v0 = x0;
    if constexpr (EARLY) {
      if (i0 < K) {
        v0 = with_delta(x0, i0, false);
        ss = gemv_sumsq8(v0, ss);
      }
    }
    for (int i = iloop; i < K; i += NTH * 8) ss = gemv_sumsq8(ldx(i, false), ss);
    const float rstd = gemv_rms_rstd<NWV>(ss, red, K, a.eps);
    if constexpr (EARLY) {
      if (i0 < Kpad) {
        u32x4 o = {0, 0, 0, 0};
        if (i0 < K) {
          if (a.x_delta && a.x_out && blockIdx.x == 0) *(u32x4*)((bf16_t*)a.x_out + i0) = v0;
          o = gemv_rmsnorm8(v0, rstd, ge0, ge1);
        }
        *(u32x4*)(xs + i0) = o;
      }
    }
    for (int i = iloop; i < Kpad; i += NTH * 8) {
      u32x4 o = {0, 0, 0, 0};
      if (i < K) o = gemv_rmsnorm8(ldx(i, true), rstd, *(const float4*)(a.norm_w + i), *(const float4*)(a.norm_w + i + 4));
      *(u32x4*)(xs + i) = o;
    }
  } else if constexpr (CMB) {
    // ---- (1) the first K/128 workgroups combine one head each on threads 0..127 (attn_merge.h, as attn_combine_kernel does)
    const int NS = a.mrg_ns;
    float* cw = (float*)smem;                                // [64] split weights + [1] 1/l (the x staging area is still free)
    if ((int)blockIdx.x < (K >> 7)) {
      const int hq = blockIdx.x, d = tid;
      if (d < 64) {
        const float inv = attn_merge_weights(NS, d, cw, [&](int s) { return a.mrg_pm[hq * NS + s]; }, [&](int s) { return a.mrg_pl[hq * NS + s]; });
        if (d == 0) cw[64] = inv;
      }
      __syncthreads();
      if (d < 128) {
        const float* p = a.mrg_po + (int64_t)hq * NS * 128 + d;
        const float o = attn_merge_sum<4>(NS, cw, [&](int s) { return p[s * 128]; });
        const unsigned v = f2bf(o * cw[64]);
        const unsigned hi = __shfl_down(v, 1, 64);           // element d + 1 (d even: same wave)
        if (!(d & 1))
          __hip_atomic_store(a.cmb_gran + hq * 64 + (d >> 1), (1ull << 32) | (unsigned long long)(v | (hi << 16)), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();                                       // cw is dead before the gather overwrites the staging area
    }
    // ---- (2) every workgroup gathers the K/2 granules into its LDS copy of x (bounded re-reads of the ones not there yet)
    {
      const unsigned long long tmo = (unsigned long long)(a.cmb_timeout_ms > 0 ? a.cmb_timeout_ms : 200) * 100000ull;
      const unsigned long long t0 = wall_clock64();
      bool late = false;
      for (int i = tid; i < (Kpad >> 1); i += NTH) {
        unsigned val = 0u;
        if (i < (K >> 1)) {
          unsigned long long g = __hip_atomic_load(a.cmb_gran + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          unsigned spins = 0;
          while ((unsigned)(g >> 32) != 1u && !late) {
            __builtin_amdgcn_s_sleep(1);
            g = __hip_atomic_load(a.cmb_gran + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((++spins & 63) == 63 && wall_clock64() - t0 > tmo) late = true;
          }
          val = (unsigned)(g >> 32) == 1u ? (unsigned)g : 0u;
        }
        *(unsigned*)(xs + 2 * i) = val;
      }
      if (late && a.cmb_err) atomicOr((int*)a.cmb_err, 1);
    }
  } else if constexpr (MRG) {
    // o_proj of the decode step: x is MERGED here from the context-split attention partials (usdm_gemv_args.mrg_*), four
    // elements of one head per thread; the partial loads of a chunk of 8 splits are requested before the first is used.
    const int NS = a.mrg_ns;
    for (int i = tid * 4; i < Kpad; i += NTH * 4) {
      u32x2 r = {0u, 0u};
      if (i < K) {
        const int hq = i >> 7, d = i & 127;
        const float* pm = a.mrg_pm + hq * NS;
        const float* pl = a.mrg_pl + hq * NS;
        const float* po = a.mrg_po + (int64_t)hq * NS * 128 + d;
        float m = -1e30f;
        for (int s = 0; s < NS; ++s) m = fmaxf(m, pm[s]);
        float l = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
        for (int s0 = 0; s0 < NS; s0 += 8) {
          float4 p[8];
          float w[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int s = min(s0 + u, NS - 1);
            p[u] = *(const float4*)(po + (int64_t)s * 128);
            w[u] = (s0 + u < NS) ? __expf(pm[s] - m) : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            l = fmaf((s0 + u < NS) ? pl[min(s0 + u, NS - 1)] : 0.f, w[u], l);
            o0 = fmaf(p[u].x, w[u], o0); o1 = fmaf(p[u].y, w[u], o1); o2 = fmaf(p[u].z, w[u], o2); o3 = fmaf(p[u].w, w[u], o3);
          }
        }
        const float inv = 1.0f / l;
        r[0] = pack_bf2(o0 * inv, o1 * inv);
        r[1] = pack_bf2(o2 * inv, o3 * inv);
      }
      *(u32x2*)(xs + i) = r;
    }
  } else {
    if constexpr (EARLY) {
      if (i0 < Kpad) {
        u32x4 v = {0, 0, 0, 0};
        if (i0 < K) v = with_delta(x0, i0, true);
        *(u32x4*)(xs + i0) = v;
      }
    }
    for (int i = iloop; i < Kpad; i += NTH * 8) {
      u32x4 v = {0, 0, 0, 0};
      if (i < K) v = ldx(i, true);
      *(u32x4*)(xs + i) = v;
    }
  }
  __syncthreads();
  GTR(2);

  // ---- stream: consume ring slot, immediately refill it UNR iterations ahead
  float acc[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) acc[j] = 0.f;
  if constexpr (MX4) {
    // slot u = group g: its four K iterations in order (the bf16 kernel's accumulation order per lane), then the refill
    auto step = [&](auto I, int g, int u) {
      constexpr int i = decltype(I)::value;
      const int it = 4 * g + i;
      if (it < nit) {
        const u32x4 xv = *(const u32x4*)(xs + (it * 64 + lane) * 8);
#pragma unroll
        for (int j = 0; j < NR; ++j) acc[j] = dot8(mx4x8_to_bf16x8<i>(ring[j][u][i], rsc[j][u]), xv, acc[j]);
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
        const u32x4 xv = *(const u32x4*)(xs + (it * 64 + lane) * 8);
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          if constexpr (FP8) acc[j] = dot8(fp8x8_to_bf16x8(ring[j][u], wsc[j]), xv, acc[j]);
          else acc[j] = dot8(ring[j][u], xv, acc[j]);
          if (it + UNR < nit) ring[j][u] = wload(j, it + UNR);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) acc[j] = wave_sum(acc[j]);
  GTR(3);

  // ---- epilogue
  if (a.part_val) {  // lm_head: bf16-rounded logits, ban mask, per-block arg-max (ties -> lowest id)
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int n = ob + j;
      if (n < a.N && !(a.ban && a.ban[n])) {
        const float v = round_bf(acc[j]);
        if (a.y32 && lane == 0) a.y32[n] = v;
        if (v > bv) { bv = v; bi = n; }
      } else if (n < a.N && a.y32 && lane == 0) {
        a.y32[n] = -INFINITY;
      }
    }
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < NWV; ++w)
        if (sv[w] > bv) { bv = sv[w]; bi = si[w]; }
      a.part_val[blockIdx.x] = bv;
      a.part_idx[blockIdx.x] = bi == 0x7fffffff ? bi : bi + a.idx_offset;
    }
    return;
  }
  if constexpr (P2P && !GLU) {
    // Row-parallel projection of the tensor-parallel decode: the all-reduce of the f32 partial sums happens HERE, between the
    // workgroups that own the same rows on every rank (protocol: include/usdm_hip.h, usdm_allreduce_p2p_*).  No workgroup
    // waits for another workgroup of its own rank, so progress never depends on how much of the grid is resident.
    const usdm_p2p_dev* d = a.p2p;
    constexpr int RPB = NWV * RW;
    float* prow = (float*)smem;          // [RPB] this rank's partials (x in LDS is dead after the K loop)
    float* pg = prow + RPB;              // [world][RPB] gathered partials
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < NR; ++j) prow[wave * RW + j] = acc[j];
    }
    __syncthreads();
    const int wb = blockIdx.x * RPB, world = d->world, me = d->rank;
    for (int t = tid; t < world * RPB; t += NTH) {          // put: one granule per (peer, row), coalesced per peer
      const int peer = t / RPB, r = t - peer * RPB;
      if (wb + r < a.N) p2p_put(p2p_slot(d, peer, p2p_epoch, a.p2p_site, me) + wb + r, p2p_epoch, prow[r]);
    }
    if (a.p2p_mode == 2) return;                            // split mode: usdm_allreduce_p2p_reduce finishes
    for (int t0 = 0; t0 < world * RPB; t0 += NTH) {         // get: uniform trip count (p2p_get is a wave-uniform bounded loop)
      const int t = t0 + tid;
      const int src = t / RPB, r = t - src * RPB;
      const bool in = t < world * RPB;
      const bool want = in && wb + r < a.N && src != me;
      const float v = p2p_get(d, p2p_slot(d, me, p2p_epoch, a.p2p_site, want ? src : 0) + (want ? wb + r : 0), p2p_epoch, want,
                              USDM_P2P_ERR_TIMEOUT_ROWS, p2p_failed);
      if (in) pg[src * RPB + r] = (src == me) ? prow[r] : v;
    }
    __syncthreads();
    if (tid < RPB && wb + tid < a.N) {
      const int n = wb + tid;
      float s = 0.f;
      for (int src = 0; src < world; ++src) s += pg[src * RPB + tid];   // fixed rank order: identical bits on every rank
      const float v = round_bf(round_bf(s) + bf2f(((const bf16_t*)a.residual)[n]));
      ((bf16_t*)a.y16)[n] = f2bf(v);
    }
    return;
  }
  if (lane != 0) return;
  if (GLU) {
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      const int o = ob + j;
      if (2 * o >= a.N) continue;
      const float r = gemv_swiglu_value(acc[j], acc[j + RW], a.round_bf16);
      if (a.y16) ((bf16_t*)a.y16)[o] = f2bf(r);
      if (a.y32) a.y32[o] = r;
    }
  } else {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int n = ob + j;
      if (n >= a.N) continue;
      const float v = gemv_plain_value(acc[j], a.round_bf16, a.residual != nullptr, [&] { return bf2f(resraw[j]); });
      if (a.y16) ((bf16_t*)a.y16)[n] = f2bf(v);
      if (a.y32) a.y32[n] = v;
    }
  }
}

template <class F, int... I>
__device__ __forceinline__ void gemv_for_seq(F&& f, std::integer_sequence<int, I...>) { (f(gemv_ic<I>{}), ...); }
// f(gemv_ic<0>{}) ... f(gemv_ic<N - 1>{}): a loop whose counter is a constant expression (asm immediates)
template <int N, class F>
__device__ __forceinline__ void gemv_for(F&& f) { gemv_for_seq(f, std::make_integer_sequence<int, N>{}); }

// ---------------------------------------------------------------------------------------------
// Resident multi-tile form of gemv_kernel<RW, true, NWV> for bf16 weights (gate/up of the decode step).
// The grid is the number of workgroups the device holds at once, not the number of tiles: workgroup b takes the tiles b,
// b + grid, ... (a tile = the NWV * RW outputs of one gemv_kernel workgroup).  The prologue - skip word, hand-counted early loads,
// first ring, the one counted wait, x staged and RMS-normalised into LDS - runs ONCE per workgroup, as gemv_kernel's.  The ring
// never drains between tiles: in the last UNR iterations of a tile every freed slot is refilled from the rows of the next tile
// (slot u = its iteration u, what the first ring holds), so the wave reduction, SwiGLU and store of a tile run with the next
// tile's ring in flight.  The last tile keeps gemv_kernel's tail.
// Per output the arithmetic is gemv_kernel's, statement for statement: the lane-to-K assignment, the iteration order, dot8,
// wave_sum, gemv_swiglu_value, the RMSNorm partition over NWV waves and its rounding points - identical bits.
// TPW > 0, NIT > 0: every workgroup has exactly TPW tiles and K = NIT * 512, both compile-time, so that the tile seam is
// straight-line code (the wait-count pass drains the ring at control-flow joins around loads: profiles/r04_decode_ablation.txt
// items 1 and 13).  TPW = 0, NIT = 0: any tile count per workgroup (also uneven), any K, ragged last tile; correct, seams not tuned.
// No x_delta (the launcher keeps the one-tile form for it).
// ---------------------------------------------------------------------------------------------
template <int RW, int NWV, int TPW, int NIT>
__global__ __launch_bounds__(NWV * 64) __attribute__((amdgpu_waves_per_eu(4))) void gemv_resident_kernel(const usdm_gemv_args a) {
  static_assert((TPW > 0) == (NIT > 0), "straight-line seams need both counts");
  constexpr int NTH = NWV * 64;
  constexpr int NR = 2 * RW;
  constexpr int UNR = gemv_ring_depth(NR, false, false);
  constexpr int TILE = NWV * RW;   // outputs per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = (bf16_t*)smem;  // [Kpad] bf16, zero padded
  __shared__ float red[NWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int skipv = a.skip ? *a.skip : 0;
  GTR(0);
  const int K = a.K;
  const int Kpad = (K + 511) & ~511;
  const int nit = NIT ? NIT : Kpad >> 9;
  const bool tail_ok = NIT ? true : ((nit - 1) << 9) + lane * 8 < K;
  // row j of this wave in tile t (packed layout: blocks of 32 rows = 16 gate + 16 up; rows past N re-read the last row, never stored)
  const int uwave = __builtin_amdgcn_readfirstlane(wave);   // the row bases are wave-uniform: scalar registers, one lane offset
  auto row_ptr = [&](int t, int j) -> const char* {
    const int o = (blockIdx.x + t * gridDim.x) * TILE + uwave * RW + (j % RW);
    int r = gemv_glu_row(o, j >= RW);
    r = r < a.N ? r : a.N - 1;
    return (const char*)((const bf16_t*)a.W + (int64_t)r * a.ldw);
  };
  const unsigned voff = lane * 16;   // this lane's 16 bytes of a K iteration (512 elements = 1024 bytes)
  // Generic form: compiler-issued loads, the last iteration past K redirected to the row start (x is zero there in LDS).
  auto wload = [&](const char* p, int it) -> u32x4 {
    return __builtin_nontemporal_load((const u32x4*)(p + ((it == nit - 1 && !tail_ok) ? 0u : voff + it * 1024u)));
  };
  // Straight-line form: HAND-COUNTED ring loads (gemv_ring_load), invisible to the wait-count pass like the early loads below, each
  // consumed behind an asm wait that names how many younger loads stay in flight.  Left to the compiler, the straight-line ring
  // was clustered into bursts with vmcnt(0) between them and spilled.
  const char* wp[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) wp[j] = row_ptr(0, j);
  // ---- prologue, once per workgroup (gemv_kernel's EARLY form)
  const int i0 = tid * 8;
  u32x4 x0 = {0u, 0u, 0u, 0u}, ge0v = x0, ge1v = x0;
  gemv_early_loads(a, i0, K, x0, ge0v, ge1v);
  u32x4 ring[NR][UNR];   // always NR x UNR loads: the wait below names an exact count
  if constexpr (TPW > 0) {
    static_assert(NIT == 0 || (NIT >= UNR && NIT % UNR == 0), "slot u = iteration u of every tile");
    gemv_for<UNR>([&](auto U) { gemv_for<NR>([&](auto J) { gemv_ring_load<U.value>(ring[J.value][U.value], wp[J.value], voff); }); });
  } else {
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int j = 0; j < NR; ++j) ring[j][u] = u < nit ? wload(wp[j], u) : __builtin_nontemporal_load((const u32x4*)wp[j]);
  }
  GTR(1);
  asm volatile("s_waitcnt vmcnt(%3)" : "+v"(x0), "+v"(ge0v), "+v"(ge1v) : "n"(UNR * NR));
  if (skipv) return;
  const float4 ge0 = __builtin_bit_cast(float4, ge0v), ge1 = __builtin_bit_cast(float4, ge1v);
  const bf16_t* xg = (const bf16_t*)a.x;
  const int iloop = i0 + NTH * 8;
  if (a.norm_w) {
    float ss = 0.f;
    if (i0 < K) ss = gemv_sumsq8(x0, ss);
    for (int i = iloop; i < K; i += NTH * 8) ss = gemv_sumsq8(*(const u32x4*)(xg + i), ss);
    const float rstd = gemv_rms_rstd<NWV>(ss, red, K, a.eps);
    if (i0 < Kpad) *(u32x4*)(xs + i0) = i0 < K ? gemv_rmsnorm8(x0, rstd, ge0, ge1) : u32x4{0, 0, 0, 0};
    for (int i = iloop; i < Kpad; i += NTH * 8) {
      u32x4 o = {0, 0, 0, 0};
      if (i < K) o = gemv_rmsnorm8(*(const u32x4*)(xg + i), rstd, *(const float4*)(a.norm_w + i), *(const float4*)(a.norm_w + i + 4));
      *(u32x4*)(xs + i) = o;
    }
  } else {
    if (i0 < Kpad) *(u32x4*)(xs + i0) = i0 < K ? x0 : u32x4{0, 0, 0, 0};
    for (int i = iloop; i < Kpad; i += NTH * 8) {
      u32x4 v = {0, 0, 0, 0};
      if (i < K) v = *(const u32x4*)(xg + i);
      *(u32x4*)(xs + i) = v;
    }
  }
  __syncthreads();
  GTR(2);

  // ---- the tiles: consume a ring slot, refill it UNR iterations ahead - in this tile's rows, else in the next tile's
  float acc[NR];
  const char* wn[NR];
  // the epilogue of tile t (gemv_kernel's), run with the next tile's ring in flight; then the next tile's rows become current
  auto finish = [&](int t) {
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[j] = wave_sum(acc[j]);
    if (t < 4) GTR(3 + t);
    if (lane == 0) {
      const int ob = (blockIdx.x + t * gridDim.x) * TILE + wave * RW;
#pragma unroll
      for (int j = 0; j < RW; ++j) {
        const int o = ob + j;
        if (2 * o >= a.N) continue;
        const float r = gemv_swiglu_value(acc[j], acc[j + RW], a.round_bf16);
        if (a.y16) ((bf16_t*)a.y16)[o] = f2bf(r);
        if (a.y32) a.y32[o] = r;
      }
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) wp[j] = wn[j];
  };
  if constexpr (TPW > 0) {
    // Loads complete in order and every consumed slot is refilled at once, so NR * UNR loads are in flight in front of every
    // consume and its load is the oldest: the wait leaves the NR * UNR - 1 younger ones.  In the last UNR iterations of the last
    // tile nothing is refilled and the count falls by one per consume.  (The epilogue's stores move the same counter; a store
    // younger than the load waited for only makes the wait take one more of the oldest loads with it.)  The lane's piece of x is
    // read from LDS one iteration ahead: the asm statements are compiler barriers, the read would otherwise sit in front of its use.
    u32x4 xv = *(const u32x4*)(xs + lane * 8);
    gemv_for<TPW>([&](auto T) {
      constexpr int t = decltype(T)::value;
      constexpr bool has_next = t + 1 < TPW;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        acc[j] = 0.f;
        wn[j] = has_next ? row_ptr(t + 1, j) : wp[j];
      }
      gemv_for<NIT>([&](auto IT) {
        constexpr int it = decltype(IT)::value, u = it % UNR;
        constexpr bool refill = it + UNR < NIT || has_next;
        const u32x4 xn = *(const u32x4*)(xs + (((it + 1) % NIT) * 64 + lane) * 8);
        gemv_for<NR>([&](auto J) {
          constexpr int j = decltype(J)::value;
          constexpr int younger = refill ? NR * UNR - 1 : NR * UNR - 1 - ((it - (NIT - UNR)) * NR + j);
          asm volatile("s_waitcnt vmcnt(%1)" : "+v"(ring[j][u]) : "n"(younger) : "memory");
          acc[j] = dot8(ring[j][u], xv, acc[j]);
          if constexpr (it + UNR < NIT) gemv_ring_load<it + UNR>(ring[j][u], wp[j], voff);
          else if constexpr (has_next) gemv_ring_load<u>(ring[j][u], wn[j], voff);
        });
        xv = xn;
      });
      finish(t);
    });
  } else {
    const int ntiles = (a.N / 2 + TILE - 1) / TILE;
    const int ntl = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // >= 1: the grid is <= ntiles
    for (int t = 0; t < ntl; ++t) {
      const bool has_next = t + 1 < ntl;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        acc[j] = 0.f;
        wn[j] = has_next ? row_ptr(t + 1, j) : wp[j];
      }
      for (int it0 = 0; it0 < nit; it0 += UNR) {
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int it = it0 + u;
          if (it < nit) {
            const u32x4 xv = *(const u32x4*)(xs + (it * 64 + lane) * 8);
#pragma unroll
            for (int j = 0; j < NR; ++j) {
              acc[j] = dot8(ring[j][u], xv, acc[j]);
              const bool own = it + UNR < nit;   // else the next tile's iteration u (u = it % UNR < nit)
              if (own || has_next) ring[j][u] = wload(own ? wp[j] : wn[j], own ? it + UNR : u);
            }
          }
        }
      }
      finish(t);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Straight-line form of gemv_kernel<1, false, 16> for bf16 weights and a long K (down_proj of the decode step, K = 14336; DESIGN.md
// section 5): one row per wave, 16 waves per workgroup, K = NIT * 512 a compile-time count, no RMSNorm, no x_delta, no lm_head mode.
// gemv_kernel's K loop refills a slot under a run-time test, and for that source the compiler lands every refill in a temporary
// and waits for it - vmcnt(0) - before the next consume: the ring drains in every iteration.  Here the NIT iterations are
// straight-line code and the ring is HAND-COUNTED, as gemv_resident_kernel's: every consume sits behind a wait that names the
// UNR - 1 younger loads, and the freed slot is refilled at once, so UNR loads per lane stay in flight until the last UNR iterations.
// Both of the thread's pieces of x are requested BEFORE the ring (gemv_kernel requests the second behind it: loads return in order,
// so its LDS write, the barrier and the first consume waited for the whole first ring).
// Per output the arithmetic is gemv_kernel's, statement for statement: the lane-to-K assignment, the iteration order, dot8,
// wave_sum, the roundings around the residual add - identical bits.  A workgroup depends on nothing another workgroup does.
// ---------------------------------------------------------------------------------------------
template <int NIT, int UNR>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) void gemv_stream_kernel(const usdm_gemv_args a) {
  constexpr int NWV = 16, NTH = NWV * 64, K = NIT * 512;
  static_assert(NIT >= UNR && UNR >= 1 && K <= 2 * NTH * 8, "a full first ring; a thread stages at most two pieces of x");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = (bf16_t*)smem;  // [K] bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int skipv = a.skip ? *a.skip : 0;   // requested now, tested once the first ring is in flight
  GTR(0);
  const int ob = blockIdx.x * NWV + wave;   // this wave's output (rows past N re-read the last row, never stored)
  const int urow = min((int)blockIdx.x * NWV + __builtin_amdgcn_readfirstlane(wave), a.N - 1);   // wave-uniform: a scalar row base
  const char* wp = (const char*)((const bf16_t*)a.W + (int64_t)urow * a.ldw);
  const unsigned voff = lane * 16;          // this lane's 16 bytes of a K iteration (512 elements = 1024 bytes)
  // ---- prologue.  The residual value as gemv_kernel requests it: unconditional, the weight row as a dummy address without one.
  const bf16_t* rbase = a.residual ? (const bf16_t*)a.residual : (const bf16_t*)a.W;
  const unsigned short resraw = rbase[min(ob, a.N - 1)];
  // Both pieces of x, hand-counted and unconditional (the second with a clamped index; written to LDS only where inside K)
  const int i0 = tid * 8, i1 = i0 + NTH * 8;
  u32x4 x0, x1;
  gemv_load16(x0, (const bf16_t*)a.x + min(i0, K - 8));
  gemv_load16(x1, (const bf16_t*)a.x + min(i1, K - 8));
  u32x4 ring[UNR];   // always UNR loads: the wait below names an exact count
  gemv_for<UNR>([&](auto U) { gemv_ring_load<U.value>(ring[U.value], wp, voff); });
  GTR(1);
  // in-order completion: x has landed, the ring stays in flight.  (The skip word is an operand so that its test, and with it the
  // wait for its scalar load, stays behind the ring's issue.)
  asm volatile("s_waitcnt vmcnt(%3)" : "+v"(x0), "+v"(x1), "+s"(skipv) : "n"(UNR));
  if (skipv) return;
  if (i0 < K) *(u32x4*)(xs + i0) = x0;
  if (i1 < K) *(u32x4*)(xs + i1) = x1;
  __syncthreads();
  GTR(2);

  // ---- stream: NIT iterations, straight-line.  The consumed slot's load is the oldest of the UNR in flight: the wait leaves the
  // UNR - 1 younger ones; in the last UNR iterations nothing is refilled and the count falls by one per consume.  The lane's piece
  // of x is read from LDS one iteration ahead (the asm statements are compiler barriers: the read would sit in front of its use).
  float acc = 0.f;
  u32x4 xv = *(const u32x4*)(xs + lane * 8);
  gemv_for<NIT>([&](auto IT) {
    constexpr int it = decltype(IT)::value, u = it % UNR;
    constexpr int younger = it + UNR < NIT ? UNR - 1 : NIT - 1 - it;
    const u32x4 xn = *(const u32x4*)(xs + (((it + 1) % NIT) * 64 + lane) * 8);
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(ring[u]) : "n"(younger) : "memory");
    acc = dot8(ring[u], xv, acc);
    if constexpr (it + UNR < NIT) gemv_ring_load<it + UNR>(ring[u], wp, voff);
    xv = xn;
  });
  acc = wave_sum(acc);
  GTR(3);

  // ---- epilogue (gemv_kernel's plain form)
  if (lane != 0 || ob >= a.N) return;
  const float v = gemv_plain_value(acc, a.round_bf16, a.residual != nullptr, [&] { return bf2f(resraw); });
  if (a.y16) ((bf16_t*)a.y16)[ob] = f2bf(v);
  if (a.y32) a.y32[ob] = v;
}

// ---------------------------------------------------------------------------------------------
// gemv_stream_kernel over the lossless 13-bit image of the weights (usdm_gemv_wpack; gemv_common.h): the same grid, waves, rows,
// prologue and epilogue, 13/16 of the bytes.  The ring holds RU units (a unit = four K iterations = four loads, 52 bytes per lane)
// instead of 16-byte slots; a unit is consumed behind a wait that names the 4 * (RU - 1) younger loads, rebuilt piece by piece
// into the bf16 pairs the bf16 kernel loads (gemv_wpack8) and refilled at once.  acc sees the same values in the same order:
// identical bits.
// A row the packer marked (a weight outside the 16-exponent window) streams from the bf16 matrix: a wave-uniform branch on the
// row's flag, taken before any ring load is issued, into gemv_stream_kernel's text with a ring of UB slots.  (The text is
// repeated here, not shared: gemv_stream_kernel's device code stays what it is.)  UB is deeper than that kernel's ring because
// the marked row is 16/13 as long as its neighbours' and ends the launch if it falls behind them.  The two paths meet at wave_sum;
// each has its own counted wait, skip return, x staging and barrier, so no branch sits around a load that a counted wait covers.
// (The compiler merges the paths' returns and the epilogue into blocks entered under constant flags: tools/check_mfma_asm.py
// audit_paths follows them.)
// ---------------------------------------------------------------------------------------------
template <int NIT, int RU, int UB>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) void gemv_stream_wpack_kernel(const usdm_gemv_args a,
                                                                                                        const usdm_gemv_wpack p) {
  constexpr int NWV = 16, NTH = NWV * 64, K = NIT * 512, NU = NIT / 4;
  static_assert(NIT % 4 == 0 && NU >= RU && RU >= 1 && NIT >= UB && UB >= 1 && K <= 2 * NTH * 8, "whole units; a full first ring");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = (bf16_t*)smem;  // [K] bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int skipv = a.skip ? *a.skip : 0;   // requested now, tested once the first ring is in flight
  const int ob = blockIdx.x * NWV + wave;
  const int urow = min((int)blockIdx.x * NWV + __builtin_amdgcn_readfirstlane(wave), a.N - 1);   // wave-uniform
  // Is the row marked?  Read from the kernel arguments (a scalar load like every other argument), not from rowflag: the first
  // memory access of a launch is its longest, and this test stands in front of the first weight load.
  const bool marked = (p.marked[urow >> 5] >> (urow & 31)) & 1u;
  const unsigned voff = lane * 16;
  const bf16_t* rbase = a.residual ? (const bf16_t*)a.residual : (const bf16_t*)a.W;
  const unsigned short resraw = rbase[min(ob, a.N - 1)];
  const int i0 = tid * 8, i1 = i0 + NTH * 8;
  const bf16_t* xp0 = (const bf16_t*)a.x + min(i0, K - 8);
  const bf16_t* xp1 = (const bf16_t*)a.x + min(i1, K - 8);
  float acc = 0.f;
  // (both pieces of x are requested inside the paths: requested in front of the branch, the two counted waits that name them made
  // the compiler copy their registers while the loads were in flight)
  if (marked) {
    // ---- a marked row: gemv_stream_kernel<NIT, UB>'s text
    const char* wp = (const char*)((const bf16_t*)a.W + (int64_t)urow * a.ldw);
    u32x4 x0, x1;
    gemv_load16(x0, xp0);
    gemv_load16(x1, xp1);
    u32x4 ring[UB];
    gemv_for<UB>([&](auto U) { gemv_ring_load<U.value>(ring[U.value], wp, voff); });
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(x0), "+v"(x1), "+s"(skipv) : "n"(UB));
    if (skipv) return;
    if (i0 < K) *(u32x4*)(xs + i0) = x0;
    if (i1 < K) *(u32x4*)(xs + i1) = x1;
    __syncthreads();
    u32x4 xv = *(const u32x4*)(xs + lane * 8);
    gemv_for<NIT>([&](auto IT) {
      constexpr int it = decltype(IT)::value, u = it % UB;
      constexpr int younger = it + UB < NIT ? UB - 1 : NIT - 1 - it;
      const u32x4 xn = *(const u32x4*)(xs + (((it + 1) % NIT) * 64 + lane) * 8);
      asm volatile("s_waitcnt vmcnt(%1)" : "+v"(ring[u]) : "n"(younger) : "memory");
      acc = dot8(ring[u], xv, acc);
      if constexpr (it + UB < NIT) gemv_ring_load<it + UB>(ring[u], wp, voff);
      xv = xn;
    });
  } else {
    // ---- the packed row: RU units in flight
    const char* pp = (const char*)p.planes + (int64_t)urow * p.stride;
    const unsigned base4 = (unsigned)p.base * 0x01010101u;
    u32x4 x0, x1;
    gemv_load16(x0, xp0);
    gemv_load16(x1, xp1);
    gemv_wunit ring[RU];
    gemv_for<RU>([&](auto U) { gemv_unit_load<U.value>(ring[U.value], pp, voff); });
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(x0), "+v"(x1), "+s"(skipv) : "n"(4 * RU));
    if (skipv) return;
    if (i0 < K) *(u32x4*)(xs + i0) = x0;
    if (i1 < K) *(u32x4*)(xs + i1) = x1;
    __syncthreads();
    // the consumed unit's four loads are the oldest of the 4 * RU in flight; in the last RU units nothing is refilled and the
    // count falls by four per consume.  x is read from LDS one iteration ahead, as in the bf16 loop.
    u32x4 xv = *(const u32x4*)(xs + lane * 8);
    gemv_for<NU>([&](auto UI) {
      constexpr int un = decltype(UI)::value, s = un % RU;
      constexpr int younger = un + RU < NU ? 4 * (RU - 1) : 4 * (NU - 1 - un);
      gemv_wunit& r = ring[s];
      asm volatile("s_waitcnt vmcnt(%4)" : "+v"(r.la), "+v"(r.lb), "+v"(r.nib), "+v"(r.sgn) : "n"(younger) : "memory");
      gemv_for<4>([&](auto PI) {
        constexpr int P = decltype(PI)::value, it = 4 * un + P;
        const u32x4 xn = *(const u32x4*)(xs + (((it + 1) % NIT) * 64 + lane) * 8);
        const u32x4& lo = P < 2 ? r.la : r.lb;
        acc = dot8(gemv_wpack8<P>(lo[2 * (P & 1)], lo[2 * (P & 1) + 1], r.nib[P], r.sgn, base4), xv, acc);
        xv = xn;
      });
      if constexpr (un + RU < NU) gemv_unit_load<un + RU>(r, pp, voff);
    });
  }
  acc = wave_sum(acc);

  // ---- epilogue (gemv_kernel's plain form)
  if (lane != 0 || ob >= a.N) return;
  const float v = gemv_plain_value(acc, a.round_bf16, a.residual != nullptr, [&] { return bf2f(resraw); });
  if (a.y16) ((bf16_t*)a.y16)[ob] = f2bf(v);
  if (a.y32) a.y32[ob] = v;
}

// ---------------------------------------------------------------------------------------------
// gemv_resident_kernel<2, 7, 2, 8> (gate/up of the 7B: two tiles per workgroup, K = 4096) over the lossless 13-bit image of the
// interleaved gate/up matrix: the same grid, tile-to-workgroup assignment, rows (gemv_glu_row), prologue and epilogue, 13/16 of
// the bytes.  A row is two units (gemv_unit_load); a wave's 2 tiles x 2 units x 4 rows are ONE straight-line sequence of 16 units,
// unit s = (tile, unit of the row, row) in that order, so that acc[j] sees its row's iterations 0..7 in order, each as
// dot8(gemv_wpack8<P>(...), the x piece of the iteration, acc[j]) - identical bits - and the four rows of a step share the four x
// pieces of its iterations (16 VGPRs, replaced piece by piece under the step's last row).  The ring holds RU units, hand-counted:
// a unit is consumed behind a wait that names the 4 * (RU - 1) younger loads and its slot is refilled at once with unit s + RU,
// which in the last RU units of tile 0 is a unit of tile 1 - the ring does not drain at the seam and the epilogue of tile 0 runs
// with tile 1's units in flight.  In the last RU units nothing is refilled and the count falls by four per consume.
// The image's marked bit o says that the gate row or the up row of OUTPUT o holds a weight outside the window.  A wave whose four
// outputs (two per tile) have a bit set streams both its tiles from the bf16 matrix: a wave-uniform branch on the bits (kernel
// arguments, no memory round trip), taken before any ring load, into gemv_resident_kernel's straight-line text (repeated here, not
// shared: that kernel's device code stays what it is).  Each path has its own early loads, counted waits, skip return, x staging
// and barriers, so no branch sits around a load that a counted wait covers; the paths meet at the end of the kernel.
// ---------------------------------------------------------------------------------------------
template <int RU>
__global__ __launch_bounds__(7 * 64) __attribute__((amdgpu_waves_per_eu(4))) void gemv_resident_wpack_kernel(const usdm_gemv_args a,
                                                                                                          const usdm_gemv_wpack p) {
  constexpr int RW = 2, NWV = 7, TPW = 2, NIT = 8;
  constexpr int NTH = NWV * 64, NR = 2 * RW, TILE = NWV * RW;
  constexpr int UNR = gemv_ring_depth(NR, false, false);   // the marked waves' ring: gemv_resident_kernel's
  constexpr int NU = NIT / 4, NSEQ = TPW * NU * NR;         // units per row; units of a wave
  static_assert(RU >= 1 && RU <= NSEQ && NIT >= UNR && NIT % UNR == 0, "a full first ring; slot u = iteration u of every tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = (bf16_t*)smem;  // [K] bf16
  __shared__ float red[NWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int skipv = a.skip ? *a.skip : 0;
  const int K = a.K;           // NIT * 512 (the launcher)
  const int Kpad = (K + 511) & ~511;
  const int uwave = __builtin_amdgcn_readfirstlane(wave);   // the row bases are wave-uniform: scalar registers, one lane offset
  // weight row j of this wave in tile t (rows past N re-read the last row, never stored)
  auto row_of = [&](int t, int j) -> int {
    const int r = gemv_glu_row((blockIdx.x + t * gridDim.x) * TILE + uwave * RW + (j % RW), j >= RW);
    return r < a.N ? r : a.N - 1;
  };
  // Is one of the wave's outputs marked?  Its two outputs of a tile are an even / odd pair: two neighbouring bits of one word.
  unsigned mk = 0u;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int o = (blockIdx.x + t * gridDim.x) * TILE + uwave * RW;
    if (2 * o < a.N) mk |= (p.marked[o >> 5] >> (o & 31)) & 3u;
  }
  const unsigned voff = lane * 16;
  const int i0 = tid * 8;
  // x into LDS, RMS-normalised where asked (gemv_resident_kernel's staging), once per workgroup, under the first ring
  auto stage = [&](u32x4 x0, u32x4 ge0v, u32x4 ge1v) {
    const float4 ge0 = __builtin_bit_cast(float4, ge0v), ge1 = __builtin_bit_cast(float4, ge1v);
    const bf16_t* xg = (const bf16_t*)a.x;
    const int iloop = i0 + NTH * 8;
    if (a.norm_w) {
      float ss = 0.f;
      if (i0 < K) ss = gemv_sumsq8(x0, ss);
      for (int i = iloop; i < K; i += NTH * 8) ss = gemv_sumsq8(*(const u32x4*)(xg + i), ss);
      const float rstd = gemv_rms_rstd<NWV>(ss, red, K, a.eps);
      if (i0 < Kpad) *(u32x4*)(xs + i0) = i0 < K ? gemv_rmsnorm8(x0, rstd, ge0, ge1) : u32x4{0, 0, 0, 0};
      for (int i = iloop; i < Kpad; i += NTH * 8) {
        u32x4 o = {0, 0, 0, 0};
        if (i < K) o = gemv_rmsnorm8(*(const u32x4*)(xg + i), rstd, *(const float4*)(a.norm_w + i), *(const float4*)(a.norm_w + i + 4));
        *(u32x4*)(xs + i) = o;
      }
    } else {
      if (i0 < Kpad) *(u32x4*)(xs + i0) = i0 < K ? x0 : u32x4{0, 0, 0, 0};
      for (int i = iloop; i < Kpad; i += NTH * 8) {
        u32x4 v = {0, 0, 0, 0};
        if (i < K) v = *(const u32x4*)(xg + i);
        *(u32x4*)(xs + i) = v;
      }
    }
    __syncthreads();
  };
  // the epilogue of tile t (gemv_resident_kernel's), run with the next tile's ring in flight
  auto finish = [&](int t, float (&acc)[NR]) {
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[j] = wave_sum(acc[j]);
    if (lane == 0) {
      const int ob = (blockIdx.x + t * gridDim.x) * TILE + wave * RW;
#pragma unroll
      for (int j = 0; j < RW; ++j) {
        const int o = ob + j;
        if (2 * o >= a.N) continue;
        const float r = gemv_swiglu_value(acc[j], acc[j + RW], a.round_bf16);
        if (a.y16) ((bf16_t*)a.y16)[o] = f2bf(r);
        if (a.y32) a.y32[o] = r;
      }
    }
  };
  float acc[NR];
  if (mk) {
    // ---- a marked wave: gemv_resident_kernel<2, 7, 2, 8>'s text over the bf16 rows of both tiles
    const char* wp[NR];
    const char* wn[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) wp[j] = (const char*)((const bf16_t*)a.W + (int64_t)row_of(0, j) * a.ldw);
    u32x4 x0 = {0u, 0u, 0u, 0u}, ge0v = x0, ge1v = x0;
    gemv_early_loads(a, i0, K, x0, ge0v, ge1v);
    u32x4 ring[NR][UNR];
    gemv_for<UNR>([&](auto U) { gemv_for<NR>([&](auto J) { gemv_ring_load<U.value>(ring[J.value][U.value], wp[J.value], voff); }); });
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(x0), "+v"(ge0v), "+v"(ge1v) : "n"(UNR * NR));
    if (skipv) return;
    stage(x0, ge0v, ge1v);
    u32x4 xv = *(const u32x4*)(xs + lane * 8);
    gemv_for<TPW>([&](auto T) {
      constexpr int t = decltype(T)::value;
      constexpr bool has_next = t + 1 < TPW;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        acc[j] = 0.f;
        wn[j] = has_next ? (const char*)((const bf16_t*)a.W + (int64_t)row_of(t + 1, j) * a.ldw) : wp[j];
      }
      gemv_for<NIT>([&](auto IT) {
        constexpr int it = decltype(IT)::value, u = it % UNR;
        constexpr bool refill = it + UNR < NIT || has_next;
        const u32x4 xn = *(const u32x4*)(xs + (((it + 1) % NIT) * 64 + lane) * 8);
        gemv_for<NR>([&](auto J) {
          constexpr int j = decltype(J)::value;
          constexpr int younger = refill ? NR * UNR - 1 : NR * UNR - 1 - ((it - (NIT - UNR)) * NR + j);
          asm volatile("s_waitcnt vmcnt(%1)" : "+v"(ring[j][u]) : "n"(younger) : "memory");
          acc[j] = dot8(ring[j][u], xv, acc[j]);
          if constexpr (it + UNR < NIT) gemv_ring_load<it + UNR>(ring[j][u], wp[j], voff);
          else if constexpr (has_next) gemv_ring_load<u>(ring[j][u], wn[j], voff);
        });
        xv = xn;
      });
      finish(t, acc);
#pragma unroll
      for (int j = 0; j < NR; ++j) wp[j] = wn[j];
    });
  } else {
    // ---- the packed rows: RU units in flight, unit s = row s % NR, unit (s / NR) % NU of the row, tile s / (NR * NU)
    const char* pp[TPW][NR];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int j = 0; j < NR; ++j) pp[t][j] = (const char*)p.planes + (int64_t)row_of(t, j) * p.stride;
    const unsigned base4 = (unsigned)p.base * 0x01010101u;
    u32x4 x0 = {0u, 0u, 0u, 0u}, ge0v = x0, ge1v = x0;
    gemv_early_loads(a, i0, K, x0, ge0v, ge1v);
    gemv_wunit ring[RU];
    gemv_for<RU>([&](auto S) {
      constexpr int s = decltype(S)::value;
      gemv_unit_load<(s / NR) % NU>(ring[s], pp[s / (NR * NU)][s % NR], voff);
    });
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(x0), "+v"(ge0v), "+v"(ge1v) : "n"(4 * RU));
    if (skipv) return;
    stage(x0, ge0v, ge1v);
    // the lane's x pieces of the step's four iterations; under the step's last row each is replaced, once used, by the piece of
    // the next step (the asm statements are compiler barriers: read in front of the next step they would wait there)
    u32x4 xq[4];
#pragma unroll
    for (int P = 0; P < 4; ++P) xq[P] = *(const u32x4*)(xs + (P * 64 + lane) * 8);
    gemv_for<TPW>([&](auto T) {
      constexpr int t = decltype(T)::value;
#pragma unroll
      for (int j = 0; j < NR; ++j) acc[j] = 0.f;
      gemv_for<NU>([&](auto UI) {
        constexpr int un = decltype(UI)::value;
        gemv_for<NR>([&](auto J) {
          constexpr int j = decltype(J)::value, s = (t * NU + un) * NR + j, s2 = s + RU;
          constexpr int younger = s2 < NSEQ ? 4 * (RU - 1) : 4 * (NSEQ - 1 - s);
          gemv_wunit& r = ring[s % RU];
          asm volatile("s_waitcnt vmcnt(%4)" : "+v"(r.la), "+v"(r.lb), "+v"(r.nib), "+v"(r.sgn) : "n"(younger) : "memory");
          gemv_for<4>([&](auto PI) {
            constexpr int P = decltype(PI)::value;
            const u32x4& lo = P < 2 ? r.la : r.lb;
            acc[j] = dot8(gemv_wpack8<P>(lo[2 * (P & 1)], lo[2 * (P & 1) + 1], r.nib[P], r.sgn, base4), xq[P], acc[j]);
            if constexpr (j == NR - 1) xq[P] = *(const u32x4*)(xs + ((4 * ((un + 1) % NU) + P) * 64 + lane) * 8);
          });
          if constexpr (s2 < NSEQ) gemv_unit_load<(s2 / NR) % NU>(r, pp[s2 / (NR * NU)][s2 % NR], voff);
        });
      });
      finish(t, acc);
    });
  }
}

// final arg-max over the per-block partials; advances the device-side decode state
// (nseg segments of nparts partials per sequence, seg_stride apart: the tensor-parallel batched step gathers [rank][sequence][nparts])
__global__ void argmax_final_kernel(const float* pv, const int* pi, int nparts, int nseg, int64_t seg_stride, usdm_decode_state st,
                                    const bf16_t* E, int Hd, bf16_t* h_out) {
  __shared__ float sv[256];
  __shared__ int si[256];
  __shared__ int s_tok;
  const int b = blockIdx.x;   // sequence of a batched step (grid = 1 when single)
  if (st.done && st.done[b]) return;
  pv += (int64_t)b * nparts; pi += (int64_t)b * nparts;
  float bv = -INFINITY;
  int bi = PICK_NO_ID;
  for (int sg = 0; sg < nseg; ++sg)
    for (int i = threadIdx.x; i < nparts; i += 256) {
      const float v = pv[sg * seg_stride + i];
      const int id = pi[sg * seg_stride + i];
      if (pick_better(v, id, bv, bi)) { bv = v; bi = id; }
    }
  pick_block_best<256>(sv, si, bv, bi);
  if (threadIdx.x == 0) {
    // every id banned (no candidate anywhere): fall back to id 0 so that nothing indexes the embedding table out of range
    const int tok = (si[0] == PICK_NO_ID ? 0 : si[0]) + st.id_offset;
    pick_commit(st, b, st.step[b], tok);
    s_tok = tok;
  }
  if (E) {  // fused nn.Embedding lookup of the token the next decode step consumes
    __syncthreads();
    pick_embed_row<256>(E, s_tok, Hd, h_out + (int64_t)b * Hd);
  }
}

// h[0:Hd] = E[token] (bf16 row copy)  — nn.Embedding of HF MistralModel
__global__ void embed_kernel(const bf16_t* E, const int64_t* ids, const int* next_token, int n, int Hd, bf16_t* out) {
  const int r = blockIdx.x;
  const int64_t id = ids ? ids[r] : (int64_t)(*next_token);
  const u32x4* src = (const u32x4*)(E + id * Hd);
  u32x4* dst = (u32x4*)(out + (int64_t)r * Hd);
  for (int i = threadIdx.x; i < Hd / 8; i += blockDim.x) dst[i] = src[i];
}

// h = bf16(h + bf16(delta))  — residual add after a tensor-parallel all-reduce of fp32 partial sums
__global__ void residual_add_kernel(bf16_t* h, const float* delta, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) h[i] = f2bf(bf2f(h[i]) + round_bf(delta[i]));
}
}  // namespace

// Workgroups of `kern` the current device holds at once (the occupancy query x its CUs), remembered for the last kernel, device
// and LDS size asked about (WHO: one memory per asker, so that the bf16 and the packed gate/up launches of a step keep theirs)
template <int WHO = 0>
static int gemv_resident_count(const void* kern, int nth, size_t lds, int* out) {
  static thread_local const void* c_kern = nullptr;
  static thread_local int c_dev = -1, c_n = 0;
  static thread_local size_t c_lds = 0;
  int dev = 0;
  USDM_HIP(hipGetDevice(&dev));
  if (kern != c_kern || dev != c_dev || lds != c_lds) {
    int ncu = 0, per = 0;
    USDM_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    USDM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, nth, lds));
    USDM_CHECK_ARG(ncu > 0 && per > 0, "usdm_gemv: the resident form does not fit a CU (%zu bytes of LDS)", lds);
    c_kern = kern; c_dev = dev; c_lds = lds; c_n = ncu * per;
  }
  *out = c_n;
  return 0;
}

// Where the selection's (2, GLU, 7) row runs in its STRAIGHT-LINE resident form: two tiles on every workgroup of `grid`, K = 4096,
// no x_delta.  The one statement of that choice: gemv_launch_resident reads it for the bf16 kernel, gemv_packed_glu_grid for the
// packed one.
static bool gemv_straight_form(const usdm_gemv_args& a, int ntiles, int grid) {
  return !a.x_delta && a.K == 8 * 512 && ntiles == 2 * grid;
}

// The resident form of the selection's (2, GLU, 7) row: *launched = false where one tile per workgroup is all there is to run
// (every tile already resident, or x_delta) and the one-tile kernel takes the launch.
static int gemv_launch_resident(const usdm_gemv_args& a, const gemv_sel& s, size_t lds, hipStream_t st, bool* launched) {
  *launched = false;
  if (a.x_delta) return 0;
  constexpr int RW = 2, NWV = 7;
  auto straight = gemv_resident_kernel<RW, NWV, 2, 8>;   // gate/up of the 7B: two tiles per workgroup, K = 4096
  auto generic = gemv_resident_kernel<RW, NWV, 0, 0>;
  const int ntiles = s.grid;
  int n = 0;
  if (int rc = gemv_resident_count((const void*)straight, NWV * 64, lds, &n)) return rc;
  int grid = min(min(n, s.res), ntiles);
  if (grid == ntiles) return 0;
  if (gemv_straight_form(a, ntiles, grid)) {
    hipLaunchKernelGGL(straight, dim3(grid), dim3(NWV * 64), lds, st, a);
  } else {
    if (int rc = gemv_resident_count((const void*)generic, NWV * 64, lds, &n)) return rc;
    grid = min(min(n, s.res), ntiles);
    if (grid == ntiles) return 0;
    hipLaunchKernelGGL(generic, dim3(grid), dim3(NWV * 64), lds, st, a);
  }
  *launched = true;
  USDM_LAUNCH_CHECK();
  return 0;
}

// Launches the instantiation gemv_select names.  One selection for every weight format, so an FP8 or MXFP4 launch partitions K and
// the RMSNorm sums exactly as the bf16 launch of the same shape.  FORM: GEMV_PLAIN (no merged input, no peer-to-peer epilogue:
// the only form of the FP8 / MXFP4 weights), GEMV_MRG or GEMV_CMB, with the kernel's MRG / P2P / CMB flags.
template <int FORM, bool MRG, bool P2P, bool CMB, bool FP8, class... FMT>
static int gemv_launch(const usdm_gemv_args& a, hipStream_t st, FMT... fmt) {
  const size_t lds = (size_t)((a.K + 511) & ~511) * 2;
  const gemv_sel s = gemv_select(a, false);
  if constexpr (FORM == GEMV_PLAIN && !FP8 && sizeof...(FMT) == 0) {
    if (s.stream) {   // K = 14336 = 28 iterations (gemv_select)
      hipLaunchKernelGGL((gemv_stream_kernel<28, USDM_GEMV_DOWN_UNR>), dim3(s.grid), dim3(1024), lds, st, a);
      USDM_LAUNCH_CHECK();
      return 0;
    }
    if (s.res > 0) {
      bool launched = false;
      if (int rc = gemv_launch_resident(a, s, lds, st, &launched)) return rc;
      if (launched) return 0;
    }
  }
  const bool found = gemv_dispatch<FORM>(s, [&](auto RW, auto GLU, auto NWV) {
    constexpr int nwv = decltype(NWV)::value;
    hipLaunchKernelGGL((gemv_kernel<decltype(RW)::value, decltype(GLU)::value != 0, nwv, MRG, P2P, CMB, FP8, FMT...>), dim3(s.grid),
                       dim3(nwv * 64), lds, st, a, fmt...);
  });
  if (!found) return gemv_no_instantiation(s);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_gemv(const usdm_gemv_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->W && (pa->x || pa->mrg_po), "usdm_gemv: null args");
  const usdm_gemv_args& a = *pa;
  if (int rc = gemv_check_shape("usdm_gemv", a, "input vector")) return rc;
  if (int rc = gemv_check_outputs("usdm_gemv", a)) return rc;
  const bool glu = a.act == USDM_ACT_SWIGLU;
  USDM_CHECK_ARG(!a.norm_w || a.K % 8 == 0, "usdm_gemv: K");
  USDM_CHECK_ARG(!a.x_out || (a.x_delta && a.x_out != a.x), "usdm_gemv: x_out needs x_delta and must not alias x");
  USDM_CHECK_ARG(!a.mrg_po || (a.mrg_pm && a.mrg_pl && a.mrg_ns >= 1 && a.mrg_ns <= 64 && a.K % 128 == 0 && !a.norm_w && !a.x_delta),
                 "usdm_gemv: merged-attention input needs pm/pl/po, 1 <= splits <= 64, K a multiple of 128, no norm / x_delta");
  USDM_CHECK_ARG(a.p2p_mode >= 0 && a.p2p_mode <= 2, "usdm_gemv: p2p_mode");
  USDM_CHECK_ARG(!a.p2p_mode || (a.p2p && a.p2p_site >= 0 && a.act == USDM_ACT_NONE && !a.part_val && a.residual && a.y16),
                 "usdm_gemv: the fused all-reduce needs a plain row-parallel projection with residual + y16");
  // (its LDS scratch, 9 x rows-per-workgroup floats <= 864 B, reuses the x staging area: Kpad * 2 >= 1024 B always)
  const int nout = glu ? a.N / 2 : a.N;
  hipStream_t st = (hipStream_t)stream;
  if (a.cmb_gran) {   // hand-off form of the merged-attention input
    USDM_CHECK_ARG(a.mrg_po && a.mrg_pm && a.mrg_pl && a.mrg_ns >= 1 && a.mrg_ns <= 64 && !a.p2p_mode && !glu && !a.part_val && !a.norm_w && !a.x_delta &&
                       nout % 256 == 0 && nout / 256 == 16 && a.K % 128 == 0 && a.K / 128 <= 256,
                   "usdm_gemv: cmb_gran needs the mrg_* partials, a plain 4096-output projection and K / 128 <= 256 heads");
    return gemv_launch<GEMV_CMB, false, false, true, false>(a, st);
  }
  if (a.mrg_po || a.p2p_mode) {   // o_proj with the attention merge in its prologue and / or a row-parallel projection with the
    // peer-to-peer all-reduce in its epilogue
    USDM_CHECK_ARG(!glu && !a.part_val, "usdm_gemv: merged-attention input / fused all-reduce are for plain projections");
    if (a.mrg_po && a.p2p_mode) return gemv_launch<GEMV_MRG, true, true, false, false>(a, st);
    if (a.mrg_po) return gemv_launch<GEMV_MRG, true, false, false, false>(a, st);
    return gemv_launch<GEMV_MRG, false, true, false, false>(a, st);
  }
  return gemv_launch<GEMV_PLAIN, false, false, false, false>(a, st);
}

// 1 where usdm_gemv_packed streams the 13-bit image: where gemv_select names the straight-line form (a plain bf16 call, K = 14336)
extern "C" int usdm_gemv_packs(const usdm_gemv_args* pa) { return gemv_select(*pa, false).stream ? 1 : 0; }

extern "C" int usdm_gemv_packed(const usdm_gemv_args* pa, const usdm_gemv_wpack* pk, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->W && pa->x && pk && pk->planes && pk->rowflag, "usdm_gemv_packed: null args");
  USDM_CHECK_ARG(pa->N <= 14336, "usdm_gemv_packed: at most 14336 rows (usdm_gemv_wpack.marked)");
  if (!usdm_gemv_packs(pa)) return usdm_gemv(pa, stream);   // no packed form of this call: the bf16 kernels, the same bits
  const usdm_gemv_args& a = *pa;
  if (int rc = gemv_check_shape("usdm_gemv_packed", a, "input vector")) return rc;
  if (int rc = gemv_check_outputs("usdm_gemv_packed", a)) return rc;
  USDM_CHECK_ARG(pk->units == 7 && pk->units * 2048 == a.K && pk->stride % 16 == 0 && pk->stride >= (int64_t)pk->units * GEMV_WPACK_UNIT &&
                     pk->base >= 0 && pk->base <= 112,
                 "usdm_gemv_packed: the image must hold K / 2048 units of 3328 bytes per row, stride a multiple of 16, base 0..112");
  USDM_CHECK_ARG(((uintptr_t)pk->planes & 15) == 0 && ((uintptr_t)pk->rowflag & 3) == 0, "usdm_gemv_packed: planes must be 16-byte, rowflag 4-byte aligned");
  const gemv_sel s = gemv_select(a, false);
  hipLaunchKernelGGL((gemv_stream_wpack_kernel<28, USDM_GEMV_WPACK_RU, USDM_GEMV_WPACK_UB>), dim3(s.grid), dim3(1024), (size_t)a.K * 2,
                     (hipStream_t)stream, a, *pk);
  USDM_LAUNCH_CHECK();
  return 0;
}
// The packed gate/up form: *grid = the grid on which gemv_resident_wpack_kernel runs the call, 0 where the call has no packed form.
// That is exactly where gemv_launch_resident launches the straight-line bf16 instantiation: a plain bf16 SwiGLU call on the
// selection's resident row, in the straight-line form on the grid of the kernel that is launched (the occupancy question is asked
// about the packed kernel; what needs no device is tested first, so that every other call is answered without one).
static int gemv_packed_glu_grid(const usdm_gemv_args& a, int* grid) {
  *grid = 0;
  const gemv_sel s = gemv_select(a, false);
  if (!(s.glu && s.rw == 2 && s.nwv == 7 && s.res > 0) || a.x_out || a.K != 8 * 512 || a.x_delta) return 0;
  int n = 0;
  if (int rc = gemv_resident_count<1>((const void*)gemv_resident_wpack_kernel<USDM_GEMV_GU_WPACK_RU>, 7 * 64, (size_t)a.K * 2, &n)) return rc;
  const int g = min(min(n, s.res), s.grid);
  if (gemv_straight_form(a, s.grid, g)) *grid = g;
  return 0;
}

// 1 where usdm_gemv_packed_glu streams the 13-bit image (0 also where the device cannot be asked: such a launch fails anyway)
extern "C" int usdm_gemv_packs_glu(const usdm_gemv_args* pa) {
  int grid = 0;
  return pa && gemv_packed_glu_grid(*pa, &grid) == 0 && grid > 0 ? 1 : 0;
}

extern "C" int usdm_gemv_packed_glu(const usdm_gemv_args* pa, const usdm_gemv_wpack* pk, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->W && pa->x && pk && pk->planes && pk->rowflag, "usdm_gemv_packed_glu: null args");
  USDM_CHECK_ARG(pa->act == USDM_ACT_SWIGLU && pa->N / 2 <= 14336, "usdm_gemv_packed_glu: a SwiGLU call of at most 14336 outputs (usdm_gemv_wpack.marked)");
  const usdm_gemv_args& a = *pa;
  int grid = 0;
  if (int rc = gemv_packed_glu_grid(a, &grid)) return rc;
  if (!grid) return usdm_gemv(pa, stream);   // no packed form of this call: the bf16 kernels, the same bits
  if (int rc = gemv_check_shape("usdm_gemv_packed_glu", a, "input vector")) return rc;
  if (int rc = gemv_check_outputs("usdm_gemv_packed_glu", a)) return rc;
  USDM_CHECK_ARG(pk->units == 2 && pk->stride % 16 == 0 && pk->stride >= (int64_t)2 * GEMV_WPACK_UNIT && pk->base >= 0 && pk->base <= 112,
                 "usdm_gemv_packed_glu: the image must hold 2 units of 3328 bytes per row, stride a multiple of 16, base 0..112");
  USDM_CHECK_ARG(((uintptr_t)pk->planes & 15) == 0 && ((uintptr_t)pk->rowflag & 3) == 0,
                 "usdm_gemv_packed_glu: planes must be 16-byte, rowflag 4-byte aligned");
  hipLaunchKernelGGL((gemv_resident_wpack_kernel<USDM_GEMV_GU_WPACK_RU>), dim3(grid), dim3(7 * 64), (size_t)a.K * 2, (hipStream_t)stream, a, *pk);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_gemv_wpack(void) { return (int)sizeof(usdm_gemv_wpack); }

int usdm_gemv_fp8_batch_launch(const usdm_gemv_fp8_args* pa, hipStream_t st);   // llm_batch_k.hip: nb = 2..4

extern "C" int usdm_gemv_fp8(const usdm_gemv_fp8_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->b.g.W && pa->b.g.x && pa->row_exp, "usdm_gemv_fp8: null args");
  const usdm_gemv_args& a = pa->b.g;
  USDM_CHECK_ARG(pa->b.nb >= 1 && pa->b.nb <= 4 && (pa->b.form == 0 || pa->b.form == -1),
                 "usdm_gemv_fp8: 1..4 sequences on the VALU form (the matrix-core form has no FP8 weights)");
  USDM_CHECK_ARG(!a.p2p && !a.p2p_mode && !a.mrg_po && !a.cmb_gran && !a.x_delta && !a.x_out,
                 "usdm_gemv_fp8: p2p / merged-attention input / cmb_gran / x_delta are not supported with FP8 weights");
  USDM_CHECK_ARG(((uintptr_t)a.W & 7) == 0, "usdm_gemv_fp8: bad N/K/ldw");
  if (int rc = gemv_check_shape("usdm_gemv_fp8", a, "input vector")) return rc;
  if (int rc = gemv_check_outputs("usdm_gemv_fp8", a)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (pa->b.nb > 1) return usdm_gemv_fp8_batch_launch(pa, st);
  return gemv_launch<GEMV_PLAIN, false, false, false, true>(a, st, pa->row_exp);
}

namespace {
// prefill operand of the FP8 model: one workgroup per row, 8 elements (8 bytes in, 16 bytes out) per thread and step
__global__ __launch_bounds__(256) void dequant_fp8_kernel(const uint8_t* q, const int8_t* row_exp, int K, int64_t ldq, bf16_t* out,
                                                          int64_t ldo) {
  const int r = blockIdx.x;
  const float s = fp8_row_scale(row_exp[r]);
  const uint8_t* qr = q + (int64_t)r * ldq;
  bf16_t* orow = out + (int64_t)r * ldo;
  for (int i = threadIdx.x * 8; i < K; i += 256 * 8) {
    const u32x2 w = __builtin_nontemporal_load((const u32x2*)(qr + i));
    *(u32x4*)(orow + i) = fp8x8_to_bf16x8(w, s);
  }
}
}  // namespace

extern "C" int usdm_dequant_fp8(const void* q, const int8_t* row_exp, int32_t N, int32_t K, int64_t ldq, void* out, int64_t ldo,
                                usdm_stream_t stream) {
  USDM_CHECK_ARG(q && row_exp && out, "usdm_dequant_fp8: null args");
  USDM_CHECK_ARG(N > 0 && K > 0 && K % 8 == 0 && ldq >= K && ldq % 8 == 0 && ldo >= K && ldo % 8 == 0, "usdm_dequant_fp8: bad N/K/ldq/ldo");
  USDM_CHECK_ARG(((uintptr_t)q & 7) == 0 && ((uintptr_t)out & 15) == 0, "usdm_dequant_fp8: q must be 8-byte, out 16-byte aligned");
  hipLaunchKernelGGL(dequant_fp8_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)q, row_exp, K, ldq, (bf16_t*)out, ldo);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_gemv_fp8_args(void) { return (int)sizeof(usdm_gemv_fp8_args); }

int usdm_gemv_mxfp4_batch_launch(const usdm_gemv_mxfp4_args* pa, hipStream_t st);   // llm_batch_k.hip: nb = 2..4

extern "C" int usdm_gemv_mxfp4(const usdm_gemv_mxfp4_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->b.g.W && pa->b.g.x && pa->scales, "usdm_gemv_mxfp4: null args");
  const usdm_gemv_args& a = pa->b.g;
  USDM_CHECK_ARG(pa->b.nb >= 1 && pa->b.nb <= 4 && (pa->b.form == 0 || pa->b.form == -1),
                 "usdm_gemv_mxfp4: 1..4 sequences on the VALU form (the matrix-core form has no MXFP4 weights)");
  USDM_CHECK_ARG(!a.p2p && !a.p2p_mode && !a.mrg_po && !a.mrg_pm && !a.mrg_pl && !a.cmb_gran && !a.x_delta && !a.x_out,
                 "usdm_gemv_mxfp4: p2p / merged-attention input / cmb_gran / x_delta are not supported with MXFP4 weights");
  USDM_CHECK_ARG(!a.part_val && !a.part_idx && !a.ban && !a.y32, "usdm_gemv_mxfp4: the lm_head mode (part_val / ban / y32) is not supported with MXFP4 weights");
  USDM_CHECK_ARG(a.N > 0 && a.K > 0 && a.K % 32 == 0 && a.K <= 16384, "usdm_gemv_mxfp4: K must be a multiple of 32, at most 16384");
  USDM_CHECK_ARG(a.ldw % 1024 == 0 && 2 * a.ldw >= a.K && pa->lds % 64 == 0 && 32 * pa->lds >= a.K,
                 "usdm_gemv_mxfp4: ldw (bytes) must hold whole groups of 1024 bytes and lds whole groups of 64 bytes covering K");
  USDM_CHECK_ARG(((uintptr_t)a.W & 15) == 0 && ((uintptr_t)pa->scales & 3) == 0 && ((uintptr_t)a.x & 15) == 0,
                 "usdm_gemv_mxfp4: codes and x must be 16-byte, scales 4-byte aligned");
  USDM_CHECK_ARG(a.act != USDM_ACT_SWIGLU || a.N % 32 == 0, "usdm_gemv_mxfp4: swiglu needs N %% 32 == 0");
  if (int rc = gemv_check_outputs("usdm_gemv_mxfp4", a)) return rc;   // (y32 and part_val are refused above: "no output" means no y16)
  hipStream_t st = (hipStream_t)stream;
  if (pa->b.nb > 1) return usdm_gemv_mxfp4_batch_launch(pa, st);
  return gemv_launch<GEMV_PLAIN, false, false, false, false>(a, st, gemv_mx4{pa->scales, pa->lds});
}

namespace {
// prefill operand of the MXFP4 model: one workgroup per row; a thread takes one 16-byte piece of a group (its codes of four K
// iterations) and writes four 16-byte pieces of bf16 (the threads of a wave write 1 KB contiguous per store)
__global__ __launch_bounds__(256) void dequant_mxfp4_kernel(const uint8_t* codes, int64_t ldw, const uint8_t* scales, int64_t lds, int K,
                                                            bf16_t* out, int64_t ldo) {
  const int r = blockIdx.x;
  const u32x4* cr = (const u32x4*)(codes + (int64_t)r * ldw);
  const unsigned* sr = (const unsigned*)(scales + (int64_t)r * lds);
  bf16_t* orow = out + (int64_t)r * ldo;
  const int npiece = ((K + 2047) >> 11) * 64;
  for (int p = threadIdx.x; p < npiece; p += 256) {
    const int g = p >> 6, L = p & 63;
    const u32x4 w = __builtin_nontemporal_load(cr + p);
    const unsigned sc = sr[g * 16 + (L >> 2)];
    const int e = g * 2048 + L * 8;
    if (e < K) *(u32x4*)(orow + e) = mx4x8_to_bf16x8<0>(w[0], sc);
    if (e + 512 < K) *(u32x4*)(orow + e + 512) = mx4x8_to_bf16x8<1>(w[1], sc);
    if (e + 1024 < K) *(u32x4*)(orow + e + 1024) = mx4x8_to_bf16x8<2>(w[2], sc);
    if (e + 1536 < K) *(u32x4*)(orow + e + 1536) = mx4x8_to_bf16x8<3>(w[3], sc);
  }
}
}  // namespace

extern "C" int usdm_dequant_mxfp4(const void* codes, int64_t ldw, const uint8_t* scales, int64_t lds, int32_t N, int32_t K, void* out,
                                  int64_t ldo, usdm_stream_t stream) {
  USDM_CHECK_ARG(codes && scales && out, "usdm_dequant_mxfp4: null args");
  USDM_CHECK_ARG(N > 0 && K > 0 && K % 32 == 0 && ldo >= K && ldo % 8 == 0, "usdm_dequant_mxfp4: bad N/K/ldo");
  USDM_CHECK_ARG(ldw % 1024 == 0 && 2 * ldw >= K && lds % 64 == 0 && 32 * lds >= K,
                 "usdm_dequant_mxfp4: ldw (bytes) must hold whole groups of 1024 bytes and lds whole groups of 64 bytes covering K");
  USDM_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)scales & 3) == 0 && ((uintptr_t)out & 15) == 0,
                 "usdm_dequant_mxfp4: codes and out must be 16-byte, scales 4-byte aligned");
  hipLaunchKernelGGL(dequant_mxfp4_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes, ldw, scales, lds, K,
                     (bf16_t*)out, ldo);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_gemv_mxfp4_args(void) { return (int)sizeof(usdm_gemv_mxfp4_args); }

#ifdef USDM_GEMV_TRACE
extern "C" int usdm_dbg_gemv_trace(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_gemv_trace), sizeof(unsigned long long) * n);
}
#endif

extern "C" int usdm_gemv_nblocks(int32_t N, int32_t act) { return cdiv(N, 16); }

// threads per workgroup of the variant usdm_gemv launches for this projection: gemv_select's, the launcher's own choice (the
// fused RMSNorm's partial sums follow that partition; usdm_gemv_engine reproduces it to stay bit-identical)
extern "C" int usdm_gemv_threads(const usdm_gemv_args* pa) { return 64 * gemv_select(*pa, false).nwv; }
// 1 where usdm_gemv runs this (bf16) projection in the straight-line form (gemv_stream_kernel)
extern "C" int usdm_gemv_streams(const usdm_gemv_args* pa) { return gemv_select(*pa, false).stream ? 1 : 0; }

extern "C" int usdm_argmax_final_seg(const float* part_val, const int32_t* part_idx, int32_t nparts, int32_t nseg, int64_t seg_stride,
                                     const usdm_decode_state* st, const void* embed_table, int32_t Hd, void* h_out,
                                     usdm_stream_t stream) {
  USDM_CHECK_ARG(part_val && part_idx && nparts > 0 && st && st->next_token && st->out_tokens && st->step && st->pos,
                 "usdm_argmax_final: bad args");
  USDM_CHECK_ARG(nseg >= 1 && (nseg == 1 || seg_stride >= (int64_t)nparts * (st->batch > 1 ? st->batch : 1)), "usdm_argmax_final_seg: segments overlap");
  USDM_CHECK_ARG(!embed_table || (h_out && Hd > 0 && Hd % 8 == 0), "usdm_argmax_final: embedding output missing");
  USDM_CHECK_ARG(st->batch >= 0 && st->batch <= 64, "usdm_argmax_final: batch");
  hipLaunchKernelGGL(argmax_final_kernel, dim3(st->batch > 1 ? st->batch : 1), dim3(256), 0, (hipStream_t)stream, part_val, part_idx, nparts, nseg,
                     seg_stride, *st, (const bf16_t*)embed_table, Hd, (bf16_t*)h_out);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_argmax_final(const float* part_val, const int32_t* part_idx, int32_t nparts,
                                 const usdm_decode_state* st, const void* embed_table, int32_t Hd, void* h_out,
                                 usdm_stream_t stream) {
  return usdm_argmax_final_seg(part_val, part_idx, nparts, 1, 0, st, embed_table, Hd, h_out, stream);
}

extern "C" int usdm_embed_rows(const void* table, const int64_t* ids, const int32_t* next_token, int32_t n, int32_t Hd,
                               void* out, usdm_stream_t stream) {
  USDM_CHECK_ARG(table && out && (ids || next_token) && n > 0, "usdm_embed_rows: bad args");
  USDM_CHECK_ARG(Hd % 8 == 0, "usdm_embed_rows: Hd=%d must be a multiple of 8 (16-byte row copies)", Hd);
  hipLaunchKernelGGL(embed_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)table, ids, next_token, n, Hd,
                     (bf16_t*)out);
  USDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int usdm_residual_add(void* h, const float* delta, int32_t n, usdm_stream_t stream) {
  USDM_CHECK_ARG(h && delta && n > 0, "usdm_residual_add: bad args");
  hipLaunchKernelGGL(residual_add_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)h, delta, n);
  USDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int usdm_sizeof_gemv_args(void) { return (int)sizeof(usdm_gemv_args); }
extern "C" int usdm_sizeof_decode_state(void) { return (int)sizeof(usdm_decode_state); }
