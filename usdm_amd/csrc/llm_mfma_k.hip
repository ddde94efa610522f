// Batched decode for 5..16 sequences (round 4): the weight-streaming projection as a skinny GEMM on the matrix cores.
//
// Reference call site: the serving path hands vLLM an arbitrary request list (src/inference_vllm.py:109-125); here a decode step
// of up to 16 sequences streams every weight byte ONCE (14.3 GB per step, HBM-bound exactly like the batch-1 step) and does the
// 16 x more arithmetic on v_mfma_f32_16x16x32_bf16, where it is free: one MFMA (16 cycles of one SIMD) per KiB of weights against
// ~100 cycles of HBM time per KiB and CU.  The VALU form (llm_batch_k.hip, <= 4 sequences) pays 4 v_dot2 per 16 bytes and sequence.
//
// Layout of the product ("swap-AB"): the WEIGHTS are the A operand - a tile is 16 weight rows, lane (r = lane % 16, g = lane / 16)
// loads the 16 bytes W[row r][k0 + 8 g .. + 8) straight from HBM into the MFMA fragment layout (a wave instruction = 16 rows x 64
// contiguous bytes; two consecutive K chunks complete every 128-byte line; non-temporal) - and the activations [16 sequences][K] are
// the B operand (lane (b, g) holds x[b][k0 + 8 g .. + 8)).  D[row][sequence]: lane (b, g) ends with 4 consecutive output features
// of sequence b.  No LDS on the weight path, no transposes.
//
// Decomposition: ONE 8-wave workgroup per CU; the 8 waves split K (wave w owns K chunks [w cpw, (w + 1) cpw) of 32), so the
// activation slice a wave needs is 16 fragments that it HOLDS in registers for every tile (K <= 4096: all RMSNorm-fed projections and
// o_proj; the RMSNorm with HF's rounding points is applied to the held fragments in the prologue, under the first weight loads), or
// streams beside the weights (down_proj, K = 14336, one tile per workgroup).  Tiles (16 rows; 12 where that balances the 256 CUs
// better; SwiGLU: 8 gate + 8 up rows of the same 8 features) are dealt round-robin to the workgroups; a wave keeps the loads of two
// tiles (16 x 16 B per lane) in flight.  The 8 partial sums per output are added in wave order through LDS (deterministic), then
// the batch-1 kernels' epilogues: bf16 rounding points of HF, residual add, SwiGLU, ban-masked arg-max partials + logits.
//
// Per sequence the result is NOT bit-identical to usdm_gemv: the K partition and the MFMA's internal summation order differ (f32
// rounding of the accumulation; the RMSNorm sum of squares is partitioned differently as well).  Parity is against the oracle
// (tests/test_batch_gpu.py: near-tie rule), not against the batch-1 kernel.
//
// FP8 weights (usdm_gemv_fp8_mfma, opt-in): the same kernel with an FP8 template flag - e4m3 bytes with a power-of-two scale per row,
// converted exactly to bf16 in registers right before each MFMA; everything else is the bf16 form, so the result equals it on the
// dequantized weights W' bit for bit.
//
// MXFP4 weights (usdm_gemv_mxfp4_mfma, opt-in): the same kernel again, selected by the type of its extra argument - a second image
// of the codes, cut so that one 16-byte load is a lane's A fragments of four consecutive chunks, and one e8m0 scale per row and chunk;
// converted exactly to bf16 right before each MFMA, equal to the bf16 form on W' bit for bit.
//
// The shape of this file (a new format or schedule: DESIGN.md 8f).  Helpers: slot aliases, drain, recut_store / recut_frag, next_unit.
// gemv_mfma_kernel: tiles and ban mask; row_of and the load bases; the first loads of the live stream; RMSNorm; the services a stream
// hands tiles to (epilogue, ks_merge, flush_group, finish_tile, keep_tile); the streams - quads (MXFP4), re-cut FP8, re-cut bf16, ring,
// pairs - one `if constexpr` branch each (as five structs every instantiation left class A / B: profiles/gemv_mfma_split.txt); the
// final flush; the lm_head partials.  Host: mfma_select, USDM_MFMA_VARIANTS (the one list of instantiations), launch_one.
#include "common.h"
#include "../../include/usdm_hip.h"
#include "gemv_common.h"
#include <type_traits>

namespace {
constexpr int MW = 8;     // waves per workgroup (two per SIMD: 256 registers each, spent on loads in flight)
constexpr int CH = 16;    // K chunks of 32 a wave can hold activations for (K <= MW * CH * 32 = 4096)
constexpr int MTG_DEF = 16;   // tiles per reduction group (LDS: MTG x MW waves x 1 KiB)
constexpr int MTG_TRL = 8;    // ... of the transposed-load variant (its LDS also holds 8 KiB of transposition buffer per wave)
#ifndef USDM_MFMA_NO_ASM
#define USDM_MFMA_NO_ASM 0   // 1: the compiler-scheduled stream everywhere (debugging)
#endif
constexpr int GAM_FLOATS = 4096;
constexpr int TAIL_BYTES = GAM_FLOATS * 4 + MW * 16 * 4 + 64 * 4 + 2 * MTG_DEF * 16 * 4;       // gam, ssum, tl, sv, si
constexpr int LDS_BYTES = MTG_DEF * MW * 1024 + TAIL_BYTES;
constexpr int TB_OFF = MTG_TRL * MW * 1024 + TAIL_BYTES;                                        // transposition buffers of the TRL variant
constexpr int LDS_BYTES_TRL = TB_OFF + MW * 8192;

#ifdef USDM_MFMA_TRACE
// debugging aid (tools/gemv_mfma_trace.py): per-workgroup phase timestamps of wave 0 (100 MHz wall clock) + hardware ids
__device__ unsigned long long g_mfma_trace[512 * 8];
#define TRM(i) do { if (threadIdx.x == 0 && blockIdx.x < 512) g_mfma_trace[blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define TRM(i) do { } while (0)
#endif

struct MfmaDev {
  usdm_gemv_batch_args ba;
  int ntiles, rt, cpw, nchunks, grid, nout;
  int ksplit, kwg;      // K split over workgroups: slices of ksplit_k elements, kwg workgroups per slice (1, grid: not split)
};
constexpr int KS_K = 2048;  // K per workgroup of the split form: 8 waves x 8 chunks, one 8-load unit per tile and wave
constexpr int KS_MAX = 8;   // slices (K <= 16384)

// MXFP4 (usdm_gemv_mxfp4_mfma): the matrix-core image of the matrix (include/usdm_hip.h) is the one extra kernel argument of the
// MX4 instantiations, which its TYPE selects: FP8 stays a bool and every bf16 / FP8 instantiation keeps its name.
struct gemv_mx4mc { const uint8_t* codes; const uint8_t* scales; int64_t ldc, lds; };
template <class... FMT> struct gemv_is_mx4mc { static constexpr bool value = false; };
template <> struct gemv_is_mx4mc<gemv_mx4mc> { static constexpr bool value = true; };
__device__ __forceinline__ const int8_t* gemv_row_exp(gemv_mx4mc) { return nullptr; }
__device__ __forceinline__ gemv_mx4mc gemv_mx4mc_fmt() { return gemv_mx4mc{nullptr, nullptr, 0, 0}; }
__device__ __forceinline__ gemv_mx4mc gemv_mx4mc_fmt(const int8_t*) { return gemv_mx4mc{nullptr, nullptr, 0, 0}; }
__device__ __forceinline__ gemv_mx4mc gemv_mx4mc_fmt(gemv_mx4mc m) { return m; }

__device__ __forceinline__ f32x4 mfma16(u32x4 w, u32x4 x, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
}

// CPWT: K chunks per wave as a compile-time constant (16: K = 4096; 56: K = 14336), 0 = read it from the launch (any K).  With a
// constant every load of the stream loop is unconditional straight-line code; behind per-chunk branches the compiler's wait-count
// pass gives up at the joins and drains the whole ring (vmcnt(0)) in front of every MFMA - measured: 3.0 instead of ~5 TB/s.
// Hand-counted loads for the straight-line part of the HOLD stream (cdna_hip_programming.md 5.7, form (ii)): the compiler neither
// sees these loads nor waits for them; every consumer below waits for exactly its own load (in-order completion: "all but the 23
// youngest") inside the same asm statement that multiplies it.
// (templates only so that the FP8 instantiations, whose generic-form ring holds u32x2, still parse the hand-counted bf16 branches they
// never take; every use is u32x4)
template <class V>
__device__ __forceinline__ void ld_nt_asm(V& dst, const V* p) {
  asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(dst) : "v"(p) : "memory");
}
// FP8 (usdm_gemv_fp8_mfma): the row exponent of the lane's A-row, hand-counted like the weight loads of its unit
__device__ __forceinline__ void ld_exp_asm(int& dst, const int8_t* p) {
  asm volatile("global_load_sbyte %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
// ---- slots of a ring of registers: compile-time indices, so that every register array is indexed by constants
template <int I> using slot = std::integral_constant<int, I>;
using Q0 = slot<0>; using Q1 = slot<1>; using Q2 = slot<2>; using Q3 = slot<3>;
template <int N> using slots = std::make_integer_sequence<int, N>;
template <int... I, class F>
__device__ __forceinline__ void each_slot(std::integer_sequence<int, I...>, F&& f) { (f(slot<I>{}), ...); }
template <int... I, class F>      // f(slot) for the slots in order until one returns false
__device__ __forceinline__ bool all_slots(std::integer_sequence<int, I...>, F&& f) { return (f(slot<I>{}) && ...); }

// drain: loads for tiles that do not exist may still be in flight into load registers; the wait for everything in one statement,
// then every load register named after it, which keeps the compiler from reusing any of them before the wait has executed
template <class V> __device__ __forceinline__ void name_reg(const V& v) { asm volatile("" ::"v"(v) : "memory"); }
template <class V, int N> __device__ __forceinline__ void name_reg(const V (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) name_reg(v[i]);
}
template <class... R> __device__ __forceinline__ void drain(const R&... regs) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  (name_reg(regs), ...);
}

// ---- re-cut of row-contiguous loads into MFMA fragments through a wave's LDS buffer [16 rows][ROWB bytes], 16-byte piece ^ row
// (conflict-free both ways).  ROWB: bytes of a row per unit (512, or FP8's 256); a load instruction covers 1024 / ROWB rows.
// the landed loads of a unit -> the buffer, by rows
template <int ROWB, int NL>
__device__ __forceinline__ void recut_store(char* tb, int lane, const u32x4 (&u)[NL]) {
  constexpr int RPI = 1024 / ROWB;
  static_assert(NL == 16 / RPI, "a unit is 16 rows");
  const int lrow = lane / (64 / RPI), lp = lane % (64 / RPI);      // row (of the instruction's RPI) and 16-byte piece this lane loaded
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int r = RPI * i + lrow;
    *(u32x4*)(tb + r * ROWB + ((lp ^ r) << 4)) = u[i];
  }
}
// chunk c of lane (r16, g)'s row: its 8 weights as V (16 bytes of bf16, 8 of e4m3)
template <int ROWB, class V>
__device__ __forceinline__ V recut_frag(const char* tb, int r16, int g, int c) {
  if constexpr (sizeof(V) == 16) return *(const V*)(tb + r16 * ROWB + (((4 * c + g) ^ r16) << 4));
  else return *(const V*)(tb + r16 * ROWB + (((2 * c + (g >> 1)) ^ r16) << 4) + (g & 1) * 8);      // (one formula in bytes left class A)
}

// ---- streamed units: K slices longer than the held activations are multiplied in units numbered through the tiles, UPT per tile
// and wave; (t, s) is a unit, next_unit moves to the following one (true: it is the first of the next tile)
struct unit_pos { int t, s; };
template <int UPT, class NEXT>
__device__ __forceinline__ bool next_unit(unit_pos& u, NEXT&& next) {
  if (++u.s == UPT) {
    u.s = 0;
    u.t = next();
    return true;
  }
  return false;
}
template <int WAIT, bool FIRST, class V>
__device__ __forceinline__ void wait_mfma_asm(f32x4& acc, const V& w, const u32x4& x) {
  if constexpr (FIRST)
    asm volatile("s_waitcnt vmcnt(%3)\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(x), "n"(WAIT));
  else
    asm volatile("s_waitcnt vmcnt(%3)\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(x), "n"(WAIT));
}

// TRL ("transposed loads", K = 4096 only): the weights are loaded ROW-CONTIGUOUSLY - a load instruction reads 512 bytes of each of
// two rows, the pattern the batch-1 kernel streams at 5.9 TB/s - and re-cut into MFMA fragments through a private 8 KiB LDS buffer
// per wave (ds_write_b128 by rows, ds_read_b128 by fragments, XOR swizzle piece ^ row: conflict-free both ways).  The fragment-shaped
// loads of the other variants (16 rows x 64 bytes per instruction) measured 4.4 TB/s at best: 64-byte requests and a DRAM page
// visit per 64 - 128 bytes.  LDS traffic: 2 x 56 MB per CU and step against 56 MB of HBM traffic at a tenth of the LDS rate.
//
// FP8 (usdm_gemv_fp8_mfma): W holds e4m3 bytes [N][ldw] and row r is scaled by 2^row_exp[r] (usdm_amd/quant.py); the row exponents
// are one extra kernel argument of the FP8 instantiations only, so the bf16 ones keep their signature and code.  Only the weight
// load and its unpack differ: every tile, chunk order, wave merge, K split and epilogue is the bf16 one, and the exact conversion
// (fp8x8_to_bf16x8) hands the MFMA the bf16 fragments of W' = q * 2^e, so the result equals the bf16 form on W' bit for bit.
template <bool HOLD, int CPWT, bool TRL, bool FP8 = false, class... FMT>
__global__ __launch_bounds__(MW * 64) void gemv_mfma_kernel(const MfmaDev d, FMT... fmt) {
  constexpr bool MX4 = gemv_is_mx4mc<FMT...>::value;
  static_assert((FP8 || MX4) == (sizeof...(FMT) == 1) && !(FP8 && MX4), "FP8 takes the row exponents, MXFP4 its matrix-core image");
  static_assert(!FP8 || TRL || CPWT == 0, "FP8: the row-contiguous forms and the generic ones (the fragment-shaped form 3 is bf16 only)");
  static_assert(!MX4 || (!TRL && (HOLD ? CPWT == 0 || CPWT == 8 || CPWT == 16 : CPWT == 0)), "MXFP4: the image is cut into fragments already");
  constexpr bool KSPLIT = (TRL || MX4) && HOLD && CPWT == 8;     // the forms of the K split over workgroups
  const usdm_gemv_args& a = d.ba.g;
  const int cpw = CPWT > 0 ? CPWT : d.cpw;
  constexpr int MTG = TRL ? MTG_TRL : MTG_DEF;             // tiles per reduction group
  constexpr int RED_BYTES = MTG * MW * 64 * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TRM(0);
#ifdef USDM_MFMA_TRACE
  if (threadIdx.x == 0 && blockIdx.x < 512)
    g_mfma_trace[blockIdx.x * 8 + 7] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | __builtin_amdgcn_s_getreg(63492);
#endif
  f32x4* red = (f32x4*)smem;                               // [MTG][MW][64] partial D fragments
  float* gam = (float*)(smem + RED_BYTES);                 // [K <= 4096] RMSNorm weight
  float* ssum = gam + GAM_FLOATS;                          // [MW][16] partial sums of squares
  int* tl = (int*)(ssum + MW * 16);                        // [MTG] tile ids of the group being reduced
  float* sv = (float*)(tl + 64);                           // lm_head: [MW][16] best value / index per reducing wave and sequence
  int* si = (int*)(sv + MTG_DEF * 16);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int nb = d.ba.nb, K = a.K;
  const bool glu = a.act == USDM_ACT_SWIGLU;
  const bool lmh = a.part_val != nullptr;
  const bf16_t* Wb = (const bf16_t*)a.W;
  const int8_t* rexp = gemv_row_exp(fmt...);
  typedef std::conditional_t<FP8, u32x2, u32x4> wvec;       // one lane's 8 weights of a chunk: 16 bf16 or 8 e4m3 bytes

  // ---- tiles of this workgroup: t = blockIdx.x + i * grid, i < ncand; lm_head: tiles whose 16 ids are all banned are not streamed
  // (K split over workgroups: workgroup = (slice ksi, member tile0 of the kwg workgroups that share the slice))
  const int ksi = d.ksplit > 1 ? (int)blockIdx.x % d.ksplit : 0;
  const int tile0 = d.ksplit > 1 ? (int)blockIdx.x / d.ksplit : (int)blockIdx.x, tstep = d.kwg;
  const int kofs = ksi * KS_K;
  const int ncand = tile0 < d.ntiles ? (d.ntiles - tile0 + tstep - 1) / tstep : 0;
  unsigned long long mask = ncand >= 64 ? ~0ull : ((1ull << ncand) - 1ull);
  if (lmh && a.ban) {
    bool act = false;
    if (lane < ncand) {
      const int t = tile0 + lane * tstep;
      if (t * 16 + 16 <= a.N && (((uintptr_t)a.ban) & 15) == 0) {      // one 16-byte load per tile (sixteen dependent byte loads cost ~10 us)
        const u32x4 bv = *(const u32x4*)(a.ban + t * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) act |= ((bv[e] & 0xff) == 0) | (((bv[e] >> 8) & 0xff) == 0) | (((bv[e] >> 16) & 0xff) == 0) | ((bv[e] >> 24) == 0);
      } else {
        for (int r = 0; r < 16 && t * 16 + r < a.N; ++r) act |= (a.ban[t * 16 + r] == 0);
      }
    }
    mask = __ballot(act);
    if (a.y32) {      // the logits of tiles that are not streamed: -inf for every sequence (what the sampling kernel expects of banned ids)
      for (int i = 0; i < ncand; ++i) {
        if ((mask >> i) & 1ull) continue;
        const int t = tile0 + i * tstep;
        for (int e = tid; e < 16 * nb; e += MW * 64) {
          const int n = t * 16 + (e & 15);
          if (n < a.N) a.y32[(int64_t)(e >> 4) * d.ba.y_bs + n] = -INFINITY;
        }
      }
    }
  }
  unsigned long long rem_ld = mask, rem_cp = mask;
  auto next_tile = [&](unsigned long long& m) -> int {
    if (!m) return -1;
    const int i = __builtin_ctzll(m);
    m &= m - 1;
    return tile0 + i * tstep;
  };
  // Per-lane base of this wave's K slice of tile t (A-row r16), and of the activation slice.  Rows / sequences that do not exist are
  // CLAMPED to existing ones instead of masked: they only feed output rows / columns that the epilogue never stores, and every load
  // below stays unconditional (uniform control flow, one 64-bit base + immediates per tile).
  const int kc0 = wave * cpw;                             // first K chunk of this wave (host: K %% (MW * 32) == 0)
  // the row of W behind A-row r of tile t (t < 0: row 0): the one place that knows how tiles are cut
  auto row_of = [&](int t, int r) -> int {
    if (t < 0) return 0;
    if (glu) return gemv_glu_row(min(t * 8 + (r & 7), d.nout - 1), r >= 8);
    return min(t * d.rt + r, a.N - 1);
  };
  auto wbase = [&](int t) -> const wvec* {
    // (row_of's text with the clamp of t < 0 INSIDE the SwiGLU row, which this base has always had - a lane of the up half reads row
    // 16 then; through row_of plus that case the ring and pair instantiations, the hand-counted one among them, left class A / B)
    int row;
    if (glu) row = gemv_glu_row(t < 0 ? 0 : min(t * 8 + (r16 & 7), d.nout - 1), r16 >= 8);
    else row = t < 0 ? 0 : min(t * d.rt + r16, a.N - 1);
    if (t < 0 && K >= 2048) {
      // No such tile: the stream loop's loads stay unconditional (uniform wait counts), but they must cost nothing - 64 bytes of the
      // activation vector per instruction (one request instead of sixteen), a different line for every wave so that no L2 channel
      // becomes a hot spot (weight row 0 for everyone did).  Row 0 of x holds K * 2 bytes; chunk offsets reach 1 KiB further.
      const int line = (int)((blockIdx.x * MW + wave) % (unsigned)(K / 32 - 16));
      return (const wvec*)a.x + line * 4 + (lane & 3);
    }
    if constexpr (FP8) return (const u32x2*)((const uint8_t*)a.W + (int64_t)row * a.ldw + (int64_t)kc0 * 32 + 8 * g);
    else return (const u32x4*)(Wb + (int64_t)row * a.ldw + (int64_t)kc0 * 32 + 8 * g);
  };
  auto wload = [&](const wvec* base, int c) -> wvec {
    return __builtin_nontemporal_load(base + c * 4);
  };
  // FP8: the scale of tile t for this lane's row r16, and the bf16 fragment of 8 loaded bytes
  auto wscale = [&](int t) -> float {
    if constexpr (FP8) return fp8_row_scale(rexp[row_of(t, r16)]);
    else return 0.f;
  };
  auto wfrag = [&](const wvec& w, float s) -> u32x4 {
    if constexpr (FP8) return fp8x8_to_bf16x8(w, s);
    else return w;
  };
  const u32x4* xbase = (const u32x4*)((const bf16_t*)a.x + (int64_t)min(r16, nb - 1) * d.ba.x_bs + kofs + (int64_t)kc0 * 32 + 8 * g);
  auto xload = [&](int c) -> u32x4 { return xbase[c * 4]; };

  // ---- loads: the activation slice first (they return first: L2 hits), then the weights of the first two tiles
  u32x4 xf[HOLD ? CH : 1];
  float4 gv[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  if constexpr (HOLD) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (c < cpw) xf[c] = xload(c);
    if (a.norm_w) {
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if ((tid + q * MW * 64) * 4 < K) gv[q] = *(const float4*)(a.norm_w + (tid + q * MW * 64) * 4);
    }
  }
  // HOLD: a ring of RS = 24 weight fragments = the loads of one and a half tiles (24 KiB per wave, 192 KiB per CU in flight; 32 slots
  // next to the 16 held activation fragments do not fit 256 registers).  Item j = (tile j / 16, chunk j % 16) lives in slot j % 24 and is
  // refilled with item j + 24 as soon as it has been multiplied; the stream loop below is unrolled over three tiles so that slot and
  // chunk indices are constants.  Otherwise (STREAM): CH (weight, activation) pairs.
  constexpr int RS = 24;
  wvec ring[TRL ? 1 : (HOLD ? RS : CH)];
  u32x4 rx[HOLD ? 1 : CH];
  // ---- TRL: NR = 3 units of 8 row-contiguous loads (16 rows x 512 bytes = 8 chunks of this wave's K slice) = one and a half tiles in
  // flight (24 KiB per wave; four units next to the 16 held activation fragments spill)
  // (streamed activations: 16 loads per unit, two units = 32 KiB per wave; the K-split form holds only 8 activation fragments: 4 units)
  constexpr int NR = HOLD ? (CPWT == 8 ? 4 : 3) : 2;
  u32x4 U[TRL ? NR : 1][8];
  u32x4 X[(TRL && !HOLD) ? NR : 1][8];                     // streamed activations of the same units (K > 4096)
  const int lrow = lane >> 5, lp = lane & 31;              // row (of a pair) and 16-byte piece this lane loads
  auto unit_ptr = [&](int t, int sub, int i) -> const u32x4* {
    if (t < 0) return (const u32x4*)a.x + ((blockIdx.x * MW + wave) & 7) * 4 + (lane & 3) + i * 32;      // placeholder: 64 B of x (see wbase)
    return (const u32x4*)(Wb + (int64_t)row_of(t, 2 * i + lrow) * a.ldw + kofs + (int64_t)wave * (cpw * 32) + sub * 256 + lp * 8);
  };
  int t0 = (TRL || MX4) ? -1 : next_tile(rem_ld), t1 = -1, t2 = -1;  // tile being multiplied, the next two (loads in flight / to be issued)
  const wvec* wp0 = wbase(t0);
  const wvec* wp1 = wp0;
  const wvec* wp2 = wp0;
  float sc0 = 0.f, sc1 = 0.f, sc2 = 0.f;                    // FP8, generic forms: the scales of t0, t1, t2 for this lane's row
  if constexpr (FP8 && !TRL) sc0 = wscale(t0);
  constexpr bool ASM_STREAM = HOLD && CPWT == CH && !USDM_MFMA_NO_ASM && !TRL && !MX4;     // hand-counted loads (see the stream loop)
  int ua = -1, ub = -1, uc = -1;                            // TRL: the tile being multiplied and the next two
  // TRL with streamed activations (K = 14336): units are numbered through the tiles, 7 per tile; lu = the next unit to load
  unit_pos lu{-1, 0};
  constexpr int UPT = CPWT / 8;                             // units per tile and wave
  auto ld_unit_x = [&](auto SLOT, int t, int sub) __attribute__((always_inline)) {
    constexpr int q = decltype(SLOT)::value;
#pragma unroll
    for (int i = 0; i < 8; ++i) ld_nt_asm(U[q][i], unit_ptr(t, sub, i));
#pragma unroll
    for (int c = 0; c < 8; ++c) ld_nt_asm(X[q][c], xbase + (sub * 8 + c) * 4);
  };
  auto adv_unit = [&]() { next_unit<UPT>(lu, [&]() { return next_tile(rem_ld); }); };
  if constexpr (!FP8 && TRL && !HOLD) {
    lu.t = next_tile(rem_ld);
    ld_unit_x(Q0{}, lu.t, lu.s); adv_unit();
    ld_unit_x(Q1{}, lu.t, lu.s); adv_unit();
  }
  int tq[4] = {-1, -1, -1, -1};                             // K-split form: the tiles whose single unit sits in slots 0 .. 3
  if constexpr (!FP8 && TRL && HOLD && CPWT == 8) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      tq[q] = next_tile(rem_ld);
#pragma unroll
      for (int i = 0; i < 8; ++i) ld_nt_asm(U[q][i], unit_ptr(tq[q], 0, i));
    }
  }
  if constexpr (!FP8 && TRL && HOLD && CPWT != 8) {
    ua = next_tile(rem_ld); ub = next_tile(rem_ld); uc = next_tile(rem_ld);
#pragma unroll
    for (int i = 0; i < 8; ++i) ld_nt_asm(U[0][i], unit_ptr(ua, 0, i));      // units 0, 1, 2 = (tile a, half 0), (a, 1), (b, 0)
#pragma unroll
    for (int i = 0; i < 8; ++i) ld_nt_asm(U[1][i], unit_ptr(ua, 1, i));
#pragma unroll
    for (int i = 0; i < 8; ++i) ld_nt_asm(U[2][i], unit_ptr(ub, 0, i));
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (c < cpw && !TRL && !MX4) {
      if constexpr (ASM_STREAM) ld_nt_asm(ring[c], wp0 + c * 4);
      else ring[c] = wload(wp0, c);
      if constexpr (!HOLD) rx[c] = xload(c);
    }
  }
  if constexpr (HOLD && !TRL && !MX4) {
    t1 = next_tile(rem_ld);
    wp1 = wbase(t1);
#pragma unroll
    for (int c = 0; c < RS - CH; ++c) {
      if (c < cpw) {
        if constexpr (ASM_STREAM) ld_nt_asm(ring[CH + c], wp1 + c * 4);
        else ring[CH + c] = wload(wp1, c);
      }
    }
    t2 = next_tile(rem_ld);
    wp2 = wbase(t2);
    if constexpr (FP8) { sc1 = wscale(t1); sc2 = wscale(t2); }
  }
  // ---- FP8, row-contiguous forms: a unit = the 16 rows x ROW8 bytes of one tile's K slice of this wave (K = 4096: the whole 512-byte
  // slice, two rows per load instruction as in bf16, 8 loads; K split / streamed: 256 bytes, four rows per instruction, 4 loads),
  // then one byte load of the lane's row exponent (streamed: and the unit's 8 activation fragments), all hand-counted.  Twice the
  // units of bf16 in flight, about the same bytes: K = 4096 three tiles (24 KiB per wave), K split eight, streamed three units.
  constexpr int RPI8 = CPWT == 16 ? 2 : 4;                  // rows per load instruction
  constexpr int ROW8 = 1024 / RPI8;                         // bytes of a row per unit
  constexpr int NL8 = 16 / RPI8;                            // weight loads per unit
  constexpr int NR8 = CPWT == 8 ? 8 : 3;                    // units in flight
  constexpr int LPU8 = NL8 + 1 + (HOLD ? 0 : 8);            // loads per unit
  u32x4 U8[FP8 && TRL ? NR8 : 1][NL8];
  int E8[FP8 && TRL ? NR8 : 1];
  u32x4 X8[FP8 && TRL && !HOLD ? NR8 : 1][8];
  int tq8[FP8 && TRL ? NR8 : 1];                            // held forms: the tile whose unit sits in slot q (tile n in slot n % NR8)
  const int lrow8 = lane / (64 / RPI8), lp8 = lane % (64 / RPI8);
  auto unit8_ptr = [&](int t, int sub, int i) -> const u32x4* {
    if (t < 0) return (const u32x4*)a.x + ((blockIdx.x * MW + wave) & 7) * 4 + (lane & 3) + i * 32;      // placeholder (see unit_ptr)
    return (const u32x4*)((const uint8_t*)a.W + (int64_t)row_of(t, RPI8 * i + lrow8) * a.ldw + kofs + (int64_t)wave * (cpw * 32) +
                          sub * ROW8 + lp8 * 16);
  };
  auto ld_unit8 = [&](auto SLOT, int t, int sub) __attribute__((always_inline)) {
    constexpr int q = decltype(SLOT)::value;
#pragma unroll
    for (int i = 0; i < NL8; ++i) ld_nt_asm(U8[q][i], unit8_ptr(t, sub, i));
    ld_exp_asm(E8[q], rexp + row_of(t, r16));
    if constexpr (!HOLD) {
#pragma unroll
      for (int c = 0; c < 8; ++c) ld_nt_asm(X8[q][c], xbase + (sub * 8 + c) * 4);
    }
  };
  if constexpr (FP8 && TRL && !HOLD) {
    lu.t = next_tile(rem_ld);
    each_slot(slots<NR8>{}, [&](auto Q) __attribute__((always_inline)) { ld_unit8(Q, lu.t, lu.s); adv_unit(); });
  }
  if constexpr (FP8 && TRL && HOLD) {
    each_slot(slots<NR8>{}, [&](auto Q) __attribute__((always_inline)) {
      tq8[decltype(Q)::value] = next_tile(rem_ld);
      ld_unit8(Q, tq8[decltype(Q)::value], 0);
    });
  }

  // ---- MXFP4 (usdm_gemv_mxfp4_mfma; the stream loop says what the image gives a lane), held activations: a unit = one tile's K slice
  // of this wave, NQ quads = NQ 16-byte loads + NQ scale dwords, ND tiles in flight (K = 4096: 4 x 4 KiB per wave; K split: all <= 8
  // tiles of the workgroup, 2 KiB each).  Six tiles of K = 4096 spill next to the 16 held activation fragments.  All loads are the compiler's (counted by its own s_waitcnt).  A unit whose
  // tile does not exist loads ONE 16-byte piece of row 0 for the whole wave (a single request, a different quad for every wave) and
  // the scale dword of that quad: inside the image, and every load of the loop stays unconditional.
  const gemv_mx4mc m = gemv_mx4mc_fmt(fmt...);
  const int kca = kofs / 32 + kc0;                          // this wave's first chunk in the row
  const int phq = (int)((blockIdx.x * MW + wave) % (unsigned)(K / 128));      // the placeholder's quad of row 0
  const bool quads = CPWT > 0 || (cpw & 3) == 0;            // else a quad would straddle two waves: dword loads (see the stream loop)
  constexpr int NQ = CPWT > 0 ? CPWT / 4 : CH / 4;
  constexpr int ND = CPWT == 8 ? 8 : 4;
  const int nq = cpw >> 2;
  u32x4 cq[MX4 && HOLD ? ND : 1][NQ];
  unsigned sq[MX4 && HOLD ? ND : 1][NQ];
  int tm[ND];
  auto ld_tile = [&](auto SLOT, int t) __attribute__((always_inline)) {
    constexpr int s = decltype(SLOT)::value;
    const int row = row_of(t, r16);
    const uint8_t* cp = t < 0 ? m.codes + phq * 64 : m.codes + (int64_t)row * m.ldc + kca * 16 + g * 16;
    const uint8_t* sp = t < 0 ? m.scales + phq * 4 : m.scales + (int64_t)row * m.lds + kca;
    const int cs = t < 0 ? 0 : 64, ss = t < 0 ? 0 : 4;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q < nq) {
        cq[s][q] = __builtin_nontemporal_load((const u32x4*)(cp + q * cs));
        sq[s][q] = *(const unsigned*)(sp + q * ss);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                      // units are issued in the order in which they are multiplied
  };
  if constexpr (MX4 && HOLD) {
    if (quads) {
      each_slot(slots<ND>{}, [&](auto Q) __attribute__((always_inline)) {
        tm[decltype(Q)::value] = next_tile(rem_ld);
        ld_tile(Q, tm[decltype(Q)::value]);
      });
    }
  }

  TRM(1);
  // ---- RMSNorm of the held activation slice (HF: bf16(bf16(x * rstd) * weight)), under the weight loads
  if constexpr (HOLD) {
    if (a.norm_w) {
      float ss = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
        if (c < cpw) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = bf2f(xf[c][e] & 0xffff), hi = bf2f(xf[c][e] >> 16);
            ss = fmaf(hi, hi, fmaf(lo, lo, ss));      // (explicit: the build contracts nothing; this prologue is ~700 vector instructions per wave)
            // (not gemv_sumsq8: this kernel's statistic is deliberately this fmaf chain with a 16-lane reduction)
          }
        }
      if (r16 >= nb) ss = 0.f;
      ss += __shfl_xor(ss, 16, 64);
      ss += __shfl_xor(ss, 32, 64);
      if (g == 0) ssum[wave * 16 + r16] = ss;
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if ((tid + q * MW * 64) * 4 < K) *(float4*)(gam + (tid + q * MW * 64) * 4) = gv[q];
      __syncthreads();
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < MW; ++w) tot += ssum[w * 16 + r16];
      const float rstd = rsqrtf(tot / (float)K + a.eps);
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (c < cpw) {
          const float4 g0 = *(const float4*)(gam + (kc0 + c) * 32 + 8 * g), g1 = *(const float4*)(gam + (kc0 + c) * 32 + 8 * g + 4);
          const float gw[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {   // (gemv_rmsnorm8's text: as the function the 16-chunk forms gained 32 instructions)
            const float lo = bf2f(xf[c][e] & 0xffff), hi = bf2f(xf[c][e] >> 16);
            xf[c][e] = pack_bf2(round_bf(round_bf(lo * rstd) * gw[2 * e]), round_bf(round_bf(hi * rstd) * gw[2 * e + 1]));
          }
        }
      }
    }
  }

#ifdef USDM_MFMA_TRACE
  if constexpr (HOLD) asm volatile("s_nop 0" : "+v"(xf[0]), "+v"(xf[(CPWT > 0 ? CPWT : CH) - 1]));      // the held activations have landed / are normalised
#endif
  TRM(2);
  // ---- epilogue of one fully reduced tile: lane (sequence b = r16, row group g) holds output rows 4 g .. 4 g + 3
  float bestv = -INFINITY;
  int besti = 0x7fffffff;
  auto epilogue = [&](int t, f32x4 v) __attribute__((always_inline)) {
    const int b = r16;
    if (lmh) {
      float lv = -INFINITY;
      int li = 0x7fffffff;
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = t * 16 + 4 * g + e;
        o[e] = -INFINITY;
        if (n < a.N && !(a.ban && a.ban[n])) {
          o[e] = round_bf(v[e]);
          if (o[e] > lv) { lv = o[e]; li = n; }
        }
      }
      if (a.y32 && b < nb) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (t * 16 + 4 * g + e < a.N) a.y32[(int64_t)b * d.ba.y_bs + t * 16 + 4 * g + e] = o[e];
      }
#pragma unroll
      for (int s = 16; s <= 32; s <<= 1) {
        const float ov = __shfl_xor(lv, s, 64);
        const int oi = __shfl_xor(li, s, 64);
        if (ov > lv || (ov == lv && oi < li)) { lv = ov; li = oi; }
      }
      if (lv > bestv || (lv == bestv && li < besti)) { bestv = lv; besti = li; }
      return;
    }
    if (glu) {
      float up[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) up[e] = __shfl_xor(v[e], 32, 64);     // rows 8 .. 15 of the tile = the up rows of features 0 .. 7
      if (g < 2 && b < nb) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = t * 8 + 4 * g + e;
          if (o >= d.nout) continue;
          float r;
          if (a.round_bf16) {
            const float gt = round_bf(v[e]), u = round_bf(up[e]);
            r = round_bf(round_bf(gt / (1.0f + __expf(-gt))) * u);
          } else {
            r = (v[e] / (1.0f + __expf(-v[e]))) * up[e];
          }
          if (a.y16) ((bf16_t*)a.y16)[(int64_t)b * d.ba.y_bs + o] = f2bf(r);
          if (a.y32) a.y32[(int64_t)b * d.ba.y_bs + o] = r;
        }
      }
      return;
    }
    if (b >= nb) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rr = 4 * g + e, n = t * d.rt + rr;
      if (rr >= d.rt || n >= a.N) continue;
      float x = v[e];
      if (a.round_bf16) x = round_bf(x);
      if (a.residual) {
        x += bf2f(((const bf16_t*)a.residual)[(int64_t)b * d.ba.res_bs + n]);
        if (a.round_bf16) x = round_bf(x);
      }
      if (a.y16) ((bf16_t*)a.y16)[(int64_t)b * d.ba.y_bs + n] = f2bf(x);
      if (a.y32) a.y32[(int64_t)b * d.ba.y_bs + n] = x;
    }
  };
  // the tiles of a group are summed over the 8 waves in wave order (wave w < ng takes tile slot w) and finished
  int done = 0;
  // K split over workgroups: this workgroup's partial tile goes to ks_part[t][slice] as write-through stores (the merging workgroup
  // may sit on another XCD, whose L2 is not coherent with ours); once they are acknowledged, one relaxed increment of the tile's
  // counter; the wave that arrives last reads all slices back (agent-scope loads, all in flight together) and sums them in SLICE
  // order - the result does not depend on who was last.  No fences (an L2 write-back / invalidate per workgroup costs ~30 us).
  auto ks_merge = [&](int t, f32x4& s) __attribute__((always_inline)) -> bool {
    float* pp = d.ba.ks_part + (int64_t)t * d.ksplit * 256 + lane * 4;
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" ::"v"(pp + ksi * 256), "v"(s) : "memory");
    int old = 0;
    if (lane == 0) {
      old = __hip_atomic_fetch_add(d.ba.ks_cnt + t, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == d.ksplit - 1) __hip_atomic_store(d.ba.ks_cnt + t, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    }
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != d.ksplit - 1) return false;
    if constexpr (MX4) {
      // MXFP4: the same slices in the same order, read with the compiler's own loads (agent scope: past this XCD's L2, what sc1 asks
      // for below), so that no MX4 instantiation holds a hand-counted load (tools/check_mfma_asm.py has nothing to audit in them)
      asm volatile("" ::: "memory");                          // (the loads stay behind the counter's increment)
      f32x4 p[KS_MAX];
#pragma unroll
      for (int k = 0; k < KS_MAX; ++k) {
        const unsigned long long* q = (const unsigned long long*)(pp + min(k, d.ksplit - 1) * 256);
        const unsigned long long lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        p[k] = f32x4{__builtin_bit_cast(float, (unsigned)lo), __builtin_bit_cast(float, (unsigned)(lo >> 32)),
                     __builtin_bit_cast(float, (unsigned)hi), __builtin_bit_cast(float, (unsigned)(hi >> 32))};
      }
      s = p[0];
#pragma unroll
      for (int k = 1; k < KS_MAX; ++k)
        if (k < d.ksplit) s += p[k];
      return true;
    }
    // all KS_MAX loads and their wait in ONE statement (slices that do not exist re-read the last one): nothing the compiler emits
    // can sit between a load and its wait
    f32x4 p[KS_MAX];
    const float* q[KS_MAX];
#pragma unroll
    for (int k = 0; k < KS_MAX; ++k) q[k] = pp + min(k, d.ksplit - 1) * 256;
    static_assert(KS_MAX == 8, "eight loads below");
    asm volatile(
        "global_load_dwordx4 %0, %8, off sc1\n\tglobal_load_dwordx4 %1, %9, off sc1\n\tglobal_load_dwordx4 %2, %10, off sc1\n\t"
        "global_load_dwordx4 %3, %11, off sc1\n\tglobal_load_dwordx4 %4, %12, off sc1\n\tglobal_load_dwordx4 %5, %13, off sc1\n\t"
        "global_load_dwordx4 %6, %14, off sc1\n\tglobal_load_dwordx4 %7, %15, off sc1\n\ts_waitcnt vmcnt(0)"
        : "=&v"(p[0]), "=&v"(p[1]), "=&v"(p[2]), "=&v"(p[3]), "=&v"(p[4]), "=&v"(p[5]), "=&v"(p[6]), "=&v"(p[7])
        : "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "v"(q[4]), "v"(q[5]), "v"(q[6]), "v"(q[7])
        : "memory");
    s = p[0];
#pragma unroll
    for (int k = 1; k < KS_MAX; ++k)
      if (k < d.ksplit) s += p[k];
    return true;
  };
  auto flush_group = [&](bool more) __attribute__((always_inline)) {
    const int ng = ((done - 1) % MTG) + 1;                  // (the K-split form keeps all its <= MTG tiles for ONE flush after the stream)
    __syncthreads();
    TRM(5);
    for (int slot = wave; slot < ng; slot += MW) {
      f32x4 s = red[(slot * MW) * 64 + lane];
#pragma unroll
      for (int w = 1; w < MW; ++w) s += red[(slot * MW + w) * 64 + lane];
      if constexpr (KSPLIT) {
        if (d.ksplit > 1 && !ks_merge(tl[slot], s)) continue;
      }
      epilogue(tl[slot], s);
    }
    if (more) __syncthreads();
  };
  auto finish_tile = [&](int t, f32x4 acc) __attribute__((always_inline)) {
    const int slot = done % MTG;
    red[(slot * MW + wave) * 64 + lane] = acc;
    if (tid == 0) tl[slot] = t;
    ++done;
#ifdef USDM_MFMA_TRACE
    if (done == 1) TRM(3);
#endif
    if (done % MTG == 0) flush_group(rem_cp != 0ull);
  };
  // ... of a stream that keeps all its (at most MTG) tiles for ONE flush after it (the K split, the straight-line part); t < 0: no tile
  auto keep_tile = [&](int t, f32x4 acc) __attribute__((always_inline)) {
    if (t < 0) return;
    red[(done * MW + wave) * 64 + lane] = acc;
    if (tid == 0) tl[done] = t;
    ++done;
#ifdef USDM_MFMA_TRACE
    if (done == 1) TRM(3);
#endif
  };

  // ---- stream
  if constexpr (MX4) {
    // MXFP4 (usdm_gemv_mxfp4_mfma).  Lane (r16, g) owns the same 8 elements of every chunk as in bf16; the image stores them as one
    // dword, the dwords of the four chunks of a quad side by side, so one 16-byte load fetches the lane's A fragments of a quad (a
    // wave instruction: 16 rows x 64 contiguous bytes) and one dword load the quad's four scales.  Each fragment is converted with
    // its own chunk's scale (mx4x8_to_bf16x8, exact) right before its MFMA, and a tile is ONE accumulation chain over the wave's
    // chunks in ascending order, as in every bf16 variant: the result equals the bf16 form on W' bit for bit.
    auto mul_quad = [&](f32x4 acc, const u32x4& c, unsigned s, const u32x4& x0, const u32x4& x1, const u32x4& x2, const u32x4& x3)
                        __attribute__((always_inline)) -> f32x4 {
      acc = mfma16(mx4x8_to_bf16x8<0>(c[0], s), x0, acc);
      acc = mfma16(mx4x8_to_bf16x8<1>(c[1], s), x1, acc);
      acc = mfma16(mx4x8_to_bf16x8<2>(c[2], s), x2, acc);
      return mfma16(mx4x8_to_bf16x8<3>(c[3], s), x3, acc);
    };
    if (!quads) {
      // a quad would straddle two waves (K = 512: 2 chunks per wave, K = 1792: 7): dword j of the quad's piece and the chunk's scale
      // byte, one tile's loads at a time (no model shape comes here)
      int t = next_tile(rem_cp);
      while (t >= 0) {
        const int row = row_of(t, r16);
        const uint8_t* cp = m.codes + (int64_t)row * m.ldc + g * 16;
        const uint8_t* sp = m.scales + (int64_t)row * m.lds + kca;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < cpw; c0 += CH) {
          unsigned cd[CH], sb[CH];
          u32x4 xd[HOLD ? 1 : CH];
#pragma unroll
          for (int u = 0; u < CH; ++u) {
            if (c0 + u < cpw) {
              const int kc = kca + c0 + u;
              cd[u] = *(const unsigned*)(cp + (kc >> 2) * 64 + (kc & 3) * 4);
              sb[u] = sp[c0 + u];
              if constexpr (!HOLD) xd[u] = xload(c0 + u);
            }
          }
#pragma unroll
          for (int u = 0; u < CH; ++u) {
            if (c0 + u < cpw) {
              if constexpr (HOLD) acc = mfma16(mx4x8_to_bf16x8<0>(cd[u], sb[u]), xf[u], acc);      // (held: cpw <= CH, one pass)
              else acc = mfma16(mx4x8_to_bf16x8<0>(cd[u], sb[u]), xd[u], acc);
            }
          }
        }
        finish_tile(t, acc);
        t = next_tile(rem_cp);
      }
    } else if constexpr (HOLD) {
      // held activations: the units of the first ND tiles are in flight since the prologue
      auto mul_tile = [&](auto SLOT) __attribute__((always_inline)) -> f32x4 {
        constexpr int s = decltype(SLOT)::value;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          if (q < nq) acc = mul_quad(acc, cq[s][q], sq[s][q], xf[4 * q], xf[4 * q + 1], xf[4 * q + 2], xf[4 * q + 3]);
        return acc;
      };
      if constexpr (KSPLIT) {
        // K split over workgroups: at most MTG_TRL tiles per workgroup (host), reduced and merged after the stream, as in bf16
        auto step = [&](auto SLOT) __attribute__((always_inline)) {
          constexpr int s = decltype(SLOT)::value;
          const int t = tm[s];
          const f32x4 acc = mul_tile(SLOT);
          tm[s] = next_tile(rem_ld);
          ld_tile(SLOT, tm[s]);
          keep_tile(t, acc);
        };
        while (tm[0] >= 0) each_slot(slots<ND>{}, step);
      } else {
        auto step = [&](auto SLOT) __attribute__((always_inline)) -> bool {
          constexpr int s = decltype(SLOT)::value;
          const int t = tm[s];
          if (t < 0) return false;
          (void)next_tile(rem_cp);                            // (rem_cp = the tiles after this one: finish_tile's "more")
          const f32x4 acc = mul_tile(SLOT);
          tm[s] = next_tile(rem_ld);
          ld_tile(SLOT, tm[s]);
          finish_tile(t, acc);
          return true;
        };
        while (all_slots(slots<ND>{}, step)) {}
      }
    } else {
      // activations streamed beside the weights (form 5 at K = 14336, any K > 4096 that is not split): a unit = one quad, its scale
      // dword and its four activation fragments; a ring of DS units inside a tile, refilled DS quads ahead
      constexpr int DS = 6;
      const int nq = cpw >> 2;
      u32x4 cq[DS], xq[DS][4];
      unsigned sq[DS];
      int t = next_tile(rem_cp);
      while (t >= 0) {
        const int row = row_of(t, r16);
        const u32x4* cp = (const u32x4*)(m.codes + (int64_t)row * m.ldc + kca * 16 + g * 16);
        const unsigned* sp = (const unsigned*)(m.scales + (int64_t)row * m.lds + kca);
        auto ld_quad = [&](int u, int q) __attribute__((always_inline)) {
          cq[u] = __builtin_nontemporal_load(cp + q * 4);
          sq[u] = sp[q];
#pragma unroll
          for (int j = 0; j < 4; ++j) xq[u][j] = xload(4 * q + j);
        };
#pragma unroll
        for (int u = 0; u < DS; ++u)
          if (u < nq) ld_quad(u, u);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int q0 = 0; q0 < nq; q0 += DS) {
#pragma unroll
          for (int u = 0; u < DS; ++u) {
            if (q0 + u < nq) {
              acc = mul_quad(acc, cq[u], sq[u], xq[u][0], xq[u][1], xq[u][2], xq[u][3]);
              if (q0 + u + DS < nq) ld_quad(u, q0 + u + DS);
            }
          }
        }
        finish_tile(t, acc);
        t = next_tile(rem_cp);
      }
    }
  } else if constexpr (FP8 && TRL) {
    char* tb = smem + TB_OFF + wave * 8192;                 // this wave's transposition buffer: [16 rows][ROW8 bytes], piece ^ row
    // wait for unit q (the younger units stay in flight), its rows -> LDS; returns the scale of this lane's row
    auto take8 = [&](auto SLOT) __attribute__((always_inline)) -> float {
      constexpr int q = decltype(SLOT)::value;
      asm volatile("s_waitcnt vmcnt(%5)" : "+v"(U8[q][0]), "+v"(U8[q][1]), "+v"(U8[q][2]), "+v"(U8[q][3]), "+v"(E8[q])
                   : "n"((NR8 - 1) * LPU8) : "memory");
      if constexpr (NL8 == 8) asm volatile("" : "+v"(U8[q][4]), "+v"(U8[q][5]), "+v"(U8[q][6]), "+v"(U8[q][7]));
      if constexpr (!HOLD)
        asm volatile("" : "+v"(X8[q][0]), "+v"(X8[q][1]), "+v"(X8[q][2]), "+v"(X8[q][3]), "+v"(X8[q][4]), "+v"(X8[q][5]), "+v"(X8[q][6]), "+v"(X8[q][7]));
      recut_store<ROW8>(tb, lane, U8[q]);
      return fp8_row_scale(E8[q]);
    };
    // chunk c of this lane's row as bf16, converted just before the MFMA
    auto frag8 = [&](int c, float s) __attribute__((always_inline)) -> u32x4 {
      return fp8x8_to_bf16x8(recut_frag<ROW8, u32x2>(tb, r16, g, c), s);
    };
    if constexpr (!HOLD) {
      // streamed activations (K = 14336): units numbered through the tiles, 7 per tile, in slot n % 3; the tile's chain runs over
      // its units in order, as in bf16
      unit_pos cu{next_tile(rem_cp), 0};
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      auto unit = [&](auto SLOT) __attribute__((always_inline)) -> bool {
        constexpr int q = decltype(SLOT)::value;
        if (cu.t < 0) return false;
        const float s = take8(SLOT);
#pragma unroll
        for (int c = 0; c < 8; ++c) acc = mfma16(frag8(c, s), X8[q][c], acc);
        ld_unit8(SLOT, lu.t, lu.s); adv_unit();
        const int t = cu.t;
        if (next_unit<UPT>(cu, [&]() { return next_tile(rem_cp); })) {
          finish_tile(t, acc);
          acc = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        return true;
      };
      while (unit(Q0{}) && unit(Q1{}) && unit(Q2{})) {}
    } else if constexpr (CPWT == 8) {
      // K split over workgroups: one unit per tile and wave, all (<= MTG) tiles of the workgroup in flight at once; reduced and merged
      // after the stream, as in bf16
      auto unit = [&](auto SLOT) __attribute__((always_inline)) {
        constexpr int q = decltype(SLOT)::value;
        const int t = tq8[q];
        const float s = take8(SLOT);
        tq8[q] = next_tile(rem_ld);
        ld_unit8(SLOT, tq8[q], 0);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; ++c) acc = mfma16(frag8(c, s), xf[c], acc);
        keep_tile(t, acc);
      };
      while (tq8[0] >= 0) each_slot(slots<NR8>{}, unit);
    } else {
      // K = 4096: one unit = one tile; refilled with the tile three further on
      auto tile8 = [&](auto SLOT) __attribute__((always_inline)) -> bool {
        constexpr int q = decltype(SLOT)::value;
        const int t = tq8[q];
        if (t < 0) return false;
        (void)next_tile(rem_cp);
        const float s = take8(SLOT);
        tq8[q] = next_tile(rem_ld);
        ld_unit8(SLOT, tq8[q], 0);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 16; ++c) acc = mfma16(frag8(c, s), xf[c], acc);
        finish_tile(t, acc);
        return true;
      };
      while (tile8(Q0{}) && tile8(Q1{}) && tile8(Q2{})) {}
    }
    if constexpr (HOLD) drain(U8, E8);
    else drain(U8, E8, X8);
  } else if constexpr (TRL && !HOLD) {
    char* tb = smem + TB_OFF + wave * 8192;
    unit_pos cu{next_tile(rem_cp), 0};                      // the unit being multiplied
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // one unit: its 16 loads have landed (the 32 younger ones stay in flight), rows -> LDS, fragments <- LDS, 8 MFMAs against the
    // unit's own activation fragments, then the slot is refilled with the unit three further on
    auto unit = [&](auto SLOT) __attribute__((always_inline)) -> bool {
      constexpr int q = decltype(SLOT)::value;
      if (cu.t < 0) return false;
      asm volatile("s_waitcnt vmcnt(%8)" : "+v"(U[q][0]), "+v"(U[q][1]), "+v"(U[q][2]), "+v"(U[q][3]), "+v"(U[q][4]), "+v"(U[q][5]), "+v"(U[q][6]), "+v"(U[q][7])
                   : "n"((NR - 1) * 16) : "memory");
      asm volatile("" : "+v"(X[q][0]), "+v"(X[q][1]), "+v"(X[q][2]), "+v"(X[q][3]), "+v"(X[q][4]), "+v"(X[q][5]), "+v"(X[q][6]), "+v"(X[q][7]));
      recut_store<512>(tb, lane, U[q]);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const u32x4 f = recut_frag<512, u32x4>(tb, r16, g, c);
        acc = mfma16(f, X[q][c], acc);
      }
      ld_unit_x(SLOT, lu.t, lu.s); adv_unit();
      const int t = cu.t;
      if (next_unit<UPT>(cu, [&]() { return next_tile(rem_cp); })) {
        finish_tile(t, acc);
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      return true;
    };
    while (unit(Q0{}) && unit(Q1{})) {}
    drain(U, X);
  } else if constexpr (TRL && CPWT == 8) {
    // K split over workgroups: ONE unit per tile and wave (16 rows x 512 bytes of this wave's 256 K), four tiles in flight; tile n
    // sits in slot n % 4 and is refilled with tile n + 4 as soon as its rows are in LDS
    char* tb = smem + TB_OFF + wave * 8192;
    // A round of four units is straight-line code: a unit whose tile does not exist (only behind the last tile: tiles are dealt to
    // the slots in order) still waits, multiplies its placeholder lines and refills - only the hand-over of the result is conditional.
    auto unit = [&](auto SLOT) __attribute__((always_inline)) {
      constexpr int q = decltype(SLOT)::value;
      const int t = tq[q];
      asm volatile("s_waitcnt vmcnt(%8)" : "+v"(U[q][0]), "+v"(U[q][1]), "+v"(U[q][2]), "+v"(U[q][3]), "+v"(U[q][4]), "+v"(U[q][5]), "+v"(U[q][6]), "+v"(U[q][7])
                   : "n"((NR - 1) * 8) : "memory");
      recut_store<512>(tb, lane, U[q]);
      tq[q] = next_tile(rem_ld);
#pragma unroll
      for (int i = 0; i < 8; ++i) ld_nt_asm(U[q][i], unit_ptr(tq[q], 0, i));
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const u32x4 f = recut_frag<512, u32x4>(tb, r16, g, c);
        acc = mfma16(f, xf[c], acc);
      }
      keep_tile(t, acc);      // at most MTG tiles per workgroup (host): reduced and merged after the stream, when the load registers are free
    };
    while (tq[0] >= 0) { unit(Q0{}); unit(Q1{}); unit(Q2{}); unit(Q3{}); }
    drain(U);
  } else if constexpr (TRL) {
    char* tb = smem + TB_OFF + wave * 8192;                 // this wave's transposition buffer: [16 rows][32 pieces of 16 B], piece ^ row
    // one unit: wait for its 8 loads (the 24 younger ones stay in flight), rows -> LDS, refill the registers with the same unit of the
    // tile after next, fragments <- LDS, 8 MFMAs.  LDS operations of one wave execute in order: no wait between the writes and the
    // reads, nor between these reads and the next unit's writes.
    // Unit n = (tile n / 2, half n % 2) sits in slot n % 3 and is refilled with unit n + 3 = (next tile, half 1) behind half 0,
    // (tile after next, half 0) behind half 1.
    auto unit = [&](auto SLOT, auto SUB, f32x4& acc, int tnext) __attribute__((always_inline)) {
      constexpr int q = decltype(SLOT)::value, sub = decltype(SUB)::value;
      asm volatile("s_waitcnt vmcnt(%8)" : "+v"(U[q][0]), "+v"(U[q][1]), "+v"(U[q][2]), "+v"(U[q][3]), "+v"(U[q][4]), "+v"(U[q][5]), "+v"(U[q][6]), "+v"(U[q][7])
                   : "n"((NR - 1) * 8) : "memory");
      recut_store<512>(tb, lane, U[q]);
#pragma unroll
      for (int i = 0; i < 8; ++i) ld_nt_asm(U[q][i], unit_ptr(tnext, 1 - sub, i));
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const u32x4 f = recut_frag<512, u32x4>(tb, r16, g, c);
        acc = mfma16(f, xf[sub * 8 + c], acc);
      }
    };
    // one tile at ring phase P (its halves sit in slots 2 P % 3 and (2 P + 1) % 3); false after the last tile
    auto ttile = [&](auto S0, auto S1) __attribute__((always_inline)) -> bool {
      if (ua < 0) return false;
      (void)next_tile(rem_cp);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      unit(S0, Q0{}, acc, ub);
      unit(S1, Q1{}, acc, uc);
      finish_tile(ua, acc);
      ua = ub; ub = uc; uc = next_tile(rem_ld);
      return true;
    };
    while (ttile(Q0{}, Q1{}) && ttile(Q2{}, Q0{}) && ttile(Q1{}, Q2{})) {}
    drain(U);
  } else if constexpr (HOLD) {
    // one tile at ring phase P (its chunk c sits in slot (16 P + c) % 24); returns false after the last tile
    auto tile_phase = [&](auto P, auto STATIC) __attribute__((always_inline)) -> bool {
      constexpr int ph = decltype(P)::value;
      constexpr bool stat = decltype(STATIC)::value;
      if (t0 < 0) return false;
      (void)next_tile(rem_cp);                               // (rem_cp = the tiles after this one: finish_tile's "more")
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int sl = (CH * ph + c) % RS;
        if (c < cpw) {
          // item + 24 = (next tile, chunk c + 8) for c < 8, (tile after next, chunk c - 8) otherwise
          const wvec* np = c < RS - CH ? wp1 + (c + (RS - CH)) * 4 : wp2 + (c - (RS - CH)) * 4;
          if constexpr (stat) {
            if (c == 0) wait_mfma_asm<RS - 1, true>(acc, ring[sl], xf[c]);
            else wait_mfma_asm<RS - 1, false>(acc, ring[sl], xf[c]);
            ld_nt_asm(ring[sl], np);
          } else {
            acc = mfma16(wfrag(ring[sl], sc0), xf[c], acc);
            if ((c < RS - CH ? c + (RS - CH) : c - (RS - CH)) < cpw) ring[sl] = __builtin_nontemporal_load(np);
            __builtin_amdgcn_sched_barrier(0);               // keep (multiply, refill) pairs in program order
          }
        }
      }
      if constexpr (stat) {                                  // straight-line part: at most MTG tiles, no flush in between
        asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc));     // the last MFMA's result before the compiler's own code reads it
        keep_tile(t0, acc);
      } else {
        finish_tile(t0, acc);
      }
      t0 = t1; t1 = t2; wp1 = wp2;
      t2 = next_tile(rem_ld);
      wp2 = wbase(t2);
      if constexpr (FP8) { sc0 = sc1; sc1 = sc2; sc2 = wscale(t2); }
      return true;
    };
    if constexpr (ASM_STREAM) {
      // The first 12 tiles (every production launch has at most 11 per workgroup) as STRAIGHT-LINE code with hand-counted loads.
      // Left to the compiler, the wait-count pass puts vmcnt(7) in front of the first eight MFMAs of every tile - in the looped AND in
      // the straight-line form, with the (multiply, refill) pairs pinned in program order - although 23 younger loads are in flight:
      // the ring drains to a third every tile (measured: 3.0 TB/s against 5.9 for the batch-1 kernel).  The ring's first fill above is
      // hand-counted as well (a compiler-issued fill would be waited for with counts that ignore the asm loads: a full drain).
      static_assert(MTG >= 12 || TRL, "the straight-line part must fit one reduction group");
      using T = std::true_type;
      do {
        if (!tile_phase(Q0{}, T{})) break; if (!tile_phase(Q1{}, T{})) break; if (!tile_phase(Q2{}, T{})) break;
        if (!tile_phase(Q0{}, T{})) break; if (!tile_phase(Q1{}, T{})) break; if (!tile_phase(Q2{}, T{})) break;
        if (!tile_phase(Q0{}, T{})) break; if (!tile_phase(Q1{}, T{})) break; if (!tile_phase(Q2{}, T{})) break;
        if (!tile_phase(Q0{}, T{})) break; if (!tile_phase(Q1{}, T{})) break; if (!tile_phase(Q2{}, T{})) break;
      } while (false);
      // (not drain(ring): naming the 24 registers behind the wait instead of in it gave this instantiation one more s_nop - class C)
      asm volatile("s_waitcnt vmcnt(0)" ::"v"(ring[0]), "v"(ring[1]), "v"(ring[2]), "v"(ring[3]), "v"(ring[4]), "v"(ring[5]), "v"(ring[6]), "v"(ring[7]),
                   "v"(ring[8]), "v"(ring[9]), "v"(ring[10]), "v"(ring[11]), "v"(ring[12]), "v"(ring[13]), "v"(ring[14]), "v"(ring[15]),
                   "v"(ring[16]), "v"(ring[17]), "v"(ring[18]), "v"(ring[19]), "v"(ring[20]), "v"(ring[21]), "v"(ring[22]), "v"(ring[23])
                   : "memory");
    }
    using F = std::false_type;
    while (tile_phase(Q0{}, F{}) && tile_phase(Q1{}, F{}) && tile_phase(Q2{}, F{})) {}
  } else {
    // activations streamed beside the weights (K slices longer than CH chunks: down_proj): a ring of CH (weight, activation) pairs,
    // each refilled CH chunks ahead as soon as it has been multiplied
    int t = next_tile(rem_cp);
    const wvec* wp = wp0;
    while (t >= 0) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int c0 = 0; c0 < cpw; c0 += CH) {
#pragma unroll
        for (int u = 0; u < CH; ++u) {
          if (c0 + u < cpw) {
            acc = mfma16(wfrag(ring[u], sc0), rx[u], acc);
            const int cn = c0 + u + CH;
            if (cn < cpw) { ring[u] = wload(wp, cn); rx[u] = xload(cn); }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      finish_tile(t, acc);
      t = next_tile(rem_cp);
      wp = wbase(t);
      if constexpr (FP8) sc0 = wscale(t);
#pragma unroll
      for (int c = 0; c < CH; ++c)
        if (c < cpw) { ring[c] = wload(wp, c); rx[c] = xload(c); }
    }
  }
  TRM(4);
  if (done % MTG || (KSPLIT && done)) flush_group(false);
#ifdef USDM_MFMA_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TRM(6);
#endif

  // ---- lm_head: per-workgroup arg-max partial of every sequence (ties -> lowest id); unused partial slots keep "no candidate"
  if (lmh) {
    __syncthreads();
    if (g == 0) { sv[wave * 16 + r16] = bestv; si[wave * 16 + r16] = besti; }
    __syncthreads();
    if (tid < nb) {
      float bv = sv[tid];
      int bi = si[tid];
      for (int w = 1; w < MW; ++w) {
        const float v = sv[w * 16 + tid];
        const int i = si[w * 16 + tid];
        if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
      }
      a.part_val[(int64_t)tid * d.ba.part_bs + blockIdx.x] = bv;
      a.part_idx[(int64_t)tid * d.ba.part_bs + blockIdx.x] = bi == 0x7fffffff ? bi : bi + a.idx_offset;
      for (int j = blockIdx.x + d.grid; j < d.ba.part_bs; j += d.grid) {
        a.part_val[(int64_t)tid * d.ba.part_bs + j] = -INFINITY;
        a.part_idx[(int64_t)tid * d.ba.part_bs + j] = 0x7fffffff;
      }
    }
  }
}

}  // namespace

#ifdef USDM_MFMA_TRACE
extern "C" int usdm_dbg_mfma_trace(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mfma_trace), sizeof(unsigned long long) * n);
}
#endif

extern "C" int64_t usdm_gemv_batch_ks_floats(int32_t N, int32_t K) {
  if (K <= MW * CH * 32 || K % KS_K != 0 || K / KS_K > KS_MAX || N <= 0) return 0;
  return (int64_t)cdiv(N, 16) * (K / KS_K) * 256;
}

namespace {
enum { MFMA_BF16 = 0, MFMA_FP8 = 1, MFMA_MX4 = 2 };
// floats of ks_part if the launch may split K over workgroups (given the ks_* buffers), else 0
int64_t mfma_ks_floats(int N, int K, bool glu, bool norm, bool lmh, int form) {
  return !glu && !lmh && !norm && form != 3 && form != 5 ? usdm_gemv_batch_ks_floats(N, K) : 0;
}

// The matrix-core launch selection: tiles, rows per tile, K split, K chunks per wave, grid and kernel variant of a shape - the same
// decisions for usdm_gemv_batch (bf16), usdm_gemv_fp8_mfma and usdm_gemv_mxfp4_mfma.  Host only (usdm_gemv_mfma_select asks it where
// there is no device); refuses, with the launcher's message, the shapes the launcher refuses.
int mfma_select(const char* who, int N, int K, bool glu, bool norm, bool lmh, bool ks_given, int form, int fmt, usdm_gemv_mfma_plan& p) {
  USDM_CHECK_ARG(K % (MW * 32) == 0, "%s (matrix-core form): K %% %d, ldw %% 8, x stride %% 8", who, MW * 32);
  p.cpw = cdiv(K / 32, MW);
  const bool hold = p.cpw <= CH;
  USDM_CHECK_ARG(!norm || (hold && K <= GAM_FLOATS && K % 4 == 0), "%s (matrix-core form): the fused RMSNorm needs K <= 4096", who);
  USDM_CHECK_ARG(!glu || N % 32 == 0, "%s (matrix-core form): swiglu needs N %% 32 == 0 (packed gate/up rows)", who);   // (else the last up rows lie past W)
  p.nout = glu ? N / 2 : N;
  p.rt = 16;
  p.ksplit = 1;
  if (ks_given && mfma_ks_floats(N, K, glu, norm, lmh, form)) {
    p.ksplit = K / KS_K;
    if (cdiv(cdiv(N, 16), min(256 / p.ksplit, cdiv(N, 16))) > MTG_TRL) p.ksplit = 1;      // one reduction group per workgroup
  }
  if (glu) {
    p.ntiles = cdiv(p.nout, 8);
  } else if (lmh) {
    p.ntiles = cdiv(N, 16);
  } else {
    // rows per tile: 16, or 12 / 8 where that shortens the longest workgroup (N = 6144: 384 tiles of 16 = 2 rounds of 16 rows, 512
    // tiles of 12 = 2 rounds of 12)
    int best = 1 << 30;
    for (int rt : {16, 12, 8}) {
      const int nt = cdiv(N, rt), per = cdiv(nt, nt < 256 ? nt : 256) * rt;
      if (per < best) { best = per; p.rt = rt; }
    }
    p.ntiles = cdiv(N, p.rt);
  }
  p.grid = p.ntiles < 256 ? p.ntiles : 256;
  p.kwg = p.grid;
  if (p.ksplit > 1) {      // 16-row tiles; 256 / ksplit workgroups per slice, each with every kwg-th tile
    p.rt = 16;
    p.ntiles = cdiv(N, 16);
    p.kwg = min(256 / p.ksplit, p.ntiles);
    p.grid = p.kwg * p.ksplit;
    p.cpw = KS_K / 32 / MW;
  }
  USDM_CHECK_ARG(cdiv(p.ntiles, p.kwg) <= 64, "%s (matrix-core form): N too large (more than 64 tiles per workgroup)", who);
  // The variant.  K = 4096 (every RMSNorm-fed projection and o_proj of the 7B) and K = 14336: K chunks per wave as a constant and
  // row-contiguous loads re-cut through LDS; form 3 forces the fragment-shaped loads there (A/B: tools/gemv_mfma_bench.py).  MXFP4:
  // the image is cut into fragments already - no re-cut, constants for K = 4096 and the K split only.
  const bool mx4 = fmt == MFMA_MX4, fixed = p.ksplit == 1 && p.cpw == (hold ? 16 : 56);
  p.hold = hold || p.ksplit > 1;
  p.trl = !mx4 && (p.ksplit > 1 || (fixed && form != 3));
  p.cpwt = p.ksplit > 1 ? 8 : fixed && !(mx4 && !hold) ? p.cpw : 0;
  if (fmt == MFMA_FP8 && !p.trl) p.cpwt = 0;      // (FP8 has no fragment-shaped variant with constant chunks: they are form 3, bf16 only)
  p.lds_bytes = p.trl ? LDS_BYTES_TRL : LDS_BYTES;
  return 0;
}

// Every instantiation of gemv_mfma_kernel, named here and nowhere else: X(HOLD, CPWT, TRL, format).  A new format or schedule adds
// its lines here; mfma_select is what picks among them.
#define USDM_MFMA_VARIANTS(X)                                                                                          \
  X(true, 0, false, MFMA_BF16) X(true, 16, false, MFMA_BF16) X(true, 16, true, MFMA_BF16) X(true, 8, true, MFMA_BF16)   \
  X(false, 0, false, MFMA_BF16) X(false, 56, false, MFMA_BF16) X(false, 56, true, MFMA_BF16)                            \
  X(true, 0, false, MFMA_FP8) X(true, 16, true, MFMA_FP8) X(true, 8, true, MFMA_FP8)                                    \
  X(false, 0, false, MFMA_FP8) X(false, 56, true, MFMA_FP8)                                                            \
  X(true, 0, false, MFMA_MX4) X(true, 16, false, MFMA_MX4) X(true, 8, false, MFMA_MX4) X(false, 0, false, MFMA_MX4)

// sets the dynamic-LDS limit of its own instantiation once (a function-local static: initialised once under any number of host
// threads) and launches it
template <bool HOLD, int CPWT, bool TRL, bool FP8, class... FMT>
int launch_one(const MfmaDev& d, hipStream_t st, FMT... fmt) {
  constexpr int lds = TRL ? LDS_BYTES_TRL : LDS_BYTES;
  static const hipError_t attr =
      hipFuncSetAttribute((const void*)gemv_mfma_kernel<HOLD, CPWT, TRL, FP8, FMT...>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  (void)attr;
  hipLaunchKernelGGL((gemv_mfma_kernel<HOLD, CPWT, TRL, FP8, FMT...>), dim3(d.grid), dim3(MW * 64), lds, st, d, fmt...);
  USDM_LAUNCH_CHECK();
  return 0;
}

// the matrix-core launch of usdm_gemv_batch (bf16), usdm_gemv_fp8_mfma (FP8: fmt = the row exponents) and usdm_gemv_mxfp4_mfma
// (fmt = gemv_mx4mc; a.W / a.ldw stand in for a bf16 matrix of the same shape): checks the buffers, asks mfma_select, launches
template <bool FP8, class... FMT>
int mfma_launch(const usdm_gemv_batch_args* pa, hipStream_t st, const char* who, FMT... fmt) {
  constexpr int FMT_ID = gemv_is_mx4mc<FMT...>::value ? MFMA_MX4 : FP8 ? MFMA_FP8 : MFMA_BF16;
  const usdm_gemv_args& a = pa->g;
  USDM_CHECK_ARG(pa->nb >= 1 && pa->nb <= 16, "%s (matrix-core form): 1..16 sequences per step", who);
  USDM_CHECK_ARG(a.K % (MW * 32) == 0 && a.ldw % 8 == 0 && a.ldw >= a.K && pa->x_bs % 8 == 0,
                 "%s (matrix-core form): K %% %d, ldw %% 8, x stride %% 8", who, MW * 32);
  const bool glu = a.act == USDM_ACT_SWIGLU, lmh = a.part_val != nullptr;
  USDM_CHECK_ARG(!lmh || (a.part_idx && !glu), "%s: lm_head partial buffers", who);
  usdm_gemv_mfma_plan p;
  if (const int rc = mfma_select(who, a.N, a.K, glu, a.norm_w != nullptr, lmh, pa->ks_part && pa->ks_cnt, pa->form, FMT_ID, p)) return rc;
  if (pa->ks_part && pa->ks_cnt) {
    const int64_t ksf = mfma_ks_floats(a.N, a.K, glu, a.norm_w != nullptr, lmh, pa->form);
    USDM_CHECK_ARG(!ksf || (pa->ks_part_floats >= ksf && (((uintptr_t)pa->ks_part) & 15) == 0), "%s: ks_part must hold %lld floats (16-byte aligned)", who, (long long)ksf);
  }
  USDM_CHECK_ARG(!lmh || pa->part_bs >= p.grid, "%s: part_bs must hold one partial per workgroup (%d)", who, p.grid);
  MfmaDev d;
  d.ba = *pa;
  d.ntiles = p.ntiles; d.rt = p.rt; d.cpw = p.cpw; d.nchunks = a.K / 32; d.grid = p.grid; d.nout = p.nout;
  d.ksplit = p.ksplit; d.kwg = p.kwg;
#define USDM_MFMA_CASE(HOLD, CPWT, TRL, F)                                         \
  if constexpr (F == FMT_ID)                                                       \
    if (p.hold == HOLD && p.cpwt == CPWT && p.trl == TRL) return launch_one<HOLD, CPWT, TRL, FP8, FMT...>(d, st, fmt...);
  USDM_MFMA_VARIANTS(USDM_MFMA_CASE)
#undef USDM_MFMA_CASE
  usdm_set_error("%s: no instantiation for hold %d, %d chunks per wave, re-cut %d", __FILE__, p.hold, p.cpwt, p.trl);      // a mistake in mfma_select
  return 1;
}

// the argument checks the two quantized entry points share
int mfma_check_quantized(const char* who, const usdm_gemv_batch_args& b) {
  const usdm_gemv_args& a = b.g;
  USDM_CHECK_ARG(b.nb >= 1 && b.nb <= 16, "%s: 1..16 sequences per step", who);
  USDM_CHECK_ARG(b.form == 0 || b.form == 5, "%s: form 0 (K split where ks_* allow it) or 5 (no K split)", who);
  USDM_CHECK_ARG(!a.p2p && !a.p2p_mode && !a.mrg_po && !a.mrg_pm && !a.mrg_pl && !a.cmb_gran && !a.x_delta && !a.x_out,
                 "%s: p2p / merged-attention input / cmb_gran / x_delta are not supported", who);
  USDM_CHECK_ARG(a.act != USDM_ACT_SWIGLU || a.N % 32 == 0, "%s: swiglu needs N %% 32 == 0 (packed gate/up rows)", who);
  return 0;
}
}  // namespace

// called by usdm_gemv_batch (llm_batch_k.hip) for 5..16 sequences, or when the caller forces the matrix-core form
int usdm_gemv_mfma_launch(const usdm_gemv_batch_args* pa, hipStream_t st) { return mfma_launch<false>(pa, st, "usdm_gemv_batch"); }

extern "C" int usdm_gemv_mfma_select(int32_t N, int32_t K, int32_t flags, int32_t form, int32_t fmt, usdm_gemv_mfma_plan* out) {
  USDM_CHECK_ARG(out && N > 0 && K > 0 && fmt >= MFMA_BF16 && fmt <= MFMA_MX4 && (flags & ~15) == 0 && !((flags & 1) && (flags & 4)),
                 "usdm_gemv_mfma_select: null plan, bad N / K / flags, or fmt not 0 (bf16), 1 (FP8), 2 (MXFP4)");
  return mfma_select("usdm_gemv_mfma_select", N, K, flags & 1, flags & 2, flags & 4, flags & 8, form, fmt, *out);
}
extern "C" int usdm_sizeof_gemv_mfma_plan(void) { return (int)sizeof(usdm_gemv_mfma_plan); }

extern "C" int usdm_gemv_fp8_mfma(const usdm_gemv_fp8_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->b.g.W && pa->b.g.x && pa->row_exp, "usdm_gemv_fp8_mfma: null args");
  const usdm_gemv_batch_args& b = pa->b;
  const usdm_gemv_args& a = b.g;
  if (const int rc = mfma_check_quantized("usdm_gemv_fp8_mfma", b)) return rc;
  USDM_CHECK_ARG(a.N > 0 && a.K > 0 && a.ldw % 16 == 0 && ((uintptr_t)a.W & 15) == 0 && ((uintptr_t)a.x & 15) == 0,
                 "usdm_gemv_fp8_mfma: bad N/K, or W / ldw / x not 16-byte aligned");
  USDM_CHECK_ARG(a.y16 || a.y32 || a.part_val, "usdm_gemv_fp8_mfma: no output");
  return mfma_launch<true>(&b, (hipStream_t)stream, "usdm_gemv_fp8_mfma", pa->row_exp);
}

extern "C" int usdm_gemv_mxfp4_mfma(const usdm_gemv_mxfp4_mfma_args* pa, usdm_stream_t stream) {
  USDM_CHECK_ARG(pa && pa->codes && pa->scales && pa->b.g.x, "usdm_gemv_mxfp4_mfma: null args");
  usdm_gemv_batch_args b = pa->b;
  usdm_gemv_args& a = b.g;
  if (const int rc = mfma_check_quantized("usdm_gemv_mxfp4_mfma", b)) return rc;
  USDM_CHECK_ARG(!a.part_val && !a.part_idx && !a.ban && !a.y32, "usdm_gemv_mxfp4_mfma: the lm_head mode (part_val / ban / y32) is not supported with MXFP4 weights");
  USDM_CHECK_ARG(a.N > 0 && a.K > 0 && a.K % (MW * 32) == 0, "usdm_gemv_mxfp4_mfma: bad N, or K not a multiple of %d", MW * 32);
  USDM_CHECK_ARG(pa->ldc % 16 == 0 && pa->ldc >= a.K / 2 && pa->lds % 4 == 0 && pa->lds >= a.K / 32,
                 "usdm_gemv_mxfp4_mfma: ldc (bytes) must be a multiple of 16 and hold K / 2, lds a multiple of 4 and hold K / 32");
  USDM_CHECK_ARG(((uintptr_t)pa->codes & 15) == 0 && ((uintptr_t)pa->scales & 3) == 0 && ((uintptr_t)a.x & 15) == 0,
                 "usdm_gemv_mxfp4_mfma: codes and x must be 16-byte, scales 4-byte aligned");
  USDM_CHECK_ARG(a.y16, "usdm_gemv_mxfp4_mfma: no output (y16)");
  a.W = pa->codes;      // (the kernel reads the image through its own argument; the launcher's shape checks see a [N][K] matrix)
  a.ldw = a.K;
  return mfma_launch<false>(&b, (hipStream_t)stream, "usdm_gemv_mxfp4_mfma", gemv_mx4mc{(const uint8_t*)pa->codes, pa->scales, pa->ldc, pa->lds});
}

extern "C" int usdm_sizeof_gemv_mxfp4_mfma_args(void) { return (int)sizeof(usdm_gemv_mxfp4_mfma_args); }
