// Host side of the decode GEMVs: the launch selection (which instantiation and grid run a shape) and the argument checks that the
// launchers of llm_k.hip and llm_batch_k.hip share.
#pragma once
#include "gemv_common.h"

namespace {
// ---- launch selection: the instantiation (rows per wave, waves per workgroup, GLU) and the grid that run a shape.  The launchers,
// usdm_gemv_threads and through it usdm_gemv_engine (which reproduces the RMSNorm partition) all read this one table.
// res: 0 = one tile per workgroup (grid = tiles); > 0 = the batch-1 bf16 launcher may run the tiles RESIDENT (gemv_resident_kernel)
// on at most that many workgroups - how many the device holds at once is its question, asked at the launch, not here (this table
// is also read where there is no device).
// stream: the batch-1 bf16 launcher runs the row's straight-line form (gemv_stream_kernel) - the same workgroups, rows and threads
// as gemv_kernel<1, false, 16>, which every other launcher of the row runs.
struct gemv_sel { int rw, nwv; bool glu; int grid; int res; bool stream; };

// Rows per wave: HBM streaming wants >= ~4 workgroups (16 waves) per CU in flight AND a grid that is a whole
// number of workgroups per CU (256 CUs); take the largest RW that gives both, else the best balanced one.
static int gemv_pick_rw(int nout, bool glu) {
  const int ncand = glu ? 2 : 4;
  const int cands[4] = {glu ? 2 : 4, glu ? 1 : 3, 2, 1};
  int best = cands[ncand - 1];
  double best_score = -1.0;
  for (int c = 0; c < ncand; ++c) {
    const int rw = cands[c];
    const int blocks = cdiv(nout, 4 * rw);
    const double eff = (blocks / 256.0) / (double)((blocks + 255) / 256);  // 1.0 = perfectly balanced
    if (blocks >= 1024 && eff >= 0.9) return rw;
    const double score = eff * (blocks >= 512 ? 1.0 : 0.5 + blocks / 1024.0);
    if (score > best_score) { best_score = score; best = rw; }
  }
  return best;
}

static gemv_sel gemv_select(const usdm_gemv_args& a, bool batched) {
  const bool glu = a.act == USDM_ACT_SWIGLU;
  const int nout = glu ? a.N / 2 : a.N;
  const int rows_per_cu = nout % 256 == 0 ? nout / 256 : 0;
  // Wide workgroups for the mid-size projections: one workgroup per CU with 12-16 waves stages x (and the fused RMSNorm) once per
  // 16-24 rows instead of once per 4, at the same number of loads in flight.
  const gemv_sel wide16{1, 16, false, 256}, wide12{2, 12, false, 256};
  // batch-1 only: the merged-attention input (also its cmb_gran hand-off form) and / or the peer-to-peer all-reduce epilogue have
  // the 4096-output shape of the 7B or the general one-row form
  if (!batched && (a.mrg_po || a.p2p_mode)) return rows_per_cu == 16 ? wide16 : gemv_sel{1, 4, false, cdiv(nout, 4)};
  // down_proj of the 7B (K = 14336: 28 K iterations per row, 20 ring refills per lane), batch-1 only: the wide16 row in its
  // straight-line form, whose weight ring stays in flight through the K loop (llm_k.hip gemv_stream_kernel)
  // usdm_gemv_args.resident at this K and form: 0 = where wide16 applies; -1 = gemv_kernel; > 0 = at every N, one workgroup per 16 rows
  const bool stream = !batched && !glu && !a.part_val && a.K == 14336 && !a.norm_w && !a.x_delta && a.resident >= 0;
  if (stream && a.resident > 0) return gemv_sel{1, 16, false, cdiv(nout, 16), 0, true};
  if (!glu && !a.part_val && rows_per_cu == 16) return gemv_sel{1, 16, false, 256, 0, stream};
  if (!glu && !a.part_val && rows_per_cu == 24) return wide12;
  // gate/up of the 7B (14336 outputs), batch-1 only: 7-wave workgroups of 14 outputs = 1024 workgroups = exactly two rounds of two
  // workgroups per CU, instead of 1792 four-wave workgroups = 1.75 rounds of four
  // (a 14-wave GLU variant with one workgroup per CU was measured 15 % slower than 7 four-wave workgroups per CU)
  // usdm_gemv_args.resident: 0 = resident where this row applies; -1 = one tile per workgroup; > 0 = resident on at most that many
  // workgroups; non-zero: this row at every SwiGLU shape (the last tile may be ragged)
  if (!batched && glu && (a.resident != 0 || (nout % 14 == 0 && (nout / 14) % 512 == 0)))
    return gemv_sel{2, 7, true, cdiv(nout, 14), a.resident < 0 ? 0 : a.resident > 0 ? a.resident : 0x7fffffff};
  const int rw = a.part_val ? 4 : gemv_pick_rw(nout, glu);   // lm_head: 4 rows
  return gemv_sel{rw, 4, glu, cdiv(nout, 4 * rw)};
}

// The supported (RW, GLU, NWV) instantiations and the forms that have each: PLAIN = batch-1 single-GPU (every weight format),
// BATCH = gemv_batch_kernel, MRG = merged-attention input and / or peer-to-peer epilogue, CMB = the hand-off form.
enum { GEMV_PLAIN = 1, GEMV_BATCH = 2, GEMV_MRG = 4, GEMV_CMB = 8 };
#define USDM_GEMV_SHAPES(X)                                   \
  X(1, false, 16, GEMV_PLAIN | GEMV_BATCH | GEMV_MRG | GEMV_CMB) \
  X(2, false, 12, GEMV_PLAIN | GEMV_BATCH)                    \
  X(2, true, 7, GEMV_PLAIN)                                   \
  X(4, false, 4, GEMV_PLAIN | GEMV_BATCH)                     \
  X(3, false, 4, GEMV_PLAIN | GEMV_BATCH)                     \
  X(2, false, 4, GEMV_PLAIN | GEMV_BATCH)                     \
  X(1, false, 4, GEMV_PLAIN | GEMV_BATCH | GEMV_MRG)          \
  X(2, true, 4, GEMV_PLAIN | GEMV_BATCH)                      \
  X(1, true, 4, GEMV_PLAIN | GEMV_BATCH)
// calls launch(gemv_ic<RW>, gemv_ic<GLU>, gemv_ic<NWV>) for the selection's tuple; false if FORM has no such instantiation
template <int FORM, class LAUNCH>
static bool gemv_dispatch(const gemv_sel& s, LAUNCH&& launch) {
#define USDM_GEMV_CASE(RW, GLU, NWV, FORMS)                                      \
  if constexpr (((FORMS) & FORM) != 0)                                           \
    if (s.rw == RW && s.glu == GLU && s.nwv == NWV) {                            \
      launch(gemv_ic<RW>{}, gemv_ic<GLU>{}, gemv_ic<NWV>{});                     \
      return true;                                                               \
    }
  USDM_GEMV_SHAPES(USDM_GEMV_CASE)
#undef USDM_GEMV_CASE
  return false;
}

// gemv_select named a tuple that FORM's part of USDM_GEMV_SHAPES lacks: a mistake in this file, never the caller's
static int gemv_no_instantiation(const gemv_sel& s) {
  usdm_set_error("%s: no instantiation for %d rows per wave, GLU %d, %d waves", __FILE__, s.rw, (int)s.glu, s.nwv);
  return 1;
}

// ---- the argument checks the launchers share; `who` is the entry point's name as its messages carry it.
// The shape, for the formats that count K and ldw in elements; x_noun: what the K limit protects ("input vector" / "input vectors")
static int gemv_check_shape(const char* who, const usdm_gemv_args& a, const char* x_noun) {
  USDM_CHECK_ARG(a.N > 0 && a.K > 0 && a.K % 8 == 0 && a.ldw % 8 == 0 && a.ldw >= a.K, "%s: bad N/K/ldw", who);
  USDM_CHECK_ARG(a.K <= 16384, "%s: K too large for the LDS-resident %s", who, x_noun);
  USDM_CHECK_ARG(a.act != USDM_ACT_SWIGLU || a.N % 32 == 0, "%s: swiglu needs N %% 32 == 0", who);
  return 0;
}
// The outputs of a batch-1 entry point
static int gemv_check_outputs(const char* who, const usdm_gemv_args& a) {
  USDM_CHECK_ARG(a.y16 || a.y32 || a.part_val, "%s: no output", who);
  USDM_CHECK_ARG(!a.part_val || (a.part_idx && a.act != USDM_ACT_SWIGLU), "%s: part_idx missing / lm_head mode is not GLU", who);
  return 0;
}
}  // namespace
