// Host side of mx_gemm / mx_conv3x3: what a descriptor runs (GemmRoute / GemmPlan), whether it may run (validate), the kernel argument
// block (fill_args) and the launch.  No kernel lives here: the families' launchers are in gemm_bf16.hip (generic), gemm_bf16_v2.hip (128-row
// tiles), gemm_bf16_v5.hip (256-row tiles), gemm_bf16_v4.hip (persistent 256 x 256), gemm_small_m.hip and conv_small_n.hip.
//
// One decision, stated once: plan_of(d, conv) is the only caller of the tile chooser.  mx_gemm / mx_conv3x3 launch what it returns and the
// eight host queries (mx_gemm_form, _launches, _stats_slabs, _ln_prefers_pass, _gn_partials_supported, _ln_final_supported, _splitk,
// _kernel_name) read their answers from the same plan, so a query cannot disagree with the launch.  tests/test_gemm_route_cpu.py holds every
// answer to a recorded table (tests/golden/gemm_route_table.json).
#include <algorithm>
#include <cstdlib>

#include <mutex>
#include <unordered_map>

#include "common.h"
#include "../../include/mxdenoise.h"
#include "gemm_args.h"
#include "gemm_forms.h"

namespace mx {

// the family launchers start the instantiation `form` (gemm_forms.h) and return non-zero for a form outside their list
int launch_generic(hipStream_t s, const GemmArgs& a, int form);
int launch_v2(hipStream_t s, const GemmArgs& a, int form);
int launch_v5(hipStream_t s, const GemmArgs& a, int form);
int launch_v4(hipStream_t s, const GemmArgs& a, int form);
int launch_small_m(hipStream_t s, const GemmArgs& a, int form);
int launch_conv_small_n(hipStream_t s, const GemmArgs& a, int form);
int launch_conv_small_cin(hipStream_t s, const GemmArgs& a, int form);
bool small_m_serves(const mx_gemm_desc* d, bool conv);      // gemm_small_m.hip: M <= 16, the weight-stream form
int small_m_form(long N, long K, int flags);
bool conv_small_n_serves(const mx_gemm_desc* d);            // conv_small_n.hip: 3x3 conv with N <= 16 output channels (conv_out)
bool conv_small_cin_serves(const mx_gemm_desc* d);          // conv_small_n.hip: 3x3 conv over <= 8 non-zero input channels (conv_in)

constexpr int BK = 64;
constexpr size_t kSplitKWsBytes = 96u << 20;     // split-K scratch per stream (below): fp32 partial tiles / arrival tickets
constexpr size_t kSplitKCntBytes = 64u << 10;

// The kernel family of a launch.  The values are mx_gemm_form's answers (mxdenoise.h).
enum GemmFamily { FAM_GENERIC = MX_FORM_TILE_GENERIC, FAM_ROWS_256 = MX_FORM_TILE_256, FAM_ROWS_128 = MX_FORM_TILE_128,
                  FAM_PERSISTENT_256 = MX_FORM_PERSISTENT_256, FAM_SMALL_M = MX_FORM_SMALL_M, FAM_CONV_SMALL_N = MX_FORM_CONV_SMALL_N,
                  FAM_CONV_SMALL_CIN = MX_FORM_CONV_SMALL_CIN };
// family of an instantiation: the list in gemm_forms.h that holds it
static GemmFamily family_of_form(int form) {
  switch (form) {
#define MX_CASE(id, ...) case id:
    MX_GEMM_GENERIC_FORMS(MX_CASE) return FAM_GENERIC;
    MX_GEMM_V2_FORMS(MX_CASE) return FAM_ROWS_128;
    MX_GEMM_V5_FORMS(MX_CASE) return FAM_ROWS_256;
    MX_GEMM_V4_FORMS(MX_CASE) return FAM_PERSISTENT_256;
    MX_GEMM_SMALL_M_FORMS(MX_CASE) return FAM_SMALL_M;
#undef MX_CASE
    case GK_CONV_SMALL_N: return FAM_CONV_SMALL_N;
    default: return FAM_CONV_SMALL_CIN;
  }
}
static const char* const kGemmKernelNames[GK_COUNT] = {
  MX_GEMM_GENERIC_FORMS(MX_FORM_NAME_T) MX_GEMM_V2_FORMS(MX_FORM_NAME_T) MX_GEMM_V5_FORMS(MX_FORM_NAME_T) MX_GEMM_V4_FORMS(MX_FORM_NAME_T)
  MX_GEMM_SMALL_M_FORMS(MX_FORM_NAME_T) MX_GEMM_CONV_SMALL_FORMS(MX_FORM_NAME_P)
};

// Everything decided for one launch.
struct GemmRoute {
  GemmFamily family = FAM_GENERIC;
  int bn = 0, rows = 0;      // tile of the pipelined kernels (features x token rows); 0 / 0: none of them serves the launch
  int splitk = 1;            // K slices (128-row tiles only)
  int form = -1;             // gemm_forms.h id of the instantiation, -1: none serves the descriptor
  int stats_slabs = 0;       // slabs of row statistics the launch writes through stats_out; 0: it cannot
  bool gn_part = false;      // can write gn_part_out
  bool ln_final_out = false; // can write ln_final_out (given stats_out and ln_final_cnt)
};
// What mx_gemm / mx_conv3x3 (d) runs: one launch of d itself, or the two halves of the tail split (below).
struct GemmPlan {
  int n = 1;
  const mx_gemm_desc* d[2] = {nullptr, nullptr};
  GemmRoute r[2];
  mx_gemm_desc half[2];      // the tail split's descriptors (d[i] points here then)
};

// One problem of a launch: segs[i] of a grouped launch, or the descriptor's own problem in the same shape (what the per-problem rules read: A,
// the rows, the remaps, ldvt and the conv grid)
static mx_gemm_seg problem_of(const mx_gemm_desc* d) {
  mx_gemm_seg g = {};
  g.a = d->a; g.M = d->M; g.rows_per_batch = d->rows_per_batch; g.ldvt = d->ldvt;
  g.B = d->B; g.Hin = d->Hin; g.Win = d->Win; g.Hout = d->Hout; g.Wout = d->Wout;
  g.a_batch_rows = d->a_batch_rows; g.a_row_off = d->a_row_off; g.c_batch_rows = d->c_batch_rows; g.c_row_off = d->c_row_off;
  return g;
}
static int problems_of(const mx_gemm_desc* d) { return d->n_segs > 0 ? d->n_segs : 1; }
static mx_gemm_seg problem_of(const mx_gemm_desc* d, int i) { return d->n_segs > 0 ? d->segs[i] : problem_of(d); }
// rows of A a problem reaches (the joint-sequence remap reads rows of a longer sequence)
static long in_rows_of(const mx_gemm_seg& g) {
  return g.a_batch_rows > 0 ? (long)(g.M / std::max(g.rows_per_batch, 1) + 1) * g.a_batch_rows : g.M;
}
// m-tiles of the launch for tiles of `rows` rows: the problems of a grouped launch are tiled one by one (no tile straddles two of them)
static long m_tiles_of(const mx_gemm_desc* d, int rows) {
  long t = 0;
  for (int i = 0; i < problems_of(d); ++i) t += cdiv(d->n_segs > 0 ? d->segs[i].M : d->M, rows);
  return t;
}
static long rows_of(const mx_gemm_desc* d) { return m_tiles_of(d, 1); }

// ---- the tile of the pipelined kernels ----
// Candidates (token rows x features): 256x256 (gemm_bf16_v4.hip), 256x160, 256x128 (gemm_bf16_v5.hip), 128x160, 128x128 (gemm_bf16_v2.hip).
// Estimated cost = full-chip rounds of 256 workgroups (one per CU) x (rows + features): the K loop of a tile is held by the CU's L2 -> LDS
// fetch stream, whose bytes per K tile are (rows + features) * 128.  A small problem therefore prefers small tiles (more CUs fetch in
// parallel: one 1024 px request gives M = 2048), a chip-filling one the tiling with the fewest rounds and the largest tile (fewest bytes per
// FLOP; the 256x256 kernel is further discounted by its measured advantage).  rows == 0: none of them, the generic 128-row kernel.
static const int kTiles[5][2] = {{256, 256}, {160, 256}, {128, 256}, {160, 128}, {128, 128}};      // {features, rows}; the 128-row tiles from [3]

// may a launch of d use tiles of `rows` x `bn`?  (whatever excludes every tile is in pick_tile)
static bool tile_serves(const mx_gemm_desc* d, bool conv, int bn, int rows, long Mtot, bool fits32) {
  if (d->N % bn != 0 || Mtot < rows) return false;
  if (bn == 256 && (conv || !fits32 || d->a2 || d->ln_stats || d->stats_out)) return false;   // (built without those hooks)
  if (d->ln_final && bn != 256) return false;   // finalised statistics are the 256 x 256 kernel's form of the fold (the others read the slabs)
  // the gated epilogue pairs whole 32-feature halves; a 64-wide RMSNorm head must lie inside one wave panel (gemm_epilogue_regs)
  if ((d->flags & (MX_EPI_GEGLU | MX_EPI_RMSNORM)) && bn == 160) return false;
  if ((d->flags & MX_EPI_QKV) && (d->seg % 64 != 0 || (bn != 256 && d->seg % (bn / 2) != 0))) return false;
  return true;
}
// the 256x256 kernel addresses its operands with 32-bit byte offsets from the base pointers (grouped: from the lowest problem base)
static uintptr_t lowest_a(const mx_gemm_desc* d) {
  uintptr_t lo = (uintptr_t)problem_of(d, 0).a;
  for (int i = 1; i < d->n_segs; ++i) lo = std::min(lo, (uintptr_t)d->segs[i].a);
  return lo;
}
static bool fits_32bit_offsets(const mx_gemm_desc* d) {
  bool fits = (long)d->N * d->K * 2 < (1L << 32);
  const uintptr_t lo = lowest_a(d);
  for (int i = 0; i < problems_of(d); ++i) {
    const mx_gemm_seg g = problem_of(d, i);
    fits = fits && (long)((uintptr_t)g.a - lo) + in_rows_of(g) * d->lda * 2 < (1L << 32);
  }
  return fits;
}

// fills bn, rows and splitk of r
static void pick_tile(const mx_gemm_desc* d, bool conv, GemmRoute& r) {
  constexpr double v4_discount = 0.87;          // measured advantage of the 256 x 256 ping-pong kernel per byte fetched (round 1 A/B sweeps)
  const long Mtot = rows_of(d);
  if (Mtot < 128 || d->K < 128) return;
  if (d->flags & (MX_EPI_OUT_F32 | MX_EPI_RES_BCAST)) return;   // the register-exchange epilogue writes bf16 only and adds a per-row residual
  // its row walk steps 16 tokens at a time with one wrap per step (gemm_epilogue_regs): batches shorter than that go to the generic kernel
  for (int i = 0; i < problems_of(d); ++i) { const int rpb = problem_of(d, i).rows_per_batch; if (rpb > 0 && rpb < 16) return; }
  // their LDS-staged epilogue moves 16-byte pieces of C and of the residual
  if (d->ldc % 8 != 0 || ((uintptr_t)d->c & 15) != 0) return;
  if (d->residual && (d->ldr % 8 != 0 || ((uintptr_t)d->residual & 15) != 0)) return;
  const bool fits32 = fits_32bit_offsets(d);
  const int ncu = cu_count();
  double best_cost = 0;
  for (const auto& t : kTiles) {
    const int bn = t[0], rows = t[1];
    if (!tile_serves(d, conv, bn, rows, Mtot, fits32)) continue;
    const long tiles = m_tiles_of(d, rows) * (d->N / bn);
    const double cost = (double)((tiles + ncu - 1) / ncu) * (rows + bn) * (bn == 256 ? v4_discount : 1.0);
    if (r.rows == 0 || cost < best_cost) { r.bn = bn; r.rows = rows; best_cost = cost; }
  }
  // Small launches (the 128-row tiles: one request, light mixed batches) leave CUs idle and run a long serial K loop whose iteration cannot be
  // shorter than the CU's LDS-DMA issue allows (0.55-0.8 us per 128 x 128 x 64 tile whatever the ring depth).  SPLIT-K deals the K tiles of an
  // output tile to `splitk` workgroups (gemm_bf16_v2.hip, splitk_combine).  What it costs was measured (round 4, tools/exp/splitk_bench.py,
  // profiles/r04_g_splitk_bench.txt): the fp32 partial tiles travel through memory -- slices x M x N x 4 bytes written through and read back
  // -- so M 2048, N 1280 in two slices moves 42 MB and the combine takes ~10 us: K 1280 got SLOWER (16.4 -> 21.2 us), K 5120 5 % faster
  // (43.3 -> 41.0), M 512 5 % faster.  The estimate below therefore charges that traffic at 4 TB/s and a split is taken only where it still
  // wins by 25 %: long K at small M x N (the convs and ff.net.2 of a single 512 px request: M 512).  Slicing K also changes the order in
  // which a row's products are added, so a split launch is not bit-equal to the unsplit one (every unsplit tiling is): the margin keeps the
  // marginal cases on the order that does not depend on what else shares the batch.
  // A forced slice count (d->splitk 2..4: tests, A/B) takes the eligible tiling with the shortest K loop at that many slices, whatever the
  // combine costs and however many workgroups it makes.
  if (d->splitk == 1 || r.rows != 128 || d->a2 || d->K / 64 < 16) return;
  const int nk = d->K / 64;
  double best_t = 0, unsplit_t = 0, forced_t = 0;
  int pick_bn = r.bn, pick_sk = 1, forced_bn = 0;
  for (int c = 3; c < 5; ++c) {
    const int bn = kTiles[c][0];
    if (!tile_serves(d, conv, bn, 128, Mtot, fits32)) continue;
    const long tiles = m_tiles_of(d, 128) * (d->N / bn);
    for (int sk = 1; sk <= 4; ++sk) {
      if ((d->splitk > 1 && sk != 1 && sk != d->splitk) || nk / sk < 8) continue;
      if (sk > 1 && (tiles * sk * 128L * bn * 4 > (long)kSplitKWsBytes || tiles * 4 > (long)kSplitKCntBytes)) continue;   // the partial tiles and tickets must fit the library's scratch
      const double loop = (double)((tiles * sk + ncu - 1) / ncu) * ((double)(nk / sk) * 0.57 * (128 + bn) / 256.0 + 5.0);   // us: rounds of the chip x (K loop + set-up)
      if (sk == d->splitk && (forced_t == 0 || loop < forced_t)) { forced_t = loop; forced_bn = bn; }
      if (sk > 1 && tiles * sk > 2L * ncu) continue;
      const double combine = sk > 1 ? 2.0 + (double)sk * (double)Mtot * d->N * 8.0 / 4.0e6 : 0.0;      // us: partial tiles out and back at ~4 TB/s
      const double t = loop + combine;
      if (sk == 1 && bn == r.bn) unsplit_t = t;
      if (best_t == 0 || t < best_t - 1e-9) { best_t = t; pick_bn = bn; pick_sk = sk; }
    }
  }
  if (pick_sk > 1 && unsplit_t > 0 && best_t <= 0.75 * unsplit_t) { r.bn = pick_bn; r.splitk = pick_sk; }
  if (forced_bn) { r.bn = forced_bn; r.splitk = d->splitk; }
}

// slabs of row statistics a launch of d on the tile of t writes: one per wave column panel of the register-exchange epilogue (gemm_epilogue_regs);
// 0 when the generic kernel serves d or the epilogue is not a plain bf16 store
static int stats_slabs_of(const mx_gemm_desc* d, bool conv, const GemmRoute& t) {
  if (conv || t.bn == 0 || t.bn == 256) return 0;     // (the 256 x 256 kernels are built without it: asking for stats_out moves the launch
                                                      //  to a 256 / 128-row tile, see tile_serves)
  if (d->flags & (MX_EPI_GEGLU | MX_EPI_QKV | MX_EPI_OUT_F32)) return 0;
  if (d->a_batch_rows > 0 || d->c_batch_rows > 0) return 0;
  for (int i = 0; i < d->n_segs; ++i) if (d->segs[i].a_batch_rows > 0 || d->segs[i].c_batch_rows > 0) return 0;
  return d->N / (t.bn / 2);                           // 4 x 2 waves of (16 MI) x (BN / 2)
}

// The kernel instantiation (gemm_forms.h id) a launch of d on the tile of t runs, or -1 if none serves it: the smallest instantiation that
// carries the launch's epilogue features (each carries only its own epilogue code: gemm_args.h, EPI_F_*).
static int form_of(const mx_gemm_desc* d, bool conv, const GemmRoute& t) {
  if (d->ln_final && t.bn != 256) return -1;    // (the launch rejects it)
  if (small_m_serves(d, conv)) return small_m_form(d->N, d->K, d->flags);
  if (conv && conv_small_n_serves(d)) return GK_CONV_SMALL_N;
  if (conv && conv_small_cin_serves(d)) return GK_CONV_SMALL_CIN;
  const int feat = gemm_epi_features(d->flags);
  const bool geglu = (d->flags & MX_EPI_GEGLU) != 0;
  const bool vec = d->rowbias || d->gate;       // per-sample vectors: compiled in only where asked for
  const bool b160 = t.bn == 160;
  if (t.bn == 256) {                            // persistent 256 x 256 (gemm_bf16_v4.hip)
    if (d->ln_final) {                          // the folded LayerNorm's instantiations: GEGLU / QKV / plain, no per-sample vectors (validate checked)
      if (geglu) return (feat & EPI_F_ACT) ? -1 : GK_V4_GEGLU_LN;
      return feat == EPI_F_QKV ? GK_V4_QKV_LN : feat == 0 ? GK_V4_LN : -1;
    }
    if (geglu) return (feat & EPI_F_ACT) ? GK_V4_GEGLU_ACT : GK_V4_GEGLU;      // (the gated epilogue takes no per-sample vectors)
    if (!vec) return feat == 0 ? GK_V4 : feat == EPI_F_QKV ? GK_V4_QKV : feat == EPI_F_TANH ? GK_V4_TANH : GK_V4_VEC_ALL;
    return feat == 0 ? GK_V4_VEC : GK_V4_VEC_ALL;
  }
  if (t.rows == 256) {                          // 256-row ping-pong tiles (gemm_bf16_v5.hip)
    if (geglu) return (feat & EPI_F_ACT) ? GK_V5_128_GEGLU_ACT : GK_V5_128_GEGLU;      // (tile_serves: 128 features only; no per-sample vectors)
    if (conv) {
      if (feat == 0 && !vec) return b160 ? GK_V5_160_CONV : GK_V5_128_CONV;
      if (feat == 0) return b160 ? GK_V5_160_CONV_VEC : GK_V5_128_CONV_VEC;
      return b160 ? GK_V5_160_CONV_ALL : GK_V5_128_CONV_ALL;
    }
    if (feat == 0 && !vec) return b160 ? GK_V5_160 : GK_V5_128;
    if (feat == EPI_F_QKV && !vec) return b160 ? GK_V5_160_QKV : GK_V5_128_QKV;
    return b160 ? GK_V5_160_ALL : GK_V5_128_ALL;
  }
  if (t.rows == 128) {                          // 128-row lock-step tiles (gemm_bf16_v2.hip)
    if (geglu) return (feat & EPI_F_ACT) ? GK_V2_128_GEGLU_ACT : GK_V2_128_GEGLU;      // (tile_serves: 128 features only)
    if (conv) return feat == 0 ? (b160 ? GK_V2_160_CONV : GK_V2_128_CONV) : (b160 ? GK_V2_160_CONV_ALL : GK_V2_128_CONV_ALL);
    if (feat == 0) return b160 ? GK_V2_160 : GK_V2_128;
    if (feat == EPI_F_QKV) return b160 ? GK_V2_160_QKV : GK_V2_128_QKV;
    return b160 ? GK_V2_160_ALL : GK_V2_128_ALL;
  }
  if (d->N % 128 == 0) return conv ? GK_GEN128_CONV : GK_GEN128;      // the generic register-prefetch tile kernel
  return conv ? GK_GEN64_CONV : GK_GEN64;
}

// Why a launch of d on route r cannot write gn_part_out (nullptr: it can).  validate's check and mx_gemm_gn_partials_supported.
static const char* gn_part_refusal(const mx_gemm_desc* d, const GemmRoute& r) {
  if (d->n_segs > 0 || r.rows != 256 || r.bn == 256 || r.bn == 0 || r.splitk > 1)
    return "gemm: gn_part_out needs an ungrouped launch on a 256-row tile (mx_gemm_gn_partials_supported)";
  if (d->flags != 0 || d->residual || d->gate || d->out_scale != 0.f || d->ln_stats || d->ln_final || d->a_batch_rows > 0 || d->c_batch_rows > 0)
    return "gemm: gn_part_out needs an epilogue of bias (+ row bias) only";
  if (d->M % 64 != 0 || (d->rowbias && (d->rows_per_batch <= 0 || d->rows_per_batch % 64 != 0)))
    return "gemm: gn_part_out needs M % 64 == 0, rows_per_batch % 64 == 0 and 16-byte alignment";
  return nullptr;
}

// A descriptor that no instantiation serves (ln_final away from the 256 x 256 kernel, or with an epilogue it is not built for) is rejected by the
// launch; mx_gemm_form still reports a family for it: the small conv forms if they would take it, else the family of its tile.
static GemmFamily family_of_unserved(const mx_gemm_desc* d, bool conv, const GemmRoute& t) {
  if (conv && conv_small_n_serves(d)) return FAM_CONV_SMALL_N;
  if (conv && conv_small_cin_serves(d)) return FAM_CONV_SMALL_CIN;
  return t.bn == 256 ? FAM_PERSISTENT_256 : t.bn == 0 ? FAM_GENERIC : t.rows == 256 ? FAM_ROWS_256 : FAM_ROWS_128;
}

// THE route of one launch of d.  Only plan_of calls it.
static GemmRoute route_of(const mx_gemm_desc* d, bool conv) {
  GemmRoute r;
  pick_tile(d, conv, r);
  r.form = form_of(d, conv, r);
  r.family = r.form >= 0 ? family_of_form(r.form) : family_of_unserved(d, conv, r);
  r.stats_slabs = stats_slabs_of(d, conv, r);
  r.gn_part = gn_part_refusal(d, r) == nullptr;
  r.ln_final_out = d->n_segs <= 0 && r.rows == 256 && r.bn != 256 && r.stats_slabs > 0;      // an ungrouped 256-row tile of the register-exchange kernels
  return r;
}

// TAIL SPLIT (round 4).  The persistent 256 x 256 kernel walks whole rounds of one tile per CU; a launch whose tile count leaves a short last round
// (one 1024 px request: GEGLU M 2048 x N 10240 = 320 tiles = 1.25 rounds, 77 us for 1.25 rounds of work) pays a full round for it.  Where the tiles
// of the whole rounds are whole column panels, the launch is cut along N: columns [0, N1) keep the 256 x 256 kernel in whole rounds, the rest
// becomes a second launch on whatever tile the chooser gives it, accepted only if that is ONE round of a cheaper tile (128 x 128 / 128 x 160 /
// 256 x 128).  Columns are independent, so the results are those of the single launch bit for bit where both tilings add a row's products in
// the same order (every unsplit tiling does).  Plain and gated epilogues only (no QKV segments, statistics, fp32 output, grouped launches).
// whole: the route of d itself.  On success p holds the two halves and their routes.
static bool tail_split(const mx_gemm_desc* d, const GemmRoute& whole, GemmPlan& p) {
  if (whole.bn != 256 || d->n_segs != 0 || d->M <= 0 || d->N <= 0 || d->K <= 0 || d->N % 256 != 0) return false;
  if (d->flags & (MX_EPI_QKV | MX_EPI_OUT_F32 | MX_EPI_RES_BCAST | MX_EPI_RMSNORM)) return false;
  if (d->stats_out || d->ln_stats || d->ln_final || d->ln_final_out || d->a_batch_rows > 0 || d->c_batch_rows > 0 || d->splitk > 1) return false;
  const int ncu = cu_count();
  if (ncu <= 0) return false;
  const long mt = cdiv(d->M, 256), nt = d->N / 256, tiles = mt * nt;
  const long full = tiles / ncu, rem = tiles % ncu;
  if (full < 1 || rem == 0 || rem * 2 > ncu || (full * ncu) % mt != 0) return false;
  const long nt1 = full * ncu / mt;
  if (nt1 <= 0 || nt1 >= nt) return false;
  const int N1 = (int)nt1 * 256, N2 = d->N - N1;
  const bool geglu = (d->flags & MX_EPI_GEGLU) != 0;
  const long cofs = geglu ? N1 / 2 : N1;       // first output column of the second launch
  if (geglu && d->residual) return false;      // (validate rejects that pair anyway; its column offsets would differ)
  mx_gemm_desc &d1 = p.half[0], &d2 = p.half[1];
  d1 = *d; d2 = *d;
  d1.N = N1; d2.N = N2;
  d1.splitk = 1; d2.splitk = 1;               // both halves add a row's products in the single launch's order (advisor, round 4)
  d2.w = (const char*)d->w + (size_t)N1 * d->K * 2;
  if (d->bias) d2.bias = d->bias + N1;
  d2.c = (char*)d->c + (size_t)cofs * 2;
  if (d->residual) d2.residual = (const char*)d->residual + (size_t)N1 * 2;
  if (d->rowbias) d2.rowbias = d->rowbias + N1;
  if (d->gate) d2.gate = d->gate + N1;
  p.r[1] = route_of(&d2, false);
  if (p.r[1].bn == 0 || p.r[1].bn == 256 || p.r[1].rows + p.r[1].bn > 384) return false;
  if (m_tiles_of(&d2, p.r[1].rows) * (N2 / p.r[1].bn) > ncu) return false;
  p.r[0] = route_of(&d1, false);
  return p.r[0].bn == 256;
}

// What mx_gemm (conv = false) / mx_conv3x3 (conv = true) runs for d (n_segs / segs sound).  false: no descriptor or no work -- p is one launch of d
// on no route, which validate rejects and for which each query answers its "no".
static bool plan_of(const mx_gemm_desc* d, bool conv, GemmPlan& p) {
  p.d[0] = d;
  if (!d || rows_of(d) <= 0 || d->N <= 0 || d->K <= 0) return false;
  const GemmRoute whole = route_of(d, conv);
  if (!conv && tail_split(d, whole, p)) { p.n = 2; p.d[0] = &p.half[0]; p.d[1] = &p.half[1]; }
  else p.r[0] = whole;
  return true;
}

// ---- validation: everything that does not depend on the route ----
// the rules of one problem (the descriptor's own, or one of a grouped launch)
static int validate_problem(const mx_gemm_desc* d, bool conv, const mx_gemm_seg& g, bool grouped) {
  if (d->rowbias || d->gate || g.a_batch_rows > 0 || g.c_batch_rows > 0 || (d->flags & (MX_EPI_QKV | MX_EPI_RES_BCAST)))
    MX_CHECK(g.rows_per_batch > 0, "gemm: rows_per_batch required");
  if (g.a_batch_rows > 0) MX_CHECK(!conv && g.a_row_off >= 0 && g.a_row_off + g.rows_per_batch <= g.a_batch_rows, "gemm: bad input row remap");
  if (g.c_batch_rows > 0) MX_CHECK(g.c_row_off >= 0 && g.c_row_off + g.rows_per_batch <= g.c_batch_rows, "gemm: bad output row remap");
  // (a grouped problem's reach is counted without its row remap, as it always was)
  MX_CHECK((grouped || conv ? (long)g.M : in_rows_of(g)) * (conv ? 1 : d->lda) < 2147483647L, "gemm: operand exceeds 32-bit indexing");
  if (conv) {
    const int Hv = g.Hin << d->up, Wv = g.Win << d->up;
    MX_CHECK(g.Hout == (Hv + d->stride - 1) / d->stride && g.Wout == (Wv + d->stride - 1) / d->stride, "conv3x3: output grid does not match input grid / stride");
    MX_CHECK((long)g.B * g.Hout * g.Wout == g.M, "conv3x3: M != B*Hout*Wout");
  }
  if (d->flags & MX_EPI_QKV) {
    MX_CHECK(g.ldvt >= MX_VT_LD(g.c_batch_rows > 0 ? g.c_batch_rows : g.rows_per_batch) && (!grouped || g.ldvt % 8 == 0), "gemm: QKV needs ldvt >= MX_VT_LD(keys per batch)");
    MX_CHECK(g.M % g.rows_per_batch == 0, "gemm: QKV needs M % rows_per_batch == 0");
  }
  return 0;
}

static int validate(const mx_gemm_desc* d, bool conv) {
  MX_CHECK(d->a && d->w && (d->c || (d->flags & MX_EPI_QKV)), "gemm: null operand");
  MX_CHECK((d->n_segs > 0 || d->M > 0) && d->N > 0 && d->K > 0, "gemm: empty problem");
  const bool grouped = d->n_segs > 0;
  for (int i = 0; i < d->n_segs; ++i) {          // a problem of a grouped launch has exactly the operands the descriptor names
    const mx_gemm_seg& g = d->segs[i];
    MX_CHECK(g.M > 0 && g.a && (g.c != nullptr) == (d->c != nullptr), "gemm: grouped launch: empty problem or missing a / c");
    MX_CHECK((g.a2 != nullptr) == (d->a2 != nullptr && !conv) && (g.residual != nullptr) == (d->residual != nullptr) && (g.vt != nullptr) == (d->vt != nullptr) &&
             (g.rowbias != nullptr) == (d->rowbias != nullptr) && (g.gate != nullptr) == (d->gate != nullptr) &&
             (g.ln_stats != nullptr) == (d->ln_stats != nullptr) && (g.stats_out != nullptr) == (d->stats_out != nullptr),
             "gemm: grouped launch: a problem's optional operands must match the descriptor's");
    const void* ptrs[] = {g.a, g.a2, g.c, g.residual, g.vt, g.rowbias, g.gate, g.ln_stats, g.stats_out};
    for (const void* q : ptrs) MX_CHECK(((uintptr_t)q & 15) == 0, "gemm: grouped launch: operand pointers must be 16-byte aligned");
    if (d->ln_stats || d->stats_out)           // (advisor, round 3: the per-problem remaps were not covered by the descriptor-level check)
      MX_CHECK(g.a_batch_rows <= 0 && g.c_batch_rows <= 0, "gemm: grouped launch: the folded LayerNorm / stats_out exclude a problem's row remaps");
  }
  MX_CHECK(d->K % BK == 0, "gemm: K must be a multiple of 64");
  MX_CHECK(d->N % 4 == 0, "gemm: N must be a multiple of 4");
  if (d->ln_final) {
    MX_CHECK(!conv && !d->ln_stats && d->ln_colsum && d->n_segs == 0, "gemm: ln_final needs ln_colsum, excludes ln_stats and grouped launches (mx_gemm only)");
    MX_CHECK(!(d->flags & MX_EPI_RMSNORM) && d->a_batch_rows <= 0 && d->c_batch_rows <= 0 && !d->a2 && !d->rowbias && !d->gate && !d->stats_out,
             "gemm: ln_final excludes RMSNORM, the row remaps, the split A operand, per-sample vectors and stats_out");
    MX_CHECK((((uintptr_t)d->ln_final & 15) | ((uintptr_t)d->ln_colsum & 15)) == 0, "gemm: ln_final / ln_colsum must be 16-byte aligned");
  }
  if (d->ln_stats) {
    MX_CHECK(!conv && d->ln_colsum && d->ln_slabs > 0, "gemm: folded LayerNorm needs ln_colsum and ln_slabs > 0 (mx_gemm only)");
    MX_CHECK(!(d->flags & MX_EPI_RMSNORM) && d->a_batch_rows <= 0 && d->c_batch_rows <= 0 && !d->a2, "gemm: folded LayerNorm excludes RMSNORM, the row remaps and the split A operand");
    MX_CHECK((((uintptr_t)d->ln_stats & 15) | ((uintptr_t)d->ln_colsum & 15)) == 0, "gemm: ln_stats / ln_colsum must be 16-byte aligned");
  }
  if (!conv && d->a2) {
    MX_CHECK(d->k_split > 0 && d->k_split < d->K && d->k_split % BK == 0, "gemm: k_split must be a multiple of 64 inside (0, K)");
    MX_CHECK(d->lda >= d->k_split && d->lda % 8 == 0 && d->lda2 >= d->K - d->k_split && d->lda2 % 8 == 0, "gemm: bad lda / lda2 for the split A operand");
    MX_CHECK(d->a_batch_rows <= 0 && ((uintptr_t)d->a2 & 15) == 0 && rows_of(d) * d->lda2 < 2147483647L, "gemm: split A operand excludes the row remap and needs 16-byte alignment");
  } else if (!conv) {
    MX_CHECK(d->lda >= d->K && d->lda % 8 == 0, "gemm: lda must be >= K and a multiple of 8");
  } else {
    MX_CHECK(d->Cin % BK == 0 && d->K == 9 * d->Cin, "conv3x3: Cin must be a multiple of 64 and K = 9*Cin");
    MX_CHECK(d->stride == 1 || d->stride == 2, "conv3x3: stride must be 1 or 2");
    MX_CHECK(d->up == 0 || d->up == 1, "conv3x3: up must be 0 or 1");
    MX_CHECK(!(d->up && d->stride != 1), "conv3x3: upsample only with stride 1");
    MX_CHECK(2 * d->Cin <= 16384, "conv3x3: Cin > 8192 (the pipelined loader walks a 16 KB zero page for padding taps)");
    MX_CHECK(!(d->flags & MX_EPI_GEGLU), "conv3x3: no GEGLU epilogue");
    MX_CHECK(d->vhalo == 0 || (d->vhalo == 1 && d->corner_patch == 0), "conv3x3: vhalo must be 0 or 1 and excludes the sliced corner rule");
  }
  // the LDS-DMA loaders and the staged epilogue move 16-byte pieces: every base pointer must be 16-byte aligned
  const void* ptrs[] = {d->a, d->w, d->c, d->bias, d->rowbias, d->residual, d->gate, d->rms_wq, d->rms_wk};
  for (const void* q : ptrs) MX_CHECK(((uintptr_t)q & 15) == 0, "gemm: operand pointers must be 16-byte aligned");
  if (d->gate) MX_CHECK(d->ldg >= d->N && d->ldg % 4 == 0, "gemm: bad ldg");
  if (d->rowbias) MX_CHECK(d->ldrb >= d->N && d->ldrb % 4 == 0, "gemm: bad ldrb");
  if (d->residual) MX_CHECK(d->ldr >= d->N && d->ldr % 4 == 0, "gemm: bad ldr");
  MX_CHECK((long)d->N * d->K < 2147483647L, "gemm: operand exceeds 32-bit indexing");
  if (d->flags & MX_EPI_GEGLU) {
    MX_CHECK(d->N % 128 == 0, "gemm: GEGLU needs N % 128 == 0");
    MX_CHECK(!(d->flags & (MX_EPI_QKV | MX_EPI_OUT_F32)) && !d->residual && !d->rowbias && d->out_scale == 0.f, "gemm: GEGLU excludes other epilogues");
    MX_CHECK(d->ldc >= d->N / 2 && d->ldc % 4 == 0, "gemm: bad ldc for GEGLU");
  } else if (d->flags & MX_EPI_QKV) {
    MX_CHECK(d->seg > 0 && d->seg % 64 == 0 && d->period >= 2 && d->N % (d->seg * d->period) == 0, "gemm: bad QKV segments");
    MX_CHECK(d->vt != nullptr, "gemm: QKV needs vt");
    MX_CHECK(d->ldc >= d->N / d->period * (d->period - 1) && d->ldc % 4 == 0, "gemm: bad ldc for QKV");
    MX_CHECK(!(d->flags & MX_EPI_OUT_F32), "gemm: QKV output is bf16");
    MX_CHECK(!d->rowbias && !d->gate && !d->residual, "gemm: QKV excludes the per-sample vectors and the residual (its V^T segment takes none of them)");
    if (d->flags & MX_EPI_RMSNORM)
      MX_CHECK(d->rms_wq && d->rms_wk && d->period == 3 && d->N % 128 == 0 && !conv, "gemm: RMSNORM needs rms_wq/rms_wk, period 3, N % 128 == 0");
  } else {
    MX_CHECK(d->ldc >= d->N && d->ldc % 4 == 0, "gemm: bad ldc");
  }
  for (int i = 0; i < problems_of(d); ++i)
    if (int rc = validate_problem(d, conv, problem_of(d, i), grouped)) return rc;
  return 0;
}

// ---- the kernel argument block of a validated d on route r (the split-K scratch and the route's optional outputs: launch()) ----
static void fill_args(const mx_gemm_desc* d, bool conv, const GemmRoute& r, GemmArgs& a) {
  a.stagger_ticks = 0;
  a.vhalo = conv ? d->vhalo : 0;
  a.a2 = conv ? nullptr : (const bf16_t*)d->a2; a.lda2 = d->lda2; a.k_split = d->k_split;
  a.a = (const bf16_t*)d->a; a.w = (const bf16_t*)d->w; a.c = d->c;
  a.bias = d->bias; a.rowbias = d->rowbias; a.residual = (const bf16_t*)d->residual; a.vt = (bf16_t*)d->vt;
  a.M = d->M; a.N = d->N; a.K = d->K; a.lda = d->lda; a.ldc = d->ldc; a.ldr = d->ldr; a.ldrb = d->ldrb;
  a.rows_per_batch = d->rows_per_batch; a.flags = d->flags; a.seg = d->seg; a.period = d->period; a.ldvt = d->ldvt;
  a.B = d->B; a.Hin = d->Hin; a.Win = d->Win; a.Cin = d->Cin; a.Hout = d->Hout; a.Wout = d->Wout;
  a.stride = d->stride; a.up = d->up; a.corner_patch = d->corner_patch;
  a.a_batch_rows = d->a_batch_rows; a.a_row_off = d->a_row_off; a.c_batch_rows = d->c_batch_rows; a.c_row_off = d->c_row_off;
  a.gate = d->gate; a.ldg = d->ldg; a.out_scale = d->out_scale;
  a.rms_wq = d->rms_wq; a.rms_wk = d->rms_wk; a.rms_eps = d->rms_eps;
  a.ln_stats = d->ln_stats; a.ln_colsum = d->ln_colsum; a.ln_slabs = d->ln_slabs; a.ln_eps = d->ln_eps;
  a.ln_final = d->ln_final;
  a.stats_out = d->stats_out; a.gn_part = d->gn_part_out;
  a.ln_final_out = d->ln_final_out; a.ln_final_cnt = d->ln_final_out ? d->ln_final_cnt : nullptr; a.ln_final_slabs = d->ln_final_out ? r.stats_slabs : 0;
  a.xcd_map = 1;
  a.splitk = 0; a.sk_ws = nullptr; a.sk_cnt = nullptr;
  a.nseg = d->n_segs; a.mt_total = 0;
  if (d->n_segs > 0) {
    // the problems' tiles follow each other in the launch's tile list; the kernel argument's own a is the lowest problem base (the 256 x 256
    // kernel addresses A by 32-bit offsets from it: fits_32bit_offsets checked the reach)
    const int rows = r.rows > 0 ? r.rows : 128;
    int t0 = 0;
    for (int i = 0; i < d->n_segs; ++i) {
      const mx_gemm_seg& g = d->segs[i];
      GemmSeg& o = a.prob[i];
      o.a = (const bf16_t*)g.a; o.a2 = conv ? nullptr : (const bf16_t*)g.a2; o.c = g.c; o.residual = (const bf16_t*)g.residual; o.vt = (bf16_t*)g.vt;
      o.rowbias = g.rowbias; o.gate = g.gate; o.ln_stats = g.ln_stats; o.stats_out = d->stats_out ? g.stats_out : nullptr;
      o.M = g.M; o.tile0 = t0; o.rows_per_batch = g.rows_per_batch; o.ldvt = g.ldvt;
      o.B = g.B; o.Hin = g.Hin; o.Win = g.Win; o.Hout = g.Hout; o.Wout = g.Wout;
      o.a_batch_rows = g.a_batch_rows; o.a_row_off = g.a_row_off; o.c_batch_rows = g.c_batch_rows; o.c_row_off = g.c_row_off;
      t0 += cdiv(g.M, rows);
    }
    a.mt_total = t0;
    a.a = (const bf16_t*)lowest_a(d);
    a.M = (int)rows_of(d);
  }
}

// scratch of the split-K launches: fp32 partial tiles and one arrival counter per output tile, per stream (launches of one stream are ordered;
// concurrent streams -- the per-resolution sequences of a mixed batch -- must not share them).  Allocated at the first split launch of a stream,
// ALSO while that stream is being captured (advisor, round 4: a capture used to bake in the unsplit kernels, so eager and replayed forwards of one
// shape added their products in different orders): the allocation runs with the thread's capture mode relaxed and zeroes the counters on a private
// stream, neither of which touches the capturing stream.  Whether a launch is split therefore depends on its descriptor alone (pick_tile); a scratch
// that cannot be had is an error, not a silent change of summation order.  mx_gemm_release_scratch frees a stream's scratch (library unload frees all).
struct SplitKScratch { float* ws = nullptr; unsigned* cnt = nullptr; };
struct SplitKPool {
  std::mutex mu;
  std::unordered_map<hipStream_t, SplitKScratch> per_stream;
  static void drop(SplitKScratch& b) { if (b.ws) (void)hipFree(b.ws); if (b.cnt) (void)hipFree(b.cnt); b = SplitKScratch{}; }
  ~SplitKPool() { for (auto& kv : per_stream) drop(kv.second); }
};
static SplitKPool& splitk_pool() { static SplitKPool p; return p; }
static bool splitk_scratch(hipStream_t s, SplitKScratch& out) {
  SplitKPool& pool = splitk_pool();
  std::lock_guard<std::mutex> lock(pool.mu);
  auto it = pool.per_stream.find(s);
  if (it != pool.per_stream.end()) { out = it->second; return out.ws != nullptr; }
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  SplitKScratch b;
  hipStream_t z = nullptr;
  bool ok = hipMalloc(&b.ws, kSplitKWsBytes) == hipSuccess && hipMalloc(&b.cnt, kSplitKCntBytes) == hipSuccess &&
            hipStreamCreateWithFlags(&z, hipStreamNonBlocking) == hipSuccess && hipMemsetAsync(b.cnt, 0, kSplitKCntBytes, z) == hipSuccess &&
            hipStreamSynchronize(z) == hipSuccess;
  if (z) (void)hipStreamDestroy(z);
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  if (!ok) { (void)hipGetLastError(); SplitKPool::drop(b); return false; }      // (not remembered: a later launch may find memory)
  pool.per_stream[s] = b;
  out = b;
  return true;
}
static void splitk_release(hipStream_t s, bool all) {
  SplitKPool& pool = splitk_pool();
  std::lock_guard<std::mutex> lock(pool.mu);
  if (all) { for (auto& kv : pool.per_stream) { (void)hipStreamSynchronize(kv.first); SplitKPool::drop(kv.second); } pool.per_stream.clear(); return; }
  auto it = pool.per_stream.find(s);
  if (it == pool.per_stream.end()) return;
  (void)hipStreamSynchronize(s);
  SplitKPool::drop(it->second);
  pool.per_stream.erase(it);
}

// one launch of a plan
static int launch(void* stream, const mx_gemm_desc* d, bool conv, const GemmRoute& r) {
  if (int rc = validate(d, conv)) return rc;
  // what the descriptor asks of the route
  if (d->stats_out) {
    MX_CHECK(r.stats_slabs > 0, "gemm: stats_out is not supported for this shape / epilogue (see mx_gemm_stats_slabs)");
    MX_CHECK(((uintptr_t)d->stats_out & 15) == 0, "gemm: stats_out must be 16-byte aligned");
  }
  if (d->gn_part_out) {
    if (const char* why = gn_part_refusal(d, r)) MX_CHECK(false, why);
    MX_CHECK(((uintptr_t)d->gn_part_out & 15) == 0, "gemm: gn_part_out needs M % 64 == 0, rows_per_batch % 64 == 0 and 16-byte alignment");
  }
  if (d->ln_final_out) {
    MX_CHECK(d->stats_out && d->ln_final_cnt && r.ln_final_out,
             "gemm: ln_final_out needs stats_out, ln_final_cnt and an ungrouped launch on a 256-row tile (mx_gemm_ln_final_supported)");
    MX_CHECK((((uintptr_t)d->ln_final_out & 15) | ((uintptr_t)d->ln_final_cnt & 3)) == 0, "gemm: ln_final_out must be 16-byte aligned");
  }
  if (d->ln_final) MX_CHECK(r.bn == 256, "gemm: ln_final is the 256 x 256 kernel's form of the folded LayerNorm; this shape does not run there (use ln_stats)");
  MX_CHECK(r.form >= 0, r.bn == 256 ? "gemm: no 256 x 256 instantiation serves ln_final with this epilogue (GEGLU, QKV or plain bias only)"
                                     : "gemm: no kernel instantiation serves this descriptor");
  GemmArgs a;
  fill_args(d, conv, r, a);
  hipStream_t s = (hipStream_t)stream;
  if (r.splitk > 1) {
    SplitKScratch sk;
    MX_CHECK(splitk_scratch(s, sk), "gemm: the split-K scratch (96 MB per stream) could not be allocated; set mx_gemm_desc.splitk = 1 to run unsplit");
    a.splitk = r.splitk; a.sk_ws = sk.ws; a.sk_cnt = sk.cnt;
  }
  if (prof_enabled()) {
    // algorithmic work: true (unpadded) contraction; bytes = operands read once + result written once
    const double kk = conv ? 9.0 * d->Cin : (double)d->K;
    const double Mt = (double)rows_of(d);
    double in_elems = conv ? 0 : Mt * d->K;
    for (int i = 0; conv && i < problems_of(d); ++i) { const mx_gemm_seg g = problem_of(d, i); in_elems += (double)g.B * g.Hin * g.Win * d->Cin; }
    const double flops = 2.0 * Mt * (double)d->N * kk;
    const double bytes = 2.0 * (in_elems + (double)d->N * d->K + Mt * d->N);
    const int kind = r.bn == 256 ? PROF_GEMM_V4_256 : r.bn ? (conv ? PROF_CONV_V2_160 : PROF_GEMM_V2_160) + (r.bn == 160 ? 0 : 2) : (conv ? PROF_CONV128 : PROF_GEMM128) + (d->N % 128 == 0 ? 0 : 1);
    prof_begin(s, kind, flops, bytes, (int)Mt, d->N, (int)kk);
  }
  int bad = 1;
  switch (r.family) {
    case FAM_GENERIC: bad = launch_generic(s, a, r.form); break;
    case FAM_ROWS_128: bad = launch_v2(s, a, r.form); break;
    // 256-row tiles: ping-pong schedule (gemm_bf16_v5.hip).  128-row tiles (small M) stay on the lock-step loop of gemm_bf16_v2.hip: the
    // ping-pong form is a tie there (same-box A/B, profiles/r03_d_gemm_bench_small_*: M2048 N1280 K1280 19.3 vs 19.2 us, conv B2 1280@32 98.9 vs
    // 108.5 us) -- with half the MFMAs per K tile its L phase (5 LDS-DMA issues + 14 fragment reads) outlasts the M phase
    case FAM_ROWS_256: bad = launch_v5(s, a, r.form); break;
    case FAM_PERSISTENT_256: bad = launch_v4(s, a, r.form); break;
    case FAM_SMALL_M: bad = launch_small_m(s, a, r.form); break;                   // M <= 16: a weight stream
    case FAM_CONV_SMALL_N: bad = launch_conv_small_n(s, a, r.form); break;         // N <= 16: the input read once
    case FAM_CONV_SMALL_CIN: bad = launch_conv_small_cin(s, a, r.form); break;     // <= 8 non-zero input channels: K = 72
  }
  MX_CHECK(bad == 0, "gemm: a family's launcher was handed a form outside its list");
  prof_end(s);
  MX_LAUNCH_CHECK();
  return 0;
}

static int run(void* stream, const mx_gemm_desc* d, bool conv) {
  MX_CHECK(d != nullptr, "gemm: null descriptor");
  MX_CHECK(d->n_segs >= 0 && d->n_segs <= MX_MAX_SEGS && (d->n_segs == 0 || d->segs != nullptr), "gemm: bad n_segs / segs");
  GemmPlan p;
  (void)plan_of(d, conv, p);
  for (int i = 0; i < p.n; ++i)
    if (int rc = launch(stream, p.d[i], conv, p.r[i])) return rc;
  return 0;
}

// Shape queries about another launch of d's problem: the one that also asks for statistics (stats = true), or the plain one without ln_stats /
// stats_out.  The chooser only looks at which operands exist.  (p may point at the local descriptor: the callers read routes only.)
static bool plan_of_variant(const mx_gemm_desc* d, bool stats, GemmPlan& p) {
  if (!d) return false;
  mx_gemm_desc q = *d;
  if (!stats) q.ln_stats = nullptr;
  q.stats_out = !stats ? nullptr : d->stats_out ? d->stats_out : reinterpret_cast<float*>(16);
  return plan_of(&q, false, p);
}

// ---- mx_conv3x3_halo / mx_conv3x3_halfrow (conv_halo.hip): entries of their own beside the routes above -- the plan asks mx_conv3x3_halo_serves, then
//      mx_conv3x3_halfrow_serves, and calls the one that serves, or mx_conv3x3 ----
int launch_conv_halo(hipStream_t s, const GemmArgs& a, bool vec, bool half_rows);
int conv_halo_lds_bytes(int width, bool half_rows);      // 0: no instantiation for that image width

// what both forms ask of d, but for the image's width and height (the conditions: include/mxdenoise.h)
static bool conv_staged_common(const mx_gemm_desc* d) {
  if (!d || d->n_segs != 0 || d->stride != 1 || d->up != 0 || d->vhalo != 0 || d->corner_patch != 0) return false;
  if (d->Cin <= 0 || d->Cin % 64 != 0 || d->Cin > 8192 || d->K != 9 * d->Cin || d->cin_valid != 0) return false;
  if (d->N <= 0 || d->N % 160 != 0) return false;
  if (d->B <= 0 || d->Hin <= 0 || d->Win <= 0 || d->Hout != d->Hin || d->Wout != d->Win) return false;
  if ((long)d->B * d->Hin * d->Win != d->M) return false;
  if (d->flags != 0 || d->gate || d->out_scale != 0.f || d->splitk > 1) return false;
  if (d->rows_per_batch != 0 && d->rows_per_batch != d->Hin * d->Win) return false;
  // the register-exchange epilogue moves 16-byte pieces of C and of the residual
  if (d->ldc % 8 != 0 || ((uintptr_t)d->c & 15) != 0) return false;
  if (d->residual && (d->ldr % 8 != 0 || ((uintptr_t)d->residual & 15) != 0)) return false;
  return true;
}

// LDS bytes of the launch, 0 when the kernel does not serve d
static int conv_halo_serves(const mx_gemm_desc* d) {
  if (!conv_staged_common(d) || (long)d->Hin * d->Win % 256 != 0) return 0;
  // shapes of the SDXL step whose median did not beat the tap-major kernel's by more than that kernel's own p10..p90 width in the per-shape A/B
  // (tools/conv_halo_bench.py, profiles/conv_halo_ab.txt): the two shortest K loops, +20.7 us against a width of 24.6 and +25.9 against 28.7
  static const int kNotFaster[][3] = {{32, 640, 1280}, {64, 320, 640}};      // {width, Cin, N}
  for (const auto& s : kNotFaster) if (d->Win == s[0] && d->Cin == s[1] && d->N == s[2]) return 0;
  return conv_halo_lds_bytes(d->Win, false);
}

// the half-row form: a 128-wide image in tiles of 4 rows x 64 columns
static int conv_halfrow_serves(const mx_gemm_desc* d) {
  if (!conv_staged_common(d) || d->Win != 128 || d->Hin % 4 != 0) return 0;
  return conv_halo_lds_bytes(d->Win, true);
}

static int run_conv_halo(void* stream, const mx_gemm_desc* d, bool half_rows) {
  MX_CHECK(d != nullptr, "conv3x3_halo: null descriptor");
  if (half_rows) MX_CHECK(conv_halfrow_serves(d) > 0, "conv3x3_halfrow: the descriptor is not served (mx_conv3x3_halfrow_serves); run mx_conv3x3");
  else MX_CHECK(conv_halo_serves(d) > 0, "conv3x3_halo: the descriptor is not served (mx_conv3x3_halo_serves); run mx_conv3x3");
  if (int rc = validate(d, true)) return rc;
  MX_CHECK(!d->stats_out && !d->ln_final_out, "conv3x3_halo: no row statistics");
  if (d->gn_part_out)      // (gn_part_refusal's conditions on the descriptor; the tile is 256 rows)
    MX_CHECK(!d->residual && (!d->rowbias || d->rows_per_batch % 64 == 0) && ((uintptr_t)d->gn_part_out & 15) == 0,
             "conv3x3_halo: gn_part_out needs an epilogue of bias (+ row bias) only and 16-byte alignment");
  GemmRoute r;
  r.bn = 160; r.rows = 256;
  GemmArgs a;
  fill_args(d, true, r, a);
  hipStream_t s = (hipStream_t)stream;
  if (prof_enabled()) {      // the conv kind of the 256 x 160 tile: the same algorithmic work as launch() counts
    const double kk = 9.0 * d->Cin, Mt = (double)d->M;
    prof_begin(s, PROF_CONV_V2_160, 2.0 * Mt * (double)d->N * kk, 2.0 * (Mt * d->Cin + (double)d->N * d->K + Mt * d->N), d->M, d->N, (int)kk);
  }
  MX_CHECK(launch_conv_halo(s, a, d->rowbias != nullptr, half_rows) == 0, "conv3x3_halo: no instantiation for this image width");
  prof_end(s);
  MX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mx

extern "C" int mx_conv3x3_halo_serves(const mx_gemm_desc* d) { return mx::conv_halo_serves(d); }
extern "C" int mx_conv3x3_halo(void* stream, const mx_gemm_desc* d) { return mx::run_conv_halo(stream, d, false); }
extern "C" int mx_conv3x3_halfrow_serves(const mx_gemm_desc* d) { return mx::conv_halfrow_serves(d); }
extern "C" int mx_conv3x3_halfrow(void* stream, const mx_gemm_desc* d) { return mx::run_conv_halo(stream, d, true); }
extern "C" int mx_gemm(void* stream, const mx_gemm_desc* d) { return mx::run(stream, d, false); }
extern "C" int mx_conv3x3(void* stream, const mx_gemm_desc* d) { return mx::run(stream, d, true); }
extern "C" void mx_gemm_release_scratch(void* stream, int all) { mx::splitk_release((hipStream_t)stream, all != 0); }

/* launches mx_gemm(d) issues: 2 where the tail split applies (tests, planning) */
extern "C" int mx_gemm_launches(const mx_gemm_desc* d) { mx::GemmPlan p; return mx::plan_of(d, false, p) ? p.n : 1; }
extern "C" int mx_gemm_form(const mx_gemm_desc* d, int conv) { mx::GemmPlan p; return mx::plan_of(d, conv != 0, p) ? (int)p.r[0].family : MX_FORM_TILE_GENERIC; }
extern "C" int mx_gemm_splitk(const mx_gemm_desc* d, int conv) { mx::GemmPlan p; return mx::plan_of(d, conv != 0, p) ? p.r[0].splitk : 0; }
extern "C" int mx_gemm_gn_partials_supported(const mx_gemm_desc* d, int conv) { mx::GemmPlan p; return mx::plan_of(d, conv != 0, p) && p.r[0].gn_part; }
extern "C" int mx_gemm_stats_slabs(const mx_gemm_desc* d) { mx::GemmPlan p; return mx::plan_of_variant(d, true, p) ? p.r[0].stats_slabs : 0; }
extern "C" int mx_gemm_ln_final_supported(const mx_gemm_desc* d) { mx::GemmPlan p; return mx::plan_of_variant(d, true, p) && p.r[0].ln_final_out; }
extern "C" int mx_gemm_ln_prefers_pass(const mx_gemm_desc* d) { mx::GemmPlan p; return mx::plan_of_variant(d, false, p) && p.r[0].bn == 256; }
/* name of the kernel instantiation launch number `launch` (0, or 0 / 1 under the tail split) of mx_gemm / mx_conv3x3 would run (host only) */
extern "C" int mx_gemm_kernel_name(const mx_gemm_desc* d, int conv, int launch, char* buf, int cap) {
  mx::GemmPlan p;
  if (launch < 0 || !mx::plan_of(d, conv != 0, p)) return -1;
  if (launch >= p.n) return 0;
  if (p.r[launch].form < 0) return -1;
  return mx::copy_name(mx::kGemmKernelNames[p.r[launch].form], buf, cap);
}
extern "C" int mx_gemm_kernel_names(char* buf, int cap) { return mx::join_names(mx::kGemmKernelNames, mx::GK_COUNT, buf, cap); }
