// The tile body of the 256-row ping-pong GEMM / implicit-GEMM conv (gemm_bf16_v5.hip holds the description and the stand-alone kernel): one
// 256 x {160, 128} output tile per call, every thread of a 512-thread workgroup calls.  Shared with the chained launch of attn_tail.hip, which walks
// several dependent GEMM stages in ONE launch on exactly this code -- same tiles, same order of summation, same epilogue: same bits.
#pragma once
#include "common.h"
#include "../../include/mxdenoise.h"
#include "gemm_args.h"
#include "gemm_dma_loader.h"

namespace mx {

constexpr int NSTAGE5 = 3;

#if defined(MX_EXP) && MX_EXP == 8   // diagnostic build: wall-clock stamps (100 MHz s_memrealtime) per workgroup, read back by tools/exp/timeline_v4.py
static __device__ unsigned long long g_v5_stamps[1024 * 2 * 4];
#define MX5_STAMP(slot) do { if (lane == 0 && (wave == 0 || wave == 7) && blockIdx.x < 1024) \
    g_v5_stamps[(blockIdx.x * 2 + (wave == 7)) * 4 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define MX5_STAMP(slot) do {} while (0)
#endif

// MI: 16-wide token blocks per wave; tile rows BM5 = 64 * MI (256, or 128 for small M); FEAT / GEGLU: the epilogue features compiled in
// (gemm_args.h EPI_F_*; the launcher picks the smallest instantiation that serves the launch)
// VEC: the per-sample vectors (row bias, gate) are compiled in -- 40 registers of the epilogue; without them the QKV form does not spill
// WT: the tile's output (and its row statistics) leave as WRITE-THROUGH (sc1) stores -- the chained launch (attn_tail.hip) hands them to other
// workgroups inside the launch; the arithmetic is the same instruction sequence, so a tile's values do not depend on WT.
// tm / tn: the tile (the stand-alone kernel derives them from blockIdx, a chained launch from its work ticket); smem: NSTAGE5 stages.
template <int BN, int MI, bool CONV, int FEAT, bool GEGLU, bool VEC, bool WT = false>
__device__ __forceinline__ void gemm_v5_tile(const GemmArgs& pk, int tm, const int tn, bf16_t* const smem) {
  constexpr int BM5 = 64 * MI;
  constexpr int NI = BN / 32;                 // 16-wide feature blocks per wave (BN / 2 features)
  constexpr int LOADS = DmaTile<BN, MI>::LOADS;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1;                   // 0..3: token quarter of the tile; groups: wm 0-1 = A, wm 2-3 = B
  const int wn = wave & 1;
  const bool group_b = wave >= 4;
  MX5_STAMP(0);
  GemmArgs p = pk;
  gemm_select_seg(p, pk, tm);
  const int nk = p.K / DMA_BK;
  constexpr bool SPLIT_K = false;             // the stream is the whole K range
  constexpr int k_first = 0;
#include "gemm_dma_loader.inc"   // the operand stream: setup_tile(), issue_group(stage), advance_cursor()

  const int fr = lane & 15;
  const int fq = lane >> 4;
  // fragment addresses (bytes inside a stage): lane (fr, fq) reads row base + fr, chunk 4 ks + fq
  unsigned wrd[2], xrd[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int wrow = wn * (BN / 2) + fr, xrow = wm * 16 * MI + fr;
    wrd[ks] = (unsigned)(((BM5 * DMA_BK) + wrow * DMA_BK + swz(wrow, ks * 4 + fq) * 8) * 2);   // (16 i more rows keep the swizzle: (row >> 1) & 7 of row + 16 i)
    xrd[ks] = (unsigned)((xrow * DMA_BK + swz(xrow, ks * 4 + fq) * 8) * 2);
  }

  setup_tile();
  issue_group(0); advance_cursor();
  issue_group(1); advance_cursor();
  wait_vmcnt<LOADS>();                        // all of this thread's DMA groups but the youngest: own part of K tile 0 landed

  f32x4 acc[NI][MI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ln_rstd[MI];
#pragma unroll
  for (int j = 0; j < MI; ++j) ln_rstd[j] = 1.0f;
  if constexpr (!CONV) {
    if (p.ln_stats != nullptr) gemm_ln_init<NI, MI>(p, acc, tm * BM5 + wm * 16 * MI, tn * BN + wn * (BN / 2), fr, fq, ln_rstd);
  }
  MX_BAR();                                  // every wave's part of K tile 0 has landed
  if (group_b) MX_BAR();                     // group B runs one barrier behind group A
  MX5_STAMP(1);

  int stage = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // ---- L: all fragments of this K tile, the DMA share of tile kt + 2, the cursor ----
    const char* sb = reinterpret_cast<const char*>(smem) + stage * (STAGE_ELEMS * 2);
    bf16x8 wf[2][NI], xf[2][MI];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < NI; ++i) wf[ks][i] = *reinterpret_cast<const bf16x8*>(sb + wrd[ks] + i * (16 * DMA_BK * 2));
#pragma unroll
      for (int j = 0; j < MI; ++j) xf[ks][j] = *reinterpret_cast<const bf16x8*>(sb + xrd[ks] + j * (16 * DMA_BK * 2));
    }
    const int st2 = stage >= 1 ? stage - 1 : NSTAGE5 - 1;      // (kt + 2) % 3: the stage of K tile kt - 1
    issue_group(st2);
    advance_cursor();
    wait_vmcnt<LOADS>();                                        // own part of K tile kt + 1
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the fragment reads have returned: the stage may be restaged one phase from now
    __builtin_amdgcn_sched_barrier(0);
    MX_BAR();
    // ---- M: registers only ----
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks][i], xf[ks][j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    MX_BAR();
    stage = stage == NSTAGE5 - 1 ? 0 : stage + 1;
  }
  MX5_STAMP(2);
  if (!group_b) MX_BAR();                    // re-align the two groups

  const int m0 = tm * BM5, n0 = tn * BN;
  static_assert(!GEGLU || (NI % 4 == 0 && !CONV), "the gated epilogue pairs whole 32-feature halves");
  gemm_epilogue_regs<NI, MI, GEGLU, VEC, true, true, FEAT, true, false, WT>(p, acc, m0 + wm * 16 * MI, n0 + wn * (BN / 2), fr, fq, ln_rstd);
  if constexpr (!GEGLU && FEAT == 0 && MI == 4) {      // GroupNorm partial sums of the accumulators (gemm_args.h): pure ALU + 10 stores behind the tile's own
    if (pk.gn_part != nullptr) gemm_gn_partials<NI, MI>(p, acc, m0 + wm * 16 * MI, n0 + wn * (BN / 2), fr, fq);
  }
  MX5_STAMP(3);
  wait_vmcnt<0>();                                     // the past-the-end DMAs are drained before the workgroup retires
  if constexpr (!CONV && !GEGLU && BM5 == 256) {      // finalised row statistics: the last workgroup of the 256-row panel folds its slabs (gemm_args.h)
    if (pk.ln_final_out != nullptr) gemm_ln_finalize(p, tm, pk.N / BN, reinterpret_cast<volatile int*>(smem));
  }
}


}  // namespace mx
