// bf16 MFMA GEMM / implicit-GEMM conv3x3, 128-row lock-step tiles with split-K for gfx950 (MI355X): the small launches (one request, mixed
// batches: M <= ~4k rows), where a 256-row tile would leave most of the chip's 256 CUs idle.  The 256-row tiles of the large launches run the
// ping-pong schedule of gemm_bf16_v5.hip, which replaced the lock-step 256-row instantiation once built here (git history; A/B in
// profiles/r03_*gemm_bench*).
//
// Same math, orientation, swizzle and epilogue semantics as gemm_bf16.hip (the generic fallback); what changes is the schedule:
//   * tile 128 tokens x BN features (BN = 160 or 128) x 64 k, 512 threads = 8 waves as 4(m) x 2(n); one tile -- or, under split-K, one K slice
//     of a tile -- per workgroup; the slices of a tile are summed by its last-arriving workgroup in slice order (gemm_args.h splitk_combine);
//   * operands go HBM/L2 -> LDS directly (global_load_lds_dwordx4, no staging VGPRs / ds_write), XOR swizzle applied on the per-lane SOURCE
//     address (the LDS image of an LDS-DMA is lane-linear; cdna guide rule 21): the loader shared with the 256-row tiles,
//     gemm_dma_loader.h / gemm_dma_loader.inc;
//   * LDS ring of four or five stages (RingDepth below), counted s_waitcnt vmcnt(N) + raw s_barrier, one barrier per K tile (cdna guide
//     "Pipelining across barriers").  All LDS lives in ONE __shared__ array and the K loop contains no ordinary global load.  A DMA group is
//     issued in EVERY iteration (past the end of the K range it reads a zero page into a stage nobody reads), so one counted wait serves every
//     iteration.  The DMA issue is branch-free and shares a basic block with the MFMAs: each LDS-DMA and the fragment reads of k-step 1 sit in
//     MFMA shadows (sched_group_barrier); all control flow of the loader (next K tile / next conv tap) runs after the MFMAs;
//   * epilogue: gemm_epilogue_regs (gemm_args.h) transposes the accumulators in registers, so global stores and residual loads move whole
//     128-byte lines per token without LDS or a barrier.
#include <cstdlib>

#include "common.h"
#include "../../include/mxdenoise.h"
#include "gemm_args.h"
#include "gemm_forms.h"
#include "gemm_dma_loader.h"

namespace mx {

// LDS ring depth.  A small launch (one request, mixed batches: M <= ~4k rows) is LATENCY-bound: a CU streams its operands from HBM / a remote
// L2 at ~2 us per round trip, so with two tiles in flight an iteration cannot be shorter than ~1 us whatever the tile (measured: 22.5 us for
// M 512, 23.2 us for M 2048 at N 1280, K 1280 = 20 K tiles).  The 128-row tiles therefore run four (BN 160: 147 KB) or five (BN 128: 160 KB)
// stages, loads three / four tiles ahead.  (MI = 4, the 256-row lock-step tile, filled the 160 KB with three; it is no longer built.)
template <int BN, int MI> struct RingDepth { static constexpr int value = MI == 4 ? 3 : (BN == 160 ? 4 : 5); };

// MI: 16-wide token blocks per wave; tile rows BM2 = 64 * MI (256, or 128 for small M); FEAT / GEGLU: the epilogue features compiled in
// (gemm_args.h EPI_F_*; the launcher picks the smallest instantiation that serves the launch)
template <int BN, int MI, bool CONV, int FEAT, bool GEGLU>
__global__ __launch_bounds__(512, 2) void gemm_v2_kernel(const GemmArgs pk) {
  constexpr int BM2 = 64 * MI;
  constexpr int NI = BN / 32;                 // 16-wide feature blocks per wave (wave covers BN/2 features)
  constexpr int LOADS = DmaTile<BN, MI>::LOADS;
  constexpr int NSTAGE = RingDepth<BN, MI>::value;
  __shared__ __attribute__((aligned(16))) bf16_t smem[NSTAGE * DmaTile<BN, MI>::STAGE_ELEMS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1;
  const int wn = wave & 1;
  // this workgroup's output tile; in a grouped launch (gemm_args.h) also its problem: p is that problem from here on
  GemmArgs p = pk;
  int tm, tn;
  // split-K: workgroups [s * tiles, (s + 1) * tiles) are slice s of every tile (tiles % 8 == 0 keeps a tile's slices on one XCD: speed only)
  const int n_tiles = gemm_m_tiles(pk, BM2) * (pk.N / BN);
  const int slice = pk.splitk > 1 ? (int)blockIdx.x / n_tiles : 0;
  const int tile_id = (int)blockIdx.x - slice * n_tiles;
  gemm_tile_of_block(tile_id, gemm_m_tiles(pk, BM2), pk.N / BN, pk.xcd_map, tm, tn);
  gemm_select_seg(p, pk, tm);
  const int nk_all = p.K / DMA_BK;
  const int k_first = pk.splitk > 1 ? (int)((long)nk_all * slice / pk.splitk) : 0;
  const int nk = pk.splitk > 1 ? (int)((long)nk_all * (slice + 1) / pk.splitk) - k_first : nk_all;
  constexpr bool SPLIT_K = true;
#include "gemm_dma_loader.inc"   // the operand stream: setup_tile(), issue_group(stage) in the MFMAs' basic block, advance_cursor() after them
  auto issue_next = [&](int stage) __attribute__((always_inline)) { issue_group(stage); advance_cursor(); };   // prologue form

  const int fr = lane & 15;
  const int fq = lane >> 4;

  auto load_frags = [&](int stage, int ks, bf16x8 (&wf)[NI], bf16x8 (&xf)[MI]) {
    const bf16_t* sx = smem + stage * STAGE_ELEMS;
    const bf16_t* sw = sx + BM2 * DMA_BK;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = wn * (BN / 2) + i * 16 + fr;
      wf[i] = *reinterpret_cast<const bf16x8*>(&sw[row * DMA_BK + swz(row, ks * 4 + fq) * 8]);
    }
#pragma unroll
    for (int j = 0; j < MI; ++j) {
      const int row = wm * 16 * MI + j * 16 + fr;
      xf[j] = *reinterpret_cast<const bf16x8*>(&sx[row * DMA_BK + swz(row, ks * 4 + fq) * 8]);
    }
  };
  constexpr int NM = NI * MI;
  constexpr int NF = NI + MI;

  setup_tile();
#pragma unroll
  for (int st = 0; st < NSTAGE - 1; ++st) issue_next(st);

  int stage = 0;   // ring stage of the K tile being computed (stream position modulo 3)
  {
    f32x4 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ln_rstd[MI];                          // folded LayerNorm (gemm_ln_init): while the first operand tiles are in flight
#pragma unroll
    for (int j = 0; j < MI; ++j) ln_rstd[j] = 1.0f;
    if constexpr (!CONV) {
      if (p.ln_stats != nullptr) {
        gemm_ln_init<NI, MI>(p, acc, tm * BM2 + wm * 16 * MI, tn * BN + wn * (BN / 2), fr, fq, ln_rstd);
        if (slice != 0) {                      // split-K: the -mean * colsum term enters the sum once, through slice 0
#pragma unroll
          for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }

    for (int kt = 0; kt < nk; ++kt) {
      // all but the NSTAGE - 2 youngest DMA groups of this thread have completed => the K tile of this iteration has landed
      constexpr int INFLIGHT = LOADS * (NSTAGE - 2);
      wait_vmcnt<INFLIGHT>();
      __builtin_amdgcn_s_barrier();
      bf16x8 wf0[NI], xf0[MI], wf1[NI], xf1[MI];
      load_frags(stage, 0, wf0, xf0);
      const int st2 = stage >= 1 ? stage - 1 : NSTAGE - 1;   // (g + NSTAGE - 1) % NSTAGE: last read in iteration g-1, which every wave has left
      issue_group(st2);
      load_frags(stage, 1, wf1, xf1);
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf0[i], xf0[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1[i], xf1[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, NF, 0);                 // fragment reads of k-step 0
#pragma unroll
      for (int s = 0; s < LOADS; ++s) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                // MFMA
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                // one LDS-DMA (VMEM read)
      }
#pragma unroll
      for (int s = 0; s < (NF + 1) / 2; ++s) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                // fragment reads of k-step 1
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * NM - LOADS - (NF + 1) / 2, 0);
      advance_cursor();
      stage = stage == NSTAGE - 1 ? 0 : stage + 1;
    }

    const int m0 = tm * BM2, n0 = tn * BN;
    if (pk.splitk > 1) {                       // only the last-arriving slice of the tile goes on, with the sum of all slices
      if (!splitk_combine<NI, MI>(pk, acc, tile_id, slice, BM2 * BN, reinterpret_cast<volatile int*>(smem))) return;
    }
    // register-exchange epilogue (gemm_args.h): no LDS, no barrier; the past-the-end DMAs are drained before the workgroup retires
    static_assert(!GEGLU || (NI % 4 == 0 && !CONV), "the gated epilogue pairs whole 32-feature halves");
    gemm_epilogue_regs<NI, MI, GEGLU, true, true, true, FEAT>(p, acc, m0 + wm * 16 * MI, n0 + wn * (BN / 2), fr, fq, ln_rstd);
    wait_vmcnt<0>();
  }
}

// This file serves the 128-row tiles (small M: one request, mixed batches); the 256-row tiles run the
// ping-pong schedule of gemm_bf16_v5.hip (the lock-step 256-row instantiation it replaced: git history, A/B in profiles/r03_*gemm_bench*).
int launch_v2(hipStream_t s, const GemmArgs& a, int form) {
  const int tiles = (a.nseg > 0 ? a.mt_total : cdiv(a.M, 128)) * (a.splitk > 1 ? a.splitk : 1);      // x N / BN: 160 or 128 features per tile
  switch (form) {                             // the instantiation the route names (gemm_dispatch.cpp): gemm_forms.h
#define MX_V2(id, k, targs) case id: hipLaunchKernelGGL((k<MX_FORM_UNPAREN targs>), dim3(tiles * (a.N / (MX_FORM_FIRST targs))), dim3(512), 0, s, a); return 0;
    MX_GEMM_V2_FORMS(MX_V2)
#undef MX_V2
    default: return 1;
  }
}

}  // namespace mx
