// bf16 MFMA GEMM / implicit-GEMM conv3x3, 256 tokens x {160, 128} features, PING-PONG schedule of the two wave-row pairs (round 3).
//
// Same tile, loader (LDS-DMA with the XOR swizzle on the source address, zero page for padding taps, per-tap row pointers), math, orientation
// and epilogue as the 256-row form of gemm_bf16_v2.hip -- what changes is how the eight waves share the CU.  gemm_v2's loop is lock-step: all
// eight waves wait, pass ONE barrier per K tile, read their 18 fragments together (LDS saturated, matrix pipe idle), then compete for the
// matrix pipe together.  Measured there (profiles/r02_g_shape_profile_b4.txt): 1.15 us per K tile against 0.62 us of matrix-pipe time and
// 0.62 us of operand streaming -- the two ADD instead of overlapping.  gemm_v4 (256 x 256) removed that for the large-N launches; this kernel
// does it for the N <= 1280 family and the convs, a third of the step each.
//
//   waves 0-3 (token rows 0-127 of the tile) = group A, waves 4-7 (rows 128-255) = group B: every SIMD holds one wave of each group.
//   per K tile and wave:   L | M        (| = s_barrier; group B runs the same program ONE barrier behind group A)
//     L  read ALL fragments of the K tile (10 W + 8 X ds_read_b128 for BN 160), issue the wave's share of the LDS-DMA for K tile t + 2,
//        move the loader's cursor (tap changes of the conv included), wait until its own DMA of tile t + 1 has landed (counted vmcnt) and
//        its fragment reads have returned (lgkmcnt 0)
//     M  40 MFMAs on registers only
//   so in every phase one group streams operands while the other owns the matrix pipe.
//   * LDS: the same three-stage ring (all 160 KB).  K tile t + 2 overwrites the stage of tile t - 1, last read by group B one phase before
//     group A issues (reads retired by the lgkmcnt(0) in front of the barrier: cdna guide, "restage a buffer 1 phase after when an lgkmcnt
//     before the reading phase's first barrier retired those reads") and two phases before group B issues;
//   * RAW: a wave's DMA of tile t + 1 is waited for in its L phase of tile t, at least one barrier before either group reads it;
//   * the groups re-align for the register-exchange epilogue (group A takes one extra barrier after the loop, group B one before it).
#include <cstdlib>

#include "common.h"
#include "../../include/mxdenoise.h"
#include "gemm_args.h"
#include "gemm_forms.h"
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
// The tile (tm, tn) is a function of its own, called once by the kernel below: written straight into the kernel body the same statements compile to
// the same work in another instruction order and register assignment in all 14 instantiations (profiles/one_path_isa.txt), and the schedule
// was tuned in this form.  smem: NSTAGE5 stages.
template <int BN, int MI, bool CONV, int FEAT, bool GEGLU, bool VEC>
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
  gemm_epilogue_regs<NI, MI, GEGLU, VEC, true, true, FEAT, true, false>(p, acc, m0 + wm * 16 * MI, n0 + wn * (BN / 2), fr, fq, ln_rstd);
  if constexpr (!GEGLU && FEAT == 0 && MI == 4) {      // GroupNorm partial sums of the accumulators (gemm_args.h): pure ALU + 10 stores behind the tile's own
    if (pk.gn_part != nullptr) gemm_gn_partials<NI, MI>(p, acc, m0 + wm * 16 * MI, n0 + wn * (BN / 2), fr, fq);
  }
  MX5_STAMP(3);
  wait_vmcnt<0>();                                     // the past-the-end DMAs are drained before the workgroup retires
  if constexpr (!CONV && !GEGLU && BM5 == 256) {      // finalised row statistics: the last workgroup of the 256-row panel folds its slabs (gemm_args.h)
    if (pk.ln_final_out != nullptr) gemm_ln_finalize(p, tm, pk.N / BN, reinterpret_cast<volatile int*>(smem));
  }
}

template <int BN, int MI, bool CONV, int FEAT, bool GEGLU, bool VEC>
__global__ __launch_bounds__(512, 2) void gemm_v5_kernel(const GemmArgs pk) {
  constexpr int STAGE_ELEMS = (64 * MI + BN) * DMA_BK;
  __shared__ __attribute__((aligned(16))) bf16_t smem[NSTAGE5 * STAGE_ELEMS];
  int tm, tn;
  gemm_tile_of_block(blockIdx.x, gemm_m_tiles(pk, 64 * MI), pk.N / BN, pk.xcd_map, tm, tn);
  gemm_v5_tile<BN, MI, CONV, FEAT, GEGLU, VEC>(pk, tm, tn, smem);
}

// 256 rows x 160 or 128 features per tile (the 128-row instantiation MI = 2 was measured and is not built: see launch() in gemm_dispatch.cpp)
int launch_v5(hipStream_t s, const GemmArgs& a, int form) {
  const int mt = a.nseg > 0 ? a.mt_total : cdiv(a.M, 256);
  switch (form) {                             // the instantiation the route names (gemm_dispatch.cpp): gemm_forms.h
#define MX_V5(id, k, targs) case id: hipLaunchKernelGGL((k<MX_FORM_UNPAREN targs>), dim3(mt * (a.N / (MX_FORM_FIRST targs))), dim3(512), 0, s, a); return 0;
    MX_GEMM_V5_FORMS(MX_V5)
#undef MX_V5
    default: return 1;
  }
}

}  // namespace mx

#if defined(MX_EXP) && MX_EXP == 8
extern "C" int mx_debug_v5_stamps(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mx::g_v5_stamps), sizeof(mx::g_v5_stamps)); }
#endif
