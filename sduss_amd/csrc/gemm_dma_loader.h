// What the LDS-DMA GEMM / implicit-GEMM conv3x3 kernels share: the K-tile depth, the XOR chunk swizzle, the 16-byte global -> LDS copy, the raw
// barrier, the counted wait, the zero page and the shape of a tile's operand stream.  gemm_bf16_v2.hip (128-row lock-step tiles) and
// gemm_bf16_v5.hip (256-row ping-pong tiles) also share ONE operand loader, gemm_dma_loader.inc;
// gemm_bf16_v4.hip takes the primitives only: its four half-tile cursors are a different loader.
//
// Why the loader is a fragment included into the kernel body and not a struct here: it was tried as one (cursor state + setup / issue / advance
// members; with the constant context as members or as arguments; with constant-index unrolling).  Every such form compiles to the same work,
// but the optimiser takes the aggregate apart at a different point of its pipeline than it does separate locals, and the instruction order and
// register assignment of all the kernels move with it; the SGPR count of the conv forms moved by 1-4.  As locals and always-inline lambdas of
// the kernel -- the form the schedules were tuned in -- every kernel kept their register and LDS budget and their instruction
// stream to the letter (profiles/loader_refactor_isa.txt: the table, and a timed example of what a 2-instruction difference in the tile set-up
// cost).  Re-run that comparison when the fragment changes.
#pragma once
#include "common.h"
#include "gemm_args.h"

namespace mx {

constexpr int DMA_BK = 64;                    // K-tile depth: 64 bf16 = one 128-byte row of eight 16-byte chunks

// zero page the loaders read for padding taps / past-the-end DMAs: as long as the widest input channel count (2 * Cin bytes); one per
// translation unit that includes this header (device symbols are not linked across them)
[[maybe_unused]] static __device__ __attribute__((aligned(64))) unsigned int g_zero_page[16384 / 4] = {0};

// slot `chunk` of LDS row `row` holds logical k-chunk swz(row, chunk) (and the other way round: the XOR is its own inverse).  An LDS-DMA's
// LDS image is lane-linear, so the loaders apply this on the per-lane SOURCE address and the fragment reads on the LDS address.
__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// global_load_lds_dwordx4: 16 bytes per lane from gsrc (per lane) to lds_dst (wave-uniform base) + lane * 16; no staging VGPRs; counts in vmcnt
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// raw barrier that neither the compiler's memory motion nor its instruction scheduler crosses
#define MX_BAR()                                  \
  do {                                            \
    asm volatile("" ::: "memory");                \
    __builtin_amdgcn_s_barrier();                 \
    asm volatile("" ::: "memory");                \
    __builtin_amdgcn_sched_barrier(0);            \
  } while (0)

// counted wait: all but the N youngest vector-memory operations (LDS-DMAs included) of this thread have completed
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "s_waitcnt vmcnt is a 6-bit field on gfx9");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// compile-time shape of the operand stream of a BM x BN output tile (BM = 64 * MI) loaded by 512 threads
template <int BN, int MI>
struct DmaTile {
  static constexpr int BM = 64 * MI;
  static constexpr int WCH = BN * 8;                 // 16-byte chunks of the W tile
  static constexpr int XI = BM * 8 / 512;            // X load instructions per thread per K tile (4, or 2 for the 128-row tile)
  static constexpr int WI = (WCH + 511) / 512;       // W load instructions per thread per K tile (3 for BN 160, 2 for 128)
  static constexpr int LOADS = XI + WI;              // per-thread DMA instructions per K tile
  static constexpr int STAGE_ELEMS = (BM + BN) * DMA_BK;   // a ring stage: the X tile, then the W tile
};

}  // namespace mx
