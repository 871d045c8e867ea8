// bf16 MFMA implicit-GEMM conv3x3 (pad 1, stride 1), 256 output pixels x 160 features per tile, the input staged ONCE per 64-channel chunk.
//
// The tap-major conv of gemm_bf16_v5.hip copies the 256 x 64 activation tile from L2 into LDS once per tap: nine copies of (almost) the same
// pixels per channel chunk, 4 of the 7 LDS-DMA instructions of every load phase.  Here a tile is R whole image rows (R = 256 / W: 8 at width 32,
// 4 at width 64), K runs CHUNK-major, and per 64-channel chunk the (R + 2) x W input pixels the nine taps read are staged once, as whole
// 128-byte pixel lines.  The nine taps of the chunk are nine K tiles on the same staged buffer: tap (dy, dx) of output pixel p reads line
// p + (dy + 1) W + dx, a constant offset per tap.
//
//   * waves, accumulator layout, ping-pong schedule (group A = waves 0-3, group B one barrier behind), the three-stage weight ring, the counted
//     waits and the epilogue (gemm_epilogue_regs, gemm_gn_partials) are those of gemm_v5_tile<160, 4, true, 0, false, VEC>: see that file;
//   * LDS: two staged buffers of (R + 2) W lines (40 KB at width 32, 48 KB at width 64), the weight ring (3 x 20 KB), two zero lines;
//   * swizzle: slot c of line P holds logical chunk c ^ ((P >> 1) & 7), applied on the DMA's source address.  (dy + 1) W and the 16-pixel
//     blocks of a wave are multiples of 16 lines, so a lane's key depends on dx alone: three keys per lane, computed once;
//   * rows above / below the image come from the zero page; the columns x = -1 and x = W are never stored (a tile spans the width): the lanes
//     of those pixels (lane row 0 of a block at x = 0 for dx = -1, lane row 15 of a block ending at x = W - 1 for dx = +1) read a zero line
//     in LDS, at the bank position the staged line would have had;
//   * the DMA of chunk c + 1 is dealt over the load phases of taps 0..7 of chunk c (one piece in 5 or 6 of them) into the other buffer, whose
//     last reads (tap 8 of chunk c - 1) were retired by the lgkmcnt(0) + barrier in front of tap 0 -- the re-staging rule at the top of
//     gemm_bf16_v5.hip.  Every wave's counted wait in the load phase of tap 8 covers its pieces, one barrier before either group reads them;
//   * weights keep their packed (kh, kw, cin) order: the K tile of (chunk c, tap t) starts at column t Cin + 64 c.
//
//
// HALF (images 128 pixels wide): two whole rows would stage 4 x 128 lines = 64 KB per buffer, and two such buffers do not fit beside the weight ring.
// A tile is then a HALF ROW BLOCK: 4 output rows x 64 columns at column origin xo = 0 or 64 -- the staged geometry, tap offsets and swizzle keys of the
// W = 64 form, read from an image whose row stride is 128 pixels (row tile tm = 2 (block of 4 rows) + half).  One of the two side columns is now a real
// neighbour (column 63 for the right half, 64 for the left half), the other is still the image edge:
//   * per staged buffer 8 more lines (1 KB): SIDE line s holds the neighbour column's pixel of staged row s (6 lines; 2 of padding), staged once per
//     chunk by ONE LDS-DMA instruction of wave 0 in the load phase of tap 3 (no other piece is dealt there), whose spare lanes fetch zero-page bytes;
//     that wave counts one more outstanding DMA in that phase's wait.  A side line carries the swizzle key of the staged line it stands in for
//     (7 for tile column -1, 0 for tile column 64), on the DMA's source address and on the read;
//   * the edge lane on the neighbour side reads side line wm + dy + 1 instead of the zero line; the lane on the image-edge side keeps the zero line.
//     Which side is which is wave-uniform (the tile's half).  A side line sits at the bank position of the line it replaces when wm + dy has the
//     right parity, else in the other bank half (a two-way conflict on one of the tap's reads);
//   * a wave's 64 output pixels are still one contiguous, 64-aligned run of rows of C: the epilogue is handed img H W + (y0 + wm) 128 + xo.
//
// Summation order over K differs from the tap-major kernel (chunk-major), so last bits may differ; products and accumulation are the same.
#include "common.h"
#include "../../include/mxdenoise.h"
#include "gemm_args.h"
#include "gemm_dma_loader.h"

#include <type_traits>

namespace mx {

constexpr int HALO_BN = 160;
constexpr int HALO_WSTAGE_BYTES = HALO_BN * DMA_BK * 2;        // one stage of the weight ring
constexpr int HALO_ZERO_BYTES = 256;                           // two zero lines: one per bank half
__host__ __device__ constexpr int halo_lines(int W) { return (256 / W + 2) * W; }
__host__ __device__ constexpr int halo_xbuf_bytes(int W) { return halo_lines(W) * DMA_BK * 2; }
constexpr int HALO_SIDE_BYTES = 1024;                          // HALF: the neighbour column of one staged buffer -- one wave-wide DMA: 6 lines + 2 of padding
__host__ __device__ constexpr int halo_lds_bytes(int W, bool half) {
  return 2 * halo_xbuf_bytes(W) + 3 * HALO_WSTAGE_BYTES + HALO_ZERO_BYTES + (half ? 2 * HALO_SIDE_BYTES : 0);
}
// pieces of the next chunk's staged tile dealt to the load phase of tap T: pieces 0..XN-1 over taps 0..7 (tap 8's wait covers the last)
__host__ __device__ constexpr int halo_pieces_in_tap(int XN, int T) {
  int n = 0;
  for (int i = 0; i < XN; ++i) n += (i * 7) / (XN - 1) == T ? 1 : 0;
  return n;
}

// W: width of a tile in pixels.  HALF: the image is 2 W wide and the tile is one half of a block of rows (the top of this file)
template <int W, bool HALF, bool VEC>
__global__ __launch_bounds__(512, 2) void conv_halo_kernel(const GemmArgs pk) {
  constexpr int BN = HALO_BN, MI = 4, NI = BN / 32;
  constexpr int IW = HALF ? 2 * W : W;         // pixels per image row
  constexpr int LINES = halo_lines(W);
  constexpr int XBUF = halo_xbuf_bytes(W);
  constexpr int XN = LINES * 8 / 512;          // activation DMA instructions per thread per chunk (5 / 6)
  constexpr int WCH = BN * 8, WI = 3;          // weight DMA instructions per thread per K tile (the last re-fetches rows 0..31: same bytes, same slots)
  constexpr int WRING = 2 * XBUF, ZERO = WRING + 3 * HALO_WSTAGE_BYTES, SIDE = ZERO + HALO_ZERO_BYTES;
  constexpr int SIDE_TAP = 3, SIDE_WAVE = 0;   // HALF: who issues the side column's DMA, and in which tap's load phase
  static_assert(W == 32 || W == 64, "a tile is whole image rows of 32 or 64 pixels");
  static_assert(!HALF || W == 64, "half rows: a 128-wide image");
  static_assert(!HALF || (256 / W + 2) * 8 <= 64, "the side column is one wave-wide DMA");
  static_assert(halo_lds_bytes(W, HALF) <= 160 * 1024, "LDS of one workgroup");
  static_assert(LINES * 8 % 512 == 0 && XBUF % 256 == 0, "whole DMA instructions; buffers keep the bank half of a line");
  __shared__ __attribute__((aligned(256))) char smem[halo_lds_bytes(W, HALF)];

  const GemmArgs& p = pk;
  int tm, tn;
  gemm_tile_of_block(blockIdx.x, p.M / 256, p.N / BN, p.xcd_map, tm, tn);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1;                    // 0..3: 64-pixel quarter of the tile; groups: wm 0-1 = A, wm 2-3 = B
  const int wn = wave & 1;
  const bool group_b = wave >= 4;
  const int cs = tid & 7;
  const int nchunks = p.Cin / DMA_BK;
  const char* zero = reinterpret_cast<const char*>(g_zero_page);

  // ---- the operand stream ----
  // activations: piece i of thread tid is 16-byte slot (i * 512 + tid) of the staged buffer: line P = slot >> 3, slot cs of the line
  const int m0 = tm * 256, n0 = tn * BN;
  const int hw = p.Hin * p.Win;                // (Win == IW; hw % 256 == 0, HALF: Hin % 4 == 0 -- a tile lies inside one image)
  const int half = HALF ? tm & 1 : 0;          // HALF: the two halves of a block of rows are neighbours in tm
  const int mrows0 = HALF ? (tm >> 1) * 512 : m0;      // first pixel of the tile's image rows
  const int img = mrows0 / hw;
  const int y0 = (mrows0 - img * hw) / IW;     // first output row of the tile
  const int xo = half * W;                     // its first column
  const char* xsrc[XN];
#pragma unroll
  for (int i = 0; i < XN; ++i) {
    const int P = (i * 512 + tid) >> 3;
    const int sr = P / W, x = P - sr * W;
    const int iy = y0 - 1 + sr;
    const bool ok = iy >= 0 && iy < p.Hin;
    const long off = (((long)img * p.Hin + iy) * IW + xo + x) * (long)p.Cin * 2;
    xsrc[i] = (ok ? reinterpret_cast<const char*>(p.a) + off : zero) + swz(P, cs) * 16;
  }
  // HALF, the side column: lane l of SIDE_WAVE fetches slot (l & 7) of side line l >> 3 = the pixel (y0 - 1 + line, xo - 1 or xo + W)
  const char* xside = zero;
  if constexpr (HALF) {
    const int sl = lane >> 3;
    const int iy = y0 - 1 + sl;
    const bool ok = sl < 256 / W + 2 && iy >= 0 && iy < p.Hin;
    const int xs = half ? xo - 1 : xo + W;
    const long off = (((long)img * p.Hin + iy) * IW + xs) * (long)p.Cin * 2;
    xside = (ok ? reinterpret_cast<const char*>(p.a) + off : zero) + (cs ^ (half ? 7 : 0)) * 16;
  }
  const char* wsrc[WI];
#pragma unroll
  for (int i = 0; i < WI; ++i) {
    int q = i * 512 + tid;
    if (q >= WCH) q -= WCH;
    const int row = q >> 3;
    wsrc[i] = reinterpret_cast<const char*>(p.w) + ((long)(n0 + row) * p.K + swz(row, cs) * 8) * 2;
  }
  const long w_tap_step = (long)p.Cin * 2, w_chunk_step = DMA_BK * 2 - 8 * (long)p.Cin * 2;

  auto issue_x = [&](int buf, int i) __attribute__((always_inline)) {      // piece i of the chunk at the cursor into staged buffer `buf`
    glds16(xsrc[i], smem + buf * XBUF + (i * 512 + wave * 64) * 16);
  };
  auto advance_x = [&](int next_chunk) __attribute__((always_inline)) {    // the cursor moves to chunk `next_chunk`; past the last: harmless bytes
#pragma unroll
    for (int i = 0; i < XN; ++i) xsrc[i] = next_chunk < nchunks ? xsrc[i] + DMA_BK * 2 : zero + lane * 16;
    if constexpr (HALF) xside = next_chunk < nchunks ? xside + DMA_BK * 2 : zero + lane * 16;
  };
  auto issue_side = [&](int buf) __attribute__((always_inline)) {          // (SIDE_WAVE only: one instruction, the whole side column of `buf`)
    glds16(xside, smem + SIDE + buf * HALO_SIDE_BYTES);
  };
  auto issue_w = [&](int stage) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int qb = (i * 512 + wave * 64 >= WCH) ? i * 512 + wave * 64 - WCH : i * 512 + wave * 64;      // wave-uniform slot base
      glds16(wsrc[i], smem + WRING + stage * HALO_WSTAGE_BYTES + qb * 16);
    }
  };
  // The weight cursor runs two K tiles ahead of the tap that is computed, so where it goes next is known per tap: branch-free.  to_next_chunk:
  // from tap 8 to tap 0 of the next chunk; past the last chunk it parks on the zero page (harmless bytes into a stage nobody reads) and stays
  auto step_w = [&](long step) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < WI; ++i) wsrc[i] += step;
  };
  auto to_next_chunk_w = [&](bool last) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < WI; ++i) wsrc[i] = last ? zero + lane * 16 : wsrc[i] + w_chunk_step;
  };

  // ---- fragment addresses (bytes inside smem) ----
  const int fr = lane & 15;
  const int fq = lane >> 4;
  unsigned wrd[2];                             // weight fragments: inside a ring stage
  unsigned xrd[3][2];                          // activation fragments per dx: line (64 wm + fr + dx), the lane's chunk under that line's key
  unsigned zrd[3][2];                          // what the edge lane reads instead: the same bank position inside the zero lines; HALF, on the neighbour's
                                               // side: the same slot of side line wm (the tap adds the buffer and dy + 1 lines)
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int wrow = wn * (BN / 2) + fr;
    wrd[ks] = (unsigned)(WRING + wrow * 128 + swz(wrow, ks * 4 + fq) * 16);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int line = wm * 64 + fr + d - 1;   // (-1 only for the lane that reads the zero line instead)
      const int key = ((fr + d - 1) >> 1) & 7;
      const int rel = line * 128 + ((ks * 4 + fq) ^ key) * 16;
      xrd[d][ks] = (unsigned)rel;
      zrd[d][ks] = (unsigned)(ZERO + (rel & 255));
      if constexpr (HALF) { if (d == (half ? 0 : 2)) zrd[d][ks] = (unsigned)(SIDE + wm * 128 + (rel & 127)); }
    }
  }
  const bool lane_left = fr == 0, lane_right = fr == 15;

  // the zero lines
  if (tid < HALO_ZERO_BYTES / 16) *reinterpret_cast<u32x4*>(smem + ZERO + tid * 16) = u32x4{0u, 0u, 0u, 0u};

  // ---- prologue: chunk 0 and the weights of K tiles 0 and 1 ----
#pragma unroll
  for (int i = 0; i < XN; ++i) issue_x(0, i);
  if constexpr (HALF) { if (wave == SIDE_WAVE) issue_side(0); }
  advance_x(1);
  issue_w(0); step_w(w_tap_step);
  issue_w(1); step_w(w_tap_step);          // (the cursor stands on tap 2 of chunk 0)
  wait_vmcnt<WI>();                            // all of this thread's DMAs but the weights of K tile 1

  f32x4 acc[NI][MI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ln_rstd[MI];
#pragma unroll
  for (int j = 0; j < MI; ++j) ln_rstd[j] = 1.0f;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the zero lines are written
  MX_BAR();                                  // every wave's part of chunk 0 and of K tile 0 has landed
  if (group_b) MX_BAR();                     // group B runs one barrier behind group A

  for (int cc = 0; cc < nchunks; ++cc) {
    const int cur = cc & 1, nxt = cur ^ 1;
    const unsigned xb = (unsigned)(cur * XBUF);
    const bool last = cc + 1 == nchunks;
    // one K tile: tap T of the chunk (weights in ring stage T % 3)
    auto phase = [&](auto tc) __attribute__((always_inline)) {
      constexpr int T = decltype(tc)::value;
      constexpr int dy = T / 3 - 1, dx = T % 3 - 1, d = dx + 1;
      constexpr int NX = halo_pieces_in_tap(XN, T);
      // HALF: the edge lane on the neighbour's side reads side line wm + dy + 1 of this buffer (wave-uniform)
      const unsigned side_off = HALF && dx != 0 && (dx < 0) == (half != 0) ? (unsigned)(cur * HALO_SIDE_BYTES + (dy + 1) * 128) : 0u;
      // ---- L: all fragments of this K tile, the DMA share of chunk cc + 1 and of K tile + 2, the cursors ----
      bf16x8 wf[2][NI], xf[2][MI];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int i = 0; i < NI; ++i) wf[ks][i] = *reinterpret_cast<const bf16x8*>(smem + wrd[ks] + (T % 3) * HALO_WSTAGE_BYTES + i * (16 * 128));
#pragma unroll
        for (int j = 0; j < MI; ++j) {
          unsigned a = xb + xrd[d][ks] + (unsigned)((dy + 1) * W * 128 + j * (16 * 128));
          if (dx == -1 && (j * 16) % W == 0) a = lane_left ? zrd[d][ks] + side_off : a;          // pixel xo - 1
          if (dx == 1 && (j * 16 + 16) % W == 0) a = lane_right ? zrd[d][ks] + side_off : a;     // pixel xo + W
          xf[ks][j] = *reinterpret_cast<const bf16x8*>(smem + a);
        }
      }
#pragma unroll
      for (int i = 0; i < XN; ++i)
        if ((i * 7) / (XN - 1) == T) issue_x(nxt, i);                // halo_pieces_in_tap: in front of the tap's weights
      constexpr bool side_tap = HALF && T == SIDE_TAP;
      if constexpr (side_tap) { if (wave == SIDE_WAVE) issue_side(nxt); }
      issue_w((T + 2) % 3);                                           // K tile + 2 into the stage of K tile - 1
      if (T == 6) to_next_chunk_w(last);                              // the cursor stood on tap 8
      else step_w(T > 6 && last ? 0 : w_tap_step);
      if (T == 8) advance_x(cc + 2);
      // own part of K tile + 1 (and every older piece); the wave that issued the side column has one more DMA behind it
      if (side_tap && wave == SIDE_WAVE) wait_vmcnt<WI + NX + 1>(); else wait_vmcnt<WI + NX>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // the fragment reads have returned: their stage / buffer may be restaged one phase from now
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
    };
    phase(std::integral_constant<int, 0>{}); phase(std::integral_constant<int, 1>{}); phase(std::integral_constant<int, 2>{});
    phase(std::integral_constant<int, 3>{}); phase(std::integral_constant<int, 4>{}); phase(std::integral_constant<int, 5>{});
    phase(std::integral_constant<int, 6>{}); phase(std::integral_constant<int, 7>{}); phase(std::integral_constant<int, 8>{});
  }
  if (!group_b) MX_BAR();                    // re-align the two groups

  const int m_wave0 = HALF ? img * hw + (y0 + wm) * IW + xo : m0 + wm * 16 * MI;      // the wave's 64 output pixels: one tile row, contiguous rows of C
  gemm_epilogue_regs<NI, MI, false, VEC, true, true, 0, true, false>(p, acc, m_wave0, n0 + wn * (BN / 2), fr, fq, ln_rstd);
  if (p.gn_part != nullptr) gemm_gn_partials<NI, MI>(p, acc, m_wave0, n0 + wn * (BN / 2), fr, fq);
  wait_vmcnt<0>();                           // the past-the-end DMAs are drained before the workgroup retires
}

// LDS bytes of the instantiation for images `width` pixels wide (half_rows: the half-row form); 0: none is built
int conv_halo_lds_bytes(int width, bool half_rows) {
  if (half_rows) return width == 128 ? halo_lds_bytes(64, true) : 0;
  return width == 32 ? halo_lds_bytes(32, false) : width == 64 ? halo_lds_bytes(64, false) : 0;
}

// a is the argument block of a descriptor mx_conv3x3_halo_serves (half_rows: mx_conv3x3_halfrow_serves) accepted (gemm_dispatch.cpp);
// vec: per-sample vectors compiled in
int launch_conv_halo(hipStream_t s, const GemmArgs& a, bool vec, bool half_rows) {
  const dim3 grid((a.M / 256) * (a.N / HALO_BN)), block(512);
  if (half_rows) {
    if (a.Win != 128) return 1;
    if (vec) hipLaunchKernelGGL((conv_halo_kernel<64, true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((conv_halo_kernel<64, true, false>), grid, block, 0, s, a);
    return 0;
  }
  if (a.Win == 32) {
    if (vec) hipLaunchKernelGGL((conv_halo_kernel<32, false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((conv_halo_kernel<32, false, false>), grid, block, 0, s, a);
    return 0;
  }
  if (a.Win == 64) {
    if (vec) hipLaunchKernelGGL((conv_halo_kernel<64, false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((conv_halo_kernel<64, false, false>), grid, block, 0, s, a);
    return 0;
  }
  return 1;
}

}  // namespace mx
