// What the small-channel 3x3 convolutions share (conv_small_n.hip: the UNet's conv_out and conv_in; conv_rgb8.hip: the VAE decoder's conv_out to 8-bit
// RGB; conv_rgb_in.hip: the VAE encoder's conv_in from the client's image).  One geometry: a workgroup of 256 threads owns a tile of four image rows x 16
// columns, a wave 16 consecutive pixels of one row; the workgroup is persistent and walks tile += gridDim.x.  Here: the tile arithmetic, the sliced
// path's halo-corner rule, the launch rule of the kernels whose LDS depends on the shape, and the whole staged body of the two Cin -> few-channels kernels
// (conv3x3_small_n_kernel and conv3x3_rgb8_kernel), which differ in the weight rows they read, in the corner rule and in their epilogue.
#pragma once
#include <algorithm>

#include "common.h"

namespace mx {

__host__ __device__ inline int conv_tiles_x(int W) { return (W + 15) >> 4; }
__host__ __device__ inline int conv_tiles_y(int H) { return (H + 3) >> 2; }
__host__ __device__ inline int conv_tiles(int B, int H, int W) { return B * conv_tiles_x(W) * conv_tiles_y(H); }

// tile index -> image b, tile row ty, tile column tx (tx fastest)
struct ConvTile { int b, ty, tx; };
__device__ __forceinline__ ConvTile conv_tile_at(int tile, int H, int W) {
  const int tiles_x = conv_tiles_x(W), per_image = tiles_x * conv_tiles_y(H);
  const int b = tile / per_image;
  const int t = tile - b * per_image;
  const int ty = t / tiles_x;
  return ConvTile{b, ty, t - ty * tiles_x};
}

// The halo-corner rule of the reference's sliced path (norm_silu_concat.cu:210-221, 228-239): with P x P patches, a diagonal tap (dy, dx) of pixel
// (y, x) that leaves the pixel's patch through a corner reads the horizontal neighbour (y, x + dx) instead.  P > 0: the caller asks only where the rule is
// on (`P > 0 && corner_folds(...)`, then an assignment -- the shape in which both kernels keep their instruction stream).
__device__ __forceinline__ bool corner_folds(int y, int x, int dy, int dx, int P) {
  if (dy == 0 || dx == 0) return false;
  const bool cross_r = ((y + dy + P) / P) != ((y + P) / P);
  const bool cross_c = ((x + dx + P) / P) != ((x + P) / P);
  return cross_r && cross_c;
}

// workgroups a launch starts: no more than the tiles, and no more than the chip holds at once (LDS; at most max_per_cu per CU)
inline int small_conv_grid(int tiles, size_t lds_bytes, int max_per_cu) {
  const int per_cu = std::max(1, std::min(max_per_cu, (int)((160 * 1024) / (lds_bytes + 256))));
  return std::min(tiles, per_cu * cu_count());
}

// ---- the staged small-N body: Cin -> a handful of output channels.  As an implicit GEMM it is M = B H W rows, K = 9 Cin, N = rows <= 16: the work is
// reading the input once.  A wave owns all the outputs of its 16 pixels: one v_mfma_f32_16x16x32_bf16 per (tap, 32 input channels) with A = the weights
// (rows >= `rows` zero, held in LDS: rows x K bf16) and B = the 16 pixels' channels.  Per 64-channel chunk the tile's halo'd 6 x 18 pixels are staged in
// LDS as whole 128-byte lines (the next chunk's reads in flight while this one multiplies), and the nine taps are nine shifted reads of that stage. ----
constexpr int kSnPix = 6 * 18;                 // a tile's pixels with their halo: (4 + 2) rows x (16 + 2) columns
constexpr int kSnStride = 144;                 // bytes per staged pixel: 64 channels + 16 of padding (16 pixels x 4 pieces read conflict-free)

__host__ __device__ inline size_t small_n_weight_bytes(int rows, long K) { return ((size_t)rows * K * 2 + 255) & ~(size_t)255; }
// dynamic LDS of a launch: the weight rows, then one staged chunk
inline size_t small_n_lds_bytes(int rows, long K) { return small_n_weight_bytes(rows, K) + (size_t)kSnPix * kSnStride; }

struct SmallNView {
  const bf16_t* x;        // NHWC bf16 [B, H, W, Cin], Cin % 64 == 0
  const bf16_t* w;        // [>= rows, 9 Cin] bf16, tap-major; only the first `rows` rows are read
  int B, H, W, Cin;
  int K;                  // a weight row's elements: 9 Cin
  int rows;               // weight rows read (<= 16)
  int corner_patch;       // the corner rule's patch size; 0 = none
};

// epilogue(acc, b, y, x, tx, j, kq): lane (j, kq) of the wave of image row y holds the accumulators of outputs n = 4 kq + {0..3} of pixel (y, x = 16 tx + j)
// of image b.  Called by every lane for every tile (y >= H and x >= W included: the caller masks).  The MFMA order -- sub, then tap 0..8, one accumulator
// -- is fixed here, so two kernels built on this body hold the same bits for the same operands.
template <class Epilogue>
__device__ __forceinline__ void conv3x3_small_n_body(const SmallNView v, Epilogue&& epilogue) {
  extern __shared__ __attribute__((aligned(16))) char smem[];        // weights [rows][K] bf16, then one staged 64-channel chunk of the tile
  bf16_t* sw = reinterpret_cast<bf16_t*>(smem);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int H = v.H, W = v.W, Cin = v.Cin, K = v.K;
  char* sx = smem + small_n_weight_bytes(v.rows, K);
  {
    const int chunks = v.rows * K / 8;                 // 16-byte pieces (K % 8 == 0)
    for (int c = tid; c < chunks; c += 256) *reinterpret_cast<u32x4*>(sw + (long)c * 8) = *reinterpret_cast<const u32x4*>(v.w + (long)c * 8);
  }
  const int tiles = conv_tiles(v.B, H, W);
  const int nch = Cin >> 6;                            // 64-channel chunks
  const bool wrow = j < v.rows;                         // lane (j, kq) holds weight row n = j as the A operand
  const bf16_t* swl = sw + (long)(wrow ? j : 0) * K + kq * 8;
  const bf16x8 zero8 = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  // this thread's pieces of a staged chunk: piece i = pixel i / 8 of the halo'd tile, 16-byte piece i % 8 of its 128 bytes
  int ppy[4], ppx[4], pc16[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = tid + 256 * q;
    const int pix = i >> 3;
    pc16[q] = i & 7;
    ppy[q] = pix / 18; ppx[q] = pix - ppy[q] * 18;
  }
  // the whole halo'd tile of one chunk comes in as full 128-byte lines (the direct form asked L1 for 16 half-lines per load and ran at one load per
  // ~64 cycles per CU whatever the occupancy: 87 us); zero padding is zeros in LDS
  auto fetch = [&](u32x4 (&r)[4], int tile, int ch) __attribute__((always_inline)) {
    const ConvTile t = conv_tile_at(tile, H, W);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gy = t.ty * 4 - 1 + ppy[q], gx = t.tx * 16 - 1 + ppx[q];
      const bool ok = (tid + 256 * q) < kSnPix * 8 && gy >= 0 && gy < H && gx >= 0 && gx < W;
      r[q] = ok ? *reinterpret_cast<const u32x4*>(v.x + ((long)(t.b * H + gy) * W + gx) * Cin + ch * 64 + pc16[q] * 8) : zero4;
    }
  };
  auto stage = [&](const u32x4 (&r)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if ((tid + 256 * q) < kSnPix * 8) *reinterpret_cast<u32x4*>(sx + ((tid + 256 * q) >> 3) * kSnStride + pc16[q] * 16) = r[q];
  };
  int tile = blockIdx.x;
  if (tile >= tiles) return;                           // (the launcher starts no more workgroups than tiles)
  u32x4 pre[4];
  fetch(pre, tile, 0);
  __syncthreads();                                      // the weights are in place
  while (tile < tiles) {
    const ConvTile t = conv_tile_at(tile, H, W);
    const int y = t.ty * 4 + wave, x = t.tx * 16 + j;
    // per tap: the staged pixel this lane reads (row wave + 1 + dy, column j + 1 + dx of the halo'd tile; a tap the corner rule folds reads row wave + 1).
    // Without the rule (corner_patch a literal 0) nothing here depends on the tile and the offsets are computed once, before the loop.
    int sp[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3 - 1, dx = tap % 3 - 1;
      int ry = wave + 1 + dy;
      if (v.corner_patch > 0 && corner_folds(y, x, dy, dx, v.corner_patch)) ry = wave + 1;
      sp[tap] = (ry * 18 + j + 1 + dx) * kSnStride + kq * 16;
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int next_tile = tile + gridDim.x;
    for (int ch = 0; ch < nch; ++ch) {
      stage(pre);
      __syncthreads();
      if (ch + 1 < nch) fetch(pre, tile, ch + 1);       // in flight while this chunk multiplies
      else if (next_tile < tiles) fetch(pre, next_tile, 0);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        bf16x8 xf[9], wf[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          xf[tap] = *reinterpret_cast<const bf16x8*>(sx + sp[tap] + sub * 64);
          wf[tap] = wrow ? *reinterpret_cast<const bf16x8*>(swl + tap * Cin + ch * 64 + sub * 32) : zero8;
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tap], xf[tap], acc, 0, 0, 0);
      }
      __syncthreads();                                  // every wave has read the chunk: the stage may be rewritten
    }
    epilogue(acc, t.b, y, x, t.tx, j, kq);
    tile = next_tile;
  }
}

}  // namespace mx
