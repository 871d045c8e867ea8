// The first launch of a request that starts from an image: the VAE encoder's conv_in (3x3, pad 1, stride 1, 3 image channels -> N features) reading the
// client's image itself -- 8-bit interleaved RGB, or the fp32 planes image_processor.preprocess yields -- instead of an NHWC bf16 tensor zero-padded to
// 64 channels.  The mirror image of conv_rgb8.hip: that one ends a request in the client's bytes, this one starts a request from them.
// As an implicit GEMM it is K = 27: ONE v_mfma_f32_16x16x32_bf16 k-step per 16 features (A = the weights [N, 32], columns 27..31 forced to zero;
// B = the 16 pixels a wave owns).  A workgroup is a tile of four rows x 16 columns; its halo'd 6 x 18 pixels are staged densely in LDS as
// [row][x][3] bf16 (the next tile's reads in flight while this one multiplies), so for a fixed ky the nine (kx, c) values of a pixel are nine consecutive
// elements and a lane's eight columns are eight 2-byte reads.  The weight fragments and the bias of up to 128 features stay in registers for the whole
// launch (blockIdx.y walks 128-feature chunks of a wider N).  The work is the output write: the 16 x 128 results of a wave go through a wave-private LDS
// patch and leave as whole 16-byte pieces of each pixel's contiguous bytes (16 pixels x 256 bytes = 4 KB contiguous per wave at N = 128).
// rotate = 1: output pixel (y, x) is the conv centred on pixel (y, x) of the image rotated by 180 degrees, i.e. on image pixel (H-1-y, W-1-x): the
// whole encoder runs in that orientation (vae_sdxl.cpp, EncodePlan).
#include <algorithm>

#include "common.h"
#include "../../include/mxdenoise.h"
#include "conv_tile.h"

// bytes -> value is evaluated operation by operation (t = u / 255; v = 2 t - 1): no contraction into an FMA in this translation unit
#pragma clang fp contract(off)

namespace mx {

constexpr int kRiRowElems = 18 * 3;            // a staged row: (16 + 2) pixels x 3 channels, dense
constexpr int kRiElems = 6 * kRiRowElems;      // (4 + 2) rows: 324 values, 648 bytes
constexpr int kRiStageBytes = 768;             // the stage, rounded up to 256
constexpr int kRiBlocks = 8;                   // 16-feature blocks a workgroup computes: 128 features
constexpr int kRiPatch = 16 * kRiBlocks * 2 + 16;   // bytes per pixel of a wave's output patch: 128 features + 16 of padding
constexpr int kRiLds = kRiStageBytes + 4 * 16 * kRiPatch;
constexpr int kRiPerCu = 4;                    // workgroups a launch starts per CU at most

struct RgbInArgs {
  const void* image;      // MX_IMAGE_RGB8_HWC: uint8 [B, H, W, 3];  MX_IMAGE_F32_CHW: fp32 [B, 3, H, W]
  const bf16_t* w;        // [N, 32], column (ky 3 + kx) 3 + c; columns 27..31 read as zero
  const float* bias;      // fp32 [N]
  bf16_t* y;              // NHWC bf16 [B, H, W, N]
  int B, H, W, N;
  int format, rotate;
};

__device__ __forceinline__ bf16_t rgb_in_value(const RgbInArgs& p, int b, int sy, int sx, int c) {
  if (p.format == MX_IMAGE_RGB8_HWC) {
    const unsigned u = reinterpret_cast<const unsigned char*>(p.image)[((long)(b * p.H + sy) * p.W + sx) * 3 + c];
    const float t = (float)u / 255.0f;
    return f32_to_bf16(2.0f * t - 1.0f);
  }
  return f32_to_bf16(reinterpret_cast<const float*>(p.image)[((long)(b * 3 + c) * p.H + sy) * p.W + sx]);
}

__global__ __launch_bounds__(256, 4) void conv3x3_rgb_in_kernel(const RgbInArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];        // the staged tile, then 4 waves x 16 pixels x kRiPatch bytes of output staging
  bf16_t* sx = reinterpret_cast<bf16_t*>(smem);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int H = p.H, W = p.W, N = p.N;
  char* patch = smem + kRiStageBytes + wave * (16 * kRiPatch);
  const int n0 = blockIdx.y * (16 * kRiBlocks);
  const int nb = std::min(kRiBlocks, (N - n0) >> 4);                  // 16-feature blocks of this chunk (N % 16 == 0: the launcher)
  const int tiles = conv_tiles(p.B, H, W);
  // A operand: lane (j, kq) holds weight row n0 + 16 i + j, columns 8 kq .. 8 kq + 7; columns >= 27 are zero whatever the tensor holds
  bf16x8 wf[kRiBlocks];
  f32x4 bv[kRiBlocks];
#pragma unroll
  for (int i = 0; i < kRiBlocks; ++i) {
    u32x4 r = {0u, 0u, 0u, 0u};
    bv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < nb) {
      r = *reinterpret_cast<const u32x4*>(p.w + (long)(n0 + 16 * i + j) * 32 + kq * 8);
      if (kq == 3) { r[1] &= 0x0000ffffu; r[2] = 0u; r[3] = 0u; }     // columns 24, 25, 26 stay
      bv[i] = *reinterpret_cast<const f32x4*>(p.bias + n0 + 16 * i + 4 * kq);
    }
    wf[i] = __builtin_bit_cast(bf16x8, r);
  }
  // B operand: element e of lane (j, kq) is column k = 8 kq + e = 9 ky + m of pixel j: staged value (wave + ky, 3 j + m)
  int xo[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = 8 * kq + e;
    const int ky = k / 9, m = k - ky * 9;
    xo[e] = k < 27 ? (wave + ky) * kRiRowElems + 3 * j + m : -1;
  }
  // this thread's values of a staged tile: value v = (row v / 54, pixel (v % 54) / 3, channel v % 3) of the halo'd tile
  int vr[2], vx[2], vc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int v = tid + 256 * q;
    vr[q] = v / kRiRowElems;
    const int rem = v - vr[q] * kRiRowElems;
    vx[q] = rem / 3; vc[q] = rem - vx[q] * 3;
  }
  auto fetch = [&](bf16_t (&r)[2], int tile) __attribute__((always_inline)) {
    const ConvTile t = conv_tile_at(tile, H, W);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int gy = t.ty * 4 - 1 + vr[q], gx = t.tx * 16 - 1 + vx[q];
      const bool ok = (tid + 256 * q) < kRiElems && gy >= 0 && gy < H && gx >= 0 && gx < W;      // zero padding is zeros in LDS
      r[q] = ok ? rgb_in_value(p, t.b, p.rotate ? H - 1 - gy : gy, p.rotate ? W - 1 - gx : gx, vc[q]) : (bf16_t)0;
    }
  };
  int tile = blockIdx.x;
  if (tile >= tiles) return;                           // (the launcher starts no more workgroups than tiles)
  bf16_t pre[2];
  fetch(pre, tile);
  while (tile < tiles) {
    const ConvTile t = conv_tile_at(tile, H, W);
    const int b = t.b, tx = t.tx;
    const int y = t.ty * 4 + wave;
    const int next_tile = tile + gridDim.x;
    sx[tid] = pre[0];
    if (tid + 256 < kRiElems) sx[tid + 256] = pre[1];
    __syncthreads();
    if (next_tile < tiles) fetch(pre, next_tile);       // in flight while this tile multiplies and leaves
    if (y < H) {                                        // (wave-uniform)
      bf16_t xe[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) xe[e] = xo[e] >= 0 ? sx[xo[e]] : (bf16_t)0;
      const u32x4 xr = {(unsigned)xe[0] | ((unsigned)xe[1] << 16), (unsigned)xe[2] | ((unsigned)xe[3] << 16), (unsigned)xe[4] | ((unsigned)xe[5] << 16),
                        (unsigned)xe[6] | ((unsigned)xe[7] << 16)};
      const bf16x8 xf = __builtin_bit_cast(bf16x8, xr);
      // lane (j, kq) holds features n0 + 16 i + 4 kq + {0..3} of pixel tx 16 + j: through the wave's patch, out as whole 16-byte pieces
#pragma unroll
      for (int i = 0; i < kRiBlocks; ++i) {
        if (i < nb) {
          f32x4 v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          v += bv[i];
          *reinterpret_cast<u32x2*>(patch + j * kRiPatch + (16 * i + 4 * kq) * 2) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (one wave: its LDS operations complete in order)
      const int per_px = 2 * nb;                          // 16-byte pieces of a pixel in this chunk
      const int pieces = 16 * per_px;
      bf16_t* row = p.y + ((long)(b * H + y) * W + tx * 16) * N + n0;
      for (int piece = lane; piece < pieces; piece += 64) {
        const int pj = piece / per_px, c16 = piece - pj * per_px;
        const u32x4 o = *reinterpret_cast<const u32x4*>(patch + pj * kRiPatch + c16 * 16);
        if (tx * 16 + pj < W) *reinterpret_cast<u32x4*>(row + (long)pj * N + c16 * 8) = o;
      }
    }
    __syncthreads();                                    // every wave has read the stage (and its patch): both may be rewritten
    tile = next_tile;
  }
}

}  // namespace mx

extern "C" int mx_conv3x3_rgb_in(void* stream, const void* image, int image_format, const void* w, const float* bias, void* y, int B, int H, int W, int N,
                                 int rotate) {
  MX_CHECK(image && w && bias && y, "conv3x3_rgb_in: null operand");
  MX_CHECK(B > 0 && H > 0 && W > 0 && N > 0, "conv3x3_rgb_in: sizes must be positive");
  MX_CHECK(image_format == MX_IMAGE_RGB8_HWC || image_format == MX_IMAGE_F32_CHW, "conv3x3_rgb_in: image_format must be MX_IMAGE_RGB8_HWC or MX_IMAGE_F32_CHW");
  MX_CHECK(rotate == 0 || rotate == 1, "conv3x3_rgb_in: rotate must be 0 or 1");
  MX_CHECK(N % 16 == 0, "conv3x3_rgb_in: N must be a multiple of 16");
  MX_CHECK(((uintptr_t)w & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)y & 15) == 0, "conv3x3_rgb_in: w, bias and y must be 16-byte aligned");
  MX_CHECK(image_format != MX_IMAGE_F32_CHW || ((uintptr_t)image & 3) == 0, "conv3x3_rgb_in: an fp32 image must be 4-byte aligned");
  MX_CHECK((long)B * H * W * 3 < 2147483647L, "conv3x3_rgb_in: the image exceeds 32-bit source offsets");
  mx::RgbInArgs a;
  a.image = image; a.w = (const mx::bf16_t*)w; a.bias = bias; a.y = (mx::bf16_t*)y;
  a.B = B; a.H = H; a.W = W; a.N = N; a.format = image_format; a.rotate = rotate;
  const int tiles = mx::conv_tiles(B, H, W);      // (< 2^31: B H W is)
  const int chunks = (N + 16 * mx::kRiBlocks - 1) / (16 * mx::kRiBlocks);
  MX_CHECK(chunks <= 65535, "conv3x3_rgb_in: N too large");
  const int grid = std::min(tiles, mx::kRiPerCu * mx::cu_count());
  hipLaunchKernelGGL(mx::conv3x3_rgb_in_kernel, dim3(grid, chunks), dim3(256), mx::kRiLds, (hipStream_t)stream, a);
  MX_LAUNCH_CHECK();
  return 0;
}
