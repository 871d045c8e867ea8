// The last launch of a request: the VAE decoder's conv_out (3x3, pad 1, stride 1, Cin -> 3 channels) with the image processor's postprocess in its
// epilogue -- (y / 2 + 0.5).clamp(0, 1), x 255, round half to even, 8-bit interleaved RGB (image_processor.postprocess(output_type="pil") of the
// reference's post_inference, pipeline_stable_diffusion_xl_esymred.py:455) -- so the image is rounded ONCE, from the fp32 accumulator, and leaves the
// device as H x W x 3 bytes instead of 3 x H x W floats.
// The body is conv3x3_small_n_kernel's (conv_small_n.hip), restated here so that kernel's code object stays what it was: a wave owns 16 consecutive pixels
// of an image row, a workgroup a tile of four rows x 16 columns; per 64-channel chunk the tile's halo'd 6 x 18 pixels are staged in LDS as whole 128-byte
// lines (the next chunk's reads in flight while this one multiplies); one v_mfma_f32_16x16x32_bf16 per (tap, 32 channels) in the same order, so the
// accumulator holds the same bits as conv_small_n's for the same operands.  Only weight rows 0..2 are read; no corner-patch rule.
// Epilogue: lanes 0..15 of a wave hold one pixel's three bytes each = 48 contiguous bytes of the image row.  Where every row starts 4-byte aligned
// (W % 4 == 0 and an aligned base: every real decode, W = 8 x the latent width) they are exchanged between lanes (two ds_bpermute) and leave as 12 dwords;
// otherwise as single bytes.
#include <algorithm>

#include "common.h"
#include "../../include/mxdenoise.h"

namespace mx {

constexpr int kRgbPix = 6 * 18;                // a tile's pixels with their halo: (4 + 2) rows x (16 + 2) columns
constexpr int kRgbStride = 144;                // bytes per staged pixel: 64 channels + 16 of padding (16 pixels x 4 pieces read conflict-free)
constexpr int kRgbRows = 3;                    // weight rows read: R, G, B (row 3 of the packed [4, 9 Cin] is padding)

struct Rgb8Args {
  const bf16_t* x;        // NHWC bf16 [B, H, W, Cin]
  const bf16_t* w;        // packed [4, 9 Cin], tap-major
  const float* bias;      // fp32 [4]
  unsigned char* out;     // [B, H, W, 3]
  int B, H, W, Cin;
  int vec;                // rows start 4-byte aligned: dword stores
};

static size_t rgb8_lds_bytes(int Cin) { return (((size_t)kRgbRows * 9 * Cin * 2 + 255) & ~(size_t)255) + (size_t)kRgbPix * kRgbStride; }

// y -> the 8-bit level, each step in fp32: t = y / 2 + 0.5, clamped to [0, 1] with NaN -> 0, rint(255 t) (round half to even, as numpy's round)
__device__ __forceinline__ unsigned rgb8_level(float y) {
  float t = y * 0.5f + 0.5f;
  t = t > 0.f ? t : 0.f;                       // (a NaN compares false)
  t = t < 1.f ? t : 1.f;
  return (unsigned)rintf(t * 255.0f);
}

__global__ __launch_bounds__(256) void conv3x3_rgb8_kernel(const Rgb8Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];        // weight rows 0..2 [3][K] bf16, then one staged 64-channel chunk of the tile
  bf16_t* sw = reinterpret_cast<bf16_t*>(smem);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int H = p.H, W = p.W, Cin = p.Cin, K = 9 * p.Cin;
  char* sx = smem + (((size_t)kRgbRows * K * 2 + 255) & ~(size_t)255);
  {
    const int chunks = kRgbRows * K / 8;               // 16-byte pieces (K % 8 == 0)
    for (int c = tid; c < chunks; c += 256) *reinterpret_cast<u32x4*>(sw + (long)c * 8) = *reinterpret_cast<const u32x4*>(p.w + (long)c * 8);
  }
  const int tiles_x = (W + 15) >> 4, tiles_y = (H + 3) >> 2;
  const int tiles = p.B * tiles_x * tiles_y;
  const int nch = Cin >> 6;                            // 64-channel chunks (Cin % 64 == 0: the launcher)
  const bool wrow = j < kRgbRows;                       // lane (j, kq) holds weight row n = j as the A operand
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
  auto fetch = [&](u32x4 (&r)[4], int tile, int ch) __attribute__((always_inline)) {
    const int b = tile / (tiles_x * tiles_y);
    const int t = tile - b * tiles_x * tiles_y;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gy = ty * 4 - 1 + ppy[q], gx = tx * 16 - 1 + ppx[q];
      const bool ok = (tid + 256 * q) < kRgbPix * 8 && gy >= 0 && gy < H && gx >= 0 && gx < W;      // zero padding is zeros in LDS
      r[q] = ok ? *reinterpret_cast<const u32x4*>(p.x + ((long)(b * H + gy) * W + gx) * Cin + ch * 64 + pc16[q] * 8) : zero4;
    }
  };
  auto stage = [&](const u32x4 (&r)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if ((tid + 256 * q) < kRgbPix * 8) *reinterpret_cast<u32x4*>(sx + ((tid + 256 * q) >> 3) * kRgbStride + pc16[q] * 16) = r[q];
  };
  int sp[9];                                            // per tap: the staged pixel this lane reads (row wave + 1 + dy, column j + 1 + dx of the halo'd tile)
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) sp[tap] = ((wave + tap / 3) * 18 + j + tap % 3) * kRgbStride + kq * 16;
  // the dword this lane sends in the vector epilogue: bytes 4 lane .. 4 lane + 3 of the wave's 48 = the tail of pixel e0 and the head of pixel e0 + 1
  const int e0 = (4 * lane) / 3, esh = 8 * ((4 * lane) % 3);
  int tile = blockIdx.x;
  if (tile >= tiles) return;                           // (the launcher starts no more workgroups than tiles)
  u32x4 pre[4];
  fetch(pre, tile, 0);
  __syncthreads();                                      // the weights are in place
  while (tile < tiles) {
    const int b = tile / (tiles_x * tiles_y);
    const int t = tile - b * tiles_x * tiles_y;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y = ty * 4 + wave, x = tx * 16 + j;
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
    // lane (j, kq) holds outputs n = 4 kq + {0..3} of pixel x: the lanes kq == 0 hold R, G, B (and the unused row 3)
    if (y < H) {                                        // (wave-uniform: the exchange below runs with the whole wave)
      const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bias);
      const unsigned px = rgb8_level(acc[0] + bv[0]) | (rgb8_level(acc[1] + bv[1]) << 8) | (rgb8_level(acc[2] + bv[2]) << 16);
      unsigned char* row = p.out + ((long)(b * H + y) * W + tx * 16) * 3;
      if (p.vec) {
        const unsigned lo = (unsigned)__shfl((int)px, e0, 64), hi = (unsigned)__shfl((int)px, e0 + 1, 64);
        const int dwords = 3 * std::min(16, W - tx * 16) / 4;          // (W % 4 == 0: whole dwords)
        if (lane < dwords) *reinterpret_cast<unsigned*>(row + 4 * lane) = (lo >> esh) | (hi << (24 - esh));
      } else if (kq == 0 && x < W) {
        row[3 * j] = (unsigned char)(px & 0xff);
        row[3 * j + 1] = (unsigned char)((px >> 8) & 0xff);
        row[3 * j + 2] = (unsigned char)(px >> 16);
      }
    }
    tile = next_tile;
  }
}

// workgroups a launch starts: as launch_conv_small_n -- no more than the tiles, and no more than the chip holds at once (LDS; at most 6 per CU)
static int rgb8_grid(int tiles, size_t lds) {
  const int per_cu = std::max(1, std::min(6, (int)((160 * 1024) / (lds + 256))));
  return std::min(tiles, per_cu * cu_count());
}

}  // namespace mx

extern "C" int mx_conv3x3_rgb8(void* stream, const void* x, const void* w, const float* bias, void* out, int B, int H, int W, int Cin) {
  MX_CHECK(x && w && bias && out, "conv3x3_rgb8: null operand");
  MX_CHECK(B > 0 && H > 0 && W > 0 && Cin > 0, "conv3x3_rgb8: sizes must be positive");
  MX_CHECK(Cin % 64 == 0, "conv3x3_rgb8: Cin must be a multiple of 64");
  MX_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)bias & 15) == 0, "conv3x3_rgb8: x, w and bias must be 16-byte aligned");
  MX_CHECK((long)B * H * W * Cin < 2147483647L, "conv3x3_rgb8: the input exceeds 32-bit source offsets");
  const size_t lds = mx::rgb8_lds_bytes(Cin);
  MX_CHECK(lds <= 64 * 1024, "conv3x3_rgb8: the weights and one staged chunk exceed 64 KB of LDS (Cin too large)");
  mx::Rgb8Args a;
  a.x = (const mx::bf16_t*)x; a.w = (const mx::bf16_t*)w; a.bias = bias; a.out = (unsigned char*)out;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin;
  a.vec = (W % 4 == 0 && ((uintptr_t)out & 3) == 0) ? 1 : 0;
  const long tiles = (long)B * ((H + 3) / 4) * ((W + 15) / 16);      // (< 2^31: B H W is)
  hipLaunchKernelGGL(mx::conv3x3_rgb8_kernel, dim3(mx::rgb8_grid((int)tiles, lds)), dim3(256), lds, (hipStream_t)stream, a);
  MX_LAUNCH_CHECK();
  return 0;
}
