// The last launch of a request: the VAE decoder's conv_out (3x3, pad 1, stride 1, Cin -> 3 channels) with the image processor's postprocess in its
// epilogue -- (y / 2 + 0.5).clamp(0, 1), x 255, round half to even, 8-bit interleaved RGB (image_processor.postprocess(output_type="pil") of the
// reference's post_inference, pipeline_stable_diffusion_xl_esymred.py:455) -- so the image is rounded ONCE, from the fp32 accumulator, and leaves the
// device as H x W x 3 bytes instead of 3 x H x W floats.
// The body is the staged small-N body of conv_tile.h, the one conv3x3_small_n_kernel (conv_small_n.hip) runs: same staging, same prefetch, the same
// v_mfma_f32_16x16x32_bf16 order, so the accumulator holds the same bits as conv_small_n's for the same operands.  Only weight rows 0..2 are read; no
// corner-patch rule (a literal 0: the tap offsets are computed once, before the tile loop).
// Epilogue: lanes 0..15 of a wave hold one pixel's three bytes each = 48 contiguous bytes of the image row.  Where every row starts 4-byte aligned
// (W % 4 == 0 and an aligned base: every real decode, W = 8 x the latent width) they are exchanged between lanes (two ds_bpermute) and leave as 12 dwords;
// otherwise as single bytes.
#include <algorithm>

#include "common.h"
#include "../../include/mxdenoise.h"
#include "conv_tile.h"

namespace mx {

constexpr int kRgbRows = 3;                    // weight rows read: R, G, B (row 3 of the packed [4, 9 Cin] is padding)

struct Rgb8Args {
  const bf16_t* x;        // NHWC bf16 [B, H, W, Cin]
  const bf16_t* w;        // packed [4, 9 Cin], tap-major
  const float* bias;      // fp32 [4]
  unsigned char* out;     // [B, H, W, 3]
  int B, H, W, Cin;
  int vec;                // rows start 4-byte aligned: dword stores
};

// y -> the 8-bit level, each step in fp32: t = y / 2 + 0.5, clamped to [0, 1] with NaN -> 0, rint(255 t) (round half to even, as numpy's round)
__device__ __forceinline__ unsigned rgb8_level(float y) {
  float t = y * 0.5f + 0.5f;
  t = t > 0.f ? t : 0.f;                       // (a NaN compares false)
  t = t < 1.f ? t : 1.f;
  return (unsigned)rintf(t * 255.0f);
}

__global__ __launch_bounds__(256) void conv3x3_rgb8_kernel(const Rgb8Args p) {
  const SmallNView v = {p.x, p.w, p.B, p.H, p.W, p.Cin, 9 * p.Cin, kRgbRows, 0};
  const int lane = threadIdx.x & 63;
  // the dword this lane sends in the vector epilogue: bytes 4 lane .. 4 lane + 3 of the wave's 48 = the tail of pixel e0 and the head of pixel e0 + 1
  const int e0 = (4 * lane) / 3, esh = 8 * ((4 * lane) % 3);
  // lane (j, kq) holds outputs n = 4 kq + {0..3} of pixel x: the lanes kq == 0 hold R, G, B (and the unused row 3)
  conv3x3_small_n_body(v, [&](const f32x4& acc, int b, int y, int x, int tx, int j, int kq) __attribute__((always_inline)) {
    if (y < p.H) {                                      // (wave-uniform: the exchange below runs with the whole wave)
      const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bias);
      const unsigned px = rgb8_level(acc[0] + bv[0]) | (rgb8_level(acc[1] + bv[1]) << 8) | (rgb8_level(acc[2] + bv[2]) << 16);
      unsigned char* row = p.out + ((long)(b * p.H + y) * p.W + tx * 16) * 3;
      if (p.vec) {
        const unsigned lo = (unsigned)__shfl((int)px, e0, 64), hi = (unsigned)__shfl((int)px, e0 + 1, 64);
        const int dwords = 3 * std::min(16, p.W - tx * 16) / 4;        // (W % 4 == 0: whole dwords)
        if (lane < dwords) *reinterpret_cast<unsigned*>(row + 4 * lane) = (lo >> esh) | (hi << (24 - esh));
      } else if (kq == 0 && x < p.W) {
        row[3 * j] = (unsigned char)(px & 0xff);
        row[3 * j + 1] = (unsigned char)((px >> 8) & 0xff);
        row[3 * j + 2] = (unsigned char)(px >> 16);
      }
    }
  });
}

}  // namespace mx

extern "C" int mx_conv3x3_rgb8(void* stream, const void* x, const void* w, const float* bias, void* out, int B, int H, int W, int Cin) {
  MX_CHECK(x && w && bias && out, "conv3x3_rgb8: null operand");
  MX_CHECK(B > 0 && H > 0 && W > 0 && Cin > 0, "conv3x3_rgb8: sizes must be positive");
  MX_CHECK(Cin % 64 == 0, "conv3x3_rgb8: Cin must be a multiple of 64");
  MX_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)bias & 15) == 0, "conv3x3_rgb8: x, w and bias must be 16-byte aligned");
  MX_CHECK((long)B * H * W * Cin < 2147483647L, "conv3x3_rgb8: the input exceeds 32-bit source offsets");
  const size_t lds = mx::small_n_lds_bytes(mx::kRgbRows, 9L * Cin);
  MX_CHECK(lds <= 64 * 1024, "conv3x3_rgb8: the weights and one staged chunk exceed 64 KB of LDS (Cin too large)");
  mx::Rgb8Args a;
  a.x = (const mx::bf16_t*)x; a.w = (const mx::bf16_t*)w; a.bias = bias; a.out = (unsigned char*)out;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin;
  a.vec = (W % 4 == 0 && ((uintptr_t)out & 3) == 0) ? 1 : 0;
  const int grid = mx::small_conv_grid(mx::conv_tiles(B, H, W), lds, 6);      // (the tiles stay below 2^31: B H W does)
  hipLaunchKernelGGL(mx::conv3x3_rgb8_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
  MX_LAUNCH_CHECK();
  return 0;
}
