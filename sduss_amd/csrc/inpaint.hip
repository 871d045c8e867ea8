// Inpainting (gfx950): repaint the masked part of an image and keep the rest -- diffusers' 4-channel rule of StableDiffusionXLInpaintPipeline and
// StableDiffusion3InpaintPipeline, which works with the base checkpoints of both models.  After every scheduler step the kept region of the latents
// is put back as the image's own latents re-noised to the step's next sigma:
//     init_proper = add_noise / scale_noise(image_latents, noise, t_next);   latents = (1 - mask) * init_proper + mask * latents
// That is part of the step launch that reads and writes the latents anyway (scheduler_step.hip, the MASKED form of cfg_step_kernel), over a batch in
// which inpainting and plain requests step together.  Here the three small kernels a request needs once: its starting latents
// (inpaint_renoise_kernel), its mask on the latent grid (mask_to_latent_kernel) and the client's own pixels back outside the mask of the decoded image
// (rgb8_paste_kernel).  HBM-bound passes: 16-byte accesses where the layout allows, element accesses otherwise.
#include <algorithm>

#include "common.h"
#include "../../include/mxdenoise.h"

// op-by-op IEEE evaluation as in elementwise.hip: no mul+add contraction in this translation unit (and -ffp-contract=off for this file in the Makefile)
#pragma clang fp contract(off)
#include "step_math.h"

namespace mx {

// out[r] = keep[r] * init[r] + sigma[r] * noise[r] over n rows of `elems`; one thread per V elements (elems % V == 0 on the vector path)
template <typename T, int V>
__global__ void inpaint_renoise_kernel(const T* __restrict__ init, const T* __restrict__ noise, T* __restrict__ out, const float* __restrict__ keep,
                                       const float* __restrict__ sigma, long elems, long n_vec) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_vec) return;
  const long e0 = idx * V;
  const int row = (int)(e0 / elems);
  typedef elem_vec<T, V> vec;
  const vec a = *reinterpret_cast<const vec*>(init + e0);
  const vec n = *reinterpret_cast<const vec*>(noise + e0);
  const float kp = keep[row], sg = sigma[row];
  vec o;
#pragma unroll
  for (int i = 0; i < V; ++i) store_from_f32<T>(o.v, i, renoise(load_as_f32<T>(a.v, i), load_as_f32<T>(n.v, i), kp, sg));
  *reinterpret_cast<vec*>(out + e0) = o;
}

// out[b, y, x] = mask[b, f y, f x] >= 128: binarise at half of 255, then the nearest resize to the latent grid (for an integer factor: source pixel (f y, f x))
__global__ void mask_to_latent_kernel(const unsigned char* __restrict__ mask, unsigned char* __restrict__ out, int H, int W, int f, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over B * (H / f) * (W / f), x fastest
  if (idx >= total) return;
  const int w = W / f, h = H / f;
  const int x = (int)(idx % w);
  const long r = idx / w;
  const int y = (int)(r % h);
  const long b = r / h;
  out[idx] = mask[(b * H + (long)y * f) * W + (long)x * f] >= 128 ? 1 : 0;
}

// decoded [P][3] in place: pixel p becomes original[p] where mask[p] < 128.  One thread per four pixels = three dwords of each image and one of the mask
// (VEC: all three bases 4-byte aligned); the pixels past the last whole four, and every pixel of a misaligned image, go byte by byte.
template <bool VEC>
__global__ void rgb8_paste_kernel(unsigned char* __restrict__ dec, const unsigned char* __restrict__ orig, const unsigned char* __restrict__ mask, long P) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long p0 = idx * 4;
  if (p0 >= P) return;
  if (VEC && p0 + 4 <= P) {
    const unsigned m = *reinterpret_cast<const unsigned*>(mask + p0);
    if ((m & 0x80808080u) == 0x80808080u) return;       // all four repainted: nothing to put back
    unsigned* d = reinterpret_cast<unsigned*>(dec + p0 * 3);
    const unsigned* o = reinterpret_cast<const unsigned*>(orig + p0 * 3);
    unsigned sel[3] = {0u, 0u, 0u};                      // 0xff in every byte that takes the original's
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (((m >> (8 * q)) & 0x80u) == 0u) {
#pragma unroll
        for (int c = 0; c < 3; ++c) sel[(3 * q + c) >> 2] |= 0xffu << (8 * ((3 * q + c) & 3));
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (sel[i]) d[i] = (d[i] & ~sel[i]) | (o[i] & sel[i]);
  } else {
    const long p1 = std::min(p0 + 4, P);
    for (long p = p0; p < p1; ++p)
      if (mask[p] < 128) {
        dec[3 * p] = orig[3 * p]; dec[3 * p + 1] = orig[3 * p + 1]; dec[3 * p + 2] = orig[3 * p + 2];
      }
  }
}

template <typename T>
static int launch_inpaint_renoise(hipStream_t s, const void* init, const void* noise, void* out, const float* keep, const float* sigma, int n, long elems) {
  constexpr int V = 16 / (int)sizeof(T);
  const long total = (long)n * elems;
  const bool vec = elems % V == 0 && aligned_to(init, 16) && aligned_to(noise, 16) && aligned_to(out, 16);
  const long n_vec = vec ? total / V : total;
  const int64_t blocks = cdiv64(n_vec, 256);
  MX_CHECK(blocks <= 0x7fffffffL, "inpaint_renoise: too many elements for one launch");
  dim3 grid((unsigned)blocks), block(256);
  if (vec) hipLaunchKernelGGL((inpaint_renoise_kernel<T, V>), grid, block, 0, s, (const T*)init, (const T*)noise, (T*)out, keep, sigma, elems, n_vec);
  else hipLaunchKernelGGL((inpaint_renoise_kernel<T, 1>), grid, block, 0, s, (const T*)init, (const T*)noise, (T*)out, keep, sigma, elems, n_vec);
  MX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mx

extern "C" int mx_inpaint_renoise(void* stream, const void* init, const void* noise, void* out, const float* keep, const float* sigma, int n, int64_t elems,
                                  int dtype) {
  MX_CHECK(init && noise && out && keep && sigma, "inpaint_renoise: null operand");
  MX_CHECK(n > 0 && elems > 0, "inpaint_renoise: sizes must be positive");
  MX_CHECK(out != init && out != noise, "inpaint_renoise: out may alias neither input");
  return mx::with_io_dtype(dtype, "inpaint_renoise", [&](auto tag) {
    return mx::launch_inpaint_renoise<decltype(tag)>((hipStream_t)stream, init, noise, out, keep, sigma, n, (long)elems);
  });
}

extern "C" int mx_mask_to_latent(void* stream, const uint8_t* mask, uint8_t* out, int B, int H, int W, int f) {
  MX_CHECK(mask && out, "mask_to_latent: null operand");
  MX_CHECK(B > 0 && H > 0 && W > 0 && f > 0, "mask_to_latent: sizes must be positive");
  MX_CHECK(H % f == 0 && W % f == 0, "mask_to_latent: H and W must be multiples of the factor");
  const long total = (long)B * (H / f) * (W / f);
  const int64_t blocks = mx::cdiv64(total, 256);
  MX_CHECK(blocks <= 0x7fffffffL, "mask_to_latent: too many elements for one launch");
  hipLaunchKernelGGL(mx::mask_to_latent_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mask, out, H, W, f, total);
  MX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mx_rgb8_paste(void* stream, uint8_t* decoded, const uint8_t* original, const uint8_t* mask, int B, int H, int W) {
  MX_CHECK(decoded && original && mask, "rgb8_paste: null operand");
  MX_CHECK(B > 0 && H > 0 && W > 0, "rgb8_paste: sizes must be positive");
  MX_CHECK(decoded != original, "rgb8_paste: the decoded image may not alias the original");
  const long P = (long)B * H * W;
  const int64_t blocks = mx::cdiv64(mx::cdiv64(P, 4), 256);
  MX_CHECK(blocks <= 0x7fffffffL, "rgb8_paste: too many pixels for one launch");
  const bool vec = mx::aligned_to(decoded, 4) && mx::aligned_to(original, 4) && mx::aligned_to(mask, 4);
  dim3 grid((unsigned)blocks), block(256);
  if (vec) hipLaunchKernelGGL((mx::rgb8_paste_kernel<true>), grid, block, 0, (hipStream_t)stream, decoded, original, mask, P);
  else hipLaunchKernelGGL((mx::rgb8_paste_kernel<false>), grid, block, 0, (hipStream_t)stream, decoded, original, mask, P);
  MX_LAUNCH_CHECK();
  return 0;
}
