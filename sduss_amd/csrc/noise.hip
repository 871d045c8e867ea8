// Seeded noise as a tensor (gfx950): out[r][i] = scale[r] * z(seed[r], step[r], domain, i) with z the noise function of noise.h -- the initial
// latents of a seeded request, the start / kept-region noise of image-to-image and inpainting.  The step's own noise never becomes a tensor: the
// NOISY step (scheduler_step.hip) calls the same function in registers.  raw: the generator's uint32 words instead, for the tests of its integer half.
// A pure store pass: 16-byte stores where the layout allows, element stores otherwise.
#include "common.h"
#include "../../include/mxdenoise.h"

#pragma clang fp contract(off)
#include "step_math.h"
#include "noise.h"

namespace mx {

// One thread per V elements.  On the vector path `elems` is a whole number of vectors, so a vector lies inside one row and starts on a group.
template <typename T, int V, bool RAW>
__global__ void noise_fill_kernel(T* __restrict__ out, int n, long elems, const unsigned long long* __restrict__ seed, const unsigned* __restrict__ step,
                                  unsigned domain, const float* __restrict__ scale) {
  const long e0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (e0 >= (long)n * elems) return;
  const int row = (int)(e0 / elems);
  const long within = e0 - (long)row * elems;
  elem_vec<T, V> o;
  if constexpr (RAW) {
#pragma unroll
    for (int k = 0; k < (V + 3) / 4; ++k) {
      unsigned w[4];
      philox4x32_10(seed[row], ((unsigned long long)within >> 2) + k, step[row], domain, w);
      if constexpr (V == 1) {
        const int lane = (int)(within & 3);
        o.v[0] = lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : w[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) o.v[4 * k + i] = w[i];
      }
    }
  } else {
    float z[V];
    noise_elems<V>(seed[row], step[row], domain, within, z);
    const float sc = scale ? scale[row] : 1.0f;
#pragma unroll
    for (int i = 0; i < V; ++i) store_from_f32<T>(o.v, i, sc * z[i]);
  }
  *reinterpret_cast<elem_vec<T, V>*>(out + e0) = o;
}

template <typename T, bool RAW>
static int launch_noise_fill(hipStream_t s, void* out, int n, long elems, const uint64_t* seed, const uint32_t* step, int domain, const float* scale) {
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec = elems % V == 0 && aligned_to(out, 16);
  const long total = (long)n * elems;
  const int64_t blocks = cdiv64(vec ? total / V : total, 256);
  MX_CHECK(blocks <= 0x7fffffffL, "noise_fill: too many elements for one launch");
  const dim3 grid((unsigned)blocks), block(256);
  const unsigned long long* sd = (const unsigned long long*)seed;
  if (vec) hipLaunchKernelGGL((noise_fill_kernel<T, V, RAW>), grid, block, 0, s, (T*)out, n, elems, sd, step, (unsigned)domain, scale);
  else hipLaunchKernelGGL((noise_fill_kernel<T, 1, RAW>), grid, block, 0, s, (T*)out, n, elems, sd, step, (unsigned)domain, scale);
  MX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mx

extern "C" int mx_noise_fill(void* stream, void* out, int dtype, int n, int64_t elems, const uint64_t* seed, const uint32_t* step, int domain,
                             const float* scale, int raw) {
  MX_CHECK(out && seed && step, "noise_fill: null operand");
  MX_CHECK(n > 0 && elems > 0, "noise_fill: sizes must be positive");
  MX_CHECK(domain >= 0, "noise_fill: domain must not be negative");
  MX_CHECK(raw == 0 || raw == 1, "noise_fill: raw must be 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  if (raw) return mx::launch_noise_fill<unsigned, true>(s, out, n, (long)elems, seed, step, domain, nullptr);
  return mx::with_io_dtype(dtype, "noise_fill", [&](auto tag) {
    typedef decltype(tag) T;
    return mx::launch_noise_fill<T, false>(s, out, n, (long)elems, seed, step, domain, scale);
  });
}
