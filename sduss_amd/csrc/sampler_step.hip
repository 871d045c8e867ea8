// Second-order multistep samplers (gfx950): ONE scheduler launch over a batch whose requests step by different samplers -- the model's own Euler
// step, DPM-Solver++ 2M (k-diffusion's sample_dpmpp_2m, the variance-exploding form of diffusers' DPMSolverMultistepScheduler) and the second-order
// Adams-Bashforth step -- with the kept region of inpainting rows put back as cfg_step_masked_kernel (inpaint.hip) does it.  Both multistep samplers
// are linear in the latent, this step's D and the previous step's D; the host makes the three coefficients (sampler_coeffs.cpp), the kernel keeps D
// of every row in an fp32 history buffer.  An HBM-bound pass: 16-byte accesses where the layout allows, element accesses otherwise.
#include "common.h"
#include "../../include/mxdenoise.h"

// op-by-op IEEE evaluation as in elementwise.hip: no mul+add contraction in this translation unit (and -ffp-contract=off for this file in the Makefile)
#pragma clang fp contract(off)
#include "step_math.h"

namespace mx {

// One thread per V elements of the latents [n_lat][C][hw] (in place); pred [2 n_lat | n_lat][C][hw]; hist fp32 [n_lat][C][hw].  Row r steps by
// kind[r]: 1 and 2 are the multistep rows (x_next = cx x + c0 D + c1 hist, hist <- D), everything else is the model's Euler step and leaves hist
// alone.  On the vector path hw is a whole number of vectors and every base is aligned, so a vector lies inside one (row, channel) plane; the V
// fp32 history values of a 16-bit vector are V / 4 accesses of 16 bytes.
template <typename T, int V, bool FLOW>
__global__ void cfg_multistep_kernel(const T* __restrict__ pred, T* __restrict__ lat, const float* __restrict__ sigma, const float* __restrict__ sigma_next,
                                     float g, int n_lat, long elems, int hw, long n_vec, const int* __restrict__ kind, const float* __restrict__ coef,
                                     float* __restrict__ hist, int k, const int* __restrict__ slot, const T* __restrict__ init,
                                     const T* __restrict__ noise, const unsigned char* __restrict__ mask) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_vec) return;
  const long e0 = idx * V;
  const int row = (int)(e0 / elems);
  typedef elem_vec<T, V> vec;
  constexpr int HV = V < 4 ? V : 4;                      // fp32 history values per access: 16 bytes on the vector path
  typedef elem_vec<float, HV> hvec;
  const vec u = *reinterpret_cast<const vec*>(pred + e0);
  vec t = u;
  if (g > 0.f) t = *reinterpret_cast<const vec*>(pred + (long)n_lat * elems + e0);
  vec x = *reinterpret_cast<const vec*>(lat + e0);
  const float s = sigma[row], sn = sigma_next[row];
  const int kd = kind[row];
  if (kd == MX_SAMPLER_DPMPP_2M || kd == MX_SAMPLER_AB2) {
    const float cx = coef[3 * (long)row], c0 = coef[3 * (long)row + 1], c1 = coef[3 * (long)row + 2];
    float d[V], h[V] = {};
    if (c1 != 0.0f) {                                    // first-order rows never read the history: it may be uninitialised
#pragma unroll
      for (int q = 0; q < V / HV; ++q) {
        const hvec hv = *reinterpret_cast<const hvec*>(hist + e0 + q * HV);
#pragma unroll
        for (int i = 0; i < HV; ++i) h[q * HV + i] = hv.v[i];
      }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float ui = load_as_f32<T>(u.v, i);
      const float m = (g > 0.f) ? cfg_combine<T>(ui, load_as_f32<T>(t.v, i), g) : ui;
      const float xi = load_as_f32<T>(x.v, i);
      d[i] = kd == MX_SAMPLER_DPMPP_2M ? multistep_data(xi, m, s) : m;
      store_from_f32<T>(x.v, i, c1 != 0.0f ? multistep_update2(xi, d[i], h[i], cx, c0, c1) : multistep_update1(xi, d[i], cx, c0));
    }
#pragma unroll
    for (int q = 0; q < V / HV; ++q) {
      hvec hv;
#pragma unroll
      for (int i = 0; i < HV; ++i) hv.v[i] = d[q * HV + i];
      *reinterpret_cast<hvec*>(hist + e0 + q * HV) = hv;
    }
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float ui = load_as_f32<T>(u.v, i);
      const float p = (g > 0.f) ? cfg_combine<T>(ui, load_as_f32<T>(t.v, i), g) : ui;
      const float xi = load_as_f32<T>(x.v, i);
      store_from_f32<T>(x.v, i, FLOW ? flow_update(xi, p, s, sn) : euler_update(xi, p, s, sn));
    }
  }
  const int j = k > 0 ? slot[row] : -1;
  if (j >= 0 && j < k) {                       // (anything else is a plain row: a wrong slot never becomes an address)
    const long within = e0 - (long)row * elems;
    const int p0 = (int)(within % hw);
    const elem_vec<unsigned char, V> m = *reinterpret_cast<const elem_vec<unsigned char, V>*>(mask + (long)j * hw + p0);
    bool any_kept = false;
#pragma unroll
    for (int i = 0; i < V; ++i) any_kept |= m.v[i] == 0;
    if (any_kept) {
      const vec a = *reinterpret_cast<const vec*>(init + (long)j * elems + within);
      const vec n = *reinterpret_cast<const vec*>(noise + (long)j * elems + within);
      const float keep = FLOW ? 1.0f - sn : 1.0f;
#pragma unroll
      for (int i = 0; i < V; ++i)
        if (m.v[i] == 0) store_from_f32<T>(x.v, i, renoise(load_as_f32<T>(a.v, i), load_as_f32<T>(n.v, i), keep, sn));
    }
  }
  *reinterpret_cast<vec*>(lat + e0) = x;
}

static bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

template <typename T, bool FLOW>
static int launch_cfg_multistep(hipStream_t s, const void* pred, void* latents, const float* sigma, const float* sigma_next, float g, int n_lat, int C, int hw,
                                const mx_multistep_rows* ms, const mx_inpaint_rows& r) {
  constexpr int V = 16 / (int)sizeof(T);
  const long elems = (long)C * hw, total = (long)n_lat * elems;
  // the vector path: every plane of hw elements starts on a 16-byte boundary in every tensor, and on a V-byte boundary in the mask
  const bool vec = hw % V == 0 && aligned_to(pred, 16) && aligned_to(latents, 16) && aligned_to(ms->hist, 16) &&
                   (r.k == 0 || (aligned_to(r.init, 16) && aligned_to(r.noise, 16) && aligned_to(r.mask, V)));
  const long n_vec = vec ? total / V : total;
  const int64_t blocks = cdiv64(n_vec, 256);
  MX_CHECK(blocks <= 0x7fffffffL, "cfg_multistep_step: too many elements for one launch");
  dim3 grid((unsigned)blocks), block(256);
  if (vec) hipLaunchKernelGGL((cfg_multistep_kernel<T, V, FLOW>), grid, block, 0, s, (const T*)pred, (T*)latents, sigma, sigma_next, g, n_lat, elems, hw, n_vec,
                              ms->kind, ms->coef, ms->hist, r.k, r.slot, (const T*)r.init, (const T*)r.noise, r.mask);
  else hipLaunchKernelGGL((cfg_multistep_kernel<T, 1, FLOW>), grid, block, 0, s, (const T*)pred, (T*)latents, sigma, sigma_next, g, n_lat, elems, hw, n_vec,
                          ms->kind, ms->coef, ms->hist, r.k, r.slot, (const T*)r.init, (const T*)r.noise, r.mask);
  MX_LAUNCH_CHECK();
  return 0;
}

template <bool FLOW>
static int cfg_multistep(hipStream_t s, const void* pred, void* latents, const float* sigma, const float* sigma_next, float g, int n_lat, int C, int hw, int dtype,
                         const mx_multistep_rows* ms, const mx_inpaint_rows& r) {
  if (dtype == MX_F32) return launch_cfg_multistep<float, FLOW>(s, pred, latents, sigma, sigma_next, g, n_lat, C, hw, ms, r);
  if (dtype == MX_F16) return launch_cfg_multistep<_Float16, FLOW>(s, pred, latents, sigma, sigma_next, g, n_lat, C, hw, ms, r);
  if (dtype == MX_BF16) return launch_cfg_multistep<bf16_t, FLOW>(s, pred, latents, sigma, sigma_next, g, n_lat, C, hw, ms, r);
  MX_CHECK(false, "cfg_multistep_step: bad dtype");
  return 1;
}

}  // namespace mx

extern "C" int mx_cfg_multistep_step(void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                                     int n_lat, int C, int hw, int dtype, int flow, const mx_multistep_rows* ms, const mx_inpaint_rows* inpaint) {
  MX_CHECK(noise_pred && latents && sigma && sigma_next && ms, "cfg_multistep_step: null operand");
  MX_CHECK(ms->kind && ms->coef && ms->hist, "cfg_multistep_step: null kind, coef or hist");
  MX_CHECK(n_lat > 0 && C > 0 && hw > 0, "cfg_multistep_step: sizes must be positive");
  MX_CHECK(dtype == MX_F32 || dtype == MX_F16 || dtype == MX_BF16, "cfg_multistep_step: bad dtype");
  {                                                      // the history is written while both are read: no byte of it may lie inside either
    const size_t esz = dtype == MX_F32 ? 4 : 2, total = (size_t)n_lat * C * hw;
    const uintptr_t h0 = (uintptr_t)ms->hist, h1 = h0 + total * 4, l0 = (uintptr_t)latents, p0 = (uintptr_t)noise_pred;
    const bool apart = (h1 <= l0 || l0 + total * esz <= h0) && (h1 <= p0 || p0 + (guidance_scale > 0.f ? 2 : 1) * total * esz <= h0);
    MX_CHECK(apart, "cfg_multistep_step: hist may alias neither the latents nor the prediction");
  }
  mx_inpaint_rows none = {0, nullptr, nullptr, nullptr, nullptr};
  const mx_inpaint_rows& r = inpaint ? *inpaint : none;
  MX_CHECK(r.k >= 0, "cfg_multistep_step: k must not be negative");
  MX_CHECK(r.k == 0 || (r.slot && r.init && r.noise && r.mask), "cfg_multistep_step: inpainting rows need slot, init, noise and mask");
  hipStream_t s = (hipStream_t)stream;
  return flow ? mx::cfg_multistep<true>(s, noise_pred, latents, sigma, sigma_next, guidance_scale, n_lat, C, hw, dtype, ms, r)
              : mx::cfg_multistep<false>(s, noise_pred, latents, sigma, sigma_next, guidance_scale, n_lat, C, hw, dtype, ms, r);
}
