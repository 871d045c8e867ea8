// The per-element arithmetic of the scheduler step (scheduler_step.hip) and of the kernels beside it that round like it (elementwise.hip's input
// scaling and vae_latent_finish_kernel, inpaint.hip's start re-noising): the io-dtype loads and stores, the CFG combine, the two Euler updates, the
// re-noising of clean latents and the linear multistep update.  Every function is a chain of separately rounded IEEE fp32 operations that torch evaluates identically op by op, so an including file
// must not contract mul + add into FMA: it is built with -ffp-contract=off (Makefile) and the pragma below covers everything that follows the
// include.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace mx {

template <typename T> __device__ __forceinline__ float load_as_f32(const T* p, long i);
template <> __device__ __forceinline__ float load_as_f32<float>(const float* p, long i) { return p[i]; }
template <> __device__ __forceinline__ float load_as_f32<bf16_t>(const bf16_t* p, long i) { return bf16_to_f32(p[i]); }
template <> __device__ __forceinline__ float load_as_f32<_Float16>(const _Float16* p, long i) { return (float)p[i]; }
template <typename T> __device__ __forceinline__ void store_from_f32(T* p, long i, float v);
template <> __device__ __forceinline__ void store_from_f32<float>(float* p, long i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void store_from_f32<bf16_t>(bf16_t* p, long i, float v) { p[i] = f32_to_bf16(v); }
template <> __device__ __forceinline__ void store_from_f32<_Float16>(_Float16* p, long i, float v) { p[i] = (_Float16)v; }

// value after a round trip through T (emulates an op whose result tensor has dtype T)
template <typename T> __device__ __forceinline__ float rnd(float v) {
  T tmp;
  store_from_f32<T>(&tmp, 0, v);
  return load_as_f32<T>(&tmp, 0);
}

// V elements of T moved as one access (16 bytes on the vector path, one element on the other)
template <typename T, int V> struct alignas(sizeof(T) * V) elem_vec { T v[V]; };

// The per-element arithmetic of the CFG steps: every form of cfg_step_kernel (scheduler_step.hip) runs these operations in this order, so the same bits.
// the combine runs in the model dtype (pipeline_..._esymred.py:383-385; pipeline_stable_diffusion_3_esymred.py:365-367): one rounding per op
template <typename T> __device__ __forceinline__ float cfg_combine(float u, float t, float g) { return rnd<T>(u + rnd<T>(g * rnd<T>(t - u))); }
// the guided prediction of V elements: u alone without guidance (the conditional half, `cond` elements on, is then not read)
template <typename T, int V> __device__ __forceinline__ void guided_prediction(const T* up, long cond, float g, float (&p)[V]) {
  typedef elem_vec<T, V> vec;
  const vec u = *reinterpret_cast<const vec*>(up);
  if (g > 0.f) {
    const vec t = *reinterpret_cast<const vec*>(up + cond);
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = cfg_combine<T>(load_as_f32<T>(u.v, i), load_as_f32<T>(t.v, i), g);
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = load_as_f32<T>(u.v, i);
  }
}
// epsilon Euler step (scheduling_euler_discrete.py:210-268): separate IEEE ops (no fma contraction) so the fp32 chain matches torch's op-by-op evaluation
__device__ __forceinline__ float euler_update(float x, float eps, float s, float sn) {
  const float pred_x0 = (x - (s * eps));
  const float d = ((x - pred_x0) / s);
  const float step = d * (sn - s);
  return x + step;
}
// flow-match Euler step: x + (sigma_next - sigma) * v
__device__ __forceinline__ float flow_update(float x, float v, float s, float sn) {
  const float step = (sn - s) * v;
  return x + step;
}
// clean latents noised to a sigma: keep * init + sigma * noise, two products and one sum (EulerDiscreteScheduler.add_noise: keep = 1; the flow-match
// scale_noise: keep = 1 - sigma).  The start noise of an image-to-image request (vae_latent_finish_kernel) and the kept region of an inpainting one.
__device__ __forceinline__ float renoise(float init, float noise, float keep, float sigma) {
  const float a = keep * init;
  const float n = sigma * noise;
  return a + n;
}

// The multistep rows (scheduler_step.hip, MULTI): x_next = cx x + c0 D + c1 D_prev, every product and sum rounded on its own.
// D of DPM-Solver++ 2M, the data prediction of the epsilon model: x - sigma * eps
__device__ __forceinline__ float multistep_data(float x, float eps, float s) {
  const float n = s * eps;
  return x - n;
}
// a first-order row: the history is not an operand (on a request's first step it is uninitialised memory)
__device__ __forceinline__ float multistep_update1(float x, float d, float cx, float c0) {
  const float a = cx * x;
  const float b = c0 * d;
  return a + b;
}
__device__ __forceinline__ float multistep_update2(float x, float d, float prev, float cx, float c0, float c1) {
  const float acc = multistep_update1(x, d, cx, c0);
  const float c = c1 * prev;
  return acc + c;
}
// the noise term of a stochastic row (scheduler_step.hip, NOISY): acc + (cn * z) behind the multistep update, z ~ N(0, 1) (noise.h)
__device__ __forceinline__ float noisy_update(float acc, float cn, float z) {
  const float n = cn * z;
  return acc + n;
}

}  // namespace mx
