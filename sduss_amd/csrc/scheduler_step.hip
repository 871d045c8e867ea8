// The scheduler step (gfx950): every kernel that steps latents, as ONE template.  Per element all forms do the same thing -- load the prediction(s) and
// the latent, CFG combine, update, store -- and differ in three compile-time features:
//   GATHERED  the prediction is read where the world gather of the split-batch patch parallelism left it (patch_parallel.py)
//   MULTI     per-row sampler kind, coefficients and an fp32 history: DPM-Solver++ 2M and AB2 beside the model's own Euler step (sampler_coeffs.cpp)
//   MASKED    the kept region of inpainting rows put back as the image's own latents re-noised to the step's next sigma (inpaint.hip)
//   NOISY     per-row noise cn z behind the multistep update, z made in registers by the request's own generator (noise.h): Euler ancestral and
//             DPM-Solver++ 2M SDE rows (sampler_coeffs.cpp)
// A form without a feature holds none of its code and reads none of its operands.  Instantiated: plain, GATHERED, MASKED, MULTI + MASKED,
// MULTI + MASKED + NOISY; each for both models' steps (FLOW) and three io dtypes.  HBM-bound passes: 16-byte accesses where the layout allows, element
// accesses otherwise.
// The plain form is always launched element-wise: its latency sits at the launch floor either way (profiles/sampler_step.txt) and it ends every step.
#include "common.h"
#include "../../include/mxdenoise.h"

// The step reproduces torch's op-by-op IEEE evaluation bit for bit: no mul+add contraction into FMA in this translation unit (HIP's __fmul_rn/__fadd_rn
// are plain operators in inlined headers and do get contracted; so plain operators, plus -ffp-contract=off for this file in the Makefile).
#pragma clang fp contract(off)
#include "step_math.h"
#include "noise.h"

namespace mx {

// The operands of one step launch, by value.  latents [n_lat][elems] of the io dtype, in place; pred [2 n_lat | n_lat][elems] (g <= 0 reads the first
// half only); sigma, sigma_next fp32 [n_lat].  Members of a feature the launched form lacks stay zero and are not read.
struct step_args {
  const void* pred; void* lat; const float* sigma; const float* sigma_next; float g; int n_lat; long elems;
  long run;                                              // elements contiguous in every tensor: hw of a (row, channel) plane; GATHERED: (H / S) W; plain: unused
  int C, S;                                              // GATHERED: pred [2 S][n_lat][C][run], slot k < S the unconditional, S + k the conditional prediction of rows [k H / S, (k + 1) H / S)
  const int* kind; const float* coef; float* hist;       // MULTI: mx_multistep_rows
  int k; const int* slot; const void* init; const void* noise; const unsigned char* mask;   // MASKED: mx_inpaint_rows
  const float* cn; const unsigned long long* seed; const unsigned* nstep;                   // NOISY: mx_noise_rows
};

// A multistep row: x_next = cx x + c0 D + c1 hist, hist <- D, with D = x - sigma m (DPM-Solver++ 2M) or D = m (AB2).  The V fp32 history values of a
// 16-bit vector are V / 4 accesses of 16 bytes.  cn != 0 (NOISY rows only): + cn z behind the update.
template <typename T, int V>
__device__ __forceinline__ void multistep_elems(elem_vec<T, V>& x, const float (&m)[V], float s, int kd, const float* coef, float* hist, float cn,
                                                const float (&z)[V]) {
  constexpr int HV = V < 4 ? V : 4;                      // fp32 history values per access: 16 bytes on the vector path
  typedef elem_vec<float, HV> hvec;
  const float cx = coef[0], c0 = coef[1], c1 = coef[2];
  float d[V], h[V] = {};
  if (c1 != 0.0f) {                                      // first-order rows never read the history: it may be uninitialised
#pragma unroll
    for (int q = 0; q < V / HV; ++q) {
      const hvec hv = *reinterpret_cast<const hvec*>(hist + q * HV);
#pragma unroll
      for (int i = 0; i < HV; ++i) h[q * HV + i] = hv.v[i];
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const float xi = load_as_f32<T>(x.v, i);
    d[i] = kd == MX_SAMPLER_DPMPP_2M ? multistep_data(xi, m[i], s) : m[i];
    const float acc = c1 != 0.0f ? multistep_update2(xi, d[i], h[i], cx, c0, c1) : multistep_update1(xi, d[i], cx, c0);
    store_from_f32<T>(x.v, i, cn != 0.0f ? noisy_update(acc, cn, z[i]) : acc);
  }
#pragma unroll
  for (int q = 0; q < V / HV; ++q) {
    hvec hv;
#pragma unroll
    for (int i = 0; i < HV; ++i) hv.v[i] = d[q * HV + i];
    *reinterpret_cast<hvec*>(hist + q * HV) = hv;
  }
}

// Put back kept: row with j = slot[row] in [0, k) is an inpainting row; where mask[j][p] == 0 the element becomes renoise(init[j], noise[j], keep, sn)
// instead of the stepped value.  `within`: the vector's first element inside its row.  On the vector path its V mask bytes are one aligned load.
template <typename T, int V, bool FLOW>
__device__ __forceinline__ void put_back_kept(elem_vec<T, V>& x, const step_args& a, int row, long within, float sn) {
  const int j = a.k > 0 ? a.slot[row] : -1;
  if (j >= 0 && j < a.k) {                               // (anything else is a plain row: a wrong slot never becomes an address)
    typedef elem_vec<T, V> vec;
    const int p0 = (int)(within % a.run);
    const elem_vec<unsigned char, V> m = *reinterpret_cast<const elem_vec<unsigned char, V>*>(a.mask + (long)j * a.run + p0);
    bool any_kept = false;
#pragma unroll
    for (int i = 0; i < V; ++i) any_kept |= m.v[i] == 0;
    if (any_kept) {
      const vec c = *reinterpret_cast<const vec*>((const T*)a.init + (long)j * a.elems + within);
      const vec n = *reinterpret_cast<const vec*>((const T*)a.noise + (long)j * a.elems + within);
      const float keep = FLOW ? 1.0f - sn : 1.0f;
#pragma unroll
      for (int i = 0; i < V; ++i)
        if (m.v[i] == 0) store_from_f32<T>(x.v, i, renoise(load_as_f32<T>(c.v, i), load_as_f32<T>(n.v, i), keep, sn));
    }
  }
}

// One thread per V elements of the latents.  On the vector path `run` is a whole number of vectors and every base is aligned, so a vector lies inside
// one run of every tensor.
template <typename T, int V, bool FLOW, bool GATHERED, bool MULTI, bool MASKED, bool NOISY>
__global__ void cfg_step_kernel(const step_args a) {
  const long e0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V;
  const long total = (long)a.n_lat * a.elems;
  if (e0 >= total) return;
  const int row = (int)(e0 / a.elems);
  typedef elem_vec<T, V> vec;
  const T* up = (const T*)a.pred + e0;
  if constexpr (GATHERED) {                              // e0 in the latents' order is ((plane * S + slab) * run + e), plane = latent * C + channel
    const long q = e0 / a.run, plane = q / a.S;
    up = (const T*)a.pred + ((q - plane * a.S) * ((long)a.n_lat * a.C) + plane) * a.run + (e0 - q * a.run);
  }
  float p[V];                                            // the guided prediction
  guided_prediction<T, V>(up, total, a.g, p);
  T* xp = (T*)a.lat + e0;
  vec x = *reinterpret_cast<const vec*>(xp);
  const float s = a.sigma[row], sn = a.sigma_next[row];
  int kd = MX_SAMPLER_EULER;
  if constexpr (MULTI) kd = a.kind[row];
  if (MULTI && (kd == MX_SAMPLER_DPMPP_2M || kd == MX_SAMPLER_AB2)) {
    float cn = 0.0f, z[V] = {};
    if constexpr (NOISY) {                               // a row without noise reads neither its seed nor its step and runs no generator
      cn = a.cn[row];
      if (cn != 0.0f) noise_elems<V>(a.seed[row], a.nstep[row], MX_NOISE_STEP, e0 - (long)row * a.elems, z);
    }
    multistep_elems<T, V>(x, p, s, kd, a.coef + 3 * (long)row, a.hist + e0, cn, z);
  } else {                                               // the model's own step; every unknown kind too.  hist is left alone
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float xi = load_as_f32<T>(x.v, i);
      store_from_f32<T>(x.v, i, FLOW ? flow_update(xi, p[i], s, sn) : euler_update(xi, p[i], s, sn));
    }
  }
  if constexpr (MASKED) put_back_kept<T, V, FLOW>(x, a, row, e0 - (long)row * a.elems, sn);
  *reinterpret_cast<vec*>(xp) = x;
}

// The one launcher: the 16-byte path when every base and run allows it (the null pointers of absent features count as aligned), one thread per element
// otherwise -- and for the plain form always.
template <bool GATHERED, bool MULTI, bool MASKED, bool NOISY = false>
static int launch_cfg_step(const char* what, void* stream, int dtype, bool flow, const step_args& a) {
  return with_io_dtype(dtype, what, [&](auto tag) {
    typedef decltype(tag) T;
    constexpr int V = GATHERED || MULTI || MASKED ? 16 / (int)sizeof(T) : 1;
    const bool vec = a.run % V == 0 && aligned_to(a.pred, 16) && aligned_to(a.lat, 16) && aligned_to(a.hist, 16) && aligned_to(a.init, 16) &&
                     aligned_to(a.noise, 16) && aligned_to(a.mask, V);
    const long total = (long)a.n_lat * a.elems;
    const int64_t blocks = cdiv64(vec ? total / V : total, 256);
    MX_CHECK(blocks <= 0x7fffffffL, std::string(what) + ": too many elements for one launch");
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (vec && flow) hipLaunchKernelGGL((cfg_step_kernel<T, V, true, GATHERED, MULTI, MASKED, NOISY>), grid, block, 0, s, a);
    else if (vec) hipLaunchKernelGGL((cfg_step_kernel<T, V, false, GATHERED, MULTI, MASKED, NOISY>), grid, block, 0, s, a);
    else if (flow) hipLaunchKernelGGL((cfg_step_kernel<T, 1, true, GATHERED, MULTI, MASKED, NOISY>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((cfg_step_kernel<T, 1, false, GATHERED, MULTI, MASKED, NOISY>), grid, block, 0, s, a);
    MX_LAUNCH_CHECK();
    return 0;
  });
}

static step_args base_args(const void* pred, void* latents, const float* sigma, const float* sigma_next, float g, int n_lat, long elems) {
  step_args a = {};
  a.pred = pred; a.lat = latents; a.sigma = sigma; a.sigma_next = sigma_next; a.g = g; a.n_lat = n_lat; a.elems = elems;
  return a;
}

static int cfg_step_plain(const char* what, bool flow, void* stream, const void* noise, void* latents, const float* sigma, const float* sigma_next, float g,
                          int n_lat, int64_t elems, int dtype) {
  MX_CHECK(noise && latents && sigma && sigma_next && n_lat > 0 && elems > 0, std::string(what) + ": bad arguments");
  return launch_cfg_step<false, false, false>(what, stream, dtype, flow, base_args(noise, latents, sigma, sigma_next, g, n_lat, (long)elems));
}

static int cfg_step_rows(bool flow, void* stream, const void* gathered, void* latents, const float* sigma, const float* sigma_next, float g, int n_lat, int C,
                         int H, int W, int n_slabs, int dtype) {
  MX_CHECK(gathered && latents && sigma && sigma_next && n_lat > 0 && C > 0 && H > 0 && W > 0, "cfg_step_rows: bad arguments");
  MX_CHECK(n_slabs > 0 && H % n_slabs == 0, "cfg_step_rows: the latent height must be a positive multiple of n_slabs");
  step_args a = base_args(gathered, latents, sigma, sigma_next, g, n_lat, (long)C * H * W);
  a.run = (long)(H / n_slabs) * W; a.C = C; a.S = n_slabs;
  return launch_cfg_step<true, false, false>("cfg_step_rows", stream, dtype, flow, a);
}

// the inpainting rows of the masked and the multistep entries: the same refusals under either name
static int set_inpaint_rows(const std::string& what, step_args& a, const mx_inpaint_rows* r) {
  if (!r) return 0;
  MX_CHECK(r->k >= 0, what + ": k must not be negative");
  MX_CHECK(r->k == 0 || (r->slot && r->init && r->noise && r->mask), what + ": inpainting rows need slot, init, noise and mask");
  if (r->k > 0) { a.k = r->k; a.slot = r->slot; a.init = r->init; a.noise = r->noise; a.mask = r->mask; }
  return 0;
}

static int cfg_step_masked(bool flow, void* stream, const void* pred, void* latents, const float* sigma, const float* sigma_next, float g, int n_lat, int C,
                           int hw, int dtype, const mx_inpaint_rows* r) {
  MX_CHECK(pred && latents && sigma && sigma_next && r, "cfg_step_masked: null operand");
  MX_CHECK(n_lat > 0 && C > 0 && hw > 0, "cfg_step_masked: sizes must be positive");
  step_args a = base_args(pred, latents, sigma, sigma_next, g, n_lat, (long)C * hw);
  a.run = hw;
  if (set_inpaint_rows("cfg_step_masked", a, r)) return 1;
  return launch_cfg_step<false, false, true>("cfg_step_masked", stream, dtype, flow, a);
}

}  // namespace mx

extern "C" int mx_cfg_euler_step(void* stream, const void* noise, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                                 int n_lat, int64_t elems, int dtype) {
  return mx::cfg_step_plain("cfg_euler_step", false, stream, noise, latents, sigma, sigma_next, guidance_scale, n_lat, elems, dtype);
}

extern "C" int mx_cfg_flow_step(void* stream, const void* noise, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                                int n_lat, int64_t elems, int dtype) {
  return mx::cfg_step_plain("cfg_flow_step", true, stream, noise, latents, sigma, sigma_next, guidance_scale, n_lat, elems, dtype);
}

extern "C" int mx_cfg_euler_step_rows(void* stream, const void* gathered, void* latents, const float* sigma, const float* sigma_next,
                                      float guidance_scale, int n_lat, int C, int H, int W, int n_slabs, int dtype) {
  return mx::cfg_step_rows(false, stream, gathered, latents, sigma, sigma_next, guidance_scale, n_lat, C, H, W, n_slabs, dtype);
}

extern "C" int mx_cfg_flow_step_rows(void* stream, const void* gathered, void* latents, const float* sigma, const float* sigma_next,
                                     float guidance_scale, int n_lat, int C, int H, int W, int n_slabs, int dtype) {
  return mx::cfg_step_rows(true, stream, gathered, latents, sigma, sigma_next, guidance_scale, n_lat, C, H, W, n_slabs, dtype);
}

extern "C" int mx_cfg_euler_step_masked(void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                                        int n_lat, int C, int hw, int dtype, const mx_inpaint_rows* rows) {
  return mx::cfg_step_masked(false, stream, noise_pred, latents, sigma, sigma_next, guidance_scale, n_lat, C, hw, dtype, rows);
}

extern "C" int mx_cfg_flow_step_masked(void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                                       int n_lat, int C, int hw, int dtype, const mx_inpaint_rows* rows) {
  return mx::cfg_step_masked(true, stream, noise_pred, latents, sigma, sigma_next, guidance_scale, n_lat, C, hw, dtype, rows);
}

namespace mx {
// the multistep and the stochastic entry: the same refusals under either name; nz: the noise rows (null: none, the form without NOISY)
static int cfg_step_multistep(const std::string& what, void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next,
                              float guidance_scale, int n_lat, int C, int hw, int dtype, int flow, const mx_multistep_rows* ms,
                              const mx_inpaint_rows* inpaint, const mx_noise_rows* nz) {
  MX_CHECK(noise_pred && latents && sigma && sigma_next && ms, what + ": null operand");
  MX_CHECK(ms->kind && ms->coef && ms->hist, what + ": null kind, coef or hist");
  MX_CHECK(!nz || (nz->cn && nz->seed && nz->step), what + ": null cn, seed or step of the noise rows");
  MX_CHECK(n_lat > 0 && C > 0 && hw > 0, what + ": sizes must be positive");
  MX_CHECK(dtype == MX_F32 || dtype == MX_F16 || dtype == MX_BF16, what + ": bad dtype");
  {                                                      // the history is written while both are read: no byte of it may lie inside either
    const size_t esz = dtype == MX_F32 ? 4 : 2, total = (size_t)n_lat * C * hw;
    const uintptr_t h0 = (uintptr_t)ms->hist, h1 = h0 + total * 4, l0 = (uintptr_t)latents, p0 = (uintptr_t)noise_pred;
    const bool apart = (h1 <= l0 || l0 + total * esz <= h0) && (h1 <= p0 || p0 + (guidance_scale > 0.f ? 2 : 1) * total * esz <= h0);
    MX_CHECK(apart, what + ": hist may alias neither the latents nor the prediction");
  }
  step_args a = base_args(noise_pred, latents, sigma, sigma_next, guidance_scale, n_lat, (long)C * hw);
  a.run = hw; a.kind = ms->kind; a.coef = ms->coef; a.hist = ms->hist;
  if (set_inpaint_rows(what, a, inpaint)) return 1;
  if (!nz) return launch_cfg_step<false, true, true>(what.c_str(), stream, dtype, flow != 0, a);
  a.cn = nz->cn; a.seed = (const unsigned long long*)nz->seed; a.nstep = nz->step;
  return launch_cfg_step<false, true, true, true>(what.c_str(), stream, dtype, flow != 0, a);
}
}  // namespace mx

extern "C" int mx_cfg_multistep_step(void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                                     int n_lat, int C, int hw, int dtype, int flow, const mx_multistep_rows* ms, const mx_inpaint_rows* inpaint) {
  return mx::cfg_step_multistep("cfg_multistep_step", stream, noise_pred, latents, sigma, sigma_next, guidance_scale, n_lat, C, hw, dtype, flow, ms, inpaint,
                                nullptr);
}

extern "C" int mx_cfg_stochastic_step(void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                                      int n_lat, int C, int hw, int dtype, int flow, const mx_multistep_rows* ms, const mx_inpaint_rows* inpaint,
                                      const mx_noise_rows* nz) {
  return mx::cfg_step_multistep("cfg_stochastic_step", stream, noise_pred, latents, sigma, sigma_next, guidance_scale, n_lat, C, hw, dtype, flow, ms, inpaint,
                                nz);
}
