// Small HBM-bound glue kernels of the step plan (gfx950): layout conversion at the model boundary,
// sinusoidal embeddings, and the scheduler's input scaling in front of the UNet (the step behind it: scheduler_step.hip).
#include <algorithm>

#include "common.h"
#include "../../include/mxdenoise.h"

// euler_scale_input_kernel and vae_latent_finish_kernel reproduce torch's op-by-op IEEE evaluation bit for bit: no mul+add contraction into FMA in this
// translation unit (HIP's __fmul_rn/__fadd_rn are plain operators in inlined headers and do get contracted; so plain operators here, plus
// -ffp-contract=off for this file in the Makefile).
#pragma clang fp contract(off)
#include "step_math.h"   // load_as_f32 / store_from_f32, rnd, renoise: shared with scheduler_step.hip and inpaint.hip

namespace mx {

// NCHW latents of any io dtype -> NHWC bf16 with the channel dim zero-padded to CP (=64), so conv_in
// runs on the same implicit-GEMM kernel as every other conv (unet.py:344).
template <typename T>
__global__ void prep_latent_kernel(const T* __restrict__ in, bf16_t* __restrict__ out, int B, int Cin, int HW, int CP) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (pixel, 8-channel chunk)
  const int chunks = CP / 8;
  const long total = (long)B * HW * chunks;
  if (idx >= total) return;
  const int ch = (int)(idx % chunks);
  const long pix = idx / chunks;
  const int b = (int)(pix / HW);
  const int p = (int)(pix - (long)b * HW);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = ch * 8 + e;
    v[e] = (c < Cin) ? load_as_f32<T>(in, ((long)b * Cin + c) * HW + p) : 0.f;
  }
  u32x4 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
  *reinterpret_cast<u32x4*>(out + idx * 8) = o;
}

// NHWC bf16 [B*HW, ld] (first C columns) -> NCHW io dtype
template <typename T>
__global__ void nhwc_to_nchw_kernel(const bf16_t* __restrict__ in, T* __restrict__ out, int B, int C, int HW, int ld) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over B*C*HW, p fastest
  const long total = (long)B * C * HW;
  if (idx >= total) return;
  const int p = (int)(idx % HW);
  const long bc = idx / HW;
  const int c = (int)(bc % C);
  const int b = (int)(bc / C);
  store_from_f32<T>(out, idx, bf16_to_f32(in[((long)b * HW + p) * ld + c]));
}

// diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin], bf16 out.
// tsin [B, d0] from timesteps; addin [B, text_dim + 6*da] = [text_embeds | sinusoid(time_ids)] (unet.py:314-334).
__global__ void time_embed_kernel(const float* __restrict__ timesteps, const bf16_t* __restrict__ text_embeds,
                                  const float* __restrict__ time_ids, bf16_t* __restrict__ tsin,
                                  bf16_t* __restrict__ addin, int B, int d0, int text_dim, int da) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int addw = text_dim + 6 * da;
  if (i < d0) {
    const int half = d0 / 2;
    const int j = (i < half) ? i : i - half;
    const float freq = __expf(-9.210340371976184f * (float)j / (float)half);
    const float ang = timesteps[b] * freq;
    tsin[(long)b * d0 + i] = f32_to_bf16((i < half) ? cosf(ang) : sinf(ang));
  }
  if (i < addw) {
    bf16_t o;
    if (i < text_dim) {
      o = text_embeds[(long)b * text_dim + i];
    } else {
      const int k = i - text_dim;
      const int which = k / da;
      const int e = k - which * da;
      const int half = da / 2;
      const int j = (e < half) ? e : e - half;
      const float freq = __expf(-9.210340371976184f * (float)j / (float)half);
      const float ang = time_ids[b * 6 + which] * freq;
      o = f32_to_bf16((e < half) ? cosf(ang) : sinf(ang));
    }
    addin[(long)b * addw + i] = o;
  }
}

// batch_scale_model_input with the CFG duplication fused (scheduling_euler_discrete.py:161-184)
template <typename T>
__global__ void euler_scale_input_kernel(const T* __restrict__ lat, T* __restrict__ out, const float* __restrict__ sigma,
                                         int n_lat, int n_rows, long elems) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n_rows * elems) return;
  const int row = (int)(idx / elems);
  const long e = idx - (long)row * elems;
  const int src = row % n_lat;
  // the reference evaluates samples / ((sigmas ** 2 + 1) ** 0.5) with sigmas cast to the tensor dtype
  // (scheduling_euler_discrete.py:175-182): one rounding to T per op
  const float s = rnd<T>(sigma[src]);
  const float denom = rnd<T>(__fsqrt_rn(rnd<T>(rnd<T>(s * s) + 1.0f)));   // correctly rounded sqrt, as torch.pow(x, 0.5) -> sqrt
  store_from_f32<T>(out, idx, load_as_f32<T>(lat, (long)src * elems + e) / denom);
}

}  // namespace mx

using namespace mx;

// ---- internal launchers used by the step plan (C++ linkage inside the library) ----
namespace mx {
int launch_prep_latent(hipStream_t s, const void* in, int dtype, void* out, int B, int Cin, int HW, int CP) {
  MX_CHECK(CP % 8 == 0 && Cin <= CP, "prep_latent: bad channel padding");
  const long total = (long)B * HW * (CP / 8);
  dim3 grid((unsigned)cdiv64(total, 256)), block(256);
  if (dtype == MX_F32) hipLaunchKernelGGL((prep_latent_kernel<float>), grid, block, 0, s, (const float*)in, (bf16_t*)out, B, Cin, HW, CP);
  else if (dtype == MX_F16) hipLaunchKernelGGL((prep_latent_kernel<_Float16>), grid, block, 0, s, (const _Float16*)in, (bf16_t*)out, B, Cin, HW, CP);
  else if (dtype == MX_BF16) hipLaunchKernelGGL((prep_latent_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)in, (bf16_t*)out, B, Cin, HW, CP);
  else MX_CHECK(false, "prep_latent: bad dtype");
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_nhwc_to_nchw(hipStream_t s, const void* in, void* out, int dtype, int B, int C, int HW, int ld) {
  MX_CHECK(ld >= C, "nhwc_to_nchw: ld must hold the C columns");
  const long total = (long)B * C * HW;
  dim3 grid((unsigned)cdiv64(total, 256)), block(256);
  if (dtype == MX_F32) hipLaunchKernelGGL((nhwc_to_nchw_kernel<float>), grid, block, 0, s, (const bf16_t*)in, (float*)out, B, C, HW, ld);
  else if (dtype == MX_F16) hipLaunchKernelGGL((nhwc_to_nchw_kernel<_Float16>), grid, block, 0, s, (const bf16_t*)in, (_Float16*)out, B, C, HW, ld);
  else if (dtype == MX_BF16) hipLaunchKernelGGL((nhwc_to_nchw_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)in, (bf16_t*)out, B, C, HW, ld);
  else MX_CHECK(false, "nhwc_to_nchw: bad dtype");
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_time_embed(hipStream_t s, const float* timesteps, const void* text_embeds, const float* time_ids,
                      void* tsin, void* addin, int B, int d0, int text_dim, int da) {
  MX_CHECK(d0 >= 2 && d0 % 2 == 0 && da >= 2 && da % 2 == 0, "time_embed: d0 and da must be even");
  const int w = (d0 > text_dim + 6 * da) ? d0 : text_dim + 6 * da;
  dim3 grid(cdiv(w, 256), B), block(256);
  hipLaunchKernelGGL(time_embed_kernel, grid, block, 0, s, timesteps, (const bf16_t*)text_embeds, time_ids,
                     (bf16_t*)tsin, (bf16_t*)addin, B, d0, text_dim, da);
  MX_LAUNCH_CHECK();
  return 0;
}
}  // namespace mx

extern "C" int mx_euler_scale_input(void* stream, const void* latents, void* out, const float* sigma,
                                    int n_lat, int n_rows, int64_t elems, int dtype) {
  MX_CHECK(latents && out && sigma && n_lat > 0 && n_rows >= n_lat && elems > 0, "euler_scale_input: bad arguments");
  const long total = (long)n_rows * elems;
  dim3 grid((unsigned)cdiv64(total, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MX_F32) hipLaunchKernelGGL((euler_scale_input_kernel<float>), grid, block, 0, s, (const float*)latents, (float*)out, sigma, n_lat, n_rows, (long)elems);
  else if (dtype == MX_F16) hipLaunchKernelGGL((euler_scale_input_kernel<_Float16>), grid, block, 0, s, (const _Float16*)latents, (_Float16*)out, sigma, n_lat, n_rows, (long)elems);
  else if (dtype == MX_BF16) hipLaunchKernelGGL((euler_scale_input_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)latents, (bf16_t*)out, sigma, n_lat, n_rows, (long)elems);
  else MX_CHECK(false, "euler_scale_input: bad dtype");
  MX_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------
// MMDiT edge kernels (SD3Transformer.py:82-83, 250-259; scheduling_flow_match_euler_discrete.py:186-196)
// ------------------------------------------------------------------------------------------
namespace mx {

// PatchEmbed im2col: latents NCHW -> tokens [B*h*w, ps*ps*C] bf16, k = (dy*ps + dx)*C + c
template <typename T>
__global__ void patchify_kernel(const T* __restrict__ in, bf16_t* __restrict__ out, int B, int Cc, int H, int W, int ps) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int K = ps * ps * Cc;
  const int h = H / ps, w = W / ps;
  if (idx >= (long)B * h * w * K) return;
  const int k = (int)(idx % K);
  const long tok = idx / K;
  const int c = k % Cc;
  const int dd = k / Cc;
  const int dy = dd / ps, dx = dd % ps;
  const int x = (int)(tok % w);
  const int y = (int)((tok / w) % h);
  const int b = (int)(tok / ((long)w * h));
  out[idx] = f32_to_bf16(load_as_f32<T>(in, (((long)b * Cc + c) * H + y * ps + dy) * W + x * ps + dx));
}

// tokens [B*h*w, ld] (first ps*ps*C columns, (p, q, c) order) -> NCHW [B, C, h*ps, w*ps]   ("nhwpqc->nchpwq")
template <typename T>
__global__ void unpatchify_kernel(const bf16_t* __restrict__ in, T* __restrict__ out, int B, int Cc, int H, int W, int ps, int ld) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // over B*C*H*W
  if (idx >= (long)B * Cc * H * W) return;
  const int X = (int)(idx % W);
  const int Y = (int)((idx / W) % H);
  const int c = (int)((idx / ((long)W * H)) % Cc);
  const int b = (int)(idx / ((long)W * H * Cc));
  const int w = W / ps, h = H / ps;
  const long tok = ((long)b * h + Y / ps) * w + X / ps;
  const int k = ((Y % ps) * ps + (X % ps)) * Cc + c;
  store_from_f32<T>(out, idx, bf16_to_f32(in[tok * ld + k]));
}

// rows (top + y, left + x) of a [m, m, d] table -> [h*w, d]   (PatchEmbed.cropped_pos_embed)
__global__ void crop_pos_kernel(const bf16_t* __restrict__ table, bf16_t* __restrict__ out, int m, int h, int w, int d) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // 16-byte chunks
  const int chunks = d / 8;
  if (idx >= (long)h * w * chunks) return;
  const int ch = (int)(idx % chunks);
  const long tok = idx / chunks;
  const int x = (int)(tok % w), y = (int)(tok / w);
  const int top = (m - h) / 2, left = (m - w) / 2;
  const long src = ((long)(top + y) * m + left + x) * d + ch * 8;
  *reinterpret_cast<u32x4*>(out + idx * 8) = *reinterpret_cast<const u32x4*>(table + src);
}

// [cos | sin] sinusoid of one scalar per row (Timesteps(dim, flip_sin_to_cos=True, freq_shift 0)), bf16 out
__global__ void sinus_embed_kernel(const float* __restrict__ t, bf16_t* __restrict__ out, int dim) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= dim) return;
  const int half = dim / 2;
  const int j = (i < half) ? i : i - half;
  const float ang = t[b] * __expf(-9.210340371976184f * (float)j / (float)half);
  out[(long)b * dim + i] = f32_to_bf16((i < half) ? cosf(ang) : sinf(ang));
}

int launch_patchify(hipStream_t s, const void* in, int dtype, void* out, int B, int C, int H, int W, int ps) {
  MX_CHECK(ps > 0 && H % ps == 0 && W % ps == 0, "patchify: H and W must be multiples of the patch size");
  const long total = (long)B * H * W * C;
  dim3 grid((unsigned)cdiv64(total, 256)), block(256);
  if (dtype == MX_F32) hipLaunchKernelGGL((patchify_kernel<float>), grid, block, 0, s, (const float*)in, (bf16_t*)out, B, C, H, W, ps);
  else if (dtype == MX_F16) hipLaunchKernelGGL((patchify_kernel<_Float16>), grid, block, 0, s, (const _Float16*)in, (bf16_t*)out, B, C, H, W, ps);
  else if (dtype == MX_BF16) hipLaunchKernelGGL((patchify_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)in, (bf16_t*)out, B, C, H, W, ps);
  else MX_CHECK(false, "patchify: bad dtype");
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_unpatchify(hipStream_t s, const void* in, void* out, int dtype, int B, int C, int H, int W, int ps, int ld) {
  MX_CHECK(ps > 0 && H % ps == 0 && W % ps == 0, "unpatchify: H and W must be multiples of the patch size");
  MX_CHECK((long)ld >= (long)ps * ps * C, "unpatchify: ld must hold the ps*ps*C columns");
  const long total = (long)B * H * W * C;
  dim3 grid((unsigned)cdiv64(total, 256)), block(256);
  if (dtype == MX_F32) hipLaunchKernelGGL((unpatchify_kernel<float>), grid, block, 0, s, (const bf16_t*)in, (float*)out, B, C, H, W, ps, ld);
  else if (dtype == MX_F16) hipLaunchKernelGGL((unpatchify_kernel<_Float16>), grid, block, 0, s, (const bf16_t*)in, (_Float16*)out, B, C, H, W, ps, ld);
  else if (dtype == MX_BF16) hipLaunchKernelGGL((unpatchify_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)in, (bf16_t*)out, B, C, H, W, ps, ld);
  else MX_CHECK(false, "unpatchify: bad dtype");
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_crop_pos(hipStream_t s, const void* table, void* out, int m, int h, int w, int d) {
  MX_CHECK(d % 8 == 0 && h <= m && w <= m, "crop_pos: bad geometry");
  const long total = (long)h * w * (d / 8);
  hipLaunchKernelGGL(crop_pos_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, s, (const bf16_t*)table, (bf16_t*)out, m, h, w, d);
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_sinus_embed(hipStream_t s, const float* t, void* out, int B, int dim) {
  MX_CHECK(dim >= 2 && dim % 2 == 0, "sinus_embed: dim must be even");
  hipLaunchKernelGGL(sinus_embed_kernel, dim3(cdiv(dim, 256), B), dim3(256), 0, s, t, (bf16_t*)out, dim);
  MX_LAUNCH_CHECK();
  return 0;
}
}  // namespace mx

// ------------------------------------------------------------------------------------------
// Row softmax in place on a bf16 [rows, L] score matrix (fp32 math): the VAE decoder's single-head, 512-wide mid-block
// attention (diffusers Attention with heads = 1; AutoencoderKL decoder) is computed as GEMM -> softmax -> GEMM.
// ------------------------------------------------------------------------------------------
namespace mx {
// exp(d), d <= 0, as __expf evaluates it -- exp2(fl(log2(e) d)), one v_exp_f32 -- but with results below 2^-126 kept as fp32 subnormals: the
// instruction alone returns +0 there, and a probability down to 2^-134 still has a bf16 value.  Below -126 the argument is raised by 64 and the
// result scaled back (exact but for the one rounding into the subnormal range); above it the bits are __expf's.
__device__ __forceinline__ float exp_gradual(float d) {
  const float a = 0x1.715476p+0f * d;
  const bool low = a < -126.0f;
  const float e = __builtin_amdgcn_exp2f(low ? a + 64.0f : a);
  return low ? e * 0x1p-64f : e;
}
__global__ __launch_bounds__(256) void softmax_rows_kernel(bf16_t* __restrict__ s, int L, long ld) {
  __shared__ float red[8];
  bf16_t* row = s + (long)blockIdx.x * ld;
  const int t = threadIdx.x;
  float mx_ = -INFINITY;
  for (int i = t; i < L / 8; i += 256) {
    const u32x4 v = reinterpret_cast<const u32x4*>(row)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) mx_ = fmaxf(mx_, fmaxf(bf16lo_to_f32(v[e]), bf16hi_to_f32(v[e])));
  }
  mx_ = wave_max(mx_);
  if ((t & 63) == 0) red[t >> 6] = mx_;
  __syncthreads();
  mx_ = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int i = t; i < L / 8; i += 256) {
    const u32x4 v = reinterpret_cast<const u32x4*>(row)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) sum += exp_gradual(bf16lo_to_f32(v[e]) - mx_) + exp_gradual(bf16hi_to_f32(v[e]) - mx_);
  }
  sum = wave_sum(sum);
  if ((t & 63) == 0) red[4 + (t >> 6)] = sum;
  __syncthreads();
  const float inv = 1.0f / (red[4] + red[5] + red[6] + red[7]);
  for (int i = t; i < L / 8; i += 256) {
    const u32x4 v = reinterpret_cast<const u32x4*>(row)[i];
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(exp_gradual(bf16lo_to_f32(v[e]) - mx_) * inv, exp_gradual(bf16hi_to_f32(v[e]) - mx_) * inv);
    reinterpret_cast<u32x4*>(row)[i] = o;
  }
}
int launch_softmax_rows(hipStream_t s, void* scores, long rows, int L, long ld) {
  MX_CHECK(L % 8 == 0 && ld % 8 == 0 && rows > 0, "softmax_rows: L and ld must be multiples of 8");
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, (bf16_t*)scores, L, ld);
  MX_LAUNCH_CHECK();
  return 0;
}
}  // namespace mx

// ----------------------------------------------------------------------------------------------------------------------
// CLIP text encoder glue (clip_text.cpp): token + position embedding lookup, and the pooled row of each prompt
// ----------------------------------------------------------------------------------------------------------------------
namespace mx {
// out[b, t, :] = tok[ids[b, t], :] + pos[t, :]   (bf16 tables, fp32 add, one rounding; pos == nullptr: token embedding only, T5); ids are clamped to the vocabulary
__global__ void clip_embed_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ tok, const bf16_t* __restrict__ pos,
                                  bf16_t* __restrict__ out, int rows, int L, int H, int vocab) {
  const int row = blockIdx.x;
  if (row >= rows) return;
  int id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const bf16_t* tr = tok + (long)id * H;
  const bf16_t* pr = pos + (long)(row % L) * H;
  bf16_t* orow = out + (long)row * H;
  for (int c = threadIdx.x * 8; c < H; c += blockDim.x * 8) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(tr + c), b = pos ? *reinterpret_cast<const u32x4*>(pr + c) : u32x4{0u, 0u, 0u, 0u};
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(bf16lo_to_f32(a[e]) + bf16lo_to_f32(b[e]), bf16hi_to_f32(a[e]) + bf16hi_to_f32(b[e]));
    *reinterpret_cast<u32x4*>(orow + c) = o;
  }
}
// pooled[b, :] = x[b, eos(b), :], eos(b) = first position holding eos_id, or (eos_id < 0: the legacy CLIP configs with eos_token_id == 2)
// the position of the largest id (transformers CLIPTextTransformer.forward)
__global__ void clip_pool_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ x, bf16_t* __restrict__ out, int L, int H, int eos_id) {
  const int b = blockIdx.x;
  __shared__ int pos_s;
  if (threadIdx.x == 0) {
    int best = 0;
    if (eos_id >= 0) {
      best = L - 1;                                      // (argmax of an all-false mask is 0 in the reference; a prompt always has its EOS)
      for (int t = 0; t < L; ++t) if (ids[b * L + t] == eos_id) { best = t; break; }
      bool any = false;
      for (int t = 0; t < L; ++t) any |= ids[b * L + t] == eos_id;
      if (!any) best = 0;
    } else {
      int mx_id = ids[b * L];
      for (int t = 1; t < L; ++t) if (ids[b * L + t] > mx_id) { mx_id = ids[b * L + t]; best = t; }
    }
    pos_s = best;
  }
  __syncthreads();
  const bf16_t* src = x + ((long)b * L + pos_s) * H;
  for (int c = threadIdx.x * 8; c < H; c += blockDim.x * 8) *reinterpret_cast<u32x4*>(out + (long)b * H + c) = *reinterpret_cast<const u32x4*>(src + c);
}
int launch_clip_embed(hipStream_t s, const int* ids, const bf16_t* tok, const bf16_t* pos, bf16_t* out, int rows, int L, int H, int vocab) {
  MX_CHECK(H % 8 == 0, "clip_embed: hidden size must be a multiple of 8");
  hipLaunchKernelGGL(clip_embed_kernel, dim3(rows), dim3(128), 0, s, ids, tok, pos, out, rows, L, H, vocab);
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_clip_pool(hipStream_t s, const int* ids, const bf16_t* x, bf16_t* out, int B, int L, int H, int eos_id) {
  MX_CHECK(H % 8 == 0, "clip_pool: hidden size must be a multiple of 8");
  hipLaunchKernelGGL(clip_pool_kernel, dim3(B), dim3(128), 0, s, ids, x, out, L, H, eos_id);
  MX_LAUNCH_CHECK();
  return 0;
}
}  // namespace mx

// ----------------------------------------------------------------------------------------------------------------------
// one launch each on caller-made operands (include/mxdenoise.h: "Glue kernels, one launch each"): the launchers above behind their host checks
// ----------------------------------------------------------------------------------------------------------------------
extern "C" int mx_prep_latent(void* stream, const void* in, int dtype, void* out, int B, int Cin, int HW, int CP) {
  MX_CHECK(in && out && B > 0 && Cin > 0 && HW > 0 && CP > 0, "prep_latent: null operand or empty shape");
  MX_CHECK(mx::aligned_to(out, 16), "prep_latent: out must be 16-byte aligned");
  return mx::launch_prep_latent((hipStream_t)stream, in, dtype, out, B, Cin, HW, CP);
}
extern "C" int mx_nhwc_to_nchw(void* stream, const void* in, void* out, int dtype, int B, int C, int HW, int ld) {
  MX_CHECK(in && out && B > 0 && C > 0 && HW > 0, "nhwc_to_nchw: null operand or empty shape");
  return mx::launch_nhwc_to_nchw((hipStream_t)stream, in, out, dtype, B, C, HW, ld);
}
extern "C" int mx_time_embed(void* stream, const float* timesteps, const void* text_embeds, const float* time_ids, void* tsin, void* addin, int B, int d0,
                             int text_dim, int da) {
  MX_CHECK(timesteps && text_embeds && time_ids && tsin && addin && B > 0 && d0 > 0 && text_dim > 0 && da > 0, "time_embed: null operand or empty shape");
  return mx::launch_time_embed((hipStream_t)stream, timesteps, text_embeds, time_ids, tsin, addin, B, d0, text_dim, da);
}
extern "C" int mx_sinus_embed(void* stream, const float* t, void* out, int B, int dim) {
  MX_CHECK(t && out && B > 0 && dim > 0, "sinus_embed: null operand or empty shape");
  return mx::launch_sinus_embed((hipStream_t)stream, t, out, B, dim);
}
extern "C" int mx_patchify(void* stream, const void* in, int dtype, void* out, int B, int C, int H, int W, int ps) {
  MX_CHECK(in && out && B > 0 && C > 0 && H > 0 && W > 0 && ps > 0, "patchify: null operand or empty shape");
  return mx::launch_patchify((hipStream_t)stream, in, dtype, out, B, C, H, W, ps);
}
extern "C" int mx_unpatchify(void* stream, const void* in, void* out, int dtype, int B, int C, int H, int W, int ps, int ld) {
  MX_CHECK(in && out && B > 0 && C > 0 && H > 0 && W > 0 && ps > 0, "unpatchify: null operand or empty shape");
  return mx::launch_unpatchify((hipStream_t)stream, in, out, dtype, B, C, H, W, ps, ld);
}
extern "C" int mx_crop_pos(void* stream, const void* table, void* out, int m, int h, int w, int d) {
  MX_CHECK(table && out && m > 0 && h > 0 && w > 0 && d > 0, "crop_pos: null operand or empty shape");
  MX_CHECK(mx::aligned_to(table, 16) && mx::aligned_to(out, 16), "crop_pos: table and out must be 16-byte aligned");
  return mx::launch_crop_pos((hipStream_t)stream, table, out, m, h, w, d);
}
extern "C" int mx_softmax_rows(void* stream, void* scores, int64_t rows, int L, int64_t ld) {
  MX_CHECK(scores && rows > 0 && L > 0 && ld >= L, "softmax_rows: null operand or empty shape");
  MX_CHECK(mx::aligned_to(scores, 16), "softmax_rows: scores must be 16-byte aligned");
  return mx::launch_softmax_rows((hipStream_t)stream, scores, (long)rows, L, (long)ld);
}
extern "C" int mx_clip_embed(void* stream, const int32_t* ids, const void* tok, const void* pos, void* out, int rows, int L, int H, int vocab) {
  MX_CHECK(ids && tok && out && rows > 0 && L > 0 && H > 0 && vocab > 0, "clip_embed: null operand or empty shape");
  MX_CHECK(mx::aligned_to(tok, 16) && mx::aligned_to(pos, 16) && mx::aligned_to(out, 16), "clip_embed: tables and out must be 16-byte aligned");
  return mx::launch_clip_embed((hipStream_t)stream, ids, (const mx::bf16_t*)tok, (const mx::bf16_t*)pos, (mx::bf16_t*)out, rows, L, H, vocab);
}
extern "C" int mx_clip_pool(void* stream, const int32_t* ids, const void* x, void* out, int B, int L, int H, int eos_id) {
  MX_CHECK(ids && x && out && B > 0 && L > 0 && H > 0, "clip_pool: null operand or empty shape");
  MX_CHECK(mx::aligned_to(x, 16) && mx::aligned_to(out, 16), "clip_pool: x and out must be 16-byte aligned");
  return mx::launch_clip_pool((hipStream_t)stream, ids, (const mx::bf16_t*)x, (mx::bf16_t*)out, B, L, H, eos_id);
}

// ----------------------------------------------------------------------------------------------------------------------
// Block-skip cache (unet_sdxl.cpp, mx_unet_forward_cached): per-sample squared difference of a block input against the input the block saw
// when it last ran -- the feature of the reference's CacheManager.get_mask (modules/cache_manager.py:105-159: mse_loss(...).mean(dim=(-1,-2,-3)))
// ----------------------------------------------------------------------------------------------------------------------
namespace mx {
constexpr int kMseChunks = 64;
// partial[b][chunk] = sum over the chunk of (a - b)^2 (fp32 in-thread, fp64 across the block); the host adds the 64 partials of a sample: the
// result does not depend on launch order
// slot (optional): sample i of `b` lives at row slot[i] (the block-skip cache keeps one row per request, not per batch position)
__global__ __launch_bounds__(256) void sq_diff_partial_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, long elems, double* __restrict__ partial,
                                                              const int* __restrict__ slot) {
  const int smp = blockIdx.y, chunk = blockIdx.x;
  const long per = (elems / 8 + kMseChunks - 1) / kMseChunks;           // 16-byte vectors per chunk
  const long v0 = (long)chunk * per, v1 = min(v0 + per, elems / 8);
  const bf16_t* pa = a + (long)smp * elems; const bf16_t* pb = b + (long)(slot ? slot[smp] : smp) * elems;
  float acc = 0.f;
  for (long v = v0 + threadIdx.x; v < v1; v += 256) {
    const u32x4 x = *reinterpret_cast<const u32x4*>(pa + v * 8), y = *reinterpret_cast<const u32x4*>(pb + v * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d0 = bf16lo_to_f32(x[e]) - bf16lo_to_f32(y[e]), d1 = bf16hi_to_f32(x[e]) - bf16hi_to_f32(y[e]);
      acc += d0 * d0 + d1 * d1;
    }
  }
  __shared__ double red[4];
  double d = (double)acc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long)smp * kMseChunks + chunk] = red[0] + red[1] + red[2] + red[3];
}
int launch_sq_diff_partial(hipStream_t s, const void* a, const void* b, long elems_per_sample, int B, double* partial, const int* slot) {
  MX_CHECK(elems_per_sample % 8 == 0, "sq_diff: elements per sample must be a multiple of 8");
  hipLaunchKernelGGL(sq_diff_partial_kernel, dim3(kMseChunks, B), dim3(256), 0, s, (const bf16_t*)a, (const bf16_t*)b, elems_per_sample, partial, slot);
  MX_LAUNCH_CHECK();
  return 0;
}
// rows of `bytes` (a multiple of 16) between a batch-ordered tensor and a slot-ordered one: scatter: slotted[slot[i]] = batch[i]; gather: batch[i] =
// slotted[slot[i]]
__global__ __launch_bounds__(256) void copy_rows_kernel(char* __restrict__ batch, char* __restrict__ slotted, long vecs, const int* __restrict__ slot, int scatter) {
  const int smp = blockIdx.y;
  if (slot[smp] < 0) return;                   // a sample the copy does not concern (block cache: partial reuse inside a running block)
  u32x4* pb = reinterpret_cast<u32x4*>(batch) + (long)smp * vecs;
  u32x4* ps = reinterpret_cast<u32x4*>(slotted) + (long)slot[smp] * vecs;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < vecs; v += (long)gridDim.x * 256) {
    if (scatter) ps[v] = pb[v]; else pb[v] = ps[v];
  }
}
int launch_copy_rows(hipStream_t s, void* batch, void* slotted, size_t bytes_per_sample, int B, const int* slot, int scatter) {
  MX_CHECK(bytes_per_sample % 16 == 0 && slot != nullptr, "copy_rows: rows must be multiples of 16 bytes");
  const long vecs = (long)(bytes_per_sample / 16);
  const int gx = (int)std::min<long>((vecs + 255) / 256, 256);
  hipLaunchKernelGGL(copy_rows_kernel, dim3(gx, B), dim3(256), 0, s, (char*)batch, (char*)slotted, vecs, slot, scatter);
  MX_LAUNCH_CHECK();
  return 0;
}
}  // namespace mx
// one launch each on caller-made operands (include/mxdenoise.h: "Block-skip cache kernels, one launch each")
extern "C" int mx_sq_diff_partial(void* stream, const void* a, const void* b, int64_t elems_per_sample, int n_samples, double* partial, const int32_t* slot) {
  MX_CHECK(a && b && partial && n_samples > 0 && elems_per_sample > 0, "sq_diff_partial: null operand or empty shape");
  return mx::launch_sq_diff_partial((hipStream_t)stream, a, b, (long)elems_per_sample, n_samples, partial, slot);
}
extern "C" int mx_copy_rows(void* stream, void* batch, void* slotted, size_t bytes_per_sample, int n_samples, const int32_t* slot, int scatter) {
  MX_CHECK(batch && slotted && n_samples > 0 && bytes_per_sample > 0, "copy_rows: null operand or empty shape");
  return mx::launch_copy_rows((hipStream_t)stream, batch, slotted, bytes_per_sample, n_samples, slot, scatter);
}

// ------------------------------------------------------------------------------------------
// The last launch of the VAE encoder (vae_sdxl.cpp, EncodePlan): moments -> the latents a request starts from.
// DiagonalGaussianDistribution.mode / .sample, (z - shift_factor) * scaling_factor and, for a request that starts inside the schedule, the start
// step's noise (EulerDiscreteScheduler.add_noise: keep = 1, sigma = sigma[t_start]; the flow-match scale_noise: keep = 1 - sigma), stored NCHW.
// Every operation in fp32, rounded on its own (this translation unit contracts nothing); one rounding to the io dtype at the store.
// ------------------------------------------------------------------------------------------
namespace mx {
template <typename T>
__global__ void vae_latent_finish_kernel(const bf16_t* __restrict__ moments, int ld, T* __restrict__ out, int B, int lc, int h, int w, float scaling, float shift,
                                         const T* __restrict__ posterior_noise, const T* __restrict__ start_noise, const float* __restrict__ keep,
                                         const float* __restrict__ sigma, int rotate) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over B*lc*h*w, x fastest: the NCHW element
  const long total = (long)B * lc * h * w;
  if (idx >= total) return;
  const int x = (int)(idx % w);
  long r = idx / w;
  const int y = (int)(r % h); r /= h;
  const int c = (int)(r % lc);
  const int b = (int)(r / lc);
  const long row = (long)b * h * w + (rotate ? (long)(h - 1 - y) * w + (w - 1 - x) : (long)y * w + x);
  float z = bf16_to_f32(moments[row * ld + c]);
  if (posterior_noise) {
    float lv = bf16_to_f32(moments[row * ld + lc + c]);
    lv = fminf(fmaxf(lv, -30.0f), 20.0f);
    const float sd = expf(0.5f * lv);
    const float t = sd * load_as_f32<T>(posterior_noise, idx);
    z = z + t;
  }
  float lat = (z - shift) * scaling;
  if (start_noise) {
    lat = renoise(lat, load_as_f32<T>(start_noise, idx), keep[b], sigma[b]);
  }
  store_from_f32<T>(out, idx, lat);
}
}  // namespace mx

extern "C" int mx_vae_latent_finish(void* stream, const void* moments, int ld, void* out, int io_dtype, int B, int lc, int h, int w, float scaling, float shift,
                                    const void* posterior_noise, const void* start_noise, const float* keep, const float* sigma, int rotate) {
  MX_CHECK(moments && out, "vae_latent_finish: null operand");
  MX_CHECK(B > 0 && lc > 0 && h > 0 && w > 0, "vae_latent_finish: sizes must be positive");
  MX_CHECK(ld >= 2 * lc, "vae_latent_finish: ld must hold the mean and the logvar columns");
  MX_CHECK(rotate == 0 || rotate == 1, "vae_latent_finish: rotate must be 0 or 1");
  MX_CHECK(!start_noise || (keep && sigma), "vae_latent_finish: start_noise needs keep and sigma");
  MX_CHECK((long)B * h * w * ld < 2147483647L, "vae_latent_finish: the moments exceed 32-bit offsets");
  const long total = (long)B * lc * h * w;
  dim3 grid((unsigned)mx::cdiv64(total, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
#define MX_FINISH(T) hipLaunchKernelGGL((mx::vae_latent_finish_kernel<T>), grid, block, 0, s, (const mx::bf16_t*)moments, ld, (T*)out, B, lc, h, w, scaling, shift, \
                                        (const T*)posterior_noise, (const T*)start_noise, keep, sigma, rotate)
  if (io_dtype == MX_F32) MX_FINISH(float);
  else if (io_dtype == MX_F16) MX_FINISH(_Float16);
  else if (io_dtype == MX_BF16) MX_FINISH(mx::bf16_t);
  else MX_CHECK(false, "vae_latent_finish: bad dtype");
#undef MX_FINISH
  MX_LAUNCH_CHECK();
  return 0;
}
