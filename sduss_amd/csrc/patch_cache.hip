// Kernels of the block-skip cache at the reference's unit, the 256-px PATCH (mx_unet_forward_cached_mixed, include/mxdenoise.h;
// sduss/model_executor/modules/cache_manager.py:84-161 with is_sliced=True).  All HBM-bound data movement on NHWC / token-major bf16:
//
//   pc_image_copy    a sample's image between the batch-ordered activations and its row of a state tensor (one row per REQUEST, slot table),
//                    state -> batch optionally adding a per-sample channel vector (the time embedding, resnet.py:421-426) and a residual
//   pc_gather        the asking patches of a whole-image tensor -> a compact batch of patches, optionally with the reference's 1-pixel halo
//                    (get_adjacency / the fused GroupNorm's scatter: rows from the top / bottom neighbour, columns from the left / right one,
//                    corners = the left / right neighbour's own corner pixel, zeros at the image border: norm_silu_concat.cu:186-241) and
//                    optionally through a nearest-2x upsample (PatchUpsample2D interpolates, then exchanges halos: resnet.py:316-329)
//   pc_scatter       a compact batch of patches (cropped) -> the patches' places in the requests' state rows (update_and_return's
//                    `output[mask] = new_output`, cache_manager.py:95-97)
//   pc_patch_sq_diff per patch: sum of (x - cached x)^2 (the predictor's feature, cache_manager.py:112-123, 141-144)
//   pc_decide        the block's run / reuse decision for every unit from those sums (opt-in, mx_block_cache.dev_down): small and latency-bound
//
// Geometry: samples are described at LEVEL 0 (latent resolution) and every kernel takes the level of its tensor: image h >> level, w >> level,
// first row row0 >> 2 level, patch edge p0 >> level (the patch grid of a sample is the same at every level).
#include "common.h"
#include "patch_cache.h"
#include "skip_decide.h"
#include "../../include/mxdenoise.h"
#include <algorithm>

namespace mx {

__global__ __launch_bounds__(256) void pc_image_copy_kernel(bf16_t* batch, bf16_t* __restrict__ state, const PcSample* __restrict__ samp, int level,
                                                            int C, long state_row_elems, int to_batch, const float* __restrict__ vec, int ldvec,
                                                            const bf16_t* residual, int gate) {
  const PcSample s = samp[blockIdx.y];
  const long n = ((long)(s.h >> level) * (s.w >> level) * C) >> 3;        // 16-byte vectors of the image
  bf16_t* pb = batch + (s.row0 >> (2 * level)) * C;
  bf16_t* ps = state + (long)s.slot * state_row_elems;
  const bf16_t* pr = residual ? residual + (s.row0 >> (2 * level)) * C : nullptr;
  const float* pv = vec ? vec + (long)blockIdx.y * ldvec : nullptr;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < n; v += (long)gridDim.x * 256) {
    if (!to_batch) { reinterpret_cast<u32x4*>(ps)[v] = reinterpret_cast<const u32x4*>(pb)[v]; continue; }
    u32x4 x = reinterpret_cast<const u32x4*>(ps)[v];
    if (pv || pr) {
      const int c0 = (int)((v << 3) % C);
      u32x4 r = pr ? reinterpret_cast<const u32x4*>(pr)[v] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float lo = bf16lo_to_f32(x[e]), hi = bf16hi_to_f32(x[e]);
        if (pv && gate) { lo *= pv[c0 + 2 * e]; hi *= pv[c0 + 2 * e + 1]; }       // AdaLN-Zero gate (transformer.py:344-345): residual + gate * state
        else if (pv) { lo += pv[c0 + 2 * e]; hi += pv[c0 + 2 * e + 1]; }
        if (pr) { lo += bf16lo_to_f32(r[e]); hi += bf16hi_to_f32(r[e]); }
        x[e] = pack_bf16x2(lo, hi);
      }
    }
    reinterpret_cast<u32x4*>(pb)[v] = x;
  }
}

// state -> batch with a residual, TOKEN ROW by token row (round 5): one wave per row, so that the row statistics of the merged hidden state come with it --
// the slab form the folded LayerNorm of the 256 / 128-row GEMMs reads (stats1[m][4][2]: one slab (sum, sum of squares)) and / or the finalised form of the
// 256 x 256 kernel (fin[m] = (mean, rstd)) -- and the (x - mean) * rstd passes in front of attn2.to_q and the GEGLU projection disappear from the cached
// forward (2.2 ms of its 64 at 8 x 1024^2: profiles/r05_e_cache_breakdown.txt).  Statistics of the bf16 values as stored (what the pass read).
__global__ __launch_bounds__(256) void pc_rows_load_stats_kernel(bf16_t* batch, const bf16_t* __restrict__ state, const PcSample* __restrict__ samp, int level, int C,
                                                                 long state_row_elems, const bf16_t* residual, float* __restrict__ stats1, float* __restrict__ fin, float eps) {
  const PcSample s = samp[blockIdx.y];
  const int rows = (s.h >> level) * (s.w >> level);
  const long r0 = s.row0 >> (2 * level);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cv = C >> 3;                       // 16-byte vectors per row
  for (int r = blockIdx.x * 4 + wave; r < rows; r += gridDim.x * 4) {
    const u32x4* ps = reinterpret_cast<const u32x4*>(state + (long)s.slot * state_row_elems + (long)r * C);
    const u32x4* pr = reinterpret_cast<const u32x4*>(residual + (r0 + r) * C);
    u32x4* pb = reinterpret_cast<u32x4*>(batch + (r0 + r) * C);
    float a = 0.f, q = 0.f;
    for (int v = lane; v < cv; v += 64) {
      u32x4 x = ps[v];
      const u32x4 rr = pr[v];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned w = pack_bf16x2(bf16lo_to_f32(x[e]) + bf16lo_to_f32(rr[e]), bf16hi_to_f32(x[e]) + bf16hi_to_f32(rr[e]));
        const float lo = bf16lo_to_f32(w), hi = bf16hi_to_f32(w);
        a += lo + hi; q += lo * lo + hi * hi;
        x[e] = w;
      }
      pb[v] = x;
    }
    a = wave_sum(a); q = wave_sum(q);
    if (lane == 0) {
      const long m = r0 + r;
      if (stats1) *reinterpret_cast<f32x2*>(stats1 + m * 8) = f32x2{a, q};
      if (fin) {
        const float mean = a / (float)C;
        const float var = fmaxf(q / (float)C - mean * mean, 0.f);
        *reinterpret_cast<f32x2*>(fin + m * 2) = f32x2{mean, rsqrtf(var + eps)};
      }
    }
  }
}

// one block per (output pixel row of the halo'd patch, compact patch): P = p + halo_lo + halo_hi pixels of C channels
__global__ __launch_bounds__(256) void pc_gather_kernel(const bf16_t* __restrict__ src, int ld_src, int C, bf16_t* __restrict__ dst, const PcPatch* __restrict__ list,
                                                        const PcSample* __restrict__ samp, int level, int p, int halo_lo, int halo_hi, int up) {
  const PcPatch q = list[blockIdx.y];
  const PcSample s = samp[q.b];
  const int P = p + halo_lo + halo_hi;
  const int yy = blockIdx.x;
  // image at the gather's resolution (the upsampled one when up): h, w; the source tensor holds it at (h >> up, w >> up)
  const int h = (s.h >> level) << up, w = (s.w >> level) << up;
  const int ws = w >> up;
  const bf16_t* img = src + (s.row0 >> (2 * level)) * ld_src;
  bf16_t* out = dst + ((long)blockIdx.y * P + yy) * (long)P * C;
  const int y = yy - halo_lo;                         // row inside the patch: -1 .. p
  const int cv = C >> 3;
  for (int i = threadIdx.x; i < P * cv; i += 256) {
    const int xx = i / cv, c8 = i - xx * cv;
    const int x = xx - halo_lo;
    const bool yin = y >= 0 && y < p, xin = x >= 0 && x < p;
    int gy = q.py * p + y, gx = q.px * p + x;
    bool ok = true;
    if (!xin) {                                        // column halo and corners: the left / right neighbour's pixel of MY row range (corner replication)
      ok = gx >= 0 && gx < w;
      if (!yin) gy = q.py * p + (y < 0 ? 0 : p - 1);
    } else if (!yin) {
      ok = gy >= 0 && gy < h;
    }
    if (y < -1 || x < -1) ok = false;                 // halo_lo == 2: an outer ring of zeros in front of the halo (stride-2 convs, see unet_sdxl.cpp pc_conv)
    u32x4 v = {0u, 0u, 0u, 0u};
    if (ok) v = *reinterpret_cast<const u32x4*>(img + ((long)(gy >> up) * ws + (gx >> up)) * ld_src + c8 * 8);
    reinterpret_cast<u32x4*>(out)[i] = v;
  }
}

// compact [n][Ps][Ps][C] -> the p x p interior starting at (o0, o0) goes to the patch's place in its request's state row
__global__ __launch_bounds__(256) void pc_scatter_kernel(const bf16_t* __restrict__ src, int Ps, int o0, int C, bf16_t* __restrict__ state, long state_row_elems,
                                                         const PcPatch* __restrict__ list, const PcSample* __restrict__ samp, int level, int p) {
  const PcPatch q = list[blockIdx.y];
  const PcSample s = samp[q.b];
  const int w = s.w >> level;
  const int y = blockIdx.x;
  const bf16_t* in = src + (((long)blockIdx.y * Ps + (y + o0)) * Ps + o0) * (long)C;
  bf16_t* out = state + (long)s.slot * state_row_elems + ((long)(q.py * p + y) * w + q.px * p) * C;
  const int n = p * (C >> 3);
  for (int i = threadIdx.x; i < n; i += 256) reinterpret_cast<u32x4*>(out)[i] = reinterpret_cast<const u32x4*>(in)[i];
}

// the listed patches of a whole-image batch tensor -> their places in the requests' state rows (a conv that was cheaper to run on the whole
// images than on the compact halo'd patches still renews the asking patches only)
__global__ __launch_bounds__(256) void pc_patch_store_kernel(const bf16_t* __restrict__ batch, bf16_t* __restrict__ state, long state_row_elems, int C,
                                                             const PcPatch* __restrict__ list, const PcSample* __restrict__ samp, int level, int p) {
  const PcPatch q = list[blockIdx.y];
  const PcSample s = samp[q.b];
  const int w = s.w >> level;
  const long off = ((long)(q.py * p + blockIdx.x) * w + q.px * p) * C;
  const u32x4* in = reinterpret_cast<const u32x4*>(batch + (s.row0 >> (2 * level)) * C + off);
  u32x4* out = reinterpret_cast<u32x4*>(state + (long)s.slot * state_row_elems + off);
  const int n = p * (C >> 3);
  for (int i = threadIdx.x; i < n; i += 256) out[i] = in[i];
}

// partial[patch][row] = sum over the patch's pixel row of (x - cached)^2; the host adds the p partials of a patch
__global__ __launch_bounds__(256) void pc_patch_sq_diff_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ state, long state_row_elems, int C,
                                                               const PcPatch* __restrict__ list, const PcSample* __restrict__ samp, int level, int p,
                                                               double* __restrict__ partial) {
  const PcPatch q = list[blockIdx.y];
  const PcSample s = samp[q.b];
  const int w = s.w >> level;
  const long off = ((long)(q.py * p + blockIdx.x) * w + q.px * p) * C;
  const bf16_t* pa = x + (s.row0 >> (2 * level)) * C + off;
  const bf16_t* pb = state + (long)s.slot * state_row_elems + off;
  float acc = 0.f;
  const int n = p * (C >> 3);
  for (int i = threadIdx.x; i < n; i += 256) {
    const u32x4 a = reinterpret_cast<const u32x4*>(pa)[i], b = reinterpret_cast<const u32x4*>(pb)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d0 = bf16lo_to_f32(a[e]) - bf16lo_to_f32(b[e]), d1 = bf16hi_to_f32(a[e]) - bf16hi_to_f32(b[e]);
      acc += d0 * d0 + d1 * d1;
    }
  }
  __shared__ double red[4];
  double d = (double)acc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long)blockIdx.y * p + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// rows [row0, row0 + rows) of a token-major batch tensor <-> rows [srow0, srow0 + rows) of a request's state row (MMDiT: the chunks are token ranges)
__global__ __launch_bounds__(256) void pc_range_copy_kernel(bf16_t* __restrict__ batch, bf16_t* __restrict__ state, long state_row_elems, int C,
                                                            const PcRange* __restrict__ ranges, int to_batch) {
  const PcRange r = ranges[blockIdx.y];
  const long n = ((long)r.rows * C) >> 3;
  u32x4* pb = reinterpret_cast<u32x4*>(batch + r.row0 * C);
  u32x4* ps = reinterpret_cast<u32x4*>(state + (long)r.slot * state_row_elems + (long)r.srow0 * C);
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < n; v += (long)gridDim.x * 256) {
    if (to_batch) pb[v] = ps[v]; else ps[v] = pb[v];
  }
}
__global__ __launch_bounds__(256) void pc_range_sq_diff_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ state, long state_row_elems, int C,
                                                               const PcRange* __restrict__ ranges, double* __restrict__ partial) {
  const PcRange r = ranges[blockIdx.y];
  const long n = ((long)r.rows * C) >> 3;
  const long per = (n + 63) / 64, v0 = (long)blockIdx.x * per, v1 = v0 + per < n ? v0 + per : n;
  const u32x4* pa = reinterpret_cast<const u32x4*>(x + r.row0 * C);
  const u32x4* pb = reinterpret_cast<const u32x4*>(state + (long)r.slot * state_row_elems + (long)r.srow0 * C);
  float acc = 0.f;
  for (long v = v0 + threadIdx.x; v < v1; v += 256) {
    const u32x4 a = pa[v], b = pb[v];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d0 = bf16lo_to_f32(a[e]) - bf16lo_to_f32(b[e]), d1 = bf16hi_to_f32(a[e]) - bf16hi_to_f32(b[e]);
      acc += d0 * d0 + d1 * d1;
    }
  }
  __shared__ double red[4];
  double d = (double)acc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long)blockIdx.y * 64 + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
int launch_pc_range_copy(hipStream_t st, void* batch, void* state, long state_row_elems, int C, const void* ranges, int n, int to_batch, long max_range_elems) {
  MX_CHECK(C % 8 == 0 && n > 0, "pc_range_copy: bad shape");
  const int gx = (int)std::max<long>(1, std::min<long>((max_range_elems / 8 + 255) / 256, 128));
  hipLaunchKernelGGL(pc_range_copy_kernel, dim3(gx, n), dim3(256), 0, st, (bf16_t*)batch, (bf16_t*)state, state_row_elems, C, (const PcRange*)ranges, to_batch);
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_pc_range_sq_diff(hipStream_t st, const void* x, const void* state, long state_row_elems, int C, const void* ranges, int n, double* partial) {
  MX_CHECK(C % 8 == 0 && n > 0, "pc_range_sq_diff: bad shape");
  hipLaunchKernelGGL(pc_range_sq_diff_kernel, dim3(64, n), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)state, state_row_elems, C, (const PcRange*)ranges, partial);
  MX_LAUNCH_CHECK();
  return 0;
}

int launch_pc_image_copy(hipStream_t st, void* batch, void* state, const void* samp, int B, int level, int C, long state_row_elems, int to_batch,
                         const float* vec, int ldvec, const void* residual, long max_image_elems, int gate) {
  MX_CHECK(C % 8 == 0 && B > 0, "pc_image_copy: C must be a multiple of 8");
  const int gx = (int)std::max<long>(1, std::min<long>((max_image_elems / 8 + 255) / 256, 128));
  hipLaunchKernelGGL(pc_image_copy_kernel, dim3(gx, B), dim3(256), 0, st, (bf16_t*)batch, (bf16_t*)state, (const PcSample*)samp, level, C, state_row_elems,
                     to_batch, vec, ldvec, (const bf16_t*)residual, gate);
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_pc_rows_load_stats(hipStream_t st, void* batch, const void* state, const void* samp, int B, int level, int C, long state_row_elems, const void* residual,
                              float* stats1, float* fin, float eps, long max_image_rows) {
  MX_CHECK(C % 8 == 0 && B > 0 && residual != nullptr && (stats1 || fin), "pc_rows_load_stats: bad arguments");
  const int gx = (int)std::max<long>(1, std::min<long>((max_image_rows + 3) / 4, 256));
  hipLaunchKernelGGL(pc_rows_load_stats_kernel, dim3(gx, B), dim3(256), 0, st, (bf16_t*)batch, (const bf16_t*)state, (const PcSample*)samp, level, C, state_row_elems,
                     (const bf16_t*)residual, stats1, fin, eps);
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_pc_gather(hipStream_t st, const void* src, int ld_src, int C, void* dst, const void* list, int n, const void* samp, int level, int p, int halo_lo,
                     int halo_hi, int up) {
  MX_CHECK(C % 8 == 0 && ld_src % 8 == 0 && n > 0 && p > 0, "pc_gather: bad shape");
  hipLaunchKernelGGL(pc_gather_kernel, dim3(p + halo_lo + halo_hi, n), dim3(256), 0, st, (const bf16_t*)src, ld_src, C, (bf16_t*)dst, (const PcPatch*)list,
                     (const PcSample*)samp, level, p, halo_lo, halo_hi, up);
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_pc_scatter(hipStream_t st, const void* src, int Ps, int o0, int C, void* state, long state_row_elems, const void* list, int n, const void* samp,
                      int level, int p) {
  MX_CHECK(C % 8 == 0 && n > 0 && p > 0 && o0 >= 0 && o0 + p <= Ps, "pc_scatter: bad shape");
  hipLaunchKernelGGL(pc_scatter_kernel, dim3(p, n), dim3(256), 0, st, (const bf16_t*)src, Ps, o0, C, (bf16_t*)state, state_row_elems, (const PcPatch*)list,
                     (const PcSample*)samp, level, p);
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_pc_patch_store(hipStream_t st, const void* batch, void* state, long state_row_elems, int C, const void* list, int n, const void* samp, int level, int p) {
  MX_CHECK(C % 8 == 0 && n > 0 && p > 0, "pc_patch_store: bad shape");
  hipLaunchKernelGGL(pc_patch_store_kernel, dim3(p, n), dim3(256), 0, st, (const bf16_t*)batch, (bf16_t*)state, state_row_elems, C, (const PcPatch*)list,
                     (const PcSample*)samp, level, p);
  MX_LAUNCH_CHECK();
  return 0;
}
int launch_pc_patch_sq_diff(hipStream_t st, const void* x, const void* state, long state_row_elems, int C, const void* list, int n, const void* samp, int level,
                            int p, double* partial) {
  MX_CHECK(C % 8 == 0 && n > 0 && p > 0, "pc_patch_sq_diff: bad shape");
  hipLaunchKernelGGL(pc_patch_sq_diff_kernel, dim3(p, n), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)state, state_row_elems, C, (const PcPatch*)list,
                     (const PcSample*)samp, level, p, partial);
  MX_LAUNCH_CHECK();
  return 0;
}

// The decision of one block for all units (skip_decide.h states the rule; mx_skip_decide_host is the same loop on the host).  One workgroup:
// thread t takes unit j0 + t of each chunk of 256; the asking units are compacted in row order by a ballot per wave, the waves' totals in LDS
// and an offset carried from chunk to chunk.  Units arrive grouped by sample, so first[b] is written by the first unit of sample b.
constexpr int kDecideThreads = 256;
__global__ __launch_bounds__(kDecideThreads) void pc_decide_kernel(const mx_skip_decide_args a, const mx_device_forest f) {
  __shared__ float s_x[kDecideThreads][2 + MX_SKIP_MAX_IN];
  __shared__ int s_wave[kDecideThreads / 64];
  __shared__ int s_group[2 * MX_MAX_SEGS];
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PcPatch* patches = (const PcPatch*)a.units;
  const PcRange* ranges = (const PcRange*)a.units;
  const PcSample* samp = (const PcSample*)a.samples;
  if (tid < 2 * MX_MAX_SEGS) s_group[tid] = 0;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  auto sample_of = [&](int j) { return a.kind == 0 ? patches[j].b : a.unit_sample[j]; };
  int base = 0;                                            // asking units before this chunk (the same in every thread)
  for (int j0 = 0; j0 < a.n; j0 += kDecideThreads) {
    const int j = j0 + tid;
    int run = 0, b = 0, bad = 0;
    if (j < a.n) {
      b = sample_of(j);
      if (b < 0 || b >= a.n_samples) { b = 0; bad = 1; }
      int slot, u, rows = 1;
      if (a.kind == 0) { slot = samp[b].slot; u = patches[j].py * a.grid_w + patches[j].px; }
      else { slot = ranges[j].slot; rows = ranges[j].rows; u = rows > 0 ? ranges[j].srow0 / rows : -1; }
      float* x = s_x[tid];
      x[0] = (float)a.block; x[1] = a.timesteps[b];
      const bool valid = a.sample_valid[b] != 0;
      for (int i = 0; i < a.n_in; ++i) {
        if (!valid) x[2 + i] = MX_MSE_UNCACHED;            // nothing cached for this request: the marker
        else if (a.kind == 0) x[2 + i] = skip_finalise(a.partial + a.part_off[i] + (long)j * a.part_len[i], a.part_len[i], a.part_elems[i]);
        else x[2 + i] = skip_finalise(a.partial + (long)j * 64, 64, (double)rows * a.part_elems[0]);
      }
      const long ci = (long)slot * a.units_per_slot + u;
      const bool inside = slot >= 0 && u >= 0 && u < a.units_per_slot && ci < a.n_counters;
      int32_t next = 0;
      run = skip_unit(f, x, inside ? a.counters[ci] : 0, a.forced_after, &next, &bad);
      if (inside) a.counters[ci] = next; else bad = 1;
      a.run[j] = (unsigned char)run;
      if (a.sample_group) {
        const int g = a.sample_group[b];
        if (g >= 0 && g < MX_MAX_SEGS) { atomicAdd(&s_group[MX_MAX_SEGS + g], 1); if (run) atomicAdd(&s_group[g], 1); } else bad = 1;
      }
      if (bad) atomicOr(&s_bad, 1);
    }
    const unsigned long long asking = __ballot(run);
    if (lane == 0) s_wave[wave] = __popcll(asking);
    __syncthreads();
    int idx = base + __popcll(asking & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) idx += s_wave[w];
    if (j < a.n) {
      if (run) {
        if (a.ask_units) ((PcPatch*)a.ask_units)[idx] = patches[j];
        if (a.ask_index) a.ask_index[idx] = j;
      }
      if (j == 0 || sample_of(j - 1) != b) a.record[MX_SKIP_REC_FIRST + b] = idx;
    }
    for (int w = 0; w < kDecideThreads / 64; ++w) base += s_wave[w];
    __syncthreads();                                       // the next chunk rewrites s_wave
  }
  if (tid == 0) { a.record[MX_SKIP_REC_STATUS] = s_bad; a.record[MX_SKIP_REC_NASK] = base; a.record[MX_SKIP_REC_FIRST + a.n_samples] = base; }
  if (tid < 2 * MX_MAX_SEGS) a.record[MX_SKIP_REC_GASK + tid] = s_group[tid];
}

int launch_pc_decide(hipStream_t st, const mx_skip_decide_args& a) {
  MX_CHECK(a.forest && a.n > 0 && a.n_samples > 0 && a.n_in >= 1 && a.n_in <= MX_SKIP_MAX_IN && (a.kind == 0 || a.kind == 1), "pc_decide: bad shape");
  const mx_device_forest& f = *a.forest;
  MX_CHECK(f.left && f.right && f.feature && f.threshold && f.p1 && f.roots && f.n_trees > 0 && f.n_nodes > 0, "pc_decide: incomplete device forest");
  MX_CHECK(f.n_feat == 2 + a.n_in, "pc_decide: the forest's n_feat must be 2 + the inputs of the block");
  MX_CHECK(a.units && a.sample_valid && a.timesteps && a.partial && a.counters && a.run && a.record, "pc_decide: null operand");
  MX_CHECK(a.kind == 0 ? (a.samples != nullptr && a.grid_w > 0) : (a.unit_sample != nullptr && a.ask_units == nullptr && a.n_in == 1),
           "pc_decide: the tables of the unit kind are missing (token ranges: unit_sample, one input, no patch list)");
  MX_CHECK(a.units_per_slot > 0 && a.n_counters >= a.units_per_slot, "pc_decide: bad counter row");
  for (int i = 0; i < (a.kind == 0 ? a.n_in : 1); ++i)
    MX_CHECK(a.part_elems[i] > 0.0 && (a.kind == 1 || (a.part_len[i] > 0 && a.part_off[i] >= 0)), "pc_decide: bad partial-sum layout");
  hipLaunchKernelGGL(pc_decide_kernel, dim3(1), dim3(kDecideThreads), 0, st, a, f);
  MX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mx

extern "C" int mx_skip_decide_device(void* stream, const mx_skip_decide_args* args) {
  MX_CHECK(args != nullptr, "skip_decide_device: null arguments");
  return mx::launch_pc_decide((hipStream_t)stream, *args);
}

// ---- one launch each (include/mxdenoise.h: "Block-skip cache kernels, one launch each"): the launchers above on caller-made tables ----
extern "C" int mx_pc_image_copy(void* stream, void* batch, void* state, const mx_pc_sample* samples, int n_samples, int level, int C, int64_t state_row_elems,
                                int to_batch, const float* vec, int ldvec, const void* residual, int64_t max_image_elems, int gate) {
  MX_CHECK(batch && state && samples && level >= 0, "pc_image_copy: null operand");
  return mx::launch_pc_image_copy((hipStream_t)stream, batch, state, samples, n_samples, level, C, (long)state_row_elems, to_batch, vec, ldvec, residual,
                                  (long)max_image_elems, gate);
}
extern "C" int mx_pc_rows_load_stats(void* stream, void* batch, const void* state, const mx_pc_sample* samples, int n_samples, int level, int C,
                                     int64_t state_row_elems, const void* residual, float* stats1, float* fin, float eps, int64_t max_image_rows) {
  MX_CHECK(batch && state && samples && level >= 0, "pc_rows_load_stats: null operand");
  return mx::launch_pc_rows_load_stats((hipStream_t)stream, batch, state, samples, n_samples, level, C, (long)state_row_elems, residual, stats1, fin, eps,
                                       (long)max_image_rows);
}
extern "C" int mx_pc_gather(void* stream, const void* src, int ld_src, int C, void* dst, const mx_pc_patch* list, int n, const mx_pc_sample* samples, int level,
                            int p, int halo_lo, int halo_hi, int up) {
  MX_CHECK(src && dst && list && samples && level >= 0, "pc_gather: null operand");
  MX_CHECK(ld_src >= C && halo_lo >= 0 && halo_lo <= 2 && halo_hi >= 0 && halo_hi <= 1 && (up == 0 || up == 1), "pc_gather: bad halo or row stride");
  return mx::launch_pc_gather((hipStream_t)stream, src, ld_src, C, dst, list, n, samples, level, p, halo_lo, halo_hi, up);
}
extern "C" int mx_pc_scatter(void* stream, const void* src, int Ps, int o0, int C, void* state, int64_t state_row_elems, const mx_pc_patch* list, int n,
                             const mx_pc_sample* samples, int level, int p) {
  MX_CHECK(src && state && list && samples && level >= 0, "pc_scatter: null operand");
  return mx::launch_pc_scatter((hipStream_t)stream, src, Ps, o0, C, state, (long)state_row_elems, list, n, samples, level, p);
}
extern "C" int mx_pc_patch_store(void* stream, const void* batch, void* state, int64_t state_row_elems, int C, const mx_pc_patch* list, int n,
                                 const mx_pc_sample* samples, int level, int p) {
  MX_CHECK(batch && state && list && samples && level >= 0, "pc_patch_store: null operand");
  return mx::launch_pc_patch_store((hipStream_t)stream, batch, state, (long)state_row_elems, C, list, n, samples, level, p);
}
extern "C" int mx_pc_patch_sq_diff(void* stream, const void* x, const void* state, int64_t state_row_elems, int C, const mx_pc_patch* list, int n,
                                   const mx_pc_sample* samples, int level, int p, double* partial) {
  MX_CHECK(x && state && list && samples && partial && level >= 0, "pc_patch_sq_diff: null operand");
  return mx::launch_pc_patch_sq_diff((hipStream_t)stream, x, state, (long)state_row_elems, C, list, n, samples, level, p, partial);
}
extern "C" int mx_pc_range_copy(void* stream, void* batch, void* state, int64_t state_row_elems, int C, const mx_pc_range* ranges, int n, int to_batch,
                                int64_t max_range_elems) {
  MX_CHECK(batch && state && ranges, "pc_range_copy: null operand");
  return mx::launch_pc_range_copy((hipStream_t)stream, batch, state, (long)state_row_elems, C, ranges, n, to_batch, (long)max_range_elems);
}
extern "C" int mx_pc_range_sq_diff(void* stream, const void* x, const void* state, int64_t state_row_elems, int C, const mx_pc_range* ranges, int n,
                                   double* partial) {
  MX_CHECK(x && state && ranges && partial, "pc_range_sq_diff: null operand");
  return mx::launch_pc_range_sq_diff((hipStream_t)stream, x, state, (long)state_row_elems, C, ranges, n, partial);
}
