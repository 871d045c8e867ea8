// Inpainting only the masked region (gfx950): what a client-size photo needs around the request that repaints part of it -- diffusers'
// VaeImageProcessor.blur / get_crop_region / apply_overlay, which are Pillow calls on the host there.  Three byte kernels, all integer arithmetic, so
// each is bit-equal to Pillow:
//   the Gaussian blur of a mask (Pillow's three box passes along the rows, then three along the columns, each rounded to a byte on its own),
//   the bounding box of a mask's non-zero bytes (the crop rule itself is host arithmetic: inpaint_region.cpp),
//   the overlay: the client's image with the decoded crop blended in under the soft mask (Pillow's premultiplied paste + alpha_composite).
// Per request, off the step path.  HBM- / LDS-bound passes over bytes: dword accesses where the layout allows, bytes otherwise.
#include <algorithm>

#include "common.h"
#include "../../include/mxdenoise.h"

namespace mx {

// ---- blur ----

// One box pass over a line: out[x] = (ww * sum_{d=-r..r} in[clamp(x + d)] + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + 2^23) >> 24.
// The weights sum to 2^24 ((2r + 1) ww + 2 fw, mx_blur_box_params), so the accumulator stays below 255 * 2^24 + 2^23 < 2^32.
__device__ __forceinline__ unsigned box_round(unsigned sum, unsigned far, unsigned ww, unsigned fw) { return (ww * sum + fw * far + (1u << 23)) >> 24; }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

constexpr int kRowThreads = 256;

// The three row passes of `rows` lines of W bytes in one launch: a workgroup takes a line into LDS and runs the passes between two LDS buffers (each
// pass reads what the one before rounded to bytes).  A thread owns `seg` consecutive outputs of a pass: the window sum once (2r + 1 taps), then one tap
// in and one out per output.  seg is four times an odd number, so the threads' segments start on different LDS banks.
template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void box3_rows_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, long rows, int W, int pitch,
                                                                int seg, int r, unsigned ww, unsigned fw) {
  extern __shared__ unsigned char line[];                   // [2][pitch], pitch a multiple of 16
  const int tid = threadIdx.x;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned char* src_row = in + row * W;
    unsigned char* dst_row = out + row * W;
    if (VEC) {                                              // W % 4 == 0 and both bases 4-byte aligned: every row starts on a dword
      for (int i = tid; i < W / 4; i += kRowThreads) reinterpret_cast<unsigned*>(line)[i] = reinterpret_cast<const unsigned*>(src_row)[i];
    } else {
      for (int i = tid; i < W; i += kRowThreads) line[i] = src_row[i];
    }
    __syncthreads();
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
      const unsigned char* a = line + (pass & 1) * pitch;
      unsigned char* b = line + ((pass & 1) ^ 1) * pitch;
      for (int x0 = tid * seg; x0 < W; x0 += kRowThreads * seg) {
        const int x1 = min(x0 + seg, W);
        unsigned sum = 0;
        for (int d = -r; d <= r; ++d) sum += a[clampi(x0 + d, W - 1)];
        for (int x = x0; x < x1; ++x) {
          const unsigned lo = a[clampi(x - r - 1, W - 1)], hi = a[clampi(x + r + 1, W - 1)];
          b[x] = (unsigned char)box_round(sum, lo + hi, ww, fw);
          sum += hi - a[clampi(x - r, W - 1)];
        }
      }
      __syncthreads();
    }
    const unsigned char* res = line + pitch;                // pass 2 wrote buffer 1
    if (VEC) {
      for (int i = tid; i < W / 4; i += kRowThreads) reinterpret_cast<unsigned*>(dst_row)[i] = reinterpret_cast<const unsigned*>(res)[i];
    } else {
      for (int i = tid; i < W; i += kRowThreads) dst_row[i] = res[i];
    }
    // the next line's load writes buffer 0, which no thread reads any more; its pass 0 writes buffer 1 behind the barrier that follows that load
  }
}

constexpr int kColThreads = 64;     // small workgroups and short segments: a 1024^2 plane is 256 column groups x 64 segments, one wave each
constexpr int kColSeg = 16;

// One column pass of [B][H][W] through memory: a thread owns V adjacent columns and kColSeg consecutive rows of one plane; the lanes of a wave read
// adjacent bytes of one row.  V = 4: W % 4 == 0 and both bases 4-byte aligned (one dword per row); V = 1 otherwise.
template <int V>
__global__ __launch_bounds__(kColThreads) void box_cols_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int H, int W, int col_blocks,
                                                               int row_segs, int r, unsigned ww, unsigned fw) {
  long blk = blockIdx.x;                                    // over B * row_segs * col_blocks, columns fastest
  const int cb = (int)(blk % col_blocks);
  blk /= col_blocks;
  const int sg = (int)(blk % row_segs);
  const long plane = blk / row_segs;
  const int cx = (cb * kColThreads + (int)threadIdx.x) * V;
  if (cx >= W) return;
  const unsigned char* p = in + plane * H * W + cx;
  unsigned char* q = out + plane * H * W + cx;
  const int y0 = sg * kColSeg, y1 = min(y0 + kColSeg, H);
  unsigned sum[V];
#pragma unroll
  for (int i = 0; i < V; ++i) sum[i] = 0;
  auto load = [&](int y, unsigned (&v)[V]) {
    const unsigned char* s = p + (long)clampi(y, H - 1) * W;
    if (V == 4) {
      const unsigned w4 = *reinterpret_cast<const unsigned*>(s);
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = (w4 >> (8 * i)) & 0xffu;
    } else {
      v[0] = s[0];
    }
  };
  unsigned t[V], lo[V], hi[V];
#pragma unroll 4
  for (int d = -r; d <= r; ++d) {                           // (independent loads: several rows in flight)
    load(y0 + d, t);
#pragma unroll
    for (int i = 0; i < V; ++i) sum[i] += t[i];
  }
  for (int y = y0; y < y1; ++y) {
    load(y - r - 1, lo);
    load(y + r + 1, hi);
    load(y - r, t);
    unsigned o4 = 0;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      o4 |= box_round(sum[i], lo[i] + hi[i], ww, fw) << (8 * i);
      sum[i] += hi[i] - t[i];
    }
    if (V == 4) *reinterpret_cast<unsigned*>(q + (long)y * W) = o4;
    else q[(long)y * W] = (unsigned char)o4;
  }
}

// ---- bounding box ----

constexpr int kBoxThreads = 256;

__device__ __forceinline__ void bbox_take(int x, int y, int& x0, int& y0, int& x1, int& y1) {
  x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x + 1); y1 = max(y1, y + 1);
}

// box [B][4] must hold (0xffffffff, 0xffffffff, -1, -1) per plane on entry (the entry's memset): the mins are unsigned minima, the maxes signed maxima,
// and a plane's first workgroup contributes at least the empty box (W, H, 0, 0), so the record ends as the box whatever the order of the atomics.
// `groups` workgroups per plane stride over the plane as a flat run of bytes; V = 16: every plane starts 16-byte aligned and holds whole 16-byte chunks.
template <int V>
__global__ __launch_bounds__(kBoxThreads) void mask_bbox_kernel(const unsigned char* __restrict__ mask, int* __restrict__ box, int H, int W, int groups) {
  const long plane = blockIdx.x / groups;
  const int g = blockIdx.x % groups;
  const long P = (long)H * W;
  const unsigned char* m = mask + plane * P;
  int x0 = W, y0 = H, x1 = 0, y1 = 0;
  const long chunks = (P + V - 1) / V;
  for (long c = (long)g * kBoxThreads + threadIdx.x; c < chunks; c += (long)groups * kBoxThreads) {
    const long at = c * V;
    if (V == 16) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(m + at);
      if ((w[0] | w[1] | w[2] | w[3]) == 0u) continue;
      int y = P <= 0xffffffffL ? (int)((unsigned)at / (unsigned)W) : (int)(at / W);
      int x = (int)(at - (long)y * W);
      if (x + 15 < W) {                                     // the chunk lies in one row: its first and its last non-zero byte decide
        int first = 0, last = 0;
#pragma unroll
        for (int j = 3; j >= 0; --j)
          if (w[j]) first = 4 * j + (__builtin_ctz(w[j]) >> 3);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (w[j]) last = 4 * j + ((31 - __builtin_clz(w[j])) >> 3);
        bbox_take(x + first, y, x0, y0, x1, y1);
        bbox_take(x + last, y, x0, y0, x1, y1);
        continue;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if ((w[i >> 2] >> (8 * (i & 3))) & 0xffu) bbox_take(x, y, x0, y0, x1, y1);
        if (++x == W) { x = 0; ++y; }
      }
    } else {
      if (m[at]) { const int y = (int)(at / W); bbox_take((int)(at - (long)y * W), y, x0, y0, x1, y1); }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
    x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
  }
  __shared__ int part[kBoxThreads / kWave][4];
  const int wave = threadIdx.x / kWave;
  if (threadIdx.x % kWave == 0) { part[wave][0] = x0; part[wave][1] = y0; part[wave][2] = x1; part[wave][3] = y1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBoxThreads / kWave; ++w) {
      x0 = min(x0, part[w][0]); y0 = min(y0, part[w][1]); x1 = max(x1, part[w][2]); y1 = max(y1, part[w][3]);
    }
    if (g != 0 && x1 == 0) return;                          // nothing found here: the plane's first workgroup contributes the empty box
    int* rec = box + plane * 4;
    atomicMin(reinterpret_cast<unsigned*>(rec), (unsigned)x0);
    atomicMin(reinterpret_cast<unsigned*>(rec + 1), (unsigned)y0);
    atomicMax(rec + 2, x1);
    atomicMax(rec + 3, y1);
  }
}

// ---- overlay ----

// One channel of diffusers' apply_overlay on bytes: Pillow's paste of the premultiplied original under the inverted mask A = 255 - m (the
// MULDIV255 of o A, then the un-premultiplication 255 p / A clipped), then alpha_composite with the decoded pixel under it.  A = 0: the decoded byte;
// A = 255: the chain returns o itself (p = o, c = o, and the blend of o with weight 255 * 128 of 255 * 128).
__device__ __forceinline__ unsigned overlay_byte(unsigned d, unsigned o, unsigned A) {
  if (A == 0u) return d;
  const unsigned t = o * A + 128u;
  const unsigned p = ((t >> 8) + t) >> 8;
  const unsigned c = min(255u, (255u * p) / A);
  const unsigned u = c * (A * 128u) + d * (255u * 128u - A * 128u) + (0x80u << 7);
  return (((u >> 8) + u) >> 8) >> 7;
}

struct overlay_box { int x, y, w, h; };

// out [B][H][W][3] = orig outside the box, the blend inside.  One thread per four pixels of the flat pixel run: three dwords of orig / out and one of
// the mask (VEC: the three bases 4-byte aligned); the pixels past the last whole four, and every pixel of a misaligned image, byte by byte.  The
// decoded crop is read by bytes: its rows start anywhere relative to the client's.
template <bool VEC>
__global__ void rgb8_overlay_kernel(const unsigned char* __restrict__ dec, const unsigned char* __restrict__ orig, const unsigned char* __restrict__ mask,
                                    unsigned char* __restrict__ out, int H, int W, overlay_box bx, long P) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long p0 = idx * 4;
  if (p0 >= P) return;
  const int n = (int)min(4L, P - p0);
  long row = p0 / W;                                        // over B * H
  int x = (int)(p0 - row * W);
  unsigned o3[3], m4 = 0;
  unsigned char* ob = reinterpret_cast<unsigned char*>(o3);
  const bool whole = VEC && n == 4;
  if (whole) {
    const unsigned* o = reinterpret_cast<const unsigned*>(orig + p0 * 3);
    o3[0] = o[0]; o3[1] = o[1]; o3[2] = o[2];
    m4 = *reinterpret_cast<const unsigned*>(mask + p0);
  } else {
    for (int i = 0; i < 3 * n; ++i) ob[i] = orig[p0 * 3 + i];
    for (int i = 0; i < n; ++i) m4 |= (unsigned)mask[p0 + i] << (8 * i);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < n) {
      const long b = row / H;
      const int y = (int)(row - b * H);
      const unsigned A = 255u - ((m4 >> (8 * q)) & 0xffu);
      if (A != 255u && x >= bx.x && x < bx.x + bx.w && y >= bx.y && y < bx.y + bx.h) {
        const unsigned char* d = dec + ((b * bx.h + (y - bx.y)) * bx.w + (x - bx.x)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) ob[3 * q + c] = (unsigned char)overlay_byte(d[c], ob[3 * q + c], A);
      }
      if (++x == W) { x = 0; ++row; }
    }
  }
  if (whole) {
    unsigned* o = reinterpret_cast<unsigned*>(out + p0 * 3);
    o[0] = o3[0]; o[1] = o3[1]; o[2] = o3[2];
  } else {
    for (int i = 0; i < 3 * n; ++i) out[p0 * 3 + i] = ob[i];
  }
}

static bool aligned4(const void* p) { return ((uintptr_t)p % 4) == 0; }
static bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uint64_t)nb && y < x + (uint64_t)na;
}

}  // namespace mx

extern "C" int mx_gaussian_blur_u8(void* stream, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, float radius) {
  MX_CHECK(src && dst, "gaussian_blur_u8: null operand");
  MX_CHECK(B > 0 && H > 0 && W > 0, "gaussian_blur_u8: sizes must be positive");
  MX_CHECK(W <= MX_BLUR_MAX_WIDTH, "gaussian_blur_u8: a row is wider than MX_BLUR_MAX_WIDTH");
  MX_CHECK(radius == radius && radius <= (float)MX_BLUR_MAX_RADIUS, "gaussian_blur_u8: the radius must be a number, at most MX_BLUR_MAX_RADIUS");
  const int64_t n = (int64_t)B * H * W;
  MX_CHECK(!mx::overlap(src, n, dst, n), "gaussian_blur_u8: dst may not alias src");
  hipStream_t s = (hipStream_t)stream;
  if (radius <= 0.0f) {                                     // Pillow: no pass at radius 0; the output is the input's bytes
    MX_HIP(hipMemcpyAsync(dst, src, (size_t)n, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  MX_CHECK(scratch, "gaussian_blur_u8: null scratch (B * H * W bytes) for a positive radius");
  MX_CHECK(!mx::overlap(scratch, n, dst, n) && !mx::overlap(scratch, n, src, n), "gaussian_blur_u8: scratch may alias neither src nor dst");
  int r = 0;
  uint32_t ww = 0, fw = 0;
  if (mx_blur_box_params(radius, &r, &ww, &fw)) return 1;
  // rows: src -> scratch (three passes in LDS); columns: scratch -> dst -> scratch -> dst
  {
    const int64_t rows = (int64_t)B * H;
    int k = mx::cdiv(mx::cdiv(W, mx::kRowThreads), 4);
    if (k % 2 == 0) ++k;
    const int seg = 4 * k, pitch = mx::cdiv(W, 16) * 16;
    const bool vec = W % 4 == 0 && mx::aligned4(src) && mx::aligned4(scratch);
    dim3 grid((unsigned)std::min<int64_t>(rows, 8 * (int64_t)mx::cu_count())), block(mx::kRowThreads);
    if (vec) hipLaunchKernelGGL((mx::box3_rows_kernel<true>), grid, block, 2 * (size_t)pitch, s, src, scratch, (long)rows, W, pitch, seg, r, ww, fw);
    else hipLaunchKernelGGL((mx::box3_rows_kernel<false>), grid, block, 2 * (size_t)pitch, s, src, scratch, (long)rows, W, pitch, seg, r, ww, fw);
    MX_LAUNCH_CHECK();
  }
  const bool vec = W % 4 == 0 && mx::aligned4(dst) && mx::aligned4(scratch);
  const int V = vec ? 4 : 1;
  const int col_blocks = mx::cdiv(W / V, mx::kColThreads), row_segs = mx::cdiv(H, mx::kColSeg);
  const int64_t blocks = (int64_t)B * row_segs * col_blocks;
  MX_CHECK(blocks <= 0x7fffffffL, "gaussian_blur_u8: too many tiles for one launch");
  const uint8_t* from = scratch;
  uint8_t* to = dst;
  for (int pass = 0; pass < 3; ++pass) {
    if (vec) hipLaunchKernelGGL((mx::box_cols_kernel<4>), dim3((unsigned)blocks), dim3(mx::kColThreads), 0, s, from, to, H, W, col_blocks, row_segs, r, ww, fw);
    else hipLaunchKernelGGL((mx::box_cols_kernel<1>), dim3((unsigned)blocks), dim3(mx::kColThreads), 0, s, from, to, H, W, col_blocks, row_segs, r, ww, fw);
    MX_LAUNCH_CHECK();
    const uint8_t* was = from;
    from = to;
    to = const_cast<uint8_t*>(was);
  }
  return 0;
}

extern "C" int mx_mask_bbox_u8(void* stream, const uint8_t* mask, int32_t* box, int B, int H, int W) {
  MX_CHECK(mask && box, "mask_bbox_u8: null operand");
  MX_CHECK(B > 0 && H > 0 && W > 0, "mask_bbox_u8: sizes must be positive");
  MX_CHECK(((uintptr_t)box % 4) == 0, "mask_bbox_u8: the box record must be 4-byte aligned");
  const int64_t P = (int64_t)H * W;
  const bool vec = ((uintptr_t)mask % 16) == 0 && P % 16 == 0;
  const int64_t chunks = vec ? P / 16 : P;
  // few workgroups a plane: each ends in four atomics on the plane's one record, and those serialise (about 12 ns each)
  const int groups = (int)std::min<int64_t>(mx::cdiv64(chunks, 4 * mx::kBoxThreads), 128);
  const int64_t blocks = (int64_t)B * groups;
  MX_CHECK(blocks <= 0x7fffffffL, "mask_bbox_u8: too many planes for one launch");
  hipStream_t s = (hipStream_t)stream;
  MX_HIP(hipMemsetAsync(box, 0xff, (size_t)B * 4 * sizeof(int32_t), s));       // the identity of the unsigned minima and of the signed maxima
  if (vec) hipLaunchKernelGGL((mx::mask_bbox_kernel<16>), dim3((unsigned)blocks), dim3(mx::kBoxThreads), 0, s, mask, box, H, W, groups);
  else hipLaunchKernelGGL((mx::mask_bbox_kernel<1>), dim3((unsigned)blocks), dim3(mx::kBoxThreads), 0, s, mask, box, H, W, groups);
  MX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mx_rgb8_overlay(void* stream, const uint8_t* decoded, const uint8_t* original, const uint8_t* mask, uint8_t* out, int B, int H, int W, int x,
                               int y, int w, int h) {
  MX_CHECK(decoded && original && mask && out, "rgb8_overlay: null operand");
  MX_CHECK(B > 0 && H > 0 && W > 0 && w > 0 && h > 0, "rgb8_overlay: sizes must be positive");
  MX_CHECK(x >= 0 && y >= 0 && (int64_t)x + w <= W && (int64_t)y + h <= H, "rgb8_overlay: the box must lie inside the image");
  const int64_t P = (int64_t)B * H * W;
  MX_CHECK(!mx::overlap(out, 3 * P, original, 3 * P) && !mx::overlap(out, 3 * P, mask, P) && !mx::overlap(out, 3 * P, decoded, 3 * (int64_t)B * h * w),
           "rgb8_overlay: out may not alias an input");
  const int64_t blocks = mx::cdiv64(mx::cdiv64(P, 4), 256);
  MX_CHECK(blocks <= 0x7fffffffL, "rgb8_overlay: too many pixels for one launch");
  const bool vec = mx::aligned4(original) && mx::aligned4(mask) && mx::aligned4(out);
  const mx::overlay_box bx = {x, y, w, h};
  dim3 grid((unsigned)blocks), block(256);
  if (vec) hipLaunchKernelGGL((mx::rgb8_overlay_kernel<true>), grid, block, 0, (hipStream_t)stream, decoded, original, mask, out, H, W, bx, (long)P);
  else hipLaunchKernelGGL((mx::rgb8_overlay_kernel<false>), grid, block, 0, (hipStream_t)stream, decoded, original, mask, out, H, W, bx, (long)P);
  MX_LAUNCH_CHECK();
  return 0;
}
