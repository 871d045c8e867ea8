// Resize of a client's 8-bit image or mask (gfx950), bit-equal to Pillow's Image.resize: diffusers' VaeImageProcessor.preprocess resizes with it in
// front of the VAE encoder, the inpainting pipelines' mask processor in front of the binarisation.  Pillow's 8-bit resampler is integer arithmetic
// on integer coefficient tables (include/mxdenoise.h states the rule); the tables come from the host (resize_coeffs.cpp), the device only
// multiplies, adds, shifts and clips.  Horizontal pass into bytes, vertical pass over those bytes -- both in ONE launch:
//   a workgroup owns kRzTileRows output rows x `ew` bytes of them (bytes, not pixels: channels are independent, so a tile may start inside a pixel);
//   it walks the input rows its vertical taps cover in chunks of `rows`; per chunk it stages the input row segments its horizontal taps cover in
//   LDS (whole dwords from HBM), filters them horizontally into a byte patch in LDS and adds the patch's rows, times their vertical coefficients,
//   into int32 accumulators in registers; after the last chunk it clips and stores (a dword where the four bytes lie on a 4-byte boundary, bytes
//   otherwise).
// The chunk loop bounds the LDS footprint for any vertical scale (a 16x downscale has 97 taps per axis), and the intermediate never sees HBM.
// Every product is a byte times a coefficient below 2^23 in magnitude (mx_resize_create refuses a table that is not): the full-rate 24-bit multiply.
// The launch is bound by vector instruction issue, not by memory (profiles/image_resize_mi355x.txt), so the loops are written for few instructions.
// Horizontal pass: lane = one output byte, adjacent lanes adjacent bytes of a patch row.  Vertical pass: lane = four adjacent bytes of two output
// rows, so one patch dword and one coefficient serve four products, and the results leave from registers.  The staged rows' pitch is an odd number
// of dwords so that the rows of a chunk start on different banks.
#include <vector>

#include "common.h"
#include "../../include/mxdenoise.h"

namespace mx {

constexpr int kRzThreads = 256;
constexpr int kRzTileBytes = 128;     // output bytes of a row per tile, at most: one lane per byte, two row groups of lanes
constexpr int kRzTileRows = 16;       // output rows per tile: a lane of the vertical pass owns four bytes of two of them
constexpr int kRzChunkRows = 16;      // input rows per chunk, at most
constexpr int kRzPatchBytes = kRzChunkRows * kRzTileBytes;
constexpr int kRzLdsBytes = 65536;    // what one workgroup may take: the patch, the tile's coefficients where they fit, the staged rows
constexpr int kRzHkLdsBytes = 16384;  // a tile's horizontal / vertical coefficients go to LDS up to these sizes, and are read from memory above them
constexpr int kRzVkLdsBytes = 12288;

// tile width in output bytes (multiple of 4), input rows per chunk, bytes of a staged row (multiple of 4), the most output columns a tile touches,
// whether the tile's coefficients are copied to LDS, and the LDS bytes of a workgroup
struct rz_tile { int ew, rows, pitch, pxw, hk_lds, vk_lds, lds_bytes; };

struct rz_args {
  const uint8_t* src; uint8_t* dst;
  const int2* hb; const int* hk;      // horizontal: (xmin, n) per output column; coefficients [ksize_h][out_w] (tap-major: adjacent lanes, adjacent words)
  const int2* vb; const int* vk;      // vertical:   (ymin, n) per output row;    coefficients [ksize_v][out_h]
  int in_h, in_w, out_h, out_w, ksize_h, ksize_v;
  rz_tile t;
  size_t src_bytes;
};

__device__ __forceinline__ int rz_clip8(int s) { return min(max((s + (1 << (MX_RESIZE_PRECISION_BITS - 1))) >> MX_RESIZE_PRECISION_BITS, 0), 255); }

// the aligned dword at p; a dword that is not wholly inside [lo, hi) is put together from its bytes that are
__device__ __forceinline__ unsigned rz_load_dword(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const unsigned*>(p);
  unsigned v = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (p + i >= lo && p + i < hi) v |= (unsigned)p[i] << (8 * i);
  return v;
}

// C: channels (a constant, so the taps of an unrolled group differ by immediate offsets).  HK_LDS / VK_LDS: the tile's horizontal / vertical
// coefficients were copied to LDS (from memory every tap would wait a cache round trip); tables too large for that (very steep downscales) are
// read where they lie.
template <int C, bool HK_LDS, bool VK_LDS>
__global__ __launch_bounds__(kRzThreads) void resize_u8_kernel(const rz_args a) {
  extern __shared__ unsigned rz_lds[];
  unsigned* hp_s = rz_lds;                                        // the horizontally filtered chunk [kRzChunkRows][kRzTileBytes]
  int* vk_s = reinterpret_cast<int*>(hp_s + kRzPatchBytes / 4);   // [ksize_v][kRzTileRows]
  int* hk_s = vk_s + (VK_LDS ? a.ksize_v * kRzTileRows : 0);      // [ksize_h][pxw]
  unsigned* in_s = reinterpret_cast<unsigned*>(hk_s + (HK_LDS ? a.ksize_h * a.t.pxw : 0));   // the staged input rows [rows][pitch]
  const uint8_t* in_b = reinterpret_cast<const uint8_t*>(in_s);
  uint8_t* hp_b = reinterpret_cast<uint8_t*>(hp_s);

  const int tid = threadIdx.x;
  const int e = tid & (kRzTileBytes - 1);
  const int rg = __builtin_amdgcn_readfirstlane(tid / kRzTileBytes);     // row group 0 / 1: wave-uniform
  const int row_out = a.out_w * C;
  const size_t row_in = (size_t)a.in_w * C;
  const int e0 = blockIdx.x * a.t.ew;
  const int ew = min(a.t.ew, row_out - e0);
  const int y0 = blockIdx.y * kRzTileRows;
  const int th = min(kRzTileRows, a.out_h - y0);
  const int pitch = a.t.pitch, pxw = a.t.pxw;

  // the input columns this tile's horizontal taps cover (xmin and xmin + n never decrease along the axis)
  const int xf = e0 / C, xl = (e0 + ew - 1) / C;
  const int2 bf = a.hb[xf], bl = a.hb[xl];
  const int seg_lo = bf.x * C;
  const int seg_len = (bl.x + bl.y) * C - seg_lo;
  const int ndw = (seg_len + 3 + 3) / 4;                          // dwords that hold a segment at any misalignment; ndw * 4 <= pitch (rz_plan_tile)
  int hx = 0, hn = 0, hpos = 0;                                   // this lane's output byte: its column, tap count, first tap's offset in the segment
  if (e < ew) {
    hx = (e0 + e) / C;
    const int2 hb = a.hb[hx];
    hn = hb.y;
    hpos = hb.x * C + (e0 + e - hx * C) - seg_lo;
  }
  // vertical pass: lane = output bytes 4 q .. 4 q + 3 of rows 2 g, 2 g + 1 of the tile
  const int q = tid & (kRzTileBytes / 4 - 1), g = tid / (kRzTileBytes / 4);
  const bool vact = 4 * q < ew;
  int acc[2][4], ymin[2], yn[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    int2 vb = make_int2(0, 0);
    if (vact && 2 * g + r < th) vb = a.vb[y0 + 2 * g + r];
    ymin[r] = vb.x; yn[r] = vb.y;
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[r][b] = 0;
  }
  const int2 vf = a.vb[y0], vl = a.vb[y0 + th - 1];
  const int r_lo = vf.x, r_hi = vl.x + vl.y;                      // the input rows the tile's vertical taps cover
  // the tile's coefficients (visible after the first chunk's barrier); xl - xf + 1 <= pxw
  if (HK_LDS) {
    const int npx = xl - xf + 1;
    for (int it = tid; it < a.ksize_h * npx; it += kRzThreads) {
      const int j = it / npx, p = it - j * npx;
      hk_s[j * pxw + p] = a.hk[(size_t)j * a.out_w + xf + p];
    }
  }
  if (VK_LDS) {
    for (int it = tid; it < a.ksize_v * kRzTileRows; it += kRzThreads) {
      const int j = it / kRzTileRows, i = it % kRzTileRows;
      vk_s[it] = i < th ? a.vk[(size_t)j * a.out_h + y0 + i] : 0;
    }
  }
  const int* hk = HK_LDS ? hk_s + (hx - xf) : a.hk + hx;          // this lane's column of the horizontal coefficients, and the step from tap to tap
  const int hk_step = HK_LDS ? pxw : a.out_w;

  const uint8_t* img = a.src + (size_t)blockIdx.z * a.in_h * row_in;
  const uint8_t* lo = a.src;
  const uint8_t* hi = a.src + a.src_bytes;
  for (int r0 = r_lo; r0 < r_hi; r0 += a.t.rows) {
    const int nr = min(a.t.rows, r_hi - r0);
    // stage rows [r0, r0 + nr): bytes [seg_lo, seg_lo + seg_len) of each, from the aligned dword at or below the first one.  A wave takes every
    // fourth row, its lanes the dwords of a row; four rows' loads are in flight before the first LDS write.
    {
      const int wave = tid / kWave, lane = tid % kWave;
      for (int rr0 = wave; rr0 < nr; rr0 += 16) {
        for (int dq = lane; dq < ndw; dq += kWave) {
          unsigned v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int rr = rr0 + 4 * u;
            v[u] = 0;
            if (rr < nr) {
              const uint8_t* p = img + (size_t)(r0 + rr) * row_in + seg_lo;
              v[u] = rz_load_dword(p - ((uintptr_t)p & 3) + 4 * dq, lo, hi);
            }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (rr0 + 4 * u < nr) in_s[(rr0 + 4 * u) * (pitch / 4) + dq] = v[u];
        }
      }
    }
    __syncthreads();
    // horizontal: rows rg * 8 .. + 7 of the chunk, four at a time under one coefficient read; a row index past the chunk repeats its last row
    // (never read by the vertical pass), so every LDS address stays inside the staged rows
    if (e < ew) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int rb = rg * 8 + half * 4;
        if (rb >= nr) break;
        int tap[4];                                               // byte offset of the first tap in the staged rows
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rr = min(rb + i, nr - 1);
          const uintptr_t p = (uintptr_t)(img + (size_t)(r0 + rr) * row_in + seg_lo);
          tap[i] = rr * pitch + (int)(p & 3) + hpos;
        }
        int s[4] = {0, 0, 0, 0};
#pragma unroll 4
        for (int j = 0; j < hn; ++j) {
          const int k = hk[(size_t)j * hk_step];
#pragma unroll
          for (int i = 0; i < 4; ++i) s[i] += __mul24((int)in_b[tap[i] + j * C], k);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) hp_b[(rb + i) * kRzTileBytes + e] = (uint8_t)rz_clip8(s[i]);
      }
    }
    __syncthreads();
    // vertical: the taps of each of this lane's two output rows that fall into the chunk; tap j reads patch row ymin + j - r0, in [0, nr)
    if (vact) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int jlo = max(0, r0 - ymin[r]), jhi = min(yn[r], r0 + nr - ymin[r]);
        const int col = (ymin[r] - r0) * (kRzTileBytes / 4) + q;
#pragma unroll 4
        for (int j = jlo; j < jhi; ++j) {
          const int k = VK_LDS ? vk_s[j * kRzTileRows + 2 * g + r] : a.vk[(size_t)j * a.out_h + y0 + 2 * g + r];
          const unsigned d = hp_s[col + j * (kRzTileBytes / 4)];
          acc[r][0] += __mul24((int)(d & 0xffu), k); acc[r][1] += __mul24((int)((d >> 8) & 0xffu), k);
          acc[r][2] += __mul24((int)((d >> 16) & 0xffu), k); acc[r][3] += __mul24((int)(d >> 24), k);
        }
      }
    }
  }
  if (vact) {
    const int cnt = min(4, ew - 4 * q);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (2 * g + r >= th) continue;
      uint8_t* d = a.dst + ((size_t)blockIdx.z * a.out_h + y0 + 2 * g + r) * row_out + e0 + 4 * q;
      if (cnt == 4 && ((uintptr_t)d & 3) == 0)
        *reinterpret_cast<unsigned*>(d) = (unsigned)rz_clip8(acc[r][0]) | ((unsigned)rz_clip8(acc[r][1]) << 8) | ((unsigned)rz_clip8(acc[r][2]) << 16) |
                                          ((unsigned)rz_clip8(acc[r][3]) << 24);
      else
        for (int b = 0; b < cnt; ++b) d[b] = (uint8_t)rz_clip8(acc[r][b]);
    }
  }
}

}  // namespace mx

struct mx_resize {
  int in_h, in_w, out_h, out_w, filter;
  int ksize_h, ksize_v;
  void* tables;                       // one device allocation: hb, vb, hk, vk
  const int2 *hb, *vb;
  const int *hk, *vk;
  mx::rz_tile tile[2];                // for C = 1 and C = 3
};

namespace mx {

// One axis as the kernel reads it: bounds as they are, coefficients tap-major [ksize][out].  An axis whose sizes agree is skipped by Pillow; here it
// gets the identity table (one tap of 2^22: ((1 << 21) + v * 2^22) >> 22 == v), which keeps one kernel for every case.
static int rz_axis(int in, int out, int filter, std::vector<int32_t>& bounds, std::vector<int32_t>& kt) {
  if (in == out) {
    bounds.resize((size_t)out * 2);
    kt.assign((size_t)out, 1 << MX_RESIZE_PRECISION_BITS);
    for (int x = 0; x < out; ++x) { bounds[2 * x] = x; bounds[2 * x + 1] = 1; }
    return 1;
  }
  const int ksize = mx_resize_coeffs(in, out, filter, nullptr, nullptr, 0);
  if (ksize <= 0) return -1;
  if ((int64_t)out * ksize > 0x7fffffffLL) { set_error("resize_create: the coefficient table is too large"); return -1; }
  std::vector<int32_t> k((size_t)out * ksize);
  bounds.resize((size_t)out * 2);
  if (mx_resize_coeffs(in, out, filter, bounds.data(), k.data(), out * ksize) != ksize) return -1;
  for (int32_t v : k)
    if (v >= (1 << 23) || v <= -(1 << 23)) { set_error("resize_create: a coefficient does not fit 24 bits"); return -1; }   // (none known: the largest seen is 1.29 * 2^22)
  kt.resize((size_t)out * ksize);
  for (int x = 0; x < out; ++x)
    for (int j = 0; j < ksize; ++j) kt[(size_t)j * out + x] = k[(size_t)x * ksize + j];
  return ksize;
}

// The widest staged segment and the most output columns over all column tiles of width ew, and from them the tile shape whose LDS fits.
static bool rz_plan_tile(const std::vector<int32_t>& hb, int out_w, int C, int ksize_h, int ksize_v, rz_tile* t) {
  const int row_out = out_w * C;
  int rows = kRzChunkRows, ew = kRzTileBytes;
  for (;;) {
    int64_t seg_max = 0, pxw = 0;
    for (int e0 = 0; e0 < row_out; e0 += ew) {
      const int xf = e0 / C, xl = (std::min(e0 + ew, row_out) - 1) / C;
      seg_max = std::max(seg_max, ((int64_t)hb[2 * xl] + hb[2 * xl + 1] - hb[2 * xf]) * C);
      pxw = std::max<int64_t>(pxw, xl - xf + 1);
    }
    int64_t pitch = (seg_max + 3 + 3) / 4 * 4;              // any misalignment of the first byte, whole dwords
    if ((pitch / 4) % 2 == 0) pitch += 4;                   // odd in dwords: the rows of a chunk start on different banks
    const int64_t hk_bytes = pxw * ksize_h * 4, vk_bytes = (int64_t)kRzTileRows * ksize_v * 4;
    const bool hk_lds = hk_bytes <= kRzHkLdsBytes, vk_lds = vk_bytes <= kRzVkLdsBytes;
    const int64_t total = kRzPatchBytes + (hk_lds ? hk_bytes : 0) + (vk_lds ? vk_bytes : 0) + pitch * rows;
    if (total <= kRzLdsBytes) {
      t->ew = ew; t->rows = rows; t->pitch = (int)pitch; t->pxw = (int)pxw; t->hk_lds = hk_lds; t->vk_lds = vk_lds; t->lds_bytes = (int)total;
      return true;
    }
    if (rows > 4) rows /= 2;
    else if (ew > 4) ew /= 2;
    else if (rows > 1) rows /= 2;
    else return false;
  }
}

template <int C>
static void rz_launch(const rz_tile& t, dim3 grid, hipStream_t s, const rz_args& a) {
  const dim3 block(kRzThreads);
  if (t.hk_lds && t.vk_lds) hipLaunchKernelGGL((resize_u8_kernel<C, true, true>), grid, block, t.lds_bytes, s, a);
  else if (t.hk_lds) hipLaunchKernelGGL((resize_u8_kernel<C, true, false>), grid, block, t.lds_bytes, s, a);
  else if (t.vk_lds) hipLaunchKernelGGL((resize_u8_kernel<C, false, true>), grid, block, t.lds_bytes, s, a);
  else hipLaunchKernelGGL((resize_u8_kernel<C, false, false>), grid, block, t.lds_bytes, s, a);
}

}  // namespace mx

extern "C" mx_resize* mx_resize_create(int in_h, int in_w, int out_h, int out_w, int filter) {
  if (in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) { mx::set_error("resize_create: sizes must be positive"); return nullptr; }
  if (in_h > MX_RESIZE_MAX_SIZE || in_w > MX_RESIZE_MAX_SIZE || out_h > MX_RESIZE_MAX_SIZE || out_w > MX_RESIZE_MAX_SIZE) {
    mx::set_error("resize_create: sizes above 2^24 are not served");
    return nullptr;
  }
  if (filter != MX_RESIZE_LANCZOS && filter != MX_RESIZE_BILINEAR && filter != MX_RESIZE_BICUBIC) { mx::set_error("resize_create: unknown filter"); return nullptr; }
  std::vector<int32_t> hb, hk, vb, vk;
  const int ksh = mx::rz_axis(in_w, out_w, filter, hb, hk);
  if (ksh <= 0) return nullptr;
  const int ksv = mx::rz_axis(in_h, out_h, filter, vb, vk);
  if (ksv <= 0) return nullptr;
  mx_resize* r = new mx_resize();
  r->in_h = in_h; r->in_w = in_w; r->out_h = out_h; r->out_w = out_w; r->filter = filter; r->ksize_h = ksh; r->ksize_v = ksv; r->tables = nullptr;
  for (int i = 0; i < 2; ++i)
    if (!mx::rz_plan_tile(hb, out_w, i == 0 ? 1 : 3, ksh, ksv, &r->tile[i])) {
      mx::set_error("resize_create: the downscale is too steep: the taps of four output bytes of one row do not fit the staging buffer");
      delete r;
      return nullptr;
    }
  const size_t n_hb = hb.size(), n_vb = vb.size(), n_hk = hk.size(), n_vk = vk.size();
  std::vector<int32_t> all;
  all.reserve(n_hb + n_vb + n_hk + n_vk);
  all.insert(all.end(), hb.begin(), hb.end());
  all.insert(all.end(), vb.begin(), vb.end());
  all.insert(all.end(), hk.begin(), hk.end());
  all.insert(all.end(), vk.begin(), vk.end());
  hipError_t err = hipMalloc(&r->tables, all.size() * sizeof(int32_t));
  if (err == hipSuccess) err = hipMemcpy(r->tables, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    mx::set_error(std::string("resize_create: uploading the tables: ") + hipGetErrorString(err));
    if (r->tables) (void)hipFree(r->tables);
    delete r;
    return nullptr;
  }
  const int32_t* base = static_cast<const int32_t*>(r->tables);     // hb and vb hold an even number of words each: every table stays 8-byte aligned
  r->hb = reinterpret_cast<const int2*>(base);
  r->vb = reinterpret_cast<const int2*>(base + n_hb);
  r->hk = base + n_hb + n_vb;
  r->vk = base + n_hb + n_vb + n_hk;
  return r;
}

extern "C" void mx_resize_destroy(mx_resize* r) {
  if (!r) return;
  if (r->tables) (void)hipFree(r->tables);
  delete r;
}

extern "C" int mx_resize_u8(mx_resize* r, void* stream, const uint8_t* src, uint8_t* dst, int B, int C) {
  MX_CHECK(r && src && dst, "resize_u8: null operand");
  MX_CHECK(B > 0, "resize_u8: sizes must be positive");
  MX_CHECK(C == 1 || C == 3, "resize_u8: C must be 1 or 3");
  MX_CHECK(src != dst, "resize_u8: dst may not alias src");
  const mx::rz_tile t = r->tile[C == 1 ? 0 : 1];
  const int64_t gx = mx::cdiv64((int64_t)r->out_w * C, t.ew), gy = mx::cdiv64(r->out_h, mx::kRzTileRows);
  MX_CHECK(gx <= 0x7fffffffL && gy <= 65535 && B <= 65535, "resize_u8: more tiles than one launch holds");
  mx::rz_args a;
  a.src = src; a.dst = dst; a.hb = r->hb; a.hk = r->hk; a.vb = r->vb; a.vk = r->vk;
  a.in_h = r->in_h; a.in_w = r->in_w; a.out_h = r->out_h; a.out_w = r->out_w; a.ksize_h = r->ksize_h; a.ksize_v = r->ksize_v; a.t = t;
  a.src_bytes = (size_t)B * r->in_h * r->in_w * C;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B);
  if (C == 1) mx::rz_launch<1>(t, grid, (hipStream_t)stream, a);
  else mx::rz_launch<3>(t, grid, (hipStream_t)stream, a);
  MX_LAUNCH_CHECK();
  return 0;
}
