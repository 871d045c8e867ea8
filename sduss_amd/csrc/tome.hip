// Token merging (Bolya & Hoffman, "Token Merging for Fast Stable Diffusion"; tomesd with use_rand = False) for the UNet's self-attention: four launches.
//
//   tome_match_kernel        node_max[i], node_idx[i] = max / argmax over the destinations j of <src_i, dst_j> / (|src_i| |dst_j|); neither the
//                            normalised metric nor the score matrix reaches memory
//   tome_select_kernel       per sample: the r sources with the largest node_max (exact radix select, no sort) and the four tables the other two read
//   tome_merge_kernel        the merged sequence: unmerged sources in ascending token order, then every destination as the mean of itself and the
//                            sources merged into it, each row LayerNorm-ed (no affine) in fp32 first when eps >= 0
//   tome_unmerge_add_kernel  y[t] = y[t] + o[row_of[t]]
//
// The token grid h x w is cut into cells of sy x sx; the top-left token of a cell is a destination, every other token a source, both in ascending
// token order.  Ordinal -> token is closed-form integer arithmetic (tome_dst_token / tome_src_token), so no launch needs an index table for the sets.
//
// tome_match_kernel.  A workgroup of four waves owns 64 consecutive sources of one sample, 16 per wave.  A wave gathers its 16 rows ONCE and keeps
// them as the A fragments of v_mfma_f32_16x16x32_bf16 in registers (C = 640: 80 VGPRs, C = 1280: 160); their squared norms come from the same
// registers.  The destination rows stream through LDS in tiles shared by the four waves, double-buffered: while the waves multiply tile t, the 16-byte
// loads of tile t + 1 are in flight into registers; they are written to the other buffer after the k loop (one barrier a tile).  A tile is 32 rows up
// to C = 640 and 16 rows above (two buffers of 32 x 1280 bf16 would be the whole 160 KB with no room for the row pad that keeps the fragment reads free
// of bank conflicts).  A destination's squared norm is summed by the threads that stage it.  Accumulator layout: a lane holds destination j = lane & 15
// of each 16-row block and sources 4 (lane >> 4) + reg; the score is acc * (1 / |dst_j|), the running (max, argmax) per source stays in registers
// (strict >, destinations ascending: the lowest ordinal wins a tie), destinations past Ndst are -inf; at the end the 16 lanes of a source reduce
// (equal maxima: the lower ordinal) and the maximum is multiplied by 1 / |src_i|, which is constant over j.  A zero row has inverse norm 0.
//
// Built without packed fp32 instructions (Makefile).
#include <mutex>

#include "common.h"

namespace mx {
namespace {

struct TomeGrid { int h, w, sy, sx, wd, L, Ndst, Nsrc, spb, n1; };     // wd = w / sx; spb, n1: the sources of a band of sy rows, of its first row
static inline TomeGrid tome_grid(int h, int w, int sy, int sx) {
  TomeGrid g; g.h = h; g.w = w; g.sy = sy; g.sx = sx; g.wd = w / sx; g.L = h * w; g.Ndst = (h / sy) * g.wd; g.Nsrc = g.L - g.Ndst;
  g.n1 = w - g.wd; g.spb = sy * w - g.wd;
  return g;
}
__device__ __forceinline__ int tome_dst_token(const TomeGrid& g, int j) { return (j / g.wd) * g.sy * g.w + (j % g.wd) * g.sx; }
__device__ __forceinline__ int tome_src_token(const TomeGrid& g, int i) {
  const int band = i / g.spb;
  int rem = i - band * g.spb;
  if (rem < g.n1) { const int q = rem / (g.sx - 1); return band * g.sy * g.w + q * g.sx + (rem - q * (g.sx - 1)) + 1; }     // (n1 = 0 when sx = 1)
  return (band * g.sy + 1) * g.w + (rem - g.n1);         // rows 1 .. sy - 1 of the band hold sources only
}
__device__ __forceinline__ float inv_norm(float ss) { return ss > 0.f ? 1.0f / sqrtf(ss) : 0.f; }
__device__ __forceinline__ float sumsq8(const u32x4 u, float s) {
  float f[8];
  unpack_bf16x8(u, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) s = fmaf(f[e], f[e], s);
  return s;
}

// KSMAX: the k-steps of 32 channels the register file is laid out for (C <= 32 KSMAX); NB: 16-row blocks of a destination tile
template <int KSMAX, int NB>
__global__ __launch_bounds__(256) void tome_match_kernel(const bf16_t* __restrict__ x, int ldx, TomeGrid g, int C, float* __restrict__ node_max,
                                                         int* __restrict__ node_idx) {
  constexpr int TJ = 16 * NB, TPR = 256 / TJ, NCH = KSMAX * 4 / TPR, PITCH = KSMAX * 32 + 8;
  __shared__ __attribute__((aligned(16))) bf16_t tile[2][TJ * PITCH];
  __shared__ float dinv[2][TJ];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.y;
  const int nks = C / 32, nch = C / 8;
  const bf16_t* xb = x + (size_t)b * g.L * ldx;

  // the wave's 16 source rows as A fragments: lane = (row lane & 15, channels 32 ks + 8 (lane >> 4) ..)
  const int i0 = blockIdx.x * 64 + wave * 16;
  const bf16_t* ap = xb + (size_t)tome_src_token(g, min(i0 + (lane & 15), g.Nsrc - 1)) * ldx + 8 * (lane >> 4);
  bf16x8 af[KSMAX];
  float ss = 0.f;
#pragma unroll
  for (int ks = 0; ks < KSMAX; ++ks)
    if (ks < nks) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(ap + ks * 32);
      af[ks] = __builtin_bit_cast(bf16x8, v);
      ss = sumsq8(v, ss);
    }
  ss += __shfl_xor(ss, 16, 64);
  ss += __shfl_xor(ss, 32, 64);
  const float sinv = inv_norm(ss);        // of source row lane & 15

  // staging: TPR consecutive threads own a destination row of the tile, chunk sub + n TPR each
  const int srow = tid / TPR, sub = tid % TPR;
  u32x4 st[NCH];
  auto load_tile = [&](int t) {
    const int j = t * TJ + srow;
    const bool valid = j < g.Ndst;
    const bf16_t* dp = xb + (size_t)tome_dst_token(g, valid ? j : 0) * ldx;
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      const int c = sub + n * TPR;
      st[n] = (valid && c < nch) ? *reinterpret_cast<const u32x4*>(dp + c * 8) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto store_tile = [&](int buf) {
    float s2 = 0.f;
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      const int c = sub + n * TPR;
      if (c < nch) {
        *reinterpret_cast<u32x4*>(&tile[buf][srow * PITCH + c * 8]) = st[n];
        s2 = sumsq8(st[n], s2);
      }
    }
#pragma unroll
    for (int o = TPR / 2; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
    if (sub == 0) dinv[buf][srow] = inv_norm(s2);
  };

  float m[4];
  int mi[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { m[q] = -INFINITY; mi[q] = 0x7fffffff; }
  const int ntiles = (g.Ndst + TJ - 1) / TJ;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntiles) load_tile(t + 1);
    f32x4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16_t* bp = &tile[buf][(lane & 15) * PITCH + 8 * (lane >> 4)];
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks)
      if (ks < nks) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], *reinterpret_cast<const bf16x8*>(bp + nb * 16 * PITCH + ks * 32), acc[nb], 0, 0, 0);
      }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int j = t * TJ + nb * 16 + (lane & 15);
      const float dv = dinv[buf][nb * 16 + (lane & 15)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = j < g.Ndst ? acc[nb][q] * dv : -INFINITY;
        if (v > m[q]) { m[q] = v; mi[q] = j; }
      }
    }
    if (t + 1 < ntiles) store_tile(buf ^ 1);     // (its last readers passed the barrier that ended tile t - 1)
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float om = __shfl_xor(m[q], o, 64);
      const int oi = __shfl_xor(mi[q], o, 64);
      if (om > m[q] || (om == m[q] && oi < mi[q])) { m[q] = om; mi[q] = oi; }
    }
    const int row = 4 * (lane >> 4) + q;
    const float si = __shfl(sinv, row, 64);
    if ((lane & 15) == 0 && i0 + row < g.Nsrc) {
      node_max[(size_t)b * g.Nsrc + i0 + row] = m[q] * si;
      node_idx[(size_t)b * g.Nsrc + i0 + row] = mi[q];
    }
  }
}

// ---- select: one workgroup per sample ----
constexpr int kSelThreads = 1024;
constexpr int kSelExtra = 256 + 16 + 4;          // histogram, wave sums, broadcast words
__device__ __forceinline__ unsigned tome_key(float v) {      // order-preserving: a < b  <=>  key(a) < key(b)
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// exclusive prefix of one int per thread over the workgroup, and the total
__device__ __forceinline__ int block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int n = __shfl_up(inc, o, 64); if (lane >= o) inc += n; }
  __syncthreads();
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
  for (int k = 0; k < kSelThreads / 64; ++k) { const int s = wsum[k]; if (k < wave) base += s; total += s; }
  return base + inc - v;
}

__global__ __launch_bounds__(kSelThreads) void tome_select_kernel(const float* __restrict__ node_max, const int* __restrict__ node_idx, TomeGrid g, int r,
                                                                  int* __restrict__ row_of, int* __restrict__ unm_src, int* __restrict__ dst_start,
                                                                  int* __restrict__ dst_src) {
  extern __shared__ int sm[];
  const int tid = threadIdx.x, b = blockIdx.x, Nsrc = g.Nsrc, Ndst = g.Ndst, n_unm = Nsrc - r;
  unsigned* key = reinterpret_cast<unsigned*>(sm);
  int* idx = sm + Nsrc;              // bit 31: merged
  int* hist = sm + 2 * Nsrc;
  int* wsum = hist + 256;
  int* bc = wsum + 16;
  int* cnt = sm;                     // the keys' place once they are spent (Ndst <= Nsrc)
  node_max += (size_t)b * Nsrc; node_idx += (size_t)b * Nsrc;
  row_of += (size_t)b * g.L; unm_src += (size_t)b * n_unm; dst_start += (size_t)b * (Ndst + 1); dst_src += (size_t)b * r;

  for (int i = tid; i < Nsrc; i += kSelThreads) { key[i] = tome_key(node_max[i]); idx[i] = min(max(node_idx[i], 0), Ndst - 1); }
  __syncthreads();
  // the r-th largest key T, byte by byte from the top; `remaining` of the keys equal to T are taken
  unsigned prefix = 0u, mask = 0u;
  int remaining = r;
  if (r > 0)
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < Nsrc; i += kSelThreads)
        if ((key[i] & mask) == prefix) atomicAdd(&hist[(key[i] >> shift) & 255u], 1);
      __syncthreads();
      if (tid == 0) {
        int cum = 0, bin = 255;
        for (; bin > 0; --bin) { const int hc = hist[bin]; if (cum + hc >= remaining) break; cum += hc; }
        bc[0] = bin; bc[1] = remaining - cum;
      }
      __syncthreads();
      prefix |= (unsigned)bc[0] << shift; mask |= 255u << shift; remaining = bc[1];
      __syncthreads();
    }
  // a thread owns a run of consecutive sources: equal keys are taken in ascending ordinal, unmerged rows are numbered in ascending ordinal
  const int per = (Nsrc + kSelThreads - 1) / kSelThreads;
  const int i0 = min(tid * per, Nsrc), i1 = min(i0 + per, Nsrc);
  int total, n = 0;
  for (int i = i0; i < i1; ++i) n += key[i] == prefix;
  int eq = block_scan(n, wsum, total);
  n = 0;
  for (int i = i0; i < i1; ++i) {
    const unsigned k = key[i];
    const bool mg = r > 0 && (k > prefix || (k == prefix && eq++ < remaining));
    if (mg) idx[i] |= 0x80000000; else ++n;
  }
  int row = block_scan(n, wsum, total);
  for (int i = i0; i < i1; ++i) {
    const int tok = tome_src_token(g, i), w = idx[i];
    if (w < 0) row_of[tok] = n_unm + (w & 0x7fffffff);
    else { unm_src[row] = tok; row_of[tok] = row++; }
  }
  for (int j = tid; j < Ndst; j += kSelThreads) row_of[tome_dst_token(g, j)] = n_unm + j;
  __syncthreads();                   // every key has been read
  // the merged sources per destination: counts, their prefix, then each thread fills the lists of the destinations it owns by walking the
  // sample's sources in order (every thread reads the same word: a broadcast), so the lists are ascending without any ordering atomics
  for (int j = tid; j < Ndst; j += kSelThreads) cnt[j] = 0;
  __syncthreads();
  for (int i = i0; i < i1; ++i) if (idx[i] < 0) atomicAdd(&cnt[idx[i] & 0x7fffffff], 1);
  __syncthreads();
  const int perd = (Ndst + kSelThreads - 1) / kSelThreads;
  const int j0 = min(tid * perd, Ndst), j1 = min(j0 + perd, Ndst);
  n = 0;
  for (int j = j0; j < j1; ++j) n += cnt[j];
  int start = block_scan(n, wsum, total);
  for (int j = j0; j < j1; ++j) { const int c = cnt[j]; dst_start[j] = start; cnt[j] = start; start += c; }
  if (tid == 0) dst_start[Ndst] = r;
  if (n > 0)
    for (int i = 0; i < Nsrc; ++i) {
      const int w = idx[i];
      if (w < 0) {
        const int j = w & 0x7fffffff;
        if (j >= j0 && j < j1) dst_src[cnt[j]++] = tome_src_token(g, i);
      }
    }
}

// ---- merge: one wave per merged row; a lane holds chunks lane, lane + 64, lane + 128 of 8 channels ----
constexpr int kMergeChunks = 3;
__device__ __forceinline__ void merge_load_row(const bf16_t* p, int nch, int C, float eps, int lane, float (&v)[kMergeChunks][8]) {
  float s = 0.f;
#pragma unroll
  for (int n = 0; n < kMergeChunks; ++n) {
    const int c = lane + 64 * n;
    if (c < nch) {
      unpack_bf16x8(*reinterpret_cast<const u32x4*>(p + c * 8), v[n]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[n][e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[n][e] = 0.f;
    }
  }
  if (eps < 0.f) return;
  const float mean = wave_sum(s) / (float)C;
  float s2 = 0.f;
#pragma unroll
  for (int n = 0; n < kMergeChunks; ++n)
    if (lane + 64 * n < nch) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { v[n][e] -= mean; s2 = fmaf(v[n][e], v[n][e], s2); }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(s2) / (float)C + eps);
#pragma unroll
  for (int n = 0; n < kMergeChunks; ++n)
#pragma unroll
    for (int e = 0; e < 8; ++e) v[n][e] *= rstd;
}

__global__ __launch_bounds__(256) void tome_merge_kernel(const bf16_t* __restrict__ x, int ldx, TomeGrid g, int C, int r, int rows, const int* __restrict__ unm_src,
                                                         const int* __restrict__ dst_start, const int* __restrict__ dst_src, float eps,
                                                         bf16_t* __restrict__ out, int ldo) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int n_unm = g.Nsrc - r, Lm = g.L - r, nch = C / 8;
  const int b = row / Lm, m = row - b * Lm;
  const bf16_t* xb = x + (size_t)b * g.L * ldx;
  float acc[kMergeChunks][8];
  if (m < n_unm) {
    merge_load_row(xb + (size_t)min(max(unm_src[(size_t)b * n_unm + m], 0), g.L - 1) * ldx, nch, C, eps, lane, acc);
  } else {
    const int j = m - n_unm;
    merge_load_row(xb + (size_t)tome_dst_token(g, j) * ldx, nch, C, eps, lane, acc);
    const int s0 = max(dst_start[(size_t)b * (g.Ndst + 1) + j], 0), s1 = min(dst_start[(size_t)b * (g.Ndst + 1) + j + 1], r);
    for (int s = s0; s < s1; ++s) {
      float v[kMergeChunks][8];
      merge_load_row(xb + (size_t)min(max(dst_src[(size_t)b * r + s], 0), g.L - 1) * ldx, nch, C, eps, lane, v);
#pragma unroll
      for (int n = 0; n < kMergeChunks; ++n)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[n][e] += v[n][e];
    }
    if (s1 > s0) {
      const float cntf = (float)(1 + s1 - s0);
#pragma unroll
      for (int n = 0; n < kMergeChunks; ++n)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[n][e] /= cntf;
    }
  }
  bf16_t* op = out + (size_t)row * ldo;
#pragma unroll
  for (int n = 0; n < kMergeChunks; ++n)
    if (lane + 64 * n < nch) *reinterpret_cast<u32x4*>(op + (lane + 64 * n) * 8) = pack_bf16x8(acc[n]);
}

// ---- unmerge: a thread per 16-byte chunk of y ----
__global__ __launch_bounds__(256) void tome_unmerge_add_kernel(const bf16_t* __restrict__ o, int ldo, const int* __restrict__ row_of, const bf16_t* res, int ldr,
                                                               bf16_t* y, int ldy, long chunks, int nch, int L, int Lm) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= chunks) return;
  const long t = id / nch;                 // token row over the batch
  const int c = (int)(id - t * nch);
  const long b = t / L;
  const int mrow = min(max(row_of[t], 0), Lm - 1);
  float v[8];
  unpack_bf16x8(*reinterpret_cast<const u32x4*>(o + (size_t)(b * Lm + mrow) * ldo + c * 8), v);
  if (res) {
    float q[8];
    unpack_bf16x8(*reinterpret_cast<const u32x4*>(res + (size_t)t * ldr + c * 8), q);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = q[e] + v[e];
  }
  *reinterpret_cast<u32x4*>(y + (size_t)t * ldy + c * 8) = pack_bf16x8(v);
}

int tome_check_grid(const char* who, int B, int h, int w, int sy, int sx) {
  MX_CHECK(B >= 1 && h >= 1 && w >= 1 && sy >= 1 && sx >= 1 && sy * sx >= 2, std::string(who) + ": B, h, w >= 1 and cells of at least two tokens are required");
  MX_CHECK(h % sy == 0 && w % sx == 0, std::string(who) + ": the cells must tile the token grid (h % sy == 0, w % sx == 0)");
  MX_CHECK((long)h * w <= 16384, std::string(who) + ": at most 16384 tokens an image");
  return 0;
}
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace
}  // namespace mx

extern "C" int mx_tome_sizes(int h, int w, int sy, int sx, float ratio, int out[4]) {
  using namespace mx;
  MX_CHECK(out != nullptr && h >= 1 && w >= 1 && sy >= 1 && sx >= 1, "tome_sizes: bad arguments");
  const int L = h * w;
  out[0] = 0; out[1] = 0; out[2] = 0; out[3] = L;
  MX_CHECK(h % sy == 0 && w % sx == 0 && sy * sx >= 2, "tome_sizes: the cells do not tile the token grid: the level runs unmerged");
  const TomeGrid g = tome_grid(h, w, sy, sx);
  out[0] = g.Ndst; out[1] = g.Nsrc;
  int r = std::max(0, std::min(g.Nsrc, (int)((double)L * (double)ratio)));
  r = std::max(0, L - (L - r + 63) / 64 * 64);       // lowered until L - r is a whole number of 64-key tiles
  out[2] = r; out[3] = L - r;
  MX_CHECK(r > 0, "tome_sizes: nothing to merge at this size and ratio: the level runs unmerged");
  return 0;
}

extern "C" size_t mx_tome_table_bytes(int B, int h, int w, int sy, int sx, int r) {
  using namespace mx;
  if (B < 1 || h < 1 || w < 1 || sy < 1 || sx < 1 || h % sy || w % sx || r < 0) return 0;
  const TomeGrid g = tome_grid(h, w, sy, sx);
  if (r > g.Nsrc) return 0;
  return align256((size_t)B * g.L * 4) + align256((size_t)B * (g.Nsrc - r) * 4) + align256((size_t)B * (g.Ndst + 1) * 4) + align256((size_t)B * r * 4);
}

extern "C" int mx_tome_match(void* stream, const void* x, int ldx, int B, int h, int w, int sy, int sx, int C, float* node_max, int* node_idx) {
  using namespace mx;
  if (tome_check_grid("tome_match", B, h, w, sy, sx)) return 1;
  MX_CHECK(C >= 64 && C % 64 == 0 && C <= 1280, "tome_match: C must be a multiple of 64, at most 1280");
  MX_CHECK(x && node_max && node_idx && ldx >= C && ldx % 8 == 0 && aligned_to(x, 16), "tome_match: x (16-byte aligned, ldx >= C, ldx % 8 == 0), node_max and node_idx are required");
  const TomeGrid g = tome_grid(h, w, sy, sx);
  const dim3 grid(cdiv(g.Nsrc, 64), B);
  if (C <= 640) hipLaunchKernelGGL((tome_match_kernel<20, 2>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, g, C, node_max, node_idx);
  else hipLaunchKernelGGL((tome_match_kernel<40, 1>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, g, C, node_max, node_idx);
  MX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mx_tome_select(void* stream, const float* node_max, const int* node_idx, int B, int h, int w, int sy, int sx, int r, int* row_of,
                              int* unm_src, int* dst_start, int* dst_src) {
  using namespace mx;
  if (tome_check_grid("tome_select", B, h, w, sy, sx)) return 1;
  const TomeGrid g = tome_grid(h, w, sy, sx);
  MX_CHECK(r >= 0 && r <= g.Nsrc, "tome_select: r must be in 0 .. Nsrc");
  MX_CHECK(node_max && node_idx && row_of && dst_start && (unm_src || r == g.Nsrc) && (dst_src || r == 0), "tome_select: null operand");
  const size_t lds = (size_t)(2 * g.Nsrc + kSelExtra) * sizeof(int);
  MX_CHECK(lds <= 160 * 1024, "tome_select: LDS budget exceeded");
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [] { attr = hipFuncSetAttribute((const void*)tome_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
  MX_CHECK(attr == hipSuccess, std::string("tome_select: ") + hipGetErrorString(attr));
  hipLaunchKernelGGL(tome_select_kernel, dim3(B), dim3(kSelThreads), lds, (hipStream_t)stream, node_max, node_idx, g, r, row_of, unm_src, dst_start, dst_src);
  MX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mx_tome_merge(void* stream, const void* x, int ldx, int B, int h, int w, int sy, int sx, int C, int r, const int* unm_src,
                             const int* dst_start, const int* dst_src, float eps, void* out, int ldo) {
  using namespace mx;
  if (tome_check_grid("tome_merge", B, h, w, sy, sx)) return 1;
  const TomeGrid g = tome_grid(h, w, sy, sx);
  MX_CHECK(r >= 0 && r <= g.Nsrc, "tome_merge: r must be in 0 .. Nsrc");
  MX_CHECK(C >= 8 && C % 8 == 0 && C <= 512 * kMergeChunks, "tome_merge: C must be a multiple of 8, at most 1536");
  MX_CHECK(x && out && dst_start && (unm_src || r == g.Nsrc) && (dst_src || r == 0), "tome_merge: null operand");
  MX_CHECK(ldx >= C && ldo >= C && ldx % 8 == 0 && ldo % 8 == 0 && aligned_to(x, 16) && aligned_to(out, 16), "tome_merge: rows must be 16-byte aligned");
  MX_CHECK(eps == eps, "tome_merge: NaN eps");
  const long rows = (long)B * (g.L - r);
  MX_CHECK(rows < 2147483647L, "tome_merge: too many rows");
  hipLaunchKernelGGL(tome_merge_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, g, C, r, (int)rows, unm_src,
                     dst_start, dst_src, eps, (bf16_t*)out, ldo);
  MX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mx_tome_unmerge(void* stream, const void* o, int ldo, const int* row_of, const void* residual, int ldr, void* y, int ldy, int B, int L,
                               int Lm, int C) {
  using namespace mx;
  MX_CHECK(B >= 1 && L >= 1 && Lm >= 1 && Lm <= L && C >= 8 && C % 8 == 0, "tome_unmerge: B, L >= 1, 1 <= Lm <= L and C a multiple of 8 are required");
  MX_CHECK(o && row_of && y && ldo >= C && ldy >= C && ldo % 8 == 0 && ldy % 8 == 0 && (!residual || (ldr >= C && ldr % 8 == 0)) && aligned_to(o, 16) &&
           aligned_to(y, 16) && aligned_to(residual, 16), "tome_unmerge: rows must be 16-byte aligned");
  // (y may be the residual itself: a thread reads and writes the same chunk; y must not overlap o)
  const size_t on = (size_t)B * Lm * ldo * 2, yn = (size_t)B * L * ldy * 2;
  MX_CHECK((uintptr_t)o + on <= (uintptr_t)y || (uintptr_t)y + yn <= (uintptr_t)o, "tome_unmerge: o and y must not overlap");
  const long chunks = (long)B * L * (C / 8);
  MX_CHECK(cdiv64(chunks, 256) < 2147483647L, "tome_unmerge: too many elements");
  hipLaunchKernelGGL(tome_unmerge_add_kernel, dim3((unsigned)cdiv64(chunks, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)o, ldo, row_of,
                     (const bf16_t*)residual, ldr, (bf16_t*)y, ldy, chunks, C / 8, L, Lm);
  MX_LAUNCH_CHECK();
  return 0;
}
