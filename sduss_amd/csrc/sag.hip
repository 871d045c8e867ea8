// Self-attention guidance (SAG; diffusers' StableDiffusionSAGPipeline) for gfx950: mx_attention_colmass, mx_sag_degrade, mx_sag_fold.
//
// mx_attention_colmass: mass[b][j] = (1 / heads) sum_h sum_i softmax_j(q_h[i] . k_h[j] * scale) -- how much attention token j receives -- and
// mask = mass > 1, from q and k alone: the probabilities never reach memory.  head_dim 64, any L >= 1.
//   A workgroup owns (sample, head, 128-row query block); its four waves own 32 query rows each and keep their Q fragments in registers for two
//   passes over the keys, which stream as 64-key K tiles (8 KB, attn_tile.h's K image) through two LDS buffers, the next tile in registers while
//   the current one computes.
//   PASS A  S^T = K Q^T (attn_tile.h's qk): a lane owns one query COLUMN, so the running maximum and sum of the row's exponentials are in-lane
//           chains and one exchange with lane ^ 32.  No V, no O.
//   Between the passes every wave leaves (m_i, 1 / l_i) of its 32 rows in its own 256 bytes of LDS (1 / l_i = 0 for a row past the end: it then
//           contributes nothing), and every lane takes those of the 16 rows it holds in pass B: the statistics never travel through HBM.
//   PASS B  S = Q K^T, the SAME fragments with the operands swapped: a lane now holds 16 query rows of one KEY column, p = exp2(s c - m_i) / l_i, and
//           the column's sum over the wave's 32 rows is 15 in-lane adds and one exchange with lane ^ 32.  The four waves' sums meet in LDS and 64
//           threads add them in wave order and write partial[b][head][query block][key].
//   A second launch adds the partials over heads, then query blocks, in index order, divides by heads and writes mass and mask.
//   Every sum has a fixed order and no atomic is used: the result is the same bits run after run.
//   Keys past L: zero rows in LDS, masked to -inf in pass A, not written in pass B.  Query rows past L: loaded clamped, weight 0.
//
// mx_sag_degrade: ONE launch.  x0 = x - sigma eps_u; out = (mask ? blur(x0) : x0) + sigma eps_u, blur the separable 9-tap Gaussian under reflect
// padding of 4, mask the nearest-neighbour upsampling of the h_m x w_m token mask.  A workgroup owns a 32 x 32 tile of one (row, channel) plane: the
// x0 tile and its halo of 4 are staged in LDS once, the horizontal pass goes to a second LDS plane, the vertical pass and the select to memory.
// mx_sag_fold: eps_c += coef (eps_u - eps_d) on the rows of the SAG requests, so that the unchanged scheduler step then computes
// eps_u + g (eps_c - eps_u) + sag_scale (eps_u - eps_d) with coef = sag_scale / g.
#include "common.h"
#include "../../include/mxdenoise.h"
#include "attn_tile.h"
#include "step_math.h"   // load_as_f32 / store_from_f32; no mul + add contraction from here on (the degrade's unmasked elements are (x - n) + n, op by op)

namespace mx {

struct MassArgs {
  const bf16_t* q; const bf16_t* k;
  int ldq, ldk;
  int B, H, L, nqb;
  float c;                                     // the scores' factor into the log2 domain: scale * log2(e), or 1 for prescaled q
  float* partial;                              // [B][H][nqb][L]
};

constexpr int kMassTile = 8192;                // one K tile: 64 rows of 128 B, 16-byte chunk ^= (row >> 1) & 7

// the thread's two 16-byte chunks (rows srow and srow + 32, chunk sch) of the K tile at key0; rows past L are zeros
__device__ __forceinline__ void mass_load(const MassArgs& p, const char* kbase, const int key0, const int srow, const int sch, u32x4 (&rk)[2]) {
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int key = key0 + srow + 32 * i;
    rk[i] = key < p.L ? *reinterpret_cast<const u32x4*>(kbase + (long)key * p.ldk * 2 + sch * 16) : zero4;
  }
}
__device__ __forceinline__ void mass_store(char* img, const unsigned st_off, const u32x4 (&rk)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(img + st_off + i * 4096) = rk[i];
}

__global__ __launch_bounds__(256, 2) void colmass_kernel(const MassArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kMassTile];
  __shared__ __attribute__((aligned(16))) float stat[4][64];      // per wave: m of its 32 rows, then 1 / l
  __shared__ float colbuf[2][4][64];                              // per tile parity and wave: the wave's column sums of the tile
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int qb = blockIdx.x % p.nqb, bh = blockIdx.x / p.nqb;
  const int head = bh % p.H, b = bh / p.H;
  const int q0 = qb * 128 + wave * 32;         // (a wave whose rows all lie past the end still stages and keeps the barriers)
  const float c = p.c;

  bf16x8 qf[4];
  {
    int qi = q0 + r;
    if (qi > p.L - 1) qi = p.L - 1;
    const bf16_t* qp = p.q + ((long)b * p.L + qi) * p.ldq + head * 64 + hh * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
  }
  const int srow = tid >> 3, sch = tid & 7;
  const char* kbase = (const char*)(p.k + (long)b * p.L * p.ldk + head * 64);
  const unsigned st_off = (unsigned)(srow * 128 + ((sch ^ ((srow >> 1) & 7)) * 16));
  unsigned koff[4];
  frag_offsets(r, hh, koff);
  const int ntiles = (p.L + KT - 1) / KT;
  const int last_valid = p.L - (ntiles - 1) * KT;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  u32x4 rk[2];
  bf16x8 fr[8];

  // ---- pass A: the row maximum and the row sum of query q0 + r, this half-wave's keys ----
  float m_run = -INFINITY, l_run = 0.f;
  mass_load(p, kbase, 0, srow, sch, rk);
  mass_store(smem, st_off, rk);
  __syncthreads();
  unsigned bofs = 0;
  for (int kt = 0; kt < ntiles; ++kt) {
    const bool has_next = kt + 1 < ntiles;
    if (has_next) mass_load(p, kbase, (kt + 1) * KT, srow, sch, rk);
    read_k(fr, smem + bofs, koff);
    f32x16 s[2];
    qk(s, fr, qf, zero16);
    if (!has_next && last_valid < KT) {        // (wave-uniform) the ragged last tile: its missing keys never count
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh >= last_valid) s[kb][e] = -INFINITY;
    }
    const float m_new = fmaxf(m_run, col_max(s) * c);            // (c > 0; key 0 of every tile exists, so m_new is finite)
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int e = 0; e < 16; ++e) psum += __builtin_amdgcn_exp2f(fmaf(s[kb][e], c, -m_new));
    l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + psum;
    m_run = m_new;
    bofs ^= kMassTile;
    if (has_next) mass_store(smem + bofs, st_off, rk);
    __syncthreads();
  }
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  if (hh == 0) {
    stat[wave][r] = m_run;
    stat[wave][32 + r] = q0 + r < p.L ? 1.0f / l_tot : 0.f;
  }
  mass_load(p, kbase, 0, srow, sch, rk);
  mass_store(smem, st_off, rk);                // (every wave is past pass A's last barrier: both buffers are free)
  __syncthreads();
  // element e of a pass-B block is query row (e & 3) + 8 (e >> 2) + 4 hh of the wave
  float mrow[16], irow[16];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 mv = *reinterpret_cast<const f32x4*>(&stat[wave][8 * g + 4 * hh]);
    const f32x4 iv = *reinterpret_cast<const f32x4*>(&stat[wave][32 + 8 * g + 4 * hh]);
#pragma unroll
    for (int j = 0; j < 4; ++j) { mrow[4 * g + j] = mv[j]; irow[4 * g + j] = iv[j]; }
  }

  // ---- pass B: the column sums of the normalised probabilities ----
  float* out = p.partial + (((long)b * p.H + head) * p.nqb + qb) * p.L;
  bofs = 0;
  for (int kt = 0; kt < ntiles; ++kt) {
    const bool has_next = kt + 1 < ntiles;
    if (has_next) mass_load(p, kbase, (kt + 1) * KT, srow, sch, rk);
    read_k(fr, smem + bofs, koff);
    f32x16 s[2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[ks], fr[kb * 4 + ks], ks == 0 ? zero16 : s[kb], 0, 0, 0);
    const int par = kt & 1;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      float cs = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) cs += __builtin_amdgcn_exp2f(fmaf(s[kb][e], c, -mrow[e])) * irow[e];
      cs += __shfl_xor(cs, 32, 64);            // (a + b = b + a: both halves hold the same bits)
      if (hh == 0) colbuf[par][wave][kb * 32 + r] = cs;
    }
    bofs ^= kMassTile;
    if (has_next) mass_store(smem + bofs, st_off, rk);
    __syncthreads();
    // (colbuf[par] is written again two tiles on, behind the next barrier, which this read precedes)
    const int key = kt * KT + tid;
    if (tid < KT && key < p.L) out[key] = ((colbuf[par][0][tid] + colbuf[par][1][tid]) + colbuf[par][2][tid]) + colbuf[par][3][tid];
  }
}

// mass[b][j] = (sum over heads, then query blocks, in index order) / heads; mask = mass > 1
__global__ __launch_bounds__(256) void colmass_reduce_kernel(const float* __restrict__ partial, float* __restrict__ mass, unsigned char* __restrict__ mask, int B, int H,
                                                             int nqb, int L) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * L) return;
  const int b = (int)(idx / L), j = (int)(idx % L);
  const float* pp = partial + (long)b * H * nqb * L + j;
  float acc = 0.f;
  for (int i = 0; i < H * nqb; ++i) acc += pp[(long)i * L];
  const float m = acc / (float)H;
  mass[idx] = m;
  mask[idx] = m > 1.0f ? 1 : 0;
}

// ---- degrade ----
constexpr int kDegTile = 32, kDegHalo = 4, kDegSpan = kDegTile + 2 * kDegHalo;
constexpr int kSagMaxRows = 64;              // SAG rows a launch: their indices (and the fold's factors) travel in the kernel arguments
struct DegArgs {
  const void* lat; const void* eps; void* out;
  const float* sigma; const unsigned char* mask;
  int rows[kSagMaxRows];                       // the request (latent row = unconditional noise row) of each output row
  int C, h, w, hm, wm, tiles_x;
  float taps[9];
};
// index i of an axis of n > 4 under reflect padding (|i - [0, n)| <= 4: one reflection); a tile's positions further out serve no output and are clamped
__device__ __forceinline__ int reflect_at(int i, const int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}
template <typename T>
__global__ __launch_bounds__(256) void sag_degrade_kernel(const DegArgs p) {
  __shared__ float x0t[kDegSpan][kDegSpan + 1];
  __shared__ float hb[kDegSpan][kDegTile];
  const int tid = threadIdx.x;
  const int y0 = (blockIdx.x / p.tiles_x) * kDegTile, x0 = (blockIdx.x % p.tiles_x) * kDegTile;
  const int ch = blockIdx.y, i = blockIdx.z;
  const int src = p.rows[i];
  const float sg = p.sigma[src];
  const long plane = (long)p.h * p.w;
  const T* lat = (const T*)p.lat + ((long)src * p.C + ch) * plane;
  const T* eps = (const T*)p.eps + ((long)src * p.C + ch) * plane;
  T* out = (T*)p.out + ((long)i * p.C + ch) * plane;
  for (int t = tid; t < kDegSpan * kDegSpan; t += 256) {
    const int ty = t / kDegSpan, tx = t % kDegSpan;
    const long at = (long)reflect_at(y0 - kDegHalo + ty, p.h) * p.w + reflect_at(x0 - kDegHalo + tx, p.w);
    const float n = sg * load_as_f32<T>(eps, at);
    x0t[ty][tx] = load_as_f32<T>(lat, at) - n;
  }
  __syncthreads();
  for (int t = tid; t < kDegSpan * kDegTile; t += 256) {
    const int ty = t / kDegTile, ox = t % kDegTile;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc = fmaf(p.taps[k], x0t[ty][ox + k], acc);
    hb[ty][ox] = acc;
  }
  __syncthreads();
  for (int t = tid; t < kDegTile * kDegTile; t += 256) {
    const int oy = t / kDegTile, ox = t % kDegTile;
    const int y = y0 + oy, x = x0 + ox;
    if (y >= p.h || x >= p.w) continue;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc = fmaf(p.taps[k], hb[oy + k][ox], acc);
    const bool on = p.mask[(long)src * p.hm * p.wm + (y * p.hm / p.h) * p.wm + x * p.wm / p.w] != 0;
    const long at = (long)y * p.w + x;
    const float n = sg * load_as_f32<T>(eps, at);
    const float v = on ? acc : x0t[oy + kDegHalo][ox + kDegHalo];
    store_from_f32<T>(out, at, v + n);
  }
}

// noise[n + rows[i]] += coef[i] (noise[rows[i]] - eps_d[i]), fp32 ops rounded once to T
struct FoldArgs { int rows[kSagMaxRows]; float coef[kSagMaxRows]; };
template <typename T>
__global__ __launch_bounds__(256) void sag_fold_kernel(T* __restrict__ noise, const T* __restrict__ eps_d, const FoldArgs f, int n, long elems) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= elems) return;
  const int i = blockIdx.y;
  const int src = f.rows[i];
  const float u = load_as_f32<T>(noise, (long)src * elems + e);
  const float d = u - load_as_f32<T>(eps_d, (long)i * elems + e);
  const float t = f.coef[i] * d;
  const long ci = ((long)n + src) * elems + e;
  store_from_f32<T>(noise, ci, load_as_f32<T>(noise, ci) + t);
}

}  // namespace mx

extern "C" size_t mx_attention_colmass_workspace_bytes(int B, int H, int L) {
  if (B <= 0 || H <= 0 || L <= 0) return 0;
  return (size_t)B * H * mx::cdiv(L, 128) * L * sizeof(float);
}

extern "C" int mx_attention_colmass(void* stream, const void* q, int ldq, const void* k, int ldk, int B, int H, int L, float scale, int prescaled,
                                    void* workspace, size_t workspace_bytes, float* mass, unsigned char* mask) {
  using namespace mx;
  MX_CHECK(q && k && workspace && mass && mask, "attention_colmass: null operand");
  MX_CHECK(B > 0 && H > 0 && L > 0, "attention_colmass: empty problem");
  MX_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)mass & 3) == 0,
           "attention_colmass: q, k and the workspace must be 16-byte aligned, mass 4-byte aligned");
  MX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldq >= H * 64 && ldk >= H * 64, "attention_colmass: ldq, ldk must be multiples of 8 elements covering H*64");
  MX_CHECK(prescaled || (scale > 0.f && scale <= 3.0e38f), "attention_colmass: the softmax scale must be positive and finite");
  MX_CHECK(workspace_bytes >= mx_attention_colmass_workspace_bytes(B, H, L), "attention_colmass: workspace too small (mx_attention_colmass_workspace_bytes)");
  MassArgs a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.ldq = ldq; a.ldk = ldk;
  a.B = B; a.H = H; a.L = L; a.nqb = cdiv(L, 128);
  a.c = prescaled ? 1.0f : MX_ATTN_QSCALE(scale);
  a.partial = (float*)workspace;
  const long blocks = (long)B * H * a.nqb;
  MX_CHECK(blocks < 2147483647L && (long)B * L < 2147483647L, "attention_colmass: too many workgroups");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(colmass_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(colmass_reduce_kernel, dim3((unsigned)cdiv64((long)B * L, 256)), dim3(256), 0, st, (const float*)workspace, mass, mask, B, H, a.nqb, L);
  MX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mx_sag_blur_taps(float blur_sigma, float taps[9]) {
  MX_CHECK(taps != nullptr, "sag_blur_taps: null operand");
  MX_CHECK(blur_sigma > 0.f && blur_sigma <= 3.0e38f, "sag_blur_taps: blur_sigma must be positive and finite");
  double t[9], sum = 0.0;
  for (int i = 0; i < 9; ++i) { const double x = (double)(i - 4) / (double)blur_sigma; t[i] = std::exp(-0.5 * x * x); sum += t[i]; }
  for (int i = 0; i < 9; ++i) taps[i] = (float)(t[i] / sum);
  return 0;
}

extern "C" int mx_sag_degrade(void* stream, const void* latents, const void* eps, const float* sigma, const unsigned char* mask, int h_m, int w_m,
                              const int* rows, int n_out, int n, int C, int h, int w, float blur_sigma, void* out, int dtype) {
  using namespace mx;
  MX_CHECK(latents && eps && sigma && mask && out, "sag_degrade: null operand");
  MX_CHECK(n_out > 0 && n_out <= kSagMaxRows && n >= n_out && C > 0 && C <= 65535 && h_m > 0 && w_m > 0, "sag_degrade: 1..64 output rows out of n >= that many, C in 1..65535, a mask grid");
  for (int i = 0; i < n_out; ++i) MX_CHECK(!rows || (rows[i] >= 0 && rows[i] < n), "sag_degrade: a row index outside [0, n)");
  MX_CHECK(h > 4 && w > 4, "sag_degrade: reflect padding of 4 needs latents of more than 4 x 4");
  MX_CHECK(dtype == MX_F32 || dtype == MX_F16 || dtype == MX_BF16, "sag_degrade: bad dtype");
  const size_t al = dtype == MX_F32 ? 4 : 2;
  MX_CHECK(aligned_to(latents, al) && aligned_to(eps, al) && aligned_to(out, al) && aligned_to(sigma, 4), "sag_degrade: misaligned operand");
  DegArgs a;
  if (mx_sag_blur_taps(blur_sigma, a.taps)) { set_error("sag_degrade: blur_sigma must be positive and finite"); return 1; }
  a.lat = latents; a.eps = eps; a.out = out; a.sigma = sigma; a.mask = mask;
  for (int i = 0; i < n_out; ++i) a.rows[i] = rows ? rows[i] : i;
  a.C = C; a.h = h; a.w = w; a.hm = h_m; a.wm = w_m; a.tiles_x = cdiv(w, kDegTile);
  const dim3 grid((unsigned)(a.tiles_x * cdiv(h, kDegTile)), (unsigned)C, (unsigned)n_out), block(256);
  hipStream_t st = (hipStream_t)stream;
  return with_io_dtype(dtype, "sag_degrade", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((sag_degrade_kernel<T>), grid, block, 0, st, a);
    MX_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int mx_sag_fold(void* stream, void* noise, const void* eps_d, const float* coef, const int* rows, int n_out, int n, int64_t elems, int dtype) {
  using namespace mx;
  MX_CHECK(noise && eps_d && coef, "sag_fold: null operand");
  MX_CHECK(n_out > 0 && n_out <= kSagMaxRows && n >= n_out && elems > 0, "sag_fold: 1..64 SAG rows out of n >= that many requests");
  FoldArgs f;
  for (int i = 0; i < n_out; ++i) {
    MX_CHECK(!rows || (rows[i] >= 0 && rows[i] < n), "sag_fold: a row index outside [0, n)");
    MX_CHECK(coef[i] == coef[i], "sag_fold: NaN factor");
    f.rows[i] = rows ? rows[i] : i; f.coef[i] = coef[i];
    for (int j = 0; j < i; ++j) MX_CHECK(f.rows[j] != f.rows[i], "sag_fold: a row index twice (two workgroup rows would update one conditional row)");
  }
  MX_CHECK(dtype == MX_F32 || dtype == MX_F16 || dtype == MX_BF16, "sag_fold: bad dtype");
  const size_t al = dtype == MX_F32 ? 4 : 2;
  MX_CHECK(aligned_to(noise, al) && aligned_to(eps_d, al), "sag_fold: misaligned operand");
  const dim3 grid((unsigned)cdiv64(elems, 256), (unsigned)n_out), block(256);
  hipStream_t st = (hipStream_t)stream;
  return with_io_dtype(dtype, "sag_fold", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((sag_fold_kernel<T>), grid, block, 0, st, (T*)noise, (const T*)eps_d, f, n, (long)elems);
    MX_LAUNCH_CHECK();
    return 0;
  });
}
