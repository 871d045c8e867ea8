// FreeU (diffusers' apply_freeu / fourier_filter, threshold = 1) on NHWC bf16 activations, gfx950: the low-frequency filter of a skip tensor without an
// FFT, and the backbone scaling of the hidden state's first half, in ONE launch per application.
//
// The filter multiplies by s the 2 x 2 box of the shifted spectrum, the bins (u, v) in {0, -1} x {0, -1}.  Per (sample, channel) plane that is
//   y = x + (s - 1) / (H W) * Re( sum_{u,v} X[u,v] e^{+2 pi i (u h / H + v w / W)} ),   X[u,v] = sum x[h,w] e^{-2 pi i (u h / H + v w / W)}:
// seven real sums (X[0,0] is real, only the real part of the result is kept) and a rank-4 correction, separable by rows.  With t_h = 2 pi h / H,
// f_w = 2 pi w / W:
//   reduce  R0[h] = sum_w x, Rc[h] = sum_w x cos f_w, Rs[h] = sum_w x sin f_w;
//           X00 = sum_h R0, X01 = sum_h (Rc + i Rs), X10 = sum_h R0 e^{i t_h}, X11 = sum_h (Rc + i Rs) e^{i t_h}
//   apply   p0[h] = Re(X00 + X10 e^{-i t_h}), q[h] = X01 + X11 e^{-i t_h};  y = x + g (p0[h] + Re q[h] cos f_w + Im q[h] sin f_w), g = (s - 1) / (H W)
// everything in fp32, rounded to bf16 once (diffusers computes in fp32 and casts once).
//
// Work split.  A workgroup owns all H W pixels of a slab of `slab` channels (64, 32 or 16) of one sample: no reduction crosses workgroups, there are no
// atomics.  Lanes run across channels, 16 bytes (8 channels) each: thread = (channel lane cl = tid % (slab / 8), pixel lane pl = tid / (slab / 8)) with
// ALWAYS 64 pixel lanes, so a workgroup has 8 * slab threads.  The plane is cut into H * S items (a row, or 1 / S of a row where H < 64); pixel lane pl
// walks the items pl, pl + 64, ... and the pixels of an item left to right.
// Summation order (fixed, a function of H and W alone -- not of the slab, the batch, the other problems of the launch or the run): a thread adds the
// pixels of an item in order into (R0, Rc, Rs), folds the item into its seven accumulators, and the 64 pixel lanes are added in a balanced xor tree
// (levels inside a wave by cross-lane moves, the levels above through LDS in the same pairing).  Longest chain: n = wseg + items per lane + 6 additions,
// which is what mx_freeu_route reports.
// Data movement.  The reduce pass reads the slab from HBM.  Where the workgroup's pixel visits fit 128 KB of the CU's 160 KB LDS it keeps every 16-byte
// chunk it read in a thread-private LDS slot ([visit][tid]: conflict-free, no barrier needed) and the apply pass reads it from there; otherwise the apply
// pass reads the slab again, from L2 / the memory-side cache.  cos / sin of f_w and t_h are built once per workgroup in LDS, in fp32, each from an exactly
// reduced argument (the octant and the remainder of 8 j / N in integers, an angle in [0, pi / 4]); there is no running rotation.  The seven
// coefficients of every channel live in LDS, the per-row triples in registers.
// Matrix instructions do not fit: the operator is 3 FMAs per element and pass, far below what feeds an MFMA, and a bf16 basis for one would cost the
// accuracy that the fp32 evaluation exists for.  Measured (profiles/freeu.txt) the launches reach 0.13 to 0.24 of their HBM floor:
// what bounds them is not bandwidth but parallelism per plane -- 160 to 320 workgroups, one per CU where the stage takes 128 KB, each thread walking its
// 16 to 64 pixels one 16-byte load after the other, the apply pass behind a barrier.
// Backbone scaling: extra workgroups of the same launch multiply channels [0, C_hidden / 2) of the hidden state by b in fp32, rounded once, in place.
#include <hip/hip_runtime.h>

#include "common.h"

namespace mx {
namespace {

constexpr int kFuPixelLanes = 64;
constexpr int kFuStageBytes = 128 * 1024;   // of the 160 KB: tables, tree scratch and coefficients take up to 24 KB more
constexpr int kFuMaxEdge = 512;             // (the four tables: 8 KB)
constexpr int kFuCUs = 256;                 // MI355X; a constant, so that the route of a shape is the same wherever it is asked
constexpr int kFuScaleVecs = 8;             // 16-byte chunks of the hidden state per thread of a scaling workgroup

struct FuProb {
  const bf16_t* skip; bf16_t* out; bf16_t* hid;
  int B, H, W;
  int S, wseg, ipl;      // segments per row, pixels per segment, items per pixel lane
  int staged;
  long hid_vecs;         // 16-byte chunks of the hidden state's first half
  float g;               // (s - 1) / (H W)
};
struct FuArgs {
  FuProb p[MX_MAX_SEGS];
  int blk0[MX_MAX_SEGS + 1];     // first filter workgroup of every problem
  int sblk0[MX_MAX_SEGS + 1];    // first scaling workgroup of every problem (behind all filter workgroups)
  int n, C, Ch, slab;
  float b;
};

// how problem (B, H, W) is cut into items, and whether its visits fit the stage
void fu_geometry(FuProb& q, int slab) {
  int S = 1;
  while (2 * S * q.H <= kFuPixelLanes && 2 * S <= q.W) S *= 2;
  q.S = S; q.wseg = cdiv(q.W, S); q.ipl = cdiv(q.H * S, kFuPixelLanes);
  q.staged = (long)q.ipl * q.wseg * kFuPixelLanes * slab * 2 <= kFuStageBytes ? 1 : 0;
}
// THE route: the slab width of a launch and, per problem, whether the slab is staged in LDS.
//   slab   = the widest of 64 / 32 / 16 channels that divides C and still gives every one of the 256 CUs a workgroup (sum of B * C / slab >= 256); where
//            none does, the narrowest that divides C: a wide slab reads whole 128-byte lines per pixel, but a launch of 80 workgroups leaves two thirds
//            of the CUs idle, and the measured launches are bound by the number of threads walking pixels, not by bandwidth (header).  The bits do
//            not depend on the choice.
//   staged = the pixel visits of a workgroup (items per lane x pixels per item x 64 lanes, >= H W) x slab x 2 bytes fit 128 KB.
//            SDXL-base at 8 x 1024 px: 32 x 32 planes are staged at every slab (64 KB at slab 32); 64 x 64 planes are staged at slab 16 (128 KB) and read
//            twice at slab 32 / 64; anything above 64 x 64 x 16 is read twice.
int fu_route(FuProb* p, int n, int C) {
  int slab = 0;
  for (int cand : {64, 32, 16}) {
    if (C % cand) continue;
    long wgs = 0;
    for (int i = 0; i < n; ++i) wgs += (long)p[i].B * (C / cand);
    slab = cand;
    if (wgs >= kFuCUs) break;
  }
  for (int i = 0; i < n; ++i) fu_geometry(p[i], slab);
  return slab;
}

// cos, sin of 2 pi j / N for 0 <= j < N: 8 j / N = k + r / N in integers, the angle inside its octant pair in [0, pi / 4], then quarter turns.
// Multiples of pi / 2 come out exact (N = 2: the Nyquist bin is (-1, 0)).
__device__ __forceinline__ void fu_cos_sin(int j, int N, float& c, float& s) {
  const int k = (8 * j) / N, r = 8 * j - k * N;
  const bool odd = k & 1;
  const float a = 0.78539816339744831f * ((float)(odd ? N - r : r) / (float)N);
  const float cd = cosf(a), sd = odd ? -sinf(a) : sinf(a);       // the angle = m * pi / 2 + d, d = +a or -a
  switch (((k + 1) >> 1) & 3) {
    case 0: c = cd; s = sd; break;
    case 1: c = -sd; s = cd; break;
    case 2: c = -cd; s = -sd; break;
    default: c = sd; s = -cd; break;
  }
}

__global__ __launch_bounds__(512) void freeu_kernel(const FuArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int slab = A.slab, CL = slab >> 3;
  int blk = blockIdx.x;

  if (blk >= A.blk0[A.n]) {          // ---- backbone scaling: hid[:, :Ch / 2] *= b ----
    blk -= A.blk0[A.n];
    int g = 0;
#pragma unroll
    for (int i = 1; i < MX_MAX_SEGS; ++i) if (i < A.n && blk >= A.sblk0[i]) g = i;
    const FuProb& P = A.p[g];
    const int hv = A.Ch >> 4;        // chunks per pixel
    long v = ((long)(blk - A.sblk0[g]) * kFuScaleVecs) * nthr + tid;
#pragma unroll
    for (int k = 0; k < kFuScaleVecs; ++k, v += nthr) {
      if (v >= P.hid_vecs) break;
      const long row = v / hv;
      u32x4* q = reinterpret_cast<u32x4*>(P.hid + row * A.Ch + (v - row * hv) * 8);
      float x[8];
      unpack_bf16x8(*q, x);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] *= A.b;
      *q = pack_bf16x8(x);
    }
    return;
  }

  // ---- the filter: one (sample, slab) ----
  int g = 0;
#pragma unroll
  for (int i = 1; i < MX_MAX_SEGS; ++i) if (i < A.n && blk >= A.blk0[i]) g = i;
  const FuProb& P = A.p[g];
  const int H = P.H, W = P.W, C = A.C, S = P.S, wseg = P.wseg;
  const int nsl = C / slab;
  const int local = blk - A.blk0[g];
  const int bi = local / nsl, sl = local - bi * nsl;
  const int cl = tid % CL, pl = tid / CL;
  const long plane = (long)bi * H * W * C + (long)sl * slab + cl * 8;
  const bf16_t* src = P.skip + plane;
  bf16_t* dst = P.out + plane;

  u32x4* stage = reinterpret_cast<u32x4*>(smem);                                    // [ipl * wseg][nthr] chunks (staged problems)
  const size_t stage_bytes = P.staged ? (size_t)P.ipl * wseg * nthr * 16 : 0;
  float* cw = reinterpret_cast<float*>(smem + stage_bytes);                         // cos, sin of f_w and t_h
  float* sw = cw + W;
  float* chh = sw + W;
  float* shh = chh + H;
  float* red = shh + H;                                                             // [waves][7][slab]
  float* coef = red + CL * 7 * slab;                                                // [7][slab]

  for (int j = tid; j < W; j += nthr) fu_cos_sin(j, W, cw[j], sw[j]);
  for (int j = tid; j < H; j += nthr) fu_cos_sin(j, H, chh[j], shh[j]);
  __syncthreads();

  // reduce: X00 | X01 re, im | X10 re, im | X11 re, im per channel
  float acc[7][8];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
  const int items = H * S;
  for (int it = pl, n_it = 0; it < items; it += kFuPixelLanes, ++n_it) {
    const int h = it / S, w0 = (it - h * S) * wseg, w1 = min(W, w0 + wseg);
    float r0[8], rc[8], rs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { r0[e] = 0.f; rc[e] = 0.f; rs[e] = 0.f; }
    const bf16_t* rowp = src + (long)h * W * C;
#pragma unroll 4
    for (int w = w0; w < w1; ++w) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(rowp + (long)w * C);
      if (P.staged) stage[(size_t)(n_it * wseg + (w - w0)) * nthr + tid] = v;
      float x[8];
      unpack_bf16x8(v, x);
      const float c = cw[w], s = sw[w];
#pragma unroll
      for (int e = 0; e < 8; ++e) { r0[e] += x[e]; rc[e] = fmaf(x[e], c, rc[e]); rs[e] = fmaf(x[e], s, rs[e]); }
    }
    const float ch = chh[h], sh = shh[h];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc[0][e] += r0[e]; acc[1][e] += rc[e]; acc[2][e] += rs[e];
      acc[3][e] = fmaf(r0[e], ch, acc[3][e]); acc[4][e] = fmaf(r0[e], sh, acc[4][e]);
      acc[5][e] += rc[e] * ch - rs[e] * sh; acc[6][e] += rc[e] * sh + rs[e] * ch;
    }
  }
  // the balanced tree over the 64 pixel lanes: pixel lane = wave * (64 / CL) + (lane / CL), so the low levels pair lanes of one wave ...
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      for (int o = CL; o < kWave; o <<= 1) acc[k][e] += __shfl_xor(acc[k][e], o, kWave);
  const int lane = tid & (kWave - 1), wave = tid >> 6;
  if (lane < CL) {
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[(wave * 7 + k) * slab + cl * 8 + e] = acc[k][e];
  }
  __syncthreads();
  // ... and the high levels pair waves (CL of them: 8, 4 or 2), in the same xor order
  if (tid < 7 * slab) {
    float v[8];
#pragma unroll
    for (int wv = 0; wv < 8; ++wv) v[wv] = wv < CL ? red[wv * 7 * slab + tid] : 0.f;
#pragma unroll
    for (int st = 1; st < 8; st <<= 1)
#pragma unroll
      for (int i = 0; i < 8; i += 2 * st) if (i + st < CL) v[i] += v[i + st];
    coef[tid] = v[0];
  }
  __syncthreads();

  // apply
  float X[7][8];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) X[k][e] = coef[k * slab + cl * 8 + e];
  const float gg = P.g;
  for (int it = pl, n_it = 0; it < items; it += kFuPixelLanes, ++n_it) {
    const int h = it / S, w0 = (it - h * S) * wseg, w1 = min(W, w0 + wseg);
    const float ch = chh[h], sh = shh[h];
    float p0[8], qr[8], qi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      p0[e] = X[0][e] + X[3][e] * ch + X[4][e] * sh;
      qr[e] = X[1][e] + X[5][e] * ch + X[6][e] * sh;
      qi[e] = X[2][e] + X[6][e] * ch - X[5][e] * sh;
    }
    const long rowo = (long)h * W * C;
#pragma unroll 4
    for (int w = w0; w < w1; ++w) {
      const u32x4 v = P.staged ? stage[(size_t)(n_it * wseg + (w - w0)) * nthr + tid] : *reinterpret_cast<const u32x4*>(src + rowo + (long)w * C);
      float x[8];
      unpack_bf16x8(v, x);
      const float c = cw[w], s = sw[w];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] += gg * (p0[e] + qr[e] * c + qi[e] * s);
      *reinterpret_cast<u32x4*>(dst + rowo + (long)w * C) = pack_bf16x8(x);
    }
  }
}

int fu_check(const mx_freeu_problem* probs, int n, int C_skip, int C_hidden, FuProb* p) {
  MX_CHECK(probs != nullptr && n >= 1 && n <= MX_MAX_SEGS, "freeu: 1..MX_MAX_SEGS problems");
  MX_CHECK(C_skip > 0 && C_skip % 16 == 0, "freeu: the skip's channels must be a multiple of 16");
  MX_CHECK(C_hidden >= 0 && C_hidden % 16 == 0, "freeu: the hidden state's channels must be a multiple of 16");
  for (int i = 0; i < n; ++i) {
    const mx_freeu_problem& q = probs[i];
    MX_CHECK(q.B >= 1 && q.H >= 2 && q.W >= 2, "freeu: a problem needs B >= 1 and H, W >= 2");
    MX_CHECK(q.H <= kFuMaxEdge && q.W <= kFuMaxEdge, "freeu: H, W up to 512");
    MX_CHECK(q.skip && q.skip_out, "freeu: skip and skip_out are required");
    MX_CHECK((q.hidden != nullptr) == (C_hidden > 0), "freeu: hidden and C_hidden come together");
    // filter workgroups read skip and write skip_out while scaling workgroups of the same launch write hidden: the three must not overlap
    const size_t px = (size_t)q.B * q.H * q.W * 2;
    auto apart = [](const void* a, size_t na, const void* b, size_t nb) { return (uintptr_t)a + na <= (uintptr_t)b || (uintptr_t)b + nb <= (uintptr_t)a; };
    MX_CHECK(apart(q.skip, px * C_skip, q.skip_out, px * C_skip) && (!q.hidden || (apart(q.hidden, px * C_hidden, q.skip, px * C_skip) &&
             apart(q.hidden, px * C_hidden, q.skip_out, px * C_skip))), "freeu: skip, skip_out and hidden must not overlap");
    MX_CHECK(aligned_to(q.skip, 16) && aligned_to(q.skip_out, 16) && aligned_to(q.hidden, 16), "freeu: operands must be 16-byte aligned");
    p[i] = FuProb{};
    p[i].skip = (const bf16_t*)q.skip; p[i].out = (bf16_t*)q.skip_out; p[i].hid = (bf16_t*)q.hidden;
    p[i].B = q.B; p[i].H = q.H; p[i].W = q.W;
  }
  return 0;
}

}  // namespace
}  // namespace mx

extern "C" int mx_freeu_route(const mx_freeu_problem* probs, int n, int C_skip, int* slab, int* staged, int* chain) {
  using namespace mx;
  MX_CHECK(probs != nullptr && n >= 1 && n <= MX_MAX_SEGS && C_skip > 0 && C_skip % 16 == 0, "freeu_route: bad arguments");
  FuProb p[MX_MAX_SEGS];
  for (int i = 0; i < n; ++i) {
    MX_CHECK(probs[i].B >= 1 && probs[i].H >= 2 && probs[i].W >= 2, "freeu_route: a problem needs B >= 1 and H, W >= 2");
    p[i] = FuProb{}; p[i].B = probs[i].B; p[i].H = probs[i].H; p[i].W = probs[i].W;
  }
  const int sl = fu_route(p, n, C_skip);
  if (slab) *slab = sl;
  for (int i = 0; i < n; ++i) {
    if (staged) staged[i] = p[i].staged;
    if (chain) chain[i] = p[i].wseg + p[i].ipl + 6;
  }
  return 0;
}

extern "C" int mx_freeu(void* stream, const mx_freeu_problem* probs, int n, int C_skip, int C_hidden, float s, float b) {
  using namespace mx;
  FuArgs A{};
  if (fu_check(probs, n, C_skip, C_hidden, A.p)) return 1;
  A.n = n; A.C = C_skip; A.Ch = C_hidden; A.b = b;
  A.slab = fu_route(A.p, n, C_skip);
  const int nthr = 8 * A.slab;
  size_t lds = 0;
  int blk = 0, sblk = 0;
  for (int i = 0; i < n; ++i) {
    FuProb& q = A.p[i];
    q.g = (float)(((double)s - 1.0) / ((double)q.H * q.W));
    q.hid_vecs = q.hid ? (long)q.B * q.H * q.W * (C_hidden / 16) : 0;
    A.blk0[i] = blk; A.sblk0[i] = sblk;
    blk += q.B * (C_skip / A.slab);
    sblk += (int)cdiv64(q.hid_vecs, (int64_t)nthr * kFuScaleVecs);
    const size_t need = (q.staged ? (size_t)q.ipl * q.wseg * nthr * 16 : 0) + (size_t)(2 * q.W + 2 * q.H + (A.slab / 8 + 1) * 7 * A.slab) * sizeof(float);
    lds = std::max(lds, need);
  }
  for (int i = n; i <= MX_MAX_SEGS; ++i) { A.blk0[i] = blk; A.sblk0[i] = sblk; }
  MX_CHECK(lds <= 160 * 1024, "freeu: LDS budget exceeded");
  hipLaunchKernelGGL(freeu_kernel, dim3(blk + sblk), dim3(nthr), lds, (hipStream_t)stream, A);
  MX_LAUNCH_CHECK();
  return 0;
}
