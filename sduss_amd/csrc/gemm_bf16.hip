// bf16 MFMA GEMM and implicit-GEMM 3x3 convolution for gfx950 (MI355X, CDNA4).
//
//   C[M, N] = X[M, K] * W[N, K]^T  (+ bias, + per-sample row bias, + residual, SiLU | GEGLU | QKV split)
//
// Orientation: the WEIGHT tile is the MFMA "A" operand and the ACTIVATION tile the "B" operand, so
// the accumulator of v_mfma_f32_16x16x32_bf16 (col = lane&15, row = 4*(lane>>4)+reg) holds, per lane,
// four CONSECUTIVE output features n of ONE token m: the epilogue stores 8 bytes per lane row-major
// and fuses bias / residual / activation without a transpose; the transposed V^T store that the
// attention kernel wants is the lane-contiguous direction (MI355X-first choice: no LDS round trip).
//
// Tile: 128 tokens x BN features (BN = 128 or 64) x BK = 64, 256 threads = 4 waves as 2(m) x 2(n);
// LDS rows are 128 B with the 16-byte chunk index XOR-swizzled by ((row>>1)&7), which makes the
// ds_read_b128 fragment reads of the 16x16x32 operand conflict-free (cdna guide T2, lane groups of
// ds_read_b128).  Register-prefetch double buffering, one barrier per K tile.
//
// Implicit GEMM conv (CONV=true): K = 9*Cin ordered tap-major, activations NHWC; the loader turns an
// output pixel + tap into a source pixel (stride 1/2, fused nearest x2 upsample, zero padding, and the
// reference's sliced-mode halo-corner rule -- see mxdenoise.h) and reads 16 B of channels from it.
//
// Reference call sites this serves: F.linear / F.conv2d issued by sduss/model_executor/modules/
// resnet.py:106,132,163 and attention.py:73-96,148-151,220 (through un-vendored diffusers/torch).
//
// This file holds the generic kernel and its launcher only.  What a descriptor runs, validation and the launch are in gemm_dispatch.cpp.
#include "common.h"
#include "../../include/mxdenoise.h"
#include "gemm_args.h"
#include "gemm_forms.h"

namespace mx {

constexpr int BM = 128;
constexpr int BK = 64;

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

template <int BN, bool CONV>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const GemmArgs pk) {
  constexpr int NI = BN / 32;  // 16-wide feature blocks per wave (wave covers BN/2 features)
  constexpr int MI = 4;        // 16-wide token blocks per wave (wave covers 64 tokens)
  constexpr int WROWS = BN / 32;  // W rows staged per thread
  __shared__ __attribute__((aligned(16))) bf16_t sX[2][BM * BK];
  __shared__ __attribute__((aligned(16))) bf16_t sW[2][BN * BK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1;  // token half
  const int wn = wave & 1;   // feature half
  GemmArgs p = pk;              // grouped launch (gemm_args.h): blockIdx.x counts the m-tiles of all problems; p becomes this tile's problem
  int tm = blockIdx.x;
  gemm_select_seg(p, pk, tm);
  const int m0 = tm * BM;
  const int n0 = blockIdx.y * BN;
  const int nk = p.K / BK;

  // ---- staging assignment: thread -> (row = (tid>>3) + 32*i, chunk = tid&7) ----
  const int srow = tid >> 3;
  const int sch = tid & 7;

  // activation row descriptors
  int xoff[4];           // GEMM: element offset of the row start (or -1 when the row is out of range)
  int xoff2[4];          // the same inside a2 (dual-source A operand)
  int cb[4], cy[4], cx[4];  // CONV: batch, centre y/x in virtual-input coordinates (cb = -1: invalid row)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + srow + 32 * i;
    if constexpr (!CONV) {
      xoff[i] = (m < p.M) ? (int)(gemm_in_row(p, m) * p.lda) + sch * 8 : -1;
      xoff2[i] = (p.a2 != nullptr && m < p.M) ? m * p.lda2 + sch * 8 : 0;
    } else {
      if (m < p.M) {
        const int hw = p.Hout * p.Wout;
        const int b = m / hw;
        const int r = m - b * hw;
        const int oy = r / p.Wout;
        cb[i] = b;
        cy[i] = oy * p.stride;
        cx[i] = (r - oy * p.Wout) * p.stride;
      } else {
        cb[i] = -1; cy[i] = 0; cx[i] = 0;
      }
    }
  }
  int woff[WROWS];
#pragma unroll
  for (int i = 0; i < WROWS; ++i) {
    const int n = n0 + srow + 32 * i;
    woff[i] = (n < p.N) ? n * p.K + sch * 8 : -1;
  }

  u32x4 rx[4], rw[WROWS];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  auto load_tile = [&](int kt) {
    const int k0 = kt * BK;
    if constexpr (!CONV) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (p.a2 != nullptr && k0 >= p.k_split) rx[i] = (xoff[i] >= 0) ? *reinterpret_cast<const u32x4*>(p.a2 + xoff2[i] + (k0 - p.k_split)) : zero4;
        else rx[i] = (xoff[i] >= 0) ? *reinterpret_cast<const u32x4*>(p.a + xoff[i] + k0) : zero4;
      }
    } else {
      const int tap = k0 / p.Cin;
      const int c0 = k0 - tap * p.Cin;
      const int dy = tap / 3 - 1;
      const int dx = tap - (tap / 3) * 3 - 1;
      const int Hv = p.Hin << p.up, Wv = p.Win << p.up;
      const int P = p.corner_patch;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int iy = cy[i] + dy;
        const int ix = cx[i] + dx;
        if (P > 0 && dy != 0 && dx != 0) {
          // halo-corner rule of the reference's sliced path (norm_silu_concat.cu:210-221, 228-239)
          const bool cross_r = ((iy + P) / P) != ((cy[i] + P) / P);
          const bool cross_c = ((ix + P) / P) != ((cx[i] + P) / P);
          if (cross_r && cross_c) iy = cy[i];
        }
        const bool ok = (cb[i] >= 0) && (iy >= -p.vhalo) && (iy < Hv + p.vhalo) && (ix >= 0) && (ix < Wv);
        if (ok) {
          const long src = (((long)cb[i] * (p.Hin + 2 * p.vhalo) + (iy >> p.up) + p.vhalo) * p.Win + (ix >> p.up)) * p.Cin + c0 + sch * 8;
          rx[i] = *reinterpret_cast<const u32x4*>(p.a + src);
        } else {
          rx[i] = zero4;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < WROWS; ++i)
      rw[i] = (woff[i] >= 0) ? *reinterpret_cast<const u32x4*>(p.w + woff[i] + k0) : zero4;
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = srow + 32 * i;
      *reinterpret_cast<u32x4*>(&sX[buf][row * BK + swz(row, sch) * 8]) = rx[i];
    }
#pragma unroll
    for (int i = 0; i < WROWS; ++i) {
      const int row = srow + 32 * i;
      *reinterpret_cast<u32x4*>(&sW[buf][row * BK + swz(row, sch) * 8]) = rw[i];
    }
  };

  f32x4 acc[NI][MI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15;  // row inside a 16-row fragment
  const int fq = lane >> 4;  // 16-byte chunk inside the 32-deep k-step

  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 wf[NI], xf[MI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int row = wn * (BN / 2) + i * 16 + fr;
        wf[i] = *reinterpret_cast<const bf16x8*>(&sW[buf][row * BK + swz(row, ks * 4 + fq) * 8]);
      }
#pragma unroll
      for (int j = 0; j < MI; ++j) {
        const int row = wm * 64 + j * 16 + fr;
        xf[j] = *reinterpret_cast<const bf16x8*>(&sX[buf][row * BK + swz(row, ks * 4 + fq) * 8]);
      }
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tile(buf ^ 1);
    __syncthreads();
  }

  gemm_epilogue<NI, MI, BN>(p, acc, m0 + wm * 64, n0 + wn * (BN / 2), fr, fq);
}

// the generic launcher: the instantiation `form` (gemm_forms.h) the route names (gemm_dispatch.cpp), one workgroup per BM x BN tile
int launch_generic(hipStream_t s, const GemmArgs& a, int form) {
  const int mt = a.nseg > 0 ? a.mt_total : cdiv(a.M, BM);
  switch (form) {
#define MX_GEN(id, k, targs) case id: hipLaunchKernelGGL((k<MX_FORM_UNPAREN targs>), dim3(mt, cdiv(a.N, MX_FORM_FIRST targs)), dim3(256), 0, s, a); return 0;
    MX_GEMM_GENERIC_FORMS(MX_GEN)
#undef MX_GEN
    default: return 1;
  }
}

}  // namespace mx
