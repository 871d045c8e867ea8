// The first launch of the CLIP vision encoder: the patch embedding (a P x P convolution at stride P, no bias) read from the client's image itself --
// 8-bit interleaved RGB with a row stride and a per-image stride in bytes, so a centre crop is a pointer offset -- plus the position rows and the class
// token, in ONE launch:
//     x[b, 1 + p, :] = W . vec(normalise(patch_p)) + pos[1 + p, :]          x[b, 0, :] = cls + pos[0, :]
// normalise(u) = (u / 255 - mean_c) / std_c in fp32, operation by operation, rounded once to bf16 (the rule of conv_rgb_in.hip for 2 (u / 255) - 1).
// Neither the normalised image nor an im2col matrix reaches HBM.
// As a GEMM it is M = patches, K = 3 P P in (row, column, channel) order -- for a fixed patch row ky the 3 P values of a patch are 3 P consecutive
// bytes of one image row -- zero-padded by the packer to ldw, a multiple of 32 (P = 14: 588 -> 608 = 19 k-steps of v_mfma_f32_16x16x32_bf16).
// A workgroup owns 16 consecutive patches of one patch row:
//   1. the P image rows it needs are staged in LDS as BYTES, coalesced (14 x 16 x 42 = 9.4 KB), next to a 3 x 256 table of the normalised values
//      (each entry formed by the exact fp32 expression: the table IS the conversion, one division per entry instead of one per pixel and wave);
//   2. the bytes are converted on the fragment read: every B fragment (16 patches x 32 k) of the tile is built once, in the register order of the
//      matrix instruction, 16 bytes per lane;
//   3. its four waves walk the output features in chunks of 256 (64 per wave, four accumulators in flight), A = weight rows straight from global
//      memory (L2: every workgroup reads the same 1.5 MB), B = one 16-byte LDS word per k-step;
//   4. the position row is added in fp32, the sum is rounded once, and the results leave through a wave-private LDS patch as whole 16-byte pieces.
// Ragged tiles (a grid width that is no multiple of 16): columns past the grid are never read from the image (zero bytes in LDS) and never stored.
#include <algorithm>

#include "common.h"
#include "../../include/mxdenoise.h"

// bytes -> value is evaluated operation by operation (t = u / 255; (t - mean) / std): no contraction in this translation unit
#pragma clang fp contract(off)

namespace mx {

constexpr int kPeChunk = 256;                   // output features of a workgroup pass: 4 waves x 4 blocks of 16
constexpr int kPePatch = 64 * 2 + 16;           // bytes per patch of a wave's output staging: 64 features + 16 of padding
constexpr int kPePerCu = 2;                     // workgroups a launch aims at per CU

struct PatchEmbedArgs {
  const unsigned char* image; long row_stride, image_stride;
  const bf16_t* w; const bf16_t* cls; const bf16_t* pos; bf16_t* x;
  int ldw, B, GH, GW, P, N, tiles_x, ksteps;
  float mean[3], std[3];
};

static inline int pe_stage_bytes(int P) { return (P * 16 * 3 * P + 15) & ~15; }
static inline int pe_lds_bytes(int P, int ksteps) { return pe_stage_bytes(P) + 768 * 2 + ksteps * 1024 + 4 * 16 * kPePatch; }

__global__ __launch_bounds__(256) void patch_embed_u8_kernel(const PatchEmbedArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int P = p.P, N = p.N, GW = p.GW, P3 = 3 * P, rowb = 16 * P3, K = P3 * P;
  const int stage_bytes = (P * rowb + 15) & ~15;
  unsigned char* stage = reinterpret_cast<unsigned char*>(smem);                     // [P][16 patches][3 P] bytes
  bf16_t* lut = reinterpret_cast<bf16_t*>(smem + stage_bytes);                       // [3][256]
  u32x4* frag = reinterpret_cast<u32x4*>(smem + stage_bytes + 768 * 2);              // [ksteps][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  char* patch = smem + stage_bytes + 768 * 2 + p.ksteps * 1024 + wave * (16 * kPePatch);
  const int tx = blockIdx.x % p.tiles_x, gy = (blockIdx.x / p.tiles_x) % p.GH, b = blockIdx.x / (p.tiles_x * p.GH);
  const int gx0 = tx * 16;
  const int ncols = std::min(16, GW - gx0);
  const int T = 1 + p.GH * GW;

  // 1. the tile's image bytes and the value table
  const unsigned char* src = p.image + b * p.image_stride + (long)gy * P * p.row_stride + (long)gx0 * P3;
  for (int idx = tid; idx < P * rowb; idx += 256) {
    const int ky = idx / rowb, xb = idx - ky * rowb;
    stage[idx] = xb < ncols * P3 ? src[ky * p.row_stride + xb] : (unsigned char)0;
  }
  for (int idx = tid; idx < 768; idx += 256) {
    const int c = idx >> 8;
    const float t = (float)(idx & 255) / 255.0f;
    lut[idx] = f32_to_bf16((t - p.mean[c]) / p.std[c]);
  }
  __syncthreads();
  // 2. B fragments: element e of lane (j, kq) of k-step s is column k = 32 s + 8 kq + e = (ky P + kx) 3 + c of patch j
  for (int f = tid; f < p.ksteps * 64; f += 256) {
    const int fj = f & 15, k0 = (f >> 6) * 32 + ((f >> 4) & 3) * 8;
    bf16_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = k0 + e, ky = k / P3, m = k - ky * P3;
      v[e] = k < K ? lut[(k % 3) * 256 + stage[ky * rowb + fj * P3 + m]] : (bf16_t)0;
    }
    frag[f] = u32x4{(unsigned)v[0] | ((unsigned)v[1] << 16), (unsigned)v[2] | ((unsigned)v[3] << 16), (unsigned)v[4] | ((unsigned)v[5] << 16),
                    (unsigned)v[6] | ((unsigned)v[7] << 16)};
  }
  __syncthreads();

  // 3. / 4. feature chunks
  const int nchunks = (N + kPeChunk - 1) / kPeChunk;
  const int pcol = std::min(gx0 + j, GW - 1);                      // this lane's patch (clamped: a column past the grid is computed and dropped)
  const long tok0 = (long)b * T + 1 + (long)gy * GW;               // token row of grid column 0
  for (int chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
    if (gy == 0 && tx == 0) {                                      // the class row of image b
      const int n = chunk * kPeChunk + tid;
      if (n < N) p.x[(long)b * T * N + n] = f32_to_bf16(bf16_to_f32(p.cls[n]) + bf16_to_f32(p.pos[n]));
    }
    const int n0 = chunk * kPeChunk + wave * 64;
    const int nb = std::min(4, (N - n0) >> 4);                     // 16-feature blocks of this wave (wave-uniform; N % 16 == 0: the launcher)
    if (nb <= 0) continue;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16_t* wp = p.w + (long)(n0 + j) * p.ldw + 8 * kq;      // A: lane (j, kq) holds weight row n0 + 16 i + j, columns 32 s + 8 kq .. + 7
    for (int s = 0; s < p.ksteps; ++s) {
      const bf16x8 xf = __builtin_bit_cast(bf16x8, frag[s * 64 + lane]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < nb) {
          const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wp + (long)(16 * i) * p.ldw + 32 * s);
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[i], 0, 0, 0);
        }
      }
    }
    // lane (j, kq) holds features n0 + 16 i + 4 kq + {0..3} of patch gx0 + j
    const bf16_t* pp = p.pos + (long)(1 + gy * GW + pcol) * N + n0 + 4 * kq;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < nb) {
        const u32x2 pv = *reinterpret_cast<const u32x2*>(pp + 16 * i);
        *reinterpret_cast<u32x2*>(patch + j * kPePatch + (16 * i + 4 * kq) * 2) =
            u32x2{pack_bf16x2(acc[i][0] + bf16lo_to_f32(pv[0]), acc[i][1] + bf16hi_to_f32(pv[0])),
                  pack_bf16x2(acc[i][2] + bf16lo_to_f32(pv[1]), acc[i][3] + bf16hi_to_f32(pv[1]))};
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // (one wave: its LDS operations complete in order)
    const int per_px = 2 * nb;                                     // 16-byte pieces of a patch in this wave's 64 features
    for (int piece = lane; piece < 16 * per_px; piece += 64) {
      const int pj = piece / per_px, c16 = piece - pj * per_px;
      const u32x4 o = *reinterpret_cast<const u32x4*>(patch + pj * kPePatch + c16 * 16);
      if (pj < ncols) *reinterpret_cast<u32x4*>(p.x + (tok0 + gx0 + pj) * N + n0 + c16 * 8) = o;
    }
  }
}

}  // namespace mx

extern "C" int mx_patch_embed_u8(void* stream, const void* image, int64_t row_stride, int64_t image_stride, const void* w, int ldw, const void* cls,
                                 const void* pos, void* x, int B, int GH, int GW, int P, int N, const float* mean, const float* std3) {
  MX_CHECK(image && w && cls && pos && x && mean && std3, "patch_embed_u8: null operand");
  MX_CHECK(B > 0 && GH > 0 && GW > 0 && P > 0 && N > 0, "patch_embed_u8: sizes must be positive");
  MX_CHECK(N % 16 == 0, "patch_embed_u8: N must be a multiple of 16");
  const int K = 3 * P * P, ksteps = (K + 31) / 32;
  MX_CHECK(P <= 32 && mx::pe_lds_bytes(P, ksteps) <= 64 * 1024, "patch_embed_u8: a tile of this patch size does not fit in 64 KB of LDS");
  MX_CHECK(ldw >= 32 * ksteps && ldw % 8 == 0, "patch_embed_u8: ldw must cover 3 P P rounded up to 32 (the packer zero-pads) and be a multiple of 8");
  MX_CHECK(row_stride >= (int64_t)GW * P * 3 && image_stride >= 0, "patch_embed_u8: the row stride is shorter than the grid's bytes");
  MX_CHECK(mx::aligned_to(w, 16) && mx::aligned_to(pos, 16) && mx::aligned_to(x, 16) && mx::aligned_to(cls, 2), "patch_embed_u8: w, pos and x must be 16-byte aligned");
  MX_CHECK(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "patch_embed_u8: std must not be zero");
  const int tiles_x = mx::cdiv(GW, 16);
  MX_CHECK((long)B * GH * tiles_x < 2147483647L && (long)N * ldw < 2147483647L, "patch_embed_u8: too many tiles");
  mx::PatchEmbedArgs a;
  a.image = (const unsigned char*)image; a.row_stride = row_stride; a.image_stride = image_stride;
  a.w = (const mx::bf16_t*)w; a.cls = (const mx::bf16_t*)cls; a.pos = (const mx::bf16_t*)pos; a.x = (mx::bf16_t*)x;
  a.ldw = ldw; a.B = B; a.GH = GH; a.GW = GW; a.P = P; a.N = N; a.tiles_x = tiles_x; a.ksteps = ksteps;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std3[c]; }
  // every workgroup converts its tile once and walks the feature chunks; the chunks are dealt over blockIdx.y only while the tiles alone leave CUs idle
  const int tiles = B * GH * tiles_x, nchunks = mx::cdiv(N, mx::kPeChunk);
  const int gy = std::min(nchunks, std::max(1, mx::kPePerCu * mx::cu_count() / tiles));
  hipLaunchKernelGGL(mx::patch_embed_u8_kernel, dim3(tiles, gy), dim3(256), mx::pe_lds_bytes(P, ksteps), (hipStream_t)stream, a);
  MX_LAUNCH_CHECK();
  return 0;
}
