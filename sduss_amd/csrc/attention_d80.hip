// Non-causal softmax attention for heads of 80 (OpenCLIP ViT-H/14, the image encoder of the SDXL IP-Adapter checkpoints: 1280 / 16), short
// sequences (the encoder's L = 257): softmax(q k^T / sqrt(80)) v per (batch, head), bf16 in, fp32 softmax, bf16 out.  Not a width of the
// 64-wide kernels of attention.hip: the shape decides the design.
//   * RESIDENT K / V.  A head's whole K and V (2 x 257 x 160 bytes = 82 KB) fit in the workgroup's LDS, so a workgroup of four waves stages
//     them ONCE -- K row-major, V transposed on the way in -- and its waves walk 16-query blocks against them.  There is no key-tile ring
//     and no online softmax: with every key at hand a block's row maxima are found by one pass of Q K^T (pass 1), and pass 2 recomputes
//     the scores, exponentiates against the final maximum and feeds P V -- no accumulator is ever rescaled.  The second Q K^T costs
//     matrix-core time the exponentials leave idle anyway.
//   * 80 = 2 x 32 + 16.  Q K^T over the head dimension is two v_mfma_f32_16x16x32_bf16 k-steps and one v_mfma_f32_16x16x16_bf16; P V has
//     80 = 5 column blocks of 16.  Nothing is padded to 96 or 128, in memory or in registers.
//   * The scores are computed TRANSPOSED (A = 16 keys, B = 16 queries), so lane (j, kq) holds keys 4 kq .. 4 kq + 3 of query j: two such tiles
//     are, as they stand, the B operand of the 32-key P V step (O^T = V^T P^T).  V^T is staged with the matching key order inside every 32
//     keys (key 16 t + 4 kq + e at slot 8 kq + 4 t + e), so a lane's eight V^T values are one 16-byte LDS word.
//   * Plain operands: q, k, v row-major with leading dimensions -- the [M, 3 hidden] output of ONE mx_gemm serves as it is; the scale
//     1 / sqrt(80) (times log2 e) is applied to the fp32 scores inside the kernel, q is NOT prescaled.
//   * Ragged edges (257 = 16 x 16 + 1: every real launch): keys >= L are zeros in LDS and -inf before the row maximum; query rows >= L read
//     row L - 1 and store nothing.
// LDS rows are padded against bank conflicts (K rows 88 elements = 44 dwords, V^T rows Lp + 8): the 16 rows a b128 read touches fall on 16
// distinct 4-bank groups.  With the padding a head fits up to L = MX_ATTN_D80_MAX_L = 480; above it the launch is refused.
#include <mutex>

#include "common.h"
#include "../../include/mxdenoise.h"

namespace mx {

typedef __attribute__((ext_vector_type(4))) short s16x4;

constexpr int kD80 = 80;
constexpr int kD80KRow = 88;                    // staged K row, elements
constexpr int kD80VPad = 8;                     // staged V^T row = Lp + 8 elements

struct AttnD80Args {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
  int ldq, ldk, ldv, ldo;
  int H, L, Lp;                                  // Lp: L rounded up to 32
  float c;                                       // log2(e) / sqrt(80)
};

__host__ __device__ constexpr int d80_lds_bytes(int Lp) { return (Lp * kD80KRow + kD80 * (Lp + kD80VPad)) * 2; }

__global__ __launch_bounds__(256) void attn_d80_kernel(const AttnD80Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int L = p.L, Lp = p.Lp, vs = Lp + kD80VPad;
  bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);               // [Lp][88]
  bf16_t* Vt = Ks + Lp * kD80KRow;                            // [80][Lp + 8], keys permuted inside every 32
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const long row0 = (long)b * L;

  // ---- stage the head's K (16-byte pieces, a key's ten pieces on consecutive threads) and V^T (consecutive threads = consecutive keys of
  // one 8-dim piece: the eight 2-byte writes of a wave fall into eight rows, 32 dwords each) ----
  for (int idx = tid; idx < Lp * 10; idx += 256) {
    const int key = idx / 10, c = idx - key * 10;
    u32x4 r = {0u, 0u, 0u, 0u};
    if (key < L) r = *reinterpret_cast<const u32x4*>(p.k + (row0 + key) * p.ldk + h * kD80 + c * 8);
    *reinterpret_cast<u32x4*>(Ks + key * kD80KRow + c * 8) = r;
  }
  for (int idx = tid; idx < Lp * 10; idx += 256) {
    const int c = idx / Lp, key = idx - c * Lp;
    u32x4 r = {0u, 0u, 0u, 0u};
    if (key < L) r = *reinterpret_cast<const u32x4*>(p.v + (row0 + key) * p.ldv + h * kD80 + c * 8);
    const int slot = (key & ~31) | (key & 3) | ((key & 16) >> 2) | ((key & 12) << 1);
    bf16_t* dst = Vt + (c * 8) * vs + slot;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dst[(2 * e) * vs] = (bf16_t)(r[e] & 0xffffu);
      dst[(2 * e + 1) * vs] = (bf16_t)(r[e] >> 16);
    }
  }
  __syncthreads();

  const float ninf = -__builtin_huge_valf();
  const int nqb = (L + 15) >> 4;
  for (int qb = blockIdx.x * 4 + wave; qb < nqb; qb += gridDim.x * 4) {
    // B operand of the scores: query qb 16 + j, dims 8 kq .. + 7, 32 + 8 kq .. + 7, 64 + 4 kq .. + 3
    const int qrow = qb * 16 + j;
    const bf16_t* qp = p.q + (row0 + (qrow < L ? qrow : L - 1)) * p.ldq + h * kD80;
    const bf16x8 q0 = *reinterpret_cast<const bf16x8*>(qp + 8 * kq);
    const bf16x8 q1 = *reinterpret_cast<const bf16x8*>(qp + 32 + 8 * kq);
    const s16x4 q2 = *reinterpret_cast<const s16x4*>(qp + 64 + 4 * kq);
    // scores of key tile t, transposed: s[e] = q_j . k_(16 t + 4 kq + e); keys >= L are -inf
    auto scores = [&](int t) __attribute__((always_inline)) {
      const bf16_t* kp = Ks + (16 * t + j) * kD80KRow;
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(kp + 8 * kq);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(kp + 32 + 8 * kq);
      const s16x4 a2 = *reinterpret_cast<const s16x4*>(kp + 64 + 4 * kq);
      f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, q0, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, q1, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a2, q2, s, 0, 0, 0);
      const int key = 16 * t + 4 * kq;
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = key + e < L ? s[e] : ninf;
      return s;
    };
    // pass 1: the row maximum over every key (key 0 always counts: the maximum is finite)
    float m = ninf;
    for (int t = 0; t < Lp / 16; ++t) {
      const f32x4 s = scores(t);
      m = fmaxf(fmaxf(m, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    // pass 2: P = exp2((s - m) c) of 32 keys, its sum, and O^T += V^T P^T
    f32x4 acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    for (int s2 = 0; s2 < Lp / 32; ++s2) {
      const f32x4 sa = scores(2 * s2), sb = scores(2 * s2 + 1);
      float pr[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pr[e] = __builtin_amdgcn_exp2f((sa[e] - m) * p.c);        // (-inf - m) c = -inf: 0
        pr[4 + e] = __builtin_amdgcn_exp2f((sb[e] - m) * p.c);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) l += pr[e];
      const bf16x8 pf = __builtin_bit_cast(bf16x8, pack_bf16x8(pr));
      const bf16_t* vp = Vt + j * vs + 32 * s2 + 8 * kq;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vp + (16 * i) * vs);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[i], 0, 0, 0);
      }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    // lane (j, kq) holds dims 16 i + 4 kq .. + 3 of query j
    if (qrow < L) {
      const float inv = 1.0f / l;
      bf16_t* op = p.o + (row0 + qrow) * p.ldo + h * kD80 + 4 * kq;
#pragma unroll
      for (int i = 0; i < 5; ++i)
        *reinterpret_cast<u32x2*>(op + 16 * i) = u32x2{pack_bf16x2(acc[i][0] * inv, acc[i][1] * inv), pack_bf16x2(acc[i][2] * inv, acc[i][3] * inv)};
    }
  }
}

}  // namespace mx

extern "C" int mx_attention_d80(void* stream, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int B, int H,
                                int L) {
  MX_CHECK(q && k && v && o, "attention_d80: null operand");
  MX_CHECK(B > 0 && H > 0 && L > 0 && B <= 65535 && H <= 65535, "attention_d80: bad shape");
  MX_CHECK(L <= MX_ATTN_D80_MAX_L, "attention_d80: L > " + std::to_string(MX_ATTN_D80_MAX_L) + " is not served (a head's K and V stay resident in LDS)");
  MX_CHECK(ldq >= H * mx::kD80 && ldk >= H * mx::kD80 && ldv >= H * mx::kD80 && ldo >= H * mx::kD80, "attention_d80: a leading dimension is shorter than 80 heads");
  MX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "attention_d80: ldq, ldk, ldv must be multiples of 8 and ldo of 4");
  MX_CHECK(mx::aligned_to(q, 16) && mx::aligned_to(k, 16) && mx::aligned_to(v, 16) && mx::aligned_to(o, 8), "attention_d80: q, k, v must be 16-byte and o 8-byte aligned");
  MX_CHECK((long)B * L * std::max(std::max(ldq, ldk), std::max(ldv, ldo)) < 2147483647L, "attention_d80: operand exceeds 32-bit indexing");
  mx::AttnD80Args a;
  a.q = (const mx::bf16_t*)q; a.k = (const mx::bf16_t*)k; a.v = (const mx::bf16_t*)v; a.o = (mx::bf16_t*)o;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.H = H; a.L = L; a.Lp = (L + 31) / 32 * 32;
  a.c = 1.4426950408889634f / sqrtf(80.0f);
  static_assert(mx::d80_lds_bytes((MX_ATTN_D80_MAX_L + 31) / 32 * 32) <= 160 * 1024, "the longest head must fit in a workgroup's LDS");
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [] {
    attr = hipFuncSetAttribute((const void*)mx::attn_d80_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, mx::d80_lds_bytes((MX_ATTN_D80_MAX_L + 31) / 32 * 32));
  });
  MX_CHECK(attr == hipSuccess, std::string("attention_d80: ") + hipGetErrorString(attr));
  // query blocks of 64 rows per workgroup; fewer, longer-walking workgroups once the heads alone fill the chip twice (each stages K and V again)
  const int qwg = mx::cdiv(L, 64);
  const int gx = std::min(qwg, std::max(1, 2 * mx::cu_count() / (B * H)));
  hipLaunchKernelGGL(mx::attn_d80_kernel, dim3(gx, H, B), dim3(256), mx::d80_lds_bytes(a.Lp), (hipStream_t)stream, a);
  MX_LAUNCH_CHECK();
  return 0;
}
