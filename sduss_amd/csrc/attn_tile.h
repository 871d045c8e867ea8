// The pieces the attention kernels of attention.hip share.  AttnArgs, pack2 and max_across_halves serve all of them (the short-key body, attn_cross_body.h,
// included); the rest is the 64-key tile of the three tiled kernels -- attn_fwd_kernel, attn_fwd_dma_kernel, attn_fwd64_kernel -- whose layout attention.hip's
// header describes.  A piece is here because it folds away: every kernel that calls it compiles to the registers and the instruction counts it had with the
// piece written out (profiles/attn_tile_pieces.txt).  What differs in its bits or its schedule between the kernels stays in the kernels.
#pragma once
#include <type_traits>
#include "common.h"
#include "../../include/mxdenoise.h"

namespace mx {

struct AttnArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* vt; bf16_t* o;
  int ldq, ldk, ldvt, ldo;
  long vt_bstride;
  int B, H, Lq, Lk;
  float scale_log2;  // scale * log2(e)
  int xcd_map;       // 1: XCD-aware workgroup order (needs B*H % 8 == 0)
  // patch-parallel K / V^T (mx_attention_prescaled_chunked): keys come in `key_chunk`-long chunks gathered from the ranks;
  // chunk c of batch b starts at k + c * k_cstride + b * k_bstride (rows of ldk) and vt + c * vt_cstride + b * vt_bstride
  int key_chunk;     // 0: one contiguous key range per batch
  long k_bstride, k_cstride, vt_cstride;
  int causal;        // 1: key j counts for query i only when j <= i (text encoders; attn_fwd_kernel only)
  const float* bias; // additive score bias [H][Lq][ldb], already in the kernel's log2 domain (T5 relative position bias; attn_fwd_kernel only)
  int ldb;
  int xq_wpb;        // short-key kernel: waves that share the 32-query blocks of one (batch, head) (launch_attention_group deals them so that the launch is ONE round)
};

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ unsigned pack2(float lo, float hi) {   // one v_cvt_pk_bf16_f32
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_t{lo, hi}, bf16x2_t));
}

// max over the two half-waves (lane l and l^32) without the LDS crossbar: v_permlane32_swap exchanges the upper half
// of a with the lower half of b.  Inline asm because the builtin folds its two results when both inputs are one value.
__device__ __forceinline__ float max_across_halves(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}

constexpr int KT = 64;                 // keys per tile
constexpr int kBufBytes = 16384;       // one LDS buffer: K tile (8 KB: 64 rows of 128 B) then V^T tile (8 KB), both with 16-byte chunk ^= (row >> 1) & 7

// Throughout: r = lane & 31 is the query column the lane owns (and its fragment row), hh = lane >> 5 its half-wave; element e of score block kb is key
// 32 kb + (e & 3) + 8 (e >> 2) + 4 hh of the tile.

// the lane's part of the queries q0 .. q0 + 31 of (b, head), rows past the end clamped: B operand of S^T = K Q^T, Q[q0 + r][16 ks + 8 hh .. +7]
__device__ __forceinline__ void load_q(const AttnArgs& p, const int b, const int head, const int q0, const int lane, bf16x8 (&qf)[4]) {
  const int r = lane & 31, hh = lane >> 5;
  int qi = q0 + r;
  if (qi > p.Lq - 1) qi = p.Lq - 1;
  const bf16_t* qp = p.q + ((long)b * p.Lq + qi) * p.ldq + head * 64 + hh * 8;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
}

// per-lane read offsets inside a buffer (loop invariant): row r, chunk 2 step + hh -- the K fragment of k-step `step` and (at +8192) the V^T fragment of
// 16-key step `step`
__device__ __forceinline__ void frag_offsets(const int r, const int hh, unsigned (&koff)[4]) {
  const int swz = (r >> 1) & 7;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) koff[ks] = (unsigned)(r * 128 + (((2 * ks + hh) ^ swz) * 16));
}
// the eight K fragments [32-key block][k-step] / V^T fragments [16-key step][32-feature half] of the buffer at `buf`
__device__ __forceinline__ void read_k(bf16x8 (&fr)[8], const char* buf, const unsigned (&koff)[4]) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fr[kb * 4 + ks] = *reinterpret_cast<const bf16x8*>(buf + koff[ks] + kb * 4096);
}
__device__ __forceinline__ void read_v(bf16x8 (&fr)[8], const char* buf, const unsigned (&koff)[4]) {
#pragma unroll
  for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
    for (int db = 0; db < 2; ++db) fr[sidx * 2 + db] = *reinterpret_cast<const bf16x8*>(buf + koff[sidx] + 8192 + db * 4096);
}

// S^T = init + K Q^T: two 32-key blocks whose accumulator chains alternate, so that the MFMA dependency never sits between two issues
__device__ __forceinline__ void qk(f32x16 (&s)[2], const bf16x8 (&fr)[8], const bf16x8 (&qf)[4], const f32x16& init) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[kb * 4 + ks], qf[ks], ks == 0 ? init : s[kb], 0, 0, 0);
}
// The reference k-step: S^T -= m_ref by the matrix core.  A operand: a K column of ones = element k == 0 of the step (held by the hh == 0 lanes); B operand:
// -m_ref (bf16-representable) in the same element of query column r.
__device__ __forceinline__ bf16x8 ref_step_ones(const int hh) { return __builtin_bit_cast(bf16x8, u32x4{hh == 0 ? 0x3F80u : 0u, 0u, 0u, 0u}); }
__device__ __forceinline__ unsigned ref_step_word(const float m_ref, const int hh) { return hh == 0 ? (pack2(-m_ref, 0.f) & 0xffffu) : 0u; }
__device__ __forceinline__ void ref_step(f32x16 (&s)[2], const bf16x8 kone, const u32x4 qm) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kone, __builtin_bit_cast(bf16x8, qm), s[kb], 0, 0, 0);
}

// column maximum of the 32-row kernels, one chain (the 64-row kernel keeps its pairwise form: the same value, other instructions)
__device__ __forceinline__ float col_max(const f32x16 (&s)[2]) {
  float mx_ = s[0][0];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int e = 0; e < 16; ++e) mx_ = fmaxf(mx_, s[kb][e]);
  return max_across_halves(mx_);
}
__device__ __forceinline__ void scale_o(f32x16 (&oacc)[2], const float alpha) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[i][e] *= alpha;
}
// The lazy reference moves, on exact scores s (= s*c - m_ref) whose column maximum is mx_: on the first tile, or where the column ran more than 8 above it, the
// new reference is m_ref + mx_ rounded to bf16 (the k-step form needs it representable; the splat form keeps the same values).  The scores take the difference,
// l and O (not on the first tile) the factor exp2(-difference): exact, softmax is invariant to the reference.  install(m_ref) puts it where the kernel's next
// S^T picks it up.
template <class Install>
__device__ __forceinline__ void move_reference(f32x16 (&s)[2], const float mx_, const bool first, float& m_ref, float& l_run, f32x16 (&oacc)[2], Install install) {
  float delta = 0.f;
  if (first || mx_ > 8.0f) {
    const float nr = bf16lo_to_f32(pack2(m_ref + mx_, 0.f));
    delta = nr - m_ref;
    m_ref = nr;
  }
  install(m_ref);
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int e = 0; e < 16; ++e) s[kb][e] -= delta;
  if (!first) {
    const float alpha = __builtin_amdgcn_exp2f(-delta);
    l_run *= alpha;
    scale_o(oacc, alpha);
  }
}

// The 32-row kernels' softmax pieces (the 64-row kernel sums its exponentials in another order: other roundings).
// p = exp2(s) in place; returns this half-wave's sum
__device__ __forceinline__ float exp_sum(f32x16 (&s)[2]) {
  float ps = 0.f;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float pe = __builtin_amdgcn_exp2f(s[kb][e]);
      s[kb][e] = pe;
      ps += pe;
    }
  return ps;
}
// the online softmax of the non-prescaled forms: running maximum m_run of s * c, p = exp2(s * c - m_run) in place, l and O rescaled
__device__ __forceinline__ void softmax_running_max(f32x16 (&s)[2], const float c, float& m_run, float& l_run, f32x16 (&oacc)[2]) {
  const float m_new = fmaxf(m_run, col_max(s) * c);
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
  m_run = m_new;
  float psum = 0.f;
  // (packed v_pk_fma_f32 / v_pk_add_f32 forms of this loop measured 0-3 % SLOWER in same-run A/B: scalar kept)
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float pe = __builtin_amdgcn_exp2f(s[kb][e] * c - m_new);
      s[kb][e] = pe;
      psum += pe;
    }
  l_run = l_run * alpha + psum;
  if (!__all(alpha == 1.0f)) scale_o(oacc, alpha);
}
// O^T += V^T P^T: the P fragments straight from the S^T accumulators (two-operand v_cvt_pk_bf16_f32)
__device__ __forceinline__ void pv(f32x16 (&oacc)[2], const f32x16 (&s)[2], const bf16x8 (&fr)[8]) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      u32x4 pw;
#pragma unroll
      for (int e = 0; e < 4; ++e) pw[e] = pack2(s[kb][8 * s2 + 2 * e], s[kb][8 * s2 + 2 * e + 1]);
      const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
      const int sidx = 2 * kb + s2;  // 16-key step inside the tile
#pragma unroll
      for (int db = 0; db < 2; ++db) oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[sidx * 2 + db], pf, oacc[db], 0, 0, 0);
    }
  }
}
// normalise and store O[qi][d] of (b, head) in 8-byte pieces: lane (r, hh) holds d = 32 db + 8 g + 4 hh + {0..3} of query qi
__device__ __forceinline__ void store_o(const AttnArgs& p, const int b, const int head, const int qi, const int hh, const float l_run, const f32x16 (&oacc)[2]) {
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_tot;
  if (qi < p.Lq) {
    bf16_t* op = p.o + ((long)b * p.Lq + qi) * p.ldo + head * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * hh;
        u32x2 o = {pack2(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv),
                   pack2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv)};
        *reinterpret_cast<u32x2*>(op + d) = o;
      }
  }
}

// K / V^T tiles staged by LDS-DMA (global_load_lds_dwordx4) into a ring of three buffers: 512 16-byte chunks per tile per operand, 2 per thread.  Chunk
// c = i * 256 + tid lands at byte 16 c of the image (an LDS-DMA writes base + 16 * lane); it is row c >> 3, slot c & 7, and holds logical chunk
// slot ^ ((row >> 1) & 7) of that row: the swizzle is applied on the SOURCE address.  Addresses are a wave-uniform base that moves with the tile (scalar
// registers; a chunk boundary of the patch-parallel layout jumps it) plus a per-lane 32-bit offset fixed for the whole kernel: no vector work per tile (the
// per-tile 64-bit address arithmetic cost the 64-row kernel 6 % of its launch).  Tiles are issued in key order.
// TAIL: a ragged last tile (rem = Lk % 64 keys) is fetched whole through a second set of offsets: its K rows >= Lk and its all-padding V^T chunks are redirected
// to addresses inside the operands (row Lk - 1; chunk 0 of the V^T row), and masked after they leave LDS.
struct AttnRingTail { unsigned toffk[2], toffv[2]; };
struct AttnRingNoTail {};
template <bool TAIL>
struct AttnRing : std::conditional_t<TAIL, AttnRingTail, AttnRingNoTail> {
  const AttnArgs& p;
  char* smem;
  unsigned wave_img;                           // this wave's 1 KB of an image (wave-uniform)
  const char* kbase; const char* vbase;
  unsigned voffk[2], voffv[2];
  const char* knext; const char* vnext;        // the next tile to issue
  int chunk_left, chunk_id;

  __device__ __forceinline__ AttnRing(const AttnArgs& p_, const int b, const int head, const int tid, const int wave, char* smem_, const int rem = 0) : p(p_), smem(smem_) {
    kbase = (const char*)(p.k + (long)b * p.k_bstride + head * 64);
    vbase = (const char*)(p.vt + (long)b * p.vt_bstride + ((long)head * 64) * p.ldvt);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = i * 256 + tid;
      const int row = c >> 3, ch = (c & 7) ^ ((row >> 1) & 7);
      voffk[i] = (unsigned)(row * p.ldk * 2 + ch * 16);
      voffv[i] = (unsigned)(row * p.ldvt * 2 + ch * 16);
      if constexpr (TAIL) {
        this->toffk[i] = (unsigned)((row < rem ? row : rem - 1) * p.ldk * 2 + ch * 16);
        this->toffv[i] = (unsigned)(row * p.ldvt * 2 + ((ch >> 1) * 16 < rem ? ch * 16 : 0));    // chunk ch = positions 8 ch ..: 16-key group ch >> 1
      }
    }
    knext = kbase;
    vnext = vbase;
    chunk_left = p.key_chunk > 0 ? p.key_chunk : 0x7fffffff;
    chunk_id = 0;
    wave_img = (unsigned)__builtin_amdgcn_readfirstlane(wave) * 1024u;
  }
  // the next tile into ring buffer `buf`; tail: it is the ragged last one
  __device__ __forceinline__ void issue(const int buf, const bool tail = false) {
    char* img = smem + buf * kBufBytes + wave_img;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      unsigned ok = voffk[i], ov = voffv[i];
      if constexpr (TAIL) { ok = tail ? this->toffk[i] : ok; ov = tail ? this->toffv[i] : ov; }
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(knext + ok),
                                       (__attribute__((address_space(3))) void*)(img + i * 4096), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vnext + ov),
                                       (__attribute__((address_space(3))) void*)(img + 8192 + i * 4096), 16, 0, 0);
    }
    knext += (long)KT * p.ldk * 2;
    vnext += KT * 2;
    chunk_left -= KT;
    if (chunk_left == 0) {                     // tiles never straddle a chunk (key_chunk % 64 == 0)
      ++chunk_id;
      chunk_left = p.key_chunk;
      knext = kbase + (long)chunk_id * p.k_cstride * 2;
      vnext = vbase + (long)chunk_id * p.vt_cstride * 2;
    }
  }
};

}  // namespace mx
