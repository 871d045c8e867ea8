// Flash-style fused attention forward for gfx950, head_dim 64, bf16 in / fp32 softmax / bf16 out.
//
//   O[b, i, h, :] = softmax_j(Q[b,i,h,:] . K[b,j,h,:] * scale) V[b,j,h,:]
//
// Serves the reference's xformers.ops.memory_efficient_attention(q, k, v) call sites
// (sduss/model_executor/modules/attention.py:86, 172, 195, 214) and the SD3 joint / dual attention
// (F.scaled_dot_product_attention, attention.py:324, 350, 394): no mask, no dropout, scale 1/sqrt(d).
//
// MI355X-first structure (cdna guide section 3 "An accumulator tile as the next MFMA's operand"):
//   * one wave = 32 query rows, 4 waves / workgroup, KV tiles of 64 keys staged in LDS and shared;
//   * S^T = K Q^T with v_mfma_f32_32x32x16_bf16 (K rows are the A operand, Q rows the B operand), so a
//     lane owns ONE query column and 2x16 key rows: row max / sum are in-lane plus one cross-half shuffle;
//   * the S^T accumulator, converted to bf16, IS the B operand of O^T += V^T P^T -- no LDS round trip for P;
//     V arrives already transposed (V^T[d][key], written by the QKV GEMM epilogue) AND with bits 2/3 of the key index
//     swapped (MX_VT_POS), which is exactly the k order the accumulator layout dictates
//     (element j of lane half h is key 16s + 8(j>>2) + 4h + (j&3)): a V^T A fragment is one aligned ds_read_b128;
//   * both LDS images share one XOR swizzle (16-byte chunk ^= (row>>1)&7 on 128-byte rows), so K and V^T reads use
//     the same per-lane offsets and are bank-conflict free;
//   * the kernel is VALU-bound at head_dim 64 (32 exp2 + ~90 other vector ops against 16 MFMAs per wave and tile), so the
//     loop carries no avoidable vector work: every LDS address is a loop-invariant per-lane offset whose buffer bit is
//     toggled by one XOR per tile, key/V^T masking exists only in a separate tail-tile path, P is packed with the
//     two-operand v_cvt_pk_bf16_f32, and the first MFMA of each S^T block takes a zero accumulator literal.
//   * PRE variant (mx_attention_prescaled; what the step plans use): Q arrives already multiplied by scale*log2(e) (the
//     producing GEMM epilogue / RMSNorm does it in fp32 before its single rounding), and the softmax reference m is
//     subtracted BY THE MATRIX CORE: a fifth k-step multiplies a constant K column of ones with a Q column holding -m, so
//     S' = s*c - m leaves the MFMA and p = exp2(S') needs no per-element vector op.  m is a lazy reference, not the
//     running max: it is set from the first tile and raised only when a tile's maximum exceeds it by more than 8 (then
//     that tile, O and l are rescaled -- exact, softmax is invariant to the reference; p <= 256 and l >= 1 always hold).
//     Per 64-key tile and lane this removes 32 v_fma, the alpha exp2 and 16 v_pk_mul for two extra MFMAs on a matrix pipe
//     that was 41 % busy while the vector ALU was 72 % busy (rocprofv3 SQ_ACTIVE_INST_VALU).
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "../../include/mxdenoise.h"
#include "attn_tile.h"
#include "attn_cross_body.h"

namespace mx {


// Grouped launch (mx_attention_prescaled_grouped): up to MX_MAX_SEGS problems -- the resolutions of a mixed batch, each with its own
// sequence lengths, batch and operand bases -- in ONE launch.  A workgroup finds its problem from its index with two compares and runs the
// ordinary kernel body on it: `p` is a wave-uniform reference into the kernel-argument segment (scalar loads).  n == 1: an ordinary launch.
struct AttnGroup {
  AttnArgs g[MX_MAX_SEGS];
  int blk0[MX_MAX_SEGS + 1];           // first workgroup of every problem: a multiple of 8, so that (workgroup & 7) is the hardware XCD in EVERY
                                       // problem (advisor, round 3: after a problem with an odd workgroup count the later problems' XCD-aware map
                                       // was rotated and their K / V^T panels lost their L2)
  int nblk[MX_MAX_SEGS];               // workgroups of every problem; the padding workgroups behind them exit at once
  int n;
};

// workgroup -> (problem, query block, batch * H + head); ROWS = query rows per workgroup.  Consecutive workgroup ids are dealt round-robin to
// the 8 XCDs (one L2 each): with the plain order (query block fastest) the query blocks of one head land on all 8 XCDs and each L2 fetches that
// head's K / V^T (rocprofv3 FETCH_SIZE: 4.4x the algorithmic bytes at Lk = 4429).  When the number of (batch, head) pairs of a problem is a
// multiple of 8, XCD x instead owns the pairs == x (mod 8) and walks their query blocks consecutively (its workgroup count is then a multiple
// of 8 as well, so the next problem starts on XCD 0 again).
// ROWS == 0: the short-key kernel's deal -- (xq_wpb + 3) / 4 workgroups per (batch, head), see launch_attention_group
template <int ROWS>
__device__ __forceinline__ const AttnArgs& attn_locate(const AttnGroup& ga, int& qb, int& bh) {
  int lin = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int i = 1; i < MX_MAX_SEGS; ++i) if (i < ga.n && lin >= ga.blk0[i]) s = i;
  const AttnArgs& p = ga.g[s];
  lin -= ga.blk0[s];
  if (lin >= ga.nblk[s]) { qb = -1; bh = 0; return p; }      // padding up to the next problem's 8-aligned start
  const int gx = ROWS > 0 ? (p.Lq + ROWS - 1) / (ROWS > 0 ? ROWS : 1) : (p.xq_wpb + 3) >> 2;
  if (p.xcd_map) {
    const int local = lin >> 3;
    qb = local % gx;
    bh = ((local / gx) << 3) + (lin & 7);
  } else {
    qb = lin % gx;
    bh = lin / gx;
  }
  return p;
}

// EXTRA: the additive-bias and causal-mask forms of the text encoders, a separate instantiation (as run-time branches they cost the
// 60 cross-attention launches of a UNet step 3.4 us each: profiles r02_f vs r02_g)
template <bool PRE, bool EXTRA = false>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const AttnGroup ga) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kBufBytes];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31;   // query column owned by this lane (and fragment row)
  const int hh = lane >> 5;  // half-wave
  int qb, bh;
  const AttnArgs& p = attn_locate<128>(ga, qb, bh);      // (problem of a grouped launch, query block, batch * H + head)
  if (qb < 0) return;
  const int head = bh % p.H;
  const int b = bh / p.H;
  const int q0 = qb * 128 + wave * 32;

  bf16x8 qf[4];
  load_q(p, b, head, q0, lane, qf);

  // ---- staging: 512 16-byte chunks per tile per operand, 2 per thread (rows srow, srow+32; chunk sch) ----
  const int srow = tid >> 3;
  const int sch = tid & 7;
  const bf16_t* kbase = p.k + (long)b * p.k_bstride + head * 64 + sch * 8;
  const bf16_t* vbase = p.vt + (long)b * p.vt_bstride + ((long)head * 64) * p.ldvt + sch * 8;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  u32x4 rk[2], rv[2];
  // (row>>1)&7 is the same for rows srow and srow+32: one store offset, +4096 B for the second row
  unsigned st_off = (unsigned)(srow * 128 + ((sch ^ ((srow >> 1) & 7)) * 16));     // byte offset inside the K image of buffer 0

  auto load_tile = [&](int kt) {               // full tile: no predicates
    int key0 = kt * KT;
    const bf16_t* kb_ = kbase;
    const bf16_t* vb_ = vbase;
    if (p.key_chunk > 0) {                     // tiles never straddle a chunk (key_chunk % 64 == 0)
      const int ch = key0 / p.key_chunk;
      key0 -= ch * p.key_chunk;
      kb_ += ch * p.k_cstride;
      vb_ += ch * p.vt_cstride;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rk[i] = *reinterpret_cast<const u32x4*>(kb_ + (long)(key0 + srow + 32 * i) * p.ldk);
      rv[i] = *reinterpret_cast<const u32x4*>(vb_ + (long)(srow + 32 * i) * p.ldvt + key0);
    }
  };
  auto load_tile_tail = [&](int kt) {          // last, partial tile: keys >= Lk are zero-filled (0 * garbage must not be NaN)
    const int key0 = kt * KT;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = key0 + srow + 32 * i;
      rk[i] = (key < p.Lk) ? *reinterpret_cast<const u32x4*>(kbase + (long)key * p.ldk) : zero4;
    }
    // chunk sch holds positions 8*sch .. +7 = keys ka .. ka+3 then ka+8 .. ka+11 (MX_VT_POS), ka = 16*(sch>>1) + 4*(sch&1)
    const int ka = key0 + 16 * (sch >> 1) + 4 * (sch & 1);
    const int nvalid = p.Lk - ka;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      u32x4 v = zero4;
      if (nvalid > 0) {
        v = *reinterpret_cast<const u32x4*>(vbase + (long)(srow + 32 * i) * p.ldvt + key0);
        if (nvalid < 12) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kk = 2 * (e & 1) + 8 * (e >> 1);   // key offset of the word's low half
            unsigned w = v[e];
            if (kk >= nvalid) w &= 0xffff0000u;
            if (kk + 1 >= nvalid) w &= 0x0000ffffu;
            v[e] = w;
          }
        }
      }
      rv[i] = v;
    }
  };
  auto store_tile = [&](unsigned off) {        // off = st_off with the destination buffer's bit set
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u32x4*>(smem + off + i * 4096) = rk[i];
      *reinterpret_cast<u32x4*>(smem + off + 8192 + i * 4096) = rv[i];
    }
  };

  unsigned koff[4];                            // for buffer 0; the buffer bit is XOR-toggled per tile
  frag_offsets(r, hh, koff);

  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 oacc[2] = {zero16, zero16};
  float m_run = -INFINITY;  // !PRE: running max of s*scale_log2 for query column r (identical in both halves)
  float l_run = 0.f;        // this half-wave's partial row sum
  // PRE: the scores leave their MFMA chain as s - m_ref through the reference k-step
  const bf16x8 kone = ref_step_ones(hh);
  u32x4 qm = {0u, 0u, 0u, 0u};
  float m_ref = 0.f;

  const int ntiles = (p.Lk + KT - 1) / KT;
  const bool ragged = (p.Lk % KT) != 0;

  if (ntiles == 1 && ragged) load_tile_tail(0); else load_tile(0);
  store_tile(st_off);
  __syncthreads();

  for (int kt = 0; kt < ntiles; ++kt) {
    const bool has_next = kt + 1 < ntiles;
    if (has_next) {
      if (ragged && kt + 2 == ntiles) load_tile_tail(kt + 1); else load_tile(kt + 1);
    }

    // All eight K fragments are requested before the first MFMA, so that no LDS latency sits between the issues.
    bf16x8 fr[8];
    read_k(fr, smem, koff);
    __builtin_amdgcn_sched_barrier(0);
    f32x16 s[2];
    qk(s, fr, qf, zero16);
    if constexpr (PRE) ref_step(s, kone, qm);
    read_v(fr, smem, koff);                    // V^T fragments (same registers): in flight while the softmax runs on the vector ALU
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (EXTRA) if (p.bias != nullptr) {   // additive bias, four consecutive keys per load; BEFORE the masks (the pad of a bias row may hold anything) (key = 32 kb + 8 g + 4 hh + {0..3})
      int qi = q0 + r;
      if (qi > p.Lq - 1) qi = p.Lq - 1;
      const float* brow = p.bias + ((long)head * p.Lq + qi) * p.ldb + kt * KT + 4 * hh;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(brow + kb * 32 + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) s[kb][4 * g + e] += b4[e];
        }
    }
    if (ragged && !has_next) {          // mask keys beyond Lk (tail tile only)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = kt * KT + kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
          if (key >= p.Lk) s[kb][e] = -INFINITY;
        }
    }
    if constexpr (EXTRA) if (p.causal) {            // keys after the query never count (every tile: short sequences only)
      const int qi = q0 + r;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = kt * KT + kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
          if (key > qi) s[kb][e] = -INFINITY;
        }
    }
    // ---- online softmax (log2 domain) ----
    if constexpr (PRE) {
      // s already holds s*c - m_ref.  The row maximum first: the reference moves only on the first tile or when a row ran more than 8 above it.
      const float mx_ = col_max(s);
      const bool first = kt == 0;
      if (first || __any(mx_ > 8.0f))
        move_reference(s, mx_, first, m_ref, l_run, oacc, [&](float m) __attribute__((always_inline)) { qm[0] = ref_step_word(m, hh); });
      l_run += exp_sum(s);
    } else {
      softmax_running_max(s, p.scale_log2, m_run, l_run, oacc);
    }
    pv(oacc, s, fr);
    // the next tile lives in the other buffer: toggle the buffer bit of every offset
    st_off ^= kBufBytes;
    if (has_next) store_tile(st_off);
#pragma unroll
    for (int i = 0; i < 4; ++i) koff[i] ^= kBufBytes;
    __syncthreads();
  }

  store_o(p, b, head, q0 + r, hh, l_run, oacc);
}


// ----------------------------------------------------------------------------------------------------------------------
// The same kernel with K / V^T tiles staged by LDS-DMA two tiles ahead (round 2), for key counts that are whole tiles (the launcher sends ragged
// ones to attn_fwd_kernel).  attn_fwd_kernel fetches tile kt + 1 into registers while it computes tile kt and writes it to LDS at the end of the
// iteration: one tile of compute (~1.2k cycles per wave) has to cover an L2 / Infinity-Cache round trip under load, and 16 VGPRs hold the staged
// tile.  Here the tile goes L2 -> LDS directly (AttnRing, attn_tile.h), issued right after the barrier of tile kt for tile kt + 2; one counted
// s_waitcnt vmcnt(4) + one raw s_barrier per tile.
// ----------------------------------------------------------------------------------------------------------------------
template <bool PRE>
__global__ __launch_bounds__(256, 2) void attn_fwd_dma_kernel(const AttnGroup ga) {
  __shared__ __attribute__((aligned(16))) char smem[3 * kBufBytes];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31;   // query column owned by this lane (and fragment row)
  const int hh = lane >> 5;  // half-wave
  int qb, bh;
  const AttnArgs& p = attn_locate<128>(ga, qb, bh);      // (problem of a grouped launch, query block, batch * H + head)
  if (qb < 0) return;
  const int head = bh % p.H;
  const int b = bh / p.H;
  const int q0 = qb * 128 + wave * 32;

  bf16x8 qf[4];
  load_q(p, b, head, q0, lane, qf);
  AttnRing<false> ring(p, b, head, tid, wave, smem);
  unsigned koff[4];
  frag_offsets(r, hh, koff);

  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 oacc[2] = {zero16, zero16};
  float m_run = -INFINITY;  // !PRE: running max of s*scale_log2 for query column r (identical in both halves)
  float l_run = 0.f;        // this half-wave's partial row sum
  // PRE: the scores leave their MFMA chain as s - m_ref: the chain STARTS from the accumulator negm = (-m_ref, ... 16 times) of the lane's query column
  // (round 5; the guide's "row constants as the initial accumulator").  It was a fifth k-step (a K column of ones times -m_ref): two MFMAs per tile on the
  // scores' dependency chain; the splat costs 16 registers and is rewritten only when the reference moves.
  f32x16 negm = zero16;
  float m_ref = 0.f;
  auto move = [&](f32x16 (&s)[2], bool first) __attribute__((always_inline)) {       // on exact scores in s
    move_reference(s, col_max(s), first, m_ref, l_run, oacc, [&](float m) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 16; ++e) negm[e] = -m;
    });
  };

  const int ntiles = (p.Lk + KT - 1) / KT;

  ring.issue(0);
  if (ntiles > 1) ring.issue(1);
  int buf = 0;                                 // ring buffer of the tile being computed
  unsigned bofs = 0;                           // its byte offset

  for (int kt = 0; kt < ntiles; ++kt) {
    // tile kt has landed (this thread's part; the next tile's four DMAs may stay in flight) ...
    if (kt + 1 < ntiles) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();              // ... for every thread, and every wave has left the buffer of tile kt - 1
    asm volatile("" ::: "memory");
    if (kt + 2 < ntiles) ring.issue(buf == 0 ? 2 : buf - 1);   // (kt + 2) % 3

    // All eight K fragments are requested before the first MFMA, so that no LDS latency sits between the issues.
    bf16x8 fr[8];
    read_k(fr, smem + bofs, koff);
    __builtin_amdgcn_sched_barrier(0);
    f32x16 s[2];
    qk(s, fr, qf, PRE ? negm : zero16);
    read_v(fr, smem + bofs, koff);             // V^T fragments (same registers): in flight while the softmax runs on the vector ALU
    __builtin_amdgcn_sched_barrier(0);
    // ---- online softmax (log2 domain) ----
    if constexpr (PRE) {
      // s already holds s*c - m_ref, m_ref a lazy reference: set from tile 0, raised only when a row runs more than 8 above it.  After
      // tile 0 the exponentials run SPECULATIVELY and the sums are watched (as in attn_fwd64_kernel): a score > 8 above the reference
      // makes its p, hence the lane's sum, exceed 256; then (rarely) the tile is redone exactly.  The row maximum leaves the hot path.
      float psum;
      if (kt == 0) {
        move(s, true);
        psum = exp_sum(s);
      } else {
        psum = exp_sum(s);
        if (__any(psum > 256.0f)) {            // redo: scores again from the K fragments (the V^T fragments took their registers)
          read_k(fr, smem + bofs, koff);
          qk(s, fr, qf, negm);
          move(s, false);
          psum = exp_sum(s);
#pragma unroll
          for (int sidx = 0; sidx < 4; ++sidx)     // (read_v written out: as a call this cold re-read costs the kernel a register, 153 -> 154)
#pragma unroll
            for (int db = 0; db < 2; ++db) fr[sidx * 2 + db] = *reinterpret_cast<const bf16x8*>(smem + bofs + koff[sidx] + 8192 + db * 4096);
        }
      }
      l_run += psum;
    } else {
      softmax_running_max(s, p.scale_log2, m_run, l_run, oacc);
    }
    pv(oacc, s, fr);
    buf = buf == 2 ? 0 : buf + 1;
    bofs = (unsigned)buf * kBufBytes;
  }

  store_o(p, b, head, q0 + r, hh, l_run, oacc);
}


// ----------------------------------------------------------------------------------------------------------------------
// 64 query rows per wave (round 2).  Ablation builds of attn_fwd_dma_kernel (MX_AEXP: tools/exp/README.md, profiles/r02_d_attention_ablation.txt) priced
// its parts at Lk = 4096: the four LDS-DMA pieces a wave issues per tile cost 19 % of the launch (an LDS-DMA instruction holds
// the wave's issue for 60-185 cycles, MI355X_MICROARCH.md), exp2 12 %, the S^T MFMAs 9 %, the barrier 4 %; a lone workgroup per CU
// runs at 57 % of three, i.e. one wave's tile is a serial chain (fragment reads -> S^T -> softmax -> O^T) that other waves must cover.
// Here a wave owns TWO 32-query blocks: the K / V^T fragments it reads from LDS and the DMA pieces it issues serve twice the MFMAs,
// and the two blocks are independent, so block 1's S^T MFMAs sit beside block 0's softmax and block 0's O^T MFMAs beside block 1's
// softmax in ONE instruction stream (sched_group_barrier pins the interleave).  A workgroup = 4 waves = 256 query rows, two
// workgroups per CU; O leaves through the (idle) K / V^T ring as whole 128-byte rows.
// ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attn_fwd64_kernel(const AttnGroup ga) {
  __shared__ __attribute__((aligned(16))) char smem[3 * kBufBytes];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31;   // query column owned by this lane (and fragment row)
  const int hh = lane >> 5;  // half-wave
  int qb, bh;
  const AttnArgs& p = attn_locate<256>(ga, qb, bh);      // (problem of a grouped launch, query block, batch * H + head)
  if (qb < 0) return;
  const int head = bh % p.H;
  const int b = bh / p.H;
  const int q0 = qb * 256 + wave * 64;

  bf16x8 qf[2][4];                             // the two 32-query blocks
  load_q(p, b, head, q0, lane, qf[0]);
  load_q(p, b, head, q0 + 32, lane, qf[1]);
  const int rem = p.Lk % KT;                   // keys of a ragged last tile
  AttnRing<true> ring(p, b, head, tid, wave, smem, rem);
  unsigned koff[4];
  frag_offsets(r, hh, koff);

  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 oacc[2][2] = {{zero16, zero16}, {zero16, zero16}};
  float l_run[2] = {0.f, 0.f};                 // this half-wave's partial row sums
  // the scores leave their MFMA chains as s - m_ref.  Block 0: the chain starts from negm0 = (-m_ref x 16) of the lane's query column (see attn_fwd_dma_kernel).
  // Block 1: the reference k-step (A operand = a K column of ones, B operand = -m_ref of query column r, bf16-representable): a splat for both blocks does not
  // fit the 256 registers of two waves per SIMD (measured with 11 spills: 332 -> 381 us at Lk 4096).
  f32x16 negm0 = zero16;
  const bf16x8 kone = ref_step_ones(hh);
  u32x4 qm1 = {0u, 0u, 0u, 0u};
  float m_ref[2] = {0.f, 0.f};
  auto set_ref = [&](int blk) __attribute__((always_inline)) {
    if (blk == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) negm0[e] = -m_ref[0];
    } else {
      qm1[0] = ref_step_word(m_ref[1], hh);
    }
  };

  const int ntiles = (p.Lk + KT - 1) / KT;     // >= 3 (launcher)

  auto col_max = [&](const f32x16 (&s)[2]) __attribute__((always_inline)) {      // (pairwise, not attn_tile.h's chain: the same value; HISTORY.md)
    float mx_ = fmaxf(s[0][0], s[1][0]);
#pragma unroll
    for (int e = 1; e < 16; ++e) mx_ = fmaxf(mx_, fmaxf(s[0][e], s[1][e]));
    return max_across_halves(mx_);
  };
  auto mask_scores = [&](f32x16 (&s)[2]) __attribute__((always_inline)) {        // ragged last tile: keys >= Lk never count
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh >= rem) s[kb][e] = -INFINITY;
  };
  auto mask_v = [&](bf16x8 (&fr)[8]) __attribute__((always_inline)) {            // ... and their V^T entries (any bit pattern) are zero
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        u32x4 w = __builtin_bit_cast(u32x4, fr[sidx * 2 + db]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {          // word j = elements 2j, 2j + 1 = keys k0, k0 + 1
          const int k0 = 16 * sidx + 4 * hh + ((2 * j) & 3) + 8 * (j >> 1);
          if (k0 >= rem) w[j] &= 0xffff0000u;
          if (k0 + 1 >= rem) w[j] &= 0x0000ffffu;
        }
        fr[sidx * 2 + db] = __builtin_bit_cast(bf16x8, w);
      }
  };
  auto scores = [&](f32x16 (&s)[2], const bf16x8 (&fr)[8], int blk) __attribute__((always_inline)) {   // s = (K Q^T) - m_ref
    qk(s, fr, qf[blk], blk == 0 ? negm0 : zero16);
    if (blk != 0) ref_step(s, kone, qm1);
  };
  // p = exp2(s) in place, packed to the four B fragments of O^T += V^T P^T; returns this half-wave's sum
  auto exp_pack = [&](f32x16 (&s)[2], u32x4 (&pw)[4]) __attribute__((always_inline)) {
    float ps = 0.f;                            // ONE chain: two would be SLP-packed into v_pk_add_f32, which costs more beside MFMAs
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float p0 = __builtin_amdgcn_exp2f(s[0][e]);
      const float p1 = __builtin_amdgcn_exp2f(s[1][e]);
      s[0][e] = p0; s[1][e] = p1;
      ps += p0; ps += p1;
    }
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
      for (int e = 0; e < 4; ++e) pw[sidx][e] = pack2(s[sidx >> 1][8 * (sidx & 1) + 2 * e], s[sidx >> 1][8 * (sidx & 1) + 2 * e + 1]);
    return ps;
  };
  // The softmax reference m_ref is lazy (attn_fwd_kernel): it only has to keep p = exp2(s - m_ref) in range.  The loop computes p
  // speculatively and looks at the sums: a score more than 8 above the reference makes its p, hence the lane's sum, exceed 256.
  // Then (rarely) this path redoes the block exactly: scores again from the K fragments, reference raised to the new maximum, p,
  // and O / l rescaled.  No false negatives; a false positive (32 scores averaging > 3 above the reference) costs time only.
  auto redo = [&](f32x16 (&s)[2], u32x4 (&pw)[4], const bf16x8 (&fr)[8], int blk, const bool tail) __attribute__((always_inline)) {
    scores(s, fr, blk);
    if (tail) mask_scores(s);
    move_reference(s, col_max(s), false, m_ref[blk], l_run[blk], oacc[blk], [&](float) __attribute__((always_inline)) { set_ref(blk); });
    return exp_pack(s, pw);
  };

  ring.issue(0);
  ring.issue(1);
  // ---- the reference starts at the maximum of tile 0 (a whole tile; its scores are computed again by the loop) ----
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  {
    bf16x8 fr[8];
    read_k(fr, smem, koff);
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      f32x16 s[2];
      scores(s, fr, blk);
      m_ref[blk] = bf16lo_to_f32(pack2(col_max(s), 0.f));
      set_ref(blk);
    }
  }
  int buf = 0;
  unsigned bofs = 0;

  // one tile: fragments of buffer `bofs`; TAIL = the ragged last tile
  auto tile = [&](const bool TAIL) __attribute__((always_inline)) {
    bf16x8 fr[8];
    f32x16 s0[2], s1[2];
    u32x4 pw0[4], pw1[4];
    read_k(fr, smem + bofs, koff);
    scores(s0, fr, 0);                           // S^T of block 0
    if (TAIL) mask_scores(s0);
    __builtin_amdgcn_sched_barrier(0);
    scores(s1, fr, 1);                           // S^T of block 1 beside the exponentials of block 0
    float ps = exp_pack(s0, pw0);
    __builtin_amdgcn_sched_barrier(0);
    if (TAIL) mask_scores(s1);
    if (__any(ps > 256.0f)) {
      ps = redo(s0, pw0, fr, 0, TAIL);
    }
    l_run[0] += ps;
    read_v(fr, smem + bofs, koff);                          // V^T fragments (the K fragments are dead: same registers)
    if (TAIL) mask_v(fr);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx)       // O^T of block 0 beside the exponentials of block 1
#pragma unroll
      for (int db = 0; db < 2; ++db)
        oacc[0][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[sidx * 2 + db], __builtin_bit_cast(bf16x8, pw0[sidx]), oacc[0][db], 0, 0, 0);
    ps = exp_pack(s1, pw1);
    __builtin_amdgcn_sched_barrier(0);
    if (__any(ps > 256.0f)) {
      read_k(fr, smem + bofs, koff);
      ps = redo(s1, pw1, fr, 1, TAIL);
      read_v(fr, smem + bofs, koff);
      if (TAIL) mask_v(fr);
    }
    l_run[1] += ps;
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx)       // O^T of block 1
#pragma unroll
      for (int db = 0; db < 2; ++db)
        oacc[1][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[sidx * 2 + db], __builtin_bit_cast(bf16x8, pw1[sidx]), oacc[1][db], 0, 0, 0);
  };

  const int nfull = rem ? ntiles - 1 : ntiles;  // whole tiles
  for (int kt = 0; kt < nfull; ++kt) {
    if (kt > 0) {
      if (kt + 1 < ntiles) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();            // tile kt has landed for every thread; every wave has left the buffer of tile kt - 1
      asm volatile("" ::: "memory");
    }
    if (kt + 2 < ntiles) ring.issue(buf == 0 ? 2 : buf - 1, rem && kt + 3 == ntiles);   // tile kt + 2 into buffer (kt + 2) % 3
    tile(false);
    buf = buf == 2 ? 0 : buf + 1;
    bofs = (unsigned)buf * kBufBytes;
  }
  if (rem) {                                   // the ragged last tile (never tile 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    tile(true);
  }

  // ---- normalise; O[q][d] through the wave's 8 KB of the ring (rows = queries, 128 B, 16-byte chunk ^= row & 7) so that the
  //      global stores are whole rows.  Lane (r, hh) holds d = 32 db + 8 g + 4 hh + {0..3} of query 32 blk + r. ----
  __syncthreads();                             // every wave has left the last tile
  char* patch = smem + wave * 8192;
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    const float inv = 1.0f / (l_run[blk] + __shfl_xor(l_run[blk], 32, 64));
    const int row = blk * 32 + r;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const u32x2 o = {pack2(oacc[blk][db][4 * g] * inv, oacc[blk][db][4 * g + 1] * inv),
                         pack2(oacc[blk][db][4 * g + 2] * inv, oacc[blk][db][4 * g + 3] * inv)};
        const int chunk = (4 * db + g) ^ (row & 7);
        *reinterpret_cast<u32x2*>(patch + row * 128 + chunk * 16 + hh * 8) = o;
      }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = (lane >> 3) + 8 * i;
    const int ch = lane & 7;
    const u32x4 o = *reinterpret_cast<const u32x4*>(patch + row * 128 + ((ch ^ (row & 7)) * 16));
    const int qi = q0 + row;
    if (qi < p.Lq) *reinterpret_cast<u32x4*>(p.o + ((long)b * p.Lq + qi) * p.ldo + head * 64 + ch * 8) = o;
  }
}


// ----------------------------------------------------------------------------------------------------------------------
// Cross-attention with a SHORT key sequence (Lk <= 96: the 77 text tokens of SDXL; PatchCrossAttention.forward,
// modules/attention.py:59-110).  Half of the attention launches of a UNet step (70 of 140) are this shape, and the general
// kernel above spends them on machinery they do not need: two 64-key LDS tiles (the second 13/64 valid), a barrier per
// tile, the online-softmax rescale, and 8-byte output stores.  Here
//   * every wave works alone (no LDS tiles, no barrier): the head's K rows and V^T rows live in REGISTERS as ready-made MFMA
//     fragments (<= 12 + 12 fragments, loaded once per wave from L2) and are reused for all of the wave's query blocks;
//   * keys are padded to the next multiple of 32 for S^T = K Q^T (3 blocks for 77 keys) and of 16 for O^T += V^T P^T (5 steps);
//   * single-pass softmax: all scores of a query are in the lane (<= 48 per half-wave), so one max, one exp2 pass, one sum;
//   * the output block is transposed through a wave-private 4-KB LDS patch, so O is written as full 128-byte rows (8 lanes x
//     16 B; the per-CU store rate of full lines is 2.7x that of 8-byte pieces: profiles/r02_a_*), and the next query block's
//     Q rows are fetched while the current one computes.
// The launch is bound by its HBM traffic (Q read + O write); K / V^T stay in L2.
// ----------------------------------------------------------------------------------------------------------------------
template <bool PRE, int LK = 0>
__global__ __launch_bounds__(256, 2) void attn_cross_kernel(const AttnGroup ga) {
  __shared__ __attribute__((aligned(16))) char smem[4 * 4096];       // one 32 x 64 bf16 patch per wave
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  int qb, bh;
  const AttnArgs& p = attn_locate<0>(ga, qb, bh);      // (problem of a grouped launch, workgroup of the pair, batch * H + head)
  if (qb < 0) return;
  // the pair's 32-query blocks are dealt to its xq_wpb waves, the first `rem` taking one more: every wave of the launch works on base or base + 1 blocks
  const int w = __builtin_amdgcn_readfirstlane(qb * 4 + wave);
  if (w >= p.xq_wpb) return;                   // (waves work alone: no barrier in this kernel)
  const int nb = (p.Lq + 31) >> 5;
  const int base = nb / p.xq_wpb, rem = nb - base * p.xq_wpb;
  const int first = w * base + (w < rem ? w : rem);
  attn_cross_wave<PRE, LK>(p, bh / p.H, bh % p.H, first * 32, base + (w < rem ? 1 : 0), smem + wave * 4096, lane);
}

}  // namespace mx

// validate one problem and fill its argument block
static int fill_attention_args(mx::AttnArgs& a, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, int64_t vt_batch_stride, void* o,
                               int ldo, int B, int H, int Lq, int Lk, float scale, bool pre, int key_chunk, int64_t k_bstride, int64_t k_cstride,
                               int64_t vt_cstride, bool causal, const float* bias, int ldb) {
  using namespace mx;
  MX_CHECK(q && k && vt && o, "attention: null operand");
  MX_CHECK(B > 0 && H > 0 && Lq > 0 && Lk > 0, "attention: empty problem");
  MX_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)o) & 15) == 0, "attention: operand pointers must be 16-byte aligned");
  MX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0, "attention: strides must be multiples of 8 elements");
  MX_CHECK(ldq >= H * 64 && ldk >= H * 64 && ldo >= H * 64, "attention: row stride smaller than H*64");
  if (key_chunk > 0) {
    MX_CHECK(key_chunk % 64 == 0 && Lk % key_chunk == 0, "attention: key_chunk must be a multiple of 64 and divide Lk");
    MX_CHECK(ldvt >= key_chunk && k_bstride % 8 == 0 && k_cstride % 8 == 0 && vt_cstride % 8 == 0, "attention: bad chunk strides");
  } else {
    MX_CHECK(ldvt >= MX_VT_LD(Lk), "attention: ldvt must cover MX_VT_LD(Lk) (keys are stored in MX_VT_POS order)");
  }
  MX_CHECK(vt_batch_stride % 8 == 0 && vt_batch_stride >= (int64_t)H * 64 * ldvt, "attention: bad vt_batch_stride");
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.vt = (const bf16_t*)vt; a.o = (bf16_t*)o;
  a.vt_bstride = (long)vt_batch_stride;
  a.ldq = ldq; a.ldk = ldk; a.ldvt = ldvt; a.ldo = ldo; a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk;
  a.scale_log2 = scale * 1.4426950408889634f;
  a.causal = causal ? 1 : 0;
  a.bias = bias; a.ldb = ldb;
  if (bias) MX_CHECK(pre && key_chunk == 0 && ldb % 4 == 0 && ldb >= (Lk + KT - 1) / KT * KT && ((uintptr_t)bias & 15) == 0,
                     "attention: bias form needs prescaled q, ldb a multiple of 4 covering whole 64-key tiles, 16-byte alignment");
  if (causal) MX_CHECK(Lq == Lk && key_chunk == 0 && Lk <= 4096, "attention: causal form is for Lq == Lk <= 4096, one key range");
  a.key_chunk = key_chunk; a.k_bstride = key_chunk > 0 ? (long)k_bstride : (long)Lk * ldk; a.k_cstride = (long)k_cstride; a.vt_cstride = (long)vt_cstride;
  a.xcd_map = ((B * H) % 8 == 0) ? 1 : 0;
  a.xq_wpb = 0;
  return 0;
}

// Every kernel instantiation the attention launcher can start: T(id, kernel, (template arguments)) / P(id, kernel).  attention_kernel_of
// returns an id, launch_attention_group starts it through one switch over this list, and mx_attention_kernel_name reports it by name.
#define MX_ATTN_FORMS(T, P)                                  \
  T(AK_CROSS_PRE77, attn_cross_kernel, (true, 77))           \
  T(AK_CROSS_PRE, attn_cross_kernel, (true))                 \
  T(AK_CROSS, attn_cross_kernel, (false))                    \
  P(AK_W64, attn_fwd64_kernel)                               \
  T(AK_DMA_PRE, attn_fwd_dma_kernel, (true))                 \
  T(AK_DMA, attn_fwd_dma_kernel, (false))                    \
  T(AK_GEN_PRE_EXTRA, attn_fwd_kernel, (true, true))         \
  T(AK_GEN_EXTRA, attn_fwd_kernel, (false, true))            \
  T(AK_GEN_PRE, attn_fwd_kernel, (true))                     \
  T(AK_GEN, attn_fwd_kernel, (false))
#define MX_ATTN_UNPAREN(...) __VA_ARGS__
#define MX_ATTN_TARGS(...) "<" #__VA_ARGS__ ">"
enum AttnKernelId {
#define MX_ATTN_ID_T(id, k, targs) id,
#define MX_ATTN_ID_P(id, k) id,
  MX_ATTN_FORMS(MX_ATTN_ID_T, MX_ATTN_ID_P)
#undef MX_ATTN_ID_T
#undef MX_ATTN_ID_P
  AK_COUNT
};
#define MX_ATTN_NAME_T(id, k, targs) #k MX_ATTN_TARGS targs,
#define MX_ATTN_NAME_P(id, k) #k,
static const char* const kAttnKernelNames[AK_COUNT] = {MX_ATTN_FORMS(MX_ATTN_NAME_T, MX_ATTN_NAME_P)};

// The instantiation a launch over ga.n problems (ga.g filled) runs.  The kernel is chosen for the launch as a whole -- by its longest query
// sequence -- and must be able to serve every problem; otherwise the general register-staged kernel takes them all.  -1: force_cross, and the
// short-key kernel cannot serve the problems.  max_lq / any_extra: what the pass over the problems found, for the launcher.
static int attention_kernel_of(const mx::AttnGroup& ga, bool pre, bool force_cross, int* max_lq = nullptr, bool* any_extra = nullptr) {
  using namespace mx;
  const int n = ga.n;
  int maxLq = 0;
  bool all_short = true, all_long_k = true, whole_tiles = true, plain = true, o8 = true, extra = false;
  bool all77 = true;                           // the text encoders' 77 keys: the short-key kernel has a compile-time form for them (attn_cross_body.h, LK), which beats the
                                               // general kernel at every query length (round 5: 15.7 vs 18.8 us at B8 H20 Lq 1024, profiles/r05_l_cross77_ab.txt)
  for (int i = 0; i < n; ++i) {
    const AttnArgs& a = ga.g[i];
    maxLq = std::max(maxLq, a.Lq);
    all_short = all_short && a.Lk <= 32 * XK_MAXBLK;
    all_long_k = all_long_k && a.Lk > 2 * KT;
    whole_tiles = whole_tiles && a.Lk % KT == 0 && a.Lk >= 3 * KT;
    plain = plain && a.key_chunk == 0 && !a.causal && !a.bias;
    o8 = o8 && a.ldo % 8 == 0;
    extra = extra || a.causal || a.bias;
    all77 = all77 && a.Lk == 77;
  }
  if (max_lq) *max_lq = maxLq;
  if (any_extra) *any_extra = extra;
  // (at Lq 1024 the general kernel is 7 % faster than the short-key one: both are latency-bound)
  if (force_cross && !(all_short && plain && o8)) return -1;
  if (all_short && (maxLq >= 2048 || force_cross || (all77 && pre)) && plain && o8)      // short key sequence: every wave keeps K / V^T in registers
    return pre && all77 ? AK_CROSS_PRE77 : pre ? AK_CROSS_PRE : AK_CROSS;
  if (extra) return pre ? AK_GEN_PRE_EXTRA : AK_GEN_EXTRA;                // the masked / biased forms live in the register-staged kernel
  if (pre && all_long_k && maxLq >= 2048 && o8) return AK_W64;            // 64 query rows per wave (a tie with the 32-row kernels at Lq 1024)
  if (whole_tiles) return pre ? AK_DMA_PRE : AK_DMA;                      // whole tiles: LDS-DMA staging two tiles ahead
  return pre ? AK_GEN_PRE : AK_GEN;
}

// One launch over ga.n problems (ga.g filled), on the instantiation attention_kernel_of chooses.
static int launch_attention_group(void* stream, mx::AttnGroup& ga, bool pre, bool force_cross = false) {
  using namespace mx;
  const int n = ga.n;
  double flops = 0, bytes = 0;
  for (int i = 0; i < n; ++i) {
    const AttnArgs& a = ga.g[i];
    flops += 4.0 * a.B * a.H * (double)a.Lq * a.Lk * 64.0;
    bytes += 2.0 * a.B * a.H * 64.0 * (2.0 * a.Lq + 2.0 * a.Lk);
  }
  int maxLq;
  bool extra;
  const int form = attention_kernel_of(ga, pre, force_cross, &maxLq, &extra);
  MX_CHECK(!extra || n == 1, "attention: the causal / bias forms are not grouped");
  MX_CHECK(form >= 0, "attention: the short-key kernel needs Lk <= 96, no mask / bias / key chunks and ldo % 8 == 0");
  const bool cross = form == AK_CROSS_PRE77 || form == AK_CROSS_PRE || form == AK_CROSS;
  const int rows = form == AK_W64 ? 256 : 128;
  if (cross) {
    // The short-key kernel is latency-bound: a wave pays ~3 us to fetch its head's 24 fragments and ~2.5 us per 32-query block, two workgroups per CU.  With a fixed
    // 64 queries per wave the step's shapes were 1.25 rounds (B8 H20 Lq1024: 640 workgroups on 512 slots) or 2.5 (Lq4096).  Deal the blocks instead: every wave of
    // a (batch, head) takes `per` or `per - 1` consecutive blocks, `per` chosen to minimise rounds x (3 + 2.5 per) -- one round whenever the pairs fit the chip.
    const long slots = 2L * cu_count();
    int best_per = 1; double best_t = 0;
    int max_nb = 1;
    for (int i = 0; i < n; ++i) max_nb = std::max(max_nb, cdiv(ga.g[i].Lq, 32));
    for (int per = 1; per <= max_nb; ++per) {
      long wgs = 0;
      for (int i = 0; i < n; ++i) wgs += (long)cdiv(cdiv(cdiv(ga.g[i].Lq, 32), per), 4) * ga.g[i].H * ga.g[i].B;
      const double t = (double)cdiv64(wgs, slots) * (3.0 + 2.5 * per);
      if (best_t == 0 || t < best_t - 1e-9) { best_t = t; best_per = per; }
      if (wgs <= slots) break;                 // one round: a larger share only lengthens it
    }
    for (int i = 0; i < n; ++i) ga.g[i].xq_wpb = cdiv(cdiv(ga.g[i].Lq, 32), best_per);
  }
  long blocks = 0;
  for (int i = 0; i < n; ++i) {
    blocks = (blocks + 7) & ~7L;
    ga.blk0[i] = (int)blocks;
    ga.nblk[i] = (cross ? cdiv(ga.g[i].xq_wpb, 4) : cdiv(ga.g[i].Lq, rows)) * ga.g[i].H * ga.g[i].B;
    blocks += ga.nblk[i];
  }
  for (int i = n; i < MX_MAX_SEGS; ++i) ga.nblk[i] = 0;
  for (int i = n; i <= MX_MAX_SEGS; ++i) ga.blk0[i] = (int)blocks;
  MX_CHECK(blocks < 2147483647L, "attention: too many workgroups");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  const AttnArgs& a0 = ga.g[0];
  prof_begin(st, cross ? PROF_ATTN_CROSS : PROF_ATTN, flops, bytes, n == 1 ? a0.B * a0.H : n, maxLq, a0.Lk);
  switch (form) {
#define MX_ATTN_T(id, k, targs) case id: hipLaunchKernelGGL((k<MX_ATTN_UNPAREN targs>), grid, block, 0, st, ga); break;
#define MX_ATTN_P(id, k) case id: hipLaunchKernelGGL(k, grid, block, 0, st, ga); break;
    MX_ATTN_FORMS(MX_ATTN_T, MX_ATTN_P)
#undef MX_ATTN_T
#undef MX_ATTN_P
  }
  prof_end(st);
  MX_LAUNCH_CHECK();
  return 0;
}

static int launch_attention(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                            int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk, float scale, bool pre,
                            int key_chunk = 0, int64_t k_bstride = 0, int64_t k_cstride = 0, int64_t vt_cstride = 0, bool causal = false,
                            const float* bias = nullptr, int ldb = 0) {
  mx::AttnGroup ga;
  ga.n = 1;
  if (fill_attention_args(ga.g[0], q, ldq, k, ldk, vt, ldvt, vt_batch_stride, o, ldo, B, H, Lq, Lk, scale, pre, key_chunk, k_bstride, k_cstride, vt_cstride,
                          causal, bias, ldb)) return 1;
  return launch_attention_group(stream, ga, pre);
}

/* Grouped form of mx_attention_prescaled: the problems of all resolutions of a mixed batch in ONE launch (the reference regroups the patches of
 * every latent per resolution and calls the attention once per resolution: modules/attention.py:152-203). */
extern "C" int mx_attention_prescaled_grouped(void* stream, const mx_attn_problem* probs, int n, int ldq, int ldk, int ldo, int H) {
  MX_CHECK(probs != nullptr && n >= 1 && n <= MX_MAX_SEGS, "attention: grouped launch needs 1..MX_MAX_SEGS problems");
  mx::AttnGroup ga;
  ga.n = n;
  for (int i = 0; i < n; ++i) {
    const mx_attn_problem& p = probs[i];
    if (fill_attention_args(ga.g[i], p.q, ldq, p.k, ldk, p.vt, p.ldvt, p.vt_batch_stride, p.o, ldo, p.B, H, p.Lq, p.Lk, 1.0f, true, 0, 0, 0, 0, false, nullptr, 0))
      return 1;
  }
  return launch_attention_group(stream, ga, true);
}

extern "C" int mx_attention(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                            int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk, float scale) {
  return launch_attention(stream, q, ldq, k, ldk, vt, ldvt, vt_batch_stride, o, ldo, B, H, Lq, Lk, scale, false);
}

extern "C" int mx_attention_prescaled(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                      int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk) {
  return launch_attention(stream, q, ldq, k, ldk, vt, ldvt, vt_batch_stride, o, ldo, B, H, Lq, Lk, 1.0f, true);
}

/* mx_attention_prescaled through the short-key kernel whatever Lq */
extern "C" int mx_attention_cross_prescaled(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                            int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk) {
  mx::AttnGroup ga;
  ga.n = 1;
  if (fill_attention_args(ga.g[0], q, ldq, k, ldk, vt, ldvt, vt_batch_stride, o, ldo, B, H, Lq, Lk, 1.0f, true, 0, 0, 0, 0, false, nullptr, 0)) return 1;
  return launch_attention_group(stream, ga, true, /*force_cross=*/true);
}

/* causal self-attention of a short sequence (the CLIP text encoders: 77 tokens), q prescaled as for mx_attention_prescaled */
extern "C" int mx_attention_prescaled_causal(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                             int64_t vt_batch_stride, void* o, int ldo, int B, int H, int L) {
  return launch_attention(stream, q, ldq, k, ldk, vt, ldvt, vt_batch_stride, o, ldo, B, H, L, L, 1.0f, true, 0, 0, 0, 0, true);
}

/* additive score bias (T5 relative position bias): softmax(q k^T + bias[h]) v with q AND bias already in the log2 domain (both multiplied by
 * log2(e) by their producers); bias fp32 [H][Lq][ldb], ldb >= Lk rounded up to 64 */
extern "C" int mx_attention_prescaled_bias(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                           int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk, const float* bias, int ldb) {
  MX_CHECK(bias != nullptr, "attention: null bias");
  return launch_attention(stream, q, ldq, k, ldk, vt, ldvt, vt_batch_stride, o, ldo, B, H, Lq, Lk, 1.0f, true, 0, 0, 0, 0, false, bias, ldb);
}

/* patch-parallel form (mx_unet_forward_pp): K rows and V^T columns of the `world` ranks arrive rank-major from the all-gather.
 * keys [c * key_chunk, (c + 1) * key_chunk) of batch b: K rows at k + c * k_chunk_stride + b * k_batch_stride (row stride ldk),
 * V^T at vt + c * vt_chunk_stride + b * vt_batch_stride + (h * 64 + d) * ldvt + MX_VT_POS(key - c * key_chunk). */
extern "C" int mx_attention_prescaled_chunked(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                              int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk, int key_chunk,
                                              int64_t k_batch_stride, int64_t k_chunk_stride, int64_t vt_chunk_stride) {
  return launch_attention(stream, q, ldq, k, ldk, vt, ldvt, vt_batch_stride, o, ldo, B, H, Lq, Lk, 1.0f, true, key_chunk,
                          k_batch_stride, k_chunk_stride, vt_chunk_stride);
}

/* name of the kernel instantiation one attention launch over a problem of this shape would run (host only): prescaled, causal, bias and key_chunk as the
 * entry points above take them; force_cross: mx_attention_cross_prescaled.  -1: no instantiation serves it */
extern "C" int mx_attention_kernel_name(int B, int H, int Lq, int Lk, int ldo, int prescaled, int causal, int bias, int key_chunk, int force_cross,
                                        char* buf, int cap) {
  if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return -1;
  mx::AttnGroup ga;
  ga.n = 1;
  mx::AttnArgs& a = ga.g[0];
  a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.ldo = ldo;
  a.causal = causal ? 1 : 0;
  a.bias = bias ? reinterpret_cast<const float*>(16) : nullptr;      // (shape query: the chooser only looks at whether there is one)
  a.key_chunk = key_chunk;
  const int form = attention_kernel_of(ga, prescaled != 0, force_cross != 0);
  if (form < 0) return -1;
  return mx::copy_name(kAttnKernelNames[form], buf, cap);
}
extern "C" int mx_attention_kernel_names(char* buf, int cap) { return mx::join_names(kAttnKernelNames, AK_COUNT, buf, cap); }
