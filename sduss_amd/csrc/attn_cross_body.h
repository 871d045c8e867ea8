// The short-key cross-attention body (attention.hip holds the description and the kernel, attn_cross_kernel): ONE wave computes
// XK_QPW = 64 queries of one (batch, head) against Lk <= 96 keys held in registers.
#pragma once
#include "common.h"
#include "../../include/mxdenoise.h"
#include "attn_tile.h"

namespace mx {

constexpr int XK_MAXBLK = 3;                   // 32-key blocks (Lk <= 96)
constexpr int XK_QPW = 64;                     // queries per wave (two 32-query blocks)

// ---- the pieces: one fragment of the head's K / V^T (global -> register, masked), one block's arithmetic (the queries of a 32-query block: load_q,
//      attn_tile.h).  The kernel's wave keeps the 24 fragments in registers (attn_cross_wave). ----
constexpr int XK_KFRAGS = XK_MAXBLK * 4;       // K fragments of a head: [32-key block][16-feature step]
constexpr int XK_VFRAGS = 2 * XK_MAXBLK * 2;   // V^T fragments: [16-key step][32-feature half]

// K fragment (A operand of S^T): K[32 kb + r][16 ks + 8 hh ..]; rows >= Lk are zero
// LK > 0: the key count is that compile-time constant (the launcher dispatches LK = 77, the text encoders' sequence length, when every problem has it): block and
// step counts, the masks of the ragged last block and the exponentials of its all-padding elements are then resolved at compile time -- the runtime form spends
// ~150 selects and ~140 moves per 32-query block on them, against ~210 essential vector instructions.  LK = 0: runtime p.Lk.
template <int LK = 0>
__device__ __forceinline__ bf16x8 xk_kfrag(const AttnArgs& p, const int b, const int head, const int kb, const int ks, const int lane) {
  const int r = lane & 31, hh = lane >> 5;
  const int Lk = LK > 0 ? LK : p.Lk;
  const int nblk = (Lk + 31) >> 5;
  const int key = kb * 32 + r;
  const bf16_t* kp = p.k + ((long)b * Lk + (key < Lk ? key : 0)) * p.ldk + head * 64 + hh * 8;
  return (kb < nblk && key < Lk) ? *reinterpret_cast<const bf16x8*>(kp + ks * 16) : __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
}
// V^T fragment (A operand of O^T): vt[64 head + 32 db + r][16 st + 8 hh ..] (MX_VT_POS order); keys >= Lk zeroed, the pad of a V^T row may hold anything
template <int LK = 0>
__device__ __forceinline__ bf16x8 xk_vfrag(const AttnArgs& p, const int b, const int head, const int st, const int db, const int lane) {
  const int r = lane & 31, hh = lane >> 5;
  const int Lk = LK > 0 ? LK : p.Lk;
  const int nst = (Lk + 15) >> 4;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (st < nst) {
    v = *reinterpret_cast<const u32x4*>(p.vt + (long)b * p.vt_bstride + ((long)head * 64 + db * 32 + r) * p.ldvt + st * 16 + hh * 8);
    // element e of the word is position 16 st + 8 hh + e = key 16 st + 4 hh + (e & 3) + 8 (e >> 2)   (MX_VT_POS swaps bits 2 and 3)
    const int kbase = st * 16 + 4 * hh;
    if (kbase + 12 > Lk) {                     // some element may be past the end (only in the last step)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k0 = kbase + 2 * (e & 1) + 8 * (e >> 1);
        unsigned w = v[e];
        if (k0 >= Lk) w &= 0xffff0000u;
        if (k0 + 1 >= Lk) w &= 0x0000ffffu;
        v[e] = w;
      }
    }
  }
  return __builtin_bit_cast(bf16x8, v);
}
// One 32-query block: S^T = K Q^T, single-pass softmax, O^T = V^T P^T, O through the wave's 4-KB LDS patch as whole rows.  kf(kb, ks) / vf(st, db) hand out
// the fragments.
template <bool PRE, int LK = 0, class KF, class VF>
__device__ __forceinline__ void xk_block(const AttnArgs& p, const int b, const int head, const int q0, const bf16x8 (&qf)[4], KF&& kf, VF&& vf, char* const patch,
                                         const int lane) {
#pragma clang fp contract(off)      // no multiply-add pair below is meant to fuse: every instantiation (PRE, LK) rounds alike
  const int r = lane & 31;
  const int hh = lane >> 5;
  const int Lk = LK > 0 ? LK : p.Lk;
  const int nblk = (Lk + 31) >> 5;             // <= XK_MAXBLK (launcher)
  const int nst = (Lk + 15) >> 4;
  const float c = PRE ? 1.0f : p.scale_log2;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // ---- S^T = K Q^T ----
  f32x16 s[XK_MAXBLK];
#pragma unroll
  for (int kb = 0; kb < XK_MAXBLK; ++kb) {
    s[kb] = zero16;
    if (kb < nblk) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf(kb, ks), qf[ks], s[kb], 0, 0, 0);
    }
  }
  // ---- single-pass softmax over the lane's keys (block kb element e = key 32 kb + (e & 3) + 8 (e >> 2) + 4 hh) ----
  float mx_ = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < XK_MAXBLK; ++kb) {
    if (kb >= nblk) continue;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      if (LK > 0 && kb * 32 + (e & 3) + 8 * (e >> 2) >= LK) { s[kb][e] = -INFINITY; continue; }       // past the end for both half-waves: known at compile time
      float v = s[kb][e] * c;
      if ((kb + 1) * 32 > Lk && key >= Lk) v = -INFINITY;
      s[kb][e] = v;
      mx_ = fmaxf(mx_, v);
    }
  }
  mx_ = max_across_halves(mx_);
  float psum = 0.f;
#pragma unroll
  for (int kb = 0; kb < XK_MAXBLK; ++kb) {
    if (kb >= nblk) continue;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (LK > 0 && kb * 32 + (e & 3) + 8 * (e >> 2) >= LK) { s[kb][e] = 0.f; continue; }             // exp2(-inf) = 0 exactly: the same value, no instruction
      const float pe = __builtin_amdgcn_exp2f(s[kb][e] - mx_);
      s[kb][e] = pe;
      psum += pe;
    }
  }
  const float inv = 1.0f / (psum + __shfl_xor(psum, 32, 64));
  // ---- O^T = V^T P^T ----
  f32x16 oacc[2] = {zero16, zero16};
#pragma unroll
  for (int st = 0; st < 2 * XK_MAXBLK; ++st) {
    if (st >= nst) continue;
    const int kb = st >> 1, s2 = st & 1;
    u32x4 pw;
#pragma unroll
    for (int e = 0; e < 4; ++e) pw[e] = pack2(s[kb][8 * s2 + 2 * e], s[kb][8 * s2 + 2 * e + 1]);
    const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
#pragma unroll
    for (int db = 0; db < 2; ++db) oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf(st, db), pf, oacc[db], 0, 0, 0);
  }
  // ---- O[q][d]: lane (r, hh) holds d = 32 db + 8 g + 4 hh + {0..3} of query r.  Through the wave's LDS patch (rows = queries,
  //      128 B, 16-byte chunk ^= row & 7) so that the global stores are whole rows. ----
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const u32x2 o = {pack2(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv), pack2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv)};
      const int chunk = (4 * db + g) ^ (r & 7);
      *reinterpret_cast<u32x2*>(patch + r * 128 + chunk * 16 + hh * 8) = o;
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (lane >> 3) + 8 * i;
    const int ch = lane & 7;
    const u32x4 o = *reinterpret_cast<const u32x4*>(patch + row * 128 + ((ch ^ (row & 7)) * 16));
    const int qi = q0 + row;
    if (qi < p.Lq) *reinterpret_cast<u32x4*>(p.o + ((long)b * p.Lq + qi) * p.ldo + head * 64 + ch * 8) = o;
  }
}

// the kernel's wave: the head's fragments in registers, XK_QPW queries in 32-query blocks, the next block's queries fetched while one computes
// the wave's share: `nblocks` consecutive 32-query blocks from query q_wave0 (wave-uniform)
template <bool PRE, int LK = 0>
__device__ __forceinline__ void attn_cross_wave(const AttnArgs& p, const int b, const int head, const int q_wave0, const int nblocks, char* const patch, const int lane) {
  bf16x8 kf[XK_MAXBLK][4];
#pragma unroll
  for (int kb = 0; kb < XK_MAXBLK; ++kb)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) kf[kb][ks] = xk_kfrag<LK>(p, b, head, kb, ks, lane);
  bf16x8 vf[2 * XK_MAXBLK][2];
#pragma unroll
  for (int st = 0; st < 2 * XK_MAXBLK; ++st)
#pragma unroll
    for (int db = 0; db < 2; ++db) vf[st][db] = xk_vfrag<LK>(p, b, head, st, db, lane);
  bf16x8 qf[4], qn[4];
  load_q(p, b, head, q_wave0, lane, qf);
  for (int blk = 0; blk < nblocks; ++blk) {
    const int q0 = q_wave0 + blk * 32;
    if (q0 >= p.Lq) break;                     // wave-uniform
    if (blk + 1 < nblocks) load_q(p, b, head, q0 + 32, lane, qn);
    xk_block<PRE, LK>(p, b, head, q0, qf, [&](int kb, int ks) __attribute__((always_inline)) { return kf[kb][ks]; },
                         [&](int st, int db) __attribute__((always_inline)) { return vf[st][db]; }, patch, lane);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
  }
}

}  // namespace mx
