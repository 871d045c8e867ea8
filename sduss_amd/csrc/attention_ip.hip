// Short-key cross-attention with a SECOND, separately normalised key set: the image prompt (IP-Adapter) of the SDXL UNet's attn2.
//
//   O[b, i, h, :] = softmax_j(q . k_text_j) v_text  +  ip_scale[b] * softmax_j(q . k_img_j) v_img          (q prescaled, log2 domain)
//
// The wave is the short-key kernel's wave (attention.hip, attn_cross_body.h): it works alone, keeps the head's text K / V^T as 24 MFMA
// fragments in registers and walks its share of 32-query blocks.  The launch is bound by the Q read and the O write; the image term rides in
// the same wave and the same launch, on the same Q fragments and into the same output accumulators:
//   * image operands: <= 16 keys per sample, stored padded to 16 rows -- ONE 32-row K block (4 fragments; rows >= n_img zero) and ONE 16-key
//     V^T step (2 fragments; keys >= n_img zeroed), loaded once per wave through xk_kfrag / xk_vfrag: 6 fragments = 24 registers;
//   * text phase: as xk_block up to the unnormalised accumulators and 1 / sum; the accumulators are then NORMALISED IN REGISTERS;
//   * image phase: S2^T = K_img Q^T (4 MFMAs) into the first score block's registers, its own maximum and its own sum over the lane's 8 keys
//     (elements 8..15 of the block are keys 16..31: never there); p * (ip_scale[b] / sum) in fp32, ONE rounding to bf16, then
//     O^T += V_img^T P^T (2 MFMAs) into the text phase's accumulators.  No second accumulator set, no second score array;
//   * ip_scale[b] is wave-uniform (a wave serves one (batch, head)).  Exactly 0: the wave loads no image operand and runs xk_block itself,
//     so such a row is bit-equal to mx_attention_cross_prescaled.
// Work split, launch bounds and the deal of 32-query blocks to waves (xq_wpb) are those of attn_cross_kernel.
#include <algorithm>

#include "common.h"
#include "../../include/mxdenoise.h"
#include "attn_tile.h"
#include "attn_cross_body.h"

namespace mx {

constexpr int XI_KEYS = 16;                    // image keys per sample as stored (n_img <= XI_KEYS valid)

struct AttnIpArgs {
  AttnArgs a;                                  // the text problem (xq_wpb: the waves of a (batch, head))
  const bf16_t* k_ip;                          // [B * XI_KEYS, ldk_ip], head h at columns [64 h, 64 h + 64)
  const bf16_t* vt_ip;                         // [B][H * 64][XI_KEYS] in MX_VT_POS order
  const float* ip_scale;                       // [B]
  long vt_ip_bstride;
  int ldk_ip, n_img;
};
struct AttnIpGroup {                           // the problems of a grouped launch: as AttnGroup (attention.hip)
  AttnIpArgs g[MX_MAX_SEGS];
  int blk0[MX_MAX_SEGS + 1];                   // first workgroup of every problem, a multiple of 8
  int nblk[MX_MAX_SEGS];
  int n;
};

// the image phase's operands as an AttnArgs of ONE sample, so that xk_kfrag / xk_vfrag (batch 0, runtime Lk = n_img) load and mask them
__device__ __forceinline__ AttnArgs ip_operands(const AttnIpArgs& p, const int b) {
  AttnArgs ip = p.a;
  ip.k = p.k_ip + (long)b * XI_KEYS * p.ldk_ip;
  ip.ldk = p.ldk_ip;
  ip.vt = p.vt_ip + (long)b * p.vt_ip_bstride;
  ip.ldvt = XI_KEYS;
  ip.vt_bstride = 0;
  ip.Lk = p.n_img;
  return ip;
}

// One 32-query block with the image term.  The text phase repeats xk_block (PRE) operation by operation.
// kfi(ks) / vfi(db) hand out the image fragments.
template <int LK, class KF, class VF, class KFI, class VFI>
__device__ __forceinline__ void xk_block_ip(const AttnArgs& p, const int b, const int head, const int q0, const bf16x8 (&qf)[4], KF&& kf, VF&& vf,
                                            KFI&& kfi, VFI&& vfi, const int n_img, const float ip_scale, char* const patch, const int lane) {
#pragma clang fp contract(off)
  const int r = lane & 31;
  const int hh = lane >> 5;
  const int Lk = LK > 0 ? LK : p.Lk;
  const int nblk = (Lk + 31) >> 5;
  const int nst = (Lk + 15) >> 4;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // ---- text: S^T = K Q^T ----
  f32x16 s[XK_MAXBLK];
#pragma unroll
  for (int kb = 0; kb < XK_MAXBLK; ++kb) {
    s[kb] = zero16;
    if (kb < nblk) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf(kb, ks), qf[ks], s[kb], 0, 0, 0);
    }
  }
  float mx_ = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < XK_MAXBLK; ++kb) {
    if (kb >= nblk) continue;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      if (LK > 0 && kb * 32 + (e & 3) + 8 * (e >> 2) >= LK) { s[kb][e] = -INFINITY; continue; }
      float v = s[kb][e];
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
      if (LK > 0 && kb * 32 + (e & 3) + 8 * (e >> 2) >= LK) { s[kb][e] = 0.f; continue; }
      const float pe = __builtin_amdgcn_exp2f(s[kb][e] - mx_);
      s[kb][e] = pe;
      psum += pe;
    }
  }
  const float inv = 1.0f / (psum + __shfl_xor(psum, 32, 64));
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
  // the text term, normalised where it sits: the same oacc * inv product xk_block packs
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[db][e] = oacc[db][e] * inv;
  // ---- image: S2^T = K_img Q^T into s[0]; element e < 8 is key (e & 3) + 8 (e >> 2) + 4 hh < 16, elements 8..15 are keys >= 16 ----
  s[0] = zero16;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) s[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfi(ks), qf[ks], s[0], 0, 0, 0);
  float mi = -INFINITY;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int key = (e & 3) + 8 * (e >> 2) + 4 * hh;
    const float v = key < n_img ? s[0][e] : -INFINITY;
    s[0][e] = v;
    mi = fmaxf(mi, v);
  }
  mi = max_across_halves(mi);                  // key 0 is always there (n_img >= 1): finite
  float isum = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float pe = __builtin_amdgcn_exp2f(s[0][e] - mi);
    s[0][e] = pe;
    isum += pe;
  }
  const float w = ip_scale / (isum + __shfl_xor(isum, 32, 64));
  u32x4 pw;
#pragma unroll
  for (int e = 0; e < 4; ++e) pw[e] = pack2(s[0][2 * e] * w, s[0][2 * e + 1] * w);
  const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
#pragma unroll
  for (int db = 0; db < 2; ++db) oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfi(db), pf, oacc[db], 0, 0, 0);
  // ---- O[q][d] through the wave's LDS patch, whole rows out (xk_block's layout) ----
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const u32x2 o = {pack2(oacc[db][4 * g], oacc[db][4 * g + 1]), pack2(oacc[db][4 * g + 2], oacc[db][4 * g + 3])};
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

// the wave: attn_cross_wave with the image fragments beside the text ones
// LK > 0: the 6 image fragments stay in registers.  LK = 0: the runtime form has no registers left for them (its masks and counts are live values), so the
// wave parks them in `park`, XI_PARK bytes of LDS of its own -- every lane reads back the 16-byte words it wrote itself: no barrier -- and an image-phase MFMA
// takes its operand from there.
constexpr int XI_PARK = 6 * 64 * 16;
template <int LK>
__device__ __forceinline__ void attn_cross_ip_wave(const AttnIpArgs& pi, const int b, const int head, const int q_wave0, const int nblocks, char* const patch,
                                                   char* const park, const int lane) {
  const AttnArgs& p = pi.a;
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
  const float ip_scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, pi.ip_scale[b])));
  const bool with_ip = ip_scale != 0.0f;       // wave-uniform
  bf16x8 kfi[4], vfi[2];
  bf16x8* const mine = reinterpret_cast<bf16x8*>(park) + lane;       // fragment f of this lane: mine[64 f]
  if (with_ip) {
    const AttnArgs ip = ip_operands(pi, b);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) kfi[ks] = xk_kfrag<0>(ip, 0, head, 0, ks, lane);
#pragma unroll
    for (int db = 0; db < 2; ++db) vfi[db] = xk_vfrag<0>(ip, 0, head, 0, db, lane);
    if (LK == 0) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) mine[64 * ks] = kfi[ks];
#pragma unroll
      for (int db = 0; db < 2; ++db) mine[64 * (4 + db)] = vfi[db];
    }
  }
  bf16x8 qf[4], qn[4];
  load_q(p, b, head, q_wave0, lane, qf);
  for (int blk = 0; blk < nblocks; ++blk) {
    const int q0 = q_wave0 + blk * 32;
    if (q0 >= p.Lq) break;                     // wave-uniform
    if (blk + 1 < nblocks) load_q(p, b, head, q0 + 32, lane, qn);
    auto kfn = [&](int kb, int ks) __attribute__((always_inline)) { return kf[kb][ks]; };
    auto vfn = [&](int st, int db) __attribute__((always_inline)) { return vf[st][db]; };
    if (with_ip) {
      if (LK == 0)
        xk_block_ip<LK>(p, b, head, q0, qf, kfn, vfn, [&](int ks) __attribute__((always_inline)) { return mine[64 * ks]; },
                        [&](int db) __attribute__((always_inline)) { return mine[64 * (4 + db)]; }, pi.n_img, ip_scale, patch, lane);
      else
        xk_block_ip<LK>(p, b, head, q0, qf, kfn, vfn, [&](int ks) __attribute__((always_inline)) { return kfi[ks]; },
                        [&](int db) __attribute__((always_inline)) { return vfi[db]; }, pi.n_img, ip_scale, patch, lane);
    }
    else xk_block<true, LK>(p, b, head, q0, qf, kfn, vfn, patch, lane);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
  }
}

// workgroup -> (problem, workgroup of the (batch, head) pair, batch * H + head): the short-key kernel's map (attention.hip, attn_locate<0>)
__device__ __forceinline__ const AttnIpArgs& attn_ip_locate(const AttnIpGroup& ga, int& qb, int& bh) {
  int lin = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int i = 1; i < MX_MAX_SEGS; ++i) if (i < ga.n && lin >= ga.blk0[i]) s = i;
  const AttnIpArgs& p = ga.g[s];
  lin -= ga.blk0[s];
  if (lin >= ga.nblk[s]) { qb = -1; bh = 0; return p; }
  const int gx = (p.a.xq_wpb + 3) >> 2;
  if (p.a.xcd_map) {
    const int local = lin >> 3;
    qb = local % gx;
    bh = ((local / gx) << 3) + (lin & 7);
  } else {
    qb = lin % gx;
    bh = lin / gx;
  }
  return p;
}

template <int LK = 0>
__global__ __launch_bounds__(256, 2) void attn_cross_ip_kernel(const AttnIpGroup ga) {
  __shared__ __attribute__((aligned(16))) char smem[4 * 4096 + (LK == 0 ? 4 * XI_PARK : 0)];       // one 32 x 64 bf16 patch per wave; LK = 0: the parked image fragments
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  int qb, bh;
  const AttnIpArgs& pi = attn_ip_locate(ga, qb, bh);
  if (qb < 0) return;
  const AttnArgs& p = pi.a;
  const int w = __builtin_amdgcn_readfirstlane(qb * 4 + wave);
  if (w >= p.xq_wpb) return;                   // (waves work alone: no barrier in this kernel)
  const int nb = (p.Lq + 31) >> 5;
  const int base = nb / p.xq_wpb, rem = nb - base * p.xq_wpb;
  const int first = w * base + (w < rem ? w : rem);
  attn_cross_ip_wave<LK>(pi, bh / p.H, bh % p.H, first * 32, base + (w < rem ? 1 : 0), smem + wave * 4096,
                         LK == 0 ? smem + 4 * 4096 + wave * XI_PARK : nullptr, lane);
}

}  // namespace mx

// validate one problem and fill its argument block
static int fill_ip_args(mx::AttnIpArgs& g, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, int64_t vt_batch_stride, const void* k_ip,
                        int ldk_ip, const void* vt_ip, int64_t vt_ip_batch_stride, int n_img, const float* ip_scale, void* o, int ldo, int B, int H, int Lq,
                        int Lk) {
  using namespace mx;
  MX_CHECK(q && k && vt && o && k_ip && vt_ip && ip_scale, "attention_ip: null operand");
  MX_CHECK(B > 0 && H > 0 && Lq > 0 && Lk > 0, "attention_ip: empty problem");
  MX_CHECK(Lk <= 32 * XK_MAXBLK, "attention_ip: the short-key kernel needs Lk <= 96");
  MX_CHECK(n_img >= 1 && n_img <= XI_KEYS, "attention_ip: n_img must be in 1..16");
  MX_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)o | (uintptr_t)k_ip | (uintptr_t)vt_ip) & 15) == 0 && ((uintptr_t)ip_scale & 3) == 0,
           "attention_ip: operand pointers must be 16-byte aligned (ip_scale: 4)");
  MX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldk_ip % 8 == 0 && ldo % 8 == 0, "attention_ip: strides must be multiples of 8 elements");
  MX_CHECK(ldq >= H * 64 && ldk >= H * 64 && ldk_ip >= H * 64 && ldo >= H * 64, "attention_ip: row stride smaller than H*64");
  MX_CHECK(ldvt >= MX_VT_LD(Lk), "attention_ip: ldvt must cover MX_VT_LD(Lk)");
  MX_CHECK(vt_batch_stride % 8 == 0 && vt_batch_stride >= (int64_t)H * 64 * ldvt, "attention_ip: bad vt_batch_stride");
  MX_CHECK(vt_ip_batch_stride % 8 == 0 && vt_ip_batch_stride >= (int64_t)H * 64 * XI_KEYS, "attention_ip: bad vt_ip_batch_stride");
  AttnArgs& a = g.a;
  a = AttnArgs{};
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.vt = (const bf16_t*)vt; a.o = (bf16_t*)o;
  a.vt_bstride = (long)vt_batch_stride;
  a.ldq = ldq; a.ldk = ldk; a.ldvt = ldvt; a.ldo = ldo; a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk;
  a.scale_log2 = 1.4426950408889634f;          // (prescaled q: unused)
  a.k_bstride = (long)Lk * ldk;
  a.xcd_map = ((B * H) % 8 == 0) ? 1 : 0;
  g.k_ip = (const bf16_t*)k_ip; g.vt_ip = (const bf16_t*)vt_ip; g.ip_scale = ip_scale;
  g.vt_ip_bstride = (long)vt_ip_batch_stride; g.ldk_ip = ldk_ip; g.n_img = n_img;
  return 0;
}

// One launch over ga.n problems (ga.g filled): the deal of launch_attention_group's short-key branch, on the LK = 77 form when every problem has 77 keys
static int launch_attention_ip(void* stream, mx::AttnIpGroup& ga) {
  using namespace mx;
  const int n = ga.n;
  double flops = 0, bytes = 0;
  bool all77 = true;
  int max_nb = 1, maxLq = 0;
  for (int i = 0; i < n; ++i) {
    const AttnArgs& a = ga.g[i].a;
    flops += 4.0 * a.B * a.H * (double)a.Lq * (a.Lk + ga.g[i].n_img) * 64.0;
    bytes += 2.0 * a.B * a.H * 64.0 * (2.0 * a.Lq + 2.0 * a.Lk + 2.0 * XI_KEYS);
    all77 = all77 && a.Lk == 77;
    max_nb = std::max(max_nb, cdiv(a.Lq, 32));
    maxLq = std::max(maxLq, a.Lq);
  }
  // every wave of a (batch, head) takes `per` or `per - 1` consecutive 32-query blocks, `per` minimising rounds x (3 + 2.5 per) us (attention.hip)
  const long slots = 2L * cu_count();
  int best_per = 1; double best_t = 0;
  for (int per = 1; per <= max_nb; ++per) {
    long wgs = 0;
    for (int i = 0; i < n; ++i) wgs += (long)cdiv(cdiv(cdiv(ga.g[i].a.Lq, 32), per), 4) * ga.g[i].a.H * ga.g[i].a.B;
    const double t = (double)cdiv64(wgs, slots) * (3.0 + 2.5 * per);
    if (best_t == 0 || t < best_t - 1e-9) { best_t = t; best_per = per; }
    if (wgs <= slots) break;
  }
  long blocks = 0;
  for (int i = 0; i < n; ++i) {
    AttnArgs& a = ga.g[i].a;
    a.xq_wpb = cdiv(cdiv(a.Lq, 32), best_per);
    blocks = (blocks + 7) & ~7L;
    ga.blk0[i] = (int)blocks;
    ga.nblk[i] = cdiv(a.xq_wpb, 4) * a.H * a.B;
    blocks += ga.nblk[i];
  }
  for (int i = n; i < MX_MAX_SEGS; ++i) ga.nblk[i] = 0;
  for (int i = n; i <= MX_MAX_SEGS; ++i) ga.blk0[i] = (int)blocks;
  MX_CHECK(blocks < 2147483647L, "attention_ip: too many workgroups");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  const AttnArgs& a0 = ga.g[0].a;
  prof_begin(st, PROF_ATTN_CROSS, flops, bytes, n == 1 ? a0.B * a0.H : n, maxLq, a0.Lk);
  if (all77) hipLaunchKernelGGL((attn_cross_ip_kernel<77>), grid, block, 0, st, ga);
  else hipLaunchKernelGGL((attn_cross_ip_kernel<0>), grid, block, 0, st, ga);
  prof_end(st);
  MX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mx_attention_cross_ip(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, int64_t vt_batch_stride,
                                     const void* k_ip, int ldk_ip, const void* vt_ip, int64_t vt_ip_batch_stride, int n_img, const float* ip_scale, void* o,
                                     int ldo, int B, int H, int Lq, int Lk) {
  mx::AttnIpGroup ga;
  ga.n = 1;
  if (fill_ip_args(ga.g[0], q, ldq, k, ldk, vt, ldvt, vt_batch_stride, k_ip, ldk_ip, vt_ip, vt_ip_batch_stride, n_img, ip_scale, o, ldo, B, H, Lq, Lk)) return 1;
  return launch_attention_ip(stream, ga);
}

extern "C" int mx_attention_cross_ip_grouped(void* stream, const mx_attn_ip_problem* probs, int n, int ldq, int ldk, int ldk_ip, int ldo, int H) {
  MX_CHECK(probs != nullptr && n >= 1 && n <= MX_MAX_SEGS, "attention_ip: grouped launch needs 1..MX_MAX_SEGS problems");
  mx::AttnIpGroup ga;
  ga.n = n;
  for (int i = 0; i < n; ++i) {
    const mx_attn_ip_problem& p = probs[i];
    if (fill_ip_args(ga.g[i], p.q, ldq, p.k, ldk, p.vt, p.ldvt, p.vt_batch_stride, p.k_ip, ldk_ip, p.vt_ip, p.vt_ip_batch_stride, p.n_img, p.ip_scale, p.o, ldo,
                     p.B, H, p.Lq, p.Lk))
      return 1;
  }
  return launch_attention_ip(stream, ga);
}
