// Regional prompts ("attention couple"): short-key cross-attention over SEVERAL separately normalised key sets, blended per query token, one launch.
//
//   O[b, i, h, :] = sum over r < counts[b] of  w[b, r, i] * softmax_j(q_i . k_{b,r,j}) v_{b,r}          (q prescaled, log2 domain)
//
// Every set is a prompt of seg_len <= 96 keys with its own maximum and its own sum; w comes from the client's masks and is not normalised here.  Set r of
// sample b is the seg_len rows of k from row (b * n_sets + r) * seg_ld, seg_ld = MX_VT_LD(seg_len), and the keys [r * seg_ld, r * seg_ld + seg_len) of the
// sample's V^T rows: what the MX_EPI_QKV projection writes for a context of n_sets * seg_ld rows.  Every set starts on a 16-key group of the V^T order.
//
// Work split: one workgroup of 4 waves per slice of a (batch, head), dealt as attn_cross_kernel deals its waves (xq_wpb, `per` 32-query blocks a wave).
// The 24 fragments of ONE set fill 96 registers, so several sets cannot be resident the way the short-key kernel keeps its one; and a 32-query block of a
// 32-wide level is a whole image row, which touches every column region, so swapping sets through registers would reload per block.  Instead the
// workgroup stages its sample's counts[b] sets ONCE into LDS and every wave pulls the fragments of a (block, live set) from there:
//   * K of a set: seg_ld rows of 128 B, 16-byte chunk ^= (row >> 1) & 7 (the tiled kernels' swizzle: the 16 lanes of a b128 read phase hit 16 chunks);
//     only rows < seg_len are staged, and a fragment row >= seg_len reads row 0 instead: its scores are replaced by -inf whatever they are;
//   * V^T of a set: per 16-key step 64 feature rows of 32 B, the row's two chunks swapped where (row >> 3) & 1; key positions >= seg_len are zeroed on
//     the way in (their P is exactly 0, and 0 * NaN must not reach the accumulator);
//   * seg_ld * 256 B a set (20 KB at 77 keys) behind the four 4-KB output patches; sized by n_sets: two sets keep two workgroups on a CU, four leave one;
//   * one barrier behind the staging; every wave, with or without queries of its own, stages and reaches it.
// Per 32-query block the lane owns one query (lane & 31), so w[b, r, q] is a per-lane scalar:
//   * a set whose weight is zero for every valid query of the block is skipped after one ballot (wave-uniform): disjoint masks cost one or two sets a block;
//   * a live set: S^T = K_r Q^T, its own softmax, p * (w / sum) in fp32, ONE rounding to bf16, O^T += V_r^T P^T into the block's two accumulators;
//   * the accumulators are rounded once and leave through the wave's patch as whole rows (xk_block's layout).
// counts[b] == 1 (workgroup-uniform): no staging, no barrier, no weight is read -- the wave loads set 0 into registers and runs xk_block<true, LK>, so such
// a sample is bit-equal to mx_attention_cross_prescaled over those keys (the branch attention_ip.hip takes for ip_scale == 0).
// The waves-per-block cost model (3 + 2.5 per microseconds a round) is the plain kernel's, reused unfitted; profiles/regions.txt has the launch's times.
#include <algorithm>
#include <mutex>

#include "common.h"
#include "../../include/mxdenoise.h"
#include "attn_tile.h"
#include "attn_cross_body.h"

namespace mx {

constexpr int XR_PATCH = 4 * 4096;             // the four waves' output patches, in front of the sets
__host__ __device__ constexpr int xr_set_bytes(int seg_len) { return MX_VT_LD(seg_len) * 256; }      // K then V^T, seg_ld * 128 B each
constexpr int XR_MAX_LDS = XR_PATCH + MX_REGION_SETS * xr_set_bytes(32 * XK_MAXBLK);
static_assert(XR_MAX_LDS <= 160 * 1024, "four sets of 96 keys must fit in a workgroup's LDS");

struct AttnRegionArgs {
  AttnArgs a;                                  // q, o, the strides, B, H, Lq; Lk = seg_len; k / vt = the whole buffers (xq_wpb: the waves of a (batch, head))
  const float* weights;                        // [B, n_sets, Lq]
  const int* counts;                           // [B]
  int n_sets;
};

// ---- staging: set `r` of (b, head) into `dst` (K image, then the V^T image), by all 256 threads ----
template <int LK>
__device__ __forceinline__ void xr_stage(const AttnRegionArgs& ra, const int b, const int head, const int r, char* const dst, const int tid) {
  const AttnArgs& p = ra.a;
  const int Lk = LK > 0 ? LK : p.Lk;
  const int seg_ld = MX_VT_LD(Lk);
  const bf16_t* kg = p.k + ((long)(b * ra.n_sets + r) * seg_ld) * p.ldk + head * 64;
  for (int c = tid; c < Lk * 8; c += 256) {
    const int row = c >> 3, ch = c & 7;
    *reinterpret_cast<u32x4*>(dst + row * 128 + ((ch ^ ((row >> 1) & 7)) * 16)) = *reinterpret_cast<const u32x4*>(kg + (long)row * p.ldk + ch * 8);
  }
  const int cpr = seg_ld >> 3;                 // 16-byte chunks of a set's V^T row
  const bf16_t* vg = p.vt + (long)b * p.vt_bstride + ((long)head * 64) * p.ldvt + r * seg_ld;
  char* const vdst = dst + seg_ld * 128;
  for (int c = tid; c < 64 * cpr; c += 256) {
    const int d = c / cpr, cc = c - d * cpr;
    const int st = cc >> 1, hh = cc & 1;
    u32x4 v = *reinterpret_cast<const u32x4*>(vg + (long)d * p.ldvt + cc * 8);
    const int kbase = st * 16 + 4 * hh;        // word e holds keys kbase + 2 (e & 1) + 8 (e >> 1) and the next (xk_vfrag)
    if (kbase + 12 > Lk) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k0 = kbase + 2 * (e & 1) + 8 * (e >> 1);
        unsigned w = v[e];
        if (k0 >= Lk) w &= 0xffff0000u;
        if (k0 + 1 >= Lk) w &= 0x0000ffffu;
        v[e] = w;
      }
    }
    *reinterpret_cast<u32x4*>(vdst + st * 2048 + d * 32 + ((hh ^ ((d >> 3) & 1)) * 16)) = v;
  }
}

// One 32-query block over the sample's `count` staged sets.  w0 = this lane's weight of set 0 (0 for a query past the end); koff / voff: the lane's
// fragment offsets inside a set's K and V^T images.
template <int LK>
__device__ __forceinline__ void xr_block(const AttnArgs& p, const int b, const int head, const int q0, const bf16x8 (&qf)[4], const char* const sets,
                                         const int count, const float* const wrow, const unsigned (&koff)[XK_MAXBLK][4], const unsigned voff,
                                         char* const patch, const int lane) {
#pragma clang fp contract(off)
  const int r = lane & 31;
  const int hh = lane >> 5;
  const int Lk = LK > 0 ? LK : p.Lk;
  const int nblk = (Lk + 31) >> 5;
  const int nst = (Lk + 15) >> 4;
  const int seg_ld = MX_VT_LD(Lk);
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int qi = q0 + r;
  const bool valid = qi < p.Lq;
  f32x16 oacc[2] = {zero16, zero16};
  float w = valid ? wrow[qi] : 0.f;
  for (int set = 0; set < count; ++set) {
    const float wn = (valid && set + 1 < count) ? wrow[(long)(set + 1) * p.Lq + qi] : 0.f;      // the next set's weight, under this set's arithmetic
    if (__ballot(w != 0.f) != 0) {             // wave-uniform: a set no valid query of the block weights costs nothing more
      const char* const kimg = sets + set * (seg_ld * 256);
      const char* const vimg = kimg + seg_ld * 128;
      // ---- S^T = K_set Q^T ----
      f32x16 s[XK_MAXBLK];
#pragma unroll
      for (int kb = 0; kb < XK_MAXBLK; ++kb) {
        s[kb] = zero16;
        if (kb < nblk) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(kimg + koff[kb][ks]), qf[ks], s[kb], 0, 0, 0);
        }
      }
      // ---- the set's own softmax (block kb element e = key 32 kb + (e & 3) + 8 (e >> 2) + 4 hh) ----
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
      mx_ = max_across_halves(mx_);            // key 0 is always there: finite
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
      const float ws = w / (psum + __shfl_xor(psum, 32, 64));
      // ---- O^T += V_set^T (w / sum * P)^T ----
#pragma unroll
      for (int st = 0; st < 2 * XK_MAXBLK; ++st) {
        if (st >= nst) continue;
        const int kb = st >> 1, s2 = st & 1;
        u32x4 pw;
#pragma unroll
        for (int e = 0; e < 4; ++e) pw[e] = pack2(s[kb][8 * s2 + 2 * e] * ws, s[kb][8 * s2 + 2 * e + 1] * ws);
        const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
#pragma unroll
        for (int db = 0; db < 2; ++db)
          oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(vimg + voff + st * 2048 + db * 1024), pf, oacc[db], 0, 0, 0);
      }
    }
    w = wn;
  }
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
    const int qo = q0 + row;
    if (qo < p.Lq) *reinterpret_cast<u32x4*>(p.o + ((long)b * p.Lq + qo) * p.ldo + head * 64 + ch * 8) = o;
  }
}

template <int LK = 0>
__global__ __launch_bounds__(256, 2) void attn_regions_kernel(const AttnRegionArgs ra) {
  extern __shared__ __attribute__((aligned(16))) char smem[];      // XR_PATCH, then n_sets images of xr_set_bytes
  const AttnArgs& p = ra.a;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // workgroup -> (workgroup of the (batch, head) pair, batch * H + head): the short-key kernel's map
  const int lin = blockIdx.x;
  const int gx = (p.xq_wpb + 3) >> 2;
  int qb, bh;
  if (p.xcd_map) {
    const int local = lin >> 3;
    qb = local % gx;
    bh = ((local / gx) << 3) + (lin & 7);
  } else {
    qb = lin % gx;
    bh = lin / gx;
  }
  const int b = bh / p.H, head = bh % p.H;
  int count = __builtin_amdgcn_readfirstlane(ra.counts[b]);
  count = count < 1 ? 1 : (count > ra.n_sets ? ra.n_sets : count);      // (the host states 1 .. n_sets; nothing outside the launch's sets is ever addressed)
  const int w = __builtin_amdgcn_readfirstlane(qb * 4 + wave);
  const bool active = w < p.xq_wpb;
  const int nb = (p.Lq + 31) >> 5;
  const int base = nb / p.xq_wpb, rem = nb - base * p.xq_wpb;
  const int q_wave0 = (w * base + (w < rem ? w : rem)) * 32;
  const int nblocks = base + (w < rem ? 1 : 0);
  char* const patch = smem + wave * 4096;
  const int Lk = LK > 0 ? LK : p.Lk;
  const int seg_ld = MX_VT_LD(Lk);

  if (count == 1) {                            // workgroup-uniform: the plain short-key wave on set 0, fragments in registers, no barrier
    if (!active) return;
    AttnArgs ps = p;                           // set 0 of sample b as a one-sample problem for xk_kfrag / xk_vfrag (batch 0)
    ps.k = p.k + ((long)b * ra.n_sets * seg_ld) * p.ldk;
    ps.vt = p.vt + (long)b * p.vt_bstride;
    bf16x8 kf[XK_MAXBLK][4];
#pragma unroll
    for (int kb = 0; kb < XK_MAXBLK; ++kb)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) kf[kb][ks] = xk_kfrag<LK>(ps, 0, head, kb, ks, lane);
    bf16x8 vf[2 * XK_MAXBLK][2];
#pragma unroll
    for (int st = 0; st < 2 * XK_MAXBLK; ++st)
#pragma unroll
      for (int db = 0; db < 2; ++db) vf[st][db] = xk_vfrag<LK>(ps, 0, head, st, db, lane);
    bf16x8 qf[4], qn[4];
    load_q(p, b, head, q_wave0, lane, qf);
    for (int blk = 0; blk < nblocks; ++blk) {
      const int q0 = q_wave0 + blk * 32;
      if (q0 >= p.Lq) break;                   // wave-uniform
      if (blk + 1 < nblocks) load_q(p, b, head, q0 + 32, lane, qn);
      xk_block<true, LK>(p, b, head, q0, qf, [&](int kb, int ks) __attribute__((always_inline)) { return kf[kb][ks]; },
                         [&](int st, int db) __attribute__((always_inline)) { return vf[st][db]; }, patch, lane);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
    }
    return;
  }

  char* const sets = smem + XR_PATCH;
  for (int r = 0; r < count; ++r) xr_stage<LK>(ra, b, head, r, sets + r * (seg_ld * 256), tid);
  __syncthreads();                             // every wave of the workgroup is here: none has returned
  if (!active) return;

  const int r = lane & 31, hh = lane >> 5;
  unsigned koff[XK_MAXBLK][4];
#pragma unroll
  for (int kb = 0; kb < XK_MAXBLK; ++kb) {
    const int key = kb * 32 + r;
    const int row = key < Lk ? key : 0;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) koff[kb][ks] = (unsigned)(row * 128 + (((2 * ks + hh) ^ ((row >> 1) & 7)) * 16));
  }
  const unsigned voff = (unsigned)(r * 32 + ((hh ^ ((r >> 3) & 1)) * 16));
  const float* const wrow = ra.weights + (long)b * ra.n_sets * p.Lq;
  bf16x8 qf[4], qn[4];
  load_q(p, b, head, q_wave0, lane, qf);
  for (int blk = 0; blk < nblocks; ++blk) {
    const int q0 = q_wave0 + blk * 32;
    if (q0 >= p.Lq) break;                     // wave-uniform
    if (blk + 1 < nblocks) load_q(p, b, head, q0 + 32, lane, qn);
    xr_block<LK>(p, b, head, q0, qf, sets, count, wrow, koff, voff, patch, lane);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
  }
}

}  // namespace mx

extern "C" int mx_attention_cross_regions(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, int64_t vt_batch_stride,
                                          const float* weights, const int32_t* counts, void* o, int ldo, int B, int H, int Lq, int n_sets, int seg_len) {
  using namespace mx;
  MX_CHECK(q && k && vt && o && weights && counts, "attention_regions: null operand");
  MX_CHECK(B > 0 && H > 0 && Lq > 0, "attention_regions: empty problem");
  MX_CHECK(n_sets >= 1 && n_sets <= MX_REGION_SETS, "attention_regions: n_sets must be in 1.." + std::to_string(MX_REGION_SETS));
  MX_CHECK(seg_len >= 1 && seg_len <= 32 * XK_MAXBLK, "attention_regions: a set needs 1..96 keys");
  MX_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)o) & 15) == 0 && (((uintptr_t)weights | (uintptr_t)counts) & 3) == 0,
           "attention_regions: operand pointers must be 16-byte aligned (weights, counts: 4)");
  MX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 8 == 0, "attention_regions: strides must be multiples of 8 elements");
  MX_CHECK(ldq >= H * 64 && ldk >= H * 64 && ldo >= H * 64, "attention_regions: row stride smaller than H*64");
  const int seg_ld = MX_VT_LD(seg_len);
  MX_CHECK(ldvt >= n_sets * seg_ld, "attention_regions: ldvt must cover n_sets * MX_VT_LD(seg_len)");
  MX_CHECK(vt_batch_stride % 8 == 0 && vt_batch_stride >= (int64_t)H * 64 * ldvt, "attention_regions: bad vt_batch_stride");
  AttnRegionArgs ra;
  AttnArgs& a = ra.a;
  a = AttnArgs{};
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.vt = (const bf16_t*)vt; a.o = (bf16_t*)o;
  a.vt_bstride = (long)vt_batch_stride;
  a.ldq = ldq; a.ldk = ldk; a.ldvt = ldvt; a.ldo = ldo; a.B = B; a.H = H; a.Lq = Lq; a.Lk = seg_len;
  a.scale_log2 = 1.4426950408889634f;          // (prescaled q: unused)
  a.xcd_map = ((B * H) % 8 == 0) ? 1 : 0;
  ra.weights = weights; ra.counts = counts; ra.n_sets = n_sets;
  const int lds = XR_PATCH + n_sets * xr_set_bytes(seg_len);
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [] {
    attr = hipFuncSetAttribute((const void*)attn_regions_kernel<77>, hipFuncAttributeMaxDynamicSharedMemorySize, XR_MAX_LDS);
    if (attr == hipSuccess) attr = hipFuncSetAttribute((const void*)attn_regions_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, XR_MAX_LDS);
  });
  MX_CHECK(attr == hipSuccess, std::string("attention_regions: ") + hipGetErrorString(attr));
  // every wave of a (batch, head) takes `per` or `per - 1` consecutive 32-query blocks, `per` minimising rounds x (3 + 2.5 per) us: the plain short-key
  // kernel's model (attention.hip), not refitted for this one; a CU holds two workgroups while two images of the launch's LDS fit in its 160 KB
  const long slots = (2 * lds <= 160 * 1024 ? 2L : 1L) * cu_count();
  const int nb = cdiv(Lq, 32);
  int best_per = 1; double best_t = 0;
  for (int per = 1; per <= nb; ++per) {
    const long wgs = (long)cdiv(cdiv(nb, per), 4) * H * B;
    const double t = (double)cdiv64(wgs, slots) * (3.0 + 2.5 * per);
    if (best_t == 0 || t < best_t - 1e-9) { best_t = t; best_per = per; }
    if (wgs <= slots) break;
  }
  a.xq_wpb = cdiv(nb, best_per);
  const long blocks = (long)cdiv(a.xq_wpb, 4) * H * B;
  MX_CHECK(blocks < 2147483647L, "attention_regions: too many workgroups");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  prof_begin(st, PROF_ATTN_CROSS, 4.0 * B * H * (double)Lq * n_sets * seg_len * 64.0, 2.0 * B * H * 64.0 * (2.0 * Lq + 2.0 * n_sets * seg_len), B * H, Lq,
             n_sets * seg_len);
  if (seg_len == 77) hipLaunchKernelGGL((attn_regions_kernel<77>), grid, block, lds, st, ra);
  else hipLaunchKernelGGL((attn_regions_kernel<0>), grid, block, lds, st, ra);
  prof_end(st);
  MX_LAUNCH_CHECK();
  return 0;
}
