// Which way each of the BasicTransformerBlock's three LayerNorms reaches the GEMM it is folded into (weights.py fold_layernorm; mxdenoise.h,
// mx_gemm_desc.ln_stats / ln_final).  Decided HERE, once per Transformer2DModel, from the shape alone; the step plan (unet_sdxl.cpp) hands the
// answer to the producer and the consumer of each norm, and mx_unet_ln_routes answers the same question without a device.  Plain C++, no HIP.
//
//   Pass    mx_layernorm(gamma = NULL) over the hidden state y; the consumer reads the normalised copy and launches without statistics
//   Slabs   the launch that wrote y left (sum, sum of squares) per row and slab (stats_out); the consumer reads them (ln_stats)
//   Final   the producer also finalised (mean, rstd) per row (ln_final_out + the panel tickets); the consumer, on the 256 x 256 kernel, reads
//           those 8 bytes per row (ln_final)
//
// The 256 / 128-row kernels hide the statistics behind their first operand fetch; on the persistent 256 x 256 kernel applying the slabs costs more
// than a pass saves (mx_gemm_ln_prefers_pass: 10-20 us per launch against an 11-us pass at M = 8192, profiles/r03_h_ln_fold_on_256x256.txt), and
// the finalised form removes the pass where the producers run on 256-row tiles (profiles/r04_o_ln_final_microbench.txt, r04_q_ln_final_step_ab.txt).
// finalise(K, residual) below = mx_gemm_ln_final_supported on a plain M x C x K linear, with a residual of row stride C when `residual` is set.
//
//   norm  consumer      Pass                                  Final                                                          Slabs
//   1     q|k|v         prefers a pass, Final does not apply  not patch-parallel, tickets, one group, would be Pass,         otherwise
//                                                             finalise(C, no residual), layers == 1 or finalise(4C, residual)
//   2     attn2.to_q    prefers a pass                        never                                                          otherwise
//   3     GEGLU proj    prefers a pass, Final does not apply  not patch-parallel, tickets, would be Pass, and                otherwise
//                                                             no patch cache: finalise(C, residual)   (producer: attn2.to_out)
//                                                             patch cache: always                     (producer: the merge kernel; norm3_from_merge)
//
// One group only for norm1: its consumer is a GROUPED launch in a mixed batch, and ln_final excludes those; norm3's consumer is one ordinary launch over
// all rows whatever the mix.  Patch-parallel runs are compared bit for bit with the unsplit run and keep the pass.  norm2 has no Final: no shape puts
// attn2.to_q on the 256 x 256 kernel with a finalising producer in front of it.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/mxdenoise.h"

namespace mx {

enum class LnVia { Pass, Slabs, Final };
struct LnRoutes { LnVia norm1, norm2, norm3; bool norm3_from_merge; };

// the token rows in front of a transformer: per resolution group (one unless the batch is mixed) its rows and the tokens of one image
struct LnRows {
  int n_groups = 1;
  int rows[MX_MAX_SEGS] = {}, per_image[MX_MAX_SEGS] = {};
  int M() const { int m = 0; for (int g = 0; g < n_groups; ++g) m += rows[g]; return m; }
  // M rows in n equal groups of one image each (the last takes the remainder): what mx_unet_ln_routes assumes of a batch it is not shown
  static LnRows even(int M, int n) {
    LnRows t; t.n_groups = n;
    for (int g = 0; g < n; ++g) t.rows[g] = t.per_image[g] = g + 1 < n ? M / n : M - (n - 1) * (M / n);
    return t;
  }
};

// the shape of the fused q | k | v projection of width C over M rows of L tokens an image: the plan's launch and the query below fill the same fields
inline void ln_qkv_shape(mx_gemm_desc& d, int M, int C, int L) {
  d.lda = C; d.ldc = 2 * C; d.M = M; d.N = 3 * C; d.K = C; d.flags = MX_EPI_QKV; d.seg = C; d.period = 3; d.ldvt = MX_VT_LD(L);
  d.rows_per_batch = L; d.out_scale = MX_ATTN_QSCALE(0.125f);   // q segment only
}

inline LnRoutes ln_routes(const LnRows& t, int C, int layers, bool patch_parallel, bool patch_cache, bool tickets) {
  const int M = t.M();
  // one address stands for every operand: the chooser looks at which operands exist, at their 16-byte alignment and at how far a grouped launch's
  // problems lie apart, never at what they hold (the plan's own come from its 256-byte aligned arena)
  char* const x = reinterpret_cast<char*>(uintptr_t(1) << 20);
  auto linear = [&](int N, int K, int ldc, int flags, float out_scale, bool residual) {
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.a = x; d.w = x; d.c = x; d.lda = K; d.ldc = ldc; d.M = M; d.N = N; d.K = K; d.flags = flags; d.out_scale = out_scale;
    if (residual) { d.residual = x; d.ldr = C; }
    return d;
  };
  mx_gemm_desc qkv; std::memset(&qkv, 0, sizeof(qkv));
  mx_gemm_seg segs[MX_MAX_SEGS];
  qkv.a = x; qkv.w = x; qkv.c = x; qkv.vt = x;
  ln_qkv_shape(qkv, M, C, t.per_image[0]);
  if (t.n_groups > 1) {
    std::memset(segs, 0, sizeof(segs));
    long r0 = 0;
    for (int g = 0; g < t.n_groups; ++g) {
      segs[g].a = x + r0 * C * 2; segs[g].c = x + r0 * 2 * C * 2; segs[g].vt = x;
      segs[g].M = t.rows[g]; segs[g].rows_per_batch = t.per_image[g]; segs[g].ldvt = MX_VT_LD(t.per_image[g]);
      r0 += t.rows[g];
    }
    qkv.segs = segs; qkv.n_segs = t.n_groups;
  }
  const mx_gemm_desc to_q = linear(C, C, C, 0, MX_ATTN_QSCALE(0.125f), false), geglu = linear(8 * C, C, 4 * C, MX_EPI_GEGLU, 0.f, false);
  auto finalise = [&](int K, bool residual) { const mx_gemm_desc d = linear(C, K, C, 0, 0.f, residual); return mx_gemm_ln_final_supported(&d) != 0; };
  const bool may_finalise = !patch_parallel && tickets;
  LnRoutes r;
  r.norm1 = !mx_gemm_ln_prefers_pass(&qkv) ? LnVia::Slabs
          : may_finalise && t.n_groups == 1 && finalise(C, false) && (layers == 1 || finalise(4 * C, true)) ? LnVia::Final : LnVia::Pass;
  r.norm2 = mx_gemm_ln_prefers_pass(&to_q) ? LnVia::Pass : LnVia::Slabs;
  r.norm3 = !mx_gemm_ln_prefers_pass(&geglu) ? LnVia::Slabs : may_finalise && (patch_cache || finalise(C, true)) ? LnVia::Final : LnVia::Pass;
  r.norm3_from_merge = patch_cache && r.norm3 == LnVia::Final;
  return r;
}

}  // namespace mx
