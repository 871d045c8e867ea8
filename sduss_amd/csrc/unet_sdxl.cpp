// Step plan of the SDXL UNet in the sduss model slot: a flat sequence of kernel launches on one HIP
// stream over NHWC/token-major bf16 activations in a caller-provided workspace (stack arena).
//
// Replaces PatchUNet.forward (sduss/model_executor/modules/unet.py:205-530) and the Patch* modules it
// drives (resnet.py:380-460, transformer.py:32-128,167-290, attention.py:59-232, unet_2d_blocks.py),
// computing on WHOLE latents:
//   is_sliced=False  -> gn_patch = 0: exact GroupNorm, zero-padded convs (the diffusers-equivalent branch);
//   is_sliced=True   -> gn_patch = p: patch-averaged GroupNorm statistics + the halo-corner rule in the conv
//                       loader, which is arithmetically the reference's patch pipeline (oracle/patch_ref.py
//                       proves the equivalence on CPU) without cutting, halo tensors or host loops.
// Design notes (MI355X-first, not a module-by-module translation):
//   * NHWC == token-major, so Transformer2DModel's permutes (transformer.py:57-60, 91-95) vanish;
//   * self-attention q/k/v are ONE fused GEMM whose epilogue writes V transposed for the attention kernel;
//   * the 70 cross-attention K/V projections of encoder_hidden_states are hoisted into one GEMM per width;
//   * the 17 time_emb_proj linears are one GEMM; its fp32 rows are added in conv1's epilogue;
//   * GEGLU, bias, residual adds and the nearest-2x upsample are fused into GEMM/conv epilogues/loaders.
// Host scaffold (arena, weight lookup, groups, block-cache bookkeeping, the forward driver): plan_base.h; this file holds the UNet's own plan,
// its checks and hooks (struct Model) and the extern "C" entry points, each of which describes its forward as an mx::ForwardCall.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/mxdenoise.h"
#include "common.h"
#include "graph_cache.h"
#include "ln_route.h"
#include "patch_cache.h"
#include "plan_base.h"

namespace mx {
int launch_prep_latent(hipStream_t s, const void* in, int dtype, void* out, int B, int Cin, int HW, int CP);
int launch_nhwc_to_nchw(hipStream_t s, const void* in, void* out, int dtype, int B, int C, int HW, int ld);
int launch_time_embed(hipStream_t s, const float* timesteps, const void* text_embeds, const float* time_ids,
                      void* tsin, void* addin, int B, int d0, int text_dim, int da);
size_t gn_workspace_exact(int B, int H, int W, int C, int patch);
int launch_sq_diff_partial(hipStream_t s, const void* a, const void* b, long elems_per_sample, int B, double* partial, const int* slot = nullptr);
int launch_gn_pp_partial(hipStream_t s, const void* x, int C1, const void* x2, int B, int H, int W, int C, int groups, void* workspace, double* sums);
int launch_gn_pp_finish(hipStream_t s, const void* x, int C1, const void* x2, void* y, long y_img_elems, const float* gamma, const float* beta, const double* all_sums,
                        int world, int B, int H, int W, int C, int groups, int H_total, float eps, int silu, void* workspace,
                        const double* fresh_own = nullptr, int own_rank = 0);
}  // namespace mx
extern "C" int mx_attention_prescaled_chunked(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                              int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk, int key_chunk,
                                              int64_t k_batch_stride, int64_t k_chunk_stride, int64_t vt_chunk_stride);

using mx::bf16_t;
using mx::LnVia;

struct mx_unet {
  mx_unet_config cfg;
  mx::WeightTable weights;
  mx::GraphCache graphs;   // hipGraph replay of the forward, keyed by its arguments (graph_cache.h)
  mx::PinnedBuf skip_pin;  // the per-block read-back of the device-side skip decision (mx_block_cache.dev_down)
  // patch-parallel stale forwards: the exchange sizes of the plan, recorded by a host-only walk ONCE per (batch, H, W, ctx_len, gn_patch, world) instead
  // of at every step (advisor, round 3: the walk sat on the path whose purpose is to hide latency)
  std::map<std::vector<long>, std::vector<size_t>> pp_sizes;
  // ---- per-composition store of the cross-attention K / V^T of encoder_hidden_states (mx_unet_set_context_key, mxdenoise.h).  The text
  // embeddings of a request are constant over its 50 steps (pipeline_stable_diffusion_xl_esymred.py:287-339 re-concatenates the same tensors every
  // step), so the hoisted projection -- M = B * 77, N = 2 * layers * dim, K = 2048 per attention width, 0.47 ms of the headline step -- is computed
  // once per batch composition and read from library-owned buffers afterwards: same GEMM, same bits.  A few entries (compositions alternate when
  // the resolutions of a mixed batch run as separate sequences on separate streams); an entry is handed from one stream to another through the
  // event its last forward recorded. ----
  struct CtxEntry {
    uint64_t key = 0; int B = 0, ctx_len = 0; bool valid = false; uint64_t stamp = 0;
    std::vector<bf16_t*> k, vt; std::vector<size_t> k_bytes, vt_bytes;
    hipEvent_t ev = nullptr; hipStream_t last = nullptr; bool recorded = false;
  };
  uint64_t ctx_key = 0;                 // the NEXT forward's composition (mx_unet_set_context_key; consumed by that forward); 0 = project encoder_hidden_states again
  std::vector<CtxEntry> ctx_store;
  uint64_t ctx_clock = 0;
  long ctx_hits = 0, ctx_misses = 0;
  void ctx_clear() {
    for (auto& e : ctx_store) {
      if (e.last) (void)hipStreamSynchronize(e.last);
      for (auto* q : e.k) if (q) (void)hipFree(q);
      for (auto* q : e.vt) if (q) (void)hipFree(q);
      if (e.ev) (void)hipEventDestroy(e.ev);
    }
    ctx_store.clear();
  }
  ~mx_unet() { ctx_clear(); }
};

namespace {

constexpr int kConvInPad = 64;  // conv_in input channels are zero-padded to one K tile

// (attention width, cross-attention layers of that width) in execution order of first use: the layout of the hoisted K / V^T buffers
static std::vector<std::pair<int, int>> kv_widths(const mx_unet_config& c) {
  const int nlev = c.n_levels;
  std::vector<std::pair<int, int>> widths;
  auto add = [&](int dim, int n) { for (auto& wv : widths) if (wv.first == dim) { wv.second += n; return; } widths.push_back({dim, n}); };
  for (int i = 0; i < nlev; ++i) if (c.down_has_attn[i]) add(c.block_out_channels[i], c.layers_per_block * c.transformer_layers[i]);
  add(c.block_out_channels[nlev - 1], c.transformer_layers[nlev - 1]);
  for (int i = 0; i < nlev; ++i) { const int lv = nlev - 1 - i; if (c.down_has_attn[lv]) add(c.block_out_channels[lv], (c.layers_per_block + 1) * c.transformer_layers[lv]); }
  return widths;
}

// ---- the arguments of Plan::linear() and Plan::conv() by name: a call states the required fields in order and adds what else it means ----
// row statistics (sum, sum of squares per row and slab) of the hidden states: what the folded LayerNorms read (mx_gemm_desc.ln_stats)
// fin / cnt: the FINALISED form (mean, rstd per row: mx_gemm_desc.ln_final) for consumers on the 256 x 256 kernel; cnt = the producers' panel tickets
struct RowStats { float* buf = nullptr; int slabs = 0; float* fin = nullptr; unsigned* cnt = nullptr; };
struct Linear {
  const bf16_t* a; int lda; std::string stem; void* c; int ldc; int M, N, K;      // c[M, N] = a[M, K] * "<stem>.weight"^T + "<stem>.bias"
  const void* residual = nullptr; int ldr = 0; int flags = 0; float out_scale = 0.f;
  const bf16_t* a2 = nullptr; int lda2 = 0;
  const RowStats* ln = nullptr; LnVia ln_via = LnVia::Pass;
  RowStats* stats_out = nullptr; LnVia stats_via = LnVia::Pass;
  Linear& plus(const void* r, int ld) { residual = r; ldr = ld; return *this; }
  Linear& epilogue(int f) { flags = f; return *this; }
  Linear& scaled(float s) { out_scale = s; return *this; }
  Linear& concat(const bf16_t* x2, int ld2) { a2 = x2; lda2 = ld2; return *this; }                  // A = [a | a2] along K (a2 null: a alone)
  // the LayerNorm in front of this linear is folded into it (weights.py fold_layernorm) and reaches it by route via (ln_route.h): Slabs / Final = a is the
  // UN-normalised hidden state with statistics st and column sums "<stem>.colsum"; Pass = nothing, a is already normalised
  Linear& folded_ln(const RowStats& st, LnVia via) { ln = &st; ln_via = via; return *this; }
  // the LayerNorm BEHIND this linear reaches its consumer by route via: Slabs = also leave the statistics of the output rows in st, Final = and
  // finalise them; Pass = nothing
  Linear& leaves_stats(RowStats& st, LnVia via) { stats_out = &st; stats_via = via; return *this; }
};
// where a 3x3 conv reads: the tensor and, patch-parallel, the base of the padded image it is the interior of (one halo row above and below)
struct ConvIn { bf16_t* t = nullptr; bf16_t* padded = nullptr; };
struct Conv {
  ConvIn in; int Hin, Win, Cin; std::string prefix; bf16_t* out; int Cout;         // (Hin, Win: the first group's image)
  int stride = 1, up = 0, corner_patch = 0;
  const float* rowbias = nullptr; int ldrb = 0; const void* residual = nullptr;
  float* gn_part = nullptr; bool* gn_done = nullptr;
  Conv& strided(int s) { stride = s; return *this; }
  Conv& upsampled() { up = 1; return *this; }                                      // nearest-2x in the loader
  Conv& row_bias(const float* rb, int ld) { rowbias = rb; ldrb = ld; return *this; }
  Conv& plus(const void* r) { residual = r; return *this; }
  // ask the launch to leave the GroupNorm partial sums of its output (mx_gemm_desc.gn_part_out); *done tells whether it could
  Conv& gn_partials(float* part, bool* done) { gn_part = part; gn_done = done; return *this; }
};

struct Plan : mx::DenoiserPlan {      // (stream, arena, weights, groups, exchange, block-cache bookkeeping: plan_base.h)
  mx_unet* u;
  int ctx_len, gn_patch;
  // Mixed-resolution batch (mx_unet_forward_mixed): the requests of every resolution present run through ONE launch sequence.  A group = the
  // samples of one resolution; activations of a level are the groups' token-major images one after the other ([sum_g B_g h_g w_g, C]), so every
  // per-token op (linear layers, LayerNorm) is one ordinary launch over all rows, and the ops with per-image structure (3x3 convs, GroupNorm,
  // the QKV epilogue's V^T, attention) are GROUPED launches: one problem per group, no tile straddling two groups (include/mxdenoise.h,
  // mx_gemm_seg).  The reference reaches the same end by cutting every latent into 256-px patches of one batch (modules/unet.py:104-185).
  int ch[MX_MAX_SEGS], cw[MX_MAX_SEGS];                                       // per group: image size at the CURRENT level
  long rows() const { long m = 0; for (int g = 0; g < ng; ++g) m += (long)gB[g] * ch[g] * cw[g]; return m; }
  long row0(int g) const { long m = 0; for (int k = 0; k < g; ++k) m += (long)gB[k] * ch[k] * cw[k]; return m; }
  char* bc_top = nullptr;         // bump pointer into bc->state: same order and sizes every step
  std::vector<int> bc_sel;               // selection table of a partially reused block (host copy kept for the forward's lifetime)
  // head of the state: comparison partial sums, the slot table, the selection table of a partially reused block
  static constexpr int kBcTables = 2;
  static int bc_part_rows(int lpb) { return lpb + 2; }
  static size_t bc_scratch_bytes(int lpb, int rows) { return bc_head_bytes(bc_part_rows(lpb), kBcTables, rows); }
  int* bc_dsel() const { return bc_table(bc_part_rows(u->cfg.layers_per_block), 1); }
  // ---- block cache at the reference's own unit, the PATCH (mx_unet_forward_cached_mixed; cache_manager.py with is_sliced=True) ----
  // Every cached op of a block (resnet conv1 / conv2, the down / upsampler conv, attn1.to_out, attn2.to_out: the modules that own a CacheManager,
  // resnet.py:283,339,386-387; attention.py:57,118) keeps its output per patch in a STATE tensor with one row per request; under a partial
  // mask the asking patches are computed -- convs on a compact batch of halo'd patches, per-token work on the compact rows -- and written to
  // their places in the state, and the op's output is the state, for asking and not-asking patches alike.  Everything else of a running block
  // (GroupNorm with its statistics and halos, LayerNorms, proj_in / proj_out, the q / k / v projections of attn1, the feed-forward, the 1x1
  // shortcut, the residual adds) runs on all rows, as in the reference.
  bool pc = false;
  int pc_p0 = 0, pc_np = 0, pc_nask = 0, pc_maxh = 0, pc_maxw = 0, pc_slots = 0;
  bool pc_partial = false;          // the running block: some patch of the batch does not ask
  std::vector<mx::PcSample> pc_samp;
  std::vector<mx::PcPatch> pc_all, pc_ask;
  std::vector<int> pc_ask_first;    // per sample: index of its first asking patch in pc_ask (B + 1 entries)
  std::vector<int> pc_group_of;     // per sample: its resolution group
  mx::PcSample* pc_dsamp = nullptr; mx::PcPatch* pc_dall = nullptr; mx::PcPatch* pc_dask = nullptr; double* pc_dpart = nullptr;
  unsigned long long pc_asked = 0, pc_total = 0;
  static size_t pc_np_max(int slots, int maxh, int maxw, int p0) { return (size_t)slots * (maxh / p0) * (maxw / p0); }
  size_t pc_head_bytes(int slots, int maxh, int maxw, int p0) const {     // comparison partial sums | sample table | all patches | asking patches
    const size_t np = pc_np_max(slots, maxh, maxw, p0);
    return (((size_t)(u->cfg.layers_per_block + 2) * np * p0 * sizeof(double) + slots * sizeof(mx::PcSample) + 2 * np * sizeof(mx::PcPatch)) + 255) & ~(size_t)255;
  }
  long pc_row_elems(int level, int C) const { return (long)(pc_maxh >> level) * (pc_maxw >> level) * C; }
  long pc_max_image(int level, int C) const { long m = 0; for (int g = 0; g < ng; ++g) m = std::max(m, (long)(gH[g] >> level) * (gW[g] >> level) * C); return m; }
  char* pc_region(int level, int C) {
    char* r = bc_top;
    bc_top += ((size_t)pc_row_elems(level, C) * pc_slots * 2 + 255) & ~(size_t)255;
    if (!dry && (size_t)(bc_top - (char*)bc->state) > bc->state_bytes) fail("patch cache: state buffer too small (mx_unet_patch_cache_bytes)");
    return r;
  }
  bool pc_store(const bf16_t* t, char* reg, int level, int C) {
    if (!ok()) return false;
    if (quiet()) return true;
    if (mx::launch_pc_image_copy(stream, (void*)t, reg, pc_dsamp, B, level, C, pc_row_elems(level, C), 0, nullptr, 0, nullptr, pc_max_image(level, C))) return fail(mx_last_error());
    return true;
  }
  // t = state (+ vec[b][c]) (+ residual); residual may be t itself
  bool pc_load(bf16_t* t, char* reg, int level, int C, const float* vec = nullptr, int ldvec = 0, const bf16_t* residual = nullptr, bool force = false) {
    if (!ok()) return false;
    if (dry || (mute && !force)) return true;
    if (mx::launch_pc_image_copy(stream, t, reg, pc_dsamp, B, level, C, pc_row_elems(level, C), 1, vec, ldvec, residual, pc_max_image(level, C))) return fail(mx_last_error());
    return true;
  }
  // t = state + residual, token row by token row, leaving the row statistics of t (round 5: patch_cache.hip pc_rows_load_stats): stats1 = the one-slab form
  // ([rows][4][2] floats: sum, sum of squares) read by the folded LayerNorm of the 256 / 128-row GEMMs, fin = (mean, rstd) per row for the 256 x 256 kernel
  bool pc_load_stats(bf16_t* t, char* reg, int level, int C, const bf16_t* residual, float* stats1, float* fin) {
    if (!ok()) return false;
    if (dry || mute) return true;
    long max_rows = 0;
    for (int g = 0; g < ng; ++g) max_rows = std::max(max_rows, (long)(gH[g] >> level) * (gW[g] >> level));
    if (mx::launch_pc_rows_load_stats(stream, t, reg, pc_dsamp, B, level, C, pc_row_elems(level, C), residual, stats1, fin, u->cfg.layer_norm_eps, max_rows)) return fail(mx_last_error());
    return true;
  }
  const mx::PcPatch* pc_list() const { return pc_partial ? pc_dask : pc_dall; }
  int pc_count() const { return pc_partial ? pc_nask : pc_np; }
  // rows of the asking patches of a token-major tensor (row stride ld, C columns taken) <-> compact [n_ask * p^2, C]
  bool pc_gather_rows(const bf16_t* src, int ld, int C, bf16_t* dst, int level) {
    if (!ok()) return false;
    if (quiet()) return true;
    if (mx::launch_pc_gather(stream, src, ld, C, dst, pc_list(), pc_count(), pc_dsamp, level, pc_p0 >> level, 0, 0, 0)) return fail(mx_last_error());
    return true;
  }
  bool pc_scatter_rows(const bf16_t* src, int C, char* reg, int level) {
    if (!ok()) return false;
    if (quiet()) return true;
    const int p = pc_p0 >> level;
    if (mx::launch_pc_scatter(stream, src, p, 0, C, reg, pc_row_elems(level, C), pc_list(), pc_count(), pc_dsamp, level, p)) return fail(mx_last_error());
    return true;
  }
  // A 3x3 conv whose output every patch caches.  c.corner_patch: that of the whole-image form (all patches ask: the ordinary
  // launch, then a copy into the state).  Partial mask: gather the asking patches with their halos (stride 2: one extra outer ring of zeros, so
  // that the pad-1 stride-2 launch's output o + 1 has the taps of the reference's pad-0 output o), ONE conv over the compact batch, scatter the
  // interiors into the state.  The op's output = state (+ time-embedding row c.rowbias) (+ c.residual) for every patch.
  bool pc_conv(const Conv& c, int level) {
    const bf16_t* x = c.in.t; const std::string& prefix = c.prefix;
    const int Cin = c.Cin, Cout = c.Cout, stride = c.stride, up = c.up;
    const int lo = level + (stride == 2 ? 1 : 0) - up;
    const int p_in = (pc_p0 >> level) << up, p_out = pc_p0 >> lo;
    const int halo_lo = stride == 2 ? 2 : 1, halo_hi = stride == 2 ? 0 : 1;
    const int P = p_in + halo_lo + halo_hi, Po = stride == 2 ? (P + 1) / 2 : P;
    char* reg = pc_region(lo, Cout);
    const size_t mk = ar.mark();
    bf16_t* cin = alloc<bf16_t>((size_t)pc_np * P * P * Cin);
    bf16_t* cout = alloc<bf16_t>((size_t)pc_np * Po * Po * Cout);
    // the compact batch carries the halos ((p + 2)^2 pixels computed per p^2 kept: 1.13x at 32-pixel patches, 1.56x at 8): where it would
    // compute more than 90 % of the whole images' pixels, the whole-image launch runs and only the asking patches are renewed from it
    const bool whole = !pc_partial || (double)pc_nask * Po * Po >= 0.9 * (double)pc_np * p_out * p_out;
    if (whole) {
      Conv w{c.in, c.Hin, c.Win, Cin, prefix, cout, Cout};
      w.stride = stride; w.up = up; w.corner_patch = c.corner_patch;
      conv(w);
      if (!pc_partial) pc_store(cout, reg, lo, Cout);
      else if (ok() && !quiet() && mx::launch_pc_patch_store(stream, cout, reg, pc_row_elems(lo, Cout), Cout, pc_dask, pc_nask, pc_dsamp, lo, p_out)) fail(mx_last_error());
    } else {
      const void* wt = wb(prefix + ".weight", (size_t)Cout * 9 * Cin); const float* bs = wf(prefix + ".bias", Cout);
      if (ok() && !quiet()) {
        if (mx::launch_pc_gather(stream, x, Cin, Cin, cin, pc_dask, pc_nask, pc_dsamp, level, p_in, halo_lo, halo_hi, up)) fail(mx_last_error());
        mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
        d.a = cin; d.w = wt; d.bias = bs; d.c = cout; d.ldc = Cout; d.B = pc_nask; d.Hin = P; d.Win = P; d.Cin = Cin; d.Hout = Po; d.Wout = Po;
        d.stride = stride; d.M = pc_nask * Po * Po; d.N = Cout; d.K = 9 * Cin; d.rows_per_batch = Po * Po; d.ldr = Cout;
        gemm(d, true);
        if (ok() && mx::launch_pc_scatter(stream, cout, Po, 1, Cout, reg, pc_row_elems(lo, Cout), pc_dask, pc_nask, pc_dsamp, lo, p_out)) fail(mx_last_error());
      }
    }
    ar.release(mk);
    return pc_load(c.out, reg, lo, Cout, c.rowbias, c.ldrb, (const bf16_t*)c.residual);
  }
  // attention of the compact query rows of every sample with asking patches against that sample's own keys: problems of one sample each
  bool pc_attention(const bf16_t* qc, const bf16_t* kbase, int ldk, long k_sample_stride, const bf16_t* vtbase, const long* vt_sample_off, const int* ldvt_s,
                    long vt_bstride_fixed, bf16_t* oc, int C, int heads, int level, const int* Lk_s) {
    if (!ok()) return false;
    if (quiet()) return true;
    const int pp = (pc_p0 >> level) * (pc_p0 >> level);
    std::vector<mx_attn_problem> pr;
    for (int b = 0; b < B; ++b) {
      const int na = pc_ask_first[b + 1] - pc_ask_first[b];
      if (!na) continue;
      mx_attn_problem q; std::memset(&q, 0, sizeof(q));
      const long r0 = (long)pc_ask_first[b] * pp;
      q.q = qc + r0 * C; q.o = oc + r0 * C;
      q.k = kbase + (k_sample_stride >= 0 ? (long)b * k_sample_stride : (pc_samp[b].row0 >> (2 * level)) * (long)ldk);
      q.vt = vtbase + vt_sample_off[b]; q.ldvt = ldvt_s[b];
      q.vt_batch_stride = vt_bstride_fixed > 0 ? vt_bstride_fixed : (int64_t)C * ldvt_s[b];
      q.B = 1; q.Lq = na * pp; q.Lk = Lk_s[b];
      pr.push_back(q);
    }
    for (size_t i = 0; i < pr.size(); i += MX_MAX_SEGS) {
      const int n = (int)std::min<size_t>(MX_MAX_SEGS, pr.size() - i);
      if (mx_attention_prescaled_grouped(stream, pr.data() + i, n, C, ldk, C, heads)) return fail(std::string("attention: ") + mx_last_error());
    }
    return true;
  }

  unsigned blocks_run = 0;
  // patch-parallel (mx_unet_forward_pp): this rank owns H (local) of Htot latent rows; distrifuser sync mode (utils.py:119-214)
  int pp_rank = 0, pp_world = 1, Htot = 0;
  bool is_pp() const { return pp_world > 1; }
  // per-forward tensors
  float* temb_all = nullptr; int temb_total = 0; int temb_off = 0;
  struct KV { bf16_t* k; bf16_t* vt; int ldk; int ldvt; long vt_bstride; int next; int dim; };
  std::vector<KV> kv;       // one per distinct attention width
  mx_unet::CtxEntry* ctx_e = nullptr;   // the composition's stored K / V^T (forward_impl: ctx_prepare); ctx_hit: already computed
  bool ctx_hit = false;

  // ---- patch-parallel helpers --------------------------------------------------------------
  bool all_gather(const void* send, void* recv, size_t bytes_per_rank, bool keep_stale_own = false) {
    if (!ok()) return false;
    if (const char* e = px.all_gather(stream, dry, send, recv, bytes_per_rank, keep_stale_own)) return fail(e);
    return true;
  }
  // [B, h + 2, wd, C] image with one halo row above and below; returns the base (the top halo row of image 0)
  bf16_t* alloc_padded(int h, int wd, int C) { return alloc<bf16_t>((size_t)B * (h + 2) * wd * C); }
  static bf16_t* interior(bf16_t* P, int wd, int C) { return P + (size_t)wd * C; }
  bool copy_to_padded(const bf16_t* x, bf16_t* P, int h, int wd, int C) {
    if (!ok()) return false;
    if (dry) return true;
    const size_t img = (size_t)h * wd * C * 2, pimg = (size_t)(h + 2) * wd * C * 2;
    if (hipMemcpy2DAsync(interior(P, wd, C), pimg, x, img, img, B, hipMemcpyDeviceToDevice, stream) != hipSuccess) return fail("copy_to_padded failed");
    return true;
  }
  // fill the halo rows of P from the neighbour ranks' boundary rows (zeros at the true image border): one all-gather of
  // [2][B][wd * C] per rank (distrifuser modules/pp/conv2d.py:98 gathers [2, b, C, pad, W] the same way)
  bool halo_exchange(bf16_t* P, int h, int wd, int C) {
    if (!ok()) return false;
    const size_t m = ar.mark();
    const size_t row = (size_t)wd * C * 2, pimg = (size_t)(h + 2) * row;
    char* send = (char*)ar.alloc(2 * B * row);
    char* recv = (char*)ar.alloc((size_t)pp_world * 2 * B * row);
    if (!send || !recv) return fail("workspace too small");
    if (dry) { if (!all_gather(send, recv, 2 * B * row)) return false; }
    if (!dry) {
      char* Pc = (char*)P;
      bool e = hipMemcpy2DAsync(send, row, Pc + row, pimg, row, B, hipMemcpyDeviceToDevice, stream) != hipSuccess;
      e |= hipMemcpy2DAsync(send + B * row, row, Pc + (size_t)h * row, pimg, row, B, hipMemcpyDeviceToDevice, stream) != hipSuccess;
      if (e) return fail("halo pack failed");
      if (!all_gather(send, recv, 2 * B * row)) return false;
      if (pp_rank > 0) e |= hipMemcpy2DAsync(Pc, pimg, recv + ((size_t)(pp_rank - 1) * 2 + 1) * B * row, row, row, B, hipMemcpyDeviceToDevice, stream) != hipSuccess;
      else e |= hipMemset2DAsync(Pc, pimg, 0, row, B, stream) != hipSuccess;
      if (pp_rank < pp_world - 1) e |= hipMemcpy2DAsync(Pc + (size_t)(h + 1) * row, pimg, recv + ((size_t)(pp_rank + 1) * 2) * B * row, row, row, B, hipMemcpyDeviceToDevice, stream) != hipSuccess;
      else e |= hipMemset2DAsync(Pc + (size_t)(h + 1) * row, pimg, 0, row, B, stream) != hipSuccess;
      if (e) return fail("halo unpack failed");
    }
    ar.release(m);
    return true;
  }
  // GroupNorm over the whole image from the ranks' partial sums; y may be the interior of a padded image (y_img elements per image)
  bool groupnorm_pp(const bf16_t* x, bf16_t* y, long y_img, const std::string& prefix, int h, int wd, int C, float eps, bool silu, int level,
                    const bf16_t* x2 = nullptr, int C1 = 0) {
    if (!ok()) return false;
    const size_t m = ar.mark();
    const int G = u->cfg.norm_num_groups;
    void* ws = ar.alloc(mx::gn_workspace_exact(B, h, wd, C, 0));
    double* sums = (double*)ar.alloc((size_t)B * G * 2 * sizeof(double));
    double* all = (double*)ar.alloc((size_t)pp_world * B * G * 2 * sizeof(double));
    if (!ws || !sums || !all) return fail("workspace too small");
    const float* g = wf(prefix + ".weight", C); const float* b = wf(prefix + ".bias", C);
    if (ok() && dry) all_gather(sums, all, (size_t)B * G * 2 * sizeof(double));
    if (ok() && !dry) {
      if (mx::launch_gn_pp_partial(stream, x, C1, x2, B, h, wd, C, G, ws, sums)) return fail(std::string("groupnorm: ") + mx_last_error());
      // stale steps: "stale_gn" = fresh own sums beside the others' stale ones; "corrected_async_gn" (distrifuser's default,
      // modules/pp/groupnorm.py:52-66) = the stale whole-image moments plus this rank's (fresh - stale) change, local variance if negative
      const bool corrected = px.mode == MX_PP_STALE && px.corrected_gn;
      if (!all_gather(sums, all, (size_t)B * G * 2 * sizeof(double), corrected)) return false;
      if (mx::launch_gn_pp_finish(stream, x, C1, x2, y, y_img, g, b, all, pp_world, B, h, wd, C, G, Htot >> level, eps, silu ? 1 : 0, ws,
                                  corrected ? sums : nullptr, pp_rank))
        return fail(std::string("groupnorm: ") + mx_last_error());
    }
    ar.release(m);
    return ok();
  }

  // ---- op wrappers -------------------------------------------------------------------------
  unsigned* ln_cnt = nullptr;     // panel tickets of the finalising producers: zeroed once per run, every launch leaves them zero
  static constexpr int kLnCnt = 4096;
  // launch d; the statistics of its output rows go to st (from the epilogue when the chosen kernel can, else a pass over the output)
  // via: the form their consumer reads, Slabs or Final (the producer side of a route)
  bool gemm_with_stats(mx_gemm_desc& d, RowStats& st, LnVia via) {
    if (!ok()) return false;
    const int slabs = mx_gemm_stats_slabs(&d);
    if (via == LnVia::Final) {
      if (slabs <= 0 || !mx_gemm_ln_final_supported(&d) || (d.M + 255) / 256 > kLnCnt) return fail("finalised row statistics: the producing launch cannot write them");
      d.ln_final_out = st.fin; d.ln_final_cnt = st.cnt; d.ln_eps = u->cfg.layer_norm_eps;
    }
    if (slabs > 0) { d.stats_out = st.buf; st.slabs = slabs; return gemm(d, false); }
    st.slabs = 1;
    if (!gemm(d, false)) return false;
    if (!quiet() && mx_row_stats(stream, d.c, d.ldc, st.buf, d.M, d.N)) return fail(std::string("row_stats: ") + mx_last_error());
    return true;
  }
  // the consumer side of a route: d reads the folded LayerNorm's statistics st by route via.  segs / row0: the problems of a grouped d and their first
  // rows -- every problem reads its own rows of the one slab buffer (ln_final excludes grouped launches: ln_route.h never finalises them)
  void use_ln(mx_gemm_desc& d, const RowStats& st, const std::string& csname, LnVia via, mx_gemm_seg* segs = nullptr, const long* row0 = nullptr) {
    const float* colsum = wf(csname, d.N);
    switch (via) {
      case LnVia::Pass: return;           // (the weight is resolved all the same, so that a validation walk asks for it at every shape)
      case LnVia::Final: d.ln_final = st.fin; break;
      case LnVia::Slabs:
        d.ln_stats = st.buf; d.ln_slabs = st.slabs;
        for (int g = 0; g < d.n_segs; ++g) segs[g].ln_stats = st.buf + row0[g] * MX_STATS_PITCH(st.slabs) * 2;
        break;
    }
    d.ln_colsum = colsum; d.ln_eps = u->cfg.layer_norm_eps;
  }
  bool linear(const Linear& l) {
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.out_scale = l.out_scale;
    if (l.a2) { d.a2 = l.a2; d.lda2 = l.lda2; d.k_split = l.lda; }      // A = [a | a2] along K, read in place
    d.a = l.a; d.lda = l.lda; d.w = wb(l.stem + ".weight", (size_t)l.N * l.K); d.bias = wf(l.stem + ".bias", l.N);
    d.c = l.c; d.ldc = l.ldc; d.M = l.M; d.N = l.N; d.K = l.K; d.residual = l.residual; d.ldr = l.ldr; d.flags = l.flags;
    if (l.ln_via != LnVia::Pass) use_ln(d, *l.ln, l.stem + ".colsum", l.ln_via);
    if (l.stats_via != LnVia::Pass) return gemm_with_stats(d, *l.stats_out, l.stats_via);
    return gemm(d, false);
  }
  // 3x3 conv over the images of every group at the current level (Hin, Win: the first group's size; the others come from ch / cw).  A mixed
  // batch is ONE grouped launch: problem g = group g's images, its output grid, its samples' rows of the time-embedding row bias.
  int conv_cin_valid = 0;   // set around conv_in's launch
  bool conv(const Conv& c) {
    const bf16_t* x = c.in.padded ? c.in.padded : c.in.t;
    const int Cin = c.Cin, Cout = c.Cout, stride = c.stride, up = c.up;
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.vhalo = c.in.padded ? 1 : 0;            // (the rows above and below the image are in memory)
    const int Hv = c.Hin << up, Wv = c.Win << up;
    d.a = x; d.w = wb(c.prefix + ".weight", (size_t)Cout * 9 * Cin); d.bias = wf(c.prefix + ".bias", Cout);
    d.c = c.out; d.ldc = Cout; d.B = gB[0]; d.Hin = c.Hin; d.Win = c.Win; d.Cin = Cin;
    d.Hout = (Hv + stride - 1) / stride; d.Wout = (Wv + stride - 1) / stride; d.stride = stride; d.up = up;
    d.corner_patch = c.corner_patch;
    d.M = gB[0] * d.Hout * d.Wout; d.N = Cout; d.K = 9 * Cin;
    d.rowbias = c.rowbias; d.ldrb = c.ldrb; d.rows_per_batch = d.Hout * d.Wout;
    d.residual = c.residual; d.ldr = Cout;
    mx_gemm_seg sg[MX_MAX_SEGS];
    if (ng > 1) {
      std::memset(sg, 0, sizeof(sg));
      long in0 = 0, out0 = 0;
      for (int g = 0; g < ng; ++g) {
        mx_gemm_seg& q = sg[g];
        q.B = gB[g]; q.Hin = ch[g]; q.Win = cw[g];
        q.Hout = ((ch[g] << up) + stride - 1) / stride; q.Wout = ((cw[g] << up) + stride - 1) / stride;
        q.M = gB[g] * q.Hout * q.Wout; q.rows_per_batch = q.Hout * q.Wout;
        q.a = x + in0 * Cin; q.c = c.out + out0 * Cout;
        q.residual = c.residual ? (const bf16_t*)c.residual + out0 * Cout : nullptr;
        q.rowbias = c.rowbias ? c.rowbias + (long)gb0[g] * c.ldrb : nullptr;
        in0 += (long)gB[g] * ch[g] * cw[g]; out0 += q.M;
      }
      d.segs = sg; d.n_segs = ng;
    }
    if (c.gn_part && c.gn_done && ng == 1 && mx_gemm_gn_partials_supported(&d, 1)) { d.gn_part_out = c.gn_part; *c.gn_done = true; }
    d.cin_valid = conv_cin_valid;             // (conv_in only: the latent's channels inside its zero-padded rows)
    // whole image rows per tile, the input staged once per channel chunk (conv_halo.hip) -- where the launch would otherwise run the same 256-row tile:
    // a small launch stays on the 128-row tiles and their split-K, which fill more CUs
    if (mx_conv3x3_halo_serves(&d) && mx_gemm_form(&d, 1) == MX_FORM_TILE_256) {
      if (!ok()) return false;
      if (quiet()) return true;
      if (mx_conv3x3_halo(stream, &d)) return fail(std::string("conv3x3_halo: ") + mx_last_error());
      return true;
    }
    // 128-wide images: the same kernel on half-row tiles (4 rows x 64 columns and the neighbouring column)
    if (mx_conv3x3_halfrow_serves(&d) && mx_gemm_form(&d, 1) == MX_FORM_TILE_256) {
      if (!ok()) return false;
      if (quiet()) return true;
      if (mx_conv3x3_halfrow(stream, &d)) return fail(std::string("conv3x3_halfrow: ") + mx_last_error());
      return true;
    }
    return gemm(d, true);
  }
  bool groupnorm(const bf16_t* x, bf16_t* y, const std::string& prefix, int h, int wd, int C, float eps, bool silu, int patch,
                 const bf16_t* x2 = nullptr, int C1 = 0) {
    if (!ok()) return false;
    const size_t m = ar.mark();
    mx_gn_problem pr[MX_MAX_SEGS];
    long r0 = 0;
    for (int k = 0; k < ng; ++k) {         // group k's images inside the concatenated activations
      pr[k].x = x + r0 * (x2 ? C1 : C); pr[k].x2 = x2 ? x2 + r0 * (C - C1) : nullptr; pr[k].y = y + r0 * C;
      pr[k].B = gB[k]; pr[k].H = ch[k]; pr[k].W = cw[k];
      r0 += (long)gB[k] * ch[k] * cw[k];
    }
    const size_t need = ng > 1 ? mx_groupnorm_nhwc_grouped_workspace_bytes(pr, ng, C) : mx::gn_workspace_exact(gB[0], h, wd, C, patch);
    void* ws = ar.alloc(need);
    if (!ws) return fail("workspace too small");
    const float* g = wf(prefix + ".weight", C); const float* b = wf(prefix + ".bias", C);
    if (ok() && !quiet()) {
      if (mx_groupnorm_nhwc_grouped(stream, pr, ng, x2 ? C1 : C, g, b, C, u->cfg.norm_num_groups, eps, silu ? 1 : 0, patch, ws))
        fail(std::string("groupnorm: ") + mx_last_error());
    }
    ar.release(m);
    return ok();
  }
  // GroupNorm whose statistics the producing launch left as partial sums per 64 rows (conv(): gn_part); one resolution group, exact statistics
  bool groupnorm_from_partials(const bf16_t* x, bf16_t* y, const std::string& prefix, int h, int wd, int C, float eps, bool silu, const float* part,
                               const float* add_bias, const float* add_rowbias, int ldrb) {
    if (!ok()) return false;
    const size_t m = ar.mark();
    void* ws = ar.alloc(mx::gn_workspace_exact(gB[0], h, wd, C, 0));
    if (!ws) return fail("workspace too small");
    const float* g = wf(prefix + ".weight", C); const float* b = wf(prefix + ".bias", C);
    if (ok() && !quiet()) {
      if (mx_groupnorm_nhwc_from_partials(stream, x, y, g, b, gB[0], h, wd, C, u->cfg.norm_num_groups, eps, silu ? 1 : 0, part, 64, add_bias, add_rowbias, ldrb, ws))
        fail(std::string("groupnorm: ") + mx_last_error());
    }
    ar.release(m);
    return ok();
  }
  bool attention(const bf16_t* q, int ldq, const bf16_t* k, int ldk, const bf16_t* vt, int ldvt, long vt_bstride, bf16_t* o,
                 int ldo, int heads, int Lq, int Lk) {
    if (!ok()) return false;
    if (quiet()) return true;
    // q carries MX_ATTN_QSCALE(1/8) from the producing GEMM's epilogue (out_scale)
    if (mx_attention_prescaled(stream, q, ldq, k, ldk, vt, ldvt, vt_bstride, o, ldo, B, heads, Lq, Lk))
      return fail(std::string("attention: ") + mx_last_error());
    return true;
  }
  // one launch over the groups' attention problems (mixed batch)
  bool attention_grouped(const mx_attn_problem* pr, int ldq, int ldk, int ldo, int heads) {
    if (!ok()) return false;
    if (quiet()) return true;
    if (mx_attention_prescaled_grouped(stream, pr, ng, ldq, ldk, ldo, heads)) return fail(std::string("attention: ") + mx_last_error());
    return true;
  }
  int level_patch(int level) const { return gn_patch > 0 ? std::max(gn_patch >> level, 1) : 0; }

  // ---- a 3x3 conv in the plan's mode: these four hide it from the blocks ------------------------
  // row-split image (patch-parallel): GroupNorm from gathered sums, convs on halo'd inputs (modules/pp/{groupnorm,conv2d}.py);
  // patch-unit cache: the conv per patch from the op's state, its GroupNorm on all rows (resnet.py:390-460 with a mask)
  ConvIn alloc_conv_in(int h, int wd, int C) {
    if (!is_pp()) return {alloc<bf16_t>((size_t)rows() * C), nullptr};
    bf16_t* P = alloc_padded(h, wd, C);
    return {interior(P, wd, C), P};
  }
  // n = silu(GroupNorm(x)) at the block's eps, halo rows included
  bool norm_into(const ConvIn& n, const bf16_t* x, const std::string& prefix, int h, int wd, int C, int level, const bf16_t* x2 = nullptr, int C1 = 0) {
    if (!is_pp()) return groupnorm(x, n.t, prefix, h, wd, C, u->cfg.norm_eps, true, level_patch(level), x2, C1);
    groupnorm_pp(x, n.t, (long)(h + 2) * wd * C, prefix, h, wd, C, u->cfg.norm_eps, true, level, x2, C1);
    return halo_exchange(n.padded, h, wd, C);
  }
  // level: that of the conv's input; the corner rule of the sliced form is that of the output grid's patch
  bool block_conv(Conv c, int level) {
    if (is_pp()) return conv(c);             // (exact arithmetic: no corner rule)
    c.corner_patch = level_patch(level - c.up);
    return pc ? pc_conv(c, level) : conv(c);
  }
  // the same for a tensor that no GroupNorm of the plan wrote (down / upsampler): patch-parallel pads a copy first, for the length of the conv
  bool block_conv_of(bf16_t* x, Conv c, int level) {
    const size_t mk = ar.mark();
    c.in = {x, nullptr};
    if (is_pp()) {
      if (c.stride == 2 && c.Hin % 2) fail("patch-parallel: local rows must stay even down to the last level");
      c.in = alloc_conv_in(c.Hin, c.Win, c.Cin);
      copy_to_padded(x, c.in.padded, c.Hin, c.Win, c.Cin);
      halo_exchange(c.in.padded, c.Hin, c.Win, c.Cin);
    }
    block_conv(c, level);
    ar.release(mk);
    return ok();
  }

  // ---- blocks ------------------------------------------------------------------------------
  // modules/resnet.py:390-460
  // x2 != nullptr: the block's input is the channel concatenation [x (Cin - C2 channels) | x2 (C2 channels)] of an up block
  // (unet.py:458-462 torch.cat), read in place by norm1 and by the 1x1 shortcut
  bf16_t* resnet(const std::string& p, const bf16_t* x, int h, int wd, int Cin, int Cout, int level, const bf16_t* x2 = nullptr, int C2 = 0) {
    const int M = (int)rows();            // the pixels of every group at this level (h, wd: the first group's image)
    const int C1 = Cin - C2;
    bf16_t* out = alloc<bf16_t>((size_t)M * Cout);
    const size_t m = ar.mark();
    ConvIn n1 = alloc_conv_in(h, wd, Cin);
    norm_into(n1, x, p + ".norm1", h, wd, Cin, level, x2, C1);
    bf16_t* h1 = alloc<bf16_t>((size_t)M * Cout);
    // norm2's statistics come from conv1's own launch where it can leave them (round 4: one resolution, exact statistics, a 256-row tile): per 64
    // output rows and channel the sums of conv + bias + time embedding, so the statistics pass over h1 does not run (resnet.py:414-429).  The
    // plain path only: patch-parallel statistics are gathered over the ranks, the patch-unit cache's h1 comes out of the state merge
    float* gpart = nullptr;
    bool gdone = false;
    if (!is_pp() && !pc && ng == 1 && level_patch(level) == 0 && M % 64 == 0 && (h * wd) % 64 == 0) gpart = (float*)ar.alloc((size_t)(M / 64) * Cout * 2 * sizeof(float));
    const float* temb = temb_all ? temb_all + temb_off : nullptr;       // this block's columns of the one time_emb_proj GEMM
    temb_off += Cout;
    block_conv(Conv{n1, h, wd, Cin, p + ".conv1", h1, Cout}.row_bias(temb, temb_total).gn_partials(gpart, &gdone), level);
    ConvIn n2 = alloc_conv_in(h, wd, Cout);
    if (gdone) groupnorm_from_partials(h1, n2.t, p + ".norm2", h, wd, Cout, u->cfg.norm_eps, true, gpart, wf(p + ".conv1.bias", Cout), temb, temb_total);
    else norm_into(n2, h1, p + ".norm2", h, wd, Cout, level);
    const bf16_t* sc = x;
    if (Cin != Cout) {                    // the 1x1 shortcut, over [x | x2] in place
      bf16_t* s2 = alloc<bf16_t>((size_t)M * Cout);
      linear(Linear{x, C1, p + ".conv_shortcut", s2, Cout, M, Cout, Cin}.concat(x2, C2));
      sc = s2;
    }
    block_conv(Conv{n2, h, wd, Cout, p + ".conv2", out, Cout}.plus(sc), level);
    ar.release(m);
    dump(p, out, (size_t)M * Cout);
    return out;
  }

  KV* kv_for(int dim) {
    for (auto& k : kv) if (k.dim == dim) return &k;
    return nullptr;
  }

  // ---- Transformer2DModel (modules/transformer.py:32-128) over BasicTransformerBlocks (:167-290) ----
  // per resolution group of the rows (one unless the batch is mixed): tokens per image, first row, its V^T block (rows of MX_VT_LD(tokens) keys)
  struct TokenGroups { int L[MX_MAX_SEGS], ldvt[MX_MAX_SEGS]; long row0[MX_MAX_SEGS], vt0[MX_MAX_SEGS], vt_elems = 0; };
  // one transformer's shape, LayerNorm routes and buffers (transformer_buffers allocates them in the order they stand here)
  struct Xf {
    int C, heads, level, M, L, ldvt;      // (L, ldvt: the first group's tokens per image)
    TokenGroups g;
    // The block's three LayerNorms are folded into the linears they feed (weights.py fold_layernorm); via says by which route each reaches its consumer
    // (ln_route.h: the table).  The producer of a norm's hidden state and its consumer are handed the same member: norm1 proj_in and the previous layer's
    // ff.net.2 -> q|k|v; norm2 attn1.to_out or the patch cache's merge -> attn2.to_q; norm3 attn2.to_out or the merge -> the GEGLU projection.
    mx::LnRoutes via;
    bf16_t* y = nullptr;                  // the hidden state
    RowStats st;                          // its row statistics: slabs (Slabs) and, where a norm takes Final, (mean, rstd)
    bf16_t* ln = nullptr;                 // its normalised copy (Pass): the GroupNorm output, dead after proj_in
    bf16_t *qk = nullptr, *vt = nullptr, *ao = nullptr, *q2 = nullptr, *ff = nullptr;
    bf16_t *pqc = nullptr, *paoc = nullptr, *ptc = nullptr;          // patch-unit cache: compact queries / attention output / projection output
    bf16_t *k_send = nullptr, *k_all = nullptr, *vt_all = nullptr;   // patch-parallel: the ranks' K rows and V^T columns
    KV* kvp = nullptr;                    // the hoisted cross-attention K / V^T of this width
    mx_gemm_seg qsegs[MX_MAX_SEGS];       // mixed batch: the fused q|k|v projection as a grouped launch (tokens per image and V^T block per group)
    std::vector<long> vt_off; std::vector<int> ldvt_s, Lk_s;         // patch-unit cache: per sample, its V^T block and keys
  };
  void transformer_buffers(Xf& t, bf16_t* gn_out) {
    const size_t M = t.M, C = t.C;
    t.y = alloc<bf16_t>(M * C);
    t.st.buf = (float*)ar.alloc(M * MX_STATS_PITCH(C / 64) * 2 * sizeof(float));
    if (!t.st.buf) fail("workspace too small");
    t.ln = gn_out;
    t.qk = alloc<bf16_t>(M * 2 * C);
    t.vt = alloc<bf16_t>((size_t)t.g.vt_elems);
    t.ao = alloc<bf16_t>(M * C);
    t.q2 = alloc<bf16_t>(M * C);
    t.ff = alloc<bf16_t>(M * 4 * C);
    if (t.via.norm1 == LnVia::Final || t.via.norm3 == LnVia::Final) { t.st.fin = (float*)ar.alloc(M * 2 * sizeof(float)); t.st.cnt = ln_cnt; if (!t.st.fin) fail("workspace too small"); }
    if (pc) { t.pqc = alloc<bf16_t>(M * C); t.paoc = alloc<bf16_t>(M * C); t.ptc = alloc<bf16_t>(M * C); }
  }
  // out = (in - mean) * rstd per row, no affine (it lives in the folded weights)
  void normalise(const bf16_t* in, bf16_t* out, int rows, int C) {
    if (ok() && !quiet() && mx_layernorm(stream, in, out, nullptr, nullptr, rows, C, u->cfg.layer_norm_eps)) fail(std::string("layernorm: ") + mx_last_error());
  }
  // the A operand of a norm's consumer on route via: Pass runs the pass and gives the normalised copy, the others read the hidden state itself
  const bf16_t* ln_operand(Xf& t, LnVia via) {
    if (via != LnVia::Pass) return t.y;
    normalise(t.y, t.ln, t.M, t.C);
    return t.ln;
  }
  // self-attention's fused q | k | v projection of block b, norm1 folded into it (the hidden state in front of it comes from ordinary GEMMs in every mode)
  void qkv(Xf& t, const std::string& b) {
    const int C = t.C;
    const bf16_t* a = ln_operand(t, t.via.norm1);
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.a = a; d.w = wb(b + ".attn1.to_qkv.weight", (size_t)3 * C * C); d.bias = wf(b + ".attn1.to_qkv.bias", 3 * C);
    d.c = t.qk; d.vt = t.vt;
    mx::ln_qkv_shape(d, t.M, C, t.L);
    if (ng > 1) {
      std::memset(t.qsegs, 0, sizeof(t.qsegs));
      for (int g = 0; g < ng; ++g) {
        t.qsegs[g].a = a + t.g.row0[g] * C; t.qsegs[g].c = t.qk + t.g.row0[g] * 2 * C; t.qsegs[g].vt = t.vt + t.g.vt0[g];
        t.qsegs[g].M = gB[g] * t.g.L[g]; t.qsegs[g].rows_per_batch = t.g.L[g]; t.qsegs[g].ldvt = t.g.ldvt[g];
      }
      d.segs = t.qsegs; d.n_segs = ng;
    }
    use_ln(d, t.st, b + ".attn1.to_qkv.colsum", t.via.norm1, t.qsegs, t.g.row0);
    gemm(d, false);
  }
  // ---- the two attention launches over all rows: one grouped launch over the groups' problems in a mixed batch ----
  void self_problems(const Xf& t, mx_attn_problem* pr) {
    const int C = t.C;
    for (int g = 0; g < ng; ++g) {
      pr[g].q = t.qk + t.g.row0[g] * 2 * C; pr[g].k = t.qk + t.g.row0[g] * 2 * C + C; pr[g].vt = t.vt + t.g.vt0[g]; pr[g].o = t.ao + t.g.row0[g] * C;
      pr[g].vt_batch_stride = (int64_t)C * t.g.ldvt[g]; pr[g].B = gB[g]; pr[g].Lq = t.g.L[g]; pr[g].Lk = t.g.L[g]; pr[g].ldvt = t.g.ldvt[g];
    }
  }
  void cross_problems(const Xf& t, mx_attn_problem* pr, int li) {      // the hoisted K / V^T are per sample: group g reads the rows of its samples
    const int C = t.C; const KV* kvp = t.kvp;
    for (int g = 0; g < ng; ++g) {
      pr[g].q = t.q2 + t.g.row0[g] * C; pr[g].k = kvp->k + (size_t)li * C + (size_t)gb0[g] * ctx_len * kvp->ldk;
      pr[g].vt = kvp->vt + (size_t)li * C * kvp->ldvt + (size_t)gb0[g] * kvp->vt_bstride; pr[g].o = t.ao + t.g.row0[g] * C;
      pr[g].vt_batch_stride = kvp->vt_bstride; pr[g].B = gB[g]; pr[g].Lq = t.g.L[g]; pr[g].Lk = ctx_len; pr[g].ldvt = kvp->ldvt;
    }
  }
  void self_attention(Xf& t) {                  // ao = attention(q, k, v of qk | vt)
    const int C = t.C;
    mx_attn_problem pr[MX_MAX_SEGS];
    if (ng > 1) { self_problems(t, pr); attention_grouped(pr, 2 * C, 2 * C, C, t.heads); }
    else attention(t.qk, 2 * C, t.qk + C, 2 * C, t.vt, t.ldvt, (long)C * t.ldvt, t.ao, C, t.heads, t.L, t.L);
  }
  void cross_attention(Xf& t, int li) {         // ao = attention(q2, layer li of the hoisted K / V^T)
    if (!ok()) return;
    const int C = t.C; const KV* kvp = t.kvp;
    mx_attn_problem pr[MX_MAX_SEGS];
    if (ng > 1) { cross_problems(t, pr, li); attention_grouped(pr, C, kvp->ldk, C, t.heads); }
    else attention(t.q2, C, kvp->k + (size_t)li * C, kvp->ldk, kvp->vt + (size_t)li * C * kvp->ldvt, kvp->ldvt, kvp->vt_bstride, t.ao, C, t.heads, t.L, ctx_len);
  }
  // ---- between the q | k | v projection and the feed-forward: y += attn1, y += attn2, leaving norm3's input form ----
  // self-attention -> to_out -> residual, then the cross-attention on layer li of the K / V^T of encoder_hidden_states (norm2 in to_q)
  void attend(Xf& t, const std::string& b, int li) {
    const int C = t.C, M = t.M;
    if (is_pp()) {      // every rank gathers the other ranks' K rows and V^T columns (modules/pp/attn.py:137: all_gather(kv))
      if (ok() && !dry && hipMemcpy2DAsync(t.k_send, (size_t)C * 2, t.qk + C, (size_t)2 * C * 2, (size_t)C * 2, M, hipMemcpyDeviceToDevice, stream) != hipSuccess)
        fail("patch-parallel: K pack failed");
      all_gather(t.k_send, t.k_all, (size_t)M * C * 2);
      all_gather(t.vt, t.vt_all, (size_t)B * C * t.ldvt * 2);
      if (ok() && !dry &&
          mx_attention_prescaled_chunked(stream, t.qk, 2 * C, t.k_all, C, t.vt_all, t.ldvt, (int64_t)C * t.ldvt, t.ao, C, B, t.heads, t.L, pp_world * t.L, t.L,
                                         (int64_t)t.L * C, (int64_t)M * C, (int64_t)B * C * t.ldvt))
        fail(std::string("attention: ") + mx_last_error());
    } else self_attention(t);
    linear(Linear{t.ao, C, b + ".attn1.to_out.0", t.y, C, M, C, C}.plus(t.y, C).leaves_stats(t.st, t.via.norm2));
    linear(Linear{ln_operand(t, t.via.norm2), C, b + ".attn2.to_q", t.q2, C, M, C, C}.scaled(MX_ATTN_QSCALE(0.125f)).folded_ln(t.st, t.via.norm2));
    cross_attention(t, li);
    linear(Linear{t.ao, C, b + ".attn2.to_out.0", t.y, C, M, C, C}.plus(t.y, C).leaves_stats(t.st, t.via.norm3));
  }
  // patch-unit cache: y += an op's (fresh or cached) output out of its state; the merge kernel is the producer of the norm behind it and leaves the
  // statistics in the form route via reads (round 5, pc_load_stats: one slab for the 256 / 128-row GEMMs, (mean, rstd) for the 256 x 256 kernel)
  void pc_merge(Xf& t, char* reg, LnVia via) {
    switch (via) {
      case LnVia::Pass: pc_load(t.y, reg, t.level, t.C, nullptr, 0, t.y); break;
      case LnVia::Slabs: pc_load_stats(t.y, reg, t.level, t.C, t.y, t.st.buf, nullptr); t.st.slabs = 1; break;
      case LnVia::Final: pc_load_stats(t.y, reg, t.level, t.C, t.y, nullptr, t.st.fin); break;
    }
  }
  // PatchBasicTransformerBlock under a per-patch mask (transformer.py:167-290): the LayerNorms, the q | k | v projection of attn1 and the
  // feed-forward run on all rows; the self-attention core + to_out and the whole cross-attention run for the asking patches and the
  // others take the op's cached output (attention.py:59-110, 121-232); then the residual adds
  void attend_masked(Xf& t, const std::string& b, int li) {
    const int C = t.C, M = t.M, level = t.level;
    const KV* kvp = t.kvp;
    const int pp2 = (pc_p0 >> level) * (pc_p0 >> level);
    const int Mc = pc_count() * pp2;
    char* reg1 = pc_region(level, C);
    if (!pc_partial) {
      self_attention(t);
      linear(Linear{t.ao, C, b + ".attn1.to_out.0", t.ptc, C, M, C, C});
      pc_store(t.ptc, reg1, level, C);
    } else {
      pc_gather_rows(t.qk, 2 * C, C, t.pqc, level);
      pc_attention(t.pqc, t.qk + C, 2 * C, -1, t.vt, t.vt_off.data(), t.ldvt_s.data(), 0, t.paoc, C, t.heads, level, t.Lk_s.data());
      linear(Linear{t.paoc, C, b + ".attn1.to_out.0", t.ptc, C, Mc, C, C});
      pc_scatter_rows(t.ptc, C, reg1, level);
    }
    // The one RUN-TIME fact outside the route table: under a partial mask (pc_partial, known per block at run time) to_q runs on the asking rows only, so
    // norm2 is a pass over those rows alone, whatever the table says (the pass over all M rows in front of the gather cost as much as attn2 saved)
    const LnVia norm2 = pc_partial ? LnVia::Pass : t.via.norm2;
    pc_merge(t, reg1, norm2);
    char* reg2 = pc_region(level, C);
    if (!pc_partial) {
      linear(Linear{ln_operand(t, norm2), C, b + ".attn2.to_q", t.q2, C, M, C, C}.scaled(MX_ATTN_QSCALE(0.125f)).folded_ln(t.st, norm2));
      cross_attention(t, li);
      linear(Linear{t.ao, C, b + ".attn2.to_out.0", t.ptc, C, M, C, C});
      pc_store(t.ptc, reg2, level, C);
    } else {
      pc_gather_rows(t.y, C, C, t.paoc, level);
      normalise(t.paoc, t.pqc, Mc, C);
      linear(Linear{t.pqc, C, b + ".attn2.to_q", t.q2, C, Mc, C, C}.scaled(MX_ATTN_QSCALE(0.125f)));
      if (ok()) {
        std::vector<long> cvt_off(B); std::vector<int> cld(B, kvp->ldvt), clk(B, ctx_len);
        for (int bb = 0; bb < B; ++bb) cvt_off[bb] = (long)bb * kvp->vt_bstride;
        pc_attention(t.q2, kvp->k + (size_t)li * C, kvp->ldk, (long)ctx_len * kvp->ldk, kvp->vt + (size_t)li * C * kvp->ldvt, cvt_off.data(), cld.data(),
                     kvp->vt_bstride, t.paoc, C, t.heads, level, clk.data());
      }
      linear(Linear{t.paoc, C, b + ".attn2.to_out.0", t.ptc, C, Mc, C, C});
      pc_scatter_rows(t.ptc, C, reg2, level);
    }
    pc_merge(t, reg2, t.via.norm3);
  }
  // GEGLU feed-forward of block b (norm3 in the GEGLU projection); next: the route of the norm that reads what ff.net.2 leaves (the next layer's norm1)
  void feed_forward(Xf& t, const std::string& b, LnVia next) {
    const int C = t.C, M = t.M;
    linear(Linear{ln_operand(t, t.via.norm3), C, b + ".ff.net.0.proj", t.ff, 4 * C, M, 8 * C, C}.epilogue(MX_EPI_GEGLU).folded_ln(t.st, t.via.norm3));
    linear(Linear{t.ff, 4 * C, b + ".ff.net.2", t.y, C, M, C, 4 * C}.plus(t.y, C).leaves_stats(t.st, next));
  }
  bf16_t* transformer(const std::string& p, const bf16_t* x, int h, int wd, int C, int heads, int layers, int level) {
    Xf t;
    t.C = C; t.heads = heads; t.level = level; t.M = (int)rows();
    t.L = h * wd;                         // tokens per image of the first group (the only one unless the batch is mixed)
    t.ldvt = MX_VT_LD(t.L);
    const int M = t.M, L = t.L;
    mx::LnRows lr; lr.n_groups = ng;
    for (int g = 0; g < ng; ++g) {
      t.g.L[g] = ch[g] * cw[g]; t.g.ldvt[g] = MX_VT_LD(t.g.L[g]); t.g.row0[g] = row0(g); t.g.vt0[g] = t.g.vt_elems;
      t.g.vt_elems += (long)gB[g] * C * t.g.ldvt[g];
      lr.rows[g] = gB[g] * t.g.L[g]; lr.per_image[g] = t.g.L[g];
    }
    bf16_t* out = alloc<bf16_t>((size_t)M * C);
    const size_t m0 = ar.mark();
    bf16_t* n = alloc<bf16_t>((size_t)M * C);
    if (is_pp()) groupnorm_pp(x, n, (long)L * C, p + ".norm", h, wd, C, u->cfg.transformer_norm_eps, false, level);
    else groupnorm(x, n, p + ".norm", h, wd, C, u->cfg.transformer_norm_eps, false, level_patch(level));
    // (tickets: the plan has its panel counters and they cover these rows)
    t.via = mx::ln_routes(lr, C, layers, is_pp(), pc, ln_cnt != nullptr && (M + 255) / 256 <= kLnCnt);
    transformer_buffers(t, n);
    linear(Linear{n, C, p + ".proj_in", t.y, C, M, C, C}.leaves_stats(t.st, t.via.norm1));
    // -- K alone travels: the QKV epilogue writes q|k interleaved, so the K halves are packed into a contiguous send buffer first
    if (is_pp()) {
      if (L % 64 != 0) fail("patch-parallel: local tokens per image must be a multiple of 64 at every attention level");
      t.k_send = alloc<bf16_t>((size_t)M * C);
      t.k_all = alloc<bf16_t>((size_t)pp_world * M * C);
      t.vt_all = alloc<bf16_t>((size_t)pp_world * B * C * t.ldvt);
    }
    t.kvp = kv_for(C);
    if (!t.kvp && ok()) fail("no cross-attention K/V buffer for width " + std::to_string(C));
    if (pc) {
      t.vt_off.resize(B); t.ldvt_s.resize(B); t.Lk_s.resize(B);
      for (int g = 0; g < ng; ++g) for (int i = 0; i < gB[g]; ++i) { const int bb = gb0[g] + i; t.vt_off[bb] = t.g.vt0[g] + (long)i * C * t.g.ldvt[g]; t.ldvt_s[bb] = t.g.ldvt[g]; t.Lk_s[bb] = t.g.L[g]; }
    }
    for (int k = 0; k < layers && ok(); ++k) {
      const std::string b = p + ".transformer_blocks." + std::to_string(k);
      qkv(t, b);
      const int li = ok() ? t.kvp->next++ : 0;
      if (pc) attend_masked(t, b, li); else attend(t, b, li);
      feed_forward(t, b, k + 1 < layers ? t.via.norm1 : LnVia::Pass);
    }
    linear(Linear{t.y, C, p + ".proj_out", out, C, M, C, C}.plus(x, C));
    ar.release(m0);
    dump(p, out, (size_t)M * C);
    return out;
  }

  bool run(const void* latents, int io_dtype, const float* timesteps, const void* ehs, const void* text_embeds,
           const float* time_ids, void* outp) {
    const mx_unet_config& c = u->cfg;
    const int nlev = c.n_levels;
    const int C0 = c.block_out_channels[0];
    const int T = 4 * C0;
    const int text_dim = c.projection_class_embeddings_input_dim - 6 * c.addition_time_embed_dim;
    const int addw = c.projection_class_embeddings_input_dim;
    const int ctx = c.cross_attention_dim;

    // panel tickets of the producers that finalise LayerNorm statistics (transformer()): zero once, every launch leaves them zero
    ln_cnt = (unsigned*)ar.alloc((size_t)kLnCnt * sizeof(unsigned));
    if (ok() && !quiet() && ln_cnt && hipMemsetAsync(ln_cnt, 0, (size_t)kLnCnt * sizeof(unsigned), stream) != hipSuccess) fail("ln tickets: memset failed");
    // ---- time / added-condition embeddings (unet.py:314-341) ----
    bf16_t* tsin = alloc<bf16_t>((size_t)B * C0);
    bf16_t* addin = alloc<bf16_t>((size_t)B * addw);
    if (ok() && !dry &&
        mx::launch_time_embed(stream, timesteps, text_embeds, time_ids, tsin, addin, B, C0, text_dim, c.addition_time_embed_dim))
      fail(mx_last_error());
    bf16_t* t1 = alloc<bf16_t>((size_t)B * T);
    bf16_t* t2 = alloc<bf16_t>((size_t)B * T);
    bf16_t* a1 = alloc<bf16_t>((size_t)B * T);
    bf16_t* semb = alloc<bf16_t>((size_t)B * T);
    linear(Linear{tsin, C0, "time_embedding.linear_1", t1, T, B, T, C0}.epilogue(MX_EPI_SILU));
    linear(Linear{t1, T, "time_embedding.linear_2", t2, T, B, T, T});
    linear(Linear{addin, addw, "add_embedding.linear_1", a1, T, B, T, addw}.epilogue(MX_EPI_SILU));
    // silu(emb + aug_emb): the only consumer of emb is time_emb_proj(silu(emb)) (resnet.py:421)
    linear(Linear{a1, T, "add_embedding.linear_2", semb, T, B, T, T}.plus(t2, T).epilogue(MX_EPI_SILU));
    // all time_emb_proj linears in one GEMM, fp32 out
    temb_total = 2 * c.block_out_channels[nlev - 1];
    for (int i = 0; i < nlev; ++i) temb_total += (2 * c.layers_per_block + 1) * c.block_out_channels[i];     // down: layers_per_block resnets a level, up: one more
    temb_all = alloc<float>((size_t)B * temb_total);
    temb_off = 0;
    linear(Linear{semb, T, "temb_proj_all", temb_all, temb_total, B, temb_total, T}.epilogue(MX_EPI_OUT_F32));

    // ---- cross-attention K / V^T of encoder_hidden_states for every layer, one GEMM per width ----
    kv.clear();
    {
      const std::vector<std::pair<int, int>> widths = kv_widths(c);
      const int ldvt = MX_VT_LD(ctx_len);
      size_t wi = 0;
      for (auto& wv : widths) {
        const int dim = wv.first, nl = wv.second;
        KV e; e.dim = dim; e.next = 0; e.ldk = nl * dim; e.ldvt = ldvt; e.vt_bstride = (long)nl * dim * ldvt;
        if (ctx_e && !dry) { e.k = ctx_e->k[wi]; e.vt = ctx_e->vt[wi]; }        // the composition's own buffers (mx_unet_set_context_key)
        else { e.k = alloc<bf16_t>((size_t)B * ctx_len * nl * dim); e.vt = alloc<bf16_t>((size_t)B * nl * dim * ldvt); }
        ++wi;
        if (!(ctx_e && ctx_hit && !dry)) {
          mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
          d.a = ehs; d.lda = ctx; d.w = wb("attn2_kv_all." + std::to_string(dim) + ".weight", (size_t)nl * 2 * dim * ctx);
          d.c = e.k; d.ldc = nl * dim; d.M = B * ctx_len; d.N = nl * 2 * dim; d.K = ctx; d.flags = MX_EPI_QKV; d.seg = dim; d.period = 2;
          d.vt = e.vt; d.ldvt = ldvt; d.rows_per_batch = ctx_len;
          gemm(d, false);
        }
        kv.push_back(e);
      }
    }

    // ---- conv_in (unet.py:344) ----
    int h = H, wd = W;                    // the first group's image at the current level; ch / cw hold every group's
    for (int g = 0; g < ng; ++g) { ch[g] = gH[g]; cw[g] = gW[g]; }
    if (ng > 1 && (is_pp() || (bc && !pc))) fail("a mixed-resolution batch runs neither patch-parallel nor through the per-sample block cache");
    bf16_t* x0 = alloc<bf16_t>((size_t)rows() * kConvInPad);
    for (int g = 0; g < ng && ok() && !dry; ++g)
      if (mx::launch_prep_latent(stream, g_lat[g], io_dtype, x0 + row0(g) * kConvInPad, gB[g], c.in_channels, ch[g] * cw[g], kConvInPad)) fail(mx_last_error());
    bf16_t* x = alloc<bf16_t>((size_t)rows() * C0);
    // patches are cut from the true latent: no corner rule (unet.py:123-158), and no patch caches conv_in: conv(), not block_conv().  The
    // patch-parallel padded copy is allocated behind x and stays for the forward (every later offset counts from it)
    ConvIn in0{x0, nullptr};
    if (is_pp()) {
      in0 = alloc_conv_in(h, wd, kConvInPad);
      copy_to_padded(x0, in0.padded, h, wd, kConvInPad);
      halo_exchange(in0.padded, h, wd, kConvInPad);
    } else conv_cin_valid = c.in_channels <= 8 ? 8 : 0;
    conv(Conv{in0, h, wd, kConvInPad, "conv_in", x, C0});
    conv_cin_valid = 0;
    dump("conv_in", x, (size_t)rows() * C0);

    struct Skip { bf16_t* t; int C; int h, wd; int level; };
    std::vector<Skip> skips;
    skips.push_back({x, C0, h, wd, 0});
    int lvl = 0;                          // level of x (patch-unit cache: the level a state tensor is laid out for)
    int Ccur = C0;
    // The seven blocks the reference wraps with a CacheManager (unet_2d_blocks.py): each body advances x / h / wd / Ccur / skips.
    auto down_block = [&](int i) {                              // unet.py:371-405
      const int Cout = c.block_out_channels[i];
      for (int j = 0; j < c.layers_per_block && ok(); ++j) {
        const std::string rp = "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
        x = resnet(rp, x, h, wd, Ccur, Cout, i);
        Ccur = Cout;
        if (c.down_has_attn[i]) {
          const std::string ap = "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j);
          x = transformer(ap, x, h, wd, Cout, c.num_heads[i], c.transformer_layers[i], i);
        }
        skips.push_back({x, Cout, h, wd, i});
      }
      if (i != nlev - 1) {
        const std::string dp = "down_blocks." + std::to_string(i) + ".downsamplers.0";
        size_t drows = 0;
        for (int g = 0; g < ng; ++g) drows += (size_t)gB[g] * ((ch[g] + 1) / 2) * ((cw[g] + 1) / 2);
        bf16_t* d = alloc<bf16_t>(drows * Cout);
        block_conv_of(x, Conv{{}, h, wd, Cout, dp + ".conv", d, Cout}.strided(2), i);   // resnet.py:364-371; PatchDownsample2D (resnet.py:341-378) under a mask
        h /= 2; wd /= 2;
        for (int g = 0; g < ng; ++g) { ch[g] = (ch[g] + 1) / 2; cw[g] = (cw[g] + 1) / 2; }
        x = d;
        lvl = i + 1;
        dump(dp, x, (size_t)rows() * Cout);
        skips.push_back({x, Cout, h, wd, i + 1});
      }
    };
    auto mid_block = [&]() {                                    // unet.py:419-445
      const int Cm = c.block_out_channels[nlev - 1];
      x = resnet("mid_block.resnets.0", x, h, wd, Cm, Cm, nlev - 1);
      x = transformer("mid_block.attentions.0", x, h, wd, Cm, c.num_heads[nlev - 1], c.transformer_layers[nlev - 1], nlev - 1);
      x = resnet("mid_block.resnets.1", x, h, wd, Cm, Cm, nlev - 1);
    };
    auto up_block = [&](int i) {                                // unet.py:458-503
      const int level = nlev - 1 - i;
      const int Cout = c.block_out_channels[level];
      for (int j = 0; j < c.layers_per_block + 1 && ok(); ++j) {
        const Skip sk = skips.back(); skips.pop_back();
        const std::string rp = "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
        x = resnet(rp, x, h, wd, Ccur + sk.C, Cout, level, sk.t, sk.C);   // torch.cat([x, skip], dim=1) is never materialised
        Ccur = Cout;
        if (c.down_has_attn[level]) {
          const std::string ap = "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j);
          x = transformer(ap, x, h, wd, Cout, c.num_heads[level], c.transformer_layers[level], level);
        }
      }
      if (i != nlev - 1) {
        const std::string upn = "up_blocks." + std::to_string(i) + ".upsamplers.0";
        bf16_t* d = alloc<bf16_t>((size_t)rows() * 4 * Cout);
        block_conv_of(x, Conv{{}, h, wd, Cout, upn + ".conv", d, Cout}.upsampled(), level);   // resnet.py:316, 327-333; PatchUpsample2D (resnet.py:280-339) under a mask
        h *= 2; wd *= 2;
        for (int g = 0; g < ng; ++g) { ch[g] *= 2; cw[g] *= 2; }
        x = d;
        lvl = level - 1;
        dump(upn, x, (size_t)rows() * Cout);
      }
    };

    // Block-skip cache (mx_unet_forward_cached; include/mxdenoise.h): inputs = the tensors the predictor's features come from, body = the
    // block.  A reused block still walks its plan (mute) so that the arena, the K / V cursors and the time-embedding offset advance as if it
    // had run; its outputs are then filled from the cache.
    struct Ten { bf16_t* p; size_t per_sample; int C = 0; int level = 0; };
    // The same at the reference's unit, the PATCH (pc; mx_unet_forward_cached_mixed): features, decision and merge per patch, ONE host decision
    // per block for the patches of every sample of every resolution group, the block's ops computing the asking patches only (Plan::pc_conv,
    // the masked transformer layer).
    auto run_block_pc = [&](int idx, bool is_up, const std::vector<Ten>& ins, const std::function<void()>& body) {
      const int nf = (int)ins.size();
      std::vector<char*> in_cache(nf);
      for (int f = 0; f < nf; ++f) in_cache[f] = pc_region(ins[f].level, ins[f].C);
      auto outputs = [&](size_t n0) {
        std::vector<Ten> outs;
        if (!is_up) for (size_t k = std::min(n0, skips.size()); k < skips.size(); ++k) outs.push_back({skips[k].t, 0, skips[k].C, skips[k].level});
        if (outs.empty() || outs.back().p != x) outs.push_back({x, 0, Ccur, lvl});
        return outs;
      };
      if (dry) {
        const size_t n0 = skips.size();
        body();
        for (auto& o : outputs(n0)) pc_region(o.level, o.C);
        return;
      }
      if (!ok()) return;
      // the features: per patch and pixel row, the sum of (input - cached input)^2, left on the device
      size_t off = 0;
      std::vector<size_t> offs(nf);
      for (int f = 0; f < nf && ok() && bc_any_valid; ++f) {
        const int pl = pc_p0 >> ins[f].level;
        offs[f] = off;
        if (mx::launch_pc_patch_sq_diff(stream, ins[f].p, in_cache[f], pc_row_elems(ins[f].level, ins[f].C), ins[f].C, pc_dall, pc_np, pc_dsamp, ins[f].level, pl,
                                        pc_dpart + off)) fail(mx_last_error());
        off += (size_t)pc_np * pl;
      }
      if (!ok()) return;
      // THE DECISION -- the one place the two modes differ.  Either way it leaves pc_nask, pc_ask_first and, when some patch does not ask, the
      // list of the asking patches in pc_dask.
      if (bc_dev) {
        // on the device (mx_block_cache.dev_down): one launch finalises the features, walks the forest, applies the counter rule and compacts
        // the list; the host reads back the counts alone (patch_cache.hip pc_decide_kernel; skip_decide.h)
        mx_skip_decide_args a{};
        a.forest = (is_up && bc->dev_up) ? bc->dev_up : bc->dev_down;
        a.n_in = nf; a.kind = 0; a.units = pc_dall; a.samples = pc_dsamp; a.partial = pc_dpart; a.grid_w = pc_maxw / pc_p0; a.ask_units = pc_dask;
        for (int f = 0; f < nf; ++f) {
          const int pl = pc_p0 >> ins[f].level;
          a.part_off[f] = (int64_t)offs[f]; a.part_len[f] = pl; a.part_elems[f] = (double)pl * pl * ins[f].C;
        }
        const int32_t* rec = bc_dev_decide(a, idx, false, nullptr);
        if (!rec) return;
        pc_nask = rec[MX_SKIP_REC_NASK];
        pc_ask_first.assign(rec + MX_SKIP_REC_FIRST, rec + MX_SKIP_REC_FIRST + B + 1);
      } else {
        // on the host: every partial sum comes back, the caller's predictor answers, the list goes out again
        std::vector<float> mse((size_t)pc_np * nf, MX_MSE_UNCACHED);
        if (bc_any_valid) {
          std::vector<double> hp(off);
          if (hipMemcpyAsync(hp.data(), pc_dpart, off * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
              hipStreamSynchronize(stream) != hipSuccess) { fail("patch cache: reading the input differences failed"); return; }
          for (int f = 0; f < nf; ++f) {
            const int pl = pc_p0 >> ins[f].level;
            for (int j = 0; j < pc_np; ++j) {
              if (!bc_valid[pc_all[j].b]) continue;                  // nothing cached for this request: the marker stays (cache_manager.py:110,139)
              double t = 0.0;
              for (int r = 0; r < pl; ++r) t += hp[offs[f] + (size_t)j * pl + r];
              mse[(size_t)j * nf + f] = (float)(t / ((double)pl * pl * ins[f].C));
            }
          }
        }
        std::vector<unsigned char> run(pc_np, 1);
        std::vector<float> tpp(pc_np);
        for (int j = 0; j < pc_np; ++j) tpp[j] = h_timesteps[pc_all[j].b];
        if (bc->predict(bc->ctx, idx, is_up ? 1 : 0, pc_np, nf, tpp.data(), mse.data(), run.data())) { fail("patch cache: the predictor failed"); return; }
        pc_ask.clear(); pc_ask_first.assign(B + 1, 0);
        for (int j = 0; j < pc_np; ++j) {
          if (!bc_valid[pc_all[j].b]) run[j] = 1;                    // a patch without cached tensors has nothing to reuse (uninitialised rows in the reference)
          if (run[j]) { pc_ask.push_back(pc_all[j]); pc_ask_first[pc_all[j].b + 1]++; }
        }
        for (int b = 0; b < B; ++b) pc_ask_first[b + 1] += pc_ask_first[b];
        pc_nask = (int)pc_ask.size();
        if (pc_nask > 0 && pc_nask < pc_np &&
            hipMemcpyAsync(pc_dask, pc_ask.data(), pc_ask.size() * sizeof(mx::PcPatch), hipMemcpyHostToDevice, stream) != hipSuccess) {
          fail("patch cache: sending the list of asking patches failed"); return;
        }
      }
      pc_partial = pc_nask < pc_np;
      const bool any = pc_nask > 0;
      pc_total += (unsigned long long)pc_np; pc_asked += (unsigned long long)pc_nask;
      for (int f = 0; f < nf && ok(); ++f) pc_store(ins[f].p, in_cache[f], ins[f].level, ins[f].C);   // the cached input is always the latest one (:133,153)
      const size_t n0 = skips.size();
      mute = !any;
      body();
      mute = false;
      for (auto& o : outputs(n0)) {
        char* oc = pc_region(o.level, o.C);
        if (!ok()) return;
        if (any ? !pc_store(o.p, oc, o.level, o.C) : !pc_load(o.p, oc, o.level, o.C)) return;
      }
      if (any) blocks_run |= 1u << idx;
    };
    auto run_block = [&](int idx, bool is_up, const std::vector<Ten>& ins, const std::function<void()>& body) {
      if (!bc) { body(); return; }
      if (pc) { run_block_pc(idx, is_up, ins, body); return; }
      const int nf = (int)ins.size();
      const size_t R = (size_t)bc_rows;
      auto region = [&](size_t per_sample) { char* r = bc_top; bc_top += (per_sample * R * 2 + 255) & ~(size_t)255; return r; };
      if (dry) {                                                 // mx_unet_block_cache_bytes: the same bump pointer, no launches
        for (int f = 0; f < nf; ++f) region(ins[f].per_sample);
        const size_t n0 = skips.size();
        body();
        size_t n_out = 0;
        bool x_listed = false;
        if (!is_up) for (size_t k = std::min(n0, skips.size()); k < skips.size(); ++k) {
          region((size_t)skips[k].h * skips[k].wd * skips[k].C); ++n_out; x_listed = skips[k].t == x;
        }
        if (!n_out || !x_listed) region((size_t)h * wd * Ccur);
        return;
      }
      std::vector<float> mse((size_t)B * nf, MX_MSE_UNCACHED);
      std::vector<char*> in_cache(nf);
      for (int f = 0; f < nf; ++f) in_cache[f] = region(ins[f].per_sample);
      if ((size_t)(bc_top - (char*)bc->state) > bc->state_bytes) { fail("block cache: state buffer too small (mx_unet_block_cache_bytes)"); return; }
      if (bc_any_valid && ok()) {
        double* part = (double*)bc->state;                       // the head of the state is scratch (bc_scratch_bytes)
        for (int f = 0; f < nf && ok(); ++f)
          if (mx::launch_sq_diff_partial(stream, ins[f].p, in_cache[f], (long)ins[f].per_sample, B, part + (size_t)f * B * 64, bc_dslot)) fail(mx_last_error());
        // feature f's B rows one after the other; a sample with nothing cached keeps the marker (cache_manager.py:110,139)
        if (ok()) bc_read_mse(part, (size_t)nf * B, 64, mse.data(), "block cache: reading the input differences failed", [&](size_t r) {
          const size_t f = r / B, b = r % B;
          return MseRow{(int)b, (double)ins[f].per_sample, b * nf + f}; });
      }
      if (!ok()) return;
      std::vector<unsigned char> run(B, 1);
      if (bc->predict(bc->ctx, idx, is_up ? 1 : 0, B, nf, h_timesteps.data(), mse.data(), run.data())) { fail("block cache: the predictor failed"); return; }
      bool any = !bc_all_valid;                                  // a sample without cached tensors has nothing to reuse
      for (int b = 0; b < B; ++b) any = any || run[b] != 0;
      // Partial reuse INSIDE a running block: a sample that did not ask keeps, for every op of the block, the output that op produced at the
      // sample's last run (every Split* / Patch* module holds its own output cache and computes the asking rows only: resnet.py:157-172,
      // 414-419, 449-454; attention.py:73-76, 104, 224; cache_manager.py:84-99 update_and_return).  Samples do not interact inside a block
      // when each is one patch (is_sliced False: unet.py:261-272 keys the caches by request), so for them this is exactly "the block's
      // outputs of a not-asking sample are the cached ones": the block runs for the batch and those rows are then restored from the state.
      // (With several patches per latent the reference also feeds the stale patches' values into their neighbours' halos, GroupNorm
      // statistics and attention keys: not reproduced -- the unit here is the sample.)
      std::vector<int>& sel = bc_sel;                          // (a Plan member: the source of the asynchronous copy below outlives this block)
      sel.assign(B, -1);
      bool partial = false;
      if (any) for (int b = 0; b < B; ++b) if (!run[b] && bc_valid[b]) { sel[b] = bc->slots ? bc->slots[b] : b; partial = true; }
      if (partial && ok() && hipMemcpyAsync(bc_dsel(), sel.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess)
        fail("block cache: sending the selection table failed");
      for (int f = 0; f < nf && ok(); ++f)                       // the cached input is always the latest one (cache_manager.py:133,153)
        bc_store(in_cache[f], ins[f].p, ins[f].per_sample * 2);
      const size_t n_skips0 = skips.size();
      mute = !any;
      body();
      mute = false;
      // outputs: the hidden state and, for the down blocks, the skip tensors the block pushed
      std::vector<Ten> outs;
      if (!is_up) for (size_t k = std::min(n_skips0, skips.size()); k < skips.size(); ++k) outs.push_back({skips[k].t, (size_t)skips[k].h * skips[k].wd * skips[k].C});
      if (outs.empty() || outs.back().p != x) outs.push_back({x, (size_t)h * wd * Ccur});
      for (auto& o : outs) {
        char* oc = region(o.per_sample);
        if ((size_t)(bc_top - (char*)bc->state) > bc->state_bytes) { fail("block cache: state buffer too small (mx_unet_block_cache_bytes)"); return; }
        if (!ok()) return;
        if (any && bc_all_valid && bc->observe && o.p == x) {     // how far the block's output moved since its last run (fitting labels)
          double* part = (double*)bc->state;
          std::vector<float> om(B);
          if (mx::launch_sq_diff_partial(stream, o.p, oc, (long)o.per_sample, B, part, bc_dslot)) { fail(mx_last_error()); return; }
          if (!bc_read_mse(part, B, 64, om.data(), "block cache: reading the output differences failed",
                           [&](size_t b) { return MseRow{(int)b, (double)o.per_sample, b}; })) return;
          bc->observe(bc->ctx, idx, B, om.data());
        }
        if (any && partial && mx::launch_copy_rows(stream, o.p, oc, o.per_sample * 2, B, bc_dsel(), 0)) { fail(mx_last_error()); return; }
        if (any ? !bc_store(oc, o.p, o.per_sample * 2) : !bc_load(o.p, oc, o.per_sample * 2)) return;
      }
      if (any) blocks_run |= 1u << idx;
    };
    auto up_inputs = [&](int n) {
      std::vector<Ten> v{{x, (size_t)h * wd * Ccur, Ccur, lvl}};
      // column order of the reference's feature row: mse(x), then res_hidden_states_tuple[0 .. n-1] = the block's skips OLDEST first, the
      // first-consumed one last (cache_manager.py:110-121; unet_2d_blocks.py:250-257 takes res_hidden_states_tuple[-1] first)
      const int have = std::min<int>(n, (int)skips.size());
      for (int k = 0; k < have; ++k) { const Skip& sk = skips[skips.size() - have + k]; v.push_back({sk.t, (size_t)sk.h * sk.wd * sk.C, sk.C, sk.level}); }
      return v;
    };
    int block = 0;
    if (bc && !pc) {
      if (bc_rows < B) bc_rows = B;
      bc_top = (dry ? (char*)(uintptr_t)0x1000 : (char*)bc->state) + bc_scratch_bytes(c.layers_per_block, bc_rows);
    }
    if (pc) bc_top = (dry ? (char*)(uintptr_t)0x1000 : (char*)bc->state) + pc_head_bytes(pc_slots, pc_maxh, pc_maxw, pc_p0);
    for (int i = 0; i < nlev && ok(); ++i, ++block) run_block(block, false, {{x, (size_t)h * wd * Ccur, Ccur, lvl}}, [&] { down_block(i); });
    if (ok()) { run_block(block, false, {{x, (size_t)h * wd * Ccur, Ccur, lvl}}, [&] { mid_block(); }); ++block; }
    for (int i = 0; i < nlev && ok(); ++i, ++block) run_block(block, true, up_inputs(c.layers_per_block + 1), [&] { up_block(i); });
    // ---- out (unet.py:508-517) ----
    {
      const size_t M = (size_t)rows();
      const int Co = c.out_channels;
      const int ldo = (Co + 3) / 4 * 4;
      bf16_t* o = alloc<bf16_t>(M * ldo);
      ConvIn n = alloc_conv_in(h, wd, C0);        // (not released: the forward ends here)
      norm_into(n, x, "conv_norm_out", h, wd, C0, 0);
      Conv co{n, h, wd, C0, "conv_out", o, ldo};  // no patch caches conv_out: conv(), not block_conv()
      co.corner_patch = level_patch(0);
      conv(co);
      dump("conv_out", o, M * ldo);
      for (int g = 0; g < ng && ok() && !dry; ++g)
        if (mx::launch_nhwc_to_nchw(stream, o + row0(g) * ldo, g_out[g], io_dtype, gB[g], Co, ch[g] * cw[g], ldo)) fail(mx_last_error());
    }
    if (stage && !dry && ok() && !stage_hit) fail(std::string("unknown stage '") + stage + "'");
    return ok();
  }
};

int check_cfg(const mx_unet_config* c) {
  MX_CHECK(c != nullptr, "unet: null config");
  MX_CHECK(c->n_levels >= 1 && c->n_levels <= 4, "unet: n_levels must be 1..4");
  MX_CHECK(c->in_channels > 0 && c->in_channels <= kConvInPad, "unet: in_channels must be <= 64");
  MX_CHECK(c->out_channels > 0 && c->out_channels <= 64, "unet: bad out_channels");
  for (int i = 0; i < c->n_levels; ++i) {
    MX_CHECK(c->block_out_channels[i] % 64 == 0, "unet: block_out_channels must be multiples of 64");
    MX_CHECK(c->block_out_channels[i] % c->norm_num_groups == 0, "unet: channels % norm_num_groups != 0");
    if (c->down_has_attn[i]) MX_CHECK(c->num_heads[i] * 64 == c->block_out_channels[i], "unet: head_dim must be 64");
  }
  MX_CHECK(c->down_has_attn[c->n_levels - 1], "unet: the mid block needs attention at the last level");
  MX_CHECK(c->cross_attention_dim % 64 == 0, "unet: cross_attention_dim must be a multiple of 64");
  MX_CHECK(c->projection_class_embeddings_input_dim % 64 == 0, "unet: projection_class_embeddings_input_dim must be a multiple of 64");
  MX_CHECK(c->addition_time_embed_dim % 2 == 0, "unet: addition_time_embed_dim must be even");
  return 0;
}

// The stored K / V^T entry of the composition u->ctx_key for a forward of `B` samples on `stream` (nullptr: the store is off or could not be had -- the
// forward then projects into its workspace as before).  hit: the entry already holds this composition's projection.  The forward's stream waits for
// whichever stream touched the entry last.  Host side only; allocations run with the thread's capture mode relaxed (never reached with MX_GRAPH on).
mx_unet::CtxEntry* ctx_prepare(mx_unet* u, hipStream_t stream, int B, int ctx_len, bool& hit) {
  hit = false;
  if (u->ctx_key == 0 || mx::GraphCache::env_on()) return nullptr;
  constexpr size_t kMaxEntries = 4;
  mx_unet::CtxEntry* e = nullptr;
  for (auto& q : u->ctx_store) if (q.valid && q.key == u->ctx_key && q.B == B && q.ctx_len == ctx_len) { e = &q; hit = true; break; }
  if (!e) {
    if (u->ctx_store.size() < kMaxEntries) { u->ctx_store.reserve(kMaxEntries); u->ctx_store.emplace_back(); e = &u->ctx_store.back(); }
    else { e = &u->ctx_store[0]; for (auto& q : u->ctx_store) if (q.stamp < e->stamp) e = &q; }
    e->valid = false;
    const std::vector<std::pair<int, int>> widths = kv_widths(u->cfg);
    const int ldvt = MX_VT_LD(ctx_len);
    if (!e->ev && hipEventCreateWithFlags(&e->ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); e->ev = nullptr; return nullptr; }
    e->k.resize(widths.size(), nullptr); e->vt.resize(widths.size(), nullptr); e->k_bytes.resize(widths.size(), 0); e->vt_bytes.resize(widths.size(), 0);
    for (size_t i = 0; i < widths.size(); ++i) {
      const size_t kb = (size_t)B * ctx_len * widths[i].second * widths[i].first * sizeof(bf16_t);
      const size_t vb = (size_t)B * widths[i].second * widths[i].first * ldvt * sizeof(bf16_t);
      if (e->k_bytes[i] < kb || e->vt_bytes[i] < vb) {
        if (e->last) (void)hipStreamSynchronize(e->last);       // (the old buffers may still be read)
        if (e->k[i]) (void)hipFree(e->k[i]);
        if (e->vt[i]) (void)hipFree(e->vt[i]);
        e->k[i] = nullptr; e->vt[i] = nullptr; e->k_bytes[i] = e->vt_bytes[i] = 0;
        if (hipMalloc(&e->k[i], kb) != hipSuccess || hipMalloc(&e->vt[i], vb) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        e->k_bytes[i] = kb; e->vt_bytes[i] = vb;
      }
    }
    e->key = u->ctx_key; e->B = B; e->ctx_len = ctx_len;
  }
  if (e->recorded && e->last != stream && hipStreamWaitEvent(stream, e->ev, 0) != hipSuccess) { (void)hipGetLastError(); hit = false; return nullptr; }
  e->stamp = ++u->ctx_clock;
  if (hit) ++u->ctx_hits; else ++u->ctx_misses;
  return e;
}

// what run_forward (plan_base.h) needs to know of the UNet; one object per call: it carries the composition's stored cross-attention K / V^T
struct Model {
  const char* name = "unet";
  mx_unet::CtxEntry* ctx_e = nullptr;
  bool ctx_hit = false;
  // H, W against the level count and the GroupNorm patch (is_sliced)
  static int check_shape(const mx_unet* u, int H, int W, int gn_patch) {
    const int div = 1 << (u->cfg.n_levels - 1);
    MX_CHECK(H % div == 0 && W % div == 0, "unet: H, W must be divisible by 2^(levels-1)");
    MX_CHECK(gn_patch >= 0, "unet: gn_patch must be >= 0");
    if (gn_patch > 0) {
      MX_CHECK(H % gn_patch == 0 && W % gn_patch == 0, "unet: H, W must be multiples of gn_patch");
      MX_CHECK((gn_patch >> (u->cfg.n_levels - 1)) >= 2 || gn_patch >= H, "unet: gn_patch too small for the deepest level (needs >= 2 pixels there)");
    }
    return 0;
  }
  // the patch unit (mx_unet_forward_cached_mixed and its sizing walks): patches of >= 2 pixels at the deepest level; the device decision's down
  // and mid blocks compare their input, an up block its input and the skips it consumes
  int check_units(const mx_unet* u, const mx::ForwardCall& c) {
    const std::string who = c.cached_who(name);
    MX_CHECK(c.gn_patch > 0 && (c.gn_patch >> (u->cfg.n_levels - 1)) >= 2, who + ": the patch unit needs is_sliced (gn_patch > 0, >= 2 pixels at the deepest level)");
    return mx::check_cache_units(who, c, c.gn_patch, "gn_patch", 2 * u->cfg.n_levels + 1, 1, u->cfg.layers_per_block + 2);
  }
  int check(const mx_unet* u, const mx::ForwardCall& c) {
    const int div = 1 << (u->cfg.n_levels - 1);
    if (!c.units()) {     // (the patch unit has stated its own rule for H, W, whole patches: a call it accepts is not measured against 2^(levels-1) as well)
      for (int g = 0; c.groups && g < c.n_groups; ++g) {
        const mx_unet_group& q = c.groups[g];
        MX_CHECK(q.H % div == 0 && q.W % div == 0, "unet: bad group shape");
        if (c.gn_patch > 0)
          MX_CHECK((q.H % c.gn_patch == 0 && q.W % c.gn_patch == 0) || (c.gn_patch >= q.H && c.gn_patch >= q.W), "unet: every group's H, W must be multiples of gn_patch");
      }
      if (c.pp()) {
        MX_CHECK(c.gn_patch == 0, "unet pp: patch-parallel runs the exact (is_sliced=False) arithmetic");
        MX_CHECK(c.H % div == 0, "unet pp: local rows must be divisible by 2^(levels-1)");
      }
      if (check_shape(u, c.H, c.W, c.gn_patch)) return 1;
    }
    MX_CHECK(c.dry || (c.text_embeds && c.time_ids), "unet: null operand");
    return 0;
  }
  // the composition's stored cross-attention K / V^T (mx_unet_set_context_key): plain and mixed forwards; not patch-parallel (its ranks hold row bands).
  // A cached forward projects into its workspace: it neither consults the store nor uses up the key, which stays for the uncached forward it names.
  void begin(mx_unet* u, const mx::ForwardCall& c) {
    if (c.dry || c.cache) return;
    if (!c.pp()) {
      int Btot = c.batch;
      if (c.groups) { Btot = 0; for (int g = 0; g < c.n_groups; ++g) Btot += c.groups[g].batch; }
      ctx_e = ctx_prepare(u, (hipStream_t)c.stream, Btot, c.ctx_len, ctx_hit);
    }
    u->ctx_key = 0;     // the key names ONE forward: a later call that does not announce itself (a trace, another caller of the handle) projects afresh
  }
  void end(mx_unet*, const mx::ForwardCall& c, bool okr) {
    if (!ctx_e) return;          // the entry belongs to this stream until the event: later forwards on other streams wait for it
    ctx_e->valid = okr;
    ctx_e->last = (hipStream_t)c.stream;
    ctx_e->recorded = hipEventRecord(ctx_e->ev, (hipStream_t)c.stream) == hipSuccess;
    if (!ctx_e->recorded) { (void)hipGetLastError(); (void)hipStreamSynchronize((hipStream_t)c.stream); }
  }
  int setup(Plan& p, mx_unet* u, const mx::ForwardCall& c) {
    p.u = u; p.ctx_len = c.ctx_len; p.ctx_e = ctx_e; p.ctx_hit = ctx_hit;
    bool patch_covers_all = !c.units();     // (the patch unit keeps its gn_patch even where it covers every group: it is the cache's unit, pc_p0)
    for (int g = 0; g < p.ng; ++g) patch_covers_all = patch_covers_all && c.gn_patch >= p.gH[g] && c.gn_patch >= p.gW[g];
    p.gn_patch = patch_covers_all ? 0 : c.gn_patch;
    if (c.pp()) { p.pp_rank = c.comm->rank; p.pp_world = c.comm->world; p.Htot = c.H * c.comm->world; }
    return c.cache ? setup_cache(p, u, c) : 0;
  }
  // The cache's mode of the plan.  A sizing walk stops at the host tables; a forward then learns which samples hold state and queues on its stream,
  // ahead of the first launch and in this order: the slot table, the sample and patch tables, the device decision's tables, the timestep read-back.
  int setup_cache(Plan& p, mx_unet* u, const mx::ForwardCall& c) {
    const std::string who = c.cached_who(name);
    mx_block_cache* cache = c.cache;
    p.bc = cache;
    if (!c.units()) {
      if (c.dry) return 0;
      return p.bc_begin(who, cache, c.batch, c.H, c.W) || p.bc_send_slots(who, Plan::bc_part_rows(u->cfg.layers_per_block), Plan::kBcTables, c.batch) ||
             p.bc_read_timesteps(who, c.timesteps, c.batch);
    }
    const int gp = c.gn_patch, B = p.B;
    p.pc = true; p.pc_p0 = gp; p.pc_maxh = cache->max_h; p.pc_maxw = cache->max_w; p.pc_slots = cache->n_slots;
    long long row0 = 0;
    for (int g = 0; g < p.ng; ++g)
      for (int i = 0; i < p.gB[g]; ++i) {
        const int b = p.gb0[g] + i;
        mx::PcSample s; s.row0 = row0; s.h = p.gH[g]; s.w = p.gW[g]; s.slot = (!c.dry && cache->slots) ? cache->slots[b] : b; s.npx = p.gW[g] / gp;
        p.pc_samp.push_back(s);
        for (int py = 0; py < p.gH[g] / gp; ++py)
          for (int px = 0; px < p.gW[g] / gp; ++px) p.pc_all.push_back(mx::PcPatch{b, py, px, 0});
        row0 += (long long)p.gH[g] * p.gW[g];
      }
    p.pc_np = (int)p.pc_all.size();
    if (c.dry) return 0;
    if (p.bc_begin_slots(who, cache, B)) return 1;
    MX_CHECK(p.pc_head_bytes(p.pc_slots, p.pc_maxh, p.pc_maxw, gp) <= cache->state_bytes, who + ": state buffer too small");
    const size_t npm = Plan::pc_np_max(p.pc_slots, p.pc_maxh, p.pc_maxw, gp);
    char* hp = (char*)cache->state;
    p.pc_dpart = (double*)hp; hp += (size_t)(u->cfg.layers_per_block + 2) * npm * gp * sizeof(double);
    p.pc_dsamp = (mx::PcSample*)hp; hp += (size_t)p.pc_slots * sizeof(mx::PcSample);
    p.pc_dall = (mx::PcPatch*)hp; hp += npm * sizeof(mx::PcPatch);
    p.pc_dask = (mx::PcPatch*)hp;
    MX_CHECK(hipMemcpyAsync(p.pc_dsamp, p.pc_samp.data(), (size_t)B * sizeof(mx::PcSample), hipMemcpyHostToDevice, p.stream) == hipSuccess &&
             hipMemcpyAsync(p.pc_dall, p.pc_all.data(), (size_t)p.pc_np * sizeof(mx::PcPatch), hipMemcpyHostToDevice, p.stream) == hipSuccess,
             who + ": moving the tables failed");
    std::vector<int> unit_b(p.pc_np);
    for (int j = 0; j < p.pc_np; ++j) unit_b[j] = p.pc_all[j].b;
    return p.bc_dev_begin(who, u->skip_pin, 2 * u->cfg.n_levels + 1, (cache->max_h / gp) * (cache->max_w / gp), c.timesteps, std::move(unit_b), p.group_of(), false) ||
           p.bc_read_timesteps(who, c.timesteps, B);
  }
  bool run(Plan& p, const mx::ForwardCall& c) {
    const bool okr = p.run(c.latents, c.io_dtype, c.timesteps, c.ehs, c.text_embeds, c.time_ids, c.out);
    if (c.units() && !c.dry) { c.cache->patches_asked = p.pc_asked; c.cache->patches_total = p.pc_total; }
    return okr;
  }
  size_t cache_bytes(const Plan& p) { return (size_t)(p.bc_top - (char*)(uintptr_t)0x1000); }     // (a dry walk's bump pointer starts at a placeholder base, as the arena does)
  std::vector<uint64_t> key_scalars(const mx::ForwardCall& c) { return {(uint64_t)c.gn_patch}; }
  std::vector<const void*> key_operands(const mx::ForwardCall& c) { return {c.text_embeds, c.time_ids}; }
};
int forward_impl(const mx_unet* u, const mx::ForwardCall& c) {
  Model m;
  return mx::run_forward<Plan>(const_cast<mx_unet*>(u), c, m);
}
using mx::dry_call;
using mx::sizing_comm;
// the fields every forward entry point fills alike; the image (latents, out, batch, H, W) or the groups, gn_patch and the mode's own fields follow
mx::ForwardCall forward_call(void* stream, int io_dtype, const float* timesteps, const void* ehs, const void* text_embeds, const float* time_ids, int ctx_len,
                             void* workspace, size_t workspace_bytes) {
  mx::ForwardCall c;
  c.stream = stream; c.io_dtype = io_dtype; c.timesteps = timesteps; c.ehs = ehs; c.text_embeds = text_embeds; c.time_ids = time_ids; c.ctx_len = ctx_len;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  return c;
}

}  // namespace

extern "C" mx_unet* mx_unet_create(const mx_unet_config* cfg) {
  if (check_cfg(cfg)) return nullptr;
  mx_unet* u = new mx_unet();
  u->cfg = *cfg;
  return u;
}

extern "C" void mx_unet_destroy(mx_unet* u) { delete u; }

extern "C" int mx_unet_ln_routes(int M, int C, int layers, int n_groups, int flags, int routes[4]) {
  MX_CHECK(routes != nullptr && C > 0 && C % 64 == 0 && layers > 0 && n_groups >= 1 && n_groups <= MX_MAX_SEGS && M >= n_groups, "unet_ln_routes: bad arguments");
  const mx::LnRoutes r = mx::ln_routes(mx::LnRows::even(M, n_groups), C, layers, (flags & MX_LN_ROUTES_PATCH_PARALLEL) != 0, (flags & MX_LN_ROUTES_PATCH_CACHE) != 0,
                                       (flags & MX_LN_ROUTES_TICKETS) != 0);
  routes[0] = (int)r.norm1; routes[1] = (int)r.norm2; routes[2] = (int)r.norm3; routes[3] = r.norm3_from_merge ? 1 : 0;
  return 0;
}

extern "C" int mx_unet_set_context_key(mx_unet* u, uint64_t key) {
  MX_CHECK(u != nullptr, "unet_set_context_key: null handle");
  u->ctx_key = key;
  return 0;
}
extern "C" int mx_unet_context_stats(const mx_unet* u, long* hits, long* misses) {
  MX_CHECK(u != nullptr, "unet_context_stats: null handle");
  if (hits) *hits = u->ctx_hits;
  if (misses) *misses = u->ctx_misses;
  return 0;
}

extern "C" int mx_unet_set_weights(mx_unet* u, const void* blob, uint64_t blob_bytes, const mx_weight_entry* table, int n) {
  MX_CHECK(u != nullptr, "unet_set_weights: null handle");
  u->graphs.clear();    // captured graphs hold addresses resolved through the old table
  u->ctx_clear();       // stored projections were made with the old weights
  return u->weights.set("unet_set_weights", blob, blob_bytes, table, n);
}

extern "C" size_t mx_unet_workspace_bytes(const mx_unet* u, int batch, int H, int W, int ctx_len) {
  if (!u) return 0;
  // the sliced variant needs the larger GroupNorm scratch: size for the smallest legal patch
  size_t best = 0;
  const int div = 1 << (u->cfg.n_levels - 1);
  for (int gp : {0, 2 * div}) {
    if (gp > 0 && (H % gp != 0 || W % gp != 0 || gp >= H)) continue;
    size_t peak = 0;
    mx::ForwardCall c = dry_call(batch, H, W, ctx_len);
    c.gn_patch = gp; c.peak = &peak;
    if (forward_impl(u, c)) return 0;
    best = std::max(best, peak);
  }
  return best + 4096;
}

extern "C" int mx_unet_validate(const mx_unet* u, int batch, int H, int W, int ctx_len) {
  MX_CHECK(u && u->weights.blob, "unet_validate: weights not set");
  mx::ForwardCall c = dry_call(batch, H, W, ctx_len);
  c.lookup = true;
  return forward_impl(u, c);
}

extern "C" int mx_unet_forward(mx_unet* u, void* stream, const void* latents, int io_dtype, const float* timesteps,
                               const void* ehs, const void* text_embeds, const float* time_ids, void* out, int batch, int H,
                               int W, int ctx_len, int gn_patch, void* workspace, size_t workspace_bytes) {
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, text_embeds, time_ids, ctx_len, workspace, workspace_bytes);
  c.latents = latents; c.out = out; c.batch = batch; c.H = H; c.W = W; c.gn_patch = gn_patch;
  return forward_impl(u, c);
}

/* ---- mixed-resolution batch: ONE launch sequence over the requests of every resolution present (the reference batches
 * 512 / 768 / 1024 px requests by cutting all of them into 256-px patches, modules/unet.py:104-185) ---- */
extern "C" size_t mx_unet_workspace_bytes_mixed(const mx_unet* u, const mx_unet_group* groups, int n_groups, int ctx_len) {
  if (!u || !groups || n_groups < 1 || n_groups > MX_MAX_SEGS) return 0;
  size_t best = 0;
  const int div = 1 << (u->cfg.n_levels - 1);
  for (int gp : {0, 2 * div}) {                 // (the sliced GroupNorm needs the larger scratch: size for the smallest legal patch)
    bool legal = true;
    for (int g = 0; g < n_groups; ++g) legal = legal && (gp == 0 || (groups[g].H % gp == 0 && groups[g].W % gp == 0));
    if (!legal) continue;
    size_t peak = 0;
    mx::ForwardCall c = dry_call(0, 0, 0, ctx_len);
    c.groups = groups; c.n_groups = n_groups; c.gn_patch = gp; c.peak = &peak;
    if (forward_impl(u, c)) return 0;
    best = std::max(best, peak);
  }
  return best + 4096;
}

extern "C" int mx_unet_forward_mixed(mx_unet* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                                     const void* ehs, const void* text_embeds, const float* time_ids, int ctx_len, int gn_patch, void* workspace,
                                     size_t workspace_bytes) {
  MX_CHECK(groups != nullptr, "unet_forward_mixed: null groups");
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, text_embeds, time_ids, ctx_len, workspace, workspace_bytes);
  c.groups = groups; c.n_groups = n_groups; c.gn_patch = gn_patch;
  return forward_impl(u, c);
}

extern "C" int mx_unet_forward_mixed_trace(mx_unet* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                                           const void* ehs, const void* text_embeds, const float* time_ids, int ctx_len, int gn_patch, void* workspace,
                                           size_t workspace_bytes, const char* stage, void* stage_out, size_t stage_out_bytes) {
  MX_CHECK(groups != nullptr && stage && stage_out, "unet_forward_mixed_trace: groups, stage and stage_out required");
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, text_embeds, time_ids, ctx_len, workspace, workspace_bytes);
  c.groups = groups; c.n_groups = n_groups; c.gn_patch = gn_patch;
  c.stage = stage; c.stage_out = stage_out; c.stage_bytes = stage_out_bytes;
  return forward_impl(u, c);
}

/* ---- block-skip cache (include/mxdenoise.h; the reference's CacheManager, modules/cache_manager.py:101-161) ---- */
extern "C" size_t mx_unet_block_cache_bytes(const mx_unet* u, int batch, int H, int W) {
  if (!u || batch <= 0 || H <= 0 || W <= 0) return 0;
  const int div = 1 << (u->cfg.n_levels - 1);
  if (H % div || W % div) return 0;
  mx_block_cache sizing{};
  size_t state = 0;
  mx::ForwardCall c = dry_call(batch, H, W, 64);     // (the state holds block inputs and outputs: no tensor of it depends on the context length or on gn_patch)
  c.cache = &sizing; c.state_bytes = &state;
  return forward_impl(u, c) ? 0 : state + 256;
}

extern "C" int mx_unet_forward_cached(mx_unet* u, void* stream, const void* latents, int io_dtype, const float* timesteps, const void* ehs,
                                      const void* text_embeds, const float* time_ids, void* out, int batch, int H, int W, int ctx_len,
                                      int gn_patch, void* workspace, size_t workspace_bytes, mx_block_cache* cache) {
  const std::string who = "unet_forward_cached";
  MX_CHECK(!cache || cache->dev_down == nullptr, who + ": the device decision (dev_down) serves the patch unit only (mx_unet_forward_cached_mixed)");
  MX_CHECK(cache && cache->predict && cache->state, who + ": cache, cache->predict and cache->state are required");
  MX_CHECK(((uintptr_t)cache->state & 255) == 0, who + ": cache->state must be 256-byte aligned");
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, text_embeds, time_ids, ctx_len, workspace, workspace_bytes);
  c.latents = latents; c.out = out; c.batch = batch; c.H = H; c.W = W; c.gn_patch = gn_patch; c.cache = cache;
  return forward_impl(u, c);
}

/* ---- block-skip cache at the reference's unit, the patch, over a mixed-resolution batch in ONE launch sequence (include/mxdenoise.h) ---- */
extern "C" size_t mx_unet_patch_cache_bytes(const mx_unet* u, int n_slots, int max_h, int max_w, int gn_patch) {
  if (!u || n_slots <= 0 || max_h <= 0 || max_w <= 0 || gn_patch <= 0 || max_h % gn_patch || max_w % gn_patch) { mx::set_error("patch_cache_bytes: bad arguments"); return 0; }
  const mx_unet_group g{nullptr, nullptr, n_slots, max_h, max_w};      // every state row in use by a latent that fills it
  mx_block_cache sizing = mx::sizing_cache(&g, 1);
  size_t state = 0;
  mx::ForwardCall c = dry_call(0, 0, 0, 64);
  c.groups = &g; c.n_groups = 1; c.gn_patch = gn_patch; c.cache = &sizing; c.state_bytes = &state;
  return forward_impl(u, c) ? 0 : state + 256;
}

extern "C" size_t mx_unet_workspace_bytes_cached_mixed(const mx_unet* u, const mx_unet_group* groups, int n_groups, int ctx_len, int gn_patch) {
  if (mx::check_cached_groups("unet_forward_cached_mixed", groups, n_groups)) return 0;
  mx_block_cache sizing = mx::sizing_cache(groups, n_groups);
  size_t peak = 0;
  mx::ForwardCall c = dry_call(0, 0, 0, ctx_len);
  c.groups = groups; c.n_groups = n_groups; c.gn_patch = gn_patch; c.cache = &sizing; c.peak = &peak;
  return forward_impl(u, c) ? 0 : peak + 256;
}

extern "C" int mx_unet_forward_cached_mixed(mx_unet* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                                            const void* ehs, const void* text_embeds, const float* time_ids, int ctx_len, int gn_patch, void* workspace,
                                            size_t workspace_bytes, mx_block_cache* cache) {
  const std::string who = "unet_forward_cached_mixed";
  MX_CHECK(cache && (cache->predict || cache->dev_down) && cache->state && cache->slots && cache->slot_valid,
           who + ": cache with predict (or dev_down), state, slots and slot_valid is required");
  MX_CHECK(((uintptr_t)cache->state & 255) == 0, who + ": cache->state must be 256-byte aligned");
  if (mx::check_cached_groups(who, groups, n_groups)) return 1;
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, text_embeds, time_ids, ctx_len, workspace, workspace_bytes);
  c.groups = groups; c.n_groups = n_groups; c.gn_patch = gn_patch; c.cache = cache;
  return forward_impl(u, c);
}

extern "C" int mx_unet_forward_trace(mx_unet* u, void* stream, const void* latents, int io_dtype, const float* timesteps,
                                     const void* ehs, const void* text_embeds, const float* time_ids, void* out, int batch,
                                     int H, int W, int ctx_len, int gn_patch, void* workspace, size_t workspace_bytes,
                                     const char* stage, void* stage_out, size_t stage_out_bytes) {
  MX_CHECK(stage && stage_out, "unet_forward_trace: stage and stage_out required");
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, text_embeds, time_ids, ctx_len, workspace, workspace_bytes);
  c.latents = latents; c.out = out; c.batch = batch; c.H = H; c.W = W; c.gn_patch = gn_patch;
  c.stage = stage; c.stage_out = stage_out; c.stage_bytes = stage_out_bytes;
  return forward_impl(u, c);
}

/* ---- patch-parallel (BASELINE configs[3]; distrifuser DistriUNetPP, models/distri_sdxl_unet_pp.py:15-216, sync mode) ---- */
extern "C" size_t mx_unet_workspace_bytes_pp(const mx_unet* u, int batch, int H_local, int W, int ctx_len, int world) {
  if (!u) return 0;
  size_t peak = 0;
  const mx_pp_comm comm = sizing_comm(world);
  mx::ForwardCall c = dry_call(batch, H_local, W, ctx_len);
  c.comm = &comm; c.peak = &peak;
  return forward_impl(u, c) ? 0 : peak + 4096;
}

extern "C" int mx_unet_forward_pp(mx_unet* u, void* stream, const void* latents_local, int io_dtype, const float* timesteps, const void* ehs,
                                  const void* text_embeds, const float* time_ids, void* out_local, int batch, int H_local, int W, int ctx_len,
                                  const mx_pp_comm* comm, void* workspace, size_t workspace_bytes) {
  MX_CHECK(comm != nullptr, "unet_forward_pp: null communicator");
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, text_embeds, time_ids, ctx_len, workspace, workspace_bytes);
  c.latents = latents_local; c.out = out_local; c.batch = batch; c.H = H_local; c.W = W; c.comm = comm;
  return forward_impl(u, c);
}

/* stale-asynchronous steps (distrifuser's default after its warm-up: utils.py:180-214 enqueue / handles; modules/pp/conv2d.py:97-117,
 * attn.py:136-146, groupnorm.py:46-66) */
extern "C" size_t mx_unet_pp_state_bytes(const mx_unet* u, int batch, int H_local, int W, int ctx_len, int world) {
  if (!u) return 0;
  size_t need = 0;
  const mx_pp_comm comm = sizing_comm(world);
  mx_pp_stale st{}; st.mode = MX_PP_WARMUP;
  mx::ForwardCall c = dry_call(batch, H_local, W, ctx_len);
  c.comm = &comm; c.stale = &st; c.state_need = &need;
  return forward_impl(u, c) ? 0 : need + 256;
}

extern "C" int mx_unet_forward_pp_stale(mx_unet* u, void* stream, const void* latents_local, int io_dtype, const float* timesteps, const void* ehs,
                                        const void* text_embeds, const float* time_ids, void* out_local, int batch, int H_local, int W,
                                        int ctx_len, const mx_pp_comm* comm, const mx_pp_stale* stale, void* workspace, size_t workspace_bytes) {
  MX_CHECK(comm != nullptr && stale != nullptr, "unet_forward_pp_stale: null communicator / state");
  MX_CHECK(stale->mode == MX_PP_WARMUP || stale->mode == MX_PP_STALE, "unet_forward_pp_stale: mode must be MX_PP_WARMUP or MX_PP_STALE");
  MX_CHECK(stale->state != nullptr && ((uintptr_t)stale->state & 255) == 0, "unet_forward_pp_stale: state must be 256-byte aligned device memory");
  MX_CHECK(stale->mode != MX_PP_STALE || stale->all_gather_async != nullptr, "unet_forward_pp_stale: a stale step needs all_gather_async");
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, text_embeds, time_ids, ctx_len, workspace, workspace_bytes);
  c.latents = latents_local; c.out = out_local; c.batch = batch; c.H = H_local; c.W = W; c.comm = comm; c.stale = stale;
  return forward_impl(u, c);
}

/* host-only walk of the patch-parallel plan that calls comm->all_gather for every exchange of one forward, in order, with
 * send / recv = 0x1000 + the byte offset the region will have inside the workspace (no launches, no GPU): what a caller needs to
 * pre-register buffers, and what tests/test_pp_gloo.py replays over gloo to check the bookkeeping */
extern "C" int mx_unet_pp_comm_plan(const mx_unet* u, int batch, int H_local, int W, int ctx_len, const mx_pp_comm* comm) {
  MX_CHECK(u && comm && comm->all_gather, "unet_pp_comm_plan: bad arguments");
  mx::ForwardCall c = dry_call(batch, H_local, W, ctx_len);
  c.comm = comm;
  return forward_impl(u, c);
}
