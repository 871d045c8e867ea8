// Step plan of the SD3.5 MMDiT in the sduss ``transformer`` slot: a flat launch sequence on one HIP stream over
// token-major bf16 activations in a caller-provided workspace.
//
// Replaces PatchSD3Transformer2DModel.forward (sduss/model_executor/modules/SD3Transformer.py:60-262) and the blocks it
// drives (PatchJointTransformerBlock modules/transformer.py:299-388, PatchSD3Attention modules/attention.py:241-424).
// With the block cache off the reference's sliced branch only re-chunks and regroups the token axis, so one plan serves
// is_sliced True and False (oracle/sd3_mmdit_ref.py).
// MI355X-first choices:
//   * every AdaLN projection of the step (24 x norm1 / norm1_context + norm_out, 325 d columns) is ONE GEMM on
//     silu(temb); LayerNorm-modulate kernels and GEMM epilogues (gated residual) read their fp32 rows from it;
//   * image and text tokens share one joint Q|K buffer, one V^T buffer and one O buffer per step: the two QKV GEMMs
//     write their rows straight into the joint sequence (row remap in the epilogue, V transposed), so the joint
//     attention of attention.py:347-350 is a single kernel launch with no torch.cat; to_out / to_add_out read their
//     token ranges back through the loader's row remap;
//   * PatchEmbed's 2x2 stride-2 conv is an im2col + GEMM whose epilogue adds bias and the cropped positional table.
// Host scaffold (arena, weight lookup, groups, block-cache bookkeeping, the forward driver): plan_base.h; this file holds the MMDiT's own plan,
// its checks and hooks (struct Model) and the extern "C" entry points, each of which describes its forward as an mx::ForwardCall.
// One plan serves every mode (exact, mixed-resolution, patch-parallel, the per-sample and the chunk-unit block cache) and states each rule once:
//   * Seq joint, image + Plan::place() -- where a group's rows lie in the streams, the joint sequence and V^T; every grouped operand comes from it;
//   * linear(Linear{...}) -- required fields in order, the rest by name (.epilogue .plus .gated .rows .from .only); qkv() beside it;
//   * attend()  -- the attention of a sequence set in the mode's form (one problem, per group, per active group, local queries x gathered keys);
//   * project() -- how an attention projection's result reaches its stream (gated epilogue; chunk cache: materialise, state, gated copy);
//   * the layer loop -- one block body between what brackets it (nothing; decide / after around a muted walk; pcm_open and the output stores).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mxdenoise.h"
#include "common.h"
#include "graph_cache.h"
#include "patch_cache.h"
#include "plan_base.h"

namespace mx {
int launch_patchify(hipStream_t s, const void* in, int dtype, void* out, int B, int C, int H, int W, int ps);
int launch_unpatchify(hipStream_t s, const void* in, void* out, int dtype, int B, int C, int H, int W, int ps, int ld);
int launch_crop_pos(hipStream_t s, const void* table, void* out, int m, int h, int w, int d);
int launch_sinus_embed(hipStream_t s, const float* t, void* out, int B, int dim);
int launch_sq_diff_partial(hipStream_t s, const void* a, const void* b, long elems_per_sample, int B, double* partial, const int* slot = nullptr);
}  // namespace mx

using mx::bf16_t;

struct mx_mmdit {
  mx_mmdit_config cfg;
  mx::WeightTable weights;
  mx::GraphCache graphs;   // hipGraph replay of the forward, keyed by its arguments (graph_cache.h)
  mx::PinnedBuf skip_pin;  // the per-block read-back of the device-side skip decision (mx_block_cache.dev_down)
  std::map<std::vector<long>, std::vector<size_t>> pp_sizes;   // recorded exchange sizes of the patch-parallel plan per shape (as in unet_sdxl.cpp)
};

namespace {

// V^T rows padded to whole 128-byte lines: with the minimal MX_VT_LD(4429) = 4432 every 64-key tile row straddles two lines and the
// joint attention ran at 850 TFLOP/s against 1000 at an aligned length (tools/exp/attn_shapes_probe.py)
int vt_ld(int keys) { return (MX_VT_LD(keys) + 63) / 64 * 64; }

// The stream the rows of a launch belong to: the image tokens (L_g rows per sample of group g) or the text tokens (Lt rows per sample everywhere)
enum Stream { kNoStream, kImage, kText };

// One attention site's q|k, V^T and O buffers and how the sequences lie in them: the samples of group g one after the other from row row0[g]
// (q|k, O) / element vt0[g] (V^T), each len[g] = image tokens + `tail` rows long.  tail = Lt: the joint sequence [image ; text]; 0: attn2's
// image tokens alone -- which is also the layout of the image STREAM's tensors (first row and rows per sample of a group).
struct Seq {
  int tail = 0;
  int len[MX_MAX_SEGS], ldvt[MX_MAX_SEGS];
  long row0[MX_MAX_SEGS], vt0[MX_MAX_SEGS];
  long rows = 0, vt_elems = 0;
  bf16_t *qk = nullptr, *vt = nullptr, *o = nullptr;
  void lay(const mx::Groups& G, int ps, int d, int tail_rows) {
    tail = tail_rows; rows = 0; vt_elems = 0;
    for (int g = 0; g < G.ng; ++g) {
      len[g] = (G.gH[g] / ps) * (G.gW[g] / ps) + tail; ldvt[g] = vt_ld(len[g]);
      row0[g] = rows; vt0[g] = vt_elems;
      rows += (long)G.gB[g] * len[g]; vt_elems += (long)G.gB[g] * d * ldvt[g];
    }
  }
};

// ---- the arguments of Plan::linear() by name: a call states the required fields in order and adds what else it means ----
struct Linear {
  const void* a; int lda; std::string stem; void* c; int ldc; int M, N, K;        // c[M, N] = a[M, K] * "<stem>.weight"^T + "<stem>.bias"
  int flags = 0; const void* residual = nullptr; int ldr = 0; const float* gate = nullptr; int ldg = 0;
  Stream stream = kNoStream; const Seq* a_seq = nullptr; const bool* act = nullptr;
  Linear& epilogue(int f) { flags = f; return *this; }
  Linear& plus(const void* r, int ld) { residual = r; ldr = ld; return *this; }
  Linear& gated(const float* g, int ld) { gate = g; ldg = ld; return *this; }      // c = residual + gate[sample] * (...): one fp32 row per sample
  // a, c, the residual are per-row tensors of stream s and the gate is per sample: yields rows_per_batch and, in a mixed batch, the groups' problems
  Linear& rows(Stream s) { stream = s; return *this; }
  // a is the O buffer of sequence set q: the launch reads the stream's rows out of every sample's sequence (the loader's row remap)
  Linear& from(const Seq& q) { a_seq = &q; return *this; }
  Linear& only(const bool* groups) { act = groups; return *this; }                // cached mixed batch: the problems of these groups only
};

struct Plan : mx::DenoiserPlan {      // (stream, arena, weights, groups, exchange, block-cache bookkeeping: plan_base.h)
  mx_mmdit* u;
  int Lt;
  // Mixed-resolution batch (mx_mmdit_forward_mixed): the requests of every resolution present in ONE launch sequence.  A group = the samples of
  // one resolution.  The image stream is the groups' token rows one after the other, the text stream is per sample (same length everywhere);
  // the joint q|k / V^T / O buffers hold each group's [image ; text] sequences at its own length.  Per-token ops are single launches; the ops
  // with per-sample structure -- AdaLN modulation, the q|k|v projections into the joint buffers, attention, the gated projections reading the
  // joint sequence back -- are GROUPED launches (mx_gemm_seg, mx_attention_prescaled_grouped, mx_layernorm_mod_grouped).  The reference
  // re-chunks the tokens of all resolutions into one batch (modules/utils.py:86-122) and regroups them per latent before attention
  // (attention.py:300-372).
  // WHERE A GROUP'S ROWS LIE is stated here once (laid out at the top of run()): every operand of every grouped launch is derived from it.
  Seq joint, image;
  long row0(Stream s, int g) const { return s == kImage ? image.row0[g] : (long)gb0[g] * Lt; }      // first row of group g in the stream's tensors
  int rpb(Stream s, int g) const { return s == kImage ? image.len[g] : Lt; }                         // rows per sample
  int rows(Stream s) const { return s == kImage ? (int)image.rows : B * Lt; }
  // Group g's operands of launch d on the rows of stream s, into q: a problem of the grouped launch, or d itself (g = 0: the descriptor
  // describes the first group).  from: A is that sequence set's O buffer; into: C is its q|k buffer, with its V^T.
  template <class Q> void place(Q& q, const mx_gemm_desc& d, Stream s, const Seq* from, const Seq* into, int g) const {
    const long r = row0(s, g);
    const int off = s == kImage ? 0 : image.len[g];            // the stream's first row inside a joint sequence
    q.rows_per_batch = rpb(s, g);
    q.a = (const bf16_t*)d.a + (from ? from->row0[g] : r) * d.lda;
    if (from && from->tail) { q.a_batch_rows = from->len[g]; q.a_row_off = off; }
    q.c = (bf16_t*)d.c + (into ? into->row0[g] : r) * d.ldc;
    if (into) { q.vt = into->vt + into->vt0[g]; q.ldvt = into->ldvt[g]; }
    if (into && into->tail) { q.c_batch_rows = into->len[g]; q.c_row_off = off; }
    if (d.residual) q.residual = (const bf16_t*)d.residual + r * d.ldr;
    if (d.gate) q.gate = d.gate + (long)gb0[g] * d.ldg;
  }
  mx_gemm_seg seg_buf[MX_MAX_SEGS];
  // act: the grouped launch covers these resolution groups only (nullptr: all).  The text stream has one length everywhere: its launches are
  // grouped only where they meet the joint sequence.
  void attach(mx_gemm_desc& d, Stream s, const Seq* from, const Seq* into, const bool* act) {
    if (s == kNoStream) return;
    place(d, d, s, from, into, 0);
    if (ng <= 1 || (s == kText && !from && !into)) return;
    std::memset(seg_buf, 0, sizeof(seg_buf));
    int n = 0;
    for (int g = 0; g < ng; ++g) if (!act || act[g]) { mx_gemm_seg& q = seg_buf[n++]; place(q, d, s, from, into, g); q.M = gB[g] * q.rows_per_batch; }
    d.segs = seg_buf; d.n_segs = n;
  }
  // patch parallelism (mx_mmdit_forward_pp; distrifuser models/distri_sd3_transformer_pp.py:87-97, modules/pp/attn.py:202-277): this rank owns
  // the image tokens of H (local) latent rows; the text stream is computed by every rank; K / V^T of the image tokens are all-gathered
  bool is_pp() const { return px.world > 1; }
  bool all_gather(const void* send, void* recv, size_t bytes_per_rank) {
    if (!ok()) return false;
    if (const char* e = px.all_gather(stream, dry, send, recv, bytes_per_rank)) return fail(e);
    return true;
  }
  bool copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height) {
    if (!ok()) return false;
    if (quiet()) return true;
    if (hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, stream) != hipSuccess) return fail("patch-parallel: K / V assembly copy failed");
    return true;
  }
  // ---- the cache at the reference's unit over a mixed batch in ONE launch sequence (mx_mmdit_forward_cached_mixed) ----
  // The unit is the token CHUNK: every latent is cut into (res // patch)^2 equal token ranges keyed "<request id>-<k>" (modules/utils.py:86-122).
  // Per joint block ONE decision for the chunks of all samples of all groups (get_sd3_mask, cache_manager.py:163-191); a block none of whose
  // chunks asks takes both streams from the state; in a running block everything runs on all tokens except the attention: a resolution group
  // with no asking chunk skips it and takes attn.output / attn.encoder_output's cached results, a group with any asking chunk computes it whole
  // (attention.py:296-372; attn2 of the dual blocks: asking ratio <= 1/16 -> only the asking chunks are renewed, :303-325).
  bool pcm = false;
  int pcm_patch = 0, pcm_slots = 0, pcm_maxh = 0, pcm_maxw = 0, pcm_nc = 0;
  std::vector<mx::PcSample> pcm_img, pcm_ctx;
  std::vector<mx::PcRange> pcm_chunks;
  std::vector<int> pcm_chunk_b, pcm_chunk_g;
  mx::PcSample* pcm_dimg = nullptr; mx::PcSample* pcm_dctx = nullptr; mx::PcRange* pcm_dchunks = nullptr; mx::PcRange* pcm_dtmp = nullptr; double* pcm_dpart = nullptr;
  unsigned long long pcm_asked = 0, pcm_total = 0;
  // host copies of the range tables sent by hipMemcpyAsync: kept until the forward's final synchronisation (a pageable source must outlive the copy)
  std::deque<std::vector<mx::PcRange>> pcm_sent;
  ~Plan() { if (!pcm_sent.empty() && !dry) (void)hipStreamSynchronize(stream); }     // (an early error return: the copies may still be reading)
  size_t pcm_ncmax() const { return (size_t)pcm_slots * (pcm_maxh / pcm_patch) * (pcm_maxw / pcm_patch); }
  size_t pcm_head_bytes() const {
    const size_t nc = pcm_ncmax();
    return ((nc * 64 * sizeof(double) + 2 * (size_t)pcm_slots * sizeof(mx::PcSample) + 4 * nc * sizeof(mx::PcRange)) + 255) & ~(size_t)255;
  }
  // the state's base: the caller's buffer, or in a sizing walk a placeholder that is only counted from
  char* pcm_base() const { return dry ? (char*)(uintptr_t)0x1000 : (char*)bc->state; }
  size_t bc_bytes = 0;             // state bytes the plan needs (also the dry answer of mx_mmdit_block_cache_bytes)
  unsigned long long blocks_run = 0;
  static constexpr int kBcPartRows = 1, kBcTables = 1;     // head of the state: one row of partial sums, the slot table
  static size_t bc_scratch_bytes(int rows) { return bc_head_bytes(kBcPartRows, kBcTables, rows); }

  // C = A W^T + bias with the optional fused pieces
  bool linear(const Linear& l) {
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.a = l.a; d.lda = l.lda; d.w = wb(l.stem + ".weight", (size_t)l.N * l.K); d.bias = wf(l.stem + ".bias", l.N);
    d.c = l.c; d.ldc = l.ldc; d.M = l.M; d.N = l.N; d.K = l.K; d.flags = l.flags; d.residual = l.residual; d.ldr = l.ldr; d.gate = l.gate; d.ldg = l.ldg;
    attach(d, l.stream, l.a_seq, nullptr, l.act);
    return gemm(d);
  }
  // fused q|k|v projection "<stem>" of stream s's tokens into their rows of sequence set `into` (q|k interleaved, V transposed); the epilogue
  // RMS-normalises every q / k head ("<norm>q.weight", "<norm>k.weight"; attention.py:332-346, 377-388) and scales q for mx_attention_prescaled
  bool qkv(const bf16_t* a, Stream s, const std::string& stem, const std::string& norm, const Seq& into) {
    const int d_model = u->cfg.num_attention_heads * 64;
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.a = a; d.lda = d_model; d.w = wb(stem + ".weight", (size_t)3 * d_model * d_model); d.bias = wf(stem + ".bias", 3 * d_model);
    d.c = into.qk; d.ldc = 2 * d_model; d.M = rows(s); d.N = 3 * d_model; d.K = d_model; d.flags = MX_EPI_QKV | MX_EPI_RMSNORM; d.seg = d_model; d.period = 3;
    d.rms_wq = wf(norm + "q.weight", 64); d.rms_wk = wf(norm + "k.weight", 64); d.rms_eps = u->cfg.norm_eps; d.out_scale = MX_ATTN_QSCALE(0.125f);
    attach(d, s, nullptr, &into, nullptr);
    return gemm(d);
  }
  // LayerNorm + modulation of stream s by per-sample fp32 rows (row stride ldmod); y2: the second modulation of the same normalised rows
  bool lnmod(Stream s, const bf16_t* x, bf16_t* y, bf16_t* y2, const float* scale, const float* shift, const float* scale2, const float* shift2, int ldmod) {
    if (!ok()) return false;
    if (quiet()) return true;
    const int C = u->cfg.num_attention_heads * 64;
    if (s == kImage && ng > 1
          ? mx_layernorm_mod_grouped(stream, x, y, y2, scale, shift, scale2, shift2, ldmod, C, u->cfg.norm_eps, gB, image.len, ng)
          : mx_layernorm_mod(stream, x, y, y2, scale, shift, scale2, shift2, ldmod, rows(s), C, rpb(s, 0), u->cfg.norm_eps))
      return fail(std::string("layernorm_mod: ") + mx_last_error());
    return true;
  }
  bool run(const void* latents, int io_dtype, const float* timesteps, const void* ehs, const void* pooled, void* outp) {
    const mx_mmdit_config& c = u->cfg;
    const int d = c.num_attention_heads * 64;
    const int heads = c.num_attention_heads;
    const int ps = c.patch_size;
    const int h = H / ps, wd = W / ps;
    const int L = h * wd;
    const int Kp = ps * ps * c.in_channels;
    joint.lay(*this, ps, d, Lt);
    image.lay(*this, ps, d, 0);
    if (ng > 1 && (is_pp() || (bc && !pcm))) return fail("mmdit: a mixed-resolution batch runs neither patch-parallel nor through the per-sample block cache");
    const int MI = rows(kImage), MT = rows(kText);
    // patch-parallel: L counts this rank's image tokens; the keys of the joint attention are all ranks' image tokens, then the text tokens
    const int world = px.world;
    const int Ltot = L * world;
    if (is_pp() && L % 16 != 0) return fail("mmdit pp: local image tokens must be a multiple of 16 (V^T key order, MX_VT_POS)");
    if (is_pp() && bc) return fail("mmdit pp: not combined with the block-skip cache");

    // ---- AdaLN column layout of the one projection GEMM ----
    std::vector<int> off_img(c.num_layers), off_ctx(c.num_layers);
    int ntot = 0;
    for (int i = 0; i < c.num_layers; ++i) {
      const bool dual = c.dual_attention[i] != 0, last = i == c.num_layers - 1;
      off_img[i] = ntot; ntot += (dual ? 9 : 6) * d;
      off_ctx[i] = ntot; ntot += (last ? 2 : 6) * d;
    }
    const int off_out = ntot; ntot += 2 * d;

    // ---- conditioning (SD3Transformer.py:81): temb = timestep_embedder(sinusoid(t)) + text_embedder(pooled) ----
    bf16_t* tsin = alloc<bf16_t>((size_t)B * 256);
    if (ok() && !dry && mx::launch_sinus_embed(stream, timesteps, tsin, B, 256)) fail(mx_last_error());
    bf16_t* t1 = alloc<bf16_t>((size_t)B * d); bf16_t* t2 = alloc<bf16_t>((size_t)B * d);
    bf16_t* p1 = alloc<bf16_t>((size_t)B * d); bf16_t* semb = alloc<bf16_t>((size_t)B * d);
    linear(Linear{tsin, 256, "time_text_embed.timestep_embedder.linear_1", t1, d, B, d, 256}.epilogue(MX_EPI_SILU));
    linear(Linear{t1, d, "time_text_embed.timestep_embedder.linear_2", t2, d, B, d, d});
    linear(Linear{pooled, c.pooled_projection_dim, "time_text_embed.text_embedder.linear_1", p1, d, B, d, c.pooled_projection_dim}.epilogue(MX_EPI_SILU));
    // silu(temb): every consumer of temb applies SiLU first (AdaLayerNormZero / ZeroX / Continuous)
    linear(Linear{p1, d, "time_text_embed.text_embedder.linear_2", semb, d, B, d, d}.epilogue(MX_EPI_SILU).plus(t2, d));
    float* mod = alloc<float>((size_t)B * ntot);
    linear(Linear{semb, d, "adaln_all", mod, ntot, B, ntot, d}.epilogue(MX_EPI_OUT_F32));

    // ---- PatchEmbed + positional table (:82-83), context_embedder (:115) ----
    bf16_t* patches = alloc<bf16_t>((size_t)MI * Kp);
    for (int g = 0; g < ng && ok() && !dry; ++g)
      if (mx::launch_patchify(stream, g_lat[g], io_dtype, patches + image.row0[g] * Kp, gB[g], c.in_channels, gH[g], gW[g], ps)) fail(mx_last_error());
    // One centre crop of the table per group, [L_g, d] at the group's first row.  Patch-parallel: the crop is taken for the WHOLE grid
    // (distri_sd3_transformer_pp.py:87 embeds before it slices) and this rank reads its rows.
    bf16_t* pos = alloc<bf16_t>(ng > 1 ? (size_t)MI * d : (size_t)Ltot * d);
    const bf16_t* table = wb("pos_embed.table", (size_t)c.pos_embed_max_size * c.pos_embed_max_size * d);
    for (int g = 0; g < ng && ok(); ++g) {
      const int gh = gH[g] / ps * world, gw = gW[g] / ps;
      if (gh > c.pos_embed_max_size || (ng > 1 && gw > c.pos_embed_max_size)) return fail("mmdit: latent larger than the positional table");   // (one group: its width is the entry point's check)
      if (!dry && mx::launch_crop_pos(stream, table, pos + image.row0[g] * d, c.pos_embed_max_size, gh, gw, d)) fail(mx_last_error());
    }
    if (pos) pos += (size_t)px.rank * L * d;
    bf16_t* x = alloc<bf16_t>((size_t)MI * d);
    linear(Linear{patches, Kp, "pos_embed.proj", x, d, MI, d, Kp}.epilogue(MX_EPI_RES_BCAST).plus(pos, d).rows(kImage));
    bf16_t* ctx = alloc<bf16_t>((size_t)MT * d);
    linear(Linear{ehs, c.joint_attention_dim, "context_embedder", ctx, d, MT, d, c.joint_attention_dim});
    dump("embed", x, (size_t)MI * d);
    dump("context_embed", ctx, (size_t)MT * d);

    // ---- per-step buffers reused by every block ----
    bf16_t* xin = alloc<bf16_t>((size_t)MI * d);
    bf16_t* x2in = alloc<bf16_t>((size_t)MI * d);
    bf16_t* cin = alloc<bf16_t>((size_t)MT * d);
    joint.qk = alloc<bf16_t>((size_t)joint.rows * 2 * d);
    joint.vt = alloc<bf16_t>((size_t)joint.vt_elems);
    joint.o = alloc<bf16_t>((size_t)joint.rows * d);
    image.qk = alloc<bf16_t>((size_t)MI * 2 * d);
    image.vt = alloc<bf16_t>((size_t)image.vt_elems);
    image.o = alloc<bf16_t>((size_t)MI * d);
    bf16_t* ff = alloc<bf16_t>((size_t)MI * 4 * d);
    bf16_t* ffc = alloc<bf16_t>((size_t)MT * 4 * d);
    bf16_t* pcm_ti = pcm ? alloc<bf16_t>((size_t)MI * d) : nullptr;          // cached mixed batch: to_out / to_add_out results before the gate
    bf16_t* pcm_tc = pcm ? alloc<bf16_t>((size_t)MT * d) : nullptr;
    char* pcm_top = pcm ? pcm_base() + pcm_head_bytes() : nullptr;
    // patch-parallel: only the image tokens' K rows and V^T columns travel (what distrifuser gathers, modules/pp/attn.py:222-233): they are packed
    // into contiguous send buffers first -- the QKV epilogue writes q|k interleaved and V^T rows padded, with the text tokens behind the image ones
    bf16_t *k_send = nullptr, *v_send = nullptr, *k_g = nullptr, *v_g = nullptr, *k_all = nullptr, *vt_all = nullptr;
    if (is_pp()) {
      k_send = alloc<bf16_t>((size_t)B * L * d);
      v_send = alloc<bf16_t>((size_t)B * d * L);
      k_g = alloc<bf16_t>((size_t)world * B * L * d);
      v_g = alloc<bf16_t>((size_t)world * B * d * L);
      k_all = alloc<bf16_t>((size_t)B * (Ltot + Lt) * d);
      vt_all = alloc<bf16_t>((size_t)B * d * vt_ld(Ltot + Lt));
    }
    // keys of a patch-parallel attention per sample: every rank's `L` image tokens in rank order, then the `tail` local-only (text) tokens:
    // k_all [B][world * L + tail][d], vt_all [B][d][ld_all]
    auto gather_kv = [&](const Seq& s, int ld_all) {
      const int tail = s.tail, ld_loc = s.ldvt[0];
      const int rows_loc = L + tail, rows_all = Ltot + tail;
      const size_t krow = (size_t)d * 2, qrow = 2 * krow;
      for (int b = 0; b < B && ok(); ++b)               // K half of this sample's image rows
        copy2d((char*)k_send + (size_t)b * L * krow, krow, (char*)s.qk + (size_t)b * rows_loc * qrow + krow, qrow, krow, L);
      copy2d(v_send, (size_t)L * 2, s.vt, (size_t)ld_loc * 2, (size_t)L * 2, (size_t)B * d);
      all_gather(k_send, k_g, (size_t)B * L * krow);
      all_gather(v_send, v_g, (size_t)B * d * L * 2);
      for (int r = 0; r < world && ok(); ++r) {
        copy2d((char*)k_all + (size_t)r * L * krow, rows_all * krow, (char*)k_g + (size_t)r * B * L * krow, L * krow, L * krow, B);
        copy2d((char*)vt_all + (size_t)r * L * 2, (size_t)ld_all * 2, (char*)v_g + (size_t)r * B * d * L * 2, (size_t)L * 2, (size_t)L * 2, (size_t)B * d);
      }
      if (tail) {
        for (int b = 0; b < B && ok(); ++b)
          copy2d((char*)k_all + ((size_t)b * rows_all + Ltot) * krow, krow, (char*)s.qk + ((size_t)b * rows_loc + L) * qrow + krow, qrow, krow, tail);
        copy2d((char*)vt_all + (size_t)Ltot * 2, (size_t)ld_all * 2, (char*)s.vt + (size_t)L * 2, (size_t)ld_loc * 2, (size_t)MX_VT_LD(tail) * 2,
               (size_t)B * d);
      }
    };
    // THE ATTENTION of one sequence set (the joint one, attn2's), in the form the mode asks for: patch-parallel -- local queries against the
    // gathered keys; a mixed batch -- one problem per group; the chunk cache -- one problem per ACTIVE group (act); otherwise one problem.
    // q carries MX_ATTN_QSCALE(1/8) from the QKV epilogue (RMSNorm + out_scale).
    auto attend = [&](const Seq& s, const bool* act) {
      const int Lk = Ltot + s.tail, ld_all = vt_ld(Lk);
      if (is_pp()) gather_kv(s, ld_all);
      if (!ok() || quiet()) return;
      int rc = 0;
      if (is_pp()) {
        rc = mx_attention_prescaled(stream, s.qk, 2 * d, k_all, d, vt_all, ld_all, (int64_t)d * ld_all, s.o, d, B, heads, s.len[0], Lk);
      } else if (ng > 1 || act) {
        mx_attn_problem pr[MX_MAX_SEGS];
        int n = 0;
        for (int g = 0; g < ng; ++g) if (!act || act[g]) {
          pr[n].q = s.qk + s.row0[g] * 2 * d; pr[n].k = s.qk + s.row0[g] * 2 * d + d; pr[n].vt = s.vt + s.vt0[g]; pr[n].o = s.o + s.row0[g] * d;
          pr[n].vt_batch_stride = (int64_t)d * s.ldvt[g]; pr[n].B = gB[g]; pr[n].Lq = s.len[g]; pr[n].Lk = s.len[g]; pr[n].ldvt = s.ldvt[g];
          ++n;
        }
        if (n) rc = mx_attention_prescaled_grouped(stream, pr, n, 2 * d, 2 * d, d, heads);
      } else {
        rc = mx_attention_prescaled(stream, s.qk, 2 * d, s.qk + d, 2 * d, s.vt, s.ldvt[0], (int64_t)d * s.ldvt[0], s.o, d, B, heads, s.len[0], s.len[0]);
      }
      if (rc) fail(std::string("attention: ") + mx_last_error());
    };

    // Block-skip cache (mx_mmdit_forward_cached; the reference's per-block CacheManagers, SD3Transformer.py:54-57,151,172,219-228): a block
    // runs when any sample asks (state_mask.sum() > 0), otherwise the image and context streams take the values the block produced last
    // time.  State per block: [input x | output x | output context], each 256-byte aligned, after the comparison scratch.
    if (bc && bc_rows < B) bc_rows = B;
    const size_t bc_x = ((size_t)bc_rows * L * d * 2 + 255) & ~(size_t)255, bc_c = ((size_t)bc_rows * Lt * d * 2 + 255) & ~(size_t)255;
    const size_t bc_scratch = bc_scratch_bytes(bc_rows);
    if (bc) {
      bc_bytes = bc_scratch + (size_t)c.num_layers * (2 * bc_x + bc_c);
      if (!dry && bc_bytes > bc->state_bytes) fail("block cache: state buffer too small (mx_mmdit_block_cache_bytes)");
    }
    // how far x is from a state tensor, per sample: the head of the state is the comparison scratch
    auto x_moved = [&](const char* st, float* mse, const char* msg) {
      if (mx::launch_sq_diff_partial(stream, x, st, (long)L * d, B, (double*)bc->state, bc_dslot)) return fail(mx_last_error());
      return bc_read_mse((double*)bc->state, B, 64, mse, msg, [&](size_t s) { return MseRow{(int)s, (double)L * d, s}; });
    };
    // decides block i; false = reuse.  Leaves the latest input in the cache (cache_manager.py:183)
    auto decide = [&](int i) -> bool {
      char* st = (char*)bc->state + bc_scratch + (size_t)i * (2 * bc_x + bc_c);
      std::vector<float> mse(B, MX_MSE_UNCACHED);
      if (bc_any_valid && !x_moved(st, mse.data(), "block cache: reading the input differences failed")) return true;
      std::vector<unsigned char> run(B, 1);
      if (bc->predict(bc->ctx, i, 0, B, 1, h_timesteps.data(), mse.data(), run.data())) { fail("block cache: the predictor failed"); return true; }
      bool any = !bc_all_valid;
      for (int s = 0; s < B; ++s) any = any || run[s] != 0;
      bc_store(st, x, (size_t)L * d * 2);
      return any;
    };
    auto after = [&](int i, bool ran, bool last) {
      char* st = (char*)bc->state + bc_scratch + (size_t)i * (2 * bc_x + bc_c);
      if (ran && bc_all_valid && bc->observe) {              // how far the block's image-stream output moved since its last run (fitting labels)
        std::vector<float> om(B);
        if (!x_moved(st + bc_x, om.data(), "block cache: reading the output differences failed")) return;
        bc->observe(bc->ctx, i, B, om.data());
      }
      bool okc = ran ? bc_store(st + bc_x, x, (size_t)L * d * 2) : bc_load(x, st + bc_x, (size_t)L * d * 2);
      if (okc && !last) okc = ran ? bc_store(st + 2 * bc_x, ctx, (size_t)Lt * d * 2) : bc_load(ctx, st + 2 * bc_x, (size_t)Lt * d * 2);
      if (ran) blocks_run |= 1ull << i;
    };

    // ---- the chunk-unit cache's view of the current block (pcm) ----
    const long row_i = pcm ? (long)(pcm_maxh / ps) * (pcm_maxw / ps) * d : 0, row_c = (long)Lt * d;      // elements of a state row, per stream
    long maxL = 0; for (int g = 0; g < ng; ++g) maxL = std::max<long>(maxL, image.len[g]);
    struct {
      char *in, *out, *octx, *a, *ae, *a2;                   // state regions: block input, outputs of both streams, attn / attn context / attn2 results
      std::vector<unsigned char> run;                        // per chunk: asks
      bool gany[MX_MAX_SEGS]; int gask[MX_MAX_SEGS], gtot[MX_MAX_SEGS];        // per group: any chunk asks; asking chunks; chunks
      std::vector<mx::PcRange> act_img, act_ctx;             // rows of the samples of the active groups, per stream
      const mx::PcRange *d_act_img, *d_act_ctx;
    } cb{};
    // a stream's tensor <-> a state region, sample by sample (to_batch) with the optional gated add: t = res + vec[sample] * state
    auto state_copy = [&](Stream s, void* t, char* reg, int to_batch, const float* vec, const void* res, int gate) {
      const bool img = s == kImage;
      if (ok() && mx::launch_pc_image_copy(stream, t, reg, img ? (void*)pcm_dimg : (void*)pcm_dctx, B, 0, d, img ? row_i : row_c, to_batch, vec, ntot, res,
                                           img ? maxL * d : row_c, gate)) fail(mx_last_error());
    };
    // a range table of the running block to the device (slot: which of the scratch tables)
    auto upload = [&](const std::vector<mx::PcRange>& v, int slot) -> const mx::PcRange* {
      mx::PcRange* dst = pcm_dtmp + (size_t)slot * pcm_ncmax();
      if (!ok() || v.empty()) return dst;
      pcm_sent.push_back(v);                // (the copy is asynchronous from pageable memory: the table must outlive the block that built it)
      if (hipMemcpyAsync(dst, pcm_sent.back().data(), v.size() * sizeof(mx::PcRange), hipMemcpyHostToDevice, stream) != hipSuccess)
        fail("mmdit patch cache: sending a range table failed");
      return dst;
    };
    // Opens block i of the chunk cache: carves its state regions (the sizing walk stops here), decides per chunk, stores the input and, when no
    // chunk asks, takes both streams from the state.  true: the block runs.
    auto pcm_open = [&](int i, bool dual, bool last) -> bool {
      auto region = [&](long row_elems) { char* r = pcm_top; pcm_top += ((size_t)row_elems * pcm_slots * 2 + 255) & ~(size_t)255; return r; };
      cb.in = region(row_i); cb.out = region(row_i); cb.octx = last ? nullptr : region(row_c);
      cb.a = region(row_i); cb.ae = last ? nullptr : region(row_c); cb.a2 = dual ? region(row_i) : nullptr;
      if (dry) return false;
      if ((size_t)(pcm_top - (char*)bc->state) > bc->state_bytes) return fail("mmdit patch cache: state buffer too small (mx_mmdit_patch_cache_bytes)");
      const int NC = pcm_nc;
      if (bc_any_valid && mx::launch_pc_range_sq_diff(stream, x, cb.in, row_i, d, pcm_dchunks, NC, pcm_dpart)) return fail(mx_last_error());
      cb.run.assign(NC, 1);
      for (int g = 0; g < MX_MAX_SEGS; ++g) { cb.gask[g] = 0; cb.gtot[g] = 0; }
      // THE DECISION -- the one place the two modes differ: it leaves run[], gask[] and gtot[]
      if (bc_dev) {
        // on the device (mx_block_cache.dev_down): one launch, one record read back (patch_cache.hip pc_decide_kernel; skip_decide.h)
        mx_skip_decide_args a{};
        a.forest = bc->dev_down; a.n_in = 1; a.kind = 1; a.units = pcm_dchunks; a.unit_sample = bc_skip.unit_sample; a.partial = pcm_dpart;
        a.part_len[0] = 64; a.part_elems[0] = (double)d;
        const unsigned char* flags = nullptr;
        const int32_t* rec = bc_dev_decide(a, i, true, &flags);
        if (!rec) return false;
        cb.run.assign(flags, flags + NC);
        for (int g = 0; g < MX_MAX_SEGS; ++g) { cb.gask[g] = rec[MX_SKIP_REC_GASK + g]; cb.gtot[g] = rec[MX_SKIP_REC_GTOT + g]; }
      } else {
        // on the host: the partial sums come back and the caller's predictor answers
        std::vector<float> mse(NC, MX_MSE_UNCACHED);
        if (bc_any_valid && !bc_read_mse(pcm_dpart, NC, 64, mse.data(), "mmdit patch cache: reading the input differences failed",
                                         [&](size_t j) { return MseRow{pcm_chunk_b[j], (double)pcm_chunks[j].rows * d, j}; })) return false;
        std::vector<float> tpp(NC);
        for (int j = 0; j < NC; ++j) tpp[j] = h_timesteps[pcm_chunk_b[j]];
        if (bc->predict(bc->ctx, i, 0, NC, 1, tpp.data(), mse.data(), cb.run.data())) return fail("mmdit patch cache: the predictor failed");
        for (int j = 0; j < NC; ++j) {
          if (!bc_valid[pcm_chunk_b[j]]) cb.run[j] = 1;
          ++cb.gtot[pcm_chunk_g[j]];
          if (cb.run[j]) ++cb.gask[pcm_chunk_g[j]];
        }
      }
      bool any = false;
      for (int g = 0; g < MX_MAX_SEGS; ++g) { cb.gany[g] = cb.gask[g] > 0; any = any || cb.gany[g]; pcm_asked += cb.gask[g]; pcm_total += cb.gtot[g]; }
      state_copy(kImage, x, cb.in, 0, nullptr, nullptr, 0);                  // the cached input is always the latest one (cache_manager.py:183)
      if (!any) {                                                             // SD3Transformer.py:219-228: both streams from the block's caches
        state_copy(kImage, x, cb.out, 1, nullptr, nullptr, 0);
        if (!last) state_copy(kText, ctx, cb.octx, 1, nullptr, nullptr, 0);
        return false;
      }
      blocks_run |= 1ull << i;
      cb.act_img.clear(); cb.act_ctx.clear();
      for (int g = 0; g < ng; ++g) if (cb.gany[g]) for (int k = 0; k < gB[g]; ++k) {
        const int bb = gb0[g] + k;
        cb.act_img.push_back(mx::PcRange{pcm_img[bb].row0, image.len[g], pcm_img[bb].slot, 0});
        cb.act_ctx.push_back(mx::PcRange{(long long)bb * Lt, Lt, pcm_img[bb].slot, 0});
      }
      cb.d_act_img = upload(cb.act_img, 0);
      cb.d_act_ctx = upload(cb.act_ctx, 1);
      return ok();
    };
    // attn2's renewal (attention.py:303-325): a group whose asking ratio is <= 1/16 renews its asking chunks only; the others renew every chunk
    auto attn2_ranges = [&] {
      std::vector<mx::PcRange> v;
      for (int g = 0; g < ng; ++g) if (cb.gany[g]) {
        const bool sparse = cb.gask[g] * 16 <= cb.gtot[g];
        if (!sparse) { for (int k = 0; k < gB[g]; ++k) { const int bb = gb0[g] + k; v.push_back(mx::PcRange{pcm_img[bb].row0, image.len[g], pcm_img[bb].slot, 0}); } }
        else for (int j = 0; j < pcm_nc; ++j) if (pcm_chunk_g[j] == g && cb.run[j]) v.push_back(pcm_chunks[j]);
      }
      return v;
    };
    // HOW AN ATTENTION PROJECTION'S RESULT REACHES ITS STREAM t (x or ctx): t += gate * (o W^T + bias).  Exact: the gated residual in the GEMM's
    // epilogue.  Chunk cache: the active groups' rows are materialised without gate or residual (what attn.output / attn.encoder_output
    // cache, attention.py:407-415), range-copied into the state region, and every row -- fresh or cached -- comes back through the gated copy.
    // ranges(): the rows to renew, asked for after the GEMM has been issued.
    auto project = [&](Linear l, const float* gate, char* reg, auto&& ranges) {
      if (!pcm) { linear(l.plus(l.c, d).gated(gate, ntot)); return; }
      const bool img = l.stream == kImage;
      void* t = l.c;
      l.c = img ? pcm_ti : pcm_tc;
      linear(l.only(cb.gany));
      const std::pair<const mx::PcRange*, size_t> r = ranges();
      if (ok() && mx::launch_pc_range_copy(stream, l.c, reg, img ? row_i : row_c, d, r.first, (int)r.second, 0, img ? maxL * d : row_c)) fail(mx_last_error());
      state_copy(l.stream, t, reg, 1, gate, t, 1);
    };

    for (int i = 0; i < c.num_layers && ok(); ++i) {
      const std::string b = "transformer_blocks." + std::to_string(i);
      const bool dual = c.dual_attention[i] != 0, last = i == c.num_layers - 1;
      // WHAT BRACKETS A BLOCK: nothing; the per-sample cache's decide / after around a muted walk; the chunk cache's pcm_open and output stores
      const bool cached = bc != nullptr && !pcm && !dry;
      bool ran = true;
      if (pcm) { if (!pcm_open(i, dual, last)) continue; }
      else if (cached) ran = decide(i);
      if (!ok()) break;
      mute = !ran;
      const bool* act = pcm ? cb.gany : nullptr;
      const float* mi = mod + off_img[i];   // chunks: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp[, shift2, scale2, gate2]
      const float* mc = mod + off_ctx[i];
      // AdaLN-Zero(-X) on the image stream, AdaLN-Zero / -continuous on the context stream (transformer.py:316-328)
      lnmod(kImage, x, xin, dual ? x2in : nullptr, mi + d, mi, dual ? mi + 7 * d : nullptr, dual ? mi + 6 * d : nullptr, ntot);
      if (last) lnmod(kText, ctx, cin, nullptr, mc, mc + d, nullptr, nullptr, ntot);        // continuous: (scale, shift)
      else lnmod(kText, ctx, cin, nullptr, mc + d, mc, nullptr, nullptr, ntot);
      // joint attention (attention.py:256-372): image rows first, then text rows
      // (mixed batch: group g's image rows go to rows [0, L_g) of its samples' joint sequences, the text rows behind them; the chunk cache
      // projects every chunk, attention.py:257-285)
      qkv(xin, kImage, b + ".attn.to_qkv", b + ".attn.norm_", joint);
      qkv(cin, kText, b + ".attn.add_qkv", b + ".attn.norm_added_", joint);
      attend(joint, act);
      // x += gate_msa * to_out(attn[:, :L])                                   (transformer.py:344-345)
      project(Linear{joint.o, d, b + ".attn.to_out.0", x, d, MI, d, d}.rows(kImage).from(joint), mi + 2 * d, cb.a,
              [&] { return std::make_pair(cb.d_act_img, cb.act_img.size()); });
      if (dual) {                                                             // attn2: image-only self-attention (:347-357)
        qkv(x2in, kImage, b + ".attn2.to_qkv", b + ".attn2.norm_", image);
        attend(image, act);
        project(Linear{image.o, d, b + ".attn2.to_out.0", x, d, MI, d, d}.rows(kImage), mi + 8 * d, cb.a2,
                [&] { const std::vector<mx::PcRange> v = attn2_ranges(); return std::make_pair(upload(v, 2), v.size()); });
      }
      // x += gate_mlp * ff(LN(x) * (1 + scale_mlp) + shift_mlp)               (:359-366)
      lnmod(kImage, x, xin, nullptr, mi + 4 * d, mi + 3 * d, nullptr, nullptr, ntot);
      linear(Linear{xin, d, b + ".ff.net.0.proj", ff, 4 * d, MI, 4 * d, d}.epilogue(MX_EPI_GELU_TANH));
      linear(Linear{ff, 4 * d, b + ".ff.net.2", x, d, MI, d, 4 * d}.rows(kImage).plus(x, d).gated(mi + 5 * d, ntot));
      if (!last) {                                                            // context stream (:371-386)
        project(Linear{joint.o, d, b + ".attn.to_add_out", ctx, d, MT, d, d}.rows(kText).from(joint), mc + 2 * d, cb.ae,
                [&] { return std::make_pair(cb.d_act_ctx, cb.act_ctx.size()); });
        lnmod(kText, ctx, cin, nullptr, mc + 4 * d, mc + 3 * d, nullptr, nullptr, ntot);
        linear(Linear{cin, d, b + ".ff_context.net.0.proj", ffc, 4 * d, MT, 4 * d, d}.epilogue(MX_EPI_GELU_TANH));
        linear(Linear{ffc, 4 * d, b + ".ff_context.net.2", ctx, d, MT, d, 4 * d}.rows(kText).plus(ctx, d).gated(mc + 5 * d, ntot));
        dump(b + ".context", ctx, (size_t)MT * d);
      }
      dump(b, x, (size_t)MI * d);
      mute = false;
      if (cached && ok()) after(i, ran, last);
      if (pcm) {
        state_copy(kImage, x, cb.out, 0, nullptr, nullptr, 0);
        if (!last) state_copy(kText, ctx, cb.octx, 0, nullptr, nullptr, 0);
      }
    }
    if (pcm) bc_bytes = (size_t)(pcm_top - pcm_base());
    // ---- norm_out (AdaLN-continuous) + proj_out + unpatchify (SD3Transformer.py:238-259) ----
    lnmod(kImage, x, xin, nullptr, mod + off_out, mod + off_out + d, nullptr, nullptr, ntot);
    const int No = ps * ps * c.out_channels;
    bf16_t* o = alloc<bf16_t>((size_t)MI * No);
    linear(Linear{xin, d, "proj_out", o, No, MI, No, d});
    dump("proj_out", o, (size_t)MI * No);
    for (int g = 0; g < ng && ok() && !dry; ++g)
      if (mx::launch_unpatchify(stream, o + image.row0[g] * No, g_out[g], io_dtype, gB[g], c.out_channels, gH[g], gW[g], ps, No)) fail(mx_last_error());
    if (stage && !dry && ok() && !stage_hit) fail(std::string("unknown stage '") + stage + "'");
    // the range tables of the patch cache were copied from pcm_sent asynchronously: they are released only once the stream has read them
    if (!pcm_sent.empty()) { if (!dry && hipStreamSynchronize(stream) != hipSuccess) fail("mmdit patch cache: final synchronisation failed"); pcm_sent.clear(); }
    return ok();
  }
};

int check_cfg(const mx_mmdit_config* c) {
  MX_CHECK(c != nullptr, "mmdit: null config");
  MX_CHECK(c->num_layers >= 1 && c->num_layers <= 64, "mmdit: num_layers must be 1..64");
  MX_CHECK(c->num_attention_heads >= 1, "mmdit: bad head count (head_dim is fixed at 64)");
  MX_CHECK(c->patch_size >= 1 && (c->patch_size * c->patch_size * c->in_channels) % 64 == 0, "mmdit: patch_size^2 * in_channels must be a multiple of 64");
  MX_CHECK((c->patch_size * c->patch_size * c->out_channels) % 4 == 0, "mmdit: bad out_channels");
  MX_CHECK(c->joint_attention_dim % 64 == 0 && c->pooled_projection_dim % 64 == 0, "mmdit: conditioning widths must be multiples of 64");
  MX_CHECK(c->pos_embed_max_size > 0, "mmdit: pos_embed_max_size required");
  return 0;
}

// what run_forward (plan_base.h) needs to know of the MMDiT
struct Model {
  const char* name = "mmdit";
  static int check_shape(const mx_mmdit* u, int H, int W, const char* msg) {
    const int ps = u->cfg.patch_size;
    MX_CHECK(H % ps == 0 && W % ps == 0, msg);
    MX_CHECK(H / ps <= u->cfg.pos_embed_max_size && W / ps <= u->cfg.pos_embed_max_size, "mmdit: latent larger than the positional table");
    return 0;
  }
  // the chunk unit (mx_mmdit_forward_cached_mixed and its sizing walks): whole patches of whole tokens, so a latent's tokens split into equal
  // chunks; the device decision's joint blocks compare their image stream (one input)
  int check_units(const mx_mmdit* u, const mx::ForwardCall& c) {
    const std::string who = c.cached_who(name);
    MX_CHECK(c.patch > 0 && c.patch % u->cfg.patch_size == 0, who + ": the chunk unit (latent pixels per patch edge) must be a multiple of patch_size");
    return mx::check_cache_units(who, c, c.patch, "the patch", u->cfg.num_layers, 1, 0);
  }
  int check(const mx_mmdit* u, const mx::ForwardCall& c) {
    for (int g = 1; c.groups && g < c.n_groups; ++g) if (check_shape(u, c.groups[g].H, c.groups[g].W, "mmdit: bad group shape")) return 1;
    if (check_shape(u, c.H, c.W, "mmdit: H, W must be multiples of patch_size")) return 1;
    MX_CHECK(c.dry || c.pooled, "mmdit: null operand");
    return 0;
  }
  void begin(mx_mmdit*, const mx::ForwardCall&) {}
  void end(mx_mmdit*, const mx::ForwardCall&, bool) {}
  int setup(Plan& p, mx_mmdit* u, const mx::ForwardCall& c) {
    p.u = u; p.Lt = c.ctx_len;
    return c.cache ? setup_cache(p, u, c) : 0;
  }
  // The cache's mode of the plan.  A sizing walk stops at the host tables; a forward then learns which samples hold state and queues on its stream,
  // ahead of the first launch and in this order: the slot table, the sample and chunk tables, the device decision's tables, the timestep read-back.
  int setup_cache(Plan& p, mx_mmdit* u, const mx::ForwardCall& c) {
    const std::string who = c.cached_who(name);
    mx_block_cache* cache = c.cache;
    p.bc = cache;
    if (!c.units()) {
      if (c.dry) return 0;
      return p.bc_begin(who, cache, c.batch, c.H, c.W) || p.bc_send_slots(who, Plan::kBcPartRows, Plan::kBcTables, c.batch) || p.bc_read_timesteps(who, c.timesteps, c.batch);
    }
    const int ps = u->cfg.patch_size, patch = c.patch, B = p.B;
    p.pcm = true; p.pcm_patch = patch; p.pcm_slots = cache->n_slots; p.pcm_maxh = cache->max_h; p.pcm_maxw = cache->max_w;
    long long row0 = 0;
    for (int g = 0; g < p.ng; ++g) {
      const int L = (p.gH[g] / ps) * (p.gW[g] / ps), nc = (p.gH[g] / patch) * (p.gW[g] / patch);
      for (int k = 0; k < p.gB[g]; ++k) {
        const int b = p.gb0[g] + k;
        const int slot = (!c.dry && cache->slots) ? cache->slots[b] : b;
        p.pcm_img.push_back(mx::PcSample{row0, L, 1, slot, 1});
        p.pcm_ctx.push_back(mx::PcSample{(long long)b * c.ctx_len, c.ctx_len, 1, slot, 1});
        for (int j = 0; j < nc; ++j) {
          p.pcm_chunks.push_back(mx::PcRange{row0 + (long long)j * (L / nc), L / nc, slot, j * (L / nc)});
          p.pcm_chunk_b.push_back(b); p.pcm_chunk_g.push_back(g);
        }
        row0 += L;
      }
    }
    p.pcm_nc = (int)p.pcm_chunks.size();
    if (c.dry) return 0;
    if (p.bc_begin_slots(who, cache, B)) return 1;
    MX_CHECK(p.pcm_head_bytes() <= cache->state_bytes, who + ": state buffer too small");
    const size_t ncm = p.pcm_ncmax();
    char* hp = (char*)cache->state;
    p.pcm_dpart = (double*)hp; hp += ncm * 64 * sizeof(double);
    p.pcm_dimg = (mx::PcSample*)hp; hp += (size_t)p.pcm_slots * sizeof(mx::PcSample);
    p.pcm_dctx = (mx::PcSample*)hp; hp += (size_t)p.pcm_slots * sizeof(mx::PcSample);
    p.pcm_dchunks = (mx::PcRange*)hp; hp += ncm * sizeof(mx::PcRange);
    p.pcm_dtmp = (mx::PcRange*)hp;
    MX_CHECK(hipMemcpyAsync(p.pcm_dimg, p.pcm_img.data(), (size_t)B * sizeof(mx::PcSample), hipMemcpyHostToDevice, p.stream) == hipSuccess &&
             hipMemcpyAsync(p.pcm_dctx, p.pcm_ctx.data(), (size_t)B * sizeof(mx::PcSample), hipMemcpyHostToDevice, p.stream) == hipSuccess &&
             hipMemcpyAsync(p.pcm_dchunks, p.pcm_chunks.data(), (size_t)p.pcm_nc * sizeof(mx::PcRange), hipMemcpyHostToDevice, p.stream) == hipSuccess,
             who + ": moving the tables failed");
    return p.bc_dev_begin(who, u->skip_pin, u->cfg.num_layers, (cache->max_h / patch) * (cache->max_w / patch), c.timesteps, p.pcm_chunk_b, p.group_of(), true) ||
           p.bc_read_timesteps(who, c.timesteps, B);
  }
  bool run(Plan& p, const mx::ForwardCall& c) {
    const bool okr = p.run(c.latents, c.io_dtype, c.timesteps, c.ehs, c.pooled, c.out);
    if (c.units() && !c.dry) { c.cache->patches_asked = p.pcm_asked; c.cache->patches_total = p.pcm_total; }
    return okr;
  }
  size_t cache_bytes(const Plan& p) { return p.bc_bytes; }
  std::vector<uint64_t> key_scalars(const mx::ForwardCall&) { return {}; }
  std::vector<const void*> key_operands(const mx::ForwardCall& c) { return {c.pooled}; }
};
int forward_impl(const mx_mmdit* u, const mx::ForwardCall& c) {
  Model m;
  return mx::run_forward<Plan>(const_cast<mx_mmdit*>(u), c, m);
}
using mx::dry_call;
using mx::sizing_comm;
// the fields every forward entry point fills alike; the image (latents, out, batch, H, W) or the groups and the mode's own fields follow
mx::ForwardCall forward_call(void* stream, int io_dtype, const float* timesteps, const void* ehs, const void* pooled, int ctx_len, void* workspace,
                             size_t workspace_bytes) {
  mx::ForwardCall c;
  c.stream = stream; c.io_dtype = io_dtype; c.timesteps = timesteps; c.ehs = ehs; c.pooled = pooled; c.ctx_len = ctx_len;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  return c;
}

}  // namespace

extern "C" mx_mmdit* mx_mmdit_create(const mx_mmdit_config* cfg) {
  if (check_cfg(cfg)) return nullptr;
  mx_mmdit* u = new mx_mmdit();
  u->cfg = *cfg;
  return u;
}
extern "C" void mx_mmdit_destroy(mx_mmdit* u) { delete u; }

extern "C" int mx_mmdit_set_weights(mx_mmdit* u, const void* blob, uint64_t blob_bytes, const mx_weight_entry* table, int n) {
  MX_CHECK(u != nullptr, "mmdit_set_weights: null handle");
  u->graphs.clear();    // captured graphs hold addresses resolved through the old table
  return u->weights.set("mmdit_set_weights", blob, blob_bytes, table, n);
}

extern "C" size_t mx_mmdit_workspace_bytes(const mx_mmdit* u, int batch, int H, int W, int ctx_len) {
  if (!u) return 0;
  size_t peak = 0;
  mx::ForwardCall c = dry_call(batch, H, W, ctx_len);
  c.peak = &peak;
  return forward_impl(u, c) ? 0 : peak + 4096;
}

extern "C" int mx_mmdit_validate(const mx_mmdit* u, int batch, int H, int W, int ctx_len) {
  MX_CHECK(u && u->weights.blob, "mmdit_validate: weights not set");
  mx::ForwardCall c = dry_call(batch, H, W, ctx_len);
  c.lookup = true;
  return forward_impl(u, c);
}

extern "C" int mx_mmdit_forward(mx_mmdit* u, void* stream, const void* latents, int io_dtype, const float* timesteps,
                                const void* ehs, const void* pooled, void* out, int batch, int H, int W, int ctx_len,
                                void* workspace, size_t workspace_bytes) {
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, pooled, ctx_len, workspace, workspace_bytes);
  c.latents = latents; c.out = out; c.batch = batch; c.H = H; c.W = W;
  return forward_impl(u, c);
}

/* ---- mixed-resolution batch: ONE launch sequence over the requests of every resolution present (see mx_unet_forward_mixed) ---- */
extern "C" size_t mx_mmdit_workspace_bytes_mixed(const mx_mmdit* u, const mx_unet_group* groups, int n_groups, int ctx_len) {
  if (!u || !groups || n_groups < 1 || n_groups > MX_MAX_SEGS) return 0;
  size_t peak = 0;
  mx::ForwardCall c = dry_call(0, 0, 0, ctx_len);
  c.groups = groups; c.n_groups = n_groups; c.peak = &peak;
  return forward_impl(u, c) ? 0 : peak + 4096;
}

extern "C" int mx_mmdit_forward_mixed(mx_mmdit* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                                      const void* encoder_hidden_states, const void* pooled_projections, int ctx_len, void* workspace,
                                      size_t workspace_bytes) {
  MX_CHECK(groups != nullptr, "mmdit_forward_mixed: null groups");
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, encoder_hidden_states, pooled_projections, ctx_len, workspace, workspace_bytes);
  c.groups = groups; c.n_groups = n_groups;
  return forward_impl(u, c);
}

/* ---- patch parallelism (distrifuser models/distri_sd3_transformer_pp.py, modules/pp/attn.py:202-277) ---- */
extern "C" size_t mx_mmdit_workspace_bytes_pp(const mx_mmdit* u, int batch, int H_local, int W, int ctx_len, int world) {
  if (!u) return 0;
  size_t peak = 0;
  const mx_pp_comm comm = sizing_comm(world);
  mx::ForwardCall c = dry_call(batch, H_local, W, ctx_len);
  c.comm = &comm; c.peak = &peak;
  return forward_impl(u, c) ? 0 : peak + 4096;
}

extern "C" size_t mx_mmdit_pp_state_bytes(const mx_mmdit* u, int batch, int H_local, int W, int ctx_len, int world) {
  if (!u) return 0;
  size_t need = 0;
  const mx_pp_comm comm = sizing_comm(world);
  mx_pp_stale st{}; st.mode = MX_PP_WARMUP;
  mx::ForwardCall c = dry_call(batch, H_local, W, ctx_len);
  c.comm = &comm; c.stale = &st; c.state_need = &need;
  return forward_impl(u, c) ? 0 : need + 256;
}

extern "C" int mx_mmdit_forward_pp(mx_mmdit* u, void* stream, const void* latents_local, int io_dtype, const float* timesteps, const void* ehs,
                                   const void* pooled, void* out_local, int batch, int H_local, int W, int ctx_len, const mx_pp_comm* comm,
                                   const mx_pp_stale* stale, void* workspace, size_t workspace_bytes) {
  MX_CHECK(comm != nullptr, "mmdit_forward_pp: null communicator");
  if (stale) {
    MX_CHECK(stale->mode == MX_PP_WARMUP || stale->mode == MX_PP_STALE, "mmdit_forward_pp: stale->mode must be MX_PP_WARMUP or MX_PP_STALE");
    MX_CHECK(stale->state != nullptr && ((uintptr_t)stale->state & 255) == 0, "mmdit_forward_pp: state must be 256-byte aligned device memory");
    MX_CHECK(stale->mode != MX_PP_STALE || stale->all_gather_async != nullptr, "mmdit_forward_pp: a stale step needs all_gather_async");
  }
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, pooled, ctx_len, workspace, workspace_bytes);
  c.latents = latents_local; c.out = out_local; c.batch = batch; c.H = H_local; c.W = W; c.comm = comm; c.stale = stale;
  return forward_impl(u, c);
}

extern "C" int mx_mmdit_pp_comm_plan(const mx_mmdit* u, int batch, int H_local, int W, int ctx_len, const mx_pp_comm* comm) {
  MX_CHECK(u && comm && comm->all_gather, "mmdit_pp_comm_plan: bad arguments");
  mx::ForwardCall c = dry_call(batch, H_local, W, ctx_len);
  c.comm = comm;
  return forward_impl(u, c);
}

/* ---- the cache at the reference's unit (token chunks) over a mixed batch in ONE launch sequence (include/mxdenoise.h) ---- */
extern "C" size_t mx_mmdit_patch_cache_bytes(const mx_mmdit* u, int n_slots, int max_h, int max_w, int patch, int ctx_len) {
  if (!u || n_slots <= 0 || max_h <= 0 || max_w <= 0 || patch <= 0 || ctx_len <= 0) { mx::set_error("mmdit_patch_cache_bytes: bad arguments"); return 0; }
  const mx_unet_group g{nullptr, nullptr, n_slots, max_h, max_w};      // every state row in use by a latent that fills it
  mx_block_cache sizing = mx::sizing_cache(&g, 1);
  size_t state = 0;
  mx::ForwardCall c = dry_call(0, 0, 0, ctx_len);
  c.groups = &g; c.n_groups = 1; c.patch = patch; c.cache = &sizing; c.state_bytes = &state;
  return forward_impl(u, c) ? 0 : state + 256;
}

extern "C" size_t mx_mmdit_workspace_bytes_cached_mixed(const mx_mmdit* u, const mx_unet_group* groups, int n_groups, int ctx_len, int patch) {
  if (mx::check_cached_groups("mmdit_forward_cached_mixed", groups, n_groups)) return 0;
  mx_block_cache sizing = mx::sizing_cache(groups, n_groups);
  size_t peak = 0;
  mx::ForwardCall c = dry_call(0, 0, 0, ctx_len);
  c.groups = groups; c.n_groups = n_groups; c.patch = patch; c.cache = &sizing; c.peak = &peak;
  return forward_impl(u, c) ? 0 : peak + 256;
}

extern "C" int mx_mmdit_forward_cached_mixed(mx_mmdit* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                                             const void* ehs, const void* pooled, int ctx_len, int patch, void* workspace, size_t workspace_bytes,
                                             mx_block_cache* cache) {
  const std::string who = "mmdit_forward_cached_mixed";
  MX_CHECK(cache && (cache->predict || cache->dev_down) && cache->state && cache->slots && cache->slot_valid,
           who + ": cache with predict (or dev_down), state, slots and slot_valid is required");
  MX_CHECK(((uintptr_t)cache->state & 255) == 0, who + ": cache->state must be 256-byte aligned");
  if (mx::check_cached_groups(who, groups, n_groups)) return 1;
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, pooled, ctx_len, workspace, workspace_bytes);
  c.groups = groups; c.n_groups = n_groups; c.patch = patch; c.cache = cache;
  return forward_impl(u, c);
}

/* ---- block-skip cache (include/mxdenoise.h; SD3Transformer.py:151-228 with cache_manager.py:163-191) ---- */
extern "C" size_t mx_mmdit_block_cache_bytes(const mx_mmdit* u, int batch, int H, int W, int ctx_len) {
  if (!u || batch <= 0 || H <= 0 || W <= 0 || ctx_len <= 0 || H % u->cfg.patch_size || W % u->cfg.patch_size) return 0;
  mx_block_cache sizing{};
  size_t state = 0;
  mx::ForwardCall c = dry_call(batch, H, W, ctx_len);
  c.cache = &sizing; c.state_bytes = &state;
  return forward_impl(u, c) ? 0 : state;
}

extern "C" int mx_mmdit_forward_cached(mx_mmdit* u, void* stream, const void* latents, int io_dtype, const float* timesteps, const void* ehs,
                                       const void* pooled, void* out, int batch, int H, int W, int ctx_len, void* workspace,
                                       size_t workspace_bytes, mx_block_cache* cache) {
  const std::string who = "mmdit_forward_cached";
  MX_CHECK(!cache || cache->dev_down == nullptr, who + ": the device decision (dev_down) serves the chunk unit only (mx_mmdit_forward_cached_mixed)");
  MX_CHECK(cache && cache->predict && cache->state, who + ": cache, cache->predict and cache->state are required");
  MX_CHECK(((uintptr_t)cache->state & 255) == 0, who + ": cache->state must be 256-byte aligned");
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, pooled, ctx_len, workspace, workspace_bytes);
  c.latents = latents; c.out = out; c.batch = batch; c.H = H; c.W = W; c.cache = cache;
  return forward_impl(u, c);
}

extern "C" int mx_mmdit_forward_trace(mx_mmdit* u, void* stream, const void* latents, int io_dtype, const float* timesteps,
                                      const void* ehs, const void* pooled, void* out, int batch, int H, int W, int ctx_len,
                                      void* workspace, size_t workspace_bytes, const char* stage, void* stage_out,
                                      size_t stage_out_bytes) {
  MX_CHECK(stage && stage_out, "mmdit_forward_trace: stage and stage_out required");
  mx::ForwardCall c = forward_call(stream, io_dtype, timesteps, ehs, pooled, ctx_len, workspace, workspace_bytes);
  c.latents = latents; c.out = out; c.batch = batch; c.H = H; c.W = W;
  c.stage = stage; c.stage_out = stage_out; c.stage_bytes = stage_out_bytes;
  return forward_impl(u, c);
}
