// Step plan of a CLIP VISION ENCODER (transformers CLIPVisionModelWithProjection): what the caller of an IP-Adapter runs on the client's reference
// image before the denoising loop -- OpenCLIP ViT-H/14 for the SDXL adapter checkpoints, ViT-L/14 for the others.  Same scaffold and building blocks
// as clip_text.cpp; two launches are its own: the patch embedding from the 8-bit image (patch_embed.hip) and, for ViT-H's heads of 80, the resident-key
// attention (attention_d80.hip).  Heads of 64 take the 64-wide flash attention through the q | k | V^T epilogue, as the text encoder does (unmasked).
//   encode(image): x = [cls | W patches] + pos;  x = pre_layrnorm(x);  per layer: x += out_proj(attn(qkv(LN1 x)));  x += fc2(act(fc1(LN2 x)));
//                  hidden = hidden_states[-2] (the last layer's input);  image_embeds = visual_projection(post_layernorm(x[:, 0]))
// Arena, weight lookup and the gemm wrapper: mx::PlanBase (plan_base.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/mxdenoise.h"
#include "common.h"
#include "plan_base.h"

using mx::bf16_t;

struct mx_clip_vision {
  mx_clip_vision_config cfg;
  mx::WeightTable weights;
};

namespace {
struct Plan : mx::PlanBase {
  mx_clip_vision* u; int B;
  bool linear(const bf16_t* a, int lda, const std::string& stem, void* c, int M, int N, int K, const void* residual = nullptr, int flags = 0, bool bias = true) {
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.a = a; d.lda = lda; d.w = wb(stem + ".weight", (size_t)N * K); d.bias = bias ? wf(stem + ".bias", N) : nullptr;
    d.c = c; d.ldc = N; d.M = M; d.N = N; d.K = K; d.residual = residual; d.ldr = N; d.flags = flags;
    return gemm(d);
  }
  bool layernorm(const bf16_t* x, bf16_t* y, const std::string& stem, int M, int H) {
    const float* g = wf(stem + ".weight", H); const float* b = wf(stem + ".bias", H);
    if (ok() && !dry && mx_layernorm(stream, x, y, g, b, M, H, u->cfg.layer_norm_eps)) fail(std::string("layernorm: ") + mx_last_error());
    return ok();
  }
  bool copy_out(void* dst, const bf16_t* src, size_t elems) {
    if (ok() && !dry && hipMemcpyAsync(dst, src, elems * 2, hipMemcpyDeviceToDevice, stream) != hipSuccess) fail("hidden copy failed");
    return ok();
  }

  bool run(const void* images, int64_t row_stride, int64_t image_stride, void* embeds_out, void* hidden_out) {
    const mx_clip_vision_config& c = u->cfg;
    const int H = c.hidden_size, heads = c.num_attention_heads, P = c.patch_size, G = c.image_size / P;
    const int L = 1 + G * G, M = B * L, ldw = MX_CLIP_VISION_LDW(P);
    const bool d80 = H == 80 * heads;
    const int ldvt = MX_VT_LD(L);
    const int keep = c.num_hidden_layers - 1;                  // hidden_states[-2] of (pre_layrnorm output, layer 1, ..., layer N): the input of layer N - 1
    bf16_t* x = alloc<bf16_t>((size_t)M * H);
    bf16_t* n = alloc<bf16_t>((size_t)M * H);
    bf16_t* qkv = alloc<bf16_t>((size_t)M * (d80 ? 3 : 2) * H);
    bf16_t* vt = d80 ? nullptr : alloc<bf16_t>((size_t)B * H * ldvt);
    bf16_t* ao = alloc<bf16_t>((size_t)M * H);
    bf16_t* ff = alloc<bf16_t>((size_t)M * c.intermediate_size);
    const std::string vm = "vision_model.";
    const bf16_t* pw = wb(vm + "embeddings.patch_embedding.weight", (size_t)H * ldw);
    const bf16_t* cls = wb(vm + "embeddings.class_embedding", H);
    const bf16_t* pos = wb(vm + "embeddings.position_embedding.weight", (size_t)L * H);
    if (ok() && !dry && mx_patch_embed_u8(stream, images, row_stride, image_stride, pw, ldw, cls, pos, n, B, G, G, P, H, c.image_mean, c.image_std))
      fail(std::string("patch embed: ") + mx_last_error());
    layernorm(n, x, vm + "pre_layrnorm", M, H);
    const int act = c.hidden_act == 1 ? MX_EPI_GELU : MX_EPI_QUICK_GELU;
    for (int l = 0; l < c.num_hidden_layers && ok(); ++l) {
      if (l == keep && hidden_out) copy_out(hidden_out, x, (size_t)M * H);
      if (l >= keep && !embeds_out) break;                     // nothing after hidden_states[-2] is asked for
      const std::string p = vm + "encoder.layers." + std::to_string(l);
      layernorm(x, n, p + ".layer_norm1", M, H);
      if (d80) {                                               // plain q | k | v rows; the kernel scales the scores and transposes V through LDS
        linear(n, H, p + ".self_attn.qkv_proj", qkv, M, 3 * H, H);
        if (ok() && !dry && mx_attention_d80(stream, qkv, 3 * H, qkv + H, 3 * H, qkv + 2 * H, 3 * H, ao, H, B, heads, L))
          fail(std::string("attention: ") + mx_last_error());
      } else {                                                 // q scaled for the prescaled attention, V written transposed
        mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
        d.a = n; d.lda = H; d.w = wb(p + ".self_attn.qkv_proj.weight", (size_t)3 * H * H); d.bias = wf(p + ".self_attn.qkv_proj.bias", 3 * H);
        d.c = qkv; d.ldc = 2 * H; d.M = M; d.N = 3 * H; d.K = H; d.flags = MX_EPI_QKV; d.seg = H; d.period = 3; d.vt = vt; d.ldvt = ldvt;
        d.rows_per_batch = L; d.out_scale = MX_ATTN_QSCALE(0.125f);
        gemm(d);
        if (ok() && !dry && mx_attention_prescaled(stream, qkv, 2 * H, qkv + H, 2 * H, vt, ldvt, (int64_t)H * ldvt, ao, H, B, heads, L, L))
          fail(std::string("attention: ") + mx_last_error());
      }
      linear(ao, H, p + ".self_attn.out_proj", x, M, H, H, x);
      layernorm(x, n, p + ".layer_norm2", M, H);
      linear(n, H, p + ".mlp.fc1", ff, M, c.intermediate_size, H, nullptr, act);
      linear(ff, c.intermediate_size, p + ".mlp.fc2", x, M, H, c.intermediate_size, x);
    }
    if (embeds_out) {                                          // the class rows alone: gathered, normalised, projected (no bias, fp32 out)
      bf16_t* crow = alloc<bf16_t>((size_t)B * H);
      bf16_t* cn = alloc<bf16_t>((size_t)B * H);
      if (ok() && !dry && hipMemcpy2DAsync(crow, (size_t)H * 2, x, (size_t)L * H * 2, (size_t)H * 2, B, hipMemcpyDeviceToDevice, stream) != hipSuccess)
        fail("class row copy failed");
      layernorm(crow, cn, vm + "post_layernorm", B, H);
      linear(cn, H, "visual_projection", embeds_out, B, c.projection_dim, H, nullptr, MX_EPI_OUT_F32, false);
    }
    return ok();
  }
};

int run_impl(mx_clip_vision* u, void* stream, const void* images, int64_t row_stride, int64_t image_stride, void* embeds_out, void* hidden_out, int batch,
             void* ws, size_t ws_bytes, bool dry, bool lookup, size_t* peak) {
  MX_CHECK(u != nullptr, "clip_vision: null handle");
  MX_CHECK(batch > 0, "clip_vision: bad batch");
  if (!dry) MX_CHECK(images && ws && u->weights.blob && (embeds_out || hidden_out), "clip_vision: null operand or weights not set");
  Plan p;
  p.u = u; p.B = batch; p.lookup = lookup;
  if (dry) p.begin_dry(u->weights); else p.begin(u->weights, (hipStream_t)stream, ws, ws_bytes);
  const bool okr = p.run(images, row_stride, image_stride, dry ? (void*)16 : embeds_out, dry ? (void*)16 : hidden_out);
  return p.finish(okr, peak);
}
}  // namespace

extern "C" mx_clip_vision* mx_clip_vision_create(const mx_clip_vision_config* c) {
  if (!c || c->hidden_size <= 0 || c->num_attention_heads <= 0 || c->hidden_size % 64 != 0 || c->intermediate_size <= 0 || c->intermediate_size % 64 != 0 ||
      c->num_hidden_layers < 1 || c->patch_size < 1 || c->image_size < c->patch_size || c->image_size % c->patch_size != 0 || c->hidden_act < 0 ||
      c->hidden_act > 1 || c->projection_dim <= 0 || c->projection_dim % 4 != 0 || c->image_std[0] == 0.f || c->image_std[1] == 0.f || c->image_std[2] == 0.f) {
    mx::set_error("clip_vision: bad config (hidden and intermediate multiples of 64, image a whole number of patches, hidden_act 0 = quick_gelu | 1 = gelu)");
    return nullptr;
  }
  if (c->hidden_size != 80 * c->num_attention_heads && c->hidden_size != 64 * c->num_attention_heads) {
    mx::set_error("clip_vision: heads of " + std::to_string(c->hidden_size / c->num_attention_heads) + " are not served (80: ViT-H/14, 64: ViT-L/14)");
    return nullptr;
  }
  const int G = c->image_size / c->patch_size;
  if (c->hidden_size == 80 * c->num_attention_heads && 1 + G * G > MX_ATTN_D80_MAX_L) {
    mx::set_error("clip_vision: " + std::to_string(1 + G * G) + " tokens exceed the 80-wide attention's " + std::to_string(MX_ATTN_D80_MAX_L));
    return nullptr;
  }
  mx_clip_vision* u = new mx_clip_vision();
  u->cfg = *c;
  return u;
}
extern "C" void mx_clip_vision_destroy(mx_clip_vision* u) { delete u; }
extern "C" int mx_clip_vision_set_weights(mx_clip_vision* u, const void* blob, uint64_t blob_bytes, const mx_weight_entry* table, int n) {
  MX_CHECK(u != nullptr, "clip_vision_set_weights: null handle");
  return u->weights.set("clip_vision_set_weights", blob, blob_bytes, table, n);
}
extern "C" size_t mx_clip_vision_workspace_bytes(const mx_clip_vision* u, int batch) {
  size_t peak = 0;
  if (run_impl(const_cast<mx_clip_vision*>(u), nullptr, nullptr, 0, 0, nullptr, nullptr, batch, nullptr, 0, true, false, &peak)) return 0;
  return peak + 4096;
}
extern "C" int mx_clip_vision_validate(const mx_clip_vision* u, int batch) {
  MX_CHECK(u && u->weights.blob, "clip_vision_validate: weights not set");
  return run_impl(const_cast<mx_clip_vision*>(u), nullptr, nullptr, 0, 0, nullptr, nullptr, batch, nullptr, 0, true, true, nullptr);
}
extern "C" int mx_clip_vision_encode(mx_clip_vision* u, void* stream, const void* images, int64_t row_stride, int64_t image_stride, void* embeds_out,
                                     void* hidden_out, int batch, void* workspace, size_t workspace_bytes) {
  return run_impl(u, stream, images, row_stride, image_stride, embeds_out, hidden_out, batch, workspace, workspace_bytes, false, false, nullptr);
}
