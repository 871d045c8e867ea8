// Step plan of the SDXL VAE DECODER (AutoencoderKL.decode), the step AFTER the denoising loop: the reference's post_inference
// (sduss/model_executor/diffusers/pipelines/stable_diffusion_xl/pipeline_stable_diffusion_xl_esymred.py:406-463) divides the latents
// by the scaling factor and calls self.vae.decode (un-vendored diffusers 0.32.1 AutoencoderKL).
// Same building blocks as the UNet plan (NHWC bf16, implicit-GEMM 3x3 convs with the nearest-2x upsample fused in the loader,
// GroupNorm+SiLU, GEMM epilogues); the one new piece is the mid block's single-head 512-wide attention, run as
// GEMM (q k^T / sqrt(C)) -> row softmax -> GEMM (P V) because the flash kernel is specialised for 64-wide heads.
//   decode(z):  post_quant_conv(z / scaling)  ->  conv_in  ->  mid: resnet, attention, resnet  ->  up blocks (3 resnets each,
//               nearest-2x + conv between them)  ->  GroupNorm + SiLU  ->  conv_out      (the scaling is folded into post_quant_conv)
// The reference runs this in fp32 (force_upcast, :48-52); here bf16 storage / fp32 accumulate, tolerance stated in tests/test_vae_gpu.py.
// Arena, weight lookup and the gemm / conv wrapper: mx::PlanBase (plan_base.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/mxdenoise.h"
#include "common.h"
#include "plan_base.h"

namespace mx {
int launch_prep_latent(hipStream_t s, const void* in, int dtype, void* out, int B, int Cin, int HW, int CP);
int launch_nhwc_to_nchw(hipStream_t s, const void* in, void* out, int dtype, int B, int C, int HW, int ld);
int launch_softmax_rows(hipStream_t s, void* scores, long rows, int L, long ld);
size_t gn_workspace_exact(int B, int H, int W, int C, int patch);
}  // namespace mx

using mx::bf16_t;

struct mx_vae {
  mx_vae_config cfg;
  mx::WeightTable weights;
};

namespace {
constexpr int kPad = 64;   // the 4 latent channels are zero-padded to one K tile
constexpr int kRgb8 = -1;  // run()'s out_dtype of mx_vae_decode_rgb8

struct Plan : mx::PlanBase {
  mx_vae* u; int B, H, W;
  bool linear(const bf16_t* a, int lda, const bf16_t* wgt, const float* bias, void* c, int ldc, int M, int N, int K, const void* residual = nullptr,
              int ldr = 0, float out_scale = 0.f) {
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.a = a; d.lda = lda; d.w = wgt; d.bias = bias; d.c = c; d.ldc = ldc; d.M = M; d.N = N; d.K = K; d.residual = residual; d.ldr = ldr; d.out_scale = out_scale;
    return gemm(d, false);
  }
  bool conv(const bf16_t* x, int h, int wd, int Cin, const std::string& prefix, bf16_t* out, int Cout, int up, const void* residual = nullptr, int stride = 1) {
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.a = x; d.w = wb(prefix + ".weight", (size_t)Cout * 9 * Cin); d.bias = wf(prefix + ".bias", Cout);
    d.c = out; d.ldc = Cout; d.B = B; d.Hin = h; d.Win = wd; d.Cin = Cin; d.Hout = ((h << up) + stride - 1) / stride; d.Wout = ((wd << up) + stride - 1) / stride;
    d.stride = stride; d.up = up;
    d.M = B * d.Hout * d.Wout; d.N = Cout; d.K = 9 * Cin; d.rows_per_batch = d.Hout * d.Wout; d.residual = residual; d.ldr = Cout;
    return gemm(d, true);
  }
  bool groupnorm(const bf16_t* x, bf16_t* y, const std::string& prefix, int h, int wd, int C, bool silu) {
    if (!ok()) return false;
    const size_t m = ar.mark();
    void* ws = ar.alloc(mx::gn_workspace_exact(B, h, wd, C, 0));
    if (!ws) return fail("workspace too small");
    const float* g = wf(prefix + ".weight", C); const float* b = wf(prefix + ".bias", C);
    if (ok() && !dry && mx_groupnorm_nhwc(stream, x, y, g, b, B, h, wd, C, u->cfg.norm_num_groups, u->cfg.norm_eps, silu ? 1 : 0, 0, ws))
      fail(std::string("groupnorm: ") + mx_last_error());
    ar.release(m);
    return ok();
  }
  // diffusers ResnetBlock2D without time embedding: GN-SiLU-conv, GN-SiLU-conv, (1x1 shortcut), add
  bf16_t* resnet(const std::string& p, const bf16_t* x, int h, int wd, int Cin, int Cout) {
    const size_t M = (size_t)B * h * wd;
    bf16_t* out = alloc<bf16_t>(M * Cout);
    const size_t m = ar.mark();
    bf16_t* n1 = alloc<bf16_t>(M * Cin);
    groupnorm(x, n1, p + ".norm1", h, wd, Cin, true);
    bf16_t* h1 = alloc<bf16_t>(M * Cout);
    conv(n1, h, wd, Cin, p + ".conv1", h1, Cout, 0);
    bf16_t* n2 = alloc<bf16_t>(M * Cout);
    groupnorm(h1, n2, p + ".norm2", h, wd, Cout, true);
    const bf16_t* sc = x;
    if (Cin != Cout) {
      bf16_t* s2 = alloc<bf16_t>(M * Cout);
      linear(x, Cin, wb(p + ".conv_shortcut.weight", (size_t)Cout * Cin), wf(p + ".conv_shortcut.bias", Cout), s2, Cout, (int)M, Cout, Cin);
      sc = s2;
    }
    conv(n2, h, wd, Cout, p + ".conv2", out, Cout, 0, sc);
    ar.release(m);
    return out;
  }
  // mid-block attention: one head of width C over the h*wd tokens of each image
  bf16_t* attention(const std::string& p, const bf16_t* x, int h, int wd, int C) {
    const int L = h * wd;
    const size_t M = (size_t)B * L;
    bf16_t* out = alloc<bf16_t>(M * C);
    const size_t m = ar.mark();
    if (L % 8 != 0) fail("vae attention: tokens per image must be a multiple of 8");
    bf16_t* n = alloc<bf16_t>(M * C);
    groupnorm(x, n, p + ".group_norm", h, wd, C, false);
    bf16_t* q = alloc<bf16_t>(M * C);
    bf16_t* k = alloc<bf16_t>(M * C);
    bf16_t* vt = alloc<bf16_t>((size_t)C * L);         // V^T of one image: [C, L]
    bf16_t* sc = alloc<bf16_t>((size_t)L * L);         // scores of one image
    bf16_t* o = alloc<bf16_t>(M * C);
    linear(n, C, wb(p + ".to_q.weight", (size_t)C * C), wf(p + ".to_q.bias", C), q, C, (int)M, C, C);
    linear(n, C, wb(p + ".to_k.weight", (size_t)C * C), wf(p + ".to_k.bias", C), k, C, (int)M, C, C);
    const float scale = 1.0f / std::sqrt((float)C);
    for (int b = 0; b < B && ok(); ++b) {
      const bf16_t* nb = n + (size_t)b * L * C;
      // V^T = Wv n^T (the value bias is added after P V: the rows of P sum to one)
      linear(wb(p + ".to_v.weight", (size_t)C * C), C, nb, nullptr, vt, L, C, L, C);
      linear(q + (size_t)b * L * C, C, k + (size_t)b * L * C, nullptr, sc, L, L, L, C, nullptr, 0, scale);
      if (ok() && !dry && mx::launch_softmax_rows(stream, sc, L, L, L)) fail(mx_last_error());
      linear(sc, L, vt, wf(p + ".to_v.bias", C), o + (size_t)b * L * C, C, L, C, L);
    }
    linear(o, C, wb(p + ".to_out.0.weight", (size_t)C * C), wf(p + ".to_out.0.bias", C), out, C, (int)M, C, C, x, C);
    ar.release(m);
    return out;
  }

  // out_dtype >= 0: images [B, out_channels, 8H, 8W] of that dtype in [-1, 1];  out_dtype < 0 (kRgb8): uint8 [B, 8H, 8W, 3]
  bool run(const void* latents, int io_dtype, void* outp, int out_dtype) {
    const mx_vae_config& c = u->cfg;
    const int nlev = c.n_levels;
    int h = H, wd = W;
    const size_t M0 = (size_t)B * h * wd;
    bf16_t* z0 = alloc<bf16_t>(M0 * kPad);
    if (ok() && !dry && mx::launch_prep_latent(stream, latents, io_dtype, z0, B, c.latent_channels, h * wd, kPad)) fail(mx_last_error());
    bf16_t* z1 = alloc<bf16_t>(M0 * kPad);             // post_quant_conv (1x1; 1 / scaling_factor folded into its weight), padded to 64 channels
    linear(z0, kPad, wb("post_quant_conv.weight", (size_t)kPad * kPad), wf("post_quant_conv.bias", kPad), z1, kPad, (int)M0, kPad, kPad);
    int C = c.block_out_channels[nlev - 1];
    bf16_t* x = alloc<bf16_t>(M0 * C);
    conv(z1, h, wd, kPad, "decoder.conv_in", x, C, 0);
    x = resnet("decoder.mid_block.resnets.0", x, h, wd, C, C);
    x = attention("decoder.mid_block.attentions.0", x, h, wd, C);
    x = resnet("decoder.mid_block.resnets.1", x, h, wd, C, C);
    for (int i = 0; i < nlev && ok(); ++i) {
      const int Cout = c.block_out_channels[nlev - 1 - i];
      for (int j = 0; j < c.layers_per_block + 1 && ok(); ++j) {
        x = resnet("decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), x, h, wd, C, Cout);
        C = Cout;
      }
      if (i != nlev - 1) {
        bf16_t* d = alloc<bf16_t>((size_t)B * (2 * h) * (2 * wd) * C);
        conv(x, h, wd, C, "decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv", d, C, 1);
        h *= 2; wd *= 2;
        x = d;
      }
    }
    const size_t M = (size_t)B * h * wd;
    bf16_t* n = alloc<bf16_t>(M * C);
    groupnorm(x, n, "decoder.conv_norm_out", h, wd, C, true);
    const int ldo = (c.out_channels + 3) / 4 * 4;
    if (out_dtype == kRgb8) {                          // conv_out + postprocess + 8-bit store in one launch; no bf16 image, no transpose
      const bf16_t* wgt = wb("decoder.conv_out.weight", (size_t)ldo * 9 * C); const float* bias = wf("decoder.conv_out.bias", ldo);
      if (ok() && !dry && mx_conv3x3_rgb8(stream, n, wgt, bias, outp, B, h, wd, C)) fail(std::string("conv3x3_rgb8: ") + mx_last_error());
      return ok();
    }
    bf16_t* o = alloc<bf16_t>(M * ldo);
    conv(n, h, wd, C, "decoder.conv_out", o, ldo, 0);
    if (ok() && !dry && mx::launch_nhwc_to_nchw(stream, o, outp, out_dtype, B, c.out_channels, h * wd, ldo)) fail(mx_last_error());
    return ok();
  }
};

// The ENCODER (AutoencoderKL.encode -> posterior -> scaled latents), the decoder's graph walked the other way on the same wrappers:
//   conv_in -> down blocks (layers_per_block resnets each, a stride-2 conv between them) -> mid: resnet, attention, resnet -> GroupNorm + SiLU
//   -> conv_out (2 lc moments, stored 64 wide) -> quant_conv (1x1 as a padded [64, 64] linear; SD3 has none) -> mode / sample, shift, scale, start noise.
// diffusers' Downsample2D pads (0, 1, 0, 1) and convolves with stride 2, pad 0.  Rotated by 180 degrees that is the stride-2 PAD-1 conv of the
// library's loader, and a pad-1 stride-1 conv commutes with the rotation when its weights are rotated too; GroupNorm, 1x1 convs and attention over
// all tokens do not see pixel order.  So the whole plan runs in the rotated orientation: the first launch reads the image backwards
// (mx_conv3x3_rgb_in, rotate = 1), the packer has rotated every 3x3 weight (vae.py, pack_vae_encoder), the last launch reads the moments backwards.
// H, W here are IMAGE pixels.
struct EncodePlan : Plan {
  bool run_encode(const mx_vae_encode_args& a) {
    const mx_vae_config& c = u->cfg;
    const int nlev = c.n_levels, lc = c.latent_channels;
    int h = H, wd = W;
    int C = c.block_out_channels[0];
    bf16_t* x = alloc<bf16_t>((size_t)B * h * wd * C);
    {
      const bf16_t* wgt = wb("encoder.conv_in.weight", (size_t)C * 32); const float* bias = wf("encoder.conv_in.bias", C);
      if (ok() && !dry && mx_conv3x3_rgb_in(stream, a.image, a.image_format, wgt, bias, x, B, h, wd, C, 1)) fail(std::string("conv3x3_rgb_in: ") + mx_last_error());
    }
    for (int i = 0; i < nlev && ok(); ++i) {
      const int Cout = c.block_out_channels[i];
      for (int j = 0; j < c.layers_per_block && ok(); ++j) {
        x = resnet("encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), x, h, wd, C, Cout);
        C = Cout;
      }
      if (i != nlev - 1) {
        bf16_t* d = alloc<bf16_t>((size_t)B * (h / 2) * (wd / 2) * C);
        conv(x, h, wd, C, "encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", d, C, 0, nullptr, 2);
        h /= 2; wd /= 2;
        x = d;
      }
    }
    x = resnet("encoder.mid_block.resnets.0", x, h, wd, C, C);
    x = attention("encoder.mid_block.attentions.0", x, h, wd, C);
    x = resnet("encoder.mid_block.resnets.1", x, h, wd, C, C);
    const size_t M = (size_t)B * h * wd;
    bf16_t* n = alloc<bf16_t>(M * C);
    groupnorm(x, n, "encoder.conv_norm_out", h, wd, C, true);
    bf16_t* mom = alloc<bf16_t>(M * kPad);               // the 2 lc moments in columns [0, 2 lc) of 64 (rows 2 lc .. 63 of the packed conv_out are zero)
    conv(n, h, wd, C, "encoder.conv_out", mom, kPad, 0);
    bf16_t* q = alloc<bf16_t>(M * kPad);                 // (sized whether or not the table names a quant_conv: the sizing walk may run before the weights are set)
    if (u->weights.table.count("quant_conv.weight")) {   // SD3's AutoencoderKL has none: conv_out's moments are the posterior's
      linear(mom, kPad, wb("quant_conv.weight", (size_t)kPad * kPad), wf("quant_conv.bias", kPad), q, kPad, (int)M, kPad, kPad);
      mom = q;
    }
    if (ok() && !dry && mx_vae_latent_finish(stream, mom, kPad, a.latents, a.io_dtype, B, lc, h, wd, a.scaling_factor, a.shift_factor, a.posterior_noise,
                                             a.start_noise, a.keep, a.sigma, 1))
      fail(std::string("vae_latent_finish: ") + mx_last_error());
    return ok();
  }
};

int encode_impl(mx_vae* u, void* stream, const mx_vae_encode_args* a, int batch, int H, int W, void* ws, size_t ws_bytes, bool dry, bool lookup, size_t* peak) {
  MX_CHECK(u != nullptr, "vae_encode: null handle");
  MX_CHECK(batch > 0 && H > 0 && W > 0, "vae_encode: bad shape");
  MX_CHECK(u->cfg.out_channels == 3, "vae_encode: an RGB image needs out_channels == 3");
  MX_CHECK(2 * u->cfg.latent_channels <= kPad, "vae_encode: the moments must fit 64 columns");
  const int f = 1 << (u->cfg.n_levels - 1);
  MX_CHECK(H % f == 0 && W % f == 0, "vae_encode: H and W must be multiples of 2^(n_levels - 1) = " + std::to_string(f));
  mx_vae_encode_args none; std::memset(&none, 0, sizeof(none));
  if (!dry) {
    MX_CHECK(a && a->image && a->latents && ws && u->weights.blob, "vae_encode: null operand or weights not set");
    MX_CHECK(a->io_dtype >= 0 && a->io_dtype <= 2, "vae_encode: bad dtype");
    MX_CHECK(a->image_format == MX_IMAGE_RGB8_HWC || a->image_format == MX_IMAGE_F32_CHW, "vae_encode: bad image format");
    MX_CHECK(!a->start_noise || (a->keep && a->sigma), "vae_encode: start_noise needs keep and sigma");
  }
  EncodePlan p;
  p.u = u; p.B = batch; p.H = H; p.W = W; p.lookup = lookup;
  if (dry) p.begin_dry(u->weights); else p.begin(u->weights, (hipStream_t)stream, ws, ws_bytes);
  const bool okr = p.run_encode(dry ? none : *a);
  return p.finish(okr, peak);
}

int run_impl(mx_vae* u, void* stream, const void* latents, int io_dtype, void* out, int out_dtype, int batch, int H, int W, void* ws, size_t ws_bytes,
             bool dry, bool lookup, size_t* peak) {
  MX_CHECK(u != nullptr, "vae: null handle");
  MX_CHECK(batch > 0 && H > 0 && W > 0, "vae: bad shape");
  if (!dry) {
    MX_CHECK(latents && out && ws && u->weights.blob, "vae: null operand or weights not set");
    MX_CHECK(io_dtype >= 0 && io_dtype <= 2 && out_dtype >= kRgb8 && out_dtype <= 2, "vae: bad dtype");
  }
  Plan p;
  p.u = u; p.B = batch; p.H = H; p.W = W; p.lookup = lookup;
  if (dry) p.begin_dry(u->weights); else p.begin(u->weights, (hipStream_t)stream, ws, ws_bytes);
  const bool okr = p.run(latents, io_dtype, out, out_dtype);
  return p.finish(okr, peak);
}
}  // namespace

extern "C" mx_vae* mx_vae_create(const mx_vae_config* c) {
  if (!c || c->n_levels < 1 || c->n_levels > 4 || c->latent_channels <= 0 || c->latent_channels > kPad || c->out_channels <= 0 || c->out_channels > 4) {
    mx::set_error("vae: bad config");
    return nullptr;
  }
  for (int i = 0; i < c->n_levels; ++i)
    if (c->block_out_channels[i] % 64 != 0 || c->block_out_channels[i] % c->norm_num_groups != 0) { mx::set_error("vae: block_out_channels must be multiples of 64 and of the group count"); return nullptr; }
  mx_vae* u = new mx_vae();
  u->cfg = *c;
  return u;
}
extern "C" void mx_vae_destroy(mx_vae* u) { delete u; }
extern "C" int mx_vae_set_weights(mx_vae* u, const void* blob, uint64_t blob_bytes, const mx_weight_entry* table, int n) {
  MX_CHECK(u != nullptr, "vae_set_weights: null handle");
  return u->weights.set("vae_set_weights", blob, blob_bytes, table, n);
}
extern "C" size_t mx_vae_workspace_bytes(const mx_vae* u, int batch, int H, int W) {
  size_t peak = 0;
  if (run_impl(const_cast<mx_vae*>(u), nullptr, nullptr, MX_BF16, nullptr, MX_F32, batch, H, W, nullptr, 0, true, false, &peak)) return 0;
  return peak + 4096;
}
extern "C" int mx_vae_validate(const mx_vae* u, int batch, int H, int W) {
  MX_CHECK(u && u->weights.blob, "vae_validate: weights not set");
  return run_impl(const_cast<mx_vae*>(u), nullptr, nullptr, MX_BF16, nullptr, MX_F32, batch, H, W, nullptr, 0, true, true, nullptr);
}
extern "C" int mx_vae_decode(mx_vae* u, void* stream, const void* latents, int io_dtype, void* out, int out_dtype, int batch, int H, int W,
                             void* workspace, size_t workspace_bytes) {
  MX_CHECK(out_dtype >= 0, "vae: bad dtype");
  return run_impl(u, stream, latents, io_dtype, out, out_dtype, batch, H, W, workspace, workspace_bytes, false, false, nullptr);
}
extern "C" int mx_vae_decode_rgb8(mx_vae* u, void* stream, const void* latents, int io_dtype, void* out, int batch, int H, int W, void* workspace,
                                  size_t workspace_bytes) {
  MX_CHECK(u != nullptr, "vae_decode_rgb8: null handle");
  MX_CHECK(u->cfg.out_channels == 3, "vae_decode_rgb8: an RGB image needs out_channels == 3");
  return run_impl(u, stream, latents, io_dtype, out, kRgb8, batch, H, W, workspace, workspace_bytes, false, false, nullptr);
}
extern "C" size_t mx_vae_encode_workspace_bytes(const mx_vae* u, int batch, int H, int W) {
  size_t peak = 0;
  if (encode_impl(const_cast<mx_vae*>(u), nullptr, nullptr, batch, H, W, nullptr, 0, true, false, &peak)) return 0;
  return peak + 4096;
}
extern "C" int mx_vae_encode_validate(const mx_vae* u, int batch, int H, int W) {
  MX_CHECK(u && u->weights.blob, "vae_encode_validate: weights not set");
  return encode_impl(const_cast<mx_vae*>(u), nullptr, nullptr, batch, H, W, nullptr, 0, true, true, nullptr);
}
extern "C" int mx_vae_encode(mx_vae* u, void* stream, const mx_vae_encode_args* args, int batch, int H, int W, void* workspace, size_t workspace_bytes) {
  return encode_impl(u, stream, args, batch, H, W, workspace, workspace_bytes, false, false, nullptr);
}
