"""Checker side of the image-prompt adapter tests: a random adapter in diffusers' module-path names, and the oracle's BasicTransformerBlock with
the image term added in fp32 (installed over oracle.sdxl_unet_ref.basic_transformer_block with pytest's monkeypatch)."""
import torch
import torch.nn.functional as F

from sduss_amd.ip_adapter import cross_attention_layers

PROJ = "encoder_hid_proj.image_projection_layers.0."


def random_adapter_sd(cfg, seed, n_img=4, embed_dim=64, prefix="unet."):
    g = torch.Generator().manual_seed(seed)
    ctx, rnd = cfg.cross_attention_dim, lambda *s: torch.randn(*s, generator=g)
    sd = {}
    for b, dim in cross_attention_layers(cfg):
        for nm in ("to_k_ip", "to_v_ip"):
            sd[f"{prefix}{b}.attn2.processor.{nm}.0.weight"] = (rnd(dim, ctx) * ctx ** -0.5).bfloat16().float()
    sd[prefix + PROJ + "image_embeds.weight"] = (rnd(n_img * ctx, embed_dim) * embed_dim ** -0.5).bfloat16().float()
    sd[prefix + PROJ + "image_embeds.bias"] = 0.1 * rnd(n_img * ctx)
    sd[prefix + PROJ + "norm.weight"] = 1.0 + 0.1 * rnd(ctx)
    sd[prefix + PROJ + "norm.bias"] = 0.1 * rnd(ctx)
    return sd


def tokens_ref(cfg, sd, image_embeds, prefix="unet."):
    ctx = cfg.cross_attention_dim                # diffusers' ImageProjection in fp32: [rows, embed_dim] -> [rows, n_img, cross_attention_dim]
    y = F.linear(image_embeds.float(), sd[prefix + PROJ + "image_embeds.weight"], sd[prefix + PROJ + "image_embeds.bias"])
    return F.layer_norm(y.reshape(image_embeds.shape[0], -1, ctx), (ctx,), sd[prefix + PROJ + "norm.weight"], sd[prefix + PROJ + "norm.bias"], 1e-5)


def block_with_image_term(ref, sd, tokens, scale, prefix="unet."):      # attn2 += scale[row] * attention(q, to_k_ip(tokens), to_v_ip(tokens)); tokens fp32
    def block(P, b, x, ctx, heads, cfg):
        dim, eps = x.shape[-1], cfg.layer_norm_eps
        ln = lambda i: F.layer_norm(x, (dim,), P[f"{b}.norm{i}.weight"], P[f"{b}.norm{i}.bias"], eps)
        n = ln(1)
        a = ref.attention(F.linear(n, P[f"{b}.attn1.to_q.weight"]), F.linear(n, P[f"{b}.attn1.to_k.weight"]), F.linear(n, P[f"{b}.attn1.to_v.weight"]), heads)
        x = F.linear(a, P[f"{b}.attn1.to_out.0.weight"], P[f"{b}.attn1.to_out.0.bias"]) + x
        q = F.linear(ln(2), P[f"{b}.attn2.to_q.weight"])
        a = ref.attention(q, F.linear(ctx, P[f"{b}.attn2.to_k.weight"]), F.linear(ctx, P[f"{b}.attn2.to_v.weight"]), heads)
        w = {nm: sd[f"{prefix}{b}.attn2.processor.{nm}.0.weight"] for nm in ("to_k_ip", "to_v_ip")}
        a = a + scale.reshape(-1, 1, 1) * ref.attention(q, F.linear(tokens, w["to_k_ip"]), F.linear(tokens, w["to_v_ip"]), heads)
        x = F.linear(a, P[f"{b}.attn2.to_out.0.weight"], P[f"{b}.attn2.to_out.0.bias"]) + x
        hid, gate = F.linear(ln(3), P[f"{b}.ff.net.0.proj.weight"], P[f"{b}.ff.net.0.proj.bias"]).chunk(2, dim=-1)
        return F.linear(hid * F.gelu(gate), P[f"{b}.ff.net.2.weight"], P[f"{b}.ff.net.2.bias"]) + x
    return block
