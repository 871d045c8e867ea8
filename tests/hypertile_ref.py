"""HyperTile reference for the tests: the oracle's UNet graph with HyperTile's two rearranges around every self-attention (tfernd/HyperTile,
``swap_size=1, scale_depth=False``), in plain torch.  The windows are made by reshape / permute, as upstream's einops patterns do; the kernel's row
arithmetic appears nowhere here."""
import torch
import torch.nn.functional as F

from oracle.sdxl_unet_ref import _gn, attention, conv3x3, resnet_block, time_and_aug_embedding


def divisor(n, tile):
    """HyperTile's random_divisor(n, tile, swap_size=1): the smallest divisor of n that is >= min(tile, n)"""
    return [d for d in range(1, n + 1) if n % d == 0 and d >= min(tile, n)][0]


def to_windows(x, gh, gw, wh, ww):
    """rearrange(x, "b (nh h nw w) c -> (b nh nw) (h w) c", h=wh, w=ww)"""
    b, _, c = x.shape
    return x.reshape(b, gh // wh, wh, gw // ww, ww, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, wh * ww, c)


def from_windows(x, b, gh, gw, wh, ww):
    """rearrange(x, "(b nh nw) (h w) c -> b (nh h nw w) c")"""
    c = x.shape[-1]
    return x.reshape(b, gh // wh, gw // ww, wh, ww, c).permute(0, 1, 3, 2, 4, 5).reshape(b, gh * gw, c)


def _block(P, b, x, ctx, heads, cfg, win):
    """oracle.sdxl_unet_ref.basic_transformer_block with attn1 per window; win = (gh, gw, wh, ww) or None"""
    dim, eps = x.shape[-1], cfg.layer_norm_eps
    ln = lambda t, k: F.layer_norm(t, (dim,), P[f"{b}.norm{k}.weight"], P[f"{b}.norm{k}.bias"], eps)      # noqa: E731
    n = ln(x, 1) if win is None else to_windows(ln(x, 1), *win)
    a = attention(*(F.linear(n, P[f"{b}.attn1.to_{k}.weight"]) for k in "qkv"), heads)
    a = F.linear(a, P[f"{b}.attn1.to_out.0.weight"], P[f"{b}.attn1.to_out.0.bias"])
    x = (a if win is None else from_windows(a, x.shape[0], *win)) + x
    a = attention(F.linear(ln(x, 2), P[f"{b}.attn2.to_q.weight"]), F.linear(ctx, P[f"{b}.attn2.to_k.weight"]), F.linear(ctx, P[f"{b}.attn2.to_v.weight"]), heads)
    x = F.linear(a, P[f"{b}.attn2.to_out.0.weight"], P[f"{b}.attn2.to_out.0.bias"]) + x
    hid, gate = F.linear(ln(x, 3), P[f"{b}.ff.net.0.proj.weight"], P[f"{b}.ff.net.0.proj.bias"]).chunk(2, dim=-1)
    return F.linear(hid * F.gelu(gate), P[f"{b}.ff.net.2.weight"], P[f"{b}.ff.net.2.bias"]) + x


def _transformer(P, p, x, ctx, heads, layers, cfg, level, tile_tokens, max_depth):
    n, c, h, w = x.shape
    win = None
    if tile_tokens and level <= max_depth:
        wh, ww = divisor(h, tile_tokens), divisor(w, tile_tokens)
        win = (h, w, wh, ww) if (wh, ww) != (h, w) and ww % 16 == 0 else None
    y = _gn(x, cfg.norm_num_groups, P[f"{p}.norm.weight"], P[f"{p}.norm.bias"], cfg.transformer_norm_eps, None)
    y = F.linear(y.permute(0, 2, 3, 1).reshape(n, h * w, c), P[f"{p}.proj_in.weight"], P[f"{p}.proj_in.bias"])
    for k in range(layers):
        y = _block(P, f"{p}.transformer_blocks.{k}", y, ctx, heads, cfg, win)
    y = F.linear(y, P[f"{p}.proj_out.weight"], P[f"{p}.proj_out.bias"])
    return y.reshape(n, h, w, c).permute(0, 3, 1, 2) + x


def unet_forward(P, cfg, sample, timestep, ehs, text_embeds, time_ids, tile_size=0, max_depth=2, dtype=torch.float32):
    """oracle.sdxl_unet_ref.unet_forward's exact (unsliced) graph in ``dtype`` with HyperTile at ``tile_size`` pixels (0: the plain graph)"""
    P = {k: v.to(dtype) for k, v in P.items()}
    x, ctx = sample.to(dtype), ehs.to(dtype)
    tokens = max(tile_size // 8, 4) if tile_size else 0
    emb = time_and_aug_embedding(P, cfg, timestep, text_embeds, time_ids)
    nlev = len(cfg.block_out_channels)
    xf = lambda p, x, lv: _transformer(P, p, x, ctx, cfg.num_heads[lv], cfg.transformer_layers_per_block[lv], cfg, lv, tokens, max_depth)      # noqa: E731
    x = F.conv2d(x, P["conv_in.weight"], P["conv_in.bias"], padding=1)
    skips = [x]
    for i in range(nlev):
        for j in range(cfg.layers_per_block):
            x = resnet_block(P, f"down_blocks.{i}.resnets.{j}", x, emb, cfg, None)
            if cfg.down_has_attn[i]:
                x = xf(f"down_blocks.{i}.attentions.{j}", x, i)
            skips.append(x)
        if i != nlev - 1:
            x = conv3x3(x, P[f"down_blocks.{i}.downsamplers.0.conv.weight"], P[f"down_blocks.{i}.downsamplers.0.conv.bias"], 2, None)
            skips.append(x)
    x = resnet_block(P, "mid_block.resnets.0", x, emb, cfg, None)
    x = xf("mid_block.attentions.0", x, nlev - 1)
    x = resnet_block(P, "mid_block.resnets.1", x, emb, cfg, None)
    for i in range(nlev):
        lv = nlev - 1 - i
        for j in range(cfg.layers_per_block + 1):
            x = resnet_block(P, f"up_blocks.{i}.resnets.{j}", torch.cat([x, skips.pop()], dim=1), emb, cfg, None)
            if cfg.down_has_attn[lv]:
                x = xf(f"up_blocks.{i}.attentions.{j}", x, lv)
        if i != nlev - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = conv3x3(x, P[f"up_blocks.{i}.upsamplers.0.conv.weight"], P[f"up_blocks.{i}.upsamplers.0.conv.bias"], 1, None)
    x = F.silu(_gn(x, cfg.norm_num_groups, P["conv_norm_out.weight"], P["conv_norm_out.bias"], cfg.norm_eps, None))
    return conv3x3(x, P["conv_out.weight"], P["conv_out.bias"], 1, None)
