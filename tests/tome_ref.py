"""Token-merging references for the tests: the rule of ToMe for Stable Diffusion with the deterministic destination choice (tomesd ``use_rand=False``)
restated in plain torch, fp64 by default -- destination / source sets, match, select, merge, unmerge -- and a UNet forward over the oracle's own pieces
whose self-attention runs on the merged sequence.  Index arithmetic is by boolean masks and sorts; the closed forms of the kernels appear nowhere here."""
import torch
import torch.nn.functional as F

from oracle.sdxl_unet_ref import _gn, attention, conv3x3, resnet_block, time_and_aug_embedding


def sets(h, w, sy, sx):
    """(dst tokens, src tokens), both ascending: the top-left token of every sy x sx cell is a destination"""
    is_dst = torch.zeros(h, w, dtype=torch.bool)
    is_dst[::sy, ::sx] = True
    tok = torch.arange(h * w).reshape(h, w)
    return tok[is_dst], tok[~is_dst]


def sizes(h, w, sy, sx, ratio):
    """(Ndst, Nsrc, r, Lm); r = 0 where the level runs unmerged"""
    L = h * w
    if h % sy or w % sx or sy * sx < 2:
        return 0, 0, 0, L
    ndst = (h // sy) * (w // sx)
    r = min(L - ndst, int(L * ratio))
    r = max(0, L - -(-(L - r) // 64) * 64)            # lowered until Lm is a multiple of 64
    return ndst, L - ndst, r, L - r


def scores(x, h, w, sy, sx, dtype=torch.float64):
    """cosine of every source against every destination, [B, Nsrc, Ndst]; a zero row scores 0"""
    dst, src = sets(h, w, sy, sx)
    x = x.to(dtype)
    nrm = x.norm(dim=-1, keepdim=True)
    m = torch.where(nrm > 0, x / nrm, torch.zeros_like(x))
    return m[:, src] @ m[:, dst].transpose(1, 2)


def match(x, h, w, sy, sx, dtype=torch.float64):
    """(node_max, node_idx): equal scores pick the lower destination ordinal"""
    s = scores(x, h, w, sy, sx, dtype)
    node_max = s.max(dim=-1).values
    first = ((s == node_max[..., None]) * torch.arange(s.shape[-1], 0, -1)).argmax(dim=-1)
    return node_max, first.to(torch.int32)


def select(node_max, node_idx, h, w, sy, sx, r):
    """(row_of [B, L], unm_src [B, Nsrc - r], dst_start [B, Ndst + 1], dst_src [B, r]) int32: the r sources with the largest node_max are merged, equal
    values the lower ordinal first; unmerged sources keep ascending token order and come first, then all destinations"""
    dst, src = sets(h, w, sy, sx)
    B, nsrc = node_max.shape
    n_unm = nsrc - r
    out = [[], [], [], []]
    for b in range(B):
        order = torch.sort(-node_max[b].double(), stable=True).indices
        merged = torch.zeros(nsrc, dtype=torch.bool)
        merged[order[:r]] = True
        row_of = torch.empty(h * w, dtype=torch.int64)
        row_of[src[~merged]] = torch.arange(n_unm)
        row_of[dst] = n_unm + torch.arange(len(dst))
        row_of[src[merged]] = n_unm + node_idx[b][merged].long()
        lists = [src[merged & (node_idx[b] == j)] for j in range(len(dst))]
        start = torch.tensor([0] + [len(v) for v in lists]).cumsum(0)
        for o, v in zip(out, (row_of, src[~merged], start, torch.cat(lists) if r else torch.zeros(0, dtype=torch.int64))):
            o.append(v.to(torch.int32))
    return tuple(torch.stack(o) for o in out)


def merge(x, tables, h, w, sy, sx, eps=None):
    """[B, Lm, C] fp64: unmerged sources, then every destination as the mean of itself and its merged sources; eps: LayerNorm without affine first"""
    _, unm_src, dst_start, dst_src = tables
    dst = sets(h, w, sy, sx)[0]
    x = x.double()
    if eps is not None:
        x = F.layer_norm(x, x.shape[-1:], eps=eps)
    rows = []
    for b in range(x.shape[0]):
        d = [x[b, [int(t)] + dst_src[b, dst_start[b, j]:dst_start[b, j + 1]].tolist()].mean(dim=0) for j, t in enumerate(dst)]
        rows.append(torch.cat([x[b, unm_src[b].long()], torch.stack(d)]))
    return torch.stack(rows)


def unmerge(o, tables, residual=None):
    y = torch.stack([o[b].double()[tables[0][b].long()] for b in range(o.shape[0])])
    return y if residual is None else residual.double() + y


def _block(P, b, x, ctx, heads, cfg, hw, tome, dtype):
    """oracle.sdxl_unet_ref.basic_transformer_block with attn1 on the merged sequence (tomesd: merge_attn only)"""
    dim, eps = x.shape[-1], cfg.layer_norm_eps
    ln = lambda t, k: F.layer_norm(t, (dim,), P[f"{b}.norm{k}.weight"], P[f"{b}.norm{k}.bias"], eps)      # noqa: E731
    n, tables = ln(x, 1), None
    if tome is not None and sizes(*hw, tome["sy"], tome["sx"], tome["ratio"])[2] > 0:
        g = (*hw, tome["sy"], tome["sx"])
        tables = select(*match(x, *g, dtype=dtype), *g, sizes(*g, tome["ratio"])[2])
        n = merge(n, tables, *g).to(x.dtype)
    a = attention(*(F.linear(n, P[f"{b}.attn1.to_{k}.weight"]) for k in "qkv"), heads)
    a = F.linear(a, P[f"{b}.attn1.to_out.0.weight"], P[f"{b}.attn1.to_out.0.bias"])
    x = (a if tables is None else unmerge(a, tables).to(x.dtype)) + x
    a = attention(F.linear(ln(x, 2), P[f"{b}.attn2.to_q.weight"]), F.linear(ctx, P[f"{b}.attn2.to_k.weight"]), F.linear(ctx, P[f"{b}.attn2.to_v.weight"]), heads)
    x = F.linear(a, P[f"{b}.attn2.to_out.0.weight"], P[f"{b}.attn2.to_out.0.bias"]) + x
    hid, gate = F.linear(ln(x, 3), P[f"{b}.ff.net.0.proj.weight"], P[f"{b}.ff.net.0.proj.bias"]).chunk(2, dim=-1)
    return F.linear(hid * F.gelu(gate), P[f"{b}.ff.net.2.weight"], P[f"{b}.ff.net.2.bias"]) + x


def _transformer(P, p, x, ctx, heads, layers, cfg, level, tome, dtype):
    n, c, h, w = x.shape
    on = tome is not None and 2 ** level <= tome["max_downsample"]
    y = _gn(x, cfg.norm_num_groups, P[f"{p}.norm.weight"], P[f"{p}.norm.bias"], cfg.transformer_norm_eps, None)
    y = F.linear(y.permute(0, 2, 3, 1).reshape(n, h * w, c), P[f"{p}.proj_in.weight"], P[f"{p}.proj_in.bias"])
    for k in range(layers):
        y = _block(P, f"{p}.transformer_blocks.{k}", y, ctx, heads, cfg, (h, w), tome if on else None, dtype)
    y = F.linear(y, P[f"{p}.proj_out.weight"], P[f"{p}.proj_out.bias"])
    return y.reshape(n, h, w, c).permute(0, 3, 1, 2) + x


def unet_forward(P, cfg, sample, timestep, ehs, text_embeds, time_ids, tome=None, dtype=torch.float32):
    """oracle.sdxl_unet_ref.unet_forward's exact (unsliced) graph in ``dtype`` with token merging ``tome`` = dict(ratio, sx, sy, max_downsample) around
    every self-attention; the match runs in ``dtype`` too (bf16: what a stock bf16 pipeline with tomesd computes)"""
    P = {k: v.to(dtype) for k, v in P.items()}
    x, ctx = sample.to(dtype), ehs.to(dtype)
    emb = time_and_aug_embedding(P, cfg, timestep, text_embeds, time_ids)
    nlev = len(cfg.block_out_channels)
    xf = lambda p, x, lv: _transformer(P, p, x, ctx, cfg.num_heads[lv], cfg.transformer_layers_per_block[lv], cfg, lv, tome, dtype)      # noqa: E731
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
