"""FreeU references for the tests: diffusers' ``fourier_filter`` / ``apply_freeu`` restated literally (fftn, fftshift, box mask, ifftn(...).real) in
fp64, and an fp32 UNet forward that calls the oracle's own pieces and applies that function at every concatenation of up blocks 0 and 1.  The
closed form the kernel evaluates appears nowhere here."""
import torch
import torch.nn.functional as F

from oracle.sdxl_unet_ref import _gn, conv3x3, resnet_block, time_and_aug_embedding, transformer_2d


def fourier_filter(x: torch.Tensor, threshold: int, scale: float) -> torch.Tensor:
    """diffusers.utils.torch_utils.fourier_filter on [B, C, H, W], in fp64 and without the final cast"""
    x_freq = torch.fft.fftshift(torch.fft.fftn(x.double(), dim=(-2, -1)), dim=(-2, -1))
    B, C, H, W = x_freq.shape
    mask = torch.ones((B, C, H, W), dtype=torch.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    return torch.fft.ifftn(torch.fft.ifftshift(x_freq * mask, dim=(-2, -1)), dim=(-2, -1)).real


def filter_wrong_diagonal(x: torch.Tensor, scale: float) -> torch.Tensor:
    """the same filter with bin (+1, -1) scaled in place of (-1, -1): what a kernel that confuses the diagonal's conjugate would compute"""
    x_freq = torch.fft.fftn(x.double(), dim=(-2, -1))
    mask = torch.ones(x_freq.shape, dtype=torch.float64)
    for u, v in ((0, 0), (-1, 0), (0, -1), (1, -1)):
        mask[..., u % x.shape[-2], v % x.shape[-1]] = scale
    return torch.fft.ifftn(x_freq * mask, dim=(-2, -1)).real


def apply_freeu(resolution_idx: int, hidden_states: torch.Tensor, res_hidden_states: torch.Tensor, s1, s2, b1, b2):
    """diffusers.utils.torch_utils.apply_freeu (NCHW); returns new tensors"""
    if resolution_idx in (0, 1):
        s, b = (s1, b1) if resolution_idx == 0 else (s2, b2)
        half = hidden_states.shape[1] // 2
        hidden_states = torch.cat([hidden_states[:, :half] * b, hidden_states[:, half:]], dim=1)
        res_hidden_states = fourier_filter(res_hidden_states, 1, s).to(res_hidden_states.dtype)
    return hidden_states, res_hidden_states


def unet_forward(P, cfg, sample, timestep, ehs, text_embeds, time_ids, freeu=None):
    """oracle.sdxl_unet_ref.unet_forward's exact (unsliced) graph in fp32 with apply_freeu(*freeu) in front of every torch.cat of the up path"""
    P = {k: v.float() for k, v in P.items()}
    x, ctx = sample.float(), ehs.float()
    emb = time_and_aug_embedding(P, cfg, timestep, text_embeds, time_ids)
    ch, nlev = cfg.block_out_channels, len(cfg.block_out_channels)
    x = F.conv2d(x, P["conv_in.weight"], P["conv_in.bias"], padding=1)
    skips = [x]
    for i in range(nlev):
        for j in range(cfg.layers_per_block):
            x = resnet_block(P, f"down_blocks.{i}.resnets.{j}", x, emb, cfg, None)
            if cfg.down_has_attn[i]:
                x = transformer_2d(P, f"down_blocks.{i}.attentions.{j}", x, ctx, cfg.num_heads[i], cfg.transformer_layers_per_block[i], cfg, None)
            skips.append(x)
        if i != nlev - 1:
            x = conv3x3(x, P[f"down_blocks.{i}.downsamplers.0.conv.weight"], P[f"down_blocks.{i}.downsamplers.0.conv.bias"], 2, None)
            skips.append(x)
    x = resnet_block(P, "mid_block.resnets.0", x, emb, cfg, None)
    x = transformer_2d(P, "mid_block.attentions.0", x, ctx, cfg.num_heads[-1], cfg.transformer_layers_per_block[-1], cfg, None)
    x = resnet_block(P, "mid_block.resnets.1", x, emb, cfg, None)
    for i in range(nlev):
        lv = nlev - 1 - i
        for j in range(cfg.layers_per_block + 1):
            skip = skips.pop()
            if freeu is not None:
                x, skip = apply_freeu(i, x, skip, *freeu)
            x = resnet_block(P, f"up_blocks.{i}.resnets.{j}", torch.cat([x, skip], dim=1), emb, cfg, None)
            if cfg.down_has_attn[lv]:
                x = transformer_2d(P, f"up_blocks.{i}.attentions.{j}", x, ctx, cfg.num_heads[lv], cfg.transformer_layers_per_block[lv], cfg, None)
        if i != nlev - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = conv3x3(x, P[f"up_blocks.{i}.upsamplers.0.conv.weight"], P[f"up_blocks.{i}.upsamplers.0.conv.bias"], 1, None)
    x = F.silu(_gn(x, cfg.norm_num_groups, P["conv_norm_out.weight"], P["conv_norm_out.bias"], cfg.norm_eps, None))
    return conv3x3(x, P["conv_out.weight"], P["conv_out.bias"], 1, None)
