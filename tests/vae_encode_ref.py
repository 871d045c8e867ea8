"""fp32 torch restatement of the VAE ENCODER as diffusers runs it: ``AutoencoderKL.encode`` = ``Encoder`` + ``quant_conv`` +
``DiagonalGaussianDistribution``, then the pipelines' ``(z - shift_factor) * scaling_factor``.  A test helper (the checker of
tests/test_vae_encode_cpu.py and tests/test_vae_encode_gpu.py), with the configs and the init recipe of oracle/vae_ref.py and its own seed.

The published ``Encoder``: conv_in -> DownEncoderBlock2D per level (layers_per_block ResnetBlock2D without time embedding, the first of a level
changing width through a 1x1 conv_shortcut; between levels Downsample2D = F.pad(x, (0, 1, 0, 1)) then a 3x3 conv with stride 2 and pad 0) ->
UNetMidBlock2D (resnet, one-head attention, resnet) -> GroupNorm -> SiLU -> conv_out to 2 x latent_channels moments.

``pad1_downsample=True`` is the form the HIP plan runs on a ROTATED image with ROTATED weights: the downsampler as a plain pad-1 stride-2 conv.
Everything runs in the dtype of ``x`` (fp32 for parity, fp64 for the rotation identity)."""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from oracle.vae_ref import VAEConfig, _attention, _resnet

SEED = 52711


def param_shapes(cfg: VAEConfig) -> Dict[str, Tuple[int, ...]]:
    s: Dict[str, Tuple[int, ...]] = {}
    m = 2 * cfg.latent_channels
    c = cfg.block_out_channels[0]
    s["encoder.conv_in.weight"] = (c, cfg.out_channels, 3, 3); s["encoder.conv_in.bias"] = (c,)

    def resnet(p, cin, cout):
        s[f"{p}.norm1.weight"] = (cin,); s[f"{p}.norm1.bias"] = (cin,)
        s[f"{p}.conv1.weight"] = (cout, cin, 3, 3); s[f"{p}.conv1.bias"] = (cout,)
        s[f"{p}.norm2.weight"] = (cout,); s[f"{p}.norm2.bias"] = (cout,)
        s[f"{p}.conv2.weight"] = (cout, cout, 3, 3); s[f"{p}.conv2.bias"] = (cout,)
        if cin != cout:
            s[f"{p}.conv_shortcut.weight"] = (cout, cin, 1, 1); s[f"{p}.conv_shortcut.bias"] = (cout,)
    n = len(cfg.block_out_channels)
    for i, cout in enumerate(cfg.block_out_channels):
        for j in range(cfg.layers_per_block):
            resnet(f"encoder.down_blocks.{i}.resnets.{j}", c, cout)
            c = cout
        if i != n - 1:
            s[f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"] = (c, c, 3, 3); s[f"encoder.down_blocks.{i}.downsamplers.0.conv.bias"] = (c,)
    resnet("encoder.mid_block.resnets.0", c, c)
    a = "encoder.mid_block.attentions.0"
    s[f"{a}.group_norm.weight"] = (c,); s[f"{a}.group_norm.bias"] = (c,)
    for nm in ("to_q", "to_k", "to_v", "to_out.0"):
        s[f"{a}.{nm}.weight"] = (c, c); s[f"{a}.{nm}.bias"] = (c,)
    resnet("encoder.mid_block.resnets.1", c, c)
    s["encoder.conv_norm_out.weight"] = (c,); s["encoder.conv_norm_out.bias"] = (c,)
    s["encoder.conv_out.weight"] = (m, c, 3, 3); s["encoder.conv_out.bias"] = (m,)
    if cfg.use_post_quant_conv:
        s["quant_conv.weight"] = (m, m, 1, 1); s["quant_conv.bias"] = (m,)
    return s


def init_params(cfg: VAEConfig, seed: int = SEED) -> Dict[str, torch.Tensor]:
    """the recipe of oracle.vae_ref.init_params: seeded, bf16-representable, fan-in scaled"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in param_shapes(cfg).items():
        if name.endswith(".weight") and len(shape) > 1:
            fan = 1
            for d in shape[1:]:
                fan *= d
            t = torch.randn(shape, generator=g) * fan ** -0.5
        elif name.endswith(".weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.05 * torch.randn(shape, generator=g)
        out[name] = t.to(torch.bfloat16).to(torch.float32)
    return out


def moments(P: Dict[str, torch.Tensor], cfg: VAEConfig, x: torch.Tensor, pad1_downsample: bool = False) -> torch.Tensor:
    """images [B, 3, H, W] in [-1, 1] -> moments [B, 2 lc, H / f, W / f] (mean | logvar), in the dtype of x"""
    P = {k: v.to(x.dtype) for k, v in P.items()}
    h = F.conv2d(x, P["encoder.conv_in.weight"], P["encoder.conv_in.bias"], padding=1)
    n = len(cfg.block_out_channels)
    for i in range(n):
        for j in range(cfg.layers_per_block):
            h = _resnet(P, f"encoder.down_blocks.{i}.resnets.{j}", h, cfg)
        if i != n - 1:
            w, b = P[f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"], P[f"encoder.down_blocks.{i}.downsamplers.0.conv.bias"]
            if pad1_downsample:
                h = F.conv2d(h, w, b, stride=2, padding=1)
            else:
                h = F.conv2d(F.pad(h, (0, 1, 0, 1), mode="constant", value=0), w, b, stride=2, padding=0)
    h = _resnet(P, "encoder.mid_block.resnets.0", h, cfg)
    h = _attention(P, "encoder.mid_block.attentions.0", h, cfg)
    h = _resnet(P, "encoder.mid_block.resnets.1", h, cfg)
    h = F.silu(F.group_norm(h, cfg.norm_num_groups, P["encoder.conv_norm_out.weight"], P["encoder.conv_norm_out.bias"], cfg.norm_eps))
    h = F.conv2d(h, P["encoder.conv_out.weight"], P["encoder.conv_out.bias"], padding=1)
    if cfg.use_post_quant_conv:
        h = F.conv2d(h, P["quant_conv.weight"], P["quant_conv.bias"])
    return h


def latents(mom: torch.Tensor, cfg: VAEConfig, posterior_noise=None) -> torch.Tensor:
    """DiagonalGaussianDistribution(moments).mode() / .sample() with the caller's noise, then (z - shift_factor) * scaling_factor"""
    mean, logvar = torch.chunk(mom, 2, dim=1)
    z = mean
    if posterior_noise is not None:
        z = mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * posterior_noise.to(mom.dtype)
    return (z - cfg.shift_factor) * cfg.scaling_factor


def encode(P, cfg: VAEConfig, x: torch.Tensor, posterior_noise=None) -> torch.Tensor:
    return latents(moments(P, cfg, x), cfg, posterior_noise)


def preprocess_u8(images: torch.Tensor) -> torch.Tensor:
    """uint8 [B, H, W, 3] -> fp32 [B, 3, H, W] in [-1, 1], as image_processor.preprocess: 2 (u / 255) - 1"""
    return (2.0 * (images.permute(0, 3, 1, 2).to(torch.float32) / 255.0) - 1.0).contiguous()
