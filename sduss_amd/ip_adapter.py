"""Image-prompt adapter (IP-Adapter) of the SDXL UNet: a second key / value set per cross-attention layer, made from a few image tokens and
added with its own softmax and a per-row scale -- attn2(x) = softmax(q k_text^T / 8) v_text + s softmax(q k_img^T / 8) v_img.

The adapter cannot be merged into the packed weights; it is a small second blob (``ip_kv_all.<dim>.weight``, the layout of
``attn2_kv_all.<dim>.weight``) that ``MxUNet.set_ip_adapter`` hands to the library, which adds the image term inside the cross-attention launch
(mx_attention_cross_ip).  State dicts use diffusers' module-path names: ``<block>.attn2.processor.to_k_ip.0.weight`` / ``to_v_ip.0.weight``
and ``encoder_hid_proj.image_projection_layers.0.{image_embeds,norm}.{weight,bias}``, with or without a ``unet.`` prefix.  The CLIP vision
encoder is not part of this package: callers bring image embeddings (diffusers' ``ip_adapter_image_embeds``), or tokens a resampler made."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .config import UNetConfig, transformer_names

IP_KEYS = 16           # image tokens per row as the library stores them (ops.IP_KEYS)
_PROJ = "encoder_hid_proj.image_projection_layers.0."


def cross_attention_layers(cfg: UNetConfig) -> List[Tuple[str, int]]:
    """(transformer block prefix, width) of every cross-attention layer in execution order: the order ``attn2_kv_all.<dim>`` packs its layers in"""
    return [(f"{p}.transformer_blocks.{k}", dim) for p, dim, _h, layers in transformer_names(cfg) for k in range(layers)]


class IPAdapter:
    """``packed``: [(name, tensor)] of the adapter's blob; ``n_img``: image tokens per row; ``proj``: the ImageProjection's tensors, or None where the
    caller brings tokens."""

    def __init__(self, cfg: UNetConfig, packed, n_img: int, proj: Optional[Dict[str, torch.Tensor]] = None):
        self.cfg, self.packed, self.n_img, self.proj = cfg, packed, n_img, proj
        self._dev: Dict[torch.device, Dict[str, torch.Tensor]] = {}

    @classmethod
    def from_state_dict(cls, cfg: UNetConfig, sd: Dict[str, torch.Tensor], n_img: Optional[int] = None) -> "IPAdapter":
        """``n_img``: the token count of a dict without an image projection (the caller brings tokens); otherwise the projection says it"""
        sd = {(k[5:] if k.startswith("unet.") else k): v for k, v in sd.items()}
        ctx = cfg.cross_attention_dim
        by_dim: Dict[int, List[torch.Tensor]] = {}
        for b, dim in cross_attention_layers(cfg):
            kv = []
            for nm in ("to_k_ip", "to_v_ip"):
                key = f"{b}.attn2.processor.{nm}.0.weight"
                if key not in sd:
                    raise KeyError(f"image-prompt adapter lacks '{key}'")
                if tuple(sd[key].shape) != (dim, ctx):
                    raise ValueError(f"'{key}' has shape {tuple(sd[key].shape)}, expected {(dim, ctx)}")
                kv.append(sd[key])
            by_dim.setdefault(dim, []).append(torch.cat(kv, dim=0))
        packed = [(f"ip_kv_all.{dim}.weight", torch.cat(lst, dim=0).to(torch.bfloat16).contiguous()) for dim, lst in by_dim.items()]
        proj = None
        if _PROJ + "image_embeds.weight" in sd:
            w = sd[_PROJ + "image_embeds.weight"]
            if w.ndim != 2 or w.shape[0] % ctx != 0 or w.shape[0] == 0:
                raise ValueError(f"'{_PROJ}image_embeds.weight' has shape {tuple(w.shape)}, expected (n_img * {ctx}, embed_dim)")
            n_img = w.shape[0] // ctx
            proj = {"w": w.to(torch.bfloat16).contiguous()}
            for nm, key, n in (("b", "image_embeds.bias", n_img * ctx), ("gamma", "norm.weight", ctx), ("beta", "norm.bias", ctx)):
                if _PROJ + key not in sd:
                    raise KeyError(f"image-prompt adapter lacks '{_PROJ}{key}'")
                if tuple(sd[_PROJ + key].shape) != (n,):
                    raise ValueError(f"'{_PROJ}{key}' has shape {tuple(sd[_PROJ + key].shape)}, expected {(n,)}")
                proj[nm] = sd[_PROJ + key].to(torch.float32).contiguous()
        if n_img is None or not 1 <= n_img <= IP_KEYS:
            raise ValueError(f"'{_PROJ}image_embeds.weight': {n_img} image tokens; 1..{IP_KEYS} are served (a dict without a projection needs n_img)")
        return cls(cfg, packed, n_img, proj)

    def project(self, image_embeds: torch.Tensor) -> torch.Tensor:
        """image embeddings [rows, embed_dim] bf16 on the device -> tokens [rows, 16, cross_attention_dim], zero past ``n_img``: diffusers'
        ImageProjection (a linear to n_img * cross_dim, then a LayerNorm per token) on ops.gemm + ops.layernorm.  Tokens made elsewhere
        ([rows, n_img, cross_attention_dim], a Plus variant's resampler output) are only padded."""
        ctx = self.cfg.cross_attention_dim
        if image_embeds.ndim == 3:
            rows, n, c = image_embeds.shape
            if c != ctx or n != self.n_img:
                raise ValueError(f"tokens of shape {tuple(image_embeds.shape)}; expected [rows, {self.n_img}, {ctx}]")
            tok = image_embeds.to(torch.bfloat16)
        else:
            from . import ops
            if self.proj is None:
                raise ValueError("this adapter has no image projection: pass tokens [rows, n_img, cross_attention_dim]")
            dev = image_embeds.device
            if dev not in self._dev:
                self._dev[dev] = {k: v.to(dev) for k, v in self.proj.items()}
            pj = self._dev[dev]
            rows, n = image_embeds.shape[0], self.n_img
            y = ops.gemm(image_embeds.to(torch.bfloat16).contiguous(), pj["w"], bias=pj["b"])
            tok = ops.layernorm(y.view(rows * n, ctx), pj["gamma"], pj["beta"], 1e-5).view(rows, n, ctx)
        out = torch.zeros((rows, IP_KEYS, ctx), dtype=torch.bfloat16, device=tok.device)
        out[:, :n] = tok
        return out
