"""CLIP vision encoder behind the C ABI (``mx_clip_vision_encode``): transformers' ``CLIPVisionModelWithProjection`` together with the steps of its
``CLIPImageProcessor``, from the client's 8-bit image to ``image_embeds`` -- what a caller of the IP-Adapter (ip_adapter.py,
``Denoiser.set_image_prompt``) needs from a reference image.  OpenCLIP ViT-H/14 (heads of 80: csrc/attention_d80.hip) is the encoder of the SDXL
adapter checkpoints; ViT-L/14 (heads of 64) runs on the 64-wide attention."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import lib as _lib
from . import ops
from .model_slot import _grow_only
from .weights import PackedWeights, pack_clip_vision

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)        # transformers' OPENAI_CLIP_MEAN / OPENAI_CLIP_STD
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


@dataclass(frozen=True)
class CLIPVisionConfig:
    hidden_size: int = 1280
    intermediate_size: int = 5120
    num_hidden_layers: int = 32
    num_attention_heads: int = 16
    image_size: int = 224
    patch_size: int = 14
    hidden_act: str = "gelu"
    projection_dim: int = 1024
    layer_norm_eps: float = 1e-5
    image_mean: Tuple[float, float, float] = CLIP_MEAN
    image_std: Tuple[float, float, float] = CLIP_STD

    @staticmethod
    def vit_h_14() -> "CLIPVisionConfig":
        """OpenCLIP ViT-H/14 (laion2b): the image encoder the SDXL ``..._vit-h`` IP-Adapter checkpoints were trained with"""
        return CLIPVisionConfig()

    @staticmethod
    def vit_l_14() -> "CLIPVisionConfig":
        return CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, hidden_act="quick_gelu",
                                projection_dim=768)

    @staticmethod
    def tiny(head_dim: int = 80, hidden_act: str = "quick_gelu") -> "CLIPVisionConfig":
        return CLIPVisionConfig(hidden_size=4 * head_dim, intermediate_size=640, num_hidden_layers=2, num_attention_heads=4, image_size=56,
                                hidden_act=hidden_act, projection_dim=64)

    @property
    def tokens(self) -> int:
        return 1 + (self.image_size // self.patch_size) ** 2


def synthetic_clip_vision_params(cfg: CLIPVisionConfig, seed: int = 10086) -> Dict[str, torch.Tensor]:
    """a random state dict with transformers' names and shapes, every value exactly representable in bf16"""
    g = torch.Generator().manual_seed(seed)
    h, i, p = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size

    def r(*shape, std):
        return (torch.randn(*shape, generator=g) * std).bfloat16().float()

    P = {"vision_model.embeddings.class_embedding": r(h, std=0.5),
         "vision_model.embeddings.patch_embedding.weight": r(h, 3, p, p, std=(3 * p * p) ** -0.5),
         "vision_model.embeddings.position_embedding.weight": r(cfg.tokens, h, std=0.5),
         "visual_projection.weight": r(cfg.projection_dim, h, std=h ** -0.5)}
    norms = ["vision_model.pre_layrnorm", "vision_model.post_layernorm"]
    for l in range(cfg.num_hidden_layers):
        b = f"vision_model.encoder.layers.{l}"
        norms += [f"{b}.layer_norm1", f"{b}.layer_norm2"]
        for n, (o, k) in {"self_attn.q_proj": (h, h), "self_attn.k_proj": (h, h), "self_attn.v_proj": (h, h), "self_attn.out_proj": (h, h),
                          "mlp.fc1": (i, h), "mlp.fc2": (h, i)}.items():
            P[f"{b}.{n}.weight"] = r(o, k, std=k ** -0.5)
            P[f"{b}.{n}.bias"] = r(o, std=0.1)
    for n in norms:
        P[f"{n}.weight"] = 1.0 + r(h, std=0.1)
        P[f"{n}.bias"] = r(h, std=0.1)
    return P


class MxCLIPVision:
    """``encode(images) -> image_embeds fp32 [B, projection_dim]`` (with ``hidden_states=True``: also hidden_states[-2], bf16 [B, tokens, H])"""

    def __init__(self, cfg: CLIPVisionConfig, params: Dict[str, torch.Tensor], device="cuda:0"):
        self.cfg = cfg
        self.device = torch.device(device)
        self._lib = _lib.load()
        cc = _lib.CLIPVisionConfigC()
        cc.hidden_size, cc.intermediate_size, cc.num_hidden_layers, cc.num_attention_heads = (cfg.hidden_size, cfg.intermediate_size,
                                                                                              cfg.num_hidden_layers, cfg.num_attention_heads)
        cc.image_size, cc.patch_size, cc.projection_dim, cc.layer_norm_eps = cfg.image_size, cfg.patch_size, cfg.projection_dim, cfg.layer_norm_eps
        cc.hidden_act = {"quick_gelu": 0, "gelu": 1}[cfg.hidden_act]
        cc.image_mean, cc.image_std = (C.c_float * 3)(*cfg.image_mean), (C.c_float * 3)(*cfg.image_std)
        self._handle = self._lib.mx_clip_vision_create(C.byref(cc))
        if not self._handle:
            raise _lib.MxError("mx_clip_vision_create: " + self._lib.mx_last_error().decode())
        self.weights = PackedWeights(pack_clip_vision(cfg, params), self.device)
        _lib.check(self._lib.mx_clip_vision_set_weights(self._handle, self.weights.blob.data_ptr(), self.weights.blob.numel(), self.weights.table,
                                                        len(self.weights.names)), "mx_clip_vision_set_weights")
        self._ws = None

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            self._lib.mx_clip_vision_destroy(h)
            self._handle = None

    def workspace_bytes(self, batch: int) -> int:
        return self._lib.mx_clip_vision_workspace_bytes(self._handle, batch)

    def validate(self, batch: int) -> None:
        _lib.check(self._lib.mx_clip_vision_validate(self._handle, batch), "mx_clip_vision_validate")

    @torch.inference_mode()
    def encode(self, images: torch.Tensor, *, hidden_states: bool = False):
        """images: uint8 [B, S, S, 3] with S = image_size, already cropped; a strided view (a crop of a larger tensor) is read in place"""
        s = self.cfg.image_size
        if not (images.dtype == torch.uint8 and images.ndim == 4 and tuple(images.shape[1:]) == (s, s, 3) and images.stride(3) == 1 and images.stride(2) == 3):
            raise ValueError(f"expected uint8 [B, {s}, {s}, 3] with interleaved pixels, got {images.dtype} {tuple(images.shape)}")
        if images.device != self.device:
            images = images.to(self.device)
        b = images.shape[0]
        ws = _grow_only(vars(self), "_ws", self.workspace_bytes(b), "mx_clip_vision_workspace_bytes", self.device)
        embeds = torch.empty((b, self.cfg.projection_dim), dtype=torch.float32, device=self.device)
        hidden = torch.empty((b, self.cfg.tokens, self.cfg.hidden_size), dtype=torch.bfloat16, device=self.device) if hidden_states else None
        _lib.check(self._lib.mx_clip_vision_encode(self._handle, _lib.current_stream(), images.data_ptr(), images.stride(1), images.stride(0) if b > 1 else 0,
                                                   embeds.data_ptr(), hidden.data_ptr() if hidden is not None else None, b, ws.data_ptr(), ws.numel()),
                   "mx_clip_vision_encode")
        return (embeds, hidden) if hidden_states else embeds

    @torch.inference_mode()
    def encode_images(self, images: torch.Tensor, *, hidden_states: bool = False):
        """images: uint8 [B, H, W, 3] of any size.  CLIPImageProcessor's steps on the device: the shortest side to image_size by Pillow's bicubic
        (ops.resize_u8), the centre crop as an offset into the resized tensor, the rescale and normalisation inside the patch-embedding launch."""
        s = self.cfg.image_size
        images = images.to(self.device).contiguous()
        h, w = images.shape[1:3]
        oh, ow = (s, int(s * w / h)) if h <= w else (int(s * h / w), s)
        if (oh, ow) != (h, w):
            images = ops.resize_u8(images, (oh, ow), "bicubic")
        top, left = (oh - s) // 2, (ow - s) // 2
        return self.encode(images[:, top:top + s, left:left + s], hidden_states=hidden_states)
