"""The VAE behind the C ABI.  The decoder (``mx_vae_decode``, ``mx_vae_decode_rgb8``): what ``post_inference`` calls as ``self.vae.decode``
(sduss/model_executor/diffusers/pipelines/stable_diffusion_xl/pipeline_stable_diffusion_xl_esymred.py:406-463).
SURVEY.md section 8f rank 2 ("next" row): the step after the denoising loop, on the same HIP kernels as the UNet.
The encoder (``mx_vae_encode``): images -> the latents a request starts from, which ``prepare_inference`` takes from the caller (:154-168)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

from . import lib as _lib
from . import ops
from .model_slot import _grow_only
from .weights import PackedWeights, _conv_pack

PAD = 64   # latent channels are zero-padded to one K tile


@dataclass(frozen=True)
class VAEConfig:
    latent_channels: int = 4
    out_channels: int = 3
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    norm_eps: float = 1e-6
    scaling_factor: float = 0.13025
    shift_factor: float = 0.0          # SD3: decode(latents / scaling_factor + shift_factor)
    use_post_quant_conv: bool = True   # SD3's AutoencoderKL has none

    @staticmethod
    def sdxl() -> "VAEConfig":
        return VAEConfig()

    @staticmethod
    def sd3() -> "VAEConfig":
        """the 16-channel VAE of SD3 / SD3.5 (vae/config.json: scaling 1.5305, shift 0.0609, no quant convs); same decoder graph
        (pipeline_stable_diffusion_3_esymred.py:408-409)"""
        return VAEConfig(latent_channels=16, scaling_factor=1.5305, shift_factor=0.0609, use_post_quant_conv=False)

    @staticmethod
    def tiny() -> "VAEConfig":
        return VAEConfig(block_out_channels=(64, 64, 128), layers_per_block=1)

    @staticmethod
    def from_hf_json(path: str) -> "VAEConfig":
        import json
        with open(path) as f:
            c = json.load(f)
        return VAEConfig(latent_channels=c["latent_channels"], out_channels=c["out_channels"], block_out_channels=tuple(c["block_out_channels"]),
                         layers_per_block=c["layers_per_block"], norm_num_groups=c["norm_num_groups"], scaling_factor=c.get("scaling_factor", 0.18215),
                         shift_factor=c.get("shift_factor") or 0.0, use_post_quant_conv=c.get("use_post_quant_conv", True))


def pack_vae(cfg: VAEConfig, P: Dict[str, torch.Tensor]) -> List[Tuple[str, torch.Tensor]]:
    """HF-named AutoencoderKL params (decoder.* and post_quant_conv.*) -> packed tensors of the step plan (csrc/vae_sdxl.cpp)."""
    bf, f32 = torch.bfloat16, torch.float32
    out: List[Tuple[str, torch.Tensor]] = []
    lc = cfg.latent_channels
    # post_quant_conv as a padded [64, 64] linear with the latent rescaling folded in (exact: all of it is affine):
    #   W (z / s + t) + b  =  (W / s) z + (b + W t 1);   without a post_quant_conv (SD3) W = I, b = 0
    w = torch.zeros(PAD, PAD, dtype=f32); b = torch.zeros(PAD, dtype=f32)
    if cfg.use_post_quant_conv:
        w0 = P["post_quant_conv.weight"].reshape(lc, lc).to(f32); b0 = P["post_quant_conv.bias"].to(f32)
    else:
        w0 = torch.eye(lc, dtype=f32); b0 = torch.zeros(lc, dtype=f32)
    w[:lc, :lc] = w0 / cfg.scaling_factor
    b[:lc] = b0 + w0.sum(dim=1) * cfg.shift_factor
    out.append(("post_quant_conv.weight", w.to(bf))); out.append(("post_quant_conv.bias", b))
    for name, t in P.items():
        if not name.startswith("decoder."):
            continue
        if name == "decoder.conv_in.weight":
            out.append((name, _conv_pack(t, PAD).to(bf)))
        elif name == "decoder.conv_out.weight":
            w = _conv_pack(t); pad = (-w.shape[0]) % 4
            out.append((name, torch.nn.functional.pad(w, (0, 0, 0, pad)).to(bf).contiguous()))
        elif name == "decoder.conv_out.bias":
            out.append((name, torch.nn.functional.pad(t.to(f32), (0, (-t.shape[0]) % 4)).contiguous()))
        elif t.ndim == 4 and t.shape[-1] == 3:
            out.append((name, _conv_pack(t).to(bf)))
        elif t.ndim == 4:                                     # 1x1 conv_shortcut
            out.append((name, t.reshape(t.shape[0], t.shape[1]).to(bf).contiguous()))
        elif t.ndim == 2:
            out.append((name, t.to(bf).contiguous()))
        else:
            out.append((name, t.to(f32).contiguous()))
    return out


def conv_in_pack(w: torch.Tensor) -> torch.Tensor:
    """encoder.conv_in weight [N, 3, 3, 3] (O, I, kh, kw) -> [N, 32]: column (ky 3 + kx) 3 + c for the 27 taps, columns 27..31 zero (mx_conv3x3_rgb_in)"""
    n = w.shape[0]
    assert tuple(w.shape) == (n, 3, 3, 3)
    return torch.nn.functional.pad(w.permute(0, 2, 3, 1).reshape(n, 27), (0, 5)).contiguous()


def rot180(t: torch.Tensor) -> torch.Tensor:
    """rotation of the spatial grid (the last two dims) by 180 degrees"""
    return t.flip(-2, -1)


def pack_vae_encoder(cfg: VAEConfig, P: Dict[str, torch.Tensor]) -> List[Tuple[str, torch.Tensor]]:
    """HF-named AutoencoderKL params (encoder.* and quant_conv.*) -> packed tensors of the encoder plan (csrc/vae_sdxl.cpp, EncodePlan).
    The plan runs in the orientation rotated by 180 degrees, where the encoder's (0, 1, 0, 1)-padded stride-2 downsampler is a pad-1 conv:
        conv(pad(x, (0, 1, 0, 1)), w, stride 2, pad 0) == rot(conv(rot(x), rot(w), stride 2, pad 1))      (H, W even)
        conv(x, w, stride 1, pad 1)                    == rot(conv(rot(x), rot(w), stride 1, pad 1))
    so every 3x3 weight is rotated here, once; nothing is rounded that was not bf16 already.  conv_out keeps its 2 lc rows in a [64, 9 C] matrix and
    quant_conv (1x1) is a padded [64, 64] linear, so the moments sit in the first 2 lc of 64 columns."""
    bf, f32 = torch.bfloat16, torch.float32
    out: List[Tuple[str, torch.Tensor]] = []
    m = 2 * cfg.latent_channels
    assert m <= PAD
    if cfg.use_post_quant_conv:                               # (the two quant convs come and go together: SD3's AutoencoderKL has neither)
        w = torch.zeros(PAD, PAD, dtype=f32); b = torch.zeros(PAD, dtype=f32)
        w[:m, :m] = P["quant_conv.weight"].reshape(m, m).to(f32); b[:m] = P["quant_conv.bias"].to(f32)
        out.append(("quant_conv.weight", w.to(bf))); out.append(("quant_conv.bias", b))
    for name, t in P.items():
        if not name.startswith("encoder."):
            continue
        if name == "encoder.conv_in.weight":
            out.append((name, conv_in_pack(rot180(t)).to(bf)))
        elif name == "encoder.conv_out.weight":
            out.append((name, torch.nn.functional.pad(_conv_pack(rot180(t)), (0, 0, 0, PAD - m)).to(bf).contiguous()))
        elif name == "encoder.conv_out.bias":
            out.append((name, torch.nn.functional.pad(t.to(f32), (0, PAD - m)).contiguous()))
        elif t.ndim == 4 and t.shape[-1] == 3:
            out.append((name, _conv_pack(rot180(t)).to(bf)))
        elif t.ndim == 4:                                     # 1x1 conv_shortcut
            out.append((name, t.reshape(t.shape[0], t.shape[1]).to(bf).contiguous()))
        elif t.ndim == 2:
            out.append((name, t.to(bf).contiguous()))
        else:
            out.append((name, t.to(f32).contiguous()))
    return out


def _config_c(cfg: VAEConfig) -> "_lib.VAEConfigC":
    cc = _lib.VAEConfigC()
    cc.latent_channels, cc.out_channels, cc.n_levels = cfg.latent_channels, cfg.out_channels, len(cfg.block_out_channels)
    for i, v in enumerate(cfg.block_out_channels):
        cc.block_out_channels[i] = v
    cc.layers_per_block, cc.norm_num_groups, cc.norm_eps = cfg.layers_per_block, cfg.norm_num_groups, cfg.norm_eps
    return cc


class MxVAEEncoder:
    """``encode(images) -> latents`` with images fp32 [B, 3, H, W] in [-1, 1] (image_processor.preprocess) and ``encode_images(images)`` with the
    client's uint8 [B, H, W, 3]; latents [B, 4 | 16, H / 8, W / 8] in ``out_dtype`` as the denoising loop expects them: (z - shift_factor) *
    scaling_factor with z the posterior's mode, or its sample when ``posterior_noise`` (shaped and typed as the latents) is given.
    ``start_noise`` with ``keep`` / ``sigma`` (fp32 [B]): the latents leave as keep * latents + sigma * start_noise, the noise of the step an
    image-to-image request starts at, in the same launch (Denoiser.start_from_image)."""

    def __init__(self, cfg: VAEConfig, params: Dict[str, torch.Tensor], device="cuda:0", out_dtype=torch.bfloat16):
        self.cfg = cfg
        self.device = torch.device(device)
        self.out_dtype = out_dtype
        self._lib = _lib.load()
        self._handle = self._lib.mx_vae_create(C.byref(_config_c(cfg)))
        if not self._handle:
            raise _lib.MxError("mx_vae_create: " + self._lib.mx_last_error().decode())
        self.weights = PackedWeights(pack_vae_encoder(cfg, params), self.device)
        _lib.check(self._lib.mx_vae_set_weights(self._handle, self.weights.blob.data_ptr(), self.weights.blob.numel(), self.weights.table,
                                                len(self.weights.names)), "mx_vae_set_weights")
        self._ws = None

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            self._lib.mx_vae_destroy(h)
            self._handle = None

    def validate(self, batch: int, h: int, w: int) -> None:
        _lib.check(self._lib.mx_vae_encode_validate(self._handle, batch, h, w), "mx_vae_encode_validate")

    def _encode(self, image: torch.Tensor, fmt: int, b: int, h: int, w: int, posterior_noise, start_noise, keep, sigma) -> torch.Tensor:
        f = 2 ** (len(self.cfg.block_out_channels) - 1)
        ws = _grow_only(vars(self), "_ws", self._lib.mx_vae_encode_workspace_bytes(self._handle, b, h, w), "mx_vae_encode_workspace_bytes", self.device)
        out = torch.empty((b, self.cfg.latent_channels, h // f, w // f), dtype=self.out_dtype, device=self.device)
        a = _lib.VAEEncodeArgs()
        a.image, a.image_format, a.latents, a.io_dtype = image.data_ptr(), fmt, out.data_ptr(), _lib.torch_dtype_code(self.out_dtype)
        a.scaling_factor, a.shift_factor = self.cfg.scaling_factor, self.cfg.shift_factor
        keepalive = []
        for field, t in (("posterior_noise", posterior_noise), ("start_noise", start_noise)):
            if t is not None:
                if t.shape != out.shape:
                    raise _lib.MxError(f"mx_vae_encode: {field} has shape {tuple(t.shape)}, the latents {tuple(out.shape)}")
                t = t.to(device=self.device, dtype=self.out_dtype).contiguous()
                keepalive.append(t)
                setattr(a, field, t.data_ptr())
        if start_noise is not None:
            if keep is None or sigma is None:
                raise _lib.MxError("mx_vae_encode: start_noise needs keep and sigma")
            for field, t in (("keep", keep), ("sigma", sigma)):
                t = torch.as_tensor(t, dtype=torch.float32).reshape(-1).to(self.device).expand(b).contiguous()
                keepalive.append(t)
                setattr(a, field, t.data_ptr())
        _lib.check(self._lib.mx_vae_encode(self._handle, _lib.current_stream(), C.byref(a), b, h, w, ws.data_ptr(), ws.numel()), "mx_vae_encode")
        return out

    @torch.inference_mode()
    def encode(self, images: torch.Tensor, posterior_noise=None, start_noise=None, keep=None, sigma=None) -> torch.Tensor:
        x = images.to(device=self.device, dtype=torch.float32).contiguous()
        b, c, h, w = x.shape
        if c != 3:
            raise _lib.MxError(f"mx_vae_encode: expected [B, 3, H, W] images, got {tuple(x.shape)}")
        return self._encode(x, _lib.IMAGE_F32_CHW, b, h, w, posterior_noise, start_noise, keep, sigma)

    @torch.inference_mode()
    def encode_images(self, images: torch.Tensor, posterior_noise=None, start_noise=None, keep=None, sigma=None) -> torch.Tensor:
        """the client's 8-bit images, uint8 [B, H, W, 3]: the first launch reads the bytes themselves (mx_conv3x3_rgb_in)"""
        if images.dtype != torch.uint8 or images.ndim != 4 or images.shape[-1] != 3:
            raise _lib.MxError(f"mx_vae_encode: expected uint8 [B, H, W, 3] images, got {images.dtype} {tuple(images.shape)}")
        x = images.to(self.device).contiguous()
        b, h, w, _c = x.shape
        return self._encode(x, _lib.IMAGE_RGB8_HWC, b, h, w, posterior_noise, start_noise, keep, sigma)


class MxVAEDecoder:
    """``decode(latents) -> images`` with latents [B, 4 | 16, H, W] as the denoising loop leaves them (``latents / scaling_factor
    (+ shift_factor)`` of post_inference, SDXL :440 / SD3 :408, is folded into the packed weights) and images [B, 3, 8H, 8W] in [-1, 1];
    ``decode_images(latents) -> uint8 [B, 8H, 8W, 3]``, the same decode ending in the 8-bit image of image_processor.postprocess."""

    def __init__(self, cfg: VAEConfig, params: Dict[str, torch.Tensor], device="cuda:0", out_dtype=torch.float32):
        self.cfg = cfg
        self.device = torch.device(device)
        self.out_dtype = out_dtype
        self._lib = _lib.load()
        self._handle = self._lib.mx_vae_create(C.byref(_config_c(cfg)))
        if not self._handle:
            raise _lib.MxError("mx_vae_create: " + self._lib.mx_last_error().decode())
        self.weights = PackedWeights(pack_vae(cfg, params), self.device)
        _lib.check(self._lib.mx_vae_set_weights(self._handle, self.weights.blob.data_ptr(), self.weights.blob.numel(), self.weights.table,
                                                len(self.weights.names)), "mx_vae_set_weights")
        self._ws = None

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            self._lib.mx_vae_destroy(h)
            self._handle = None

    def validate(self, batch: int, h: int, w: int) -> None:
        _lib.check(self._lib.mx_vae_validate(self._handle, batch, h, w), "mx_vae_validate")

    @torch.inference_mode()
    def decode(self, latents: torch.Tensor) -> torch.Tensor:
        x = latents.contiguous()
        b, _c, h, w = x.shape
        ws = _grow_only(vars(self), "_ws", self._lib.mx_vae_workspace_bytes(self._handle, b, h, w), "mx_vae_workspace_bytes", self.device)
        f = 2 ** (len(self.cfg.block_out_channels) - 1)
        out = torch.empty((b, self.cfg.out_channels, f * h, f * w), dtype=self.out_dtype, device=self.device)
        _lib.check(self._lib.mx_vae_decode(self._handle, _lib.current_stream(), x.data_ptr(), _lib.torch_dtype_code(x.dtype), out.data_ptr(),
                                           _lib.torch_dtype_code(self.out_dtype), b, h, w, ws.data_ptr(), ws.numel()), "mx_vae_decode")
        return out

    @torch.inference_mode()
    def decode_images(self, latents: torch.Tensor) -> torch.Tensor:
        """latents -> the 8-bit images the client receives, uint8 [B, 8H, 8W, 3] on the device (mx_vae_decode_rgb8): the decoder with
        image_processor.postprocess in its last launch, rint(255 clamp(x / 2 + 0.5, 0, 1)) of the fp32 accumulator"""
        x = latents.contiguous()
        b, _c, h, w = x.shape
        ws = _grow_only(vars(self), "_ws", self._lib.mx_vae_workspace_bytes(self._handle, b, h, w), "mx_vae_workspace_bytes", self.device)
        f = 2 ** (len(self.cfg.block_out_channels) - 1)
        out = torch.empty((b, f * h, f * w, 3), dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.mx_vae_decode_rgb8(self._handle, _lib.current_stream(), x.data_ptr(), _lib.torch_dtype_code(x.dtype), out.data_ptr(),
                                                b, h, w, ws.data_ptr(), ws.numel()), "mx_vae_decode_rgb8")
        return out

    def images_to_host(self, images: Dict[str, torch.Tensor]) -> Dict[str, "numpy.ndarray"]:  # noqa: F821
        """device uint8 images per resolution -> numpy views [n, res, res, 3] into ONE grow-only pinned host buffer: non-blocking copies on
        the current stream, one event, one wait.  The views are valid until the next call."""
        need = sum(t.numel() for t in images.values())
        pin = getattr(self, "_pin", None)
        if pin is None or pin.numel() < need:
            self._pin = None
            pin = self._pin = torch.empty(max(need, 1), dtype=torch.uint8, pin_memory=True)
        if getattr(self, "_pin_event", None) is None:
            self._pin_event = torch.cuda.Event()
        host, at = {}, 0
        for res, t in images.items():
            assert t.dtype == torch.uint8 and t.is_contiguous()
            host[res] = pin[at:at + t.numel()].view(t.shape)
            host[res].copy_(t, non_blocking=True)
            at += t.numel()
        self._pin_event.record()
        self._pin_event.synchronize()
        return {res: h.numpy() for res, h in host.items()}


OUTPUT_TYPES = ("pt", "uint8", "pil")


def finish_cropped(req, decoded_row: torch.Tensor, resample: str = "lanczos") -> torch.Tensor:
    """The client-size result of a request that repainted a crop (Denoiser.start_inpaint with ``crop_pad``): ``decoded_row`` uint8 [1, res, res, 3],
    the request's decoded image, is resized to the region's (h, w) (ops.resize_u8, Pillow's bytes) and blended into the client's whole image under
    the soft whole mask (ops.rgb8_overlay, diffusers' apply_overlay with crop_coords) -> uint8 [1, H_client, W_client, 3] on the device.  Pixels
    whose soft mask is 0, everything outside the region among them, are the client's own bytes.  The resize goes straight to the region's size
    (start_inpaint's docstring: diffusers' _resize_and_crop differs by edge pixels where the region's aspect is a pixel off)."""
    s = getattr(req, "inpaint", None)
    if s is None or s.region is None:
        raise _lib.MxError("finish_cropped: the request was not started with crop_pad")
    x1, y1, x2, y2 = s.region
    if decoded_row.dtype != torch.uint8 or decoded_row.ndim != 4 or decoded_row.shape[0] != 1 or decoded_row.shape[-1] != 3:
        raise _lib.MxError(f"finish_cropped: expected the request's decoded uint8 [1, H, W, 3] image, got {decoded_row.dtype} {tuple(decoded_row.shape)}")
    small = ops.resize_u8(decoded_row.contiguous(), (y2 - y1, x2 - x1), resample)
    return ops.rgb8_overlay(small, s.full_image_u8, s.full_mask_u8, x1, y1)


def post_inference(vae: MxVAEDecoder, worker_reqs: Dict[str, list], output_type: str = "pt") -> Dict[str, object]:
    """mirror of post_inference (:406-463): gather the finished requests' latents per resolution, decode, postprocess.
      "pt"     {resolution: fp32 images [n, 3, res, res] in [0, 1]} on the device (the tensor stage);
      "uint8"  {resolution: uint8 images [n, res, res, 3]} on the device (MxVAEDecoder.decode_images); an inpainting request with
               ``inpaint.paste`` keeps the client's own pixels outside its mask (mx_rgb8_paste), one with ``inpaint.overlay`` has the client's
               image blended in under its soft mask (mx_rgb8_overlay).  A request that repainted a crop (``inpaint.region``) stays as decoded
               here, at the request's size: its result has the client's size, which a [n, res, res, 3] tensor cannot hold -- ``finish_cropped``
               makes it from this row;
      "pil"    {resolution: [PIL.Image, ...]}, the reference's default: the "uint8" images through the decoder's pinned host buffer; a request
               that repainted a crop comes back at the client's size (``finish_cropped``)."""
    if output_type not in OUTPUT_TYPES:
        raise ValueError(f"post_inference: output_type must be one of {OUTPUT_TYPES}, got {output_type!r}")
    images = {}
    for res, reqs in worker_reqs.items():
        if not reqs:
            continue
        lat = torch.cat([r.latents for r in reqs], dim=0)
        if output_type == "pt":
            images[res] = (vae.decode(lat) / 2 + 0.5).clamp(0, 1)
            continue
        images[res] = vae.decode_images(lat)
        for i, r in enumerate(reqs):       # an inpainting request that asked for it gets its own pixels back outside the mask, on the device
            s = getattr(r, "inpaint", None)
            if s is not None and s.paste:
                ops.rgb8_paste_(images[res][i:i + 1], s.image_u8, s.mask_u8)
            if s is not None and s.overlay and s.region is None:
                with torch.inference_mode():                               # (the decoder's images are inference tensors)
                    images[res][i:i + 1] = ops.rgb8_overlay(images[res][i:i + 1], s.image_u8, s.mask_u8)
    if output_type == "pil":
        from PIL import Image
        full = {(res, i): finish_cropped(r, images[res][i:i + 1]) for res, reqs in worker_reqs.items() for i, r in enumerate(reqs)
                if getattr(getattr(r, "inpaint", None), "region", None) is not None}
        pil = {res: [Image.fromarray(a) for a in arr] for res, arr in vae.images_to_host(images).items()}       # (an RGB fromarray copies)
        for (res, i), t in full.items():                                   # a size of its own: a copy of its own
            pil[res][i] = Image.fromarray(t[0].cpu().numpy())
        return pil
    return images
