"""The caller of the model slot: one ``denoising_step`` over a heterogeneous batch of requests, mirroring
``ESyMReDStableDiffusionXLPipeline.denoising_step``
(sduss/model_executor/diffusers/pipelines/stable_diffusion_xl/pipeline_stable_diffusion_xl_esymred.py:259-403)
and the batched Euler scheduler either side of it (schedulers/scheduling_euler_discrete.py:161-274).

What stays host-side is bookkeeping (which request is at which step); the arithmetic -- input scaling with the CFG
duplication, the UNet, the CFG combine and the Euler step -- runs in libmxdenoise.so.  Text encoders and the VAE
(prepare_inference / post_inference) are out of scope and stay on stock PyTorch.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops
from .lib import MxError
from .step_state import StepCache, _upload, new_uid
from .unet import MxUNet


def euler_tables(num_inference_steps: int, num_train_timesteps: int = 1000, beta_start: float = 0.00085,
                 beta_end: float = 0.012, steps_offset: int = 1):
    """diffusers EulerDiscreteScheduler.set_timesteps for the SDXL-base scheduler config (scaled_linear betas,
    'leading' spacing, steps_offset 1, linear sigma interpolation) -- what ``batch_set_timesteps``
    (scheduling_euler_discrete.py:72-113) stores per request.  Returns (timesteps f32[n], sigmas f32[n+1], init_noise_sigma)."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
    step_ratio = num_train_timesteps // num_inference_steps
    timesteps = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.float32) + steps_offset
    sig = (((1 - alphas_cumprod) / alphas_cumprod) ** 0.5).numpy()
    sigmas = np.interp(timesteps, np.arange(0, len(sig)), sig)
    sigmas = np.concatenate([sigmas, [0.0]]).astype(np.float32)
    return timesteps, sigmas, float((sigmas.max() ** 2 + 1) ** 0.5)


def karras_tables(num_inference_steps: int, rho: float = 7.0):
    """The Karras et al. (2022) sigma schedule between the first and the last non-zero sigma of ``euler_tables(n)``, as diffusers'
    ``use_karras_sigmas`` and k-diffusion's ``get_sigmas_karras`` make it: sigma_i = (max^(1/rho) + i / (n - 1) (min^(1/rho) - max^(1/rho)))^rho in
    fp64, a final 0 appended, rounded to fp32 once; n = 1 gives the single sigma max.  The timesteps are diffusers' ``_sigma_to_t``, the position of
    log sigma among the 1000 training log sigmas by linear interpolation, left fractional (the UNet entry takes float timesteps).  Returns
    (timesteps f32[n], sigmas f32[n+1], init_noise_sigma) like ``euler_tables``; init_noise_sigma is the same, since sigma max is."""
    _ts, base, init_noise_sigma = euler_tables(num_inference_steps)
    n = num_inference_steps
    hi, lo = float(base[0]) ** (1.0 / rho), float(base[n - 1]) ** (1.0 / rho)
    ramp = np.linspace(0.0, 1.0, n) if n > 1 else np.zeros(1)
    sig = (hi + ramp * (lo - hi)) ** rho
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2       # the training sigmas of euler_tables, ascending
    alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
    log_train = np.log((((1 - alphas_cumprod) / alphas_cumprod) ** 0.5).numpy().astype(np.float64))
    log_sig = np.log(sig)
    low = np.clip(np.searchsorted(log_train, log_sig, side="right") - 1, 0, len(log_train) - 2)   # the last training sigma not above sigma
    w = np.clip((log_train[low] - log_sig) / (log_train[low] - log_train[low + 1]), 0.0, 1.0)
    timesteps = ((1.0 - w) * low + w * (low + 1)).astype(np.float32)
    return timesteps, np.concatenate([sig, [0.0]]).astype(np.float32), init_noise_sigma


@dataclass
class InpaintState:
    """What an inpainting request carries beside its latents (Denoiser.start_inpaint): after every step the kept region of the latents becomes
    ``init`` noised with ``noise`` to the step's next sigma."""
    init: torch.Tensor                    # [1, C, h, w] model dtype: the image's clean latents
    noise: torch.Tensor                   # [1, C, h, w] model dtype: the request's fixed N(0, 1) noise
    mask: torch.Tensor                    # uint8 [1, h, w] on the latent grid: 1 = repaint, 0 = keep
    image_u8: Optional[torch.Tensor]      # uint8 [1, H, W, 3]: the client's image (None when it came as floats)
    mask_u8: torch.Tensor                 # uint8 [1, H, W]: the client's mask, >= 128 = repaint
    paste: bool                           # post_inference gives the client's own pixels back outside the mask
    full_image_u8: Optional[torch.Tensor] = None   # uint8 [1, Hc, Wc, 3]: the client's whole image, of a request that repaints a crop of it
    full_mask_u8: Optional[torch.Tensor] = None    # uint8 [1, Hc, Wc]: the client's whole mask, soft (after the blur)
    region: Optional[tuple] = None                 # (x1, y1, x2, y2) of the crop in the client's image; image_u8 / mask_u8 are that crop resized
    overlay: bool = False                          # the result is blended into the client's image under the soft mask (mx_rgb8_overlay)


@dataclass
class Request:
    """The per-request state the reference keeps on RunnerRequest (worker/runner/wrappers.py:19-36)."""
    request_id: int
    resolution: int
    num_inference_steps: int
    latents: torch.Tensor                 # [1, 4, res/8, res/8] model dtype, on device
    prompt_embeds: torch.Tensor           # [1, 77, 2048]
    negative_prompt_embeds: torch.Tensor  # [1, 77, 2048]
    pooled_prompt_embeds: torch.Tensor    # [1, 1280]
    negative_pooled_prompt_embeds: torch.Tensor
    add_time_ids: torch.Tensor            # [1, 6]
    negative_add_time_ids: torch.Tensor
    timesteps: np.ndarray = None
    sigmas: np.ndarray = None
    step_index: int = 0
    arrival: float = 0.0
    start: Optional[float] = None
    finish: Optional[float] = None
    inpaint: Optional[InpaintState] = None
    sampler: str = "euler"                # "euler" | "dpmpp_2m" | "ab2" | "euler_a" | "dpmpp_2m_sde" (set_timesteps)
    history: Optional[torch.Tensor] = None   # fp32 [1, C, h, w]: D of the last step of a multistep sampler, a view of its composition's buffer
    history_step: int = -1                # the step that left ``history``; the next step is second order only if it follows it directly
    seed: Optional[int] = None            # the request's noise is a function of (seed, purpose, step, element) alone (csrc/noise.h); None: unseeded
    eta: float = 0.0                      # the noise level of a stochastic sampler (set_timesteps)

    def done(self) -> bool:
        return self.step_index >= self.num_inference_steps


@dataclass
class _Part:
    """one resolution of a step"""
    res: str
    reqs: list
    entry: object                         # its StepCache entry: .cond, .uid
    latents: torch.Tensor                 # [n, ...]
    sigma: torch.Tensor
    sigma_next: torch.Tensor
    timesteps: torch.Tensor               # one per model row ([uncond..., cond...] under CFG)
    x_in: torch.Tensor                    # the model's input rows


def start_step(num_inference_steps: int, strength: float) -> int:
    """the step an image-to-image request starts at, diffusers' ``get_timesteps``: init = min(int(steps * strength), steps),
    t_start = max(steps - init, 0).  strength 1 starts at step 0 (pure noise at the first sigma), strength 0 at ``steps`` (nothing left to do)."""
    init = min(int(num_inference_steps * strength), num_inference_steps)
    return max(num_inference_steps - init, 0)


class Denoiser:
    """One ``denoising_step`` over a heterogeneous batch of requests, for either model.  A subclass says which request fields make the
    conditioning (``_cond``), how the model input is made from the latents (``_scale_input``), which scheduler step follows
    (``flow``: the flow-match model; ``ops.cfg_step_`` picks the launch a resolution's requests need), how its model slot is called (``_forward``,
    ``_forward_mixed``) and whether a batch composition is announced to it (``announces_composition``: MxUNet.set_context_key)."""
    announces_composition = False
    flow = False                         # the flow-match model: its Euler step and the keep factor of its inpainting rows
    samplers = ("euler",)                # what set_timesteps accepts
    stochastic_samplers = ()             # those of them that draw noise every step: they need a seeded request

    def __init__(self, model, guidance_scale: float):
        self._model = model
        self.guidance_scale = guidance_scale
        self._tables: Dict[object, tuple] = {}
        self.concurrent_resolutions = True
        self._streams: List[torch.cuda.Stream] = []
        self._cache = StepCache(model.device)      # per batch composition: conditioning cats, sigma/timestep tables (step_state.py)
        self._mixed_cond: Dict[tuple, tuple] = {}  # per mixed composition: the conditioning of all resolutions concatenated

    @staticmethod
    def _cond(reqs, do_classifier_free_guidance: bool) -> tuple:
        """(encoder_hidden_states, pooled) of one resolution's requests; with CFG in the row order [uncond..., cond...]
        (pipeline_stable_diffusion_xl_esymred.py:322-339, pipeline_stable_diffusion_3_esymred.py:281-292)"""
        if do_classifier_free_guidance:
            return (torch.cat([r.negative_prompt_embeds for r in reqs] + [r.prompt_embeds for r in reqs], dim=0),
                    torch.cat([r.negative_pooled_prompt_embeds for r in reqs] + [r.pooled_prompt_embeds for r in reqs], dim=0))
        return torch.cat([r.prompt_embeds for r in reqs], dim=0), torch.cat([r.pooled_prompt_embeds for r in reqs], dim=0)

    @torch.inference_mode()
    def denoising_step(self, worker_reqs: Dict[str, list], do_classifier_free_guidance: bool = True,
                       is_sliced: bool = False, patch_size: int = 256) -> None:
        """One timestep for every request in ``worker_reqs`` ({str(res): [requests]}), in place.

        The reference runs the resolutions of a mixed batch as one patch batch, and so does this: ONE launch sequence for all of them --
        also with ESYMRED_USE_CACHE=TRUE, where the cache at its reference unit, the patch / token chunk, decides once per block for the
        patches of every resolution.  Where that does not apply (``mixed_one_sequence = False``, the per-sample cache, more resolutions than
        a sequence holds) each resolution is its own launch sequence, issued on separate streams: a small batch (one 512-1024 px request fills
        about a quarter of the CUs) leaves room for the other sequences to run beside it.  The caller's stream waits for all of them;
        ``self.concurrent_resolutions = False`` serialises them."""
        res_list = [r for r in sorted(worker_reqs.keys(), key=lambda r: int(r)) if worker_reqs[r]]       # :275-276
        m = self._model
        cache_on = getattr(m, "_block_caches", None) is not None
        cached_unit = (cache_on and is_sliced and 1 <= len(res_list) <= m.max_mixed_groups
                       and all(int(r) % patch_size == 0 and int(r) > patch_size for r in res_list))
        if cached_unit or (1 < len(res_list) <= m.max_mixed_groups and m.mixed_one_sequence and not cache_on):
            self._step(res_list, worker_reqs, do_classifier_free_guidance, is_sliced, patch_size, through_dict=cached_unit)
            return
        if len(res_list) <= 1 or not self.concurrent_resolutions:
            for res in res_list:
                self._step_resolution(res, worker_reqs[res], do_classifier_free_guidance, is_sliced, patch_size)
            return
        cur = torch.cuda.current_stream()
        fork = torch.cuda.Event()
        fork.record(cur)
        while len(self._streams) < len(res_list):
            self._streams.append(torch.cuda.Stream(device=m.device))
        for i, res in enumerate(res_list):
            side = self._streams[i]
            side.wait_event(fork)
            with torch.cuda.stream(side):
                self._step_resolution(res, worker_reqs[res], do_classifier_free_guidance, is_sliced, patch_size)
            join = torch.cuda.Event()
            join.record(side)
            cur.wait_event(join)
        for res in res_list:                       # the new latents were allocated on side streams: consumers on `cur`
            for r in worker_reqs[res]:             # (post_inference / VAE) are now known to the allocator
                r.latents.record_stream(cur)

    @staticmethod
    def _start_mix(sigma: np.float32) -> tuple:
        """(keep, sigma) of the start step's noise: latents = keep * clean + sigma * noise"""
        raise NotImplementedError

    def _check_sampler(self, sampler: str) -> None:
        if sampler not in self.samplers:
            raise MxError(f"{type(self).__name__}.set_timesteps: sampler must be one of {self.samplers}, got {sampler!r}")

    def _restart(self, req) -> None:
        """the schedule of a request that starts from an image: the sampler and sigmas its ``set_timesteps`` chose stay (the defaults for a
        request that never had one), and it forgets its history: its first step, wherever it starts, is first order"""
        if getattr(req, "sigmas", None) is None or len(req.timesteps) != req.num_inference_steps:
            self.set_timesteps(req)
        req.step_index, req.history, req.history_step = 0, None, -1

    def init_noise_sigma(self, num_inference_steps: int) -> float:
        """what N(0, 1) noise is scaled by to make a request's initial latents (the flow model: 1)"""
        return 1.0

    def seed_request(self, req, seed: int) -> None:
        """Make ``req`` a seeded request: its initial latents become init_noise_sigma times its own noise (domain 0, step 0; ops.seeded_noise), and
        every noise drawn for it later -- the start noise of image-to-image and inpainting, the step noise of a stochastic sampler -- comes from
        ``seed`` too, so its image does not depend on the batches it travels in."""
        req.seed = int(seed) & (2 ** 64 - 1)
        lat = req.latents
        req.latents = ops.seeded_noise(lat.shape, req.seed, 0, 0, dtype=lat.dtype, device=lat.device,
                                       scale=float(self.init_noise_sigma(req.num_inference_steps)))

    def _start_noise(self, req, shape, encoder) -> torch.Tensor:
        """the start / kept-region noise of a request that starts from an image: its own (domain 1) when it is seeded, torch's otherwise"""
        if getattr(req, "seed", None) is not None:
            return ops.seeded_noise(shape, [req.seed] * shape[0], 0, 1, dtype=encoder.out_dtype, device=encoder.device)
        return torch.randn(tuple(shape), device=encoder.device, dtype=encoder.out_dtype)

    def _multistep_rows(self, reqs) -> Optional[tuple]:
        """(kind per row, coefficient table [n, S, 4]) of one resolution's requests as mx_cfg_multistep_step steps them: kind 0 rows (zeros in the
        table) are the model's Euler step.  None when every request is an Euler one: the resolution then issues the plain or the masked launch.
        With a stochastic request (a kind-1 row on the device) a third member follows: (cn table [n, S], seed per row) of mx_cfg_stochastic_step,
        zeros for the rows without noise."""
        from .lib import SAMPLERS, STOCHASTIC_SAMPLERS
        names = [getattr(r, "sampler", "euler") for r in reqs]
        if all(n == "euler" for n in names):
            return None
        steps = max(len(r.timesteps) for r in reqs)
        tab = np.zeros((len(reqs), steps, 4), dtype=np.float32)
        cn, seeds = np.zeros((len(reqs), steps), dtype=np.float32), [0] * len(reqs)
        for i, (r, name) in enumerate(zip(reqs, names)):
            self._check_sampler(name)
            k = len(r.timesteps)
            if name in STOCHASTIC_SAMPLERS:
                if getattr(r, "seed", None) is None:
                    raise MxError(f"the stochastic sampler {name!r} needs a seeded request (Denoiser.seed_request)")
                five = ops.sampler_coeffs(name, r.sigmas[:k + 1], self.flow, eta=r.eta)
                tab[i, :k], cn[i, :k], seeds[i] = five[:, :4], five[:, 4], r.seed
            elif name != "euler":
                tab[i, :k] = ops.sampler_coeffs(name, r.sigmas[:k + 1], self.flow)
        kinds = [SAMPLERS["dpmpp_2m"] if n in STOCHASTIC_SAMPLERS else SAMPLERS[n] for n in names]
        if any(n in STOCHASTIC_SAMPLERS for n in names):
            return kinds, tab, (cn, seeds)
        return kinds, tab

    @staticmethod
    def _resize_client_u8(what: str, t: torch.Tensor, size, resample: str, device) -> torch.Tensor:
        """a client's uint8 image [1, H, W, 3] or mask [1, H, W] at the request's (H, W): Pillow's resize on the device (ops.resize_u8)"""
        if t.dtype != torch.uint8:
            raise MxError(f"{what}: size= resizes the client's uint8 image; a float image must come at the request's resolution")
        return ops.resize_u8(t.to(device).contiguous(), size, resample)

    def start_from_image(self, req, encoder, image: torch.Tensor, strength: float, posterior_noise: Optional[torch.Tensor] = None,
                         start_noise: Optional[torch.Tensor] = None, size=None, resample: str = "lanczos") -> None:
        """Make ``req`` an image-to-image request: it starts at step t_start = ``start_step(steps, strength)`` of its schedule from the latents of
        ``image`` (uint8 [1, H, W, 3] as a client sends it, or float [1, 3, H, W] in [-1, 1]) noised to that step's sigma.  ONE call of the
        encoder (vae.MxVAEEncoder): posterior (its mode; its sample with ``posterior_noise``), latent scaling and the start noise leave its last
        launch together.  ``start_noise``: N(0, 1) shaped as the latents; drawn here when None.  The step itself does not change: a batch already
        holds requests at different ``step_index``.  ``size`` = (H, W): the uint8 image comes at the client's size and is resized to the request's
        first, as diffusers' VaeImageProcessor.preprocess does with Pillow (``resample``: "lanczos" | "bicubic" | "bilinear"), on the device and
        to the same bytes; None: the image has the request's size already."""
        if size is not None:
            image = self._resize_client_u8("start_from_image", image, size, resample, encoder.device)
        self._restart(req)
        t_start = start_step(req.num_inference_steps, strength)
        keep, sigma = self._start_mix(np.float32(req.sigmas[t_start]))
        f = 2 ** (len(encoder.cfg.block_out_channels) - 1)
        h, w = (image.shape[1], image.shape[2]) if image.dtype == torch.uint8 else (image.shape[2], image.shape[3])
        if start_noise is None:
            start_noise = self._start_noise(req, (image.shape[0], encoder.cfg.latent_channels, h // f, w // f), encoder)
        enc = encoder.encode_images if image.dtype == torch.uint8 else encoder.encode
        req.latents = enc(image, posterior_noise=posterior_noise, start_noise=start_noise, keep=float(keep), sigma=float(sigma))
        req.step_index = t_start

    def _inpaint_start_mix(self, req, t_start: int, strength: float) -> tuple:
        """(keep, sigma) of an inpainting request's starting latents = keep * init + sigma * noise"""
        return self._start_mix(np.float32(req.sigmas[t_start]))

    def start_inpaint(self, req, encoder, image: torch.Tensor, mask: torch.Tensor, strength: float = 1.0, posterior_noise: Optional[torch.Tensor] = None,
                      noise: Optional[torch.Tensor] = None, paste: bool = False, size=None, resample: str = "lanczos", blur: float = 0.0,
                      crop_pad: Optional[int] = None, overlay: bool = False) -> None:
        """Make ``req`` an inpainting request (diffusers' 4-channel rule, for the base checkpoints): the part of ``image`` where ``mask`` (uint8
        [1, H, W] as a client sends it) is >= 128 is repainted, the rest is kept.  ``image`` as for ``start_from_image``.  ONE call of the encoder,
        with no start noise: its result, the clean latents in the model dtype, stays on the request (``req.inpaint.init``, diffusers' image_latents)
        beside the fixed ``noise`` (N(0, 1) shaped as the latents; drawn here when None) and the mask on the latent grid.  The request starts at step
        t_start = ``start_step(steps, strength)`` from init noised to that step's sigma; at strength >= 1 from pure noise (is_strength_max).  Every
        step then puts the kept region back inside its scheduler launch (``ops.cfg_step_`` with ``inpaint``).  ``paste``: post_inference returns the
        client's own pixels outside the mask, which needs the uint8 image.  ``size`` = (H, W): image and mask come at the client's size and are
        resized to the request's first (``start_from_image``), the mask as a grey image by the same filter -- diffusers' mask processor, whose
        binarisation is then the >= 128 rule on the resized mask; the request keeps the resized pair, so ``paste`` works at the request's size.

        Repainting only the masked region of a large photo, diffusers' ``padding_mask_crop`` with a blurred mask -- all on the device, to Pillow's bytes:
        ``blur`` > 0: the client's mask goes through Pillow's GaussianBlur(blur) first, at the client's size (diffusers' VaeImageProcessor.blur, which
        its user calls before the pipeline); the latent mask is then the >= 128 rule on the soft mask.
        ``overlay``: the result is blended into the client's image under the soft mask (apply_overlay: post_inference "uint8" / "pil"), where ``paste``
        cuts at 128; needs the uint8 image.
        ``crop_pad`` (implies ``overlay``): the bounding box of the soft mask (ops.mask_bbox: one 16-byte read-back here, off the step path), padded by
        ``crop_pad`` and grown to the request's aspect (ops.crop_region, diffusers' get_crop_region), is cut out of image and mask, and that pair, resized
        to the request's size (``size``, or the size of the request's latents) by ``resample``, is what the request encodes and repaints; an empty mask
        is refused.  ``req.inpaint`` keeps the client's whole image, the soft whole mask and the region, and ``vae.finish_cropped`` resizes the decoded
        image back to the region and blends it into the whole image.  Two departures from diffusers, whose pipeline is not available to compare with:
        the crop is resized straight to the request's size and the decoded image straight to the region's, both by ``resample``, where diffusers goes
        through _resize_and_fill and _resize_and_crop -- those differ by edge pixels when the integer truncation of the crop rule leaves the region's
        aspect a pixel off the request's."""
        full_image = full_mask = region = None
        if blur > 0 or crop_pad is not None or overlay:
            if image.dtype != torch.uint8 or image.ndim != 4 or image.shape[-1] != 3:
                raise MxError("start_inpaint: blur, crop_pad and overlay work on the client's uint8 [1, H, W, 3] image")
            if mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(image.shape[:3]):
                raise MxError(f"start_inpaint: expected a uint8 mask {tuple(image.shape[:3])}, got {mask.dtype} {tuple(mask.shape)}")
            image, mask = image.to(encoder.device).contiguous(), mask.to(encoder.device).contiguous()
        if blur > 0:
            mask = ops.gaussian_blur_u8(mask, blur)
        if crop_pad is not None:
            if image.shape[0] != 1:
                raise MxError("start_inpaint: crop_pad takes one image")
            overlay = True
            f = 2 ** (len(encoder.cfg.block_out_channels) - 1)
            target = tuple(int(s) for s in size) if size is not None else (f * req.latents.shape[-2], f * req.latents.shape[-1])
            box = ops.mask_bbox(mask)[0].tolist()                 # the one read-back of a request's start
            if box[2] <= box[0] or box[3] <= box[1]:
                raise MxError("start_inpaint: crop_pad needs a mask with something to repaint; this one is empty")
            region = ops.crop_region(box, mask.shape[1:], target, crop_pad)
            full_image, full_mask = image, mask
            x1, y1, x2, y2 = region
            image = ops.resize_u8(image[:, y1:y2, x1:x2].contiguous(), target, resample)
            mask = ops.resize_u8(mask[:, y1:y2, x1:x2].contiguous(), target, resample)
            size = None
        if size is not None:
            client = tuple(image.shape[:3])
            image = self._resize_client_u8("start_inpaint", image, size, resample, encoder.device)
            if mask.dtype != torch.uint8 or tuple(mask.shape) != client:
                raise MxError(f"start_inpaint: expected a uint8 mask {client}, got {mask.dtype} {tuple(mask.shape)}")
            mask = ops.resize_u8(mask.to(encoder.device).contiguous(), size, resample)
        u8 = image.dtype == torch.uint8
        if paste and not u8:
            raise MxError("start_inpaint: paste=True needs the client's uint8 [1, H, W, 3] image")
        h, w = (image.shape[1], image.shape[2]) if u8 else (image.shape[2], image.shape[3])
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (image.shape[0], h, w):
            raise MxError(f"start_inpaint: expected a uint8 mask {(image.shape[0], h, w)}, got {mask.dtype} {tuple(mask.shape)}")
        self._restart(req)
        t_start = start_step(req.num_inference_steps, strength)
        f = 2 ** (len(encoder.cfg.block_out_channels) - 1)
        init = (encoder.encode_images if u8 else encoder.encode)(image, posterior_noise=posterior_noise)
        mask_u8 = mask.to(encoder.device).contiguous()
        if noise is None:
            noise = self._start_noise(req, tuple(init.shape), encoder)
        noise = noise.to(device=encoder.device, dtype=encoder.out_dtype).contiguous()
        req.inpaint = InpaintState(init, noise, ops.mask_to_latent(mask_u8, f), image.to(encoder.device).contiguous() if u8 else None, mask_u8, paste,
                                   full_image, full_mask, region, overlay)
        req.latents = ops.inpaint_renoise(init, noise, *self._inpaint_start_mix(req, t_start, strength))
        req.step_index = t_start

    @staticmethod
    def _inpaint_rows(reqs) -> Optional[tuple]:
        """(slot, init, noise, mask) of one resolution's requests as the masked step reads them: the inpainting requests' tensors packed in batch
        order and, per batch row, its index among them or -1 (mx_inpaint_rows).  None when no request inpaints."""
        states = [getattr(r, "inpaint", None) for r in reqs]
        rows = [s for s in states if s is not None]
        if not rows:
            return None
        order = iter(range(len(rows)))
        slot = [next(order) if s is not None else -1 for s in states]
        dev = rows[0].init.device
        return (_upload(torch.tensor(slot, dtype=torch.int32), dev), torch.cat([s.init for s in rows], dim=0).contiguous(),
                torch.cat([s.noise for s in rows], dim=0).contiguous(), torch.cat([s.mask for s in rows], dim=0).contiguous())

    def _gather(self, res: str, reqs: list, do_classifier_free_guidance: bool) -> _Part:
        """the per-resolution gather of :287-339 through the per-composition cache, and the model's input rows (:357-360 + the cat of :327).
        Embeddings are fixed for a request's lifetime: one cat per batch composition, not per step."""
        here = torch.cuda.current_stream()
        for r in reqs:                                                   # latents may have been produced on another stream
            r.latents.record_stream(here)
        e = self._cache.entry((res, do_classifier_free_guidance, tuple(r.request_id for r in reqs), tuple(id(r) for r in reqs),
                               tuple(getattr(r, "sampler", "euler") for r in reqs),
                               tuple((getattr(r, "seed", None), getattr(r, "eta", 0.0)) for r in reqs)), reqs,
                              lambda: self._cond(reqs, do_classifier_free_guidance), lambda: self._inpaint_rows(reqs), lambda: self._multistep_rows(reqs))
        lat = self._cache.latents(e, reqs)
        sig, sig_next, ts = self._cache.step_scalars(e, reqs)
        return _Part(res, reqs, e, lat, sig, sig_next, torch.cat([ts, ts], dim=0) if do_classifier_free_guidance else ts,
                     self._scale_input(lat, sig, do_classifier_free_guidance))

    def _mixed_composition(self, parts: List[_Part]) -> tuple:
        """(conditioning of all resolutions concatenated, uid): rows in ascending resolution.  Lives as long as its per-resolution entries."""
        entries = [p.entry for p in parts]
        key = tuple(id(e) for e in entries)
        hit = self._mixed_cond.get(key)
        if hit is None or any(a is not b for a, b in zip(hit[0], entries)):
            cat = tuple(torch.cat([e.cond[k] for e in entries], dim=0) for k in range(len(entries[0].cond)))
            if len(self._mixed_cond) > 32:
                self._mixed_cond.clear()
            hit = self._mixed_cond[key] = (entries, cat, new_uid())
        return hit[1], hit[2]

    def _step(self, res_list: List[str], worker_reqs: Dict[str, list], do_classifier_free_guidance: bool, is_sliced: bool, patch_size: int,
              through_dict: bool) -> None:
        """The resolutions ``res_list`` in one call of the model slot.  ``through_dict``: its reference entry ``forward({res: rows}, ...)`` with
        the request ids the block-skip caches are keyed by (:369-380) -- where the per-sample cache and the unsliced rule live; else
        ``forward_mixed``, ONE launch sequence.  Conditioning rows: ascending resolution, [uncond..., cond...] inside each (:275-276, 327-339)."""
        parts = [self._gather(res, worker_reqs[res], do_classifier_free_guidance) for res in res_list]
        if len(parts) == 1:
            (cond, uid), ts = (parts[0].entry.cond, parts[0].entry.uid), parts[0].timesteps
        else:
            (cond, uid), ts = self._mixed_composition(parts), torch.cat([p.timesteps for p in parts])
        if self.announces_composition:       # the composition's text embeddings are fixed: K / V^T of all layers once per composition
            self._model.set_context_key(uid)
        if through_dict:
            out = self._forward({p.res: p.x_in for p in parts}, ts, cond, is_sliced=is_sliced, patch_size=patch_size,
                                input_indices={p.res: [str(r.request_id) for r in p.reqs] for p in parts})
            noise = [out[p.res] for p in parts]
        else:
            noise = self._forward_mixed([p.x_in for p in parts], ts, cond, patch_size // 8 if is_sliced else 0)
        g = self.guidance_scale if do_classifier_free_guidance else 0.0
        for p, nz in zip(parts, noise):
            ms, hist = p.entry.multistep, None
            if ms is not None:                                                     # a request here steps by DPM-Solver++ 2M or AB2: one launch for all samplers
                hist = self._cache.history(p.entry, p.reqs, p.latents)
                hist.record_stream(torch.cuda.current_stream())                    # like the latents, it may have been made on another stream
            ops.cfg_step_(nz, p.latents, p.sigma, p.sigma_next, g, self.flow, inpaint=p.entry.inpaint,      # :382-397; the kept region of
                          multistep=None if ms is None else (ms.kind, ms.coef, hist),                       # inpainting rows put back
                          noise=None if ms is None or ms.seed is None else (ms.cn, ms.seed, ms.nstep))      # a stochastic request: still one launch
            for i, r in enumerate(p.reqs):                                         # :399-403
                if ms is not None and ms.host_kind[i]:                             # the history travels on the request, like its latents
                    r.history, r.history_step = hist[i:i + 1], r.step_index
                r.step_index += 1
                r.latents = p.latents[i:i + 1]

    def _step_resolution(self, res: str, reqs: list, do_classifier_free_guidance: bool, is_sliced: bool, patch_size: int) -> None:
        self._step([res], {res: reqs}, do_classifier_free_guidance, is_sliced, patch_size, through_dict=True)


class SDXLDenoiser(Denoiser):
    announces_composition = True
    samplers = ("euler", "dpmpp_2m", "ab2", "euler_a", "dpmpp_2m_sde")
    stochastic_samplers = ("euler_a", "dpmpp_2m_sde")

    def __init__(self, unet: MxUNet, guidance_scale: float = 5.0):
        super().__init__(unet, guidance_scale)     # reference default (pipeline_..._esymred.py:265)
        self.unet = unet

    def set_timesteps(self, req: Request, sampler: str = "euler", schedule: str = "default", eta: float = 1.0) -> None:
        """the request's schedule and sampler.  ``sampler``: "euler" (EulerDiscreteScheduler, the default), "dpmpp_2m" (DPM-Solver++ 2M), "ab2"
        (second-order Adams-Bashforth), or the stochastic "euler_a" (k-diffusion's Euler ancestral) and "dpmpp_2m_sde" (DPM-Solver++ 2M SDE,
        midpoint), which add ``eta``-scaled noise of the request's own generator every step and so need a seeded request (``seed_request``);
        ``schedule``: "default" (``euler_tables``) or "karras" (``karras_tables``) -- "dpmpp_2m" with "karras" is what users call DPM++ 2M Karras,
        "dpmpp_2m_sde" with it DPM++ 2M SDE Karras, and the sampler gains little without the schedule."""
        self._check_sampler(sampler)
        if schedule not in ("default", "karras"):
            raise MxError(f"SDXLDenoiser.set_timesteps: schedule must be 'default' or 'karras', got {schedule!r}")
        stochastic = sampler in self.stochastic_samplers
        if stochastic and getattr(req, "seed", None) is None:
            raise MxError(f"SDXLDenoiser.set_timesteps: the stochastic sampler {sampler!r} needs a seeded request (seed_request)")
        if stochastic and not eta >= 0.0:
            raise MxError(f"SDXLDenoiser.set_timesteps: eta must not be negative, got {eta!r}")
        req.timesteps, req.sigmas = self._table(req.num_inference_steps, schedule)[:2]
        req.step_index = 0
        req.sampler, req.history, req.history_step = sampler, None, -1
        req.eta = float(eta) if stochastic else 0.0

    def init_noise_sigma(self, num_inference_steps: int) -> float:
        return self._table(num_inference_steps)[2]

    def _table(self, num_inference_steps: int, schedule: str = "default") -> tuple:
        key = num_inference_steps if schedule == "default" else (num_inference_steps, schedule)
        if key not in self._tables:
            self._tables[key] = euler_tables(num_inference_steps) if schedule == "default" else karras_tables(num_inference_steps)
        return self._tables[key]

    @staticmethod
    def _cond(reqs, do_classifier_free_guidance: bool) -> tuple:
        if do_classifier_free_guidance:          # add_time_ids are interleaved neg/pos per request in the reference (:302-305)
            tids = torch.cat([t for r in reqs for t in (r.negative_add_time_ids, r.add_time_ids)], dim=0)
        else:
            tids = torch.cat([r.add_time_ids for r in reqs], dim=0)
        return (*Denoiser._cond(reqs, do_classifier_free_guidance), tids)

    @staticmethod
    def _scale_input(lat: torch.Tensor, sig: torch.Tensor, do_classifier_free_guidance: bool) -> torch.Tensor:
        return ops.euler_scale_input(lat, sig, (2 if do_classifier_free_guidance else 1) * lat.shape[0])

    @staticmethod
    def _start_mix(sigma: np.float32) -> tuple:
        return np.float32(1.0), sigma                        # EulerDiscreteScheduler.add_noise: original + sigma * noise

    def _inpaint_start_mix(self, req, t_start: int, strength: float) -> tuple:
        if strength >= 1.0:                                  # is_strength_max: pure noise times init_noise_sigma, nothing of the image
            return np.float32(0.0), np.float32(self.init_noise_sigma(req.num_inference_steps))
        return super()._inpaint_start_mix(req, t_start, strength)

    def _forward(self, x: Dict[str, torch.Tensor], ts, cond, **kwargs) -> Dict[str, torch.Tensor]:
        ehs, pooled, tids = cond
        return self.unet.forward(x, ts, ehs, added_cond_kwargs={"text_embeds": pooled, "time_ids": tids}, return_dict=False, **kwargs)[0]

    def _forward_mixed(self, xs: List[torch.Tensor], ts, cond, gn_patch: int) -> List[torch.Tensor]:
        return self.unet.forward_mixed(xs, ts, *cond, gn_patch=gn_patch)


def _synthetic_embeds(seed: int, shared: Optional[dict], ctx_len: int, ehs_dim: int, pooled_dim: int, device, dtype) -> tuple:
    """(prompt, negative prompt, pooled, negative pooled) embeddings ~N(0,1) from ``seed``; made once per ``shared`` dict"""
    if shared is None or "pe" not in shared:
        ge = torch.Generator(device="cpu").manual_seed(seed)
        made = [torch.randn(*shape, generator=ge).to(device=device, dtype=dtype)
                for shape in ((1, ctx_len, ehs_dim), (1, ctx_len, ehs_dim), (1, pooled_dim), (1, pooled_dim))]
        if shared is None:
            return tuple(made)
        shared.update(zip(("pe", "ne", "pp", "npp"), made))
    return shared["pe"], shared["ne"], shared["pp"], shared["npp"]


def synthetic_request(rid: int, resolution: int, steps: int, cfg, denoiser: SDXLDenoiser, device, dtype=torch.bfloat16,
                      seed: int = 10086, shared: Optional[dict] = None, sampler: str = "euler", schedule: str = "default") -> Request:
    """Fixed-prompt synthetic request: embeddings ~N(0,1) from the reference seed, time ids
    (res, res, 0, 0, res, res) (pipeline_..._esymred.py:181-187), latents randn * init_noise_sigma."""
    g = torch.Generator(device="cpu").manual_seed(seed + 17 * rid)
    pe, ne, pp, npp = _synthetic_embeds(seed, shared, 77, cfg.cross_attention_dim, cfg.text_embed_dim, device, dtype)
    r = float(resolution)
    tid = torch.tensor([[r, r, 0.0, 0.0, r, r]], device=device, dtype=torch.float32)
    lat = torch.randn(1, cfg.in_channels, resolution // 8, resolution // 8, generator=g)
    lat = (lat * denoiser.init_noise_sigma(steps)).to(device=device, dtype=dtype)
    req = Request(rid, resolution, steps, lat, pe, ne, pp, npp, tid, tid.clone())
    denoiser.set_timesteps(req, sampler=sampler, schedule=schedule)
    return req
