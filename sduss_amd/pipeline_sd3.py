"""SD3.5 caller of the model slot: ``denoising_step`` mirroring ``ESyMReDStableDiffusion3Pipeline.denoising_step``
(sduss/model_executor/diffusers/pipelines/stable_diffusion_3/pipeline_stable_diffusion_3_esymred.py:231-388) with the
batched flow-match Euler step (schedulers/scheduling_flow_match_euler_discrete.py:159-202).  Host side = bookkeeping only."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops
from .lib import MxError
from .pipeline import Denoiser, InpaintState, _synthetic_embeds
from .transformer_sd3 import MxSD3Transformer


def flow_match_tables(num_inference_steps: int, num_train_timesteps: int = 1000, shift: float = 3.0):
    """diffusers FlowMatchEulerDiscreteScheduler.set_timesteps (SD3.5 scheduler config: shift 3.0, no dynamic shifting).
    Returns (timesteps f32[n], sigmas f32[n+1])."""
    base = np.linspace(1, num_train_timesteps, num_train_timesteps, dtype=np.float32)[::-1].copy() / num_train_timesteps
    base = shift * base / (1 + (shift - 1) * base)
    sigma_max, sigma_min = float(base[0]), float(base[-1])
    timesteps = np.linspace(sigma_max * num_train_timesteps, sigma_min * num_train_timesteps, num_inference_steps)
    sigmas = timesteps / num_train_timesteps
    sigmas = shift * sigmas / (1 + (shift - 1) * sigmas)
    timesteps = (sigmas * num_train_timesteps).astype(np.float32)
    sigmas = np.concatenate([sigmas, [0.0]]).astype(np.float32)
    return timesteps, sigmas


@dataclass
class SD3Request:
    request_id: int
    resolution: int
    num_inference_steps: int
    latents: torch.Tensor                 # [1, 16, res/8, res/8]
    prompt_embeds: torch.Tensor           # [1, 333, 4096]
    negative_prompt_embeds: torch.Tensor
    pooled_prompt_embeds: torch.Tensor    # [1, 2048]
    negative_pooled_prompt_embeds: torch.Tensor
    timesteps: np.ndarray = None
    sigmas: np.ndarray = None
    step_index: int = 0
    arrival: float = 0.0
    start: Optional[float] = None
    finish: Optional[float] = None
    inpaint: Optional[InpaintState] = None
    sampler: str = "euler"                # "euler" | "ab2" (set_timesteps)
    history: Optional[torch.Tensor] = None   # fp32 [1, C, h, w]: the model output of the last AB2 step, a view of its composition's buffer
    history_step: int = -1                # the step that left ``history``

    def done(self) -> bool:
        return self.step_index >= self.num_inference_steps


class SD3Denoiser(Denoiser):
    """``denoising_step`` as SDXLDenoiser's (pipeline.Denoiser), with the flow-match step and no input scaling."""

    def __init__(self, transformer: MxSD3Transformer, guidance_scale: float = 7.0):
        super().__init__(transformer, guidance_scale)     # reference default (pipeline_stable_diffusion_3_esymred.py:236)
        self.transformer = transformer

    flow = True
    samplers = ("euler", "ab2")

    def set_timesteps(self, req: SD3Request, sampler: str = "euler", schedule: str = "default") -> None:
        """the request's schedule and sampler: "euler" (the flow-match Euler step, the default) or "ab2" (second-order Adams-Bashforth in sigma).
        DPM-Solver++ 2M is refused on the flow model: its log-SNR is -infinity at sigma = 1, and on the analytic Gaussian problem it is worse
        than Euler at every step count.  The Karras schedule is defined for the epsilon model's sigma range only."""
        if sampler == "dpmpp_2m":
            raise MxError("SD3Denoiser.set_timesteps: dpmpp_2m is refused on the flow model (log-SNR is -infinity at sigma = 1; worse than Euler "
                          "on the analytic problem); use 'ab2'")
        self._check_sampler(sampler)
        if schedule != "default":
            raise MxError(f"SD3Denoiser.set_timesteps: the flow model has one schedule; {schedule!r} is for SDXL")
        if req.num_inference_steps not in self._tables:
            self._tables[req.num_inference_steps] = flow_match_tables(req.num_inference_steps)
        req.timesteps, req.sigmas = self._tables[req.num_inference_steps]
        req.step_index = 0
        req.sampler, req.history, req.history_step = sampler, None, -1

    @staticmethod
    def _scale_input(lat: torch.Tensor, sig: torch.Tensor, do_classifier_free_guidance: bool) -> torch.Tensor:
        if do_classifier_free_guidance:
            return ops.euler_scale_input(lat, torch.zeros_like(sig), 2 * lat.shape[0])  # exact x/1 copy == torch.cat([latents] * 2)
        return lat

    @staticmethod
    def _start_mix(sigma: np.float32) -> tuple:
        return np.float32(1.0) - sigma, sigma                # FlowMatchEulerDiscreteScheduler.scale_noise: (1 - sigma) * sample + sigma * noise


    def _forward(self, x: Dict[str, torch.Tensor], ts, cond, **kwargs) -> Dict[str, torch.Tensor]:
        ehs, pooled = cond
        return self.transformer.forward(x, encoder_hidden_states=ehs, pooled_projections=pooled, timestep=ts, return_dict=False, **kwargs)[0]   # :312-322

    def _forward_mixed(self, xs: List[torch.Tensor], ts, cond, gn_patch: int) -> List[torch.Tensor]:
        return self.transformer.forward_mixed(xs, ts, *cond)


def synthetic_sd3_request(rid: int, resolution: int, steps: int, cfg, denoiser: SD3Denoiser, device, dtype=torch.bfloat16,
                          seed: int = 10086, shared: Optional[dict] = None, ctx_len: int = 333, sampler: str = "euler",
                          schedule: str = "default") -> SD3Request:
    g = torch.Generator(device="cpu").manual_seed(seed + 17 * rid)
    pe, ne, pp, npp = _synthetic_embeds(seed, shared, ctx_len, cfg.joint_attention_dim, cfg.pooled_projection_dim, device, dtype)
    lat = torch.randn(1, cfg.in_channels, resolution // 8, resolution // 8, generator=g).to(device=device, dtype=dtype)
    req = SD3Request(rid, resolution, steps, lat, pe, ne, pp, npp)
    denoiser.set_timesteps(req, sampler=sampler, schedule=schedule)
    return req
