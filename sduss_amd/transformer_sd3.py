"""The model-slot adapter for SD3.5: presents ``PatchSD3Transformer2DModel.forward``'s signature
(sduss/model_executor/modules/SD3Transformer.py:60-74, 262) over the MI355X MMDiT step plan in libmxdenoise.so.
Installed where ``instantiate_pipeline`` wraps the transformer
(pipelines/stable_diffusion_3/pipeline_stable_diffusion_3_esymred.py:24-36)."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import lib as _lib
from .config import MMDiTConfig
from .model_slot import ModelSlot, _Config
from .weights import pack_mmdit


def mmdit_config_c(cfg: MMDiTConfig) -> "_lib.MMDiTConfigC":
    cc = _lib.MMDiTConfigC()
    cc.patch_size, cc.in_channels, cc.out_channels = cfg.patch_size, cfg.in_channels, cfg.out_channels
    cc.num_layers, cc.num_attention_heads = cfg.num_layers, cfg.num_attention_heads
    cc.joint_attention_dim, cc.pooled_projection_dim = cfg.joint_attention_dim, cfg.pooled_projection_dim
    cc.pos_embed_max_size, cc.norm_eps = cfg.pos_embed_max_size, cfg.norm_eps
    assert cfg.attention_head_dim == 64, "the attention kernel is built for head_dim 64"
    for i in range(cfg.num_layers):
        cc.dual_attention[i] = int(i in cfg.dual_attention_layers)
    return cc


class MxSD3Transformer(ModelSlot):
    """``forward(hidden_states: {str(res): [n,16,h,w]}, encoder_hidden_states [N,333,4096], pooled_projections [N,2048],
    timestep [N], ..., return_dict=False, is_sliced, patch_size, input_indices) -> (dict,)``.  Unlike the reference it does
    NOT mutate its input dict (the reference overwrites it with the patch embeddings, SD3Transformer.py:82-83)."""

    ABI = "mmdit"
    COND = ((torch.bfloat16, (None, "joint_attention_dim")),     # encoder_hidden_states [rows, tokens, joint_attention_dim]
            (torch.bfloat16, ("pooled_projection_dim",)))        # pooled_projections
    CACHE_CTX_LEN = True

    def __init__(self, cfg: MMDiTConfig, params: Dict[str, torch.Tensor], device="cuda:0"):
        super().__init__(cfg, mmdit_config_c(cfg), pack_mmdit(cfg, params), device)
        self.config = _Config(in_channels=cfg.in_channels, patch_size=cfg.patch_size, sample_size=cfg.sample_size,
                              joint_attention_dim=cfg.joint_attention_dim, pooled_projection_dim=cfg.pooled_projection_dim)

    def forward_one(self, latents: torch.Tensor, timestep: torch.Tensor, encoder_hidden_states: torch.Tensor,
                    pooled: torch.Tensor, stage: Optional[str] = None, stage_shape=None, cache=None, batch_key: int = 0, row_ids=None) -> torch.Tensor:
        """`cache` (sduss_amd/block_cache.py BlockSkipCache, forced_after=2) routes the step through mx_mmdit_forward_cached: the
        reference's ESYMRED_USE_CACHE=TRUE path (SD3Transformer.py:151-228).  Approximate by design; off by default."""
        return self._one(latents, timestep, (encoder_hidden_states, pooled), cache=cache, batch_key=batch_key, row_ids=row_ids,
                         stage=stage, stage_shape=stage_shape)

    def forward_mixed(self, latents, timestep: torch.Tensor, encoder_hidden_states: torch.Tensor, pooled: torch.Tensor):
        """ONE launch sequence over the latents of several resolutions (mx_mmdit_forward_mixed): ``latents[g]`` is [B_g, C, H_g, W_g]; the
        conditioning rows are those of all groups concatenated in list order (SD3Transformer.py:86 re-chunks all resolutions into one batch)."""
        return self._mixed(latents, timestep, (encoder_hidden_states, pooled))

    def forward_mixed_cached(self, cache, latents, row_ids, timestep: torch.Tensor, encoder_hidden_states: torch.Tensor, pooled: torch.Tensor, patch: int):
        """forward_mixed through the block-skip cache at the reference's unit, the token chunk (block_cache.PatchSkipCache with mmdit_ctx_len;
        mx_mmdit_forward_cached_mixed): ONE launch sequence, one host decision per joint block for the chunks of every resolution.  ``patch``: the
        patch edge in latent pixels (patch_size / 8 of the reference's call)."""
        return self._mixed(latents, timestep, (encoder_hidden_states, pooled), patch, cache=cache, row_ids=row_ids)

    def forward(self, hidden_states: Dict[str, torch.Tensor], encoder_hidden_states: torch.Tensor = None,
                pooled_projections: torch.Tensor = None, timestep: torch.Tensor = None, block_controlnet_hidden_states=None,
                joint_attention_kwargs=None, return_dict: bool = True, skip_layers=None, patch_size: int = None,
                is_sliced: bool = False, save_index: int = 0, input_indices: dict = None):
        assert block_controlnet_hidden_states is None and skip_layers is None and not joint_attention_kwargs
        return self._route(hidden_states, timestep, (encoder_hidden_states, pooled_projections), is_sliced, patch_size, input_indices)

    def enable_block_cache(self, predictor, forced_after: Optional[int] = None, observe: bool = False) -> None:
        """Route forward() through the block-skip cache, one state per resolution key (SD3Transformer.py:151-228 with
        ESYMRED_USE_CACHE=TRUE).  `predictor`: an object with .predict(features) (block_cache.py)."""
        from .block_cache import BlockSkipCache, FORCED_RUN_AFTER_SD3, PatchSkipCache
        fa = FORCED_RUN_AFTER_SD3 if forced_after is None else forced_after
        ml = min(128, self.cfg.pos_embed_max_size * self.cfg.patch_size)                                    # state rows: up to 1024 px (or the positional table)
        self._install_block_cache(lambda: BlockSkipCache(predictor, forced_after=fa, observe=observe),
                                  lambda lt: PatchSkipCache(predictor, forced_after=fa, mmdit_ctx_len=lt, max_latent=ml))
