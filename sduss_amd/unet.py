"""The model-slot adapter: presents ``PatchUNet.forward``'s signature
(sduss/model_executor/modules/unet.py:205-225, 521-530) over the MI355X step plan in libmxdenoise.so.

Installed where ``instantiate_pipeline`` puts ``PatchUNet(unet)``
(pipelines/stable_diffusion_xl/pipeline_stable_diffusion_xl_esymred.py:30-41) -- see INTEGRATION.md.
PyTorch is used for device memory and the current stream only; every FLOP runs in the HIP library.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import lib as _lib
from .config import UNetConfig
from .model_slot import ModelSlot, _Config
from .lora import LoraAdapter, LoraLayout, norm_params, scaled_terms
from .weights import pack


class _LoraState:
    """what MxUNet.set_adapters keeps between calls"""

    def __init__(self, norms):
        self.norms = norms          # gamma / beta of the folded LayerNorms (the blob no longer holds them)
        self.layout = None          # LoraLayout of this model's blob, built on first use
        self.active = None          # the active blob: base + the current adapter set
        self.dirty = {}             # {row range key: byte spans} the active blob differs from the base in
        self.table = None           # device memory for the merge's term table, grow-only


class MxUNet(ModelSlot):
    """Drop-in for ``PatchUNet``: ``forward(sample_dict, timestep, encoder_hidden_states, ..., added_cond_kwargs,
    return_dict=False, is_sliced, patch_size, input_indices) -> (dict,)``.

    Row order contract (same as the reference): resolutions in the dict's (ascending) order, the conditioning rows
    of all resolutions concatenated in that order (pipeline_..._esymred.py:275-276, 327-339).
    """

    ABI = "unet"
    COND = ((torch.bfloat16, (None, "cross_attention_dim")),     # encoder_hidden_states [rows, tokens, cross_attention_dim]
            (torch.bfloat16, ("text_embed_dim",)),               # text_embeds
            (torch.float32, (6,)))                               # time_ids
    GN_PATCH = True

    def __init__(self, cfg: UNetConfig, params: Dict[str, torch.Tensor], device="cuda:0"):
        cc = _lib.UNetConfigC()
        cc.in_channels, cc.out_channels = cfg.in_channels, cfg.out_channels
        cc.n_levels = len(cfg.block_out_channels)
        for i, v in enumerate(cfg.block_out_channels):
            cc.block_out_channels[i] = v
            cc.down_has_attn[i] = int(cfg.down_has_attn[i])
            cc.transformer_layers[i] = cfg.transformer_layers_per_block[i]
            cc.num_heads[i] = cfg.num_heads[i]
        cc.layers_per_block = cfg.layers_per_block
        cc.cross_attention_dim = cfg.cross_attention_dim
        cc.addition_time_embed_dim = cfg.addition_time_embed_dim
        cc.projection_class_embeddings_input_dim = cfg.projection_class_embeddings_input_dim
        cc.norm_num_groups = cfg.norm_num_groups
        cc.norm_eps, cc.transformer_norm_eps, cc.layer_norm_eps = cfg.norm_eps, cfg.transformer_norm_eps, cfg.layer_norm_eps
        super().__init__(cfg, cc, pack(cfg, params), device)
        self._lora = _LoraState(norm_params(params))
        self._next_ctx_key = 0             # set_context_key: names the batch composition of the NEXT forward only
        self.config = _Config(in_channels=cfg.in_channels, time_cond_proj_dim=None,
                              addition_time_embed_dim=cfg.addition_time_embed_dim,
                              projection_class_embeddings_input_dim=cfg.projection_class_embeddings_input_dim,
                              sample_size=128, center_input_sample=False)

    def set_context_key(self, key: int) -> None:
        """Name the batch composition of the NEXT forward (mx_unet_set_context_key): forwards announced with the same non-zero key receive
        encoder_hidden_states of identical content, so the cross-attention K / V^T of all 70 layers are projected once per composition instead
        of once per step (the reference re-concatenates and re-projects them every step: pipeline_..._esymred.py:287-339, attention.py:59-110).
        One-shot: a forward that is not announced projects as before."""
        self._next_ctx_key = int(key)

    def _take_announcement(self) -> int:
        key, self._next_ctx_key = self._next_ctx_key, 0
        return key

    _announce = set_context_key        # forward() took the key; where the call is ONE uncached sequence, that sequence gets it back

    def _before_forward(self) -> None:
        _lib.check(self._lib.mx_unet_set_context_key(self._handle, self._take_announcement()), "mx_unet_set_context_key")

    def context_stats(self):
        """(hits, misses) of the per-composition K / V^T store since the handle was created"""
        h, m = C.c_long(0), C.c_long(0)
        _lib.check(self._lib.mx_unet_context_stats(self._handle, C.byref(h), C.byref(m)), "mx_unet_context_stats")
        return h.value, m.value

    # -------------------------------------------------------------------------------------------------
    def forward_one(self, sample: torch.Tensor, timestep: torch.Tensor, encoder_hidden_states: torch.Tensor,
                    text_embeds: torch.Tensor, time_ids: torch.Tensor, gn_patch: int = 0,
                    stage: Optional[str] = None, stage_shape=None) -> torch.Tensor:
        """One launch sequence over a batch of same-resolution latents [B, C, H, W] (any of fp32/fp16/bf16)."""
        return self._one(sample, timestep, (encoder_hidden_states, text_embeds, time_ids), gn_patch, stage=stage, stage_shape=stage_shape)

    def forward_mixed(self, samples: List[torch.Tensor], timestep: torch.Tensor, encoder_hidden_states: torch.Tensor,
                      text_embeds: torch.Tensor, time_ids: torch.Tensor, gn_patch: int = 0, stage: Optional[str] = None) -> List[torch.Tensor]:
        """ONE launch sequence over the latents of several resolutions (mx_unet_forward_mixed): ``samples[g]`` is [B_g, C, H_g, W_g]; the
        conditioning rows are those of all groups concatenated in list order.  What the reference's sliced branch does by cutting every latent
        into one patch batch (unet.py:104-185, 242-260).  With ``stage`` returns that stage's NHWC activation of all groups instead
        ([sum of pixels, C], tests)."""
        return self._mixed(samples, timestep, (encoder_hidden_states, text_embeds, time_ids), gn_patch, stage=stage)

    def forward_one_cached(self, cache, sample: torch.Tensor, timestep: torch.Tensor, encoder_hidden_states: torch.Tensor,
                           text_embeds: torch.Tensor, time_ids: torch.Tensor, batch_key: int = 0, gn_patch: int = 0, row_ids=None) -> torch.Tensor:
        """forward_one through the block-skip cache (sduss_amd/block_cache.py BlockSkipCache; the reference's ESYMRED_USE_CACHE=TRUE
        path, cache_manager.py:101-161).  Approximate by design; forward_one never consults it."""
        return self._one(sample, timestep, (encoder_hidden_states, text_embeds, time_ids), gn_patch, cache=cache, batch_key=batch_key, row_ids=row_ids)

    def forward_mixed_cached(self, cache, samples: List[torch.Tensor], row_ids, timestep: torch.Tensor, encoder_hidden_states: torch.Tensor,
                             text_embeds: torch.Tensor, time_ids: torch.Tensor, gn_patch: int) -> List[torch.Tensor]:
        """forward_mixed through the block-skip cache at the reference's unit, the patch (block_cache.PatchSkipCache; mx_unet_forward_cached_mixed):
        ONE launch sequence over the latents of every resolution, one host decision per block for all their patches.  ``row_ids``: one id per
        sample in row order (request id + CFG half)."""
        return self._mixed(samples, timestep, (encoder_hidden_states, text_embeds, time_ids), gn_patch, cache=cache, row_ids=row_ids)

    def forward(self, sample: Dict[str, torch.Tensor], timestep, encoder_hidden_states: torch.Tensor,
                class_labels=None, timestep_cond=None, attention_mask=None, cross_attention_kwargs=None,
                added_cond_kwargs: Optional[dict] = None, down_block_additional_residuals=None,
                mid_block_additional_residual=None, down_intrablock_additional_residuals=None,
                encoder_attention_mask=None, return_dict: bool = True, record: bool = False, patch_size: int = None,
                is_sliced: bool = False, save_index: int = 0, input_indices: dict = None):
        # same argument contract as unet.py:229-238
        assert (class_labels is None and timestep_cond is None and attention_mask is None
                and cross_attention_kwargs is None and down_block_additional_residuals is None
                and mid_block_additional_residual is None and down_intrablock_additional_residuals is None
                and encoder_attention_mask is None)
        assert added_cond_kwargs is not None, "SDXL needs added_cond_kwargs (text_embeds, time_ids)"
        return self._route(sample, timestep, (encoder_hidden_states, added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"]),
                           is_sliced, patch_size, input_indices)

    # ---- LoRA adapters (sduss_amd/lora.py; mx_lora_merge) ---------------------------------------------
    def _point_at(self, blob: torch.Tensor) -> None:
        _lib.check(self._lib.mx_unet_set_weights(self._handle, blob.data_ptr(), blob.numel(), self.weights.table, len(self.weights.names)),
                   "mx_unet_set_weights")

    def set_adapters(self, adapters: Sequence[Tuple[LoraAdapter, float]]) -> None:
        """Serve with ``W + sum scale_i (alpha_i / r_i) B_i A_i`` from now on: ``adapters`` = [(LoraAdapter, scale), ...], an empty list = none.
        The first call allocates the ACTIVE blob as a copy of the packed weights (the base stays pristine).  Every call brings the active blob to
        exactly the state a fresh copy of the base plus ONE merge of this set has: row ranges and their derived vectors that the previous set
        changed and this one does not target are copied back from the base, then one launch (mx_lora_merge) rewrites the targeted ranges from
        the base, so sets never accumulate.  The handle is then pointed at the active blob (mx_unet_set_weights), which drops the stored
        cross-attention K / V^T and captured graphs.  Runs on the current stream.
        The set belongs to the SLOT: change it between batches, never under requests in flight (their remaining steps would run with other
        weights).  An enabled block-skip cache holds activations made with the old weights: the caller resets it (``disable_block_cache`` /
        ``enable_block_cache``)."""
        from . import ops
        st = self._lora
        if st.layout is None:
            st.layout = LoraLayout(self.cfg, self.weights.names, st.norms, self.device)
        base = self.weights.blob
        terms = scaled_terms(st.layout, adapters)
        ops.lora_merge_validate(terms, base.numel())         # refuse before anything is touched
        if not terms and st.active is None:
            return
        with torch.cuda.device(self.device):
            if st.active is None:
                st.active = base.clone()
            new = {}
            for t in terms:
                spans = [(t["w_off"] + t["row0"] * t["K"] * 2, t["rows"] * t["K"] * 2)]
                if "colsum_off" in t:
                    spans += [(t["colsum_off"] + 4 * t["row0"], 4 * t["rows"]), (t["bias_off"] + 4 * t["row0"], 4 * t["rows"])]
                new[(t["w_off"], t["row0"], t["rows"])] = spans
            for key, spans in st.dirty.items():
                if key not in new:
                    for off, nb in spans:
                        st.active[off:off + nb].copy_(base[off:off + nb])
            need = self._lib.mx_lora_table_bytes(len(terms))
            if st.table is None or st.table.numel() < need:
                st.table = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            ops.lora_merge(base, st.active, terms, table=st.table)
            st.dirty = new
        self._point_at(st.active if terms else base)

    def clear_adapters(self) -> None:
        """Serve the base weights again: the handle points back at the base blob (the active blob is kept for the next set)."""
        if self._lora.active is not None:
            self._point_at(self.weights.blob)

    def enable_block_cache(self, down, up=None, forced_after: Optional[int] = None, observe: bool = False) -> None:
        """Route forward() through the block-skip cache, one state per resolution key: what ESYMRED_USE_CACHE=TRUE does to the
        reference's model (cache_manager.py:46-50).  `down` / `up`: objects with .predict(features) (block_cache.py)."""
        from .block_cache import BlockSkipCache, FORCED_RUN_AFTER, PatchSkipCache
        fa = FORCED_RUN_AFTER if forced_after is None else forced_after
        self._install_block_cache(lambda: BlockSkipCache(down, up, forced_after=fa, observe=observe),
                                  lambda _ctx_len: PatchSkipCache(down, up, forced_after=fa))

    @property
    def add_embedding(self):  # unet.py:533-535; the pipeline only reads .linear_1.in_features
        class _L:  # noqa
            in_features = self.cfg.projection_class_embeddings_input_dim
        class _A:  # noqa
            linear_1 = _L
        return _A
