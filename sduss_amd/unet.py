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
from .weights import PackedWeights, pack


def config_c(cfg: UNetConfig) -> "_lib.UNetConfigC":
    """mx_unet_config of ``cfg``"""
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
    return cc


def hypertile_windows(cfg: UNetConfig, state: Optional[Tuple[int, int]], H_lat: int, W_lat: int) -> list:
    """MxUNet.hypertile_windows for ``state`` = (tile_tokens, max_depth) or None (off): the step plan's rule (mx_unet_set_hypertile), host only"""
    def divisor(n, tile):                      # HyperTile's random_divisor with swap_size = 1: the smallest divisor of n that is >= min(tile, n)
        return next(d for d in range(min(tile, n), n + 1) if n % d == 0)
    out = []
    last = len(cfg.down_has_attn) - 1
    for depth, has_attn in enumerate(cfg.down_has_attn):
        if not has_attn and depth != last:     # (the mid block attends at the last level whatever its down block does)
            continue
        gh, gw = H_lat >> depth, W_lat >> depth
        win = None
        if state and depth <= state[1]:
            wh, ww = divisor(gh, state[0]), divisor(gw, state[0])
            if (wh < gh or ww < gw) and ww % 16 == 0:
                win = (gh, gw, wh, ww)
        out.append(win)
    return out


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
        super().__init__(cfg, config_c(cfg), pack(cfg, params), device)
        self._lora = _LoraState(norm_params(params))
        self._next_ctx_key = 0             # set_context_key: names the batch composition of the NEXT forward only
        self._ip = None                    # set_ip_adapter: (IPAdapter, its PackedWeights on the device)
        self._ip_next = None               # set_image_tokens: (tokens, scales) of the NEXT forward only, handed over right before its launches
        self._ip_live = None
        self._mass_next = None             # set_attention_mass: (mass, mask, rows) of the NEXT forward only
        self._mass_live = None
        self._regions_next = None          # set_regions: (counts, weights per grid, seg_len, n_sets) of the NEXT forward only
        self._regions_live = None
        self._freeu_on = False             # enable_freeu
        self._tome = None                  # enable_tome: (ratio, sx, sy, max_downsample) while on
        self._hypertile = None             # enable_hypertile: (tile_tokens, max_depth) while on
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

    def _take_announcement(self) -> tuple:
        """(context key, image tokens, attention-mass buffers, regions) announced for the next forward, all one-shot"""
        announced = (self._next_ctx_key, self._ip_next, self._mass_next, self._regions_next)
        self._next_ctx_key, self._ip_next, self._mass_next, self._regions_next = 0, None, None, None
        return announced

    def _announce(self, announced) -> None:      # forward() took them; where the call is ONE uncached sequence, that sequence gets them back
        self._next_ctx_key, self._ip_next, self._mass_next, self._regions_next = announced

    def _hand_regions(self, rg, rows: int) -> None:
        if rg is not None:
            counts, tables, seg_len, n_sets = rg
            if counts.numel() != rows:
                raise _lib.MxError(f"regions of {counts.numel()} rows announced for a forward of {rows} rows")
            ptrs = (C.c_void_p * len(tables))(*[t.data_ptr() for t in tables])
            _lib.check(self._lib.mx_unet_set_regions(self._handle, n_sets, seg_len, counts.data_ptr(), ptrs, len(tables)), "mx_unet_set_regions")
            self._regions_live = rg        # alive until the next announcement, like the image tokens

    def _hand_attention_mass(self, am, rows: int) -> None:
        if am is not None:
            if am[2] > rows:
                raise _lib.MxError(f"the attention mass of {am[2]} rows announced for a forward of {rows} rows")
            _lib.check(self._lib.mx_unet_set_attn_mass(self._handle, am[0].data_ptr(), am[1].data_ptr(), am[2]), "mx_unet_set_attn_mass")
            self._mass_live = am           # alive until the next announcement, like the image tokens

    def _hand_image_tokens(self, ip, rows: int) -> None:
        if ip is not None:
            if ip[0].shape[0] != rows:
                raise _lib.MxError(f"image tokens of {ip[0].shape[0]} rows announced for a forward of {rows} rows")
            _lib.check(self._lib.mx_unet_set_image_tokens(self._handle, ip[0].data_ptr(), ip[1].data_ptr()), "mx_unet_set_image_tokens")
            self._ip_live = ip             # alive until the next announcement: the forward that reads them has been issued by then

    def _before_forward(self, rows: int) -> None:
        key, ip, am, rg = self._take_announcement()
        _lib.check(self._lib.mx_unet_set_context_key(self._handle, key), "mx_unet_set_context_key")
        self._hand_image_tokens(ip, rows)
        self._hand_attention_mass(am, rows)
        self._hand_regions(rg, rows)

    def _before_trace(self, rows: int) -> None:
        ip, self._ip_next = self._ip_next, None
        am, self._mass_next = self._mass_next, None
        rg, self._regions_next = self._regions_next, None
        self._hand_image_tokens(ip, rows)
        self._hand_attention_mass(am, rows)
        self._hand_regions(rg, rows)

    def _drop_announcement(self, announced, what: str) -> None:
        if announced is None:
            ip, self._ip_next = self._ip_next, None
            am, self._mass_next = self._mass_next, None
            rg, self._regions_next = self._regions_next, None
        else:
            ip, am, rg = announced[1], announced[2], announced[3]
        if rg is not None:
            raise _lib.MxError(f"regional prompts do not run through {what}: they are served by ONE uncached launch sequence")
        if ip is not None:
            raise _lib.MxError(f"an image prompt does not run through {what}: it is served by ONE uncached launch sequence")
        if am is not None:
            raise _lib.MxError(f"the attention mass is not captured through {what}: it is served by ONE uncached launch sequence")

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
        if added_cond_kwargs.get("image_embeds") is not None:      # rows of all resolutions in the conditioning's order; "ip_scale": a number or [rows]
            if self._ip is None:
                raise _lib.MxError("forward: image_embeds without an image-prompt adapter (set_ip_adapter)")
            tokens = self._ip[0].project(added_cond_kwargs["image_embeds"].to(self.device))
            scale = added_cond_kwargs.get("ip_scale", 1.0)
            scale = scale if torch.is_tensor(scale) else torch.full((tokens.shape[0],), float(scale))
            self.set_image_tokens(tokens, scale)
        if added_cond_kwargs.get("region_counts") is not None:    # the wide context is encoder_hidden_states itself: [rows, n_sets * seg_ld, dim]
            self.set_regions(added_cond_kwargs["region_counts"], added_cond_kwargs["region_weights"], added_cond_kwargs.get("region_seg_len", 77))
        return self._route(sample, timestep, (encoder_hidden_states, added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"]),
                           is_sliced, patch_size, input_indices)

    # ---- image-prompt adapter (sduss_amd/ip_adapter.py; mx_attention_cross_ip) -------------------------
    def set_ip_adapter(self, adapter) -> None:
        """Serve image prompts with ``adapter`` (an ip_adapter.IPAdapter) from now on: its blob goes to the device and the handle
        (mx_unet_set_ip_adapter).  Independent of the LoRA set -- the two live in different blobs.  Forwards change only where image tokens are
        announced (set_image_tokens, or forward()'s added_cond_kwargs["image_embeds"])."""
        packed = PackedWeights(adapter.packed, self.device)
        _lib.check(self._lib.mx_unet_set_ip_adapter(self._handle, packed.blob.data_ptr(), packed.blob.numel(), packed.table, len(packed.names), adapter.n_img),
                   "mx_unet_set_ip_adapter")
        self._ip, self._ip_next = (adapter, packed), None
        self._ws_need = {}                 # the plan of a handle with an adapter takes the image tokens' K / V^T as well

    def clear_ip_adapter(self) -> None:
        _lib.check(self._lib.mx_unet_set_ip_adapter(self._handle, None, 0, None, 0, 0), "mx_unet_set_ip_adapter")
        self._ip, self._ip_next = None, None
        self._ws_need = {}

    def set_image_tokens(self, tokens: torch.Tensor, ip_scale: torch.Tensor) -> None:
        """Announce the image tokens [rows, 16, cross_attention_dim] (IPAdapter.project) and scales [rows] of the NEXT forward of this model, rows in
        that forward's batch order (mx_unet_set_image_tokens; one-shot like set_context_key).  The block-cache and patch-parallel forwards refuse
        an announced call."""
        tokens = tokens.to(device=self.device, dtype=torch.bfloat16).contiguous()
        ip_scale = ip_scale.to(device=self.device, dtype=torch.float32).contiguous()
        assert tokens.ndim == 3 and tokens.shape[1:] == (16, self.cfg.cross_attention_dim) and ip_scale.shape == (tokens.shape[0],)
        self._ip_next = (tokens, ip_scale)

    # ---- regional prompts (sduss_amd/regions.py; mx_attention_cross_regions) ---------------------------------
    def set_regions(self, counts: torch.Tensor, weights_by_grid: Sequence[torch.Tensor], seg_len: int = 77) -> None:
        """Announce regional prompts for the NEXT forward of this model (mx_unet_set_regions; one-shot like set_image_tokens): ``counts`` int [rows], the
        prompts of each row (1..4); ``weights_by_grid`` one fp32 [rows, n_sets, L] per token grid with transformers, finest first (regions.token_grids).
        That forward takes encoder_hidden_states [rows, n_sets * vt_ld(seg_len), dim] (regions.batch_operands).  Rows with count 1 compute the plain
        forward's bits.  The block-cache and patch-parallel forwards, a batch of several resolutions and a forward with image tokens refuse."""
        counts = counts.to(device=self.device, dtype=torch.int32).contiguous()
        tables = [t.to(device=self.device, dtype=torch.float32).contiguous() for t in weights_by_grid]
        assert counts.ndim == 1 and tables and all(t.ndim == 3 and t.shape[:2] == (counts.numel(), tables[0].shape[1]) for t in tables)
        self._regions_next = (counts, tables, int(seg_len), int(tables[0].shape[1]))

    # ---- self-attention guidance's capture (mx_unet_set_attn_mass; sag.hip) --------------------------------
    def mid_grid(self, H_lat: int, W_lat: int) -> Tuple[int, int]:
        """the token grid of the mid block's attention for an H_lat x W_lat latent"""
        d = len(self.cfg.block_out_channels) - 1
        return H_lat >> d, W_lat >> d

    def set_attention_mass(self, mass: torch.Tensor, mask: torch.Tensor, rows: int) -> None:
        """Announce capture for the NEXT forward of this model (mx_unet_set_attn_mass; one-shot like set_image_tokens): behind the q | k | v projection
        of ``mid_block.attentions.0.transformer_blocks.0.attn1`` the column mass of sample rows [0, rows) -- the unconditional half of a CFG batch --
        goes to ``mass`` fp32 [rows, L_mid] and ``mask`` uint8 [rows, L_mid] (``mass > 1``).  The forward's output keeps its bits.  The block-cache and
        patch-parallel forwards, a batch of several resolutions, ToMe, and HyperTile where it cuts the mid level refuse an announced forward."""
        assert mass.is_cuda and mass.dtype == torch.float32 and mass.is_contiguous() and mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous()
        assert rows >= 1 and mass.ndim == 2 and mass.shape[0] == rows and mask.shape == mass.shape
        self._mass_next = (mass, mask, int(rows))

    # ---- FreeU (mx_unet_set_freeu; freeu.hip) -----------------------------------------------------------
    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float) -> None:
        """diffusers' ``UNet2DConditionModel.enable_freeu``: from now on every resnet of up blocks 0 and 1 reads its skip low-frequency-filtered (scale
        s1 / s2) beside a hidden state whose first half of the channels is scaled (b1 / b2).  On only when all four are non-zero, as in diffusers.
        Served by the plain and mixed forwards; the block-skip cache and patch-parallel forwards refuse while it is on."""
        _lib.check(self._lib.mx_unet_set_freeu(self._handle, float(s1), float(s2), float(b1), float(b2)), "mx_unet_set_freeu")
        on = all(float(v) != 0.0 for v in (s1, s2, b1, b2))
        if on != self._freeu_on:           # the plan takes a buffer for the filtered skips while FreeU is on: the arena sizes are walked again
            self._freeu_on, self._ws_need = on, {}

    def disable_freeu(self) -> None:
        """diffusers' ``disable_freeu``: the plain launch sequence again"""
        self.enable_freeu(0.0, 0.0, 0.0, 0.0)

    # ---- token merging (mx_unet_set_tome; tome.hip) ------------------------------------------------------
    def enable_tome(self, ratio: float = 0.5, sx: int = 2, sy: int = 2, max_downsample: int = 2) -> None:
        """``tomesd.apply_patch(pipe, ratio, sx=sx, sy=sy, max_downsample=max_downsample, use_rand=False)``: from now on the self-attention of every
        transformer block at a level downsampled by at most ``max_downsample`` (2: the first attention level, 4: both) runs on a sequence from which
        ``ratio`` of the tokens have been merged into their most similar cell corner.  ``ratio`` in [0, 0.75]; 0 is the plain forward.  Served by the
        plain forward and a mixed batch of one resolution; the block-skip cache and patch-parallel forwards refuse while it is on."""
        _lib.check(self._lib.mx_unet_set_tome(self._handle, float(ratio), int(sx), int(sy), int(max_downsample)), "mx_unet_set_tome")
        state = (float(ratio), int(sx), int(sy), int(max_downsample)) if ratio > 0 else None
        if state != self._tome:            # the plan takes tables and merged buffers while it is on: the arena sizes are walked again
            self._tome, self._ws_need = state, {}

    def disable_tome(self) -> None:
        """the plain launch sequence again"""
        self.enable_tome(0.0)

    # ---- HyperTile (mx_unet_set_hypertile; attention_window.hip) -----------------------------------------
    def enable_hypertile(self, tile_size: int = 128, max_depth: int = 2) -> None:
        """HyperTile (tfernd/HyperTile, ComfyUI's node) with ``swap_size=1, scale_depth=False``: from now on the self-attention of every transformer
        block at depth <= ``max_depth`` runs per window of the token grid, every window attending to itself.  ``tile_size`` is in pixels
        (``max(tile_size // 8, 4)`` tokens); 0 is the plain forward.  ``hypertile_windows`` says what a geometry gets.  Served by the plain forward and
        a mixed batch of one resolution; the block-skip cache and patch-parallel forwards, and a forward with ToMe on as well, refuse while it is on."""
        tokens = max(int(tile_size) // 8, 4) if tile_size > 0 else 0
        _lib.check(self._lib.mx_unet_set_hypertile(self._handle, tokens, int(max_depth)), "mx_unet_set_hypertile")
        state = (tokens, int(max_depth)) if tokens else None
        if state != self._hypertile:       # no buffer is added, but a sizing walk refuses HyperTile with ToMe: its answers are asked for again
            self._hypertile, self._ws_need = state, {}

    def disable_hypertile(self) -> None:
        """the plain launch sequence again"""
        self.enable_hypertile(0)

    def hypertile_windows(self, H_lat: int, W_lat: int) -> list:
        """Per attention level of an H_lat x W_lat latent, ``(gh, gw, wh, ww)`` -- the token grid and the window HyperTile cuts it into -- or None where
        the level runs the plain launch (off, deeper than max_depth, the window is the whole grid, or its width is no multiple of 16)."""
        return hypertile_windows(self.cfg, self._hypertile, H_lat, W_lat)

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
