"""Regional prompts ("attention couple") for the SDXL slot: a request carries up to ops.REGION_SETS prompts and one non-negative mask per prompt; every
cross-attention layer blends the prompts' separately normalised attention outputs per query token (csrc/attention_regions.hip,
mx_attention_cross_regions).  Here is the plumbing around that launch, in torch, once per request and token grid:

  * the mask-to-weights rule: a token's weight for prompt r is the AREA MEAN of mask r over the token's cell of the latent, divided by the sum of those
    means over the prompts; a token no mask covers gets weight 1 on prompt 0 (the request's own prompt).  This is the formulation of ComfyUI's Attention
    Couple and of the Regional Prompter's attention mode with a downsampling rule of our own, stated here; no byte parity with either is claimed;
  * the batch's operands: the wide context [rows, n_sets * seg_ld, cross_dim] (prompt r of a row at tokens r * seg_ld .., padding and unused sets zero),
    counts int32 [rows] and one weight table [rows, n_sets, L] per token grid.  Unconditional rows and requests without regions have count 1."""
from typing import List, Optional, Sequence, Tuple

import torch

from .lib import MxError

REGION_SETS = 4        # MX_REGION_SETS


def vt_ld(n: int) -> int:
    """MX_VT_LD: rows a prompt of n tokens takes in the wide context"""
    return (n + 15) // 16 * 16


def token_grids(cfg, h_lat: int, w_lat: int) -> List[Tuple[int, int]]:
    """the token grids of an h_lat x w_lat latent that have transformers, finest first (SDXL-base at 128 x 128: 64 x 64 and 32 x 32)"""
    last = len(cfg.down_has_attn) - 1
    return [(h_lat >> l, w_lat >> l) for l, has in enumerate(cfg.down_has_attn) if has or l == last]


def mask_weights(masks: torch.Tensor, grid: Tuple[int, int]) -> torch.Tensor:
    """fp32 [R, gh * gw]: the weights of R prompts on the tokens of ``grid`` from masks [R, H, W] (non-negative; H, W multiples of the grid)"""
    r, h, w = masks.shape
    gh, gw = grid
    if h % gh or w % gw:
        raise MxError(f"regions: masks of {h} x {w} do not cut into a {gh} x {gw} token grid")
    m = masks.float().view(r, gh, h // gh, gw, w // gw).mean(dim=(2, 4)).reshape(r, gh * gw)
    tot = m.sum(dim=0, keepdim=True)
    wts = torch.where(tot > 0, m / tot.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(m))
    wts[0] = torch.where(tot[0] > 0, wts[0], torch.ones_like(wts[0]))
    return wts


class Regions:
    """what SDXLDenoiser.set_regions leaves on a request: the prompts' embeddings, the masks, and the weights per token grid (made on first use)"""

    def __init__(self, prompt_embeds: torch.Tensor, masks: torch.Tensor, latent_hw: Optional[Tuple[int, int]] = None):
        if prompt_embeds.ndim != 3 or not 1 <= prompt_embeds.shape[0] <= REGION_SETS:
            raise MxError(f"regions: prompt_embeds must be [R, tokens, dim] with R in 1..{REGION_SETS}, got {tuple(prompt_embeds.shape)}")
        if prompt_embeds.shape[1] > 96:
            raise MxError(f"regions: a prompt has at most 96 tokens, got {prompt_embeds.shape[1]}")
        if masks.ndim != 3 or masks.shape[0] != prompt_embeds.shape[0] or (latent_hw is not None and tuple(masks.shape[1:]) != tuple(latent_hw)):
            want = (prompt_embeds.shape[0], *(latent_hw or ("H_lat", "W_lat")))
            raise MxError(f"regions: masks must be {want}, one per prompt at the latent's size, got {tuple(masks.shape)}")
        if masks.dtype != torch.bool and bool((masks < 0).any()):
            raise MxError("regions: masks must not be negative")
        self.prompt_embeds, self.masks = prompt_embeds, masks
        self._weights = {}

    @property
    def count(self) -> int:
        return self.prompt_embeds.shape[0]

    @property
    def seg_len(self) -> int:
        return self.prompt_embeds.shape[1]

    def weights(self, grid: Tuple[int, int]) -> torch.Tensor:
        if grid not in self._weights:
            self._weights[grid] = mask_weights(self.masks, grid)
        return self._weights[grid]


def batch_operands(regions: Sequence[Optional[Regions]], ehs: torch.Tensor, cfg_halves: int, grids: Sequence[Tuple[int, int]]) -> tuple:
    """(wide context bf16 [rows, n_sets * seg_ld, dim], counts int32 [rows], [weights fp32 [rows, n_sets, L] per grid], seg_len) of one resolution's model
    rows: ``ehs`` [rows, seg_len, dim] is the plain conditioning, rows = cfg_halves * len(regions) in the order [uncond..., cond...]; only the
    conditional row of a request with regions gets its prompts and weights, every other row count 1 (its weights are never read)."""
    n, dev = len(regions), ehs.device
    have = [g for g in regions if g is not None]
    seg = ehs.shape[1]
    if any(g.seg_len != seg or g.prompt_embeds.shape[2] != ehs.shape[2] for g in have):
        raise MxError(f"regions: every prompt must be [{seg}, {ehs.shape[2]}] like the batch's conditioning")
    n_sets, seg_ld, rows = max(g.count for g in have), vt_ld(seg), ehs.shape[0]
    wide = ehs.new_zeros((rows, n_sets, seg_ld, ehs.shape[2]))
    wide[:, 0, :seg] = ehs
    counts = torch.ones(rows, dtype=torch.int32)
    tables = [torch.zeros((rows, n_sets, gh * gw), dtype=torch.float32, device=dev) for gh, gw in grids]
    for i, g in enumerate(regions):
        if g is None:
            continue
        row = (cfg_halves - 1) * n + i
        counts[row] = g.count
        wide[row, 1:g.count, :seg] = g.prompt_embeds[1:].to(device=dev, dtype=ehs.dtype)
        for t, grid in zip(tables, grids):
            t[row, :g.count] = g.weights(grid).to(dev)
    return wide.view(rows, n_sets * seg_ld, ehs.shape[2]), counts.to(dev), tables, seg
