"""LoRA adapters for the SDXL UNet, merged into the packed weights on the device (mx_lora_merge, include/mxdenoise.h).

The reference inherits ``load_lora_weights`` / ``fuse_lora`` from diffusers' ``StableDiffusionXLPipeline`` and passes ``lora_scale`` on
(pipeline_stable_diffusion_xl_esymred.py:119-141; modules/unet.py:359 reads ``cross_attention_kwargs["scale"]``).  Here the step plan reads one
packed blob (weights.pack), and every packing transform is linear in W: a low-rank update ``s (alpha / r) B A`` of an HF linear is the same update of
its rows in packed space, with the factors carried through the transform --

  attn1.to_q / to_k / to_v  rows [0, C) / [C, 2C) / [2C, 3C) of ``attn1.to_qkv``                      LayerNorm norm1 folded
  attn2.to_q                ``attn2.to_q``                                                          LayerNorm norm2 folded
  attn2.to_k / to_v         rows [2C l, 2C l + C) / [2C l + C, 2C (l + 1)) of ``attn2_kv_all.{C}``, l = the layer's index among that width's
  ff.net.0.proj             ``ff.net.0.proj`` with B's rows through weights._geglu_interleave       LayerNorm norm3 folded
  attn1.to_out.0, attn2.to_out.0, ff.net.2, proj_in, proj_out   as they are

For a folded target (weights.fold_layernorm: W' = bf16(W gamma), colsum = row sums of W', bias' = bias + W beta) the down factor is multiplied by
gamma in fp32 before its bf16 rounding, and the bias moves by ``dbias = B (A beta)``; the kernel recomputes colsum from the values it stores.

Fidelity: the merge rounds W + delta to bf16 once, so a delta below half an ulp of W (between 2^-9 |W| and 2^-8 |W|) is lost, as with ``fuse_lora`` on bf16 weights.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .config import UNetConfig, transformer_names
from .weights import _ALIGN, _geglu_interleave

RANK_PAD = 32      # the kernel's k-step over the rank: factors are zero-padded to a multiple of it


@dataclass(frozen=True)
class LoraTarget:
    """where one HF linear lives in the packed blob"""
    packed: str                 # the packed matrix, without ".weight"
    N: int                      # rows of the packed matrix
    K: int
    row0: int
    rows: int
    norm: Optional[str] = None  # HF prefix of the LayerNorm folded into the matrix
    geglu: bool = False         # rows interleaved by weights._geglu_interleave


def lora_targets(cfg: UNetConfig) -> Dict[str, LoraTarget]:
    """{HF module name: LoraTarget} of every linear an adapter may address: the linears of the transformer blocks plus proj_in / proj_out"""
    out: Dict[str, LoraTarget] = {}
    ctx = cfg.cross_attention_dim
    per_dim: Dict[int, int] = {}
    for _p, dim, _h, layers in transformer_names(cfg):
        per_dim[dim] = per_dim.get(dim, 0) + layers
    seen: Dict[int, int] = {}
    for p, dim, _h, layers in transformer_names(cfg):
        for l in ("proj_in", "proj_out"):
            out[f"{p}.{l}"] = LoraTarget(f"{p}.{l}", dim, dim, 0, dim)
        for k in range(layers):
            b = f"{p}.transformer_blocks.{k}"
            for i, n in enumerate(("to_q", "to_k", "to_v")):
                out[f"{b}.attn1.{n}"] = LoraTarget(f"{b}.attn1.to_qkv", 3 * dim, dim, i * dim, dim, norm=f"{b}.norm1")
            out[f"{b}.attn1.to_out.0"] = LoraTarget(f"{b}.attn1.to_out.0", dim, dim, 0, dim)
            out[f"{b}.attn2.to_q"] = LoraTarget(f"{b}.attn2.to_q", dim, dim, 0, dim, norm=f"{b}.norm2")
            layer = seen.get(dim, 0)
            seen[dim] = layer + 1
            for i, n in enumerate(("to_k", "to_v")):
                out[f"{b}.attn2.{n}"] = LoraTarget(f"attn2_kv_all.{dim}", per_dim[dim] * 2 * dim, ctx, (2 * layer + i) * dim, dim)
            out[f"{b}.attn2.to_out.0"] = LoraTarget(f"{b}.attn2.to_out.0", dim, dim, 0, dim)
            out[f"{b}.ff.net.0.proj"] = LoraTarget(f"{b}.ff.net.0.proj", 8 * dim, dim, 0, 8 * dim, norm=f"{b}.norm3", geglu=True)
            out[f"{b}.ff.net.2"] = LoraTarget(f"{b}.ff.net.2", dim, 4 * dim, 0, dim)
    return out


def norm_params(params: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the gamma / beta of the folded LayerNorms (norm1 / norm2 / norm3 of every transformer block), fp32 on the host: the packed blob no longer
    holds them, and folding an adapter needs them"""
    pat = re.compile(r"\.transformer_blocks\.\d+\.norm[123]\.(weight|bias)$")
    return {k: v.detach().to("cpu", torch.float32) for k, v in params.items() if pat.search(k)}


def blob_table(entries: Sequence[Tuple[str, torch.Tensor]]) -> List[Tuple[str, int, int]]:
    """(name, byte offset, bytes) of packed entries laid out as weights.PackedWeights lays them out"""
    total, out = 0, []
    for name, t in entries:
        total = (total + _ALIGN - 1) // _ALIGN * _ALIGN
        nb = t.numel() * t.element_size()
        out.append((name, total, nb))
        total += nb
    return out


class LoraLayout:
    """One model's side of a merge: where every target lives in ITS blob and the LayerNorm parameters folded into it."""

    def __init__(self, cfg: UNetConfig, names: Sequence[Tuple[str, int, int]], norms: Dict[str, torch.Tensor], device="cpu"):
        self.cfg = cfg
        self.device = torch.device(device)
        self.offsets = {n: (off, nb) for n, off, nb in names}
        self.norms = norms
        self.targets = lora_targets(cfg)
        for t in self.targets.values():
            assert self.offsets[f"{t.packed}.weight"][1] == t.N * t.K * 2, f"{t.packed}: packed size does not match the layout"


_SUFFIXES = ((".lora_A.weight", "A"), (".lora_B.weight", "B"), (".lora.down.weight", "A"), (".lora.up.weight", "B"), (".alpha", "alpha"))


class LoraAdapter:
    """The factors of one adapter by HF module name, as loaded; placed into a model's packed space on first use with that model."""

    def __init__(self, cfg: UNetConfig, modules: Dict[str, Tuple[torch.Tensor, torch.Tensor, float]], skipped: List[str]):
        self.cfg = cfg
        self.modules = modules          # {module: (A fp32 [r, K], B fp32 [N, r], alpha / r)}
        self.skipped = skipped          # keys of the state dict that have no place in the packed UNet (strict=False)
        self._placed: List[Tuple[LoraLayout, list]] = []

    @classmethod
    def from_state_dict(cls, cfg: UNetConfig, sd: Dict[str, torch.Tensor], strict: bool = True) -> "LoraAdapter":
        """diffusers / PEFT names: ``<module>.lora_A.weight`` [r, K], ``<module>.lora_B.weight`` [N, r], optional ``<module>.alpha`` (the factor is
        alpha / r, 1 without it); an optional ``unet.`` prefix and the older ``<module>.lora.down.weight`` / ``.lora.up.weight`` spellings are accepted.
        Keys without a place in the packed UNet (conv / LoCon modules, time_emb_proj, text_encoder.*, anything unknown) raise ValueError with the
        list under ``strict``; otherwise they are returned in ``.skipped``.  kohya ``lora_unet_*`` names are not translated."""
        targets = lora_targets(cfg)
        found: Dict[str, dict] = {}
        skipped: List[str] = []
        for key, v in sd.items():
            name = key[len("unet."):] if key.startswith("unet.") else key
            for suf, role in _SUFFIXES:
                if name.endswith(suf) and name[:-len(suf)] in targets:
                    found.setdefault(name[:-len(suf)], {})[role] = (key, v)
                    break
            else:
                skipped.append(key)
        modules: Dict[str, Tuple[torch.Tensor, torch.Tensor, float]] = {}
        for m, parts in found.items():
            if "A" not in parts or "B" not in parts:
                raise ValueError(f"LoRA module {m}: needs both factors, got {sorted(k for k, _ in parts.values())}")
            t = targets[m]
            a, b = parts["A"][1], parts["B"][1]
            if a.ndim != 2 or b.ndim != 2:            # a conv-shaped factor on a linear target
                skipped.extend(k for k, _ in parts.values())
                continue
            r = a.shape[0]
            if tuple(a.shape) != (r, t.K) or tuple(b.shape) != (t.rows, r) or r == 0:
                raise ValueError(f"LoRA module {m}: factors {tuple(a.shape)} / {tuple(b.shape)} do not fit a [{t.rows}, {t.K}] linear")
            alpha = float(parts["alpha"][1]) if "alpha" in parts else float(r)
            modules[m] = (a.detach().to("cpu", torch.float32), b.detach().to("cpu", torch.float32), alpha / r)
        if skipped and strict:
            raise ValueError(f"{len(skipped)} LoRA keys have no place in the packed UNet (strict): {sorted(skipped)}")
        return cls(cfg, modules, sorted(skipped))

    def placed(self, layout: LoraLayout) -> list:
        """the adapter's terms in ``layout``'s packed space, built once per layout: dicts as ops.lora_terms takes them, plus "module", "factor"
        (alpha / r; the term's scale is the caller's scale times it) and "packed" (the packed matrix name)"""
        for lay, terms in self._placed:
            if lay is layout:
                return terms
        terms = []
        for m, (a, b, factor) in self.modules.items():
            t = layout.targets[m]
            r = a.shape[0]
            rp = (r + RANK_PAD - 1) // RANK_PAD * RANK_PAD
            up = _geglu_interleave(b) if t.geglu else b
            down = a
            dbias = None
            if t.norm is not None:
                gamma, beta = layout.norms[f"{t.norm}.weight"], layout.norms[f"{t.norm}.bias"]
                down = a * gamma[None, :]
                dbias = up @ (a @ beta)
            up_p = torch.zeros((t.rows, rp), dtype=torch.bfloat16)
            up_p[:, :r] = up.to(torch.bfloat16)
            down_t = torch.zeros((t.K, rp), dtype=torch.bfloat16)
            down_t[:, :r] = down.t().to(torch.bfloat16)
            term = {"module": m, "packed": t.packed, "factor": factor, "w_off": layout.offsets[f"{t.packed}.weight"][0], "N": t.N, "K": t.K,
                    "row0": t.row0, "rows": t.rows, "up": up_p.to(layout.device), "down_t": down_t.to(layout.device)}
            if t.norm is not None:
                term["colsum_off"] = layout.offsets[f"{t.packed}.colsum"][0]
                term["bias_off"] = layout.offsets[f"{t.packed}.bias"][0]
                term["dbias"] = dbias.contiguous().to(layout.device)
            terms.append(term)
        self._placed.append((layout, terms))
        return terms


def scaled_terms(layout: LoraLayout, adapters: Sequence[Tuple[LoraAdapter, float]]) -> list:
    """the term table of an adapter set: every adapter's placed terms with scale = the set's scale times the adapter's alpha / r, in set order"""
    out = []
    for adapter, scale in adapters:
        for t in adapter.placed(layout):
            out.append({**t, "scale": float(scale) * t["factor"]})
    return out


def merged_params(params: Dict[str, torch.Tensor], adapters: Sequence[Tuple[LoraAdapter, float]]) -> Dict[str, torch.Tensor]:
    """HF-named parameters with the adapters added in fp32, W + s (alpha / r) B A: what diffusers' ``fuse_lora`` computes, and what the parent route
    ``MxUNet(cfg, merged_params(...))`` packs.  For tests and the comparison in tools/lora_swap_bench.py."""
    out = dict(params)
    for adapter, scale in adapters:
        for m, (a, b, factor) in adapter.modules.items():
            k = f"{m}.weight"
            w = out[k].to(torch.float32)
            out[k] = w + (float(scale) * factor) * (b @ a).reshape(w.shape)
    return out
