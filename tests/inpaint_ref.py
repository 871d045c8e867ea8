"""Torch restatements of the inpainting kernels (csrc/scheduler_step.hip, csrc/inpaint.hip) for tests/test_inpaint_cpu.py and tests/test_inpaint_gpu.py.  Every arithmetic
chain is fp32, one torch op per operation (torch rounds each on its own and contracts nothing), one cast at the end: the kernels must return
the same bits.  Everything here runs on the CPU."""
from __future__ import annotations

import torch


def latent_mask(mask_u8: torch.Tensor, f: int) -> torch.Tensor:
    """a client's mask uint8 [B, H, W] -> uint8 [B, H / f, W / f] of 0 / 1: binarised at byte 128, source pixel (f y, f x) (mx_mask_to_latent)"""
    return (mask_u8[:, ::f, ::f] >= 128).to(torch.uint8)


def _per_row(v, like: torch.Tensor) -> torch.Tensor:
    v = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
    return v.reshape(-1, *([1] * (like.ndim - 1)))


def renoise(init: torch.Tensor, noise: torch.Tensor, keep, sigma) -> torch.Tensor:
    """keep * init + sigma * noise per row of init [n, ...]: two fp32 products, one fp32 sum, one cast to init's dtype (mx_inpaint_renoise and the
    kept region of the masked steps); keep / sigma: a scalar or one value per row"""
    a = _per_row(keep, init) * init.to(torch.float32)
    n = _per_row(sigma, init) * noise.to(torch.float32)
    return (a + n).to(init.dtype)


def step_keep(flow: bool, sigma_next: torch.Tensor) -> torch.Tensor:
    """the keep factor of the kept region: 1 (EulerDiscreteScheduler.add_noise) or 1 - sigma_next in fp32 (the flow-match scale_noise)"""
    sigma_next = sigma_next.to(torch.float32)
    return torch.tensor(1.0, dtype=torch.float32) - sigma_next if flow else torch.ones_like(sigma_next)


def masked_step(stepped: torch.Tensor, flow: bool, sigma_next: torch.Tensor, slot, init: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """what mx_cfg_*_step_masked leaves, from the plain step's result ``stepped`` [n, C, h, w]: rows whose slot j is in [0, k) take
    renoise(init[j], noise[j], keep, sigma_next[row]) where mask[j] == 0; every other element is the plain step's"""
    out = stepped.clone()
    k = init.shape[0]
    keep = step_keep(flow, sigma_next)
    for r, j in enumerate(slot):
        if 0 <= j < k:
            kept = renoise(init[j:j + 1], noise[j:j + 1], keep[r], sigma_next[r].to(torch.float32))[0]
            out[r] = torch.where((mask[j] == 0)[None], kept, stepped[r])
    return out


def paste(decoded: torch.Tensor, original: torch.Tensor, mask_u8: torch.Tensor) -> torch.Tensor:
    """decoded uint8 [B, H, W, 3] with original's pixel wherever mask_u8 [B, H, W] < 128 (mx_rgb8_paste)"""
    return torch.where((mask_u8 < 128)[..., None], original, decoded)


def bits(t: torch.Tensor) -> torch.Tensor:
    """the raw bits of a tensor as integers, for torch.equal (a NaN equals itself, -0 differs from +0)"""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])
