"""CPU references for the glue kernels at the models' boundaries (csrc/elementwise.hip: prep_latent, nhwc_to_nchw, time_embed, sinus_embed,
patchify, unpatchify, crop_pos, softmax_rows, clip_embed, clip_pool), in the style of cache_move_ref.py and with its guards and comparator.

Eight of the ten are copies or conversions: their references return the BITS the kernel must leave, each stated on index views of the tensors
(reshape / permute / slice / gather) and converted by torch's own casts, not by the kernels' index arithmetic.  Two carry a derived bound.

Sinusoids (time_embed, sinus_embed; diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0) = [cos | sin]), per cell:
  x_j = fl32(fl32(-ln(1e4) j) / half) in fp32, operation by operation: the kernel and oracle/sdxl_unet_ref.py::timestep_embedding share it.
  f_j = exp(x_j), a = t f_j, c = cos(a) or sin(a) in fp64.
  e   = |a| ((|x_j| + 1) 2^-23 + 2^-24) + 2^-22.
  The kernel's __expf(x) is exp2(fl32(x log2 e)) (__clang_hip_math.h: __builtin_amdgcn_exp2f(0x1.715476p+0 * x)), one v_exp_f32, 1 ulp in the
  CDNA ISA document's accuracy table: the product x log2 e is off by |x| 2^-24 relative to f twice over (the constant's rounding and the
  product's, each |x log2 e| 2^-24 ln 2 <= |x| 2^-24), exp2 by 2^-23 and the product t f by 2^-24 more: |a| ((|x| + 1) 2^-23 + 2^-24) covers the
  angle (cos and sin are 1-Lipschitz); 2^-22 is 2 ulp of cosf / sinf at a result of magnitude <= 1 plus nothing else.  The oracle's
  torch.exp is within the same term.  A cell passes iff bf16(c - e) <= out <= bf16(c + e), both ends rounded to nearest even.

softmax_rows, per cell of a row of L scores s:
  d_i = s_i - max (exact in fp32: both are bf16 values), p = the fp64 softmax.
  tau_i = (1.5 |d_i| + 1) 2^-23: exp2(fl32(d log2 e)) as above, |d| 2^-23 for the argument and 2^-23 for the instruction (the 1.5: 2^-23 + 2^-24).
  r_i = tau_i + sum_k p_k tau_k + (L + 2) 2^-24: the numerator's error, the denominator's (a p-weighted mean of the terms' errors, whatever the
  order of the sum: at most L - 1 roundings touch any term), the reciprocal's and the final product's roundings.
  A cell passes iff bf16(p (1 - r)) <= out <= bf16(p (1 + r)).
  The bound is relative, so it asks for gradual underflow: a probability down to 2^-134 has a bf16 (subnormal) value and +0 is outside its
  interval.  v_exp_f32 alone returns +0 where its result would be an fp32 subnormal; softmax_rows_kernel evaluates arguments below -126 raised by
  64 and scales the result by 2^-64 (exp_gradual in elementwise.hip).  The raise's rounding, |d log2 e| 2^-24 in the argument, is the third
  |d| 2^-24 of tau; the roundings into the subnormal range (2^-150 absolute, 2^-17 of a bf16 subnormal step) are not in r and have not cost a cell.
"""
import math

import torch

from cache_move_ref import bits, guard_violations, guarded  # noqa: F401

LN1E4_F32 = torch.tensor(-math.log(10000.0), dtype=torch.float32)          # -9.210340371976184f
LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=torch.float32)          # 0x1.715476p+0
INF = float("inf")


def bf16_of_f64(x):
    """fp64 -> bf16 with ONE rounding to nearest even.  torch goes through fp32; that first rounding misleads the second only where it lands
    exactly on a bf16 tie from elsewhere: there the fp32 value moves one step back towards x before the second rounding."""
    f = x.float()
    tie = (f.view(torch.int32) & 0xFFFF) == 0x8000
    back = torch.where(x > f.double(), torch.nextafter(f, torch.full_like(f, INF)), torch.nextafter(f, torch.full_like(f, -INF)))
    return torch.where(tie & (f.double() != x), back, f).to(torch.bfloat16)


# ---- copies and conversions: bits ----

def prep_latent_ref(x, CP):
    """x NCHW [B, Cin, H, W] of any io dtype -> NHWC bf16 [B * H * W, CP], channels Cin.. are +0"""
    B, Cin = x.shape[:2]
    out = torch.zeros((B, x[0, 0].numel(), CP), dtype=torch.bfloat16)
    out[:, :, :Cin] = x.reshape(B, Cin, -1).permute(0, 2, 1).to(torch.bfloat16)
    return out.reshape(-1, CP)


def nhwc_to_nchw_ref(x, B, C, HW, dtype):
    """x bf16 [B * HW, ld >= C] -> NCHW [B, C, HW] of dtype"""
    return x[:, :C].reshape(B, HW, C).permute(0, 2, 1).to(dtype).contiguous()


def patchify_view(x, ps, order=(0, 2, 4, 3, 5, 1)):
    """x NCHW [B, C, H, W] -> [B * h * w, ps * ps * C] in x's dtype, columns in (dy, dx, c) order (order: the permutation of (b, c, y, dy, x, dx))"""
    B, Cc, H, W = x.shape
    h, w = H // ps, W // ps
    return x.reshape(B, Cc, h, ps, w, ps).permute(*order).reshape(B * h * w, ps * ps * Cc)


def patchify_ref(x, ps):
    """the PatchEmbed im2col, rounded once to bf16"""
    return patchify_view(x, ps).to(torch.bfloat16)


def unpatchify_ref(tok, B, Cc, H, W, ps, dtype, order=(0, 5, 1, 3, 2, 4)):
    """tokens bf16 [B * h * w, ld >= ps * ps * C] -> NCHW [B, C, H, W] of dtype: the 'nhwpqc->nchpwq' of the MMDiT's last line"""
    h, w = H // ps, W // ps
    x = tok[:, :ps * ps * Cc].reshape(B, h, w, ps, ps, Cc)
    return x.permute(*order).reshape(B, Cc, H, W).to(dtype).contiguous()


def crop_pos_ref(table, h, w):
    """table [m, m, d] -> the centred h x w window as [h * w, d] (PatchEmbed.cropped_pos_embed: the offsets round down)"""
    m, _m, d = table.shape
    top, left = (m - h) // 2, (m - w) // 2
    return table[top:top + h, left:left + w].reshape(h * w, d)


def clip_embed_ref(ids, tok, pos):
    """ids [B, L], tok [vocab, H], pos [L, H] or None -> bf16 [B * L, H]: fp32 sum of the two bf16 rows (+0 without a table), one rounding"""
    B, L = ids.shape
    s = tok[ids.clamp(0, tok.shape[0] - 1).reshape(-1).long()].float()
    s = s + (pos.float().repeat(B, 1) if pos is not None else 0.0)
    return s.to(torch.bfloat16)


def clip_pool_ref(ids, x, eos_id):
    """x [B, L, H] -> [B, H]: the row of the first EOS, or (eos_id < 0) of the largest id; transformers CLIPTextTransformer.forward literally"""
    e = (ids == eos_id).int().argmax(-1) if eos_id >= 0 else ids.argmax(-1)
    return x[torch.arange(x.shape[0]), e.long()]


# ---- sinusoids: derived bound ----

def sinusoid_exponent(dim):
    half = dim // 2
    return (LN1E4_F32 * torch.arange(half, dtype=torch.float32)) / torch.tensor(float(half), dtype=torch.float32)


def sinusoid_ref(t, dim, mutate=None):
    """t fp32 [n] -> (c, e) fp64 [n, dim]; mutate: a deliberately wrong variant (tests): 'swap', 'j+1', 'half-1', or a relative frequency error"""
    half = dim // 2
    x = sinusoid_exponent(dim)
    if mutate == "j+1":
        x = (LN1E4_F32 * torch.arange(1, half + 1, dtype=torch.float32)) / torch.tensor(float(half), dtype=torch.float32)
    elif mutate == "half-1":
        x = (LN1E4_F32 * torch.arange(half, dtype=torch.float32)) / torch.tensor(float(half - 1), dtype=torch.float32)
    f = torch.exp(x.double())
    if isinstance(mutate, float):
        f = f * (1.0 + mutate)
    a = t.double().reshape(-1, 1) * f
    c = torch.cat([torch.sin(a), torch.cos(a)] if mutate == "swap" else [torch.cos(a), torch.sin(a)], dim=1)
    e1 = a.abs() * ((x.double().abs() + 1.0) * 2.0 ** -23 + 2.0 ** -24) + 2.0 ** -22
    return c, torch.cat([e1, e1], dim=1)


def interval(c, e):
    """(lo, hi) as bf16: what a cell may hold"""
    return bf16_of_f64(c - e), bf16_of_f64(c + e)


def outside(got, lo, hi):
    """cells of got (bf16) outside [lo, hi]; a NaN is outside"""
    g = got.float()
    return ~((g >= lo.float()) & (g <= hi.float()))


def excess(got, c, e):
    """worst (|got - c| - half a bf16 step at the cell) / e over the cells with e > 0: how much of its bound the evaluation in front of the final
    rounding used (the rounding itself may move a cell by half a step); at most 1 wherever the cell lies inside its interval"""
    mag = torch.maximum(c.abs() + e, got.double().abs()).clamp_min(2.0 ** -126)
    half_step = torch.exp2(torch.floor(torch.log2(mag)) - 8.0)
    live = e > 0
    return float((((got.double() - c).abs() - half_step)[live] / e[live]).clamp_min(0.0).max())


def two_valued(lo, hi):
    """share of cells whose interval holds more than one bf16 value"""
    return float((lo.float() != hi.float()).double().mean())


def time_embed_ref(timesteps, time_ids, d0, da):
    """-> ((c, e) of tsin [B, d0], (c, e) of the sinusoid part of addin [B, 6 * da]); the first text_dim columns of addin are text_embeds' bits"""
    B = timesteps.shape[0]
    c, e = sinusoid_ref(time_ids.reshape(-1), da)
    return sinusoid_ref(timesteps, d0), (c.reshape(B, 6 * da), e.reshape(B, 6 * da))


def sinusoid_oracle_f32(t, dim):
    """the oracle's own evaluation (oracle/sdxl_unet_ref.py::timestep_embedding is this expression), fp32"""
    from oracle.sdxl_unet_ref import timestep_embedding
    return timestep_embedding(t, dim)


def sinusoid_kernel_f32(t, dim):
    """an fp32 emulation of the kernel's evaluation: exp2(fl(x log2 e)), t f, cos / sin"""
    f = torch.exp2(sinusoid_exponent(dim) * LOG2E_F32)
    a = t.float().reshape(-1, 1) * f
    return torch.cat([torch.cos(a), torch.sin(a)], dim=1)


# ---- softmax_rows: derived bound ----

def softmax_ref(s):
    """s bf16 [rows, L] -> (p, r) fp64"""
    L = s.shape[1]
    d = s.double() - s.double().max(dim=1, keepdim=True).values
    p = torch.softmax(d, dim=1)
    tau = (1.5 * d.abs() + 1.0) * 2.0 ** -23
    r = tau + (p * tau).sum(dim=1, keepdim=True) + (L + 2) * 2.0 ** -24
    return p, r


def softmax_interval(p, r):
    return bf16_of_f64(p * (1.0 - r)), bf16_of_f64(p * (1.0 + r))
