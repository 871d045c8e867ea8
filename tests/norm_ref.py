"""Elementwise fp64 references for the normalisation kernels (csrc/norm.hip, csrc/gn_halo_nchw.hip), in the style of kernel_ref.py and with its
guards, NaN padding and comparator.

Every reference is computed in float64 from the values the kernel actually receives (bf16 / fp16 / fp32 activations, fp32 affine and
modulation), and every output element gets its OWN bound, the sum of the rounding steps the kernel's arithmetic can take on the way to it.

Row norms (row_norm_kernel with its three stores -- affine, AdaLN modulate, RMS weight -- and rmsnorm_heads_kernel): two passes over registers, C values a row
  mean           fp32 sum of C terms in any order, one divide:                     d_mean = C 2^-24 mean|x| + 2^-24 |mean|
  variance       fp32 centred sum of squares, likewise (each d = x - mean rounded, each square rounded: 3 2^-24 more), plus the effect of
                 the mean's error on it:                                            d_var = (C + 3) 2^-24 var + 2 mean|x - mean| d_mean + d_mean^2
                 (RMSNorm: no mean; the squares of bf16 values are exact in fp32)
  rstd           relative: d_var / (2 (var + eps)) + 2^-21 (rsqrtf) + 2 2^-24 (the divide by C, the add of eps; the heads kernel's
                 multiply by q_scale takes one more 2^-24)
  normalised     n = (x - mean) rstd:   rstd (d_mean + 2^-24 |x - mean|) + |n| (rel(rstd) + 2^-24)
  affine         n gamma + beta  /  n (1 + scale) + shift  /  n w:   2^-24 |intermediate| per fp32 multiply or add (1 + scale is one more)
  output         bf16 round to nearest: 2^-8 (|ref| + bound so far)

row_stats_kernel: fp32 outputs, single pass: |sum - ref| <= C 2^-24 sum|x|, |sumsq - ref| <= C 2^-24 sum x^2.

GroupNorm, NHWC (gn_stats_kernel / gn_fold_kernel / gn_apply_kernel, every route): single-pass fp32 partial sums of n_t terms, folded in fp64
(exactly, at this precision).  n_t is the number of terms one fp32 partial sum holds: the pixels of a spatial tile, times the channels of a
group where the statistics pass adds those in fp32 as well (the fold-in-apply route).  Per (image, patch, group):
  d_mean = n_t 2^-24 mean|x|        d_q = n_t 2^-24 E[x^2]        d_var = d_q + 2 |mean| d_mean + d_mean^2      (var = q - mean^2)
averaged over the patches of an image as the kernel averages them.  rstd = (var + eps)^-1/2 moves by at most
  d_rstd = max(rstd - (var + d_var + eps)^-1/2, (max(var - d_var, 0) + eps)^-1/2 - rstd)
-- the exact image of [var - d_var, var + d_var] (the kernel clamps var at 0); to first order (var + eps)^-3/2 d_var / 2.  The output error is
written in the correlated form
  |x - mean| |gamma| d_rstd + (rstd + d_rstd) |gamma| d_mean
(NOT |x| d_scale + d_shift: the scale's and the shift's errors cancel, and that form is 50 times looser on offset inputs and unbounded on a
constant group), plus the fp32 steps of scale = rstd gamma, shift = beta - scale mean, x scale + shift:
  2^-24 (2 |x scale| + 2 |scale mean| + |shift| + |y|)
then SiLU through kernel_ref.act_bound and the output rounding.  mx_groupnorm_nhwc_from_partials: the partial sums are INPUTS; the reference
folds them in fp64 by the kernel's closed form, so n_t = 0 and only the fp64 fold's own cancellation (2^-50 (q + mean^2)) remains.

GroupNorm + halo, NCHW (moments_kernel / merge_kernel / apply_gather_kernel / apply_plain_kernel): the same derivation with n_t = cpg H W
(+ 1 for fp32 inputs, whose squares are rounded), and
  stored         fp32 mean and var between the launches: 2^-24 relative each
  merge          fp32 sum over the P patches of a latent and a divide: (P + 1) 2^-24 of mean|mean_p| and of the mean variance; rsqrtf 2^-21
  output         2^-22 for fp32, 2^-11 for fp16, 2^-8 for bf16
A halo cell is a copy of the SENDER's output pixel: the sender's reference and the sender's bound.  mx_halo_only moves data: bit for bit.
"""
import torch

from kernel_ref import (ACT_EVAL, LIP, U32, SILU, act_bound, act_ref, assert_within, guard_violations, guarded, nan_padded,  # noqa: F401
                        violations, GUARD_BF16, GUARD_F32)

RSQRT = 2.0 ** -21             # rsqrtf, relative (what _rms_apply of test_kernel_forms_gpu.py uses)
OUT_REL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -22}


def _out(v, e, rel=2.0 ** -8):
    return v, e + rel * (v.abs() + e)


# ---- row norms ----

def row_normalise(x, eps, centre=True, extra_rel=0.0):
    """x [M, C] (any float dtype) -> fp64 (n, e_n): n = (x - mean) rstd (centre) or x rstd (RMS) and its bound before any affine"""
    x = x.double()
    C = x.shape[1]
    if centre:
        mean = x.mean(1, keepdim=True)
        d_mean = C * U32 * x.abs().mean(1, keepdim=True) + U32 * mean.abs()
        d = x - mean
        var = (d * d).mean(1, keepdim=True)
        d_var = (C + 3) * U32 * var + 2.0 * d.abs().mean(1, keepdim=True) * d_mean + d_mean ** 2
    else:
        d, d_mean = x, torch.zeros_like(x[:, :1])
        var = (d * d).mean(1, keepdim=True)
        d_var = C * U32 * var
    rstd = 1.0 / torch.sqrt(var + eps)
    rel = 0.5 * d_var / (var + eps) + RSQRT + 2 * U32 + extra_rel
    n = d * rstd
    return n, rstd * (d_mean + (U32 * d.abs() if centre else 0.0)) + n.abs() * (rel + U32)


def layernorm_ref(x, gamma, beta, eps):
    """mx_layernorm: (x - mean) rstd gamma + beta; gamma is None: the plain normalisation"""
    n, e = row_normalise(x, eps)
    if gamma is None:
        return _out(n, e)
    g, b = gamma.double(), beta.double()
    v = n * g
    o = v + b
    return _out(o, e * g.abs() + U32 * v.abs() + U32 * o.abs())


def modulate_ref(x, scale, shift, sample, eps):
    """mx_layernorm_mod: LN(x) (1 + scale[sample]) + shift[sample]; scale / shift fp32 [samples, C], sample [M] the modulation row of a row"""
    n, e = row_normalise(x, eps)
    g = 1.0 + scale.double()[sample]
    v = n * g
    o = v + shift.double()[sample]
    return _out(o, e * g.abs() + 2 * U32 * v.abs() + U32 * o.abs())       # 1 + scale, the multiply, the add


def rmsnorm_ref(x, w, eps):
    """mx_rmsnorm: x rsqrt(mean(x^2) + eps) w"""
    n, e = row_normalise(x, eps, centre=False)
    o = n * w.double()
    return _out(o, e * w.double().abs() + U32 * o.abs())


def rmsnorm_heads_ref(x, heads_q, wq, wk, eps, q_scale):
    """mx_rmsnorm_heads on the selected rows x [R, 64 heads]: every 64-wide head by its own rms; heads below heads_q by wq and q_scale"""
    R, D = x.shape
    H = D // 64
    n, e = row_normalise(x.reshape(R * H, 64), eps, centre=False, extra_rel=U32)
    n, e = n.reshape(R, H, 64), e.reshape(R, H, 64)
    isq = (torch.arange(H, device=x.device) < heads_q)[None, :, None]
    w = torch.where(isq, wq.double()[None, None, :], wk.double()[None, None, :])
    f = torch.where(isq, torch.tensor(float(q_scale), dtype=torch.float64, device=x.device), torch.tensor(1.0, dtype=torch.float64, device=x.device))
    o = n * f * w
    v, b = _out(o, e * (f * w).abs() + U32 * o.abs())
    return v.reshape(R, D), b.reshape(R, D)


def row_stats_ref(x):
    """mx_row_stats: (ref [M, 2], bound [M, 2]) of (sum, sum of squares)"""
    x = x.double()
    C = x.shape[1]
    s1, s2 = x.sum(1), (x * x).sum(1)
    return torch.stack([s1, s2], 1), torch.stack([C * U32 * x.abs().sum(1), C * U32 * s2], 1)


# ---- GroupNorm ----

def patch_moments(x4, groups, ph, pw, n_t):
    """x4 fp64 [B, C, H, W]; statistics per (image, group, patch of ph x pw) averaged over the patches of an image.
    Returns (mean, d_mean, var, d_var), each [B, groups]"""
    B, C, H, W = x4.shape
    v = x4.reshape(B, groups, C // groups, H // ph, ph, W // pw, pw)
    dims = (2, 4, 6)
    m, a, q = v.mean(dims), v.abs().mean(dims), (v * v).mean(dims)
    d_m = n_t * U32 * a
    var = (q - m * m).clamp_min(0.0)
    d_var = n_t * U32 * q + 2.0 * m.abs() * d_m + d_m ** 2
    return m.mean((2, 3)), d_m.mean((2, 3)), var.mean((2, 3)), d_var.mean((2, 3))


def rstd_interval(var, d_var, eps, rel=0.0):
    """rstd = (var + eps)^-1/2 and the most it moves for a variance within d_var (clamped at 0), plus rel of itself"""
    rstd = 1.0 / torch.sqrt(var + eps)
    up = 1.0 / torch.sqrt((var - d_var).clamp_min(0.0) + eps) - rstd
    down = rstd - 1.0 / torch.sqrt(var + d_var + eps)
    return rstd, torch.maximum(up, down) + rel * rstd


def groupnorm_apply_ref(x4, mean, d_mean, rstd, d_rstd, gamma, beta, silu, out_rel):
    """x4 fp64 [B, C, H, W]; mean .. d_rstd [B, groups]; gamma / beta [C] or None.  Returns (ref, bound) [B, C, H, W]"""
    B, C = x4.shape[:2]
    cpg = C // mean.shape[1]
    ex = lambda t: t.repeat_interleave(cpg, dim=1)[:, :, None, None]
    mean, d_mean, rstd, d_rstd = ex(mean), ex(d_mean), ex(rstd), ex(d_rstd)
    g = gamma.double()[None, :, None, None] if gamma is not None else torch.ones((1, C, 1, 1), dtype=torch.float64, device=x4.device)
    b = beta.double()[None, :, None, None] if beta is not None else torch.zeros((1, C, 1, 1), dtype=torch.float64, device=x4.device)
    sc = rstd * g
    sf = b - sc * mean
    y = (x4 - mean) * sc + b
    e = (x4 - mean).abs() * g.abs() * d_rstd + (rstd + d_rstd) * g.abs() * d_mean
    e = e + U32 * (2.0 * (x4 * sc).abs() + 2.0 * (sc * mean).abs() + sf.abs() + y.abs())
    if silu:
        e = act_bound(y, e)
        y = act_ref(SILU, y)
    return _out(y, e, out_rel)


def groupnorm_nhwc_ref(x, gamma, beta, groups, eps, patch, silu, n_t):
    """mx_groupnorm_nhwc / _cat / _grouped on x [B, H, W, C] bf16 (a concatenation: already joined).  patch: 0 or the patch edge (a patch that
    covers the image is exact, as in the kernel).  Returns (ref, bound) [B, H, W, C]"""
    B, H, W, C = x.shape
    if patch >= H and patch >= W:
        patch = 0
    x4 = x.double().permute(0, 3, 1, 2)
    mean, d_mean, var, d_var = patch_moments(x4, groups, patch or H, patch or W, n_t)
    rstd, d_rstd = rstd_interval(var, d_var, eps)
    y, e = groupnorm_apply_ref(x4, mean, d_mean, rstd, d_rstd, gamma, beta, silu, 2.0 ** -8)
    return y.permute(0, 2, 3, 1), e.permute(0, 2, 3, 1)


def fold_partials(part, chunk, groups, add_bias=None, add_rowbias=None):
    """gn_fold_kernel's closed form in fp64: part fp32 [B, HW / chunk, C, 2] holds the sums of (x - c) and (x - c)^2 over chunks of `chunk` pixels,
    c = add_bias[ch] + add_rowbias[image, ch].  Returns (mean, var, q) per [B, groups]"""
    B, T, C, _ = part.shape
    p = part.double()
    s, q = p[..., 0], p[..., 1]
    if add_bias is not None:
        c = add_bias.double()[None, None, :]
        if add_rowbias is not None:
            c = c + add_rowbias.double()[:, None, :]
        q = q + 2.0 * c * s + chunk * c * c
        s = s + chunk * c
    cnt = T * chunk * (C // groups)
    mean = s.reshape(B, T, groups, -1).sum((1, 3)) / cnt
    q = q.reshape(B, T, groups, -1).sum((1, 3)) / cnt
    return mean, (q - mean * mean).clamp_min(0.0), q


def groupnorm_from_partials_ref(x, part, chunk, gamma, beta, groups, eps, silu, add_bias=None, add_rowbias=None):
    """mx_groupnorm_nhwc_from_partials: the statistics are what the given partial sums say, folded in fp64"""
    mean, var, q = fold_partials(part, chunk, groups, add_bias, add_rowbias)
    d_var = 2.0 ** -50 * (q + mean * mean)
    rstd, d_rstd = rstd_interval(var, d_var, eps)
    x4 = x.double().permute(0, 3, 1, 2)
    y, e = groupnorm_apply_ref(x4, mean, 2.0 ** -50 * mean.abs(), rstd, d_rstd, gamma, beta, silu, 2.0 ** -8)
    return y.permute(0, 2, 3, 1), e.permute(0, 2, 3, 1)


def halo_gather(inner, pidx):
    """inner [N, C, H, W] -> [N, C, H + 2, W + 2]: the interior, and the 1-pixel frame the SENDERS write (sender b, direction d of its row of
    the adjacency table pidx [N, 4] = up, left, down, right neighbour: its edge row / column goes into the facing frame side of that neighbour;
    the corners go with the columns); zero where nobody writes.  Any dtype: pure data movement"""
    N, C, H, W = inner.shape
    out = torch.zeros((N, C, H + 2, W + 2), dtype=inner.dtype, device=inner.device)
    out[:, :, 1:-1, 1:-1] = inner
    rows = torch.tensor([0] + list(range(H)) + [H - 1], device=inner.device)
    for b, nbrs in enumerate(pidx.reshape(N, 4).tolist()):
        up, left, down, right = nbrs
        if up >= 0:
            out[up, :, H + 1, 1:W + 1] = inner[b, :, 0, :]
        if down >= 0:
            out[down, :, 0, 1:W + 1] = inner[b, :, H - 1, :]
        if left >= 0:
            out[left, :, :, W + 1] = inner[b][:, rows, 0]
        if right >= 0:
            out[right, :, :, 0] = inner[b][:, rows, W - 1]
    return out


def groupnorm_nchw_ref(x, gamma, beta, cpg, eps, latent_offset, patch_map):
    """mx_groupnorm_halo's interior: x [N, C, H, W] (fp32 / fp16 / bf16), gamma / beta of x's dtype [C]; statistics per (patch, group), merged over
    the patches [latent_offset[l - 1], latent_offset[l]) of the patch's latent l = patch_map[n] (1-based).  Returns (ref, bound) [N, C, H, W]"""
    N, C, H, W = x.shape
    G = C // cpg
    x4 = x.double()
    n_t = cpg * H * W + (1 if x.dtype == torch.float32 else 0)
    m, d_m, var, d_var = patch_moments(x4, G, H, W, n_t)                 # per patch [N, G]
    d_m = d_m + U32 * m.abs()                                            # stored as fp32
    d_var = d_var + U32 * var
    mean, d_mean, mvar, d_mvar = (torch.empty_like(m) for _ in range(4))
    for n in range(N):
        lo, hi = latent_offset[int(patch_map[n]) - 1], latent_offset[int(patch_map[n])]
        P = hi - lo
        mean[n] = m[lo:hi].mean(0)
        d_mean[n] = d_m[lo:hi].mean(0) + (P + 1) * U32 * m[lo:hi].abs().mean(0)
        mvar[n] = var[lo:hi].mean(0)
        d_mvar[n] = d_var[lo:hi].mean(0) + (P + 2) * U32 * (mvar[n] + eps)
    rstd, d_rstd = rstd_interval(mvar, d_mvar, eps, rel=RSQRT)
    return groupnorm_apply_ref(x4, mean, d_mean, rstd, d_rstd, gamma, beta, False, OUT_REL[x.dtype])


def reference(c, p, n_t=None):
    """{output name: (ref, bound)} of a case of norm_form_cases.py on the operands p = build(c, device)"""
    import norm_form_cases as NC
    k, eps = c["kind"], p["eps"]
    if k == "ln":
        return {"y": layernorm_ref(p["x"], p["gamma"], p["beta"], eps)}
    if k in ("lnmod", "lnmod_grouped"):
        out = {"y": modulate_ref(p["x"], p["scale"], p["shift"], p["sample"], eps)}
        if c["dual"]:
            out["y2"] = modulate_ref(p["x"], p["scale2"], p["shift2"], p["sample"], eps)
        return out
    if k == "rms":
        return {"y": rmsnorm_ref(p["x"], p["w"], eps)}
    if k == "rms_heads":
        return {"y": rmsnorm_heads_ref(p["buf"][p["rows"], :64 * c["ht"]], c["hq"], p["wq"], p["wk"], eps, p["q_scale"])}
    if k == "row_stats":
        return {"stats": row_stats_ref(p["x"])}
    if k == "gn":
        fold = NC.gn_fold_in_apply(c["groups"], c["patch"], [(c["B"], c["H"], c["W"])])
        return {"y": groupnorm_nhwc_ref(p["x"], p["gamma"], p["beta"], c["groups"], eps, c["patch"], c["silu"], NC.gn_terms(c, c["B"], c["H"], c["W"], fold))}
    if k == "gn_grouped":
        fold = NC.gn_fold_in_apply(c["groups"], c["patch"], c["probs"])
        return {f"y{i}": groupnorm_nhwc_ref(x, p["gamma"], p["beta"], c["groups"], eps, c["patch"], c["silu"], NC.gn_terms(c, b, h, w, fold))
                for i, (x, (b, h, w)) in enumerate(zip(p["xs"], c["probs"]))}
    if k == "gn_partials":
        return {"y": groupnorm_from_partials_ref(p["x"], p["part"], c["chunk"], p["gamma"], p["beta"], c["groups"], eps, c["silu"], p["bias"], p["rowbias"])}
    if k == "gn_nchw":
        ref, bound = groupnorm_nchw_ref(p["x"], p["gamma"], p["beta"], c["shape"][2], eps, NC.NCHW_LAT_OFF, NC.NCHW_PMAP)
        if c["padding"]:
            ref, bound = halo_gather(ref, p["pidx"]), halo_gather(bound, p["pidx"])
        return {"y": (ref, bound)}
    raise ValueError(k)
