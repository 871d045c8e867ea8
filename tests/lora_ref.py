"""fp64 restatement of the LoRA merge (mx_lora_merge, include/mxdenoise.h) and its per-element acceptance rule.

The device computes, per element of a targeted row range,

    out[n][k] = bf16_rn( f32(base[n][k]) + sum_t scale_t * sum_r up_t[n][r] * down_t[k][r] )

with exact bf16 x bf16 products, fp32 accumulation over r (any order: the matrix core's), the fp32 scale applied to each term's sum, fp32 adds of
the terms onto the base, and ONE rounding to bf16.  With v the same expression in float64 (from the bf16 factors and the fp32 scales the kernel
receives), every fp32 operation on the way errs by at most 2^-24 of the magnitude it handles, and there are at most R_total + n_terms + (a few) of
them, each on a partial sum no larger than |W| + sum_t |s_t| (|up_t| @ |down_t|^T); hence

    tol = (R_total + 4) 2^-24 (|W| + sum_t |s_t| (|up_t| @ |down_t|^T))          (the fp32 accumulation bound, any summation order)

and, rounding being monotone, an output element is right iff  rn_bf16(v - tol) <= out <= rn_bf16(v + tol).  Every element is checked.  The rule is
only as sharp as the inputs make it: where rn(v - tol) != rn(v + tol) two neighbouring bf16 values pass, so the share of such elements must stay
under 10 % (with W ~ 0.03 N(0,1) and factors ~ 0.05 N(0,1) it is 0.7 % - 4.6 % at the shapes of tests/test_lora_merge_gpu.py).

colsum[n] is the fp32 sum over k of the rounded out[n][k]: |cs - sum_k out[n][k]| <= K 2^-24 sum_k |out[n][k]| in any order of summation.
"""
import torch

U32 = 2.0 ** -24
AMBIGUOUS_MAX = 0.10


def rn_bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even), returned as float64.  Directly from float64: going through float32 would round twice.
    (bf16 keeps 8 significant bits: 2^p <= |x| < 2^(p + 1) has ulp 2^(p - 7); the magnitudes here are far from the subnormals.  2^p is taken
    from x's exponent bits, which is exact on every device; pow / ldexp on the GPU need not be.)"""
    assert x.dtype == torch.float64
    p2 = (x.contiguous().view(torch.int64) & 0x7FF0000000000000).view(torch.float64)
    ulp = torch.where(p2 == 0, torch.ones_like(p2), p2 * 2.0 ** -7)
    return torch.round(x / ulp) * ulp


def f32_scale(s: float) -> float:
    """the scale as the kernel holds it (mx_lora_term.scale is a float)"""
    return float(torch.tensor(s, dtype=torch.float32))


def merge_ref(base: torch.Tensor, terms):
    """base bf16 [rows, K]; terms = [(up bf16 [rows, R], down_t bf16 [K, R], scale)] on the same row range, in table order
    -> (v, tol) float64 [rows, K]"""
    w = base.to(torch.float64)
    v, mag, r_total = w.clone(), w.abs(), 0
    for up, down_t, scale in terms:
        s = f32_scale(scale)
        u, d = up.to(torch.float64), down_t.to(torch.float64)
        v += s * (u @ d.t())
        mag += abs(s) * (u.abs() @ d.abs().t())
        r_total += up.shape[1]
    return v, (r_total + 4) * U32 * mag


def interval(v: torch.Tensor, tol: torch.Tensor):
    return rn_bf16(v - tol), rn_bf16(v + tol)


def check_merge(out: torch.Tensor, base: torch.Tensor, terms, what: str) -> float:
    """asserts the interval rule for EVERY element of out (bf16 [rows, K]) and the condition on the inputs; returns the ambiguous share"""
    v, tol = merge_ref(base, terms)
    lo, hi = interval(v, tol)
    o = out.to(torch.float64)
    assert torch.isfinite(o).all(), f"{what}: non-finite output"
    bad = (o < lo) | (o > hi)
    share = float((lo != hi).double().mean())
    print(f"{what}: {int(bad.sum())} of {o.numel()} outside the interval, {100 * share:.2f} % of the intervals hold two values")
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {o.numel()} elements outside [rn(v - tol), rn(v + tol)]; first at flat index {i}: "
                             f"out {o.reshape(-1)[i]:.9g}, v {v.reshape(-1)[i]:.9g}, tol {tol.reshape(-1)[i]:.3g}")
    assert share < AMBIGUOUS_MAX, f"{what}: {100 * share:.1f} % of the intervals hold two bf16 values: the inputs make the rule too loose"
    return share


def check_colsum(colsum: torch.Tensor, out: torch.Tensor, what: str) -> None:
    """colsum fp32 [rows] against the rounded values out bf16 [rows, K] the launch stored"""
    o = out.to(torch.float64)
    want, mag = o.sum(dim=1), o.abs().sum(dim=1)
    err = (colsum.to(torch.float64) - want).abs()
    bound = out.shape[1] * U32 * mag
    assert bool((err <= bound).all()), f"{what}: colsum off by up to {float(err.max()):.3g}, bound {float(bound[err.argmax()]):.3g}"


def apply_terms(packed: dict, terms) -> dict:
    """The device formula restated on the host over packed tensors {name: tensor} (weights.pack) and placed terms (lora.scaled_terms, tensors on
    the CPU): the targeted rows of every matrix as float64 -> bf16 with ONE rounding, colsum as the fp32 row sums of the rounded rows, bias' =
    bias'_base + sum scale * dbias in fp32.  Terms on one row range add up in table order.  Returns only the tensors that changed."""
    groups = {}
    for t in terms:
        groups.setdefault((t["packed"], t["row0"], t["rows"]), []).append(t)
    out = {}
    for (name, row0, rows), ts in groups.items():
        wname = f"{name}.weight"
        w = out.setdefault(wname, packed[wname].clone())
        v, _tol = merge_ref(packed[wname][row0:row0 + rows], [(t["up"], t["down_t"], t["scale"]) for t in ts])
        w[row0:row0 + rows] = rn_bf16(v).to(torch.bfloat16)
        if "colsum_off" in ts[0]:
            cs = out.setdefault(f"{name}.colsum", packed[f"{name}.colsum"].clone())
            cs[row0:row0 + rows] = w[row0:row0 + rows].to(torch.float32).sum(dim=1)
            b = out.setdefault(f"{name}.bias", packed[f"{name}.bias"].clone())
            for t in ts:
                b[row0:row0 + rows] += torch.tensor(t["scale"], dtype=torch.float32) * t["dbias"]
    return out


def random_adapter_sd(cfg, seed, ranks=(4, 24), modules=None, alpha_every=3, prefix="", old_spelling=False, gain=1.0):
    """a random adapter state dict in diffusers / PEFT names over every target of ``cfg`` (or ``modules``), ranks dealt in turn, an ``alpha`` of
    r / 2 on every ``alpha_every``-th module.  With gain 1, |B A| is comparable to |W| (A ~ N(0, 1) K^-1/2 like W, B ~ N(0, 1))."""
    from sduss_amd import lora
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, (m, t) in enumerate(sorted(lora.lora_targets(cfg).items())):
        if modules is not None and m not in modules:
            continue
        r = ranks[i % len(ranks)]
        a, b = (".lora.down.weight", ".lora.up.weight") if old_spelling else (".lora_A.weight", ".lora_B.weight")
        sd[f"{prefix}{m}{a}"] = torch.randn((r, t.K), generator=g) * t.K ** -0.5
        sd[f"{prefix}{m}{b}"] = gain * torch.randn((t.rows, r), generator=g)
        if alpha_every and i % alpha_every == 0:
            sd[f"{prefix}{m}.alpha"] = torch.tensor(float(r) * 0.5)
    return sd
