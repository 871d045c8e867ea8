"""The comparator of the normalisation matrix on the CPU (no GPU): for every case of tests/norm_form_cases.py the correctly rounded fp64
reference, and a plain fp32 torch emulation of the kernel's stated arithmetic (single-pass tile sums for GroupNorm, two passes for the row
norms), stay inside the per-element bound of tests/norm_ref.py; and each of a list of subtle mutants of that emulation is flagged."""
import math

import pytest
import torch

import norm_form_cases as NC
import norm_ref as R


def _out_dtype(c):
    if c["kind"] == "row_stats":
        return torch.float32
    return NC.DTYPES[c["dtype"]] if c["kind"] == "gn_nchw" else torch.bfloat16


# ---- the emulation: fp32 torch, in the kernels' order of operations; `mut` names one deliberate defect ----

def _rows(x, eps, centre, mut):
    xf = x.float()
    C = xf.shape[1]
    if mut == "eps100":
        eps = eps * 100
    if centre:
        xf = xf - xf.sum(1, keepdim=True) / C
    rstd = torch.rsqrt((xf * xf).sum(1, keepdim=True) / C + eps)
    if mut == "rstd_1pct":
        rstd = rstd * 1.01
    return xf * rstd


def _gn_coef(mean, var, gamma, beta, eps, mut):
    """fp64 fold -> fp32 scale / shift per (image, channel), as gn_fold_kernel / gn_apply_kernel<.., true> finish them"""
    if mut == "eps100":
        eps = eps * 100
    rstd = 1.0 / torch.sqrt(var + eps)
    if mut == "rstd_1pct":
        rstd = rstd * 1.01
    cpg = gamma.numel() // mean.shape[1]
    g = gamma.double()
    if mut == "rstd_1pct_group":                                    # ... of one group only: the one whose gammas are smallest
        rstd = rstd.clone()
        rstd[:, g.abs().reshape(-1, cpg).amax(1).argmin()] *= 1.01
    if mut == "gamma_neighbour":
        g = g.clone(); g[3] = g[4]
    rg = rstd.repeat_interleave(cpg, 1) * g
    return rg.float(), (beta.double() - rg * mean.repeat_interleave(cpg, 1)).float()


def _gn_nhwc(c, x, gamma, beta, eps, B, H, W, fold, mut):
    C, G = c["C"], c["groups"]
    patch = 0 if (mut == "whole_image_stats" or (c["patch"] >= H and c["patch"] >= W)) else c["patch"]
    th, tw = NC.gn_tile(B, H, W, patch)
    xf = x.float()
    t = xf.reshape(B, H // th, th, W // tw, tw, C)
    s, q = t.sum((2, 4)), (t * t).sum((2, 4))                       # fp32 sums per (image, tile, channel)
    if fold:                                                        # ... and per group, still fp32
        s, q = s.reshape(*s.shape[:3], G, -1).sum(-1, keepdim=True), q.reshape(*q.shape[:3], G, -1).sum(-1, keepdim=True)
    ph, pw = patch or H, patch or W
    shape = (B, H // ph, ph // th, W // pw, pw // tw, G, -1)
    cnt = ph * pw * (C // G)
    m = s.double().reshape(shape).sum((2, 4, 6)) / cnt              # [B, ppy, ppx, G]
    v = (q.double().reshape(shape).sum((2, 4, 6)) / cnt - m * m).clamp_min(0.0)
    sc, sf = _gn_coef(m.mean((1, 2)), v.mean((1, 2)), gamma, beta, eps, mut)
    y = xf * sc.view(B, 1, 1, C) + sf.view(B, 1, 1, C)
    if c["silu"]:
        y = y * torch.sigmoid(y)
    return y.to(torch.bfloat16)


def _gn_nchw(c, p, mut):
    x, eps = p["x"], p["eps"]
    N, C, H, W = x.shape
    cpg = c["shape"][2]
    G = C // cpg
    xf = x.float()
    t = xf.reshape(N, G, -1)
    cnt = t.shape[2]
    m = t.sum(2).double() / cnt
    v = ((t * t).sum(2).double() / cnt - m * m).clamp_min(0.0)
    m, v = m.float(), v.float()                                     # stored between the launches
    mean2, rstd2 = torch.empty_like(m), torch.empty_like(m)
    for n in range(N):
        lo, hi = NC.NCHW_LAT_OFF[NC.NCHW_PMAP[n] - 1], NC.NCHW_LAT_OFF[NC.NCHW_PMAP[n]]
        mean2[n] = m[lo:hi].sum(0) / float(hi - lo)
        rstd2[n] = torch.rsqrt(v[lo:hi].sum(0) / float(hi - lo) + eps)
    if mut == "rstd_1pct":
        rstd2 = rstd2 * 1.01
    sc = rstd2.repeat_interleave(cpg, 1) * p["gamma"].float()
    sf = p["beta"].float() - sc * mean2.repeat_interleave(cpg, 1)
    y = (xf * sc.view(N, C, 1, 1) + sf.view(N, C, 1, 1)).to(x.dtype)
    if not c["padding"]:
        return y
    out = R.halo_gather(y, p["pidx"])
    if mut == "halo_receiver_stats":                                # the frame from the sender's pixels but the RECEIVER's scale / shift
        raw = R.halo_gather(x, p["pidx"]).float()
        frame = R.halo_gather(torch.ones_like(x), p["pidx"]).bool()
        frame[:, :, 1:-1, 1:-1] = False
        alt = (raw * sc.view(N, C, 1, 1) + sf.view(N, C, 1, 1)).to(x.dtype)
        out = torch.where(frame, alt, out)
    return out


def emulate(c, p, mut=None):
    k, eps = c["kind"], p["eps"]
    bf = torch.bfloat16
    if k == "ln":
        n = _rows(p["x"], eps, True, mut)
        if p["gamma"] is None:
            return {"y": n.to(bf)}
        g = p["gamma"].clone()
        if mut == "gamma_neighbour":
            g[3] = g[4]
        return {"y": (n * g + p["beta"]).to(bf)}
    if k in ("lnmod", "lnmod_grouped"):
        n = _rows(p["x"], eps, True, mut)
        sample = p["sample"].clone()
        if mut == "mod_next_sample":
            sample[1] = sample[1] + 1
        if mut == "group_off_by_one":                               # the last row of group 0 looked up in group 1: its first sample
            r0 = c["batches"][0] * c["rpbs"][0]
            sample[r0 - 1] = c["batches"][0]
        out = {"y": (n * (1.0 + p["scale"][sample]) + p["shift"][sample]).to(bf)}
        if c["dual"]:
            out["y2"] = (n * (1.0 + p["scale2"][sample]) + p["shift2"][sample]).to(bf)
        return out
    if k == "rms":
        return {"y": (_rows(p["x"], eps, False, mut) * p["w"]).to(bf)}
    if k == "rms_heads":
        D = 64 * c["ht"]
        x = p["buf"][p["rows"], :D]
        n = _rows(x.reshape(-1, 64), eps, False, mut).reshape(-1, c["ht"], 64)
        hq = c["hq"] + (1 if mut == "q_scale_on_k" else 0)
        isq = (torch.arange(c["ht"]) < hq).view(1, -1, 1)
        isw = (torch.arange(c["ht"]) < c["hq"]).view(1, -1, 1)
        n = n * torch.where(isq, torch.tensor(p["q_scale"], dtype=torch.float32), torch.tensor(1.0))
        return {"y": (n * torch.where(isw, p["wq"].view(1, 1, 64), p["wk"].view(1, 1, 64))).to(bf).reshape(-1, D)}
    if k == "row_stats":
        xf = p["x"].float()
        return {"stats": torch.stack([xf.sum(1), (xf * xf).sum(1)], 1)}
    if k == "gn":
        fold = NC.gn_fold_in_apply(c["groups"], c["patch"], [(c["B"], c["H"], c["W"])])
        return {"y": _gn_nhwc(c, p["x"], p["gamma"], p["beta"], eps, c["B"], c["H"], c["W"], fold, mut)}
    if k == "gn_grouped":
        fold = NC.gn_fold_in_apply(c["groups"], c["patch"], c["probs"])
        return {f"y{i}": _gn_nhwc(c, x, p["gamma"], p["beta"], eps, b, h, w, fold, mut) for i, (x, (b, h, w)) in enumerate(zip(p["xs"], c["probs"]))}
    if k == "gn_partials":
        mean, var, _q = R.fold_partials(p["part"], c["chunk"], c["groups"], p["bias"], p["rowbias"])
        sc, sf = _gn_coef(mean, var, p["gamma"], p["beta"], eps, mut)
        B, C = c["B"], c["C"]
        y = p["x"].float() * sc.view(B, 1, 1, C) + sf.view(B, 1, 1, C)
        if c["silu"]:
            y = y * torch.sigmoid(y)
        return {"y": y.to(bf)}
    if k == "gn_nchw":
        return {"y": _gn_nchw(c, p, mut)}
    raise ValueError(k)


def _count(c, p, ref, got):
    """(violations over all outputs of the case, worst ratio)"""
    n, worst = 0, 0.0
    for name, (r, b) in ref.items():
        v, ratio = R.violations(got[name], r, b)
        n, worst = n + v, max(worst, ratio)
    return n, worst


def _case(name):
    return next(c for c in NC.ALL_CASES if c["name"] == name)


@pytest.fixture(scope="module")
def refs():
    """operands and reference of every case, computed once"""
    out = {}
    for c in NC.ALL_CASES:
        p = NC.build(c, torch.device("cpu"))
        out[c["name"]] = (p, R.reference(c, p))
    return out


def test_case_names_are_unique_and_sizes_small():
    names = [c["name"] for c in NC.ALL_CASES]
    assert len(set(names)) == len(names)
    for c in NC.GN_CASES:
        assert c["B"] * c["H"] * c["W"] * c["C"] <= 2 << 20
        assert c["patch"] == 0 or (c["H"] % c["patch"] == 0 and c["W"] % c["patch"] == 0) or (c["patch"] >= c["H"] and c["patch"] >= c["W"])


@pytest.mark.parametrize("c", NC.ALL_CASES, ids=lambda c: c["name"])
def test_reference_and_emulation_stay_inside_the_bound(refs, c):
    p, ref = refs[c["name"]]
    for name, (r, b) in ref.items():
        assert torch.isfinite(r).all() and torch.isfinite(b).all(), f"{c['name']} {name}: reference or bound not finite"
        R.assert_within(r.to(_out_dtype(c)), r, b, f"{c['name']} {name}: the correctly rounded reference")
    got = emulate(c, p)
    for name, (r, b) in ref.items():
        R.assert_within(got[name], r, b, f"{c['name']} {name}: the fp32 emulation")


def test_constant_row_and_group_give_the_shift(refs):
    """family (d): where the input is constant the reference is beta (the modulation's shift, zero without an affine) and the bound stays small"""
    p, ref = refs["ln_c1544_m6_d"]
    r, b = ref["y"]
    assert torch.allclose(r[3], p["beta"].double(), atol=1e-9) and b[3].max() < 0.05 * (1 + p["beta"].abs().max())
    p, ref = refs["gn_fold_c64_d"]
    r, b = ref["y"]
    assert torch.allclose(r[0, :, :, 2:4], p["beta"].double()[2:4].expand(16, 16, 2), atol=1e-9)
    assert b[0, :, :, 2:4].max() < 0.05 * (1 + p["beta"].abs().max())


# mutant -> the cases that must flag it
MUTANTS = [
    ("gamma_neighbour", ["ln_c520_m7_b", "gn_fold_silu", "gn_sliced_p8_f", "gnp_bias_chunk16"]),      # one channel's gamma from its neighbour
    ("mod_next_sample", ["mod_c520_rpb333_b", "mod_c1024_rpb1_dual", "modg_n3_dual"]),               # one row's modulation from the next sample
    ("group_off_by_one", ["modg_n3_dual", "modg_n4_b"]),                                             # group index off by one at a group boundary
    ("whole_image_stats", ["gn_sliced_p8_f", "gn_8x24_p8_f", "gn_4x6_p2_f", "gn_16x40_p8_f", "gng_sliced4_cat_f"]),   # exact where sliced was asked, family (f)
    ("eps100", ["ln_c2056_m5_e", "mod_c2048_rpb5_dual_e", "rms_c1032_m5_e", "heads_9_4_e", "gn_fold_c64_e"]),          # eps times 100, family (e)
    ("rstd_1pct", ["ln_c8_m1", "ln_c520_m7_b", "rms_c1024_m5", "rms_c520_m5_b", "heads_48_24", "gn_fold_silu", "gn_fold_c64_b", "gn_g128_c1024_b",
                   "nchw_8x8_bf16_pad1", "nchw_6x10_f32_pad0"]),                                     # rstd off by 1 %, families (a) and (b)
    ("q_scale_on_k", ["heads_6_3_off", "heads_9_4_off_b", "heads_1_0"]),                             # q_scale applied to a k head
    ("halo_receiver_stats", ["nchw_8x8_bf16_pad1", "nchw_6x10_f16_pad1", "nchw_7x7c6_f32_pad1"]),    # a halo cell with the receiver's statistics
]


@pytest.mark.parametrize("mut,names", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_comparator_flags_mutant(refs, mut, names):
    for name in names:
        c = _case(name)
        p, ref = refs[name]
        assert _count(c, p, ref, emulate(c, p))[0] == 0
        n, ratio = _count(c, p, ref, emulate(c, p, mut))
        assert n > 0, f"{mut} on {name} is not flagged (worst err / bound = {ratio:.3g})"


def _close(got, want, rel):
    """tests/test_ops_gpu.py's global criterion"""
    return (got.double() - want).abs().max().item() <= rel * (want.abs().max().item() + 1e-6)


def test_the_global_criterion_lets_the_rstd_mutant_through(refs):
    """rstd off by 1 % on family (b) against the old max|err| <= 2^-7 max|want| of test_layernorm / test_groupnorm_nhwc.  Off in EVERY group it
    moves the largest element by 1 % > 2^-7, so the old criterion sees it, at 1.1 to 1.5 times its tolerance on these cases; off in ONE group
    (the one with the smallest gammas, whose outputs stay below the tensor's maximum) it passes the old criterion, and the elementwise bound
    flags both -- the gap this matrix closes"""
    for name in ("gn_fold_c64_b", "gn_fold_plain_b", "gn_sliced_p8_b"):
        c = _case(name)
        p, ref = refs[name]
        got = emulate(c, p, "rstd_1pct_group")
        assert _count(c, p, ref, got)[0] > 0, name
        assert _close(got["y"], ref["y"][0], 2.0 ** -7), name
        assert _count(c, p, ref, emulate(c, p, "rstd_1pct"))[0] > 0, name


def test_comparator_flags_nan_and_guard(refs):
    c = _case("gn_fold_silu")
    p, ref = refs[c["name"]]
    r, b = ref["y"]
    good = emulate(c, p)["y"]
    bad = good.clone()
    bad[1, 3, 5, 7] = math.nan                                        # one element NaN
    assert R.violations(good, r, b)[0] == 0 and R.violations(bad, r, b)[0] == 1
    rows = c["B"] * c["H"] * c["W"]
    buf, view = R.guarded(rows, c["C"], c["C"], torch.bfloat16, "cpu")
    view.copy_(good.reshape(rows, c["C"]))
    assert R.guard_violations(buf, rows, c["C"]) == 0
    buf[rows, 0] = 0                                                  # one guard element changed: the first past the last image
    assert R.guard_violations(buf, rows, c["C"]) == 1
    sbuf, sview = R.guarded(5, 2, 8, torch.float32, "cpu")            # mx_row_stats: the entries past a row's two floats
    sview.zero_()
    assert R.guard_violations(sbuf, 5, 2) == 0
    sbuf[2, 2] = 0
    assert R.guard_violations(sbuf, 5, 2) == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_halo_gather_equals_the_oracles_scatter(dtype):
    """norm_ref.halo_gather against the oracle's literal sender-driven scatter, on the asymmetric table and a non-square plane"""
    from oracle import patch_ref
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 4, 6, 10, generator=g).to(dtype)
    pidx = NC.asymmetric_table(6)
    assert torch.equal(R.halo_gather(x, pidx).view(torch.uint8), patch_ref.mock_groupnorm(x, pidx).view(torch.uint8))
