"""The form matrix of the normalisation kernels: one case per instantiation, branch and edge of csrc/norm.hip and csrc/gn_halo_nchw.hip, each
naming in a comment the branch it targets and the rule that selects it.  Plain data plus the input builders, shared by the CPU comparator
test (tests/test_norm_forms_cpu.py) and the GPU runs (tests/test_norm_forms_gpu.py).

Input families (`fam`):
  a  randn * 1.5 + 0.7
  b  mean / std = 8: offsets of +-12 per row / per group, std 1.5          (the family that must discriminate on cancellation)
  c  mean / std = 32: offset 24, std 0.75                                  (the ill-conditioned probe; its bound is loose)
  d  (a) with one row / one group constant: the output there is beta / the shift within bound, and finite
  e  std 2^-7 about zero: eps = 1e-5 carries a good 10 % of the variance
  f  (sliced statistics) patches whose means differ by 4 std: whole-image statistics are far outside the bound
"""
import zlib

import torch

MAX_SEGS = 4                    # MX_MAX_SEGS (include/mxdenoise.h)
LN_EPS, MOD_EPS = 1e-5, 1e-6


def seed_of(name):
    return zlib.crc32(name.encode())


def _k(kind, name, **kw):
    kw.update(kind=kind, name=name)
    kw.setdefault("fam", "a")
    return kw


# ------------------------------------------------------------------------------------------------------------------------------------------
# The row norms share row_norm_kernel<VPL, CENTRE, Store> and ONE ladder (with_vpl): vpl = ceil(C / 8 / 64) -> <1> <2> <3> <4>, above 4 -> <8>;
# four rows a workgroup (row >= M exits).
# mx_layernorm: row_norm_kernel<VPL, true, AffineStore>
# ------------------------------------------------------------------------------------------------------------------------------------------
LN_CASES = [
    _k("ln", "ln_c8_m1", C=8, M=1, affine=True),                       # <1>, one lane of 64 holds data; M = 1: three waves exit
    _k("ln", "ln_c512_m5_plain", C=512, M=5, affine=False),             # <1> full; gamma == nullptr; M = 4k + 1
    _k("ln", "ln_c520_m7_b", C=520, M=7, affine=True, fam="b"),         # <2>, 65 chunks: one lane in the second chunk
    _k("ln", "ln_c1024_m6", C=1024, M=6, affine=True),                  # <2> full; M = 4k + 2
    _k("ln", "ln_c1032_m5_plain_b", C=1032, M=5, affine=False, fam="b"),  # <3>, 129 chunks
    _k("ln", "ln_c1536_m7_c", C=1536, M=7, affine=True, fam="c"),       # <3> full
    _k("ln", "ln_c1544_m6_d", C=1544, M=6, affine=True, fam="d"),       # <4>, 193 chunks; a constant row
    _k("ln", "ln_c2048_m1_plain", C=2048, M=1, affine=False),           # <4> full
    _k("ln", "ln_c2056_m5_e", C=2056, M=5, affine=True, fam="e"),       # <8> (vpl = 5), 257 chunks
    _k("ln", "ln_c4096_m6_b", C=4096, M=6, affine=True, fam="b"),       # <8> full
    _k("ln", "ln_c4096_m7_plain", C=4096, M=7, affine=False),           # <8> full, gamma == nullptr
    _k("ln", "ln_c520_m6_plain_d", C=520, M=6, affine=False, fam="d"),  # <2> ragged without affine; a constant row
]

# ------------------------------------------------------------------------------------------------------------------------------------------
# mx_layernorm_mod: row_norm_kernel<VPL, true, ModStore>; sample = row / rows_per_batch; scale / shift (and scale2 / shift2 when y2 is
# given) are column slices of ONE fp32 matrix [B, 6 C + 4] (ldmod = 6 C + 4 > C), NaN outside the slices
# ------------------------------------------------------------------------------------------------------------------------------------------
MOD_CASES = [
    _k("lnmod", "mod_c8_rpb1", C=8, B=5, rpb=1, dual=False),                      # <1> ragged; rows_per_batch = 1
    _k("lnmod", "mod_c512_rpb333_dual", C=512, B=2, rpb=333, dual=True),          # <1> full; rows_per_batch = 333 (M = 666 = 4k + 2)
    _k("lnmod", "mod_c520_rpb333_b", C=520, B=3, rpb=333, dual=False, fam="b"),   # <2> ragged (M = 999 = 4k + 3)
    _k("lnmod", "mod_c1024_rpb1_dual", C=1024, B=7, rpb=1, dual=True),            # <2> full
    _k("lnmod", "mod_c1032_rpb1_dual_b", C=1032, B=5, rpb=1, dual=True, fam="b"),  # <3> ragged
    _k("lnmod", "mod_c1536_rpb3_d", C=1536, B=3, rpb=3, dual=False, fam="d"),     # <3> full (the MMDiT width); a constant row
    _k("lnmod", "mod_c1544_rpb1", C=1544, B=6, rpb=1, dual=False),                # <4> ragged
    _k("lnmod", "mod_c2048_rpb5_dual_e", C=2048, B=2, rpb=5, dual=True, fam="e"),  # <4> full
    _k("lnmod", "mod_c2056_rpb1_c", C=2056, B=5, rpb=1, dual=False, fam="c"),     # <8> ragged
    _k("lnmod", "mod_c4096_rpb3_dual", C=4096, B=3, rpb=3, dual=True),            # <8> full
]

# mx_layernorm_mod_grouped: RowGroups lookup -- group of a row (r0), sample inside the group (b0 + (row - r0) / rpb), ldmod row stride
MODG_CASES = [
    _k("lnmod_grouped", "modg_n1", C=520, batches=[2], rpbs=[5], dual=False),                               # n = 1; 10 rows = 4k + 2
    _k("lnmod_grouped", "modg_n3_dual", C=1536, batches=[1, 2, 3], rpbs=[7, 1, 4], dual=True),              # a group of one-row samples; batches > 1 later (b0 = 1, 3); 21 rows
    _k("lnmod_grouped", "modg_n4_b", C=520, batches=[2, 1, 3, 2], rpbs=[3, 1, 5, 2], dual=False, fam="b"),  # n = MX_MAX_SEGS; 26 rows
]

# ------------------------------------------------------------------------------------------------------------------------------------------
# mx_rmsnorm: row_norm_kernel<VPL, false, RmsStore>.  Its own ladder once had no <3> rung: vpl == 3 ran <4> with an empty fourth chunk, which
# every loop skipped (ch < nch), so the two cases of that width compute the same bytes on either rung
# ------------------------------------------------------------------------------------------------------------------------------------------
RMS_CASES = [
    _k("rms", "rms_c8_m1", C=8, M=1),                        # <1> ragged
    _k("rms", "rms_c512_m301", C=512, M=301),                # <1> full; M = 4k + 1, many workgroups
    _k("rms", "rms_c520_m5_b", C=520, M=5, fam="b"),         # <2> ragged
    _k("rms", "rms_c1024_m5", C=1024, M=5),                  # <2> full
    _k("rms", "rms_c1032_m5_e", C=1032, M=5, fam="e"),       # <3> ragged: the third chunk holds one lane
    _k("rms", "rms_c1536_m301", C=1536, M=301),              # <3> full; many workgroups
    _k("rms", "rms_c2048_m1_d", C=2048, M=1, fam="d"),       # <4> full; the one row constant
    _k("rms", "rms_c2056_m5_c", C=2056, M=5, fam="c"),       # <8> (vpl = 5)
    _k("rms", "rms_c4096_m5", C=4096, M=5),                  # <8> full (the T5 width)
]

# ------------------------------------------------------------------------------------------------------------------------------------------
# mx_rmsnorm_heads: a wave covers 8 heads of one row; groups = ceil(heads_total / 8); waves = nbatch * rows_per_batch * groups, four a
# workgroup (wid >= total exits); heads below heads_q take wq and q_scale; ld = 64 heads_total + 8 (NaN in the padding columns); the rows
# outside [row_off, row_off + rows_per_batch) of every sample and the padding columns come back bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------------
HEADS_CASES = [
    _k("rms_heads", "heads_1_0", ht=1, hq=0, nbatch=1, rpb=5, batch_rows=5, row_off=0),        # one head of a group of 8 (7 idle), all k; 5 waves
    _k("rms_heads", "heads_6_3_off", ht=6, hq=3, nbatch=2, rpb=3, batch_rows=7, row_off=2),     # row_off > 0; 6 waves
    _k("rms_heads", "heads_8_8", ht=8, hq=8, nbatch=1, rpb=7, batch_rows=7, row_off=0),         # a full group, heads_q == heads_total; 7 waves
    _k("rms_heads", "heads_9_4_off_b", ht=9, hq=4, nbatch=3, rpb=3, batch_rows=6, row_off=3, fam="b"),   # second group holds one head; 18 waves
    _k("rms_heads", "heads_48_24", ht=48, hq=24, nbatch=2, rpb=5, batch_rows=5, row_off=0),     # the MMDiT's q | k row; 60 waves
    _k("rms_heads", "heads_9_4_e", ht=9, hq=4, nbatch=1, rpb=5, batch_rows=5, row_off=0, fam="e"),       # eps carries weight; 10 waves
]

# mx_row_stats: one wave a row, chunks strided by 64; writes two floats per row at pitch 8 floats (one slab of four)
STATS_CASES = [
    _k("row_stats", "stats_c8", C=8, M=5),                   # one lane holds data
    _k("row_stats", "stats_c520_b", C=520, M=5, fam="b"),    # 65 chunks: lane 0 takes two
    _k("row_stats", "stats_c1536_c", C=1536, M=5, fam="c"),  # 192 chunks: three a lane
]

# ------------------------------------------------------------------------------------------------------------------------------------------
# NHWC GroupNorm (mx_groupnorm_nhwc_cat / _grouped).  Routes: fold-in-apply (groups <= kFoldGroups = 64 and every problem exact): gn_stats
# with per-group sums + gn_apply<SILU, true>; otherwise gn_stats per channel + gn_fold + gn_apply<SILU, false>.  Geometry (gn_geom): tpr = C / 8
# threads a pixel, L = min(32, 1024 / tpr) pixel lanes, tile tw = patch or W, th = 256 / tw walked down to a divisor of patch or H, halved while
# the launch has fewer than two tiles a CU; apply blocks of ppb = min(8 L, H W) pixels.  A patch covering the image is exact.
# ------------------------------------------------------------------------------------------------------------------------------------------
def _gn(name, B, H, W, C, groups=32, patch=0, silu=True, c1=0, **kw):
    return _k("gn", name, B=B, H=H, W=W, C=C, groups=groups, patch=patch, silu=silu, c1=c1, **kw)


GN_CASES = [
    _gn("gn_fold_silu", 2, 16, 16, 320),                                  # fold-in-apply, SiLU; L = 25, ppb = 200: 256 pixels end in a partial block
    _gn("gn_fold_plain_b", 1, 16, 16, 320, silu=False, fam="b"),          # fold-in-apply without SiLU
    _gn("gn_fold_c64_b", 2, 16, 16, 64, fam="b"),                         # the shape of the CPU prototype: L = 32, ppb = 256
    _gn("gn_fold_c64_c", 2, 16, 16, 64, fam="c"),
    _gn("gn_fold_c64_d", 2, 16, 16, 64, silu=False, fam="d"),             # a constant group
    _gn("gn_fold_c64_e", 2, 16, 16, 64, fam="e"),
    _gn("gn_sliced_p8_f", 2, 16, 16, 320, patch=8, fam="f"),              # separate fold, patch > 0: mean of patch means / variances
    _gn("gn_sliced_p8_b", 1, 16, 16, 320, patch=8, silu=False, fam="b"),
    _gn("gn_sliced_p8_c64_d", 2, 16, 16, 64, patch=8, fam="d"),
    _gn("gn_g128_c1024", 1, 8, 8, 1024, groups=128),                      # groups > kFoldGroups: separate fold with patch == 0
    _gn("gn_g128_c1024_b", 2, 8, 8, 1024, groups=128, silu=False, fam="b"),
    _gn("gn_cat_192_of_320", 2, 16, 16, 320, c1=192),                     # concatenation read in place, fold-in-apply
    _gn("gn_cat_8_of_320_p8_f", 2, 16, 16, 320, c1=8, patch=8, fam="f"),  # uneven concatenation: the first source is one 16-byte vector a pixel
    _gn("gn_cat_8_of_320_b", 1, 7, 9, 320, c1=8, fam="b"),
    _gn("gn_c1920_7x9", 1, 7, 9, 1920),                                   # tpr = 240 does not divide 1024 (L = 4, 64 idle threads); H, W odd: th walks 28 -> 7
    _gn("gn_c2560_16x40_b", 1, 16, 40, 2560, fam="b"),                    # tpr = 320 (L = 3); H != W; th walks 6 -> 4, halved
    _gn("gn_2x264", 1, 2, 264, 320),                                      # W > 256: th = 256 / 264 = 0 -> 1
    _gn("gn_2x2_p2_B9", 9, 2, 2, 320, patch=2),                           # patch >= H, W collapses to exact; B = 9; four pixels an image
    _gn("gn_4x6_p2_f", 1, 4, 6, 64, patch=2, fam="f"),                    # the smallest patch: tiles of four pixels (the workspace bound's edge)
    _gn("gn_8x24_p8_f", 2, 8, 24, 64, patch=8, fam="f"),                  # H == patch < W: one row of three patches
    _gn("gn_16x40_p8_f", 1, 16, 40, 320, patch=8, silu=False, fam="f"),   # H != W with patches
    _gn("gn_16x16_p32", 2, 16, 16, 64, patch=32),                         # patch >= H, W -> exact, so fold-in-apply
    _gn("gn_B9_8x8_b", 9, 8, 8, 320, fam="b"),                            # B = 9
]

# a grouped launch of MX_MAX_SEGS problems of different sizes: each must also equal its separate launch bit for bit
GNG_CASES = [
    _k("gn_grouped", "gng_exact4", C=320, groups=32, patch=0, silu=True, c1=0, probs=[(2, 16, 16), (1, 24, 8), (3, 7, 9), (1, 2, 264)]),
    _k("gn_grouped", "gng_sliced4_cat_f", C=320, groups=32, patch=8, silu=True, c1=192, probs=[(2, 16, 16), (1, 8, 24), (1, 24, 24), (3, 8, 8)], fam="f"),
]

# mx_groupnorm_nhwc_from_partials: gn_fold_kernel's closed form on given partial sums of x - c over chunks of `chunk` pixels, layout
# [B][H W / chunk][C][2]; c = add_bias + add_rowbias (row stride ldrb = C + 8, NaN in the padding)
GNP_CASES = [
    _k("gn_partials", "gnp_bias_chunk16", B=2, H=16, W=16, C=320, groups=32, silu=True, chunk=16, bias=True, rowbias=False),
    _k("gn_partials", "gnp_bias_rowbias_chunk64_b", B=2, H=16, W=16, C=320, groups=32, silu=True, chunk=64, bias=True, rowbias=True, fam="b"),
    _k("gn_partials", "gnp_neither_chunk16_b", B=1, H=8, W=24, C=64, groups=32, silu=False, chunk=16, bias=False, rowbias=False, fam="b"),
    _k("gn_partials", "gnp_bias_rowbias_chunk16_g128", B=3, H=8, W=8, C=1024, groups=128, silu=True, chunk=16, bias=True, rowbias=True),
]


def gn_tile(B, H, W, patch, cus=256):
    """(th, tw) of gn_geom on a 256-CU device"""
    if patch >= H and patch >= W:
        patch = 0
    tw = patch or W
    th = max(256 // tw, 1)
    hlim = patch or H
    while hlim % th:
        th -= 1
    while th > 1 and th * tw >= 64 and B * (H // th) * (W // tw) < 2 * cus:
        th //= 2
        while hlim % th:
            th -= 1
    return th, tw


def gn_fold_in_apply(groups, patch, sizes):
    return groups <= 64 and all(patch == 0 or (patch >= h and patch >= w) for _b, h, w in sizes)


def gn_terms(c, B, H, W, fold):
    """n_t of a problem: the terms of one fp32 partial sum -- the tile's pixels, times the group's channels on the fold-in-apply route"""
    th, tw = gn_tile(B, H, W, c["patch"])
    return th * tw * (c["C"] // c["groups"] if fold else 1)


# ------------------------------------------------------------------------------------------------------------------------------------------
# NCHW GroupNorm + halo (mx_groupnorm_halo, mx_halo_only): six patches of two latents on the asymmetric adjacency table of test_ops_gpu.py.
# VE = 16 / sizeof(T) elements a 16-byte access.  moments_kernel: scalar when cpg H W % VE != 0; apply kernels: scalar when W % VE != 0 (gather)
# / H W % VE != 0 (plain); apply_gather stores PB = clamp(2048 / (H W), 1, 32) padded planes a block as 16-byte, 8-byte or element stores by
# the block's byte count
# ------------------------------------------------------------------------------------------------------------------------------------------
NCHW_SHAPES = [
    # name, C, cpg, H, W
    ("6x10", 16, 4, 6, 10),     # H != W (per = 2 W2 + 2 H); W % 8 and W % 4 != 0: scalar interiors for every dtype; moments vectorised (240)
    ("7x7c6", 6, 3, 7, 7),      # odd width; cpg H W = 147: scalar moments for every dtype; 36 planes = blocks of 32 + 4: 16-byte, then 8-byte stores (2-byte types)
    ("7x7c3", 3, 3, 7, 7),      # 18 planes of 81 in one block: 2916 bytes -> element stores (2-byte types), 5832 -> 8-byte stores (fp32)
    ("8x8", 16, 4, 8, 8),       # PB = 32 > C: a block spans two patches
    ("32x32", 4, 2, 32, 32),    # PB = 2
]
NCHW_CASES = [_k("gn_nchw", f"nchw_{s[0]}_{dn}_pad{p}", shape=s, dtype=dn, padding=p)
              for s in NCHW_SHAPES for dn in ("f32", "f16", "bf16") for p in (1, 0)]
NCHW_N, NCHW_LAT_OFF, NCHW_PMAP = 6, [0, 3, 6], [1, 1, 1, 2, 2, 2]
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

ROW_CASES = LN_CASES + MOD_CASES + MODG_CASES + RMS_CASES + HEADS_CASES + STATS_CASES
ALL_CASES = ROW_CASES + GN_CASES + GNG_CASES + GNP_CASES + NCHW_CASES


def asymmetric_table(n):
    """tests/test_ops_gpu.py::_asymmetric_table: one-directional links, a link between two latents, a self link; one writer a halo side"""
    pidx = torch.full((n, 4), -1, dtype=torch.int32)
    pidx[0, 3] = 1
    pidx[1, 2] = 4
    pidx[4, 0] = 2
    pidx[3, 1] = 3
    pidx[5, 3] = 0
    pidx[2, 0] = 5
    return pidx.reshape(-1)


# ---- inputs ----

def rows_input(fam, M, C, gen):
    """[M, C] bf16 of the family"""
    z = torch.randn(M, C, generator=gen)
    if fam == "b":
        x = z * 1.5 + 12.0 * (1.0 - 2.0 * (torch.arange(M) % 2)).view(M, 1)
    elif fam == "c":
        x = z * 0.75 + 24.0
    elif fam == "e":
        x = z * 2.0 ** -7
    else:
        x = z * 1.5 + 0.7
        if fam == "d":
            x[M // 2] = 3.0
    return x.to(torch.bfloat16)


def nhwc_input(fam, B, H, W, C, groups, patch, gen):
    """[B, H, W, C] bf16 of the family"""
    z = torch.randn(B, H, W, C, generator=gen)
    cpg = C // groups
    grp = torch.arange(C) // cpg
    if fam == "b":
        sign = 1.0 - 2.0 * ((grp.view(1, C) + torch.arange(B).view(B, 1)) % 2)
        x = z * 1.5 + 12.0 * sign.view(B, 1, 1, C)
    elif fam == "c":
        x = z * 0.75 + 24.0
    elif fam == "e":
        x = z * 2.0 ** -7
    elif fam == "f":
        p = patch
        pid = (torch.arange(H).view(H, 1) // p) * ((W + p - 1) // p) + torch.arange(W).view(1, W) // p
        x = z * 1.5 + 0.7 + 6.0 * ((pid % 3) - 1.0).view(1, H, W, 1)
    else:
        x = z * 1.5 + 0.7
        if fam == "d":
            x[0, :, :, cpg:2 * cpg] = 3.0                    # group 1 of image 0
    return x.to(torch.bfloat16)


def nchw_input(shape, dtype, gen):
    """[6, C, H, W]: the second latent five times as wide, every patch around its own mean (3 n)"""
    _n, C, _cpg, H, W = shape
    N = NCHW_N
    x = torch.randn(N, C, H, W, generator=gen) * torch.tensor([1., 1., 1., 5., 5., 5.]).view(N, 1, 1, 1) + 3.0 * torch.arange(N).view(N, 1, 1, 1).float()
    return x.to(dtype)


def affine(C, gen, dtype=torch.float32):
    return (torch.randn(C, generator=gen) * 0.5 + 1.0).to(dtype), torch.randn(C, generator=gen).to(dtype)


def eps_of(c):
    if c["fam"] == "e" or c["kind"] in ("ln", "gn", "gn_grouped", "gn_partials", "gn_nchw"):
        return LN_EPS
    return MOD_EPS


Q_SCALE = 0.125 * 1.4426950408889634      # what the MMDiT folds into q: softmax scale in the log2 domain


def build(c, dev):
    """the logical operands of a case on `dev` (generated on the host from the case's name): what the reference, the emulation and the launch share"""
    gen = torch.Generator().manual_seed(seed_of(c["name"]))
    k, fam = c["kind"], c["fam"]
    p = dict(eps=eps_of(c))
    to = lambda t: t.to(dev)
    if k == "ln":
        p["x"] = to(rows_input(fam, c["M"], c["C"], gen))
        p["gamma"], p["beta"] = [to(t) for t in affine(c["C"], gen)] if c["affine"] else (None, None)
    elif k in ("lnmod", "lnmod_grouped"):
        C = c["C"]
        if k == "lnmod":
            B, sample = c["B"], torch.arange(c["B"] * c["rpb"]) // c["rpb"]
        else:
            B = sum(c["batches"])
            sample = torch.cat([b0 + torch.arange(b * r) // r for b0, b, r in
                                zip([sum(c["batches"][:i]) for i in range(len(c["batches"]))], c["batches"], c["rpbs"])])
        p["x"] = to(rows_input(fam, sample.numel(), C, gen))
        mod = torch.full((B, 6 * C + 4), float("nan"))
        for j in (0, 1, 3, 4):                               # shift | scale | (gate) | shift2 | scale2 | (gate2) | four more
            mod[:, j * C:(j + 1) * C] = torch.randn(B, C, generator=gen) * (0.3 if j in (1, 4) else 1.0)
        p["mod"] = mod = to(mod)
        p["shift"], p["scale"], p["shift2"], p["scale2"] = (mod[:, j * C:(j + 1) * C] for j in (0, 1, 3, 4))
        p["sample"] = to(sample)
    elif k == "rms":
        p["x"] = to(rows_input(fam, c["M"], c["C"], gen))
        p["w"] = to(affine(c["C"], gen)[0])
    elif k == "rms_heads":
        D = 64 * c["ht"]
        rows = c["nbatch"] * c["batch_rows"]
        buf = torch.full((rows, D + 8), float("nan"), dtype=torch.bfloat16)
        buf[:, :D] = rows_input(fam, rows, D, gen)
        p["buf"] = to(buf)
        r = torch.arange(c["nbatch"] * c["rpb"])
        p["rows"] = to((r // c["rpb"]) * c["batch_rows"] + c["row_off"] + r % c["rpb"])
        p["wq"], p["wk"] = to(affine(64, gen)[0]), to(affine(64, gen)[0])
        p["q_scale"] = Q_SCALE
    elif k == "row_stats":
        p["x"] = to(rows_input(fam, c["M"], c["C"], gen))
    elif k in ("gn", "gn_partials"):
        p["x"] = to(nhwc_input(fam, c["B"], c["H"], c["W"], c["C"], c["groups"], c.get("patch", 0), gen))
        p["gamma"], p["beta"] = [to(t) for t in affine(c["C"], gen)]
        if k == "gn_partials":
            B, H, W, C, chunk = c["B"], c["H"], c["W"], c["C"], c["chunk"]
            bias = torch.randn(C, generator=gen) if c["bias"] else None
            rb = torch.full((B, C + 8), float("nan"))
            rb[:, :C] = torch.randn(B, C, generator=gen)
            rb = to(rb) if c["rowbias"] else None
            p["bias"], p["rbbuf"], p["rowbias"] = (to(bias) if c["bias"] else None), rb, (rb[:, :C] if c["rowbias"] else None)
            cc = torch.zeros(B, 1, C, device=dev)
            if c["bias"]:
                cc = cc + p["bias"].view(1, 1, C)
            if c["rowbias"]:
                cc = cc + p["rowbias"].reshape(B, 1, C)
            d = (p["x"].float().reshape(B, H * W, C) - cc).reshape(B, H * W // chunk, chunk, C)      # fp32 sums of x - c, as a producer leaves them
            p["part"] = torch.stack([d.sum(2), (d * d).sum(2)], dim=-1).contiguous()
    elif k == "gn_grouped":
        p["xs"] = [to(nhwc_input(fam, b, h, w, c["C"], c["groups"], c["patch"], gen)) for b, h, w in c["probs"]]
        p["gamma"], p["beta"] = [to(t) for t in affine(c["C"], gen)]
    elif k == "gn_nchw":
        dt = DTYPES[c["dtype"]]
        p["x"] = to(nchw_input(c["shape"], dt, gen))
        p["gamma"], p["beta"] = [to(t) for t in affine(c["shape"][1], gen, dt)]
        p["pidx"] = asymmetric_table(NCHW_N)
    else:
        raise ValueError(k)
    return p
