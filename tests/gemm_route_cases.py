"""The route sweep: a deterministic list of mx_gemm / mx_conv3x3 descriptors (fake 16-byte-aligned pointers, host only) that crosses the
epilogue and operand variants with a pruned (M, N, K) grid around every boundary the GEMM dispatch branches on, and one descriptor per rule
of its validation, each violating exactly that rule.  tests/golden/gemm_route_table.json holds the library's answers for all of them as
recorded before the dispatch was gathered into gemm_dispatch.cpp; tests/test_gemm_route_cpu.py asserts they have not moved.

    PYTHONPATH=. python tests/gemm_route_cases.py --record    rewrites the table from the library that is loaded (MXDENOISE_LIB selects it)
"""
import ctypes as C
import json
import os

import kernel_form_cases as KC
from sduss_amd import lib as L

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_route_table.json")

S, GT, G = L.EPI_SILU, L.EPI_GELU_TANH, L.EPI_GELU
QKV, RMS, GEGLU, F32, RB = L.EPI_QKV, L.EPI_RMSNORM, L.EPI_GEGLU, L.EPI_OUT_F32, L.EPI_RES_BCAST

# the boundaries the chooser branches on: small-M (16 / 17), one 128-row tile, one 256-row tile, a chip's worth of 256-row tiles (8192), the
# 256 x 256 kernel's domain (32768); N at the small conv, the 160 / 128 / 256 panels, a ragged 1288, the q|k|v widths and GEGLU's 10240;
# K at one tile, the pipelined kernels' minimum, the split-K threshold (16 K tiles) and a long K
MS = [16, 17, 127, 128, 129, 255, 256, 8191, 8192, 8193, 32768]
NS = [4, 16, 128, 160, 256, 1280, 1288, 1920, 2304, 10240]
KS = [64, 128, 1024, 5120]
MS_WIDE = [1, 4] + MS[:7] + [512, 2048, 4096] + MS[7:] + [16384]       # the plain variants: also the small-M stream and the split-K range
NS_WIDE = NS + [320, 640, 1024, 5120]
KS_WIDE = KS + [320, 1280, 2560]
MS_SPLIT = [128, 129, 255, 256, 512, 2048, 8192]                        # forced slice counts: where a 128-row tiling can be chosen


def _rpb(M):
    """rows per batch of a variant with per-sample vectors: two batches where M allows"""
    return M // 2 if M % 2 == 0 and M >= 32 else M


def _gemm_variants():
    """(name, keyword arguments of kernel_form_cases._g as a function of (M, N, K) or None to skip the point, grid)"""
    base = (MS, NS, KS)
    v = []

    def add(name, fn, grid=base):
        v.append((name, fn, grid))
    add("plain", lambda M, N, K: {}, (MS_WIDE, NS_WIDE, KS_WIDE))
    add("nobias", lambda M, N, K: dict(bias=False))
    add("res_silu", lambda M, N, K: dict(residual=True, flags=S))
    add("tanh", lambda M, N, K: dict(flags=GT))
    add("res_gelu_scale", lambda M, N, K: dict(residual=True, flags=G, out_scale=0.5))
    add("rowbias_gate", lambda M, N, K: dict(rowbias=True, gate=True, rpb=_rpb(M)))
    add("rowbias", lambda M, N, K: dict(rowbias=True, rpb=_rpb(M)))
    add("rowbias_rpb15", lambda M, N, K: dict(rowbias=True, rpb=15))
    add("geglu", lambda M, N, K: dict(flags=GEGLU) if N % 128 == 0 else None)
    add("geglu_tanh", lambda M, N, K: dict(flags=GEGLU | L.EPI_GEGLU_TANH) if N % 128 == 0 else None)
    for seg, period in [(64, 2), (64, 3), (128, 3), (320, 2), (512, 2), (640, 3), (96, 2)]:
        add(f"qkv{seg}x{period}", lambda M, N, K, seg=seg, period=period:
            dict(flags=QKV, seg=seg, period=period, rpb=_rpb(M)) if N % (seg * period) == 0 else None)
    add("qkv64x3_rms", lambda M, N, K: dict(flags=QKV | RMS, seg=64, period=3, rpb=_rpb(M), rms=True, out_scale=0.125)
        if N % 192 == 0 and N % 128 == 0 else None)
    add("qkv64x2_remap", lambda M, N, K: dict(flags=QKV, seg=64, period=2, rpb=_rpb(M), arem=(_rpb(M) + 77, 77), crem=(_rpb(M) + 5, 4))
        if N % 128 == 0 else None)
    add("f32", lambda M, N, K: dict(flags=F32))
    add("f32_silu_res", lambda M, N, K: dict(flags=F32 | S, residual=True))
    add("res_bcast", lambda M, N, K: dict(flags=RB, residual=True, rpb=_rpb(M)))
    add("a2", lambda M, N, K: dict(a2=64) if K >= 128 else None)
    add("a2_res", lambda M, N, K: dict(a2=K // 2, residual=True) if K >= 128 else None)
    add("ln_stats", lambda M, N, K: dict(ln="stats", ln_slabs=2))
    add("ln_stats_geglu", lambda M, N, K: dict(ln="stats", ln_slabs=1, flags=GEGLU) if N % 128 == 0 else None)
    add("ln_stats_qkv64x2", lambda M, N, K: dict(ln="stats", ln_slabs=3, flags=QKV, seg=64, period=2, rpb=_rpb(M)) if N % 128 == 0 else None)
    add("stats_out", lambda M, N, K: dict(stats_out=True))
    add("stats_out_res", lambda M, N, K: dict(stats_out=True, residual=True))
    add("stats_out_ln_stats", lambda M, N, K: dict(stats_out=True, ln="stats", ln_slabs=2))
    add("ln_final_out", lambda M, N, K: dict(stats_out=True, ln_final_out=True))
    add("ln_final", lambda M, N, K: dict(ln="final"))
    add("ln_final_geglu", lambda M, N, K: dict(ln="final", flags=GEGLU) if N % 128 == 0 else None)
    add("ln_final_qkv64x2", lambda M, N, K: dict(ln="final", flags=QKV, seg=64, period=2, rpb=_rpb(M)) if N % 128 == 0 else None)
    add("ln_final_silu", lambda M, N, K: dict(ln="final", flags=S))          # no 256 x 256 instantiation carries it: form -1 everywhere
    add("gn_part", lambda M, N, K: dict(gn_part=True))
    add("gn_part_rowbias", lambda M, N, K: dict(gn_part=True, rowbias=True, rpb=_rpb(M)))
    add("c_misaligned", lambda M, N, K: dict(c_off=8))
    add("ldc_mod8", lambda M, N, K: dict(ldc_pad=4))
    add("ldr_mod8", lambda M, N, K: dict(residual=True, ldr_pad=4))
    add("remap", lambda M, N, K: dict(rpb=_rpb(M), arem=(_rpb(M) + 77, 77), crem=(_rpb(M) + 5, 4)))
    add("remap_res_silu", lambda M, N, K: dict(rpb=_rpb(M), arem=(_rpb(M) + 17, 17), crem=(_rpb(M) + 3, 3), residual=True, flags=S))
    for sk in (1, 2, 3, 4):
        add(f"splitk{sk}", lambda M, N, K, sk=sk: dict(splitk=sk), (MS_SPLIT, NS, KS + [1536, 2048]))
        add(f"splitk{sk}_res_silu", lambda M, N, K, sk=sk: dict(splitk=sk, residual=True, flags=S), (MS_SPLIT, NS, KS + [1536]))
    add("splitk2_geglu", lambda M, N, K: dict(splitk=2, flags=GEGLU) if N % 128 == 0 else None, (MS_SPLIT, NS, KS))
    add("splitk3_qkv64x3", lambda M, N, K: dict(splitk=3, flags=QKV, seg=64, period=3, rpb=_rpb(M)) if N % 192 == 0 else None, (MS_SPLIT, NS, KS))
    add("splitk2_a2", lambda M, N, K: dict(splitk=2, a2=64) if K >= 128 else None, (MS_SPLIT, NS, KS))

    def parts(M, n):                                   # n problems of unequal sizes that add up to M
        p = [M // n + (1 if i == 0 else 0) for i in range(n)]
        p[-1] = M - sum(p[:-1])
        return p if min(p) > 0 else None
    add("grouped2", lambda M, N, K: dict(M=0, segs=[(m, 0) for m in parts(M, 2)]))
    add("grouped3_res_silu", lambda M, N, K: dict(M=0, segs=[(m, 0) for m in parts(M, 3)], residual=True, flags=S))
    add("grouped4_rowbias", lambda M, N, K: dict(M=0, segs=[(m, m) for m in parts(M, 4)], rowbias=True))
    add("grouped2_rpb15", lambda M, N, K: dict(M=0, segs=[(m, 15) for m in parts(M, 2)], gate=True))
    add("grouped2_qkv64x2", lambda M, N, K: dict(M=0, segs=[(m, m) for m in parts(M, 2)], flags=QKV, seg=64, period=2) if N % 128 == 0 else None)
    add("grouped3_stats_out", lambda M, N, K: dict(M=0, segs=[(m, 0) for m in parts(M, 3)], stats_out=True))
    add("grouped2_ln_stats", lambda M, N, K: dict(M=0, segs=[(m, 0) for m in parts(M, 2)], ln="stats", ln_slabs=2))
    add("grouped2_splitk2", lambda M, N, K: dict(M=0, segs=[(m, 0) for m in parts(M, 2)], splitk=2), (MS_SPLIT, NS, KS))
    return v


# conv grids: (B, H, W) whose B * H * W walks the same M boundaries
CONV_BHW = [(1, 4, 4), (1, 1, 17), (1, 1, 127), (1, 8, 16), (1, 3, 43), (1, 15, 17), (1, 16, 16), (2, 16, 16), (2, 32, 32), (1, 1, 8191),
            (2, 64, 64), (1, 3, 2731), (2, 128, 128)]
CONV_CIN = [64, 128, 576]
CONV_NS = [4, 16, 128, 160, 256, 320, 1280, 1288]


def _conv_variants():
    v = []

    def add(name, fn):
        v.append((name, fn))
    add("conv", lambda B, H, W: {})
    add("conv_res_silu", lambda B, H, W: dict(residual=True, flags=S))
    add("conv_rowbias", lambda B, H, W: dict(rowbias=True, rpb=H * W))
    add("conv_stride2", lambda B, H, W: dict(stride=2))
    add("conv_up", lambda B, H, W: dict(up=1) if B * H * W <= 8192 else None)
    add("conv_up_res", lambda B, H, W: dict(up=1, residual=True) if B * H * W <= 8192 else None)
    add("conv_cin_valid4", lambda B, H, W: dict(cin_valid=4))
    add("conv_cin_valid4_res", lambda B, H, W: dict(cin_valid=4, residual=True))
    add("conv_vhalo", lambda B, H, W: dict(vhalo=1))
    add("conv_corner_patch", lambda B, H, W: dict(corner_patch=8))
    add("conv_gn_part", lambda B, H, W: dict(gn_part=True))
    add("conv_gn_part_rowbias", lambda B, H, W: dict(gn_part=True, rowbias=True, rpb=H * W))
    add("conv_splitk2", lambda B, H, W: dict(splitk=2))
    add("conv_splitk4_res", lambda B, H, W: dict(splitk=4, residual=True))
    add("conv_splitk1", lambda B, H, W: dict(splitk=1))
    add("conv_ldc_mod8", lambda B, H, W: dict(ldc_pad=4))
    add("conv_stats_out", lambda B, H, W: dict(stats_out=True))
    add("conv_ln_final", lambda B, H, W: dict(ln="final"))                    # (rejected by the launch; the queries still answer)
    add("conv_grouped2", lambda B, H, W: dict(conv_segs=[(B, H, W), (B, H + 1, W)]))
    add("conv_grouped3_res", lambda B, H, W: dict(conv_segs=[(B, H, W), (1, H, W + 2), (B, H + 1, W)], residual=True, flags=S))
    return v


def _kept(variant, *point):
    """the pruning of the grid: the plain variant keeps the whole cross; every other one keeps the points with at least two coordinates on a
    pivot, so that each value of M, N and K still meets it (at the pivots of the other two) without the full cross per variant"""
    pivots = ((128, 2048, 8192), (256, 1280), (1024, 2048)) if len(point) == 3 else (((1, 8, 16), (2, 64, 64)), (128,), (160, 1280))
    return variant == "plain" or sum(x in p for x, p in zip(point, pivots)) >= 2


def route_cases():
    """every descriptor of the sweep as a kernel_form_cases case (plus the keys desc_of understands), with a unique "name" """
    out = []
    for name, fn, (ms, ns, ks) in _gemm_variants():
        for M in ms:
            for N in ns:
                for K in ks:
                    kw = fn(M, N, K) if _kept(name, M, N, K) else None
                    if kw is not None:
                        out.append(KC._g(f"{name}/{M}/{N}/{K}", [], **{"M": M, "N": N, "K": K, **kw}))
    for name, fn in _conv_variants():
        for (B, H, W) in CONV_BHW:
            for Cin in CONV_CIN:
                for N in CONV_NS:
                    kw = fn(B, H, W) if _kept(name, (B, H, W), Cin, N) else None
                    if kw is not None:
                        out.append(KC._c(f"{name}/{B}x{H}x{W}/{Cin}/{N}", [], B, H, W, Cin, N, **kw))
    for c in KC.GEMM_CASES + KC.CONV_CASES:            # the form matrix: one descriptor per instantiation, whatever the grid reaches
        out.append(dict(c, name="forms/" + c["name"]))
    return out


def variant_of(name):
    return name.split("/")[0]


def desc_of(c, ptr=None):
    """mx_gemm_desc of a sweep case: kernel_form_cases.gemm_desc plus the operands only this sweep uses"""
    ptr = ptr or KC.fake_ptrs()
    cs = c.get("conv_segs")
    if cs:
        c = dict(c, segs=[(0, c["rpb"])] * len(cs))
    d = KC.gemm_desc(c, ptr)
    grouped = d.n_segs > 0
    if c.get("stats_out"):
        d.stats_out = ptr("stats_out")
    if c.get("ln_final_out"):
        d.ln_final_out, d.ln_final_cnt = ptr("ln_final_out"), ptr("ln_final_cnt")
    if c.get("gn_part"):
        d.gn_part_out = ptr("gn_part")
    if c.get("c_off"):
        d.c += c["c_off"]
    d.corner_patch = c.get("corner_patch", 0)
    for i in range(d.n_segs):
        g = d.segs[i]
        if d.vt:
            g.vt, g.ldvt = ptr("vt"), KC.vt_ld(g.rows_per_batch) + 8
        if d.ln_stats:
            g.ln_stats = ptr("ln_stats")
        if d.stats_out:
            g.stats_out = ptr("stats_out")
        if cs:
            B, H, W = cs[i]
            Ho, Wo = ((H << d.up) + d.stride - 1) // d.stride, ((W << d.up) + d.stride - 1) // d.stride
            g.B, g.Hin, g.Win, g.Hout, g.Wout, g.M = B, H, W, Ho, Wo, B * Ho * Wo
            if d.rowbias:
                g.rows_per_batch = Ho * Wo
    if grouped:
        d.M = 0
    return d


def answers_of(d, conv, names):
    """what the table records for one descriptor: [kernel of each launch as an index into `names` (or -1: none serves it), mx_gemm_launches,
    mx_gemm_form, mx_gemm_splitk, mx_gemm_stats_slabs, mx_gemm_ln_prefers_pass, mx_gemm_gn_partials_supported, mx_gemm_ln_final_supported]"""
    lib = L.load()
    try:
        kernels = [names.index(k) for k in L.gemm_kernels_of(d, conv=conv)]
    except L.MxError:
        kernels = -1
    p = C.byref(d)
    return [kernels, lib.mx_gemm_launches(p), lib.mx_gemm_form(p, int(conv)), lib.mx_gemm_splitk(p, int(conv)),
            lib.mx_gemm_stats_slabs(p), lib.mx_gemm_ln_prefers_pass(p), lib.mx_gemm_gn_partials_supported(p, int(conv)),
            lib.mx_gemm_ln_final_supported(p)]


# ---- rejections: one descriptor per rule of the validation, violating exactly that rule ----
_GEMM = dict(M=200, N=256, K=192)                      # a 128-row launch
_BIG = dict(M=8192, N=1280, K=128)                     # a 256-row launch
_HUGE = dict(M=16384, N=1024, K=192)                   # a 256 x 256 launch
_CONV = (2, 9, 11, 64, 160)
_QKV = dict(M=200, N=384, K=128, flags=QKV, seg=64, period=3, rpb=100)
_G2 = dict(M=0, N=256, K=192, segs=[(120, 60), (80, 40)])


def _set(**kw):
    def f(d):
        for k, val in kw.items():
            setattr(d, k, val)
    return f


def _seg(i, **kw):
    def f(d):
        for k, val in kw.items():
            setattr(d.segs[i], k, val)
    return f


def _off(field, by):
    def f(d):
        setattr(d, field, getattr(d, field) + by)
    return f


def _conv_grid(stride, up, dH=0):
    def f(d):
        d.stride, d.up = stride, up
        d.Hout, d.Wout = ((d.Hin << up) + stride - 1) // stride + dH, ((d.Win << up) + stride - 1) // stride
        d.M = d.B * d.Hout * d.Wout
    return f


def rejection_cases():
    """(name, case, mutation of its descriptor or None): every MX_CHECK of the validation that a single violated rule can reach (not: the
    split-K scratch allocation and the launchers' "form outside its list", which no descriptor reaches without a device)"""
    g, c = KC._g, KC._c
    r = []

    def add(name, case, mut=None):
        r.append((name, dict(case, name=name), mut))
    add("null_operand", g("", [], **_GEMM), _set(w=None))
    add("bad_n_segs", g("", [], **_GEMM), _set(n_segs=5))
    add("empty_problem", g("", [], **_GEMM), _set(M=0))
    add("grouped_empty_problem", g("", [], **_G2), _seg(1, M=0))
    add("grouped_operands_differ", g("", [], **_G2), _seg(1, residual=1 << 20))
    add("grouped_misaligned", g("", [], **_G2), lambda d: setattr(d.segs[1], "a", d.segs[1].a + 8))
    add("grouped_rpb_required", g("", [], **_G2, rowbias=True), _seg(1, rows_per_batch=0))
    add("grouped_bad_input_remap", g("", [], **_G2), _seg(0, a_batch_rows=64, a_row_off=5))
    add("grouped_bad_output_remap", g("", [], **_G2), _seg(0, c_batch_rows=64, c_row_off=5))
    add("grouped_ln_stats_remap", g("", [], **_G2, ln="stats"), _seg(0, a_batch_rows=64, a_row_off=4))
    add("grouped_qkv_whole_batches", g("", [], M=0, N=384, K=128, segs=[(120, 60), (80, 40)], flags=QKV, seg=64, period=3),
        _seg(1, M=81))
    add("grouped_conv_grid", dict(c("", [], *_CONV), conv_segs=[(2, 9, 11), (2, 10, 11)]), _seg(1, Hout=11))
    add("grouped_32bit", g("", [], M=0, N=256, K=2048, segs=[(120, 0), (1 << 20, 0)], lda_pad=0))
    add("k_mod_64", g("", [], M=200, N=256, K=100, lda_pad=4))
    add("n_mod_4", g("", [], M=200, N=254, K=192, ldc_pad=10))
    add("ln_final_needs_colsum", g("", [], **_HUGE, ln="final"), _set(ln_colsum=None))
    add("ln_final_excludes", g("", [], **_HUGE, ln="final", rowbias=True, rpb=4096))
    add("ln_final_misaligned", g("", [], **_HUGE, ln="final"), _off("ln_final", 8))
    add("ln_stats_needs_slabs", g("", [], **_GEMM, ln="stats"), _set(ln_slabs=0))
    add("ln_stats_excludes", g("", [], M=200, N=256, K=320, ln="stats", a2=128))
    add("ln_stats_misaligned", g("", [], **_GEMM, ln="stats"), _off("ln_stats", 8))
    add("a2_k_split", g("", [], M=200, N=256, K=320, a2=128), _set(k_split=100))
    add("a2_lda2", g("", [], M=200, N=256, K=320, a2=128), _set(lda2=184))
    add("a2_misaligned", g("", [], M=200, N=256, K=320, a2=128), _off("a2", 8))
    add("lda", g("", [], **_GEMM), _set(lda=184))
    add("conv_k", c("", [], *_CONV), _set(K=640))
    add("conv_stride", c("", [], *_CONV), _conv_grid(3, 0))
    add("conv_up", c("", [], *_CONV), _conv_grid(1, 2))
    add("conv_up_stride", c("", [], *_CONV), _conv_grid(2, 1))
    add("conv_grid", c("", [], *_CONV), _conv_grid(1, 0, dH=1))
    add("conv_m", c("", [], *_CONV), _off("M", 1))
    add("conv_cin_8192", c("", [], 1, 4, 4, 8256, 160))
    add("conv_geglu", c("", [], 2, 9, 11, 64, 256, flags=GEGLU))
    add("conv_vhalo", c("", [], *_CONV, vhalo=2))
    add("misaligned", g("", [], **_GEMM), _off("bias", 4))
    add("rpb_required", g("", [], **_GEMM, rowbias=True, rpb=0))
    add("ldg", g("", [], **_GEMM, gate=True, rpb=100), _set(ldg=252))
    add("bad_input_remap", g("", [], **_GEMM, rpb=100, arem=(104, 5)))
    add("bad_output_remap", g("", [], **_GEMM, rpb=100, crem=(104, 5)))
    add("ldrb", g("", [], **_GEMM, rowbias=True, rpb=100), _set(ldrb=252))
    add("a_32bit", g("", [], M=1 << 20, N=256, K=2048, lda_pad=0))
    add("w_32bit", g("", [], M=200, N=65536, K=32768))
    add("ldr", g("", [], **_GEMM, residual=True), _set(ldr=252))
    add("stats_out_unsupported", dict(g("", [], **_GEMM, flags=F32), stats_out=True))
    add("stats_out_misaligned", dict(g("", [], **_GEMM), stats_out=True), _off("stats_out", 8))
    add("gn_part_tile", dict(g("", [], **_GEMM), gn_part=True))
    add("gn_part_epilogue", dict(g("", [], **_BIG, residual=True), gn_part=True))
    add("gn_part_m_mod_64", dict(g("", [], M=8193, N=960, K=192), gn_part=True))
    add("ln_final_out_needs", dict(g("", [], **_BIG), stats_out=True, ln_final_out=True), _set(ln_final_cnt=None))
    add("ln_final_out_misaligned", dict(g("", [], **_BIG), stats_out=True, ln_final_out=True), _off("ln_final_out", 8))
    add("geglu_n_mod_128", g("", [], M=200, N=192, K=192, flags=GEGLU))
    add("geglu_excludes", g("", [], **_GEMM, flags=GEGLU, residual=True))
    add("geglu_ldc", g("", [], **_GEMM, flags=GEGLU), _set(ldc=124))
    add("qkv_segments", g("", [], **dict(_QKV, seg=96, period=2)))
    add("qkv_vt", g("", [], **_QKV), _set(vt=None))
    add("qkv_ldvt", g("", [], **_QKV), _set(ldvt=104))
    add("qkv_whole_batches", g("", [], **dict(_QKV, rpb=96)))
    add("qkv_ldc", g("", [], **_QKV), _set(ldc=252))
    add("qkv_f32", g("", [], **dict(_QKV, flags=QKV | F32)))
    add("qkv_excludes", g("", [], **_QKV, residual=True))
    add("rmsnorm_needs", g("", [], **dict(_QKV, flags=QKV | RMS), rms=True), _set(rms_wq=None))
    add("ldc", g("", [], **_GEMM), _set(ldc=252))
    add("ln_final_tile", g("", [], **_GEMM, ln="final"))
    add("ln_final_epilogue", g("", [], **_HUGE, ln="final", flags=S))
    return r


def rejection_of(name, case, mut):
    """(status, message) of mx_gemm / mx_conv3x3 for one rejection case.  Fake pointers: only ever called where no device is visible."""
    lib = L.load()
    d = desc_of(case)
    if mut:
        mut(d)
    fn = lib.mx_conv3x3 if case["kind"] == "conv" else lib.mx_gemm
    rc = fn(None, C.byref(d))
    return rc, (lib.mx_last_error().decode() if rc else "")


def record():
    names = L.gemm_kernel_names()
    rows = {c["name"]: answers_of(desc_of(c), c["kind"] == "conv", names) for c in route_cases()}
    lib = L.load()
    rej = {"null_descriptor": [lib.mx_gemm(None, None), lib.mx_last_error().decode()]}
    for name, case, mut in rejection_cases():
        rej[name] = list(rejection_of(name, case, mut))
    # a few hundred distinct answers: a row names its answer by index, and the rows of a variant (the case name up to the first '/') are one
    # list in the generator's order
    answers = sorted({json.dumps(v) for v in rows.values()})
    by_variant = {}
    for k, v in rows.items():
        by_variant.setdefault(variant_of(k), []).append(answers.index(json.dumps(v)))
    with open(TABLE, "w") as f:
        f.write('{"names": %s,\n"rejections": {\n%s},\n"answers": [\n%s],\n"rows": {\n%s}}\n' % (
            json.dumps(names), ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rej.items()), ",\n".join(answers),
            ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in by_variant.items())))
    return names, rows, rej


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        names, rows, rej = record()
        print(len(rows), "rows,", len(rej), "rejections,", os.path.getsize(TABLE), "bytes")
