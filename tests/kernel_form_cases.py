"""The form matrix: one case per kernel instantiation (and edge) of the GEMM / conv / attention launchers, each naming the instantiation it
targets.  Plain data plus the descriptor builder, shared by the CPU coverage test (fake pointers: tests/test_kernel_forms_cpu.py) and the
GPU runs (tests/test_kernel_forms_gpu.py)."""
from sduss_amd import lib as L


def vt_ld(lk):
    return (lk + 15) // 16 * 16


def _g(name, target, M, N, K, **kw):
    c = dict(name=name, target=target if isinstance(target, list) else [target], kind="gemm", M=M, N=N, K=K, flags=0, bias=True, residual=False,
             rowbias=False, gate=False, rpb=0, out_scale=0.0, splitk=0, lda_pad=8, ldc_pad=8, ldr_pad=8, seg=0, period=0,
             a2=0, arem=None, crem=None, rms=False, ln=None, ln_slabs=1, segs=None, vhalo=0)
    c.update(kw)
    return c


def _c(name, target, B, H, W, Cin, N, **kw):
    stride, up = kw.get("stride", 1), kw.get("up", 0)
    Ho, Wo = ((H << up) + stride - 1) // stride, ((W << up) + stride - 1) // stride
    c = _g(name, target, B * Ho * Wo, N, 9 * Cin, kind="conv", B=B, Hin=H, Win=W, Cin=Cin, Hout=Ho, Wout=Wo, stride=stride, up=up, cin_valid=0, lda_pad=0)
    c.update(kw)
    return c


V2 = "gemm_v2_kernel<{}, 2, {}, {}, {}>"
V5 = "gemm_v5_kernel<{}, 4, {}, {}, {}, {}>"
V4 = "gemm_v4_kernel<{}>"
S, G, GT, Q, RB = L.EPI_SILU, L.EPI_GELU, L.EPI_GELU_TANH, L.EPI_QUICK_GELU, L.EPI_RES_BCAST

GEMM_CASES = [
    # generic register-prefetch tile kernel: fp32 output, broadcast residual, short batches, N % 128 != 0, M below one tile
    _g("gen64_bias_res", "gemm_kernel<64, false>", 200, 192, 192, residual=True),
    _g("gen128_f32_silu", "gemm_kernel<128, false>", 127, 256, 128, flags=S | L.EPI_OUT_F32),
    _g("gen128_f32_res_m17", "gemm_kernel<128, false>", 17, 128, 320, flags=L.EPI_OUT_F32, residual=True),
    _g("gen128_resbcast_rpb15", "gemm_kernel<128, false>", 45, 256, 192, flags=RB, residual=True, rpb=15),
    _g("gen128_rowbias_gate_rpb17", "gemm_kernel<128, false>", 51, 256, 128, rowbias=True, gate=True, rpb=17),
    _g("gen128_gelu", "gemm_kernel<128, false>", 100, 128, 192, flags=G),
    _g("gen128_quick_gelu", "gemm_kernel<128, false>", 100, 128, 192, flags=Q),
    _g("gen128_gelu_tanh_scale", "gemm_kernel<128, false>", 100, 128, 192, flags=GT, out_scale=0.375),
    _g("gen128_geglu", "gemm_kernel<128, false>", 100, 256, 192, flags=L.EPI_GEGLU),
    _g("gen128_geglu_tanh", "gemm_kernel<128, false>", 100, 256, 192, flags=L.EPI_GEGLU | L.EPI_GEGLU_TANH),
    # 128-row lock-step tiles (M in [128, 256): only 128-row tiles fit)
    _g("v2_160_plain_m129", V2.format(160, "false", 0, "false"), 129, 320, 128),
    _g("v2_160_all_res_silu", V2.format(160, "false", "EPI_F_ALL", "false"), 255, 320, 576, flags=S, residual=True),
    _g("v2_160_rowbias_gate_rpb16", V2.format(160, "false", 0, "false"), 160, 160, 192, rowbias=True, gate=True, rpb=16),
    _g("v2_128_plain_m128", V2.format(128, "false", 0, "false"), 128, 256, 128),
    _g("v2_128_all_gelu_tanh_res", V2.format(128, "false", "EPI_F_ALL", "false"), 200, 256, 320, flags=GT, residual=True),
    _g("v2_128_all_quick_gelu", V2.format(128, "false", "EPI_F_ALL", "false"), 200, 128, 192, flags=Q),
    _g("v2_128_all_gelu_scale", V2.format(128, "false", "EPI_F_ALL", "false"), 200, 128, 192, flags=G, out_scale=0.5),
    _g("v2_128_geglu", V2.format(128, "false", 0, "true"), 200, 256, 192, flags=L.EPI_GEGLU),
    _g("v2_128_geglu_tanh", V2.format(128, "false", "EPI_F_ACT", "true"), 200, 256, 192, flags=L.EPI_GEGLU | L.EPI_GEGLU_TANH),
    _g("v2_128_qkv3", V2.format(128, "false", "EPI_F_QKV", "false"), 200, 384, 128, flags=L.EPI_QKV, seg=64, period=3, rpb=100, bias=True),
    _g("v2_160_qkv3", V2.format(160, "false", "EPI_F_QKV", "false"), 160, 960, 128, flags=L.EPI_QKV, seg=320, period=3, rpb=80),
    _g("v2_splitk2", V2.format(128, "false", 0, "false"), 200, 128, 1024, splitk=2),
    _g("v2_splitk3_res", V2.format(128, "false", "EPI_F_ALL", "false"), 200, 128, 1536, splitk=3, residual=True, flags=S),
    _g("v2_splitk4", V2.format(160, "false", 0, "false"), 200, 160, 2048, splitk=4),
    # 256-row ping-pong tiles (enough tiles that one 256-row round beats two 128-row rounds)
    _g("v5_160_plain", V5.format(160, "false", 0, "false", "false"), 8192, 1280, 128),
    _g("v5_160_all_res_m_tile_plus1", V5.format(160, "false", "EPI_F_ALL", "false", "true"), 8193, 960, 192, residual=True, flags=S),
    _g("v5_160_qkv2", V5.format(160, "false", "EPI_F_QKV", "false", "false"), 8192, 1280, 128, flags=L.EPI_QKV, seg=320, period=2, rpb=1024),
    _g("v5_128_plain_m_tile_minus1", V5.format(128, "false", 0, "false", "false"), 8191, 1024, 128),
    _g("v5_128_all_rowbias_gate", V5.format(128, "false", "EPI_F_ALL", "false", "true"), 8192, 1024, 128, rowbias=True, gate=True, rpb=1000),
    _g("v5_128_qkv3", V5.format(128, "false", "EPI_F_QKV", "false", "false"), 8192, 1152, 128, flags=L.EPI_QKV, seg=128, period=3, rpb=2048),
    _g("v5_128_geglu", V5.format(128, "false", 0, "true", "false"), 8192, 1024, 128, flags=L.EPI_GEGLU),
    _g("v5_128_geglu_tanh", V5.format(128, "false", "EPI_F_ACT", "true", "false"), 8192, 1024, 128, flags=L.EPI_GEGLU | L.EPI_GEGLU_TANH),
    # persistent 256 x 256 (and the two launches of its tail split)
    _g("v4_plain", V4.format("false, 0, false"), 16384, 1024, 128),
    _g("v4_tanh", V4.format("false, EPI_F_TANH, false"), 16384, 1024, 128, flags=GT),
    _g("v4_all_res_silu", V4.format("true, EPI_F_ALL, false"), 16384, 1024, 128, flags=S, residual=True),
    _g("v4_vec_rowbias", V4.format("true, 0, false"), 16384, 1024, 128, rowbias=True, rpb=4096),
    _g("v4_qkv2", V4.format("false, EPI_F_QKV, false"), 16384, 1024, 128, flags=L.EPI_QKV, seg=512, period=2, rpb=4096),
    _g("v4_geglu", V4.format("false, 0, true"), 16384, 1024, 128, flags=L.EPI_GEGLU),
    _g("v4_geglu_tanh", V4.format("false, EPI_F_ACT, true"), 16384, 1024, 128, flags=L.EPI_GEGLU | L.EPI_GEGLU_TANH),
    _g("v4_tail_split", [V4.format("false, 0, false"), V2.format(128, "false", 0, "false")], 8192, 2304, 128),
    # M <= 16: the weight stream (wide: K >= 1024 and few 16-feature groups; long: > 32 M weights)
    # QKV: the q-only out_scale, RMSNorm of the q / k heads (+ out_scale), the joint-sequence row remaps (A and C / V^T key index)
    _g("v2_128_qkv3_qscale", V2.format(128, "false", "EPI_F_QKV", "false"), 200, 384, 128, flags=L.EPI_QKV, seg=64, period=3, rpb=100, out_scale=0.18),
    _g("v5_128_qkv3_rms_qscale", V5.format(128, "false", "EPI_F_QKV", "false", "false"), 8192, 1152, 128, flags=L.EPI_QKV | L.EPI_RMSNORM,
       seg=128, period=3, rpb=2048, out_scale=0.18, rms=True),
    _g("v2_128_qkv3_rms", V2.format(128, "false", "EPI_F_QKV", "false"), 192, 384, 128, flags=L.EPI_QKV | L.EPI_RMSNORM, seg=64, period=3, rpb=96, rms=True),
    _g("v4_qkv2_qscale_remap", V4.format("false, EPI_F_QKV, false"), 16384, 1024, 128, flags=L.EPI_QKV, seg=512, period=2, rpb=4096, out_scale=0.5,
       arem=(4173, 77), crem=(4200, 100)),
    _g("v2_160_remap_res", V2.format(160, "false", "EPI_F_ALL", "false"), 200, 320, 192, residual=True, flags=S, rpb=100, arem=(117, 17), crem=(130, 3)),
    _g("v5_128_remap_rowbias", V5.format(128, "false", "EPI_F_ALL", "false", "true"), 8192, 1024, 128, rowbias=True, rpb=4096, arem=(4173, 77), crem=(4100, 4)),
    _g("gen128_remap_rpb15", "gemm_kernel<128, false>", 45, 256, 128, residual=True, rpb=15, arem=(20, 5), crem=(16, 1)),
    # the split A operand (a2: columns [k_split, K) from a second source)
    _g("v2_128_a2", V2.format(128, "false", 0, "false"), 200, 256, 320, a2=128),
    _g("v5_160_a2_res", V5.format(160, "false", 0, "false", "false"), 8192, 960, 320, a2=192, residual=True),
    _g("gen64_a2", "gemm_kernel<64, false>", 100, 192, 256, a2=64),
    # folded LayerNorm: slabs of row statistics (ln_stats, 128 / 256-row tiles) and finalised (mean, rstd) per row (ln_final, 256 x 256)
    _g("v2_128_ln_stats_3slabs", V2.format(128, "false", 0, "false"), 200, 256, 192, ln="stats", ln_slabs=3),
    _g("v5_128_ln_stats_gelu", V5.format(128, "false", "EPI_F_ALL", "false", "true"), 8192, 1024, 192, ln="stats", ln_slabs=2, flags=G),
    _g("v5_128_ln_stats_geglu", V5.format(128, "false", 0, "true", "false"), 8192, 1024, 192, ln="stats", ln_slabs=1, flags=L.EPI_GEGLU),
    _g("gen128_ln_stats", "gemm_kernel<128, false>", 100, 128, 192, ln="stats", ln_slabs=5),
    _g("v4_ln_final", V4.format("false, 0, false, true"), 16384, 1024, 192, ln="final"),
    _g("v4_ln_final_geglu", V4.format("false, 0, true, true"), 16384, 1024, 192, ln="final", flags=L.EPI_GEGLU),
    _g("v4_ln_final_qkv2", V4.format("false, EPI_F_QKV, false, true"), 16384, 1024, 192, ln="final", flags=L.EPI_QKV, seg=512, period=2, rpb=4096),
    # grouped launches (n_segs problems in one launch): M of each problem; the tiles of one problem never straddle the next
    _g("gen128_grouped", "gemm_kernel<128, false>", 0, 256, 128, segs=[(17, 0), (100, 0), (3, 0)], residual=True),
    _g("v2_128_grouped_rowbias", V2.format(128, "false", "EPI_F_ALL", "false"), 0, 256, 192, segs=[(129, 43), (60, 20)], rowbias=True, flags=S),
    _g("v5_160_grouped", V5.format(160, "false", 0, "false", "false"), 0, 960, 128, segs=[(4096, 0), (2049, 0), (2300, 0)]),
    _g("v4_grouped_res", V4.format("true, EPI_F_ALL, false"), 0, 1024, 128, segs=[(8192, 0), (8191, 0)], residual=True, flags=S),
    _g("small_m16_res_silu", "gemm_small_m_kernel<false, 16>", 8, 1280, 1280, residual=True, flags=S),
    _g("small_m16_f32", "gemm_small_m_kernel<true, 16>", 5, 1280, 1024, flags=L.EPI_OUT_F32),
    _g("small_m4", "gemm_small_m_kernel<false, 4>", 16, 1280, 320, residual=True),
    _g("small_m4_f32_silu", "gemm_small_m_kernel<true, 4>", 1, 1536, 256, flags=S | L.EPI_OUT_F32),
    _g("small_m_stream", "gemm_small_m_stream_kernel<false>", 8, 33792, 1024),
    _g("small_m_stream_f32", "gemm_small_m_stream_kernel<true>", 3, 16896, 2048, flags=L.EPI_OUT_F32),
]

CONV_CASES = [
    _c("conv_gen64", "gemm_kernel<64, true>", 1, 9, 7, 64, 64, residual=True),
    _c("conv_gen128_stride2_odd", "gemm_kernel<128, true>", 1, 13, 11, 64, 128, stride=2),
    _c("conv_v2_160", V2.format(160, "true", 0, "false"), 2, 9, 11, 64, 160),
    _c("conv_v2_160_all", V2.format(160, "true", "EPI_F_ALL", "false"), 2, 10, 10, 64, 160, residual=True, flags=S),
    _c("conv_v2_128_up", V2.format(128, "true", 0, "false"), 2, 5, 5, 64, 128, up=1),
    _c("conv_v2_128_all_stride2", V2.format(128, "true", "EPI_F_ALL", "false"), 1, 31, 29, 64, 128, stride=2, residual=True, flags=S),
    _c("conv_v5_160", V5.format(160, "true", 0, "false", "false"), 2, 64, 64, 64, 1280),
    _c("conv_v5_160_vec", V5.format(160, "true", 0, "false", "true"), 2, 64, 64, 64, 1280, rowbias=True, rpb=4096),
    _c("conv_v5_160_all", V5.format(160, "true", "EPI_F_ALL", "false", "true"), 2, 64, 64, 64, 1280, residual=True, flags=S),
    _c("conv_v5_128", V5.format(128, "true", 0, "false", "false"), 2, 64, 64, 64, 1024),
    _c("conv_v5_128_vec", V5.format(128, "true", 0, "false", "true"), 2, 64, 64, 64, 1024, rowbias=True, rpb=4096),
    _c("conv_v5_128_all", V5.format(128, "true", "EPI_F_ALL", "false", "true"), 2, 63, 65, 64, 1024, residual=True, flags=S),
    _c("conv_v2_128_cin2560", V2.format(128, "true", 0, "false"), 1, 13, 12, 2560, 128),
    _c("conv_v2_160_vhalo", V2.format(160, "true", "EPI_F_ALL", "false"), 2, 9, 11, 64, 160, vhalo=1, residual=True, flags=S),
    _c("conv_v5_128_vhalo", V5.format(128, "true", 0, "false", "false"), 2, 64, 64, 64, 1024, vhalo=1),
    _c("conv_gen64_vhalo", "gemm_kernel<64, true>", 1, 7, 9, 64, 64, vhalo=1),
    _c("conv_small_n", "conv3x3_small_n_kernel", 2, 17, 19, 64, 16),
    _c("conv_small_cin", "conv3x3_small_cin_kernel", 1, 13, 21, 64, 320, cin_valid=4),
]

# instantiations the matrix does not reach (none): listed so that the coverage test stays exact -- a new instantiation without a case fails it
NOT_COVERED = set()


def attn(name, target, B, H, Lq, Lk, pre=True, causal=False, bias=False, cross=False, ldo_pad=0, ldq_pad=0, chunks=0):
    return dict(name=name, target=target, B=B, H=H, Lq=Lq, Lk=Lk, pre=pre, causal=causal, bias=bias, cross=cross, ldo_pad=ldo_pad, ldq_pad=ldq_pad,
                chunks=chunks)


ATTN_CASES = [
    attn("cross77_pre", "attn_cross_kernel<true, 77>", 2, 2, 33, 77),
    attn("cross_pre_lq2048", "attn_cross_kernel<true>", 1, 2, 2048, 63),
    attn("cross_forced_lk95", "attn_cross_kernel<true>", 2, 3, 31, 95, cross=True),
    attn("cross_forced_lk1", "attn_cross_kernel<true>", 1, 8, 129, 1, cross=True),
    attn("cross_nonpre_lq2049", "attn_cross_kernel<false>", 1, 1, 2049, 33, pre=False),
    attn("w64_lk129", "attn_fwd64_kernel", 1, 1, 2048, 129),
    attn("w64_lk193_bh8", "attn_fwd64_kernel", 2, 4, 2049, 193),
    attn("ldo_odd_moves_off_w64", "attn_fwd_kernel<true>", 1, 1, 2048, 129, ldo_pad=4),
    attn("dma_pre_lk192", "attn_fwd_dma_kernel<true>", 2, 3, 129, 192),
    attn("dma_nonpre_lk4416", "attn_fwd_dma_kernel<false>", 1, 2, 31, 4416, pre=False),
    attn("gen_pre_lk97", "attn_fwd_kernel<true>", 2, 3, 129, 97),
    attn("gen_pre_lk4429", "attn_fwd_kernel<true>", 1, 2, 33, 4429),
    attn("gen_nonpre_lk65", "attn_fwd_kernel<false>", 3, 1, 33, 65, pre=False),
    attn("gen_nonpre_lk127", "attn_fwd_kernel<false>", 1, 2, 1, 127, pre=False),
    attn("causal_1", "attn_fwd_kernel<true, true>", 1, 2, 1, 1, causal=True),
    attn("causal_63", "attn_fwd_kernel<true, true>", 2, 2, 63, 63, causal=True),
    attn("causal_64", "attn_fwd_kernel<true, true>", 1, 2, 64, 64, causal=True),
    attn("causal_65", "attn_fwd_kernel<true, true>", 1, 3, 65, 65, causal=True),
    attn("causal_77", "attn_fwd_kernel<true, true>", 2, 12, 77, 77, causal=True),
    attn("causal_129", "attn_fwd_kernel<true, true>", 1, 2, 129, 129, causal=True),
    attn("causal_1024", "attn_fwd_kernel<true, true>", 1, 1, 1024, 1024, causal=True),
    attn("ldo_odd_moves_off_cross", "attn_fwd_kernel<true>", 1, 2, 2048, 63, ldo_pad=4),
    attn("gen_pre_lk31_lq2047", "attn_fwd_kernel<true>", 1, 2, 2047, 31),
    attn("dma_pre_lk191x_lq2047", "attn_fwd_kernel<true>", 1, 1, 2047, 191),
    attn("cross_pre_lk96_lq2049_bh_odd", "attn_cross_kernel<true>", 1, 3, 2049, 96),
    attn("w64_lk4429", "attn_fwd64_kernel", 1, 1, 2048, 4429),
    attn("chunked_2", "attn_fwd_dma_kernel<true>", 2, 2, 129, 256, chunks=2),
    attn("chunked_4", "attn_fwd_dma_kernel<true>", 1, 3, 65, 256, chunks=4),
    attn("chunked_8", "attn_fwd_dma_kernel<true>", 1, 2, 33, 512, chunks=8),
    attn("bias_lk77", "attn_fwd_kernel<true, true>", 1, 2, 77, 77, bias=True),
    # key chunks off the LDS-DMA kernel: two whole tiles are fewer than its three (the register-staged kernel's chunk branch), and the 64-row kernel's ring
    attn("chunked_gen_lk128", "attn_fwd_kernel<true>", 2, 2, 65, 128, chunks=2),
    attn("w64_chunked_2", "attn_fwd64_kernel", 1, 2, 2048, 256, chunks=2),
]
ATTN_NOT_COVERED = {"attn_fwd_kernel<false, true>"}      # (no entry point runs a non-prescaled masked / biased launch)


def nout_of(c):
    if c["flags"] & L.EPI_GEGLU:
        return c["N"] // 2
    if c["flags"] & L.EPI_QKV:
        return c["N"] // c["period"] * (c["period"] - 1)
    return c["N"]


def ldvt_of(c):
    return vt_ld(c["crem"][0] if c["crem"] else c["rpb"]) + 8


def gemm_desc(c, ptr):
    """mx_gemm_desc of case c; ptr(name) gives each operand's address (fake on the CPU).  Grouped cases: ptr(name + str(i)) per problem i."""
    d = L.GemmDesc()
    M, N, K = c["M"], c["N"], c["K"]
    qkv = bool(c["flags"] & L.EPI_QKV)
    grouped = c["segs"] is not None
    sfx = "0" if grouped else ""
    d.a, d.w, d.c = ptr("a" + sfx), ptr("w"), ptr("c" + sfx)
    d.bias = ptr("bias") if c["bias"] else None
    d.residual = ptr("residual" + sfx) if c["residual"] else None
    d.rowbias = ptr("rowbias" + sfx) if c["rowbias"] else None
    d.gate = ptr("gate" + sfx) if c["gate"] else None
    d.M, d.N, d.K, d.flags = M, N, K, c["flags"]
    d.lda = (c["a2"] or K) + c["lda_pad"] if c["kind"] == "gemm" else 0
    if c["a2"]:
        d.a2, d.k_split, d.lda2 = ptr("a2"), c["a2"], K - c["a2"] + c["lda_pad"]
    d.ldc = nout_of(c) + c["ldc_pad"]
    d.ldr = N + c["ldr_pad"] if c["residual"] else 0
    d.ldrb = N + 4 if c["rowbias"] else 0
    d.ldg = N + 4 if c["gate"] else 0
    d.rows_per_batch, d.out_scale, d.splitk = c["rpb"], c["out_scale"], c["splitk"]
    if c["arem"]:
        d.a_batch_rows, d.a_row_off = c["arem"]
    if c["crem"]:
        d.c_batch_rows, d.c_row_off = c["crem"]
    if qkv:
        d.seg, d.period, d.vt, d.ldvt = c["seg"], c["period"], ptr("vt" + sfx), ldvt_of(c)
    if c["rms"]:
        d.rms_wq, d.rms_wk, d.rms_eps = ptr("rms_wq"), ptr("rms_wk"), 1e-6
    if c["ln"] == "stats":
        d.ln_stats, d.ln_colsum, d.ln_slabs, d.ln_eps = ptr("ln_stats" + sfx), ptr("ln_colsum"), c["ln_slabs"], 1e-5
    elif c["ln"] == "final":
        d.ln_final, d.ln_colsum, d.ln_eps = ptr("ln_final"), ptr("ln_colsum"), 1e-5
    if c["kind"] == "conv":
        d.B, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride, d.up = c["B"], c["Hin"], c["Win"], c["Cin"], c["Hout"], c["Wout"], c["stride"], c["up"]
        d.cin_valid, d.vhalo = c["cin_valid"], c["vhalo"]
    if grouped:
        segs = (L.GemmSeg * len(c["segs"]))()
        for i, (m, rpb) in enumerate(c["segs"]):
            g, si = segs[i], str(i)
            g.a, g.c, g.M, g.rows_per_batch = ptr("a" + si), ptr("c" + si), m, rpb
            g.residual = ptr("residual" + si) if c["residual"] else None
            g.rowbias = ptr("rowbias" + si) if c["rowbias"] else None
            g.gate = ptr("gate" + si) if c["gate"] else None
        d.segs, d.n_segs = segs, len(segs)
    return d


def fake_ptrs():
    addr = [1 << 32]

    def ptr(_name):
        addr[0] += 1 << 24
        return addr[0]
    return ptr


def attn_target_of(c):
    ldo = c["H"] * 64 + c["ldo_pad"]
    return L.attention_kernel_of(c["B"], c["H"], c["Lq"], c["Lk"], ldo, prescaled=c["pre"], causal=c["causal"], bias=c["bias"],
                                key_chunk=c["Lk"] // c["chunks"] if c["chunks"] else 0, force_cross=c["cross"])


def gemm_targets_of(c):
    return L.gemm_kernels_of(gemm_desc(c, fake_ptrs()), conv=c["kind"] == "conv")
