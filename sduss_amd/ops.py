"""Thin torch-tensor wrappers over the per-kernel entry points of the C ABI (mx_gemm, mx_conv3x3, mx_conv3x3_rgb8, mx_conv3x3_rgb_in, mx_attention,
mx_layernorm, mx_groupnorm_nhwc, scheduler steps, the multistep samplers, the inpainting entries, the image resize, the mask blur / bounding box / overlay, the LoRA merge).  They allocate outputs with torch and pass raw pointers + the current
stream; nothing is computed in Python.  Used by the parity tests and by ``pipeline.py``."""
from __future__ import annotations

import collections
import ctypes as C
from typing import Optional

import torch

from . import lib as _lib


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _bf16(t):
    assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous(), "expected a contiguous CUDA bf16 tensor"
    return t


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         rowbias: Optional[torch.Tensor] = None, rows_per_batch: int = 0, silu: bool = False, geglu: bool = False,
         out_f32: bool = False, out_scale: float = 0.0, ln_stats: Optional[torch.Tensor] = None, ln_colsum: Optional[torch.Tensor] = None,
         ln_eps: float = 1e-5, want_stats: bool = False, splitk: int = 0, ln_final: Optional[torch.Tensor] = None, want_final: bool = False,
         final_buffers=None):
    """C[M,N] = (A[M,K] W[N,K]^T + bias) * out_scale (+rowbias +residual, silu | geglu).  With ``geglu`` the weight/bias rows must be
    interleaved as weights._geglu_interleave does; the output is [M, N/2].
    ``ln_stats`` = (stats [M, pitch, 2], slabs) + ``ln_colsum`` [N]: LayerNorm folded into this GEMM (w, bias folded by
    weights.fold_layernorm).  ``want_stats``: also return the row statistics of C as such a pair (from the epilogue when the kernel can,
    else mx_row_stats); entries past ``slabs`` of a row are not initialised.
    ``want_final`` (with ``want_stats``): also return the FINALISED statistics [M, 2] = (mean, rstd with ``ln_eps``) the launch's last workgroup per
    256-row panel leaves (mx_gemm_desc.ln_final_out), or None where the launch cannot (mx_gemm_ln_final_supported); ``ln_final`` + ``ln_colsum``:
    the consumer side (the 256 x 256 kernel's form of the folded LayerNorm).  ``final_buffers`` = (final [M, 2] fp32, tickets [ceil(M / 256)] int32,
    zero): reuse these instead of allocating (and skip the host-side check of the tickets, which synchronises)."""
    l = _lib.load()
    _bf16(a); _bf16(w)
    m, k = a.shape
    n = w.shape[0]
    d = _lib.GemmDesc()
    flags = (_lib.EPI_SILU if silu else 0) | (_lib.EPI_GEGLU if geglu else 0) | (_lib.EPI_OUT_F32 if out_f32 else 0)
    nout = n // 2 if geglu else n
    c = torch.empty((m, nout), dtype=torch.float32 if out_f32 else torch.bfloat16, device=a.device)
    d.a, d.w, d.c = a.data_ptr(), w.data_ptr(), c.data_ptr()
    d.bias, d.rowbias, d.residual = _p(bias), _p(rowbias), _p(residual)
    d.M, d.N, d.K, d.lda, d.ldc = m, n, k, k, nout
    d.ldr = residual.shape[1] if residual is not None else 0
    d.ldrb = rowbias.shape[1] if rowbias is not None else 0
    d.rows_per_batch, d.flags, d.out_scale = rows_per_batch, flags, out_scale
    d.splitk = splitk                           # 0 auto, 1 never, 2..4 forced (mx_gemm_desc.splitk)
    if ln_stats is not None:
        st_, slabs_ = ln_stats
        assert st_.dtype == torch.float32 and ln_colsum.dtype == torch.float32 and st_.shape == (m, stats_pitch(slabs_), 2)
        d.ln_stats, d.ln_colsum, d.ln_slabs, d.ln_eps = st_.data_ptr(), ln_colsum.data_ptr(), slabs_, ln_eps
    if ln_final is not None:
        assert ln_final.dtype == torch.float32 and ln_final.shape == (m, 2) and ln_colsum.dtype == torch.float32
        d.ln_final, d.ln_colsum, d.ln_eps = ln_final.data_ptr(), ln_colsum.data_ptr(), ln_eps
    stats = None
    final = None
    if want_stats:
        slabs = l.mx_gemm_stats_slabs(C.byref(d))
        stats = torch.full((m, stats_pitch(max(slabs, 1)), 2), float("nan"), dtype=torch.float32, device=a.device)
        if slabs > 0:
            d.stats_out = stats.data_ptr()
            if want_final and l.mx_gemm_ln_final_supported(C.byref(d)):
                if final_buffers is not None:
                    final, cnt = final_buffers
                else:
                    final = torch.full((m, 2), float("nan"), dtype=torch.float32, device=a.device)
                    cnt = torch.zeros((m + 255) // 256, dtype=torch.int32, device=a.device)
                d.ln_final_out, d.ln_final_cnt, d.ln_eps = final.data_ptr(), cnt.data_ptr(), ln_eps
    _lib.check(l.mx_gemm(_lib.current_stream(), C.byref(d)), "mx_gemm")
    if want_stats:
        if not d.stats_out:
            _lib.check(l.mx_row_stats(_lib.current_stream(), c.data_ptr(), nout, stats.data_ptr(), m, nout), "mx_row_stats")
        if want_final:
            if final is not None and final_buffers is None:
                assert int(cnt.abs().sum()) == 0, "ln_final_cnt must be zero again after the launch"
            return c, (stats, max(slabs, 1)), final
        return c, (stats, max(slabs, 1))
    return c


def stats_pitch(slabs: int) -> int:
    """MX_STATS_PITCH: slabs per row of a statistics buffer."""
    return (slabs + 3) & ~3


def row_stats(x: torch.Tensor) -> torch.Tensor:
    """(sum, sum of squares) of every row of a bf16 [M, C] matrix -> (fp32 [M, 4, 2] with slab 0 filled, 1): the one-slab ``ln_stats``."""
    l = _lib.load()
    _bf16(x)
    m, c = x.shape
    st = torch.full((m, 4, 2), float("nan"), dtype=torch.float32, device=x.device)
    _lib.check(l.mx_row_stats(_lib.current_stream(), x.data_ptr(), c, st.data_ptr(), m, c), "mx_row_stats")
    return st, 1


def vt_ld(lk: int) -> int:
    """MX_VT_LD: row length of a V^T image for lk keys."""
    return (lk + 15) // 16 * 16


def vt_pos(lk: int) -> torch.Tensor:
    """MX_VT_POS for keys 0..lk-1 (bits 2 and 3 of the key index swapped; its own inverse)."""
    k = torch.arange(lk)
    return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1)


def pack_vt(v: torch.Tensor, pad: float = 0.0) -> torch.Tensor:
    """v [B, Lk, C] -> V^T image [B, C, MX_VT_LD(Lk)] in the attention kernel's key order (include/mxdenoise.h)."""
    b, lk, c = v.shape
    vt = torch.full((b, c, vt_ld(lk)), pad, dtype=v.dtype, device=v.device)
    vt[:, :, vt_pos(lk).to(v.device)] = v.permute(0, 2, 1)
    return vt


def unpack_vt(vt: torch.Tensor, lk: int) -> torch.Tensor:
    """inverse of pack_vt: [B, C, ld] -> [B, Lk, C]."""
    return vt[:, :, vt_pos(lk).to(vt.device)].permute(0, 2, 1)


def gemm_qkv(a: torch.Tensor, w: torch.Tensor, seg: int, period: int, rows_per_batch: int, q_scale: float = 0.0,
             ln_stats: Optional[torch.Tensor] = None, ln_colsum: Optional[torch.Tensor] = None, ln_eps: float = 1e-5,
             bias: Optional[torch.Tensor] = None, ln_final: Optional[torch.Tensor] = None):
    """Fused projection with the V segments written transposed.  Returns (c [M, N/period*(period-1)],
    vt [M/rows_per_batch, N/period, ldvt] in MX_VT_POS key order; see unpack_vt)."""
    l = _lib.load()
    _bf16(a); _bf16(w)
    m, k = a.shape
    n = w.shape[0]
    nb = m // rows_per_batch
    ldvt = vt_ld(rows_per_batch)
    c = torch.empty((m, n // period * (period - 1)), dtype=torch.bfloat16, device=a.device)
    vt = torch.zeros((nb, n // period, ldvt), dtype=torch.bfloat16, device=a.device)
    d = _lib.GemmDesc()
    d.a, d.w, d.c, d.vt = a.data_ptr(), w.data_ptr(), c.data_ptr(), vt.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldc = m, n, k, k, c.shape[1]
    d.rows_per_batch, d.flags, d.seg, d.period, d.ldvt = rows_per_batch, _lib.EPI_QKV, seg, period, ldvt
    d.out_scale = q_scale                       # scales the q segment only (mx_attention_prescaled)
    d.bias = _p(bias)
    if ln_stats is not None:
        d.ln_stats, d.ln_colsum, d.ln_slabs, d.ln_eps = ln_stats[0].data_ptr(), ln_colsum.data_ptr(), ln_stats[1], ln_eps
    if ln_final is not None:
        d.ln_final, d.ln_colsum, d.ln_eps = ln_final.data_ptr(), ln_colsum.data_ptr(), ln_eps
    _lib.check(l.mx_gemm(_lib.current_stream(), C.byref(d)), "mx_gemm(qkv)")
    return c, vt


def conv3x3(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1, up: int = 0,
            corner_patch: int = 0, rowbias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, splitk: int = 0, want_gn_partials: bool = False,
            cin_valid: int = 0):
    """x NHWC bf16 [B,H,W,Cin]; w bf16 [Cout, 9*Cin] tap-major; returns NHWC bf16 [B,Ho,Wo,Cout].  ``cin_valid`` > 0: the caller's promise that only the first
    cin_valid (<= 8) channels of x are non-zero (mx_gemm_desc.cin_valid: conv_in's zero-padded latent).  ``want_gn_partials``: also return the per-64-row,
    per-channel (sum, sum of squares) of its ACCUMULATORS (the output minus bias and row bias) [M / 64, Cout, 2] (mx_gemm_desc.gn_part_out), or None where it cannot."""
    l = _lib.load()
    _bf16(x); _bf16(w)
    b, h, wd, cin = x.shape
    cout = w.shape[0]
    hv, wv = h << up, wd << up
    ho, wo = (hv + stride - 1) // stride, (wv + stride - 1) // stride
    c = torch.empty((b, ho, wo, cout), dtype=torch.bfloat16, device=x.device)
    d = _lib.GemmDesc()
    d.a, d.w, d.c, d.bias, d.rowbias, d.residual = x.data_ptr(), w.data_ptr(), c.data_ptr(), _p(bias), _p(rowbias), _p(residual)
    d.M, d.N, d.K, d.ldc, d.ldr = b * ho * wo, cout, 9 * cin, cout, cout
    d.ldrb = rowbias.shape[1] if rowbias is not None else 0
    d.rows_per_batch = ho * wo
    d.B, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride, d.up, d.corner_patch = b, h, wd, cin, ho, wo, stride, up, corner_patch
    d.splitk = splitk
    d.cin_valid = cin_valid
    part = None
    if want_gn_partials and l.mx_gemm_gn_partials_supported(C.byref(d), 1):
        part = torch.full((b * ho * wo // 64, cout, 2), float("nan"), dtype=torch.float32, device=x.device)
        d.gn_part_out = part.data_ptr()
    _lib.check(l.mx_conv3x3(_lib.current_stream(), C.byref(d)), "mx_conv3x3")
    if want_gn_partials:
        return c, part
    return c


def conv3x3_rgb8(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x NHWC bf16 [B,H,W,Cin] (Cin % 64 == 0); w bf16 [4, 9*Cin] tap-major (row 3 padding); bias fp32 [4] -> uint8 [B,H,W,3] =
    rint(255 clamp((conv + bias) / 2 + 0.5, 0, 1)), rounded once from the fp32 accumulator (mx_conv3x3_rgb8).  ``out``: write into this
    contiguous uint8 [B,H,W,3] tensor (a view into a guarded buffer, say) instead of allocating."""
    l = _lib.load()
    _bf16(x); _bf16(w)
    b, h, wd, cin = x.shape
    assert w.shape == (4, 9 * cin) and bias.dtype == torch.float32 and bias.numel() == 4 and bias.is_contiguous()
    if out is None:
        out = torch.empty((b, h, wd, 3), dtype=torch.uint8, device=x.device)
    assert out.dtype == torch.uint8 and out.shape == (b, h, wd, 3) and out.is_contiguous() and out.device == x.device
    _lib.check(l.mx_conv3x3_rgb8(_lib.current_stream(), x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), b, h, wd, cin), "mx_conv3x3_rgb8")
    return out


def conv3x3_rgb_in(image: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, rotate: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """image uint8 [B,H,W,3] (a client's bytes; value 2 (u / 255) - 1) or fp32 [B,3,H,W] in [-1, 1]; w bf16 [N, 32], column (ky 3 + kx) 3 + c, columns
    27..31 read as zero; bias fp32 [N] -> NHWC bf16 [B,H,W,N], the pad-1 3x3 conv (mx_conv3x3_rgb_in).  ``rotate``: of the image rotated by 180
    degrees.  ``out``: write into this contiguous bf16 [B,H,W,N] tensor instead of allocating."""
    l = _lib.load()
    _bf16(w)
    assert image.is_cuda and image.is_contiguous()
    if image.dtype == torch.uint8:
        fmt = _lib.IMAGE_RGB8_HWC
        b, h, wd, c = image.shape
    else:
        assert image.dtype == torch.float32, "expected a uint8 [B,H,W,3] or an fp32 [B,3,H,W] image"
        fmt = _lib.IMAGE_F32_CHW
        b, c, h, wd = image.shape
    n = w.shape[0]
    assert c == 3 and w.shape == (n, 32) and bias.dtype == torch.float32 and bias.numel() == n and bias.is_contiguous()
    if out is None:
        out = torch.empty((b, h, wd, n), dtype=torch.bfloat16, device=image.device)
    assert out.dtype == torch.bfloat16 and out.shape == (b, h, wd, n) and out.is_contiguous() and out.device == image.device
    _lib.check(l.mx_conv3x3_rgb_in(_lib.current_stream(), image.data_ptr(), fmt, w.data_ptr(), bias.data_ptr(), out.data_ptr(), b, h, wd, n, int(rotate)),
               "mx_conv3x3_rgb_in")
    return out


def vae_latent_finish(moments: torch.Tensor, lc: int, h: int, w: int, scaling: float, shift: float, dtype: torch.dtype,
                      posterior_noise: Optional[torch.Tensor] = None, start_noise: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                      sigma: Optional[torch.Tensor] = None, rotate: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """moments bf16 [B h w, ld] (columns [0, lc) mean, [lc, 2 lc) logvar) -> latents [B, lc, h, w] of ``dtype``: the posterior's mode, or its sample with
    ``posterior_noise``; (z - shift) * scaling; with ``start_noise``: keep[b] * latents + sigma[b] * start_noise (mx_vae_latent_finish)."""
    l = _lib.load()
    assert moments.is_cuda and moments.dtype == torch.bfloat16 and moments.ndim == 2 and moments.stride(1) == 1
    ld = moments.stride(0)
    b = moments.shape[0] // (h * w)
    assert moments.shape[0] == b * h * w and moments.shape[1] >= 2 * lc
    if out is None:
        out = torch.empty((b, lc, h, w), dtype=dtype, device=moments.device)
    assert out.dtype == dtype and out.shape == (b, lc, h, w) and out.is_contiguous()
    for t in (posterior_noise, start_noise):
        assert t is None or (t.is_cuda and t.dtype == dtype and t.shape == out.shape and t.is_contiguous())
    for t in (keep, sigma):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.numel() == b and t.is_contiguous())
    _lib.check(l.mx_vae_latent_finish(_lib.current_stream(), moments.data_ptr(), ld, out.data_ptr(), _lib.torch_dtype_code(dtype), b, lc, h, w, scaling, shift,
                                      _p(posterior_noise), _p(start_noise), _p(keep), _p(sigma), int(rotate)), "mx_vae_latent_finish")
    return out


ATTN_QSCALE = 0.125 * 1.4426950408889634     # MX_ATTN_QSCALE(1/sqrt(64))


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, lq: int, lk: int, prescaled: bool = False) -> torch.Tensor:
    """q [B*Lq, H*64], k [B*Lk, H*64], vt [B, H*64, ldvt] (all bf16) -> o [B*Lq, H*64].  ``prescaled``: q already carries
    the factor ATTN_QSCALE (mx_attention_prescaled)."""
    l = _lib.load()
    _bf16(q); _bf16(k); _bf16(vt)
    b = vt.shape[0]
    o = torch.empty_like(q)
    if prescaled:
        _lib.check(l.mx_attention_prescaled(_lib.current_stream(), q.data_ptr(), q.shape[1], k.data_ptr(), k.shape[1], vt.data_ptr(),
                                            vt.shape[2], vt.shape[1] * vt.shape[2], o.data_ptr(), o.shape[1], b, heads, lq, lk),
                   "mx_attention_prescaled")
        return o
    _lib.check(l.mx_attention(_lib.current_stream(), q.data_ptr(), q.shape[1], k.data_ptr(), k.shape[1], vt.data_ptr(),
                              vt.shape[2], vt.shape[1] * vt.shape[2], o.data_ptr(), o.shape[1], b, heads, lq, lk,
                              0.125), "mx_attention")
    return o


def attn_tail(ao: torch.Tensor, y: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, wq: torch.Tensor, bq: torch.Tensor, colsum_q: torch.Tensor,
              k: torch.Tensor, vt: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, heads: int, L: int, ctx_len: int, ln_eps: float = 1e-5,
              finalise: bool = True):
    """The attention tail of a BasicTransformerBlock on the hidden state ``y`` [M, C] (a copy is updated and returned), as the step plan issues it:
    y1 = ao w1^T + b1 + y;  q2 = norm2(y1) wq^T + bq (wq / bq / colsum_q LayerNorm-folded, prescaled);  ao2 = cross-attention(q2, k, vt);
    y2 = ao2 w2^T + b2 + y1 -- four launches, with slab statistics of y1 feeding the folded norm2 and slab (``finalise``: and finalised) statistics of y2.
    k [B * ctx_len, ldk >= C], vt [B, C, MX_VT_LD(ctx_len)].  Returns (y2, (slab statistics, slabs) of y2, finalised statistics [M, 2] or None, q2, ao2)."""
    l = _lib.load()
    for t_ in (ao, y, w1, wq, w2, k, vt):
        _bf16(t_)
    m, c = y.shape
    b = m // L
    dev = y.device
    y = y.clone()
    q2 = torch.empty_like(y)
    ao2 = torch.empty_like(y)

    def lin(a_, w_, bias, c_, res):
        d = _lib.GemmDesc()
        d.a, d.w, d.c, d.bias = a_.data_ptr(), w_.data_ptr(), c_.data_ptr(), bias.data_ptr()
        d.M, d.N, d.K, d.lda, d.ldc = m, c, c, c, c
        if res is not None:
            d.residual, d.ldr = res.data_ptr(), c
        return d
    out1 = lin(ao, w1, b1, y, y)
    to_q = lin(y, wq, bq, q2, None)
    out2 = lin(ao2, w2, b2, y, y)
    out1.stats_out = 16                          # (shape query below: which operands exist)
    slabs = l.mx_gemm_stats_slabs(C.byref(out1))
    assert slabs > 0, "out1 cannot write slab statistics at this shape"
    st1 = torch.full((m, stats_pitch(slabs), 2), float("nan"), dtype=torch.float32, device=dev)
    st2 = torch.full((m, stats_pitch(slabs), 2), float("nan"), dtype=torch.float32, device=dev)
    out1.stats_out = st1.data_ptr()
    to_q.ln_stats, to_q.ln_colsum, to_q.ln_slabs, to_q.ln_eps = st1.data_ptr(), colsum_q.data_ptr(), slabs, ln_eps
    to_q.out_scale = ATTN_QSCALE
    out2.stats_out = st2.data_ptr()
    final = cnt = None
    if finalise:
        final = torch.full((m, 2), float("nan"), dtype=torch.float32, device=dev)
        cnt = torch.zeros((m + 255) // 256, dtype=torch.int32, device=dev)
        out2.ln_final_out, out2.ln_final_cnt, out2.ln_eps = final.data_ptr(), cnt.data_ptr(), ln_eps
    stream = _lib.current_stream()
    _lib.check(l.mx_gemm(stream, C.byref(out1)), "mx_gemm")
    _lib.check(l.mx_gemm(stream, C.byref(to_q)), "mx_gemm")
    _lib.check(l.mx_attention_cross_prescaled(stream, q2.data_ptr(), c, k.data_ptr(), k.shape[1], vt.data_ptr(), vt.shape[2], vt.shape[1] * vt.shape[2],
                                              ao2.data_ptr(), c, b, heads, L, ctx_len), "mx_attention_cross_prescaled")
    _lib.check(l.mx_gemm(stream, C.byref(out2)), "mx_gemm")
    return y, (st2, slabs), final, q2, ao2


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    l = _lib.load()
    _bf16(x)
    y = torch.empty_like(x)
    _lib.check(l.mx_layernorm(_lib.current_stream(), x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                              x.shape[0], x.shape[1], eps), "mx_layernorm")
    return y


def groupnorm_nhwc_from_partials(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool, part: torch.Tensor,
                                 chunk: int = 64, add_bias: Optional[torch.Tensor] = None, add_rowbias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm (+SiLU) of x NHWC from the partial sums the producing launch left (conv3x3(..., want_gn_partials=True): sums of its accumulators, i.e. of
    x minus ``add_bias`` [C] + ``add_rowbias`` [B, ld] -- pass the conv's bias and row bias): no statistics pass."""
    l = _lib.load()
    _bf16(x)
    b, h, w, c = x.shape
    y = torch.empty_like(x)
    ws = torch.empty(l.mx_groupnorm_nhwc_workspace_bytes(b, h, w, c), dtype=torch.uint8, device=x.device)
    _lib.check(l.mx_groupnorm_nhwc_from_partials(_lib.current_stream(), x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), b, h, w, c, groups, eps,
                                                 1 if silu else 0, part.data_ptr(), chunk, _p(add_bias), _p(add_rowbias),
                                                 add_rowbias.shape[1] if add_rowbias is not None else 0, ws.data_ptr()), "mx_groupnorm_nhwc_from_partials")
    return y


def groupnorm_nhwc(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool,
                   patch: int = 0) -> torch.Tensor:
    l = _lib.load()
    _bf16(x)
    b, h, w, c = x.shape
    y = torch.empty_like(x)
    ws = torch.empty(l.mx_groupnorm_nhwc_workspace_bytes(b, h, w, c), dtype=torch.uint8, device=x.device)
    _lib.check(l.mx_groupnorm_nhwc(_lib.current_stream(), x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                   b, h, w, c, groups, eps, int(silu), patch, ws.data_ptr()), "mx_groupnorm_nhwc")
    return y


def euler_scale_input(latents: torch.Tensor, sigma: torch.Tensor, n_rows: int) -> torch.Tensor:
    """[n_lat, ...] -> [n_rows, ...] = latents[r % n_lat] / sqrt(sigma^2+1)  (CFG duplication fused)."""
    l = _lib.load()
    latents = latents.contiguous()
    n_lat = latents.shape[0]
    elems = latents[0].numel()
    out = torch.empty((n_rows, *latents.shape[1:]), dtype=latents.dtype, device=latents.device)
    sg = sigma.to(device=latents.device, dtype=torch.float32).contiguous()
    _lib.check(l.mx_euler_scale_input(_lib.current_stream(), latents.data_ptr(), out.data_ptr(), sg.data_ptr(), n_lat, n_rows,
                                      elems, _lib.torch_dtype_code(latents.dtype)), "mx_euler_scale_input")
    return out


def _cfg_step_plain_(fn_name: str, noise: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                     guidance_scale: float) -> torch.Tensor:
    l = _lib.load()
    assert latents.is_contiguous() and noise.is_contiguous() and noise.dtype == latents.dtype
    sg = sigma.to(device=latents.device, dtype=torch.float32).contiguous()
    sn = sigma_next.to(device=latents.device, dtype=torch.float32).contiguous()
    _lib.check(getattr(l, fn_name)(_lib.current_stream(), noise.data_ptr(), latents.data_ptr(), sg.data_ptr(), sn.data_ptr(),
                                   float(guidance_scale), latents.shape[0], latents[0].numel(), _lib.torch_dtype_code(latents.dtype)), fn_name)
    return latents


def cfg_euler_step_(noise: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                    guidance_scale: float) -> torch.Tensor:
    """In place: latents <- Euler step with eps = u + g (t - u); noise = [uncond rows ; cond rows] (g > 0)
    or the plain prediction (g <= 0)."""
    return _cfg_step_plain_("mx_cfg_euler_step", noise, latents, sigma, sigma_next, guidance_scale)


def cfg_flow_step_(noise: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                   guidance_scale: float) -> torch.Tensor:
    """The flow-match step on the same layout: latents <- latents + (sigma_next - sigma) * (u + g (t - u))."""
    return _cfg_step_plain_("mx_cfg_flow_step", noise, latents, sigma, sigma_next, guidance_scale)


def layernorm_mod(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, rows_per_batch: int, eps: float = 1e-6,
                  scale2: Optional[torch.Tensor] = None, shift2: Optional[torch.Tensor] = None):
    """x bf16 [M, C]; scale/shift fp32 [B, C] (contiguous rows) -> y (and y2 when scale2/shift2 are given)."""
    l = _lib.load()
    _bf16(x)
    m, c = x.shape
    y = torch.empty_like(x)
    y2 = torch.empty_like(x) if scale2 is not None else None
    for t in (scale, shift, scale2, shift2):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == c)
    _lib.check(l.mx_layernorm_mod(_lib.current_stream(), x.data_ptr(), y.data_ptr(), _p(y2), scale.data_ptr(), shift.data_ptr(),
                                  _p(scale2), _p(shift2), c, m, c, rows_per_batch, eps), "mx_layernorm_mod")
    return (y, y2) if y2 is not None else y


def rmsnorm_heads_(x: torch.Tensor, nbatch: int, rows_per_batch: int, batch_rows: int, row_off: int, heads_total: int,
                   heads_q: int, wq: torch.Tensor, wk: torch.Tensor, eps: float = 1e-6, q_scale: float = 1.0) -> torch.Tensor:
    l = _lib.load()
    _bf16(x)
    _lib.check(l.mx_rmsnorm_heads(_lib.current_stream(), x.data_ptr(), x.shape[1], nbatch, rows_per_batch, batch_rows, row_off,
                                  heads_total, heads_q, wq.data_ptr(), wk.data_ptr(), eps, q_scale), "mx_rmsnorm_heads")
    return x


def cfg_step_rows_(gathered: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                   guidance_scale: float, n_slabs: int, flow: bool) -> torch.Tensor:
    """In place: the model's step (``flow``: the flow-match one) on the world gather of the split-batch patch parallelism, read where it lies:
    gathered [2 * n_slabs, n_lat, C, H / n_slabs, W] = [uncond row slabs ; cond row slabs], latents [n_lat, C, H, W]."""
    fn_name = "mx_cfg_flow_step_rows" if flow else "mx_cfg_euler_step_rows"
    l = _lib.load()
    assert latents.ndim == 4 and latents.is_contiguous() and gathered.is_contiguous() and gathered.dtype == latents.dtype
    n_lat, c, h, w = latents.shape
    assert gathered.numel() >= (2 if guidance_scale > 0 else 1) * latents.numel(), "the gather buffer is smaller than its slots"
    sg = sigma.to(device=latents.device, dtype=torch.float32).contiguous()
    sn = sigma_next.to(device=latents.device, dtype=torch.float32).contiguous()
    _lib.check(getattr(l, fn_name)(_lib.current_stream(), gathered.data_ptr(), latents.data_ptr(), sg.data_ptr(), sn.data_ptr(),
                                   float(guidance_scale), n_lat, c, h, w, int(n_slabs), _lib.torch_dtype_code(latents.dtype)), fn_name)
    return latents


def cfg_euler_step_rows_(gathered: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                         guidance_scale: float, n_slabs: int) -> torch.Tensor:
    """cfg_step_rows_ with the Euler step (mx_cfg_euler_step_rows)."""
    return cfg_step_rows_(gathered, latents, sigma, sigma_next, guidance_scale, n_slabs, False)


def cfg_flow_step_rows_(gathered: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                        guidance_scale: float, n_slabs: int) -> torch.Tensor:
    """cfg_step_rows_ with the flow-match step (mx_cfg_flow_step_rows)."""
    return cfg_step_rows_(gathered, latents, sigma, sigma_next, guidance_scale, n_slabs, True)


# ---- the masked and the multistep step (csrc/scheduler_step.hip), inpainting (csrc/inpaint.hip) ----

def _need(cond: bool, what: str) -> None:
    if not cond:
        raise _lib.MxError(what)


def _step_operands(fn_name: str, noise_pred: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                   guidance_scale: float) -> tuple:
    """the operands every step on [n, C, h, w] latents shares, checked -> (sigma, sigma_next) as fp32 on the latents' device"""
    _need(latents.ndim == 4 and latents.is_contiguous(), f"{fn_name}: latents must be a contiguous [n, C, h, w] tensor")
    n_lat, c, h, w = latents.shape
    rows = (2 if guidance_scale > 0 else 1) * n_lat
    _need(noise_pred.is_contiguous() and noise_pred.dtype == latents.dtype and noise_pred.device == latents.device
          and noise_pred.numel() == rows * c * h * w, f"{fn_name}: the prediction must be contiguous [{rows}, {c}, {h}, {w}] of the latents' dtype")
    for name, t in (("sigma", sigma), ("sigma_next", sigma_next)):
        _need(t.numel() == n_lat, f"{fn_name}: {name} must hold one value per latent row")
    return tuple(t.to(device=latents.device, dtype=torch.float32).contiguous() for t in (sigma, sigma_next))


def _inpaint_rows(fn_name: str, latents: torch.Tensor, slot: Optional[torch.Tensor], init: Optional[torch.Tensor], noise: Optional[torch.Tensor],
                  mask: Optional[torch.Tensor]) -> "_lib.InpaintRows":
    """the inpainting rows of a step on ``latents``, checked; without init: no rows (k = 0)"""
    n_lat, c, h, w = latents.shape
    r = _lib.InpaintRows()
    if init is None:
        _need(slot is None and noise is None and mask is None, f"{fn_name}: slot, noise and mask come with init")
        return r
    k = init.shape[0]
    _need(slot is not None and noise is not None and mask is not None, f"{fn_name}: inpainting rows need slot, init, noise and mask")
    _need(slot.dtype == torch.int32 and slot.numel() == n_lat and slot.is_contiguous() and slot.device == latents.device,
          f"{fn_name}: slot must be a contiguous int32 [{n_lat}] on the latents' device")
    for name, t in (("init", init), ("noise", noise)):
        _need(t.dtype == latents.dtype and tuple(t.shape) == (k, c, h, w) and t.is_contiguous() and t.device == latents.device,
              f"{fn_name}: {name} must be contiguous [{k}, {c}, {h}, {w}] of the latents' dtype, got {t.dtype} {tuple(t.shape)}")
    _need(mask.dtype == torch.uint8 and tuple(mask.shape) == (k, h, w) and mask.is_contiguous() and mask.device == latents.device,
          f"{fn_name}: mask must be contiguous uint8 [{k}, {h}, {w}], got {mask.dtype} {tuple(mask.shape)}")
    r.k, r.slot, r.init, r.noise, r.mask = k, slot.data_ptr(), init.data_ptr(), noise.data_ptr(), mask.data_ptr()
    return r


def _cfg_step_masked_(fn_name: str, noise_pred: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                      guidance_scale: float, slot: Optional[torch.Tensor], init: Optional[torch.Tensor], noise: Optional[torch.Tensor],
                      mask: Optional[torch.Tensor]) -> torch.Tensor:
    l = _lib.load()
    sg, sn = _step_operands(fn_name, noise_pred, latents, sigma, sigma_next, guidance_scale)
    r = _inpaint_rows(fn_name, latents, slot, init, noise, mask)
    n_lat, c, h, w = latents.shape
    _lib.check(getattr(l, fn_name)(_lib.current_stream(), noise_pred.data_ptr(), latents.data_ptr(), sg.data_ptr(), sn.data_ptr(),
                                   float(guidance_scale), n_lat, c, h * w, _lib.torch_dtype_code(latents.dtype), C.byref(r)), fn_name)
    return latents


def cfg_euler_step_masked_(noise_pred: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor, guidance_scale: float,
                           slot: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                           mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place: cfg_euler_step_ on latents [n, C, h, w] with the kept region of the inpainting rows put back in the same launch
    (mx_cfg_euler_step_masked).  slot int32 [n]: row -> its row of init / noise [k, C, h, w] and mask uint8 [k, h, w] (non-zero = repaint), or -1 for a
    plain row; where the mask is 0 the element becomes init + sigma_next * noise.  Without init every row is plain."""
    return _cfg_step_masked_("mx_cfg_euler_step_masked", noise_pred, latents, sigma, sigma_next, guidance_scale, slot, init, noise, mask)


def cfg_flow_step_masked_(noise_pred: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor, guidance_scale: float,
                          slot: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                          mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The flow-match step on the same layout: kept elements become (1 - sigma_next) * init + sigma_next * noise (mx_cfg_flow_step_masked)."""
    return _cfg_step_masked_("mx_cfg_flow_step_masked", noise_pred, latents, sigma, sigma_next, guidance_scale, slot, init, noise, mask)


# ---- second-order multistep samplers (csrc/scheduler_step.hip, sampler_coeffs.cpp) ----

def cfg_multistep_step_(noise_pred: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor, guidance_scale: float,
                        kind: torch.Tensor, coef: torch.Tensor, hist: torch.Tensor, flow: bool, slot: Optional[torch.Tensor] = None,
                        init: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place: one scheduler step on latents [n, C, h, w] whose rows use different samplers (mx_cfg_multistep_step).  kind int32 [n]: 0 = the
    model's Euler step (``flow``: the flow-match one), 1 = DPM-Solver++ 2M (D = x - sigma m), 2 = AB2 (D = m); coef fp32 [n, 3] = (cx, c0, c1) of this
    step per row (``sampler_coeffs``); hist fp32 [n, C, h, w]: D of every multistep row's previous step, read where c1 != 0 and overwritten with
    this step's.  The new latent of a multistep row is cx x + c0 D + c1 hist.  slot / init / noise / mask: the inpainting rows as for
    ``cfg_euler_step_masked_``."""
    fn_name = "mx_cfg_multistep_step"
    l = _lib.load()
    sg, sn = _step_operands(fn_name, noise_pred, latents, sigma, sigma_next, guidance_scale)
    n_lat, c, h, w = latents.shape
    _need(kind.dtype == torch.int32 and kind.numel() == n_lat and kind.is_contiguous() and kind.device == latents.device,
          f"{fn_name}: kind must be a contiguous int32 [{n_lat}] on the latents' device")
    _need(coef.dtype == torch.float32 and tuple(coef.shape) == (n_lat, 3) and coef.is_contiguous() and coef.device == latents.device,
          f"{fn_name}: coef must be contiguous fp32 [{n_lat}, 3] on the latents' device, got {coef.dtype} {tuple(coef.shape)}")
    _need(hist.dtype == torch.float32 and tuple(hist.shape) == (n_lat, c, h, w) and hist.is_contiguous() and hist.device == latents.device,
          f"{fn_name}: hist must be contiguous fp32 [{n_lat}, {c}, {h}, {w}] on the latents' device, got {hist.dtype} {tuple(hist.shape)}")
    ms = _lib.MultistepRows()
    ms.kind, ms.coef, ms.hist = kind.data_ptr(), coef.data_ptr(), hist.data_ptr()
    r = _inpaint_rows(fn_name, latents, slot, init, noise, mask)
    _lib.check(l.mx_cfg_multistep_step(_lib.current_stream(), noise_pred.data_ptr(), latents.data_ptr(), sg.data_ptr(), sn.data_ptr(),
                                       float(guidance_scale), n_lat, c, h * w, _lib.torch_dtype_code(latents.dtype), int(bool(flow)), C.byref(ms),
                                       C.byref(r)), fn_name)
    return latents


def _seeds_and_steps(fn_name: str, n: int, seed, step, device) -> tuple:
    """(seed int64 [n] holding the uint64 bits, step int32 [n] holding the uint32 bits) on ``device``; tensors of those dtypes pass through"""
    out = []
    for name, t, dt, bits in (("seed", seed, torch.int64, 64), ("step", step, torch.int32, 32)):
        if not isinstance(t, torch.Tensor):
            vals = [int(v) & ((1 << bits) - 1) for v in (t if isinstance(t, (list, tuple)) else [t] * n)]
            t = torch.tensor([v - (1 << bits) if v >> (bits - 1) else v for v in vals], dtype=dt)
        _need(t.dtype == dt and t.numel() == n, f"{fn_name}: {name} must hold one {dt} value per row")
        out.append(t.to(device).contiguous())
    return tuple(out)


def seeded_noise(shape, seed, step, domain: int, dtype=torch.float32, device="cuda", scale=None, raw: bool = False) -> torch.Tensor:
    """[n, ...] of ``dtype``: row r holds scale[r] * N(0, 1) noise that is a function of (seed[r], step[r], domain, index within the row) alone
    (mx_noise_fill; csrc/noise.h) -- not of n, of r or of the other rows.  seed / step: an int (every row), a list, or an int64 / int32 tensor of the
    raw bits; ``scale``: None, a float or fp32 [n]; ``raw``: the generator's uint32 words instead, as an int32 tensor of their bits."""
    fn_name = "mx_noise_fill"
    l = _lib.load()
    shape = tuple(int(v) for v in shape)
    _need(len(shape) >= 2 and all(v > 0 for v in shape), f"{fn_name}: the shape must be [n, ...] with positive sizes")
    n = shape[0]
    sd, st = _seeds_and_steps(fn_name, n, seed, step, device)
    sc = None
    if scale is not None and not raw:
        sc = torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
        _need(sc.numel() in (1, n), f"{fn_name}: scale must hold one value, or one per row")
        sc = sc.to(device).expand(n).contiguous()
    out = torch.empty(shape, dtype=torch.int32 if raw else dtype, device=device)
    _lib.check(l.mx_noise_fill(_lib.current_stream(), out.data_ptr(), 0 if raw else _lib.torch_dtype_code(dtype), n, out[0].numel(), sd.data_ptr(),
                               st.data_ptr(), int(domain), _p(sc), int(bool(raw))), fn_name)
    return out


def cfg_stochastic_step_(noise_pred: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor, guidance_scale: float,
                         kind: torch.Tensor, coef: torch.Tensor, hist: torch.Tensor, flow: bool, cn: torch.Tensor, seed: torch.Tensor,
                         step: torch.Tensor, slot: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None,
                         noise: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place: ``cfg_multistep_step_`` with noise made inside the launch (mx_cfg_stochastic_step): a kind-1 / kind-2 row with cn[r] != 0 ends as
    cx x + c0 D + c1 hist + cn z, z the request's own N(0, 1) noise of this step (``seeded_noise`` at domain 2 gives the same values).  cn fp32 [n];
    seed int64 [n] (the uint64 bits); step int32 [n] (the request's step index)."""
    fn_name = "mx_cfg_stochastic_step"
    l = _lib.load()
    sg, sn = _step_operands(fn_name, noise_pred, latents, sigma, sigma_next, guidance_scale)
    n_lat, c, h, w = latents.shape
    _need(kind.dtype == torch.int32 and kind.numel() == n_lat and kind.is_contiguous() and kind.device == latents.device,
          f"{fn_name}: kind must be a contiguous int32 [{n_lat}] on the latents' device")
    _need(coef.dtype == torch.float32 and tuple(coef.shape) == (n_lat, 3) and coef.is_contiguous() and coef.device == latents.device,
          f"{fn_name}: coef must be contiguous fp32 [{n_lat}, 3] on the latents' device, got {coef.dtype} {tuple(coef.shape)}")
    _need(hist.dtype == torch.float32 and tuple(hist.shape) == (n_lat, c, h, w) and hist.is_contiguous() and hist.device == latents.device,
          f"{fn_name}: hist must be contiguous fp32 [{n_lat}, {c}, {h}, {w}] on the latents' device, got {hist.dtype} {tuple(hist.shape)}")
    for name, t, dt in (("cn", cn, torch.float32), ("seed", seed, torch.int64), ("step", step, torch.int32)):
        _need(t.dtype == dt and t.numel() == n_lat and t.is_contiguous() and t.device == latents.device,
              f"{fn_name}: {name} must be a contiguous {dt} [{n_lat}] on the latents' device")
    ms = _lib.MultistepRows()
    ms.kind, ms.coef, ms.hist = kind.data_ptr(), coef.data_ptr(), hist.data_ptr()
    nz = _lib.NoiseRows()
    nz.cn, nz.seed, nz.step = cn.data_ptr(), seed.data_ptr(), step.data_ptr()
    r = _inpaint_rows(fn_name, latents, slot, init, noise, mask)
    _lib.check(l.mx_cfg_stochastic_step(_lib.current_stream(), noise_pred.data_ptr(), latents.data_ptr(), sg.data_ptr(), sn.data_ptr(),
                                        float(guidance_scale), n_lat, c, h * w, _lib.torch_dtype_code(latents.dtype), int(bool(flow)), C.byref(ms),
                                        C.byref(r), C.byref(nz)), fn_name)
    return latents


def cfg_step_(pred: torch.Tensor, latents: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor, guidance_scale: float, flow: bool,
              inpaint: Optional[tuple] = None, multistep: Optional[tuple] = None, noise: Optional[tuple] = None) -> torch.Tensor:
    """In place: the scheduler step of one resolution's rows, by the entry its requests need.  ``flow``: the flow-match model.  ``inpaint``: (slot,
    init, noise, mask) of ``cfg_euler_step_masked_`` when a row is an inpainting request; ``multistep``: (kind, coef, hist) of
    ``cfg_multistep_step_`` when a row steps by DPM-Solver++ 2M or AB2; ``noise``: (cn, seed, step) of ``cfg_stochastic_step_`` beside ``multistep``
    when a row steps by a stochastic sampler.  With none of them it is the plain step, so Euler requests get the launch they always had."""
    if noise is not None:
        _need(multistep is not None, "cfg_step_: noise rows come with multistep rows")
        return cfg_stochastic_step_(pred, latents, sigma, sigma_next, guidance_scale, *multistep, flow, *noise, *(inpaint or ()))
    if multistep is not None:
        return cfg_multistep_step_(pred, latents, sigma, sigma_next, guidance_scale, *multistep, flow, *(inpaint or ()))
    if inpaint is not None:
        return (cfg_flow_step_masked_ if flow else cfg_euler_step_masked_)(pred, latents, sigma, sigma_next, guidance_scale, *inpaint)
    return (cfg_flow_step_ if flow else cfg_euler_step_)(pred, latents, sigma, sigma_next, guidance_scale)


def sampler_coeffs(sampler: str, sigmas, flow: bool, eta: Optional[float] = None):
    """the step coefficients of a multistep sampler ("dpmpp_2m" | "ab2") over a schedule, on the host (mx_sampler_coeffs; no GPU needed):
    sigmas fp32 [n + 1] -> numpy fp32 [n, 4] = (cx, c0 first order, c0 second order, c1 second order) per step.  With ``eta`` (mx_sampler_coeffs_eta):
    [n, 5], the noise coefficient cn behind them, and the stochastic samplers "euler_a" | "dpmpp_2m_sde" beside the two."""
    import numpy as np
    l = _lib.load()
    names = dict(_lib.SAMPLERS, **(_lib.STOCHASTIC_SAMPLERS if eta is not None else {}))
    _need(sampler in names, f"mx_sampler_coeffs: sampler must be one of {sorted(names)}, got {sampler!r}")
    sig = np.ascontiguousarray(np.asarray(sigmas, dtype=np.float32).reshape(-1))
    _need(sig.size >= 2, "mx_sampler_coeffs: a schedule holds at least one step (two sigmas)")
    if eta is not None:
        out = np.empty((sig.size - 1, 5), dtype=np.float32)
        _lib.check(l.mx_sampler_coeffs_eta(names[sampler], int(bool(flow)), sig.ctypes.data, sig.size - 1, float(eta), out.ctypes.data),
                   "mx_sampler_coeffs_eta")
        return out
    out = np.empty((sig.size - 1, 4), dtype=np.float32)
    _lib.check(l.mx_sampler_coeffs(_lib.SAMPLERS[sampler], int(bool(flow)), sig.ctypes.data, sig.size - 1, out.ctypes.data), "mx_sampler_coeffs")
    return out


def inpaint_renoise(init: torch.Tensor, noise: torch.Tensor, keep, sigma) -> torch.Tensor:
    """keep[r] * init[r] + sigma[r] * noise[r] over the rows of init [n, ...], fp32 ops rounded once to init's dtype (mx_inpaint_renoise);
    keep / sigma: fp32 [n] tensors or scalars."""
    l = _lib.load()
    _need(init.is_cuda and init.ndim >= 2 and init.is_contiguous(), "mx_inpaint_renoise: init must be a contiguous CUDA tensor [n, ...]")
    _need(noise.dtype == init.dtype and noise.shape == init.shape and noise.is_contiguous() and noise.device == init.device,
          f"mx_inpaint_renoise: noise must be contiguous {tuple(init.shape)} of dtype {init.dtype}, got {noise.dtype} {tuple(noise.shape)}")
    n = init.shape[0]
    scal = []
    for name, t in (("keep", keep), ("sigma", sigma)):
        t = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
        _need(t.numel() in (1, n), f"mx_inpaint_renoise: {name} must hold one value, or one per row")
        scal.append(t.to(init.device).expand(n).contiguous())
    out = torch.empty_like(init)
    _lib.check(l.mx_inpaint_renoise(_lib.current_stream(), init.data_ptr(), noise.data_ptr(), out.data_ptr(), scal[0].data_ptr(), scal[1].data_ptr(),
                                    n, init[0].numel(), _lib.torch_dtype_code(init.dtype)), "mx_inpaint_renoise")
    return out


def mask_to_latent(mask: torch.Tensor, factor: int) -> torch.Tensor:
    """a client's mask uint8 [B, H, W] -> uint8 [B, H / factor, W / factor] of 0 / 1: mask[b, factor y, factor x] >= 128 (mx_mask_to_latent)"""
    l = _lib.load()
    _need(mask.is_cuda and mask.dtype == torch.uint8 and mask.ndim == 3 and mask.is_contiguous(),
          f"mx_mask_to_latent: expected a contiguous CUDA uint8 [B, H, W] mask, got {mask.dtype} {tuple(mask.shape)}")
    b, h, w = mask.shape
    _need(factor > 0 and h % factor == 0 and w % factor == 0, f"mx_mask_to_latent: {h} x {w} is no multiple of the factor {factor}")
    out = torch.empty((b, h // factor, w // factor), dtype=torch.uint8, device=mask.device)
    _lib.check(l.mx_mask_to_latent(_lib.current_stream(), mask.data_ptr(), out.data_ptr(), b, h, w, int(factor)), "mx_mask_to_latent")
    return out


def rgb8_paste_(decoded: torch.Tensor, original: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """In place: decoded uint8 [B, H, W, 3] takes original's pixel wherever mask uint8 [B, H, W] is below 128 (mx_rgb8_paste)"""
    l = _lib.load()
    _need(decoded.is_cuda and decoded.dtype == torch.uint8 and decoded.ndim == 4 and decoded.shape[-1] == 3 and decoded.is_contiguous(),
          f"mx_rgb8_paste: expected a contiguous CUDA uint8 [B, H, W, 3] image, got {decoded.dtype} {tuple(decoded.shape)}")
    b, h, w, _c = decoded.shape
    _need(original.dtype == torch.uint8 and original.shape == decoded.shape and original.is_contiguous() and original.device == decoded.device,
          f"mx_rgb8_paste: the original must be contiguous uint8 {tuple(decoded.shape)}, got {original.dtype} {tuple(original.shape)}")
    _need(mask.dtype == torch.uint8 and tuple(mask.shape) == (b, h, w) and mask.is_contiguous() and mask.device == decoded.device,
          f"mx_rgb8_paste: the mask must be contiguous uint8 [{b}, {h}, {w}], got {mask.dtype} {tuple(mask.shape)}")
    _lib.check(l.mx_rgb8_paste(_lib.current_stream(), decoded.data_ptr(), original.data_ptr(), mask.data_ptr(), b, h, w), "mx_rgb8_paste")
    return decoded


class _ResizePlans:
    """mx_resize plans of one device, least recently used out first: a serving slot sees a handful of (client size, request size) pairs"""
    CAPACITY = 16

    def __init__(self):
        self._plans = collections.OrderedDict()

    def get(self, key: tuple) -> int:
        l = _lib.load()
        h = self._plans.get(key)
        if h is not None:
            self._plans.move_to_end(key)
            return h
        h = l.mx_resize_create(*key)
        if not h:
            _lib.check(1, "mx_resize_create")
        self._plans[key] = h
        if len(self._plans) > self.CAPACITY:
            # the evicted plan's tables may still be read by a launch in flight: hipFree waits for the device before it releases them
            l.mx_resize_destroy(self._plans.popitem(last=False)[1])
        return h


_resize_plans = {}


def resize_u8(x: torch.Tensor, size, resample: str = "lanczos") -> torch.Tensor:
    """uint8 [B, H, W, 3] or [B, H, W] -> [B, size[0], size[1](, 3)], bit-equal to Pillow's Image.resize((size[1], size[0]), resample) of every
    image (mx_resize_u8: both passes in one launch); ``resample``: "lanczos" (diffusers' VaeImageProcessor default), "bicubic" or "bilinear".
    The plan (the coefficient tables in device memory) is made on first use and kept per device."""
    l = _lib.load()
    _need(x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous() and (x.ndim == 3 or (x.ndim == 4 and x.shape[-1] == 3)),
          f"mx_resize_u8: expected a contiguous CUDA uint8 [B, H, W, 3] or [B, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    _need(resample in _lib.RESIZE_FILTERS, f"mx_resize_u8: resample must be one of {sorted(_lib.RESIZE_FILTERS)}, got {resample!r}")
    oh, ow = (int(s) for s in size)
    b, h, w = x.shape[:3]
    _need(b > 0 and h > 0 and w > 0 and oh > 0 and ow > 0, f"mx_resize_u8: sizes must be positive, got {tuple(x.shape)} -> {(oh, ow)}")
    c = 3 if x.ndim == 4 else 1
    with torch.cuda.device(x.device):
        plan = _resize_plans.setdefault(x.device.index, _ResizePlans()).get((h, w, oh, ow, _lib.RESIZE_FILTERS[resample]))
        out = torch.empty((b, oh, ow) + tuple(x.shape[3:]), dtype=torch.uint8, device=x.device)
        _lib.check(l.mx_resize_u8(plan, _lib.current_stream(), x.data_ptr(), out.data_ptr(), b, c), "mx_resize_u8")
    return out


# ---- inpainting only the masked region (csrc/inpaint_overlay.hip, inpaint_region.cpp) ----

def _need_mask(what: str, mask: torch.Tensor) -> tuple:
    _need(mask.is_cuda and mask.dtype == torch.uint8 and mask.ndim == 3 and mask.is_contiguous() and mask.numel() > 0,
          f"{what}: expected a contiguous CUDA uint8 [B, H, W] mask, got {mask.dtype} {tuple(mask.shape)} on {mask.device.type}")
    return tuple(mask.shape)


def blur_box_params(radius: float) -> tuple:
    """(r, ww, fw) of one box pass of Pillow's GaussianBlur(radius) (mx_blur_box_params); host only"""
    r, ww, fw = C.c_int(), C.c_uint32(), C.c_uint32()
    _lib.check(_lib.load().mx_blur_box_params(float(radius), C.byref(r), C.byref(ww), C.byref(fw)), "mx_blur_box_params")
    return r.value, ww.value, fw.value


def gaussian_blur_u8(mask: torch.Tensor, radius: float) -> torch.Tensor:
    """uint8 [B, H, W] -> a new tensor of the same shape, every plane bit-equal to Pillow's ``Image.filter(ImageFilter.GaussianBlur(radius))`` --
    diffusers' VaeImageProcessor.blur (mx_gaussian_blur_u8: the three row passes in one launch, one launch per column pass); radius <= 0 copies"""
    l = _lib.load()
    b, h, w = _need_mask("mx_gaussian_blur_u8", mask)
    with torch.cuda.device(mask.device):
        out = torch.empty_like(mask)
        scratch = torch.empty_like(mask) if radius > 0 else None
        _lib.check(l.mx_gaussian_blur_u8(_lib.current_stream(), mask.data_ptr(), out.data_ptr(), _p(scratch), b, h, w, float(radius)), "mx_gaussian_blur_u8")
    return out


def mask_bbox(mask: torch.Tensor) -> torch.Tensor:
    """uint8 [B, H, W] -> int32 [B, 4] on the device: (x_min, y_min, x_max + 1, y_max + 1) over the non-zero bytes of each plane, (W, H, 0, 0) for an
    empty one (mx_mask_bbox_u8)"""
    l = _lib.load()
    b, h, w = _need_mask("mx_mask_bbox_u8", mask)
    with torch.cuda.device(mask.device):
        out = torch.empty((b, 4), dtype=torch.int32, device=mask.device)
        _lib.check(l.mx_mask_bbox_u8(_lib.current_stream(), mask.data_ptr(), out.data_ptr(), b, h, w), "mx_mask_bbox_u8")
    return out


def crop_region(bbox, mask_size, size, pad: int) -> tuple:
    """diffusers' get_crop_region applied to a mask's bounding box (mx_crop_region; host only): ``bbox`` = (x1, y1, x2, y2) as one row of mask_bbox
    gives it, ``mask_size`` = (H, W) of the mask, ``size`` = (H, W) the crop will be processed at -> (x1, y1, x2, y2) inside the mask with about that
    aspect.  An empty box, what an empty mask gives, is refused."""
    x1, y1, x2, y2 = (int(v) for v in bbox)
    out = (C.c_int32 * 4)()
    _lib.check(_lib.load().mx_crop_region(x1, y1, x2, y2, int(mask_size[1]), int(mask_size[0]), int(size[1]), int(size[0]), int(pad), out), "mx_crop_region")
    return tuple(out)


def rgb8_overlay(decoded: torch.Tensor, original: torch.Tensor, mask: torch.Tensor, x: int = 0, y: int = 0) -> torch.Tensor:
    """decoded uint8 [B, h, w, 3] blended into original uint8 [B, H, W, 3] at (x, y) under the soft mask uint8 [B, H, W] (255 = repaint) -> a new
    uint8 [B, H, W, 3]: original's bytes outside the box, diffusers' apply_overlay inside (mx_rgb8_overlay, one launch)"""
    l = _lib.load()
    _need(original.is_cuda and original.dtype == torch.uint8 and original.ndim == 4 and original.shape[-1] == 3 and original.is_contiguous()
          and original.numel() > 0,
          f"mx_rgb8_overlay: expected a contiguous CUDA uint8 [B, H, W, 3] original, got {original.dtype} {tuple(original.shape)} on {original.device.type}")
    b, hh, ww, _c = original.shape
    _need(decoded.dtype == torch.uint8 and decoded.ndim == 4 and decoded.shape[0] == b and decoded.shape[-1] == 3 and decoded.is_contiguous()
          and decoded.device == original.device and decoded.numel() > 0,
          f"mx_rgb8_overlay: the decoded image must be contiguous uint8 [{b}, h, w, 3] on the original's device, got {decoded.dtype} {tuple(decoded.shape)}")
    _need(mask.dtype == torch.uint8 and tuple(mask.shape) == (b, hh, ww) and mask.is_contiguous() and mask.device == original.device,
          f"mx_rgb8_overlay: the mask must be contiguous uint8 [{b}, {hh}, {ww}], got {mask.dtype} {tuple(mask.shape)}")
    h, w = decoded.shape[1:3]
    with torch.cuda.device(original.device):
        out = torch.empty_like(original)
        _lib.check(l.mx_rgb8_overlay(_lib.current_stream(), decoded.data_ptr(), original.data_ptr(), mask.data_ptr(), out.data_ptr(), b, hh, ww,
                                     int(x), int(y), w, h), "mx_rgb8_overlay")
    return out


def lora_terms(terms) -> "C.Array":
    """a list of term dicts -> the mx_lora_term array (the tensors stay referenced by the caller).  Keys: w_off, N, K, up (bf16 [rows, R]),
    down_t (bf16 [K, R]), scale; optional row0 (0), rows (N), colsum_off / bias_off (byte offsets of the folded matrix's fp32 vectors), dbias
    (fp32 [rows]).  Tensors may also be given as raw device addresses (ints), then with an explicit R."""
    arr = (_lib.LoraTerm * max(len(terms), 1))()
    for i, t in enumerate(terms):
        a = arr[i]
        a.w_off, a.N, a.K = int(t["w_off"]), int(t["N"]), int(t["K"])
        a.row0 = int(t.get("row0", 0))
        a.rows = int(t.get("rows", a.N - a.row0))
        up, down_t, dbias = t["up"], t["down_t"], t.get("dbias")
        if torch.is_tensor(up):
            _need(up.dtype == torch.bfloat16 and down_t.dtype == torch.bfloat16 and up.is_contiguous() and down_t.is_contiguous()
                  and up.ndim == 2 and down_t.ndim == 2 and up.shape == (a.rows, down_t.shape[1]) and down_t.shape[0] == a.K,
                  f"mx_lora_merge: term {i}: up must be bf16 [rows, R] and down_t bf16 [K, R], got {tuple(up.shape)} and {tuple(down_t.shape)}")
            _need(dbias is None or (dbias.dtype == torch.float32 and dbias.is_contiguous() and dbias.shape == (a.rows,)),
                  f"mx_lora_merge: term {i}: dbias must be fp32 [rows]")
            a.R = int(t.get("R", up.shape[1]))
            a.up, a.down_t, a.dbias = up.data_ptr(), down_t.data_ptr(), _p(dbias)
        else:
            a.R, a.up, a.down_t, a.dbias = int(t["R"]), up, down_t, dbias
        a.scale = float(t["scale"])
        cs, bs = t.get("colsum_off"), t.get("bias_off")
        a.colsum_off = _lib.LORA_NO_VECTOR if cs is None else int(cs)
        a.bias_off = _lib.LORA_NO_VECTOR if bs is None else int(bs)
    return arr


def lora_merge_validate(terms, blob_bytes: int) -> None:
    """mx_lora_merge_validate (host only): raises MxError with the library's reason for a table the merge would refuse"""
    _lib.check(_lib.load().mx_lora_merge_validate(lora_terms(terms), len(terms), int(blob_bytes)), "mx_lora_merge_validate")


def lora_merge(base: torch.Tensor, out: torch.Tensor, terms, table: Optional[torch.Tensor] = None) -> None:
    """out[rows of every term] = bf16(base + sum scale * up down_t^T) in ONE launch (mx_lora_merge): ``base`` and ``out`` are two blobs of the same
    size (any dtype, viewed as bytes; every offset of a term counts from their first byte), ``terms`` as lora_terms takes them.  ``table``: a uint8
    device buffer of at least mx_lora_table_bytes(len(terms)) bytes to reuse; allocated here when None."""
    l = _lib.load()
    _need(base.is_cuda and out.is_cuda and base.is_contiguous() and out.is_contiguous() and base.device == out.device,
          "mx_lora_merge: base and out must be contiguous CUDA tensors on one device")
    nbytes = base.numel() * base.element_size()
    _need(out.numel() * out.element_size() == nbytes, "mx_lora_merge: base and out differ in size")
    arr = lora_terms(terms)
    with torch.cuda.device(base.device):
        need = l.mx_lora_table_bytes(len(terms))
        if table is None:
            table = torch.empty(max(need, 16), dtype=torch.uint8, device=base.device)
        _lib.check(l.mx_lora_merge(_lib.current_stream(), base.data_ptr(), out.data_ptr(), nbytes, arr, len(terms), table.data_ptr(), table.numel()),
                   "mx_lora_merge")
