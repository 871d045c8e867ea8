"""The addressing the three 64-key-tile attention kernels share (csrc/attn_tile.h), held against itself on the raw bits.  Nothing here is compared with a
reference: that is tests/test_kernel_forms_gpu.py's job.
  * A problem with B = 2, H = 4 is dealt by the XCD-aware workgroup map.  It must equal, bit for bit, its eight (batch, head) slices launched alone as
    B = 1, H = 1 problems (the plain map) on the same buffers: pointers offset by head * 64 and the batch's rows, the same leading dimensions.
  * mx_attention_prescaled_chunked with two key chunks must equal mx_attention_prescaled on the same keys laid out contiguously, bit for bit: the tiles and
    their order are the same, only where the ring (or the register stager) fetches them differs.
Every case pins its route (mx_attention_kernel_name), writes into guarded buffers (the guards are compared too) and runs twice."""
import zlib

import pytest
import torch

import kernel_ref as R
from kernel_form_cases import vt_ld
from sduss_amd import lib as L
from sduss_amd.ops import vt_pos

pytestmark = pytest.mark.gpu

B, H, D = 2, 4, 256
LDQ = LDK = LDO = D + 8                         # NaN (inputs) / guard (output) columns past H * 64
GEN, DMA, W64 = "attn_fwd_kernel<true>", "attn_fwd_dma_kernel<true>", "attn_fwd64_kernel"
# kernel: (Lq, Lk) of the XCD-map problem, (Lq, Lk) of the two-chunk problem
CASES = {GEN: ((129, 97), (65, 128)), DMA: ((129, 192), (129, 256)), W64: ((2049, 193), (2048, 256))}


def _inputs(name, lq, lk, dev):
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    bf = torch.bfloat16
    q = (torch.randn((B * lq, D), generator=gen) * (0.125 * 1.4426950408889634)).to(bf).to(dev)
    k = torch.randn((B * lk, D), generator=gen).to(bf).to(dev)
    v = torch.randn((B * lk, D), generator=gen).to(bf).to(dev)
    return q, k, v


def _vt_image(v, nch, lk, dev):
    """V^T [nch, B, D, ldvt] of v [B * lk, D]: chunk c holds keys [c * lk / nch, (c + 1) * lk / nch) in MX_VT_POS order, zero where no key lands, NaN past it"""
    kc = lk // nch
    ldvt = vt_ld(kc) + 8
    vt = torch.full((nch, B, D, ldvt), float("nan"), dtype=v.dtype, device=dev)
    vt[..., :vt_ld(kc)] = 0
    vt[..., vt_pos(kc).to(dev)] = v.view(B, nch, kc, D).permute(1, 0, 3, 2)
    return vt, ldvt


def _twice(launch, obuf, what):
    """two launches into obuf, which must agree; returns the first result"""
    outs = []
    for _ in range(2):
        launch()
        torch.cuda.synchronize()
        outs.append(obuf.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{what}: two runs differ"
    return outs[0]


def xcd_case(kernel, lq, lk, dev="cuda"):
    """(whole problem through the XCD-aware map, the eight slices through the plain map): two guarded O buffers"""
    lib = L.load()
    assert L.attention_kernel_of(B, H, lq, lk, LDO) == kernel and L.attention_kernel_of(1, 1, lq, lk, LDO) == kernel
    q, k, v = _inputs(f"xcd {kernel} {lq} {lk}", lq, lk, dev)
    qbuf, _ = R.nan_padded(q, LDQ)
    kbuf, _ = R.nan_padded(k, LDK, extra_rows=16)
    vt, ldvt = _vt_image(v, 1, lk, dev)
    whole, _ = R.guarded(B * lq, D, LDO, torch.bfloat16, dev)
    parts, _ = R.guarded(B * lq, D, LDO, torch.bfloat16, dev)
    st = L.current_stream()

    def run_whole():
        L.check(lib.mx_attention_prescaled(st, qbuf.data_ptr(), LDQ, kbuf.data_ptr(), LDK, vt.data_ptr(), ldvt, D * ldvt, whole.data_ptr(), LDO, B, H, lq, lk), "whole")

    def run_parts():
        for b in range(B):
            for h in range(H):
                L.check(lib.mx_attention_prescaled(st, qbuf.data_ptr() + 2 * (b * lq * LDQ + h * 64), LDQ, kbuf.data_ptr() + 2 * (b * lk * LDK + h * 64), LDK,
                                                   vt.data_ptr() + 2 * (b * D + h * 64) * ldvt, ldvt, D * ldvt,
                                                   parts.data_ptr() + 2 * (b * lq * LDO + h * 64), LDO, 1, 1, lq, lk), f"slice b{b} h{h}")

    return _twice(run_whole, whole, "whole problem"), _twice(run_parts, parts, "slices")


def chunk_case(kernel, lq, lk, dev="cuda"):
    """(two key chunks in the patch-parallel layout, the same keys contiguous): two guarded O buffers"""
    lib = L.load()
    nch = 2
    kc = lk // nch
    assert L.attention_kernel_of(B, H, lq, lk, LDO, key_chunk=kc) == kernel and L.attention_kernel_of(B, H, lq, lk, LDO) == kernel
    q, k, v = _inputs(f"chunk {kernel} {lq} {lk}", lq, lk, dev)
    qbuf, _ = R.nan_padded(q, LDQ)
    kbuf, _ = R.nan_padded(k, LDK, extra_rows=16)
    kcbuf, _ = R.nan_padded(k.view(B, nch, kc, D).transpose(0, 1).reshape(B * lk, D), LDK, extra_rows=16)    # chunk c of batch b at row (c * B + b) * kc
    vt, ldvt = _vt_image(v, 1, lk, dev)
    vtc, ldvtc = _vt_image(v, nch, lk, dev)
    chunked, _ = R.guarded(B * lq, D, LDO, torch.bfloat16, dev)
    plain, _ = R.guarded(B * lq, D, LDO, torch.bfloat16, dev)
    st = L.current_stream()

    def run_chunked():
        L.check(lib.mx_attention_prescaled_chunked(st, qbuf.data_ptr(), LDQ, kcbuf.data_ptr(), LDK, vtc.data_ptr(), ldvtc, D * ldvtc, chunked.data_ptr(), LDO,
                                                   B, H, lq, lk, kc, kc * LDK, B * kc * LDK, B * D * ldvtc), "chunked")

    def run_plain():
        L.check(lib.mx_attention_prescaled(st, qbuf.data_ptr(), LDQ, kbuf.data_ptr(), LDK, vt.data_ptr(), ldvt, D * ldvt, plain.data_ptr(), LDO, B, H, lq, lk), "plain")

    return _twice(run_chunked, chunked, "chunked"), _twice(run_plain, plain, "contiguous")


def _same_bits(a, b, rows, what):
    assert R.guard_violations(a, rows, D) == 0 and R.guard_violations(b, rows, D) == 0, f"{what}: a launch wrote outside O"
    assert not torch.isnan(a[:rows, :D].float()).any(), f"{what}: NaN in O"
    bad = int((a.view(torch.int16) != b.view(torch.int16)).sum())
    assert bad == 0, f"{what}: {bad} of {a.numel()} elements differ in their bits"


@pytest.mark.parametrize("kernel", list(CASES))
def test_attention_addressing_bit_exact(cuda_device, kernel):
    (lq, lk), (clq, clk) = CASES[kernel]
    whole, parts = xcd_case(kernel, lq, lk, cuda_device)
    _same_bits(whole, parts, B * lq, f"{kernel} Lq {lq} Lk {lk}: XCD-aware map vs eight (batch, head) slices")
    chunked, plain = chunk_case(kernel, clq, clk, cuda_device)
    _same_bits(chunked, plain, B * clq, f"{kernel} Lq {clq} Lk {clk}: two key chunks vs contiguous keys")
