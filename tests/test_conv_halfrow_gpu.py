"""mx_conv3x3_halfrow (csrc/conv_halo.hip, the half-row form) on the GPU: the 3x3 conv of a 128-wide image whose tile is 4 output rows x 64 columns,
staged once per 64-channel chunk with the neighbouring half's column beside it.  Built like tests/test_conv_halo_gpu.py: every case runs plain, with
a row bias, with a residual and with GroupNorm partial sums; NaN-padded inputs, guarded outputs, two runs equal bit for bit, every element against
the fp64 reference within its own bound (tests/kernel_ref.py: conv_acc, epilogue_ref).  With random inputs a lane that reads memory's (y, -1) =
(y - 1, 127) or (y, 128) = (y + 1, 0) instead of zero, or the zero line instead of column 63 / 64, falls outside its bound: no special data.
The reference of a case is computed once and shared by its four variants."""
import ctypes as C
import functools
import zlib

import pytest
import torch

import kernel_ref as R
from sduss_amd import lib as L

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, N)
CASES = {
    "one_row_block_one_chunk": (1, 4, 128, 64, 160),     # both halves, both vertical halos are zero rows
    "buffer_turnover": (1, 4, 128, 128, 160),            # the second buffer and its side column
    "five_chunks": (1, 4, 128, 320, 160),                # an odd count
    "two_row_blocks_two_panels": (1, 8, 128, 128, 320),  # tiles share halo rows; two feature panels
    "tile_edge_is_image_edge": (2, 4, 128, 128, 160),    # the halo must be zero, not the neighbouring image
}
VARIANTS = ("plain", "rowbias", "residual", "gn_partials")
PAD_ROWS = 192                                           # NaN pixels in front of and behind the input: more than a halo row and its side columns


def _randn(shape, gen, dev, scale=1.0):
    return (torch.randn(shape, generator=gen, dtype=torch.float32) * scale).to(dev)


@functools.lru_cache(maxsize=None)
def _case(name, dev):
    """operands of a case (device buffers with NaN padding) and the fp64 accumulators with their bounds"""
    B, H, W, Cin, N = CASES[name]
    bf = torch.bfloat16
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    M, K = B * H * W, 9 * Cin
    x = _randn((B, H, W, Cin), gen, dev).to(bf)
    xbuf = torch.full((PAD_ROWS + M + PAD_ROWS, Cin), float("nan"), dtype=bf, device=dev)
    xbuf[PAD_ROWS:PAD_ROWS + M] = x.reshape(M, Cin)
    w = _randn((N, K), gen, dev, K ** -0.5).to(bf)
    wbuf = torch.full((N + 2, K), float("nan"), dtype=bf, device=dev)
    wbuf[:N] = w
    bias = _randn((N,), gen, dev)
    rbbuf, rb = R.nan_padded(_randn((B, N), gen, dev), N + 4, extra_rows=1)
    res = _randn((M, N), gen, dev).to(bf)
    resbuf, _ = R.nan_padded(res, N + 8, extra_rows=2)
    acc, e = R.conv_acc(x, w, Cin)
    return dict(B=B, H=H, W=W, Cin=Cin, N=N, M=M, K=K, xbuf=xbuf, wbuf=wbuf, bias=bias, rbbuf=rbbuf, rb=rb, res=res, resbuf=resbuf, acc=acc, e=e)


def _desc(c, variant, cbuf, part):
    d = L.GemmDesc()
    d.a = c["xbuf"][PAD_ROWS:].data_ptr()
    d.w, d.c, d.bias = c["wbuf"].data_ptr(), cbuf.data_ptr(), c["bias"].data_ptr()
    d.M, d.N, d.K, d.ldc = c["M"], c["N"], c["K"], cbuf.shape[1]
    d.rows_per_batch = c["H"] * c["W"]
    d.B, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride = c["B"], c["H"], c["W"], c["Cin"], c["H"], c["W"], 1
    if variant in ("rowbias", "gn_partials"):
        d.rowbias, d.ldrb = c["rbbuf"].data_ptr(), c["rbbuf"].shape[1]
    if variant == "residual":
        d.residual, d.ldr = c["resbuf"].data_ptr(), c["resbuf"].shape[1]
    if part is not None:
        d.gn_part_out = part.data_ptr()
    return d


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_conv_halfrow(cuda_device, name, variant):
    dev = str(cuda_device)
    c = _case(name, dev)
    lib = L.load()
    M, N = c["M"], c["N"]
    cbuf, _ = R.guarded(M, N, N + 8, torch.bfloat16, dev)
    part = None
    if variant == "gn_partials":
        part = torch.full((M // 64 + 1, N, 2), float("nan"), dtype=torch.float32, device=dev)
    d = _desc(c, variant, cbuf, part)
    assert lib.mx_conv3x3_halfrow_serves(C.byref(d)) > 0, L.load().mx_last_error()

    def run():
        L.check(lib.mx_conv3x3_halfrow(L.current_stream(), C.byref(d)), f"{name}/{variant}")
        torch.cuda.synchronize()
        return cbuf.clone(), (part.clone() if part is not None else None)

    (o1, p1), (o2, p2) = run(), run()
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)), "two runs differ"
    rb = c["rb"] if variant in ("rowbias", "gn_partials") else None
    ref, bound = R.epilogue_ref(c["acc"], c["e"], bias=c["bias"], rowbias=rb, rows_per_batch=c["H"] * c["W"],
                                residual=c["res"] if variant == "residual" else None)
    n, ratio = R.violations(o1[:M, :N], ref, bound)
    print(f"{name}/{variant}: worst err / bound = {ratio:.3g}")
    assert n == 0, f"{n} of {M * N} elements outside their fp64 bound (worst err / bound = {ratio:.3g})"
    assert R.guard_violations(o1, M, N) == 0, "the launch wrote outside its output rows / columns"
    if part is None:
        return
    # the partial sums are those of the ACCUMULATORS: the stored values minus bias + row bias.  A stored value is the fp32 sum rounded to bf16, so
    # a_i = stored_i - const differs from the accumulator by d_i = 2^-8 |stored_i| (rounding) + 4 2^-24 (|stored_i| + |const|) (the fp32 adds); the
    # kernel sums 64 values in fp32: 64 2^-24 of the sum of magnitudes.  Squares: |a^2 - acc^2| <= d (2 |a| + d), plus the fp32 square and sum.
    # (The rule of tests/test_conv_halo_gpu.py; chunk k of the partial sums is output rows 64 k .. 64 k + 63 = one tile row of one half.)
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)), "two runs differ (partial sums)"
    assert bool(torch.isnan(p1[M // 64:]).all()), "partial sums written past the last 64-row chunk"
    const = c["bias"].double()[None, :] + c["rb"].double()[torch.arange(M, device=dev) // (c["H"] * c["W"])]
    stored = o1[:M, :N].double()
    a = stored - const
    dlt = 2.0 ** -8 * stored.abs() + 4 * R.U32 * (stored.abs() + const.abs())
    blk = lambda t: t.reshape(M // 64, 64, N).sum(1)
    got_s, got_q = p1[:M // 64, :, 0].double(), p1[:M // 64, :, 1].double()
    bs = blk(dlt) + 64 * R.U32 * blk(a.abs())
    bq = blk(dlt * (2 * a.abs() + dlt)) + 66 * R.U32 * blk(a * a)
    ns, rs = R.violations(got_s, blk(a), bs)
    nq, rq = R.violations(got_q, blk(a * a), bq)
    print(f"{name}/{variant}: partial sums worst err / bound = {rs:.3g}, squares {rq:.3g}")
    assert ns == 0 and nq == 0, f"partial sums outside their bound: {ns} sums (worst {rs:.3g}), {nq} sums of squares (worst {rq:.3g})"
