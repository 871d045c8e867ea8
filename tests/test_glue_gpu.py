"""The glue kernels at the models' boundaries, ONE LAUNCH per test body through the entry points of include/mxdenoise.h ("Glue kernels, one launch
each"): the cases of tests/glue_cases.py against the references of tests/glue_ref.py.

Every copy and conversion is compared BIT FOR BIT, whole tensors: outputs live in guarded buffers (guard rows behind them, guard columns where
the launch takes a row stride), inputs carry NaN behind their last element and in their padding columns.  The two bounded families (the
sinusoids of time_embed / sinus_embed, softmax_rows) are held to the derived per-cell intervals of glue_ref.py; those tests print their worst
err / bound (glue_ref.excess) and how many cells differ from the fp32 oracle's rounding, a figure and not an assertion (profiles/glue_kernels_digest.txt holds
one run's figures)."""
import pytest
import torch

import glue_cases as K
import glue_ref as R
from sduss_amd import lib as L

pytestmark = pytest.mark.gpu
NAN = float("nan")
BF16 = torch.bfloat16


def _in(t, dev, tail=64):
    """an operand the launch only reads, flat, with NaN behind its last element (an integer operand: the largest value)"""
    flat = t.reshape(-1)
    buf = torch.full((flat.numel() + tail,), NAN if t.dtype.is_floating_point else torch.iinfo(t.dtype).max, dtype=t.dtype, device=dev)
    buf[:flat.numel()] = flat.to(dev)
    return buf


def _out(rows, cols, dtype, dev):
    """a guarded output [rows, cols] of a 2-byte or 4-byte dtype; returns (buffer, typed view of the buffer)"""
    buf, _view = R.guarded(rows, cols, cols, BF16 if dtype == torch.float16 else dtype, dev)
    return buf, buf.view(dtype) if dtype == torch.float16 else buf


def _guards(buf, rows, cols, what):
    assert R.guard_violations(buf, rows, cols) == 0, f"{what}: wrote outside its rows / columns"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(got, want, what):
    g, w = _bits(got.cpu()), _bits(want)
    assert g.shape == w.shape, what
    bad = g != w
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} of {g.numel()} cells differ bit for bit, the first at {tuple(bad.nonzero()[0].tolist())}"


def _launch(status, what):
    L.check(status, what)
    torch.cuda.synchronize()


# ---- prep_latent, nhwc_to_nchw ----

@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_IDS)
@pytest.mark.parametrize("case", K.PREP_CASES, ids=str)
def test_prep_latent(cuda_device, case, dtype):
    dev, (B, Cin, H, W, CP) = cuda_device, case
    x = K.build_prep(case, dtype)
    want = R.prep_latent_ref(x, CP)
    d_x = _in(x, dev)
    buf, view = _out(B * H * W, CP, BF16, dev)
    _launch(L.load().mx_prep_latent(L.current_stream(), d_x.data_ptr(), L.torch_dtype_code(dtype), buf.data_ptr(), B, Cin, H * W, CP), f"prep_latent {case}")
    _same(view[:B * H * W], want, f"prep_latent {case} {dtype}")                  # the padded channels as +0: their bits are compared too
    _guards(buf, B * H * W, CP, f"prep_latent {case}")


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_IDS)
@pytest.mark.parametrize("case", K.TO_NCHW_CASES, ids=str)
def test_nhwc_to_nchw(cuda_device, case, dtype):
    dev, (B, Cc, HW, ld) = cuda_device, case
    x = K.build_to_nchw(case)                                                     # NaN in columns C .. ld
    want = R.nhwc_to_nchw_ref(x, B, Cc, HW, dtype)
    if dtype == torch.float16:
        assert torch.isinf(want).sum() >= 4 and want.reshape(-1).float().abs().min() == 0.0
    d_x = _in(x, dev)
    buf, view = _out(B * Cc, HW, dtype, dev)
    _launch(L.load().mx_nhwc_to_nchw(L.current_stream(), d_x.data_ptr(), buf.data_ptr(), L.torch_dtype_code(dtype), B, Cc, HW, ld), f"nhwc_to_nchw {case}")
    _same(view[:B * Cc], want.reshape(B * Cc, HW), f"nhwc_to_nchw {case} {dtype}")
    _guards(buf, B * Cc, HW, f"nhwc_to_nchw {case}")


# ---- patchify, unpatchify, crop_pos ----

@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_IDS)
@pytest.mark.parametrize("case", K.PATCH_CASES, ids=str)
def test_patchify(cuda_device, case, dtype):
    dev, (B, Cc, H, W, ps) = cuda_device, case
    x = K.build_patchify(case, dtype)
    want = R.patchify_ref(x, ps)
    d_x = _in(x, dev)
    buf, view = _out(*want.shape, BF16, dev)
    _launch(L.load().mx_patchify(L.current_stream(), d_x.data_ptr(), L.torch_dtype_code(dtype), buf.data_ptr(), B, Cc, H, W, ps), f"patchify {case}")
    _same(view[:want.shape[0]], want, f"patchify {case} {dtype}")
    _guards(buf, *want.shape, f"patchify {case}")


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_IDS)
@pytest.mark.parametrize("case", K.PATCH_CASES, ids=str)
def test_unpatchify(cuda_device, case, dtype, pad):
    dev, (B, Cc, H, W, ps) = cuda_device, case
    tok = K.build_unpatchify(case, pad)                                           # NaN in the padding columns
    want = R.unpatchify_ref(tok, B, Cc, H, W, ps, dtype)
    d_tok = _in(tok, dev)
    buf, view = _out(B * Cc * H, W, dtype, dev)
    _launch(L.load().mx_unpatchify(L.current_stream(), d_tok.data_ptr(), buf.data_ptr(), L.torch_dtype_code(dtype), B, Cc, H, W, ps, tok.shape[1]),
            f"unpatchify {case}")
    _same(view[:B * Cc * H], want.reshape(B * Cc * H, W), f"unpatchify {case} {dtype} pad {pad}")
    _guards(buf, B * Cc * H, W, f"unpatchify {case}")


@pytest.mark.parametrize("case", K.CROP_CASES, ids=str)
def test_crop_pos(cuda_device, case):
    dev, (m, h, w, d) = cuda_device, case
    table = K.build_crop(case)
    want = R.crop_pos_ref(table, h, w)
    d_table = _in(table, dev)
    buf, view = _out(h * w, d, BF16, dev)
    _launch(L.load().mx_crop_pos(L.current_stream(), d_table.data_ptr(), buf.data_ptr(), m, h, w, d), f"crop_pos {case}")
    _same(view[:h * w], want, f"crop_pos {case}")
    _guards(buf, h * w, d, f"crop_pos {case}")


# ---- clip_embed, clip_pool ----

@pytest.mark.parametrize("with_pos", [1, 0], ids=["pos", "nopos"])
@pytest.mark.parametrize("H", K.EMBED_H)
def test_clip_embed(cuda_device, H, with_pos):
    dev = cuda_device
    ids, tok, pos = K.build_embed(H)
    want = R.clip_embed_ref(ids, tok, pos if with_pos else None)
    d_ids, d_tok, d_pos = _in(ids, dev), _in(tok, dev), _in(pos, dev)             # NaN behind both tables: an id past the vocabulary, a position by row
    rows = ids.numel()
    buf, view = _out(rows, H, BF16, dev)
    _launch(L.load().mx_clip_embed(L.current_stream(), d_ids.data_ptr(), d_tok.data_ptr(), d_pos.data_ptr() if with_pos else None, buf.data_ptr(), rows,
                                   K.EMBED_L, H, K.EMBED_VOCAB), f"clip_embed H {H}")
    _same(view[:rows], want, f"clip_embed H {H} pos {with_pos}")
    _guards(buf, rows, H, f"clip_embed H {H}")


@pytest.mark.parametrize("legacy", [0, 1], ids=["eos", "legacy"])
@pytest.mark.parametrize("H", K.POOL_H)
def test_clip_pool(cuda_device, H, legacy):
    dev = cuda_device
    ids = torch.tensor(K.POOL_IDS_LEGACY if legacy else K.POOL_IDS_EOS, dtype=torch.int32)
    eos = -1 if legacy else K.POOL_EOS
    x = K.build_pool(H)
    want = R.clip_pool_ref(ids, x, eos)
    d_ids, d_x = _in(ids, dev), _in(x, dev)
    buf, view = _out(K.POOL_B, H, BF16, dev)
    _launch(L.load().mx_clip_pool(L.current_stream(), d_ids.data_ptr(), d_x.data_ptr(), buf.data_ptr(), K.POOL_B, K.POOL_L, H, eos), f"clip_pool H {H}")
    _same(view[:K.POOL_B], want, f"clip_pool H {H} legacy {legacy}")
    _guards(buf, K.POOL_B, H, f"clip_pool H {H}")


# ---- the sinusoids ----

def _check_sinusoid(got, t, dim, what):
    """got bf16 [n, dim] on the CPU against the interval of (t, dim); prints the figures; returns the number of cells that admit two values"""
    c, e = R.sinusoid_ref(t, dim)
    lo, hi = R.interval(c, e)
    bad = R.outside(got, lo, hi)
    worst, raw = R.excess(got, c, e), float(((got.double() - c).abs() / e).max())
    off = int((R.bits(got) != R.bits(R.sinusoid_oracle_f32(t, dim).to(BF16))).sum())
    share = R.two_valued(lo, hi)
    print(f"{what}: worst |out - c| / e {raw:.1f} with the bf16 rounding, {worst:.3f} beyond half a bf16 step, two-valued cells {100 * share:.2f} %, "
          f"{off} of {got.numel()} cells differ from the fp32 oracle's rounding")
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} of {got.numel()} cells outside their interval, the first at {tuple(bad.nonzero()[0].tolist())}"
    return share * got.numel()


@pytest.mark.parametrize("dim", K.SINUS_DIMS)
def test_sinus_embed(cuda_device, dim):
    dev = cuda_device
    t = torch.tensor(K.TIMES, dtype=torch.float32)
    d_t = _in(t, dev)
    buf, view = _out(len(K.TIMES), dim, BF16, dev)
    _launch(L.load().mx_sinus_embed(L.current_stream(), d_t.data_ptr(), buf.data_ptr(), len(K.TIMES), dim), f"sinus_embed {dim}")
    _guards(buf, len(K.TIMES), dim, f"sinus_embed {dim}")
    assert _check_sinusoid(view[:len(K.TIMES)].cpu(), t, dim, f"sinus_embed dim {dim}") <= 0.15 * len(K.TIMES) * dim


@pytest.mark.parametrize("case", K.TIME_EMBED_CASES, ids=str)
def test_time_embed(cuda_device, case):
    dev, (B, d0, text_dim, da) = cuda_device, case
    t, text, ids = K.build_time_embed(case)
    addw = text_dim + 6 * da
    d_t, d_text, d_ids = _in(t, dev), _in(text, dev), _in(ids, dev)
    buf_t, view_t = _out(B, d0, BF16, dev)
    buf_a, view_a = _out(B, addw, BF16, dev)
    _launch(L.load().mx_time_embed(L.current_stream(), d_t.data_ptr(), d_text.data_ptr(), d_ids.data_ptr(), buf_t.data_ptr(), buf_a.data_ptr(), B, d0, text_dim, da),
            f"time_embed {case}")
    _guards(buf_t, B, d0, f"time_embed {case} tsin")
    _guards(buf_a, B, addw, f"time_embed {case} addin")
    addin = view_a[:B].cpu()
    _same(addin[:, :text_dim], text, f"time_embed {case}: the text_embeds part of addin")
    two = _check_sinusoid(view_t[:B].cpu(), t, d0, f"time_embed {case} tsin")
    two += _check_sinusoid(addin[:, text_dim:].reshape(B * 6, da), ids.reshape(-1), da, f"time_embed {case} addin")
    assert two <= 0.15 * B * (d0 + 6 * da)                      # over the launch's sinusoid cells: the test cannot go slack


# ---- softmax_rows ----

@pytest.mark.parametrize("c", K.SOFTMAX_CASES, ids=[c["name"] for c in K.SOFTMAX_CASES])
def test_softmax_rows(cuda_device, c):
    dev, Lc, pad, rows = cuda_device, c["L"], c["pad"], K.SOFTMAX_ROWS
    s = K.build_softmax(c["name"])
    p, r = R.softmax_ref(s)
    lo, hi = R.softmax_interval(p, r)
    buf = K.softmax_buffer(s, pad).to(dev)                                        # in place: the scores in a buffer of guard rows and guard columns
    _launch(L.load().mx_softmax_rows(L.current_stream(), buf.data_ptr(), rows, Lc, Lc + pad), c["name"])
    _guards(buf, rows, Lc, c["name"])
    got = buf[:rows, :Lc].cpu()
    bad = R.outside(got, lo, hi)
    worst, raw = R.excess(got, p, p * r), float(((got.double() - p).abs()[p > 0] / (p * r)[p > 0]).max())
    off = int((R.bits(got.contiguous()) != R.bits(torch.softmax(s.float(), dim=1).to(BF16))).sum())
    share = R.two_valued(lo, hi)
    print(f"softmax_rows {c['name']}: worst |out - p| / (p r) {raw:.1f} with the bf16 rounding, {worst:.3f} beyond half a bf16 step, two-valued cells {100 * share:.2f} %, "
          f"{off} of {got.numel()} cells differ from the fp32 oracle's rounding")
    assert share <= 0.15
    far = (s.double() - s.double().max(dim=1, keepdim=True).values) < -1.0e3
    assert int(far.sum()) >= Lc // 4 and torch.equal(R.bits(got.contiguous())[far], torch.zeros(int(far.sum()), dtype=torch.int16)), "1e4 below the maximum: +0"
    n = int(bad.sum())
    assert n == 0, f"{c['name']}: {n} of {got.numel()} cells outside their interval, the first at {tuple(bad.nonzero()[0].tolist())}"
