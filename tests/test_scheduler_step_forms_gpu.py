"""The forms of the one scheduler-step kernel (csrc/scheduler_step.hip) held against each other on the raw bits: a form with a feature that no row
uses must leave what the form without it leaves.  Plain, masked, multistep and gathered launches over the shapes at which each access path can go
wrong (tests/step_operands.py), Euler and flow, three dtypes, with and without guidance; every written tensor lies between guard elements.  What a
form computes is the business of test_ops_gpu.py, test_inpaint_gpu.py, test_sampler_gpu.py and test_pp_split_gpu.py; here only that they agree."""
import functools

import pytest
import torch

from step_operands import DTYPES, K, SLOTS, STEP_SHAPES, guards_intact, placed

pytestmark = pytest.mark.gpu

KINDS = {3: [2, 0, 1], 2: [1, 2]}                                             # permuted: row != kind
# H % n_slabs == 0 for one and two slabs; (1, 16, 6, 10): with two slabs a run of 30 elements, no whole number of 16-byte vectors
ROWS_SHAPES = [pytest.param((2, 4, 8, 8), id="2x4x8x8"), pytest.param((3, 16, 16, 16), id="3x16x16x16"), pytest.param((1, 16, 6, 10), id="1x16x6x10")]
CASES = [pytest.mark.parametrize("g", [5.0, 0.0], ids=["g5", "g0"]), pytest.mark.parametrize("dtype", DTYPES),
         pytest.mark.parametrize("flow", [False, True], ids=["euler", "flow"])]


def cases(fn):
    for mark in CASES:
        fn = mark(fn)
    return fn


def raw(t):
    return t.contiguous().view(torch.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b))


@functools.lru_cache(maxsize=None)
def operands(shape, dtype, flow, g):
    """CPU operands of one case, made once and never written: pred, lat, sigma, sigma_next, (init, noise, mask), coef, a NaN history"""
    n, C, h, w = shape
    gen = torch.Generator().manual_seed(3000 * C + 10 * h + int(flow))
    pred = torch.randn((2 if g > 0 else 1) * n, C, h, w, generator=gen).to(dtype)
    lat = (torch.randn(n, C, h, w, generator=gen) * (1.0 if flow else 3.0)).to(dtype)
    sigma = torch.tensor([1.0, 0.7368, 0.3][:n] if flow else [14.6146, 3.1875, 0.9][:n])
    sigma_next = torch.tensor([0.9231, 0.5, 0.0][:n] if flow else [9.8123, 2.0625, 0.0][:n])
    init = torch.randn(K, C, h, w, generator=gen).to(dtype)
    noise = torch.randn(K, C, h, w, generator=gen).to(dtype)
    mask = torch.randint(0, 2, (K, h, w), generator=gen, dtype=torch.uint8) * torch.randint(1, 256, (K, h, w), generator=gen, dtype=torch.uint8)
    mask[0, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)
    coef = torch.tensor([(0.6713867, 0.5432129, -0.2145996), (1.0, -0.1977539, 0.0834961), (0.25, 1.125, -0.375)][:n], dtype=torch.float32)
    return pred, lat, sigma, sigma_next, (init, noise, mask), coef, torch.full((n, C, h, w), float("nan"))


def launch(step, pred, lat, offset, hist=None, slot=None, rows=None):
    """step(pred, latents, hist, inpaint) on fresh copies between guards -> (latents, hist) it leaves, on the CPU.  inpaint: (slot, init, noise, mask) on
    the device or None.  Checked: in place, the guards of the latents and the history, the prediction unchanged."""
    pbuf, pv = placed(pred, offset)
    lbuf, lv = placed(lat, offset)
    hbuf, hv = placed(hist, offset) if hist is not None else (None, None)
    held = [] if rows is None else [placed(torch.tensor(slot, dtype=torch.int32), 0)] + [placed(t, offset) for t in rows]
    got = step(pv, lv, hv, tuple(v for _b, v in held) or None)
    torch.cuda.synchronize()
    assert got.data_ptr() == lv.data_ptr() and guards_intact(lbuf, lv) and torch.equal(pv.cpu(), pred)
    assert hist is None or guards_intact(hbuf, hv)
    return lv.cpu(), None if hist is None else hv.cpu()


def entries(flow, sigma, sigma_next, g, kind=None, coef=None):
    """the public entries as step(pred, latents, hist, inpaint) callables"""
    from sduss_amd import ops
    sg, sn = sigma.cuda(), sigma_next.cuda()
    ms = None if kind is None else (torch.tensor(kind, dtype=torch.int32).cuda(), coef.cuda())
    return dict(
        plain=lambda p, l, h, r: (ops.cfg_flow_step_ if flow else ops.cfg_euler_step_)(p, l, sg, sn, g),
        masked=lambda p, l, h, r: (ops.cfg_flow_step_masked_ if flow else ops.cfg_euler_step_masked_)(p, l, sg, sn, g, *(r or ())),
        multistep=lambda p, l, h, r: ops.cfg_multistep_step_(p, l, sg, sn, g, *ms, h, flow, *(r or ())),
        selected=lambda p, l, h, r: ops.cfg_step_(p, l, sg, sn, g, flow, inpaint=r, multistep=None if h is None else (*ms, h)))


@functools.lru_cache(maxsize=None)
def plain_step(shape, offset, dtype, flow, g):
    """what the plain entry leaves: the reference of every identity below, computed once per case"""
    pred, lat, sigma, sigma_next, *_ = operands(shape, dtype, flow, g)
    out, _h = launch(entries(flow, sigma, sigma_next, g)["plain"], pred, lat, offset)
    assert not same(out, lat)
    return out


@pytest.mark.parametrize("shape,offset", STEP_SHAPES)
@cases
def test_masked_without_inpainting_rows_is_plain(cuda_device, flow, dtype, shape, offset, g):
    pred, lat, sigma, sigma_next, rows, _coef, _nan = operands(shape, dtype, flow, g)
    masked = entries(flow, sigma, sigma_next, g)["masked"]
    want = plain_step(shape, offset, dtype, flow, g)
    assert same(launch(masked, pred, lat, offset)[0], want)                                             # k = 0
    assert same(launch(masked, pred, lat, offset, slot=[-1] * shape[0], rows=rows)[0], want)            # rows given, no slot points at them


@pytest.mark.parametrize("shape,offset", STEP_SHAPES)
@cases
def test_multistep_with_every_kind_euler_is_plain_or_masked(cuda_device, flow, dtype, shape, offset, g):
    pred, lat, sigma, sigma_next, rows, coef, nan = operands(shape, dtype, flow, g)
    n = shape[0]
    e = entries(flow, sigma, sigma_next, g, [0] * n, coef)
    got, hist = launch(e["multistep"], pred, lat, offset, hist=nan)
    assert same(got, plain_step(shape, offset, dtype, flow, g)) and same(hist, nan)                     # the history: neither read nor written
    masked, _h = launch(e["masked"], pred, lat, offset, slot=SLOTS[n], rows=rows)
    assert not same(masked, plain_step(shape, offset, dtype, flow, g))
    got, hist = launch(e["multistep"], pred, lat, offset, hist=nan, slot=SLOTS[n], rows=rows)
    assert same(got, masked) and same(hist, nan)


def gather_layout(pred, n, n_slabs):
    """[2n | n, C, H, W] -> [2 n_slabs | n_slabs, n, C, H / n_slabs, W]: slot k the unconditional rows of slab k, slot n_slabs + k the conditional"""
    hs = pred.shape[2] // n_slabs
    return torch.stack([pred[b * n:(b + 1) * n, :, k * hs:(k + 1) * hs] for b in range(pred.shape[0] // n) for k in range(n_slabs)]).contiguous()


@pytest.mark.parametrize("n_slabs", [1, 2], ids=["1slab", "2slabs"])
@pytest.mark.parametrize("shape", ROWS_SHAPES)
@cases
def test_rows_are_plain_on_the_gather_layout(cuda_device, flow, dtype, shape, n_slabs, g):
    from sduss_amd import ops
    pred, lat, sigma, sigma_next, *_ = operands(shape, dtype, flow, g)
    gathered = gather_layout(pred, shape[0], n_slabs)
    assert gathered.numel() == pred.numel() and (n_slabs > 1 or torch.equal(gathered.view(pred.shape), pred))
    fn = ops.cfg_flow_step_rows_ if flow else ops.cfg_euler_step_rows_
    got, _h = launch(lambda p, l, h, r: fn(p, l, sigma.cuda(), sigma_next.cuda(), g, n_slabs), gathered, lat, 0)
    assert same(got, plain_step(shape, 0, dtype, flow, g))
    both, _h = launch(lambda p, l, h, r: ops.cfg_step_rows_(p, l, sigma.cuda(), sigma_next.cuda(), g, n_slabs, flow), gathered, lat, 0)
    assert same(both, got)


@pytest.mark.parametrize("shape,offset", STEP_SHAPES)
@cases
def test_cfg_step_selects_the_entry(cuda_device, flow, dtype, shape, offset, g):
    """ops.cfg_step_ with each combination of inpaint / multistep against the entry it stands for, on rows that use the feature"""
    pred, lat, sigma, sigma_next, rows, coef, _nan = operands(shape, dtype, flow, g)
    n = shape[0]
    kind = [2 if k == 1 else k for k in KINDS[n]] if flow else KINDS[n]                                 # (DPM-Solver++ 2M is no flow sampler)
    e = entries(flow, sigma, sigma_next, g, kind, coef)
    hist0 = torch.randn(shape, generator=torch.Generator().manual_seed(7)) * 2.0
    for entry, hist, inpaint in (("plain", None, {}), ("masked", None, dict(slot=SLOTS[n], rows=rows)),
                                 ("multistep", hist0, {}), ("multistep", hist0, dict(slot=SLOTS[n], rows=rows))):
        want, want_hist = launch(e[entry], pred, lat, offset, hist=hist, **inpaint)
        got, got_hist = launch(e["selected"], pred, lat, offset, hist=hist, **inpaint)
        assert same(got, want) and not same(got, lat), (entry, bool(inpaint))
        assert hist is None or (same(got_hist, want_hist) and not same(got_hist, hist0)), (entry, bool(inpaint))
