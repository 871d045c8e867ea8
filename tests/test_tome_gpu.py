"""Token merging on the GPU: the four launches of tome.hip against tests/tome_ref.py in fp64, and MxUNet.enable_tome on UNetConfig.tiny() against the
reference forward.

Match.  gamma = (C + 4) 2^-24 bounds the fp32 accumulation of a dot product of unit vectors and of the two squared norms.  The argmax is discrete, so the
test states properties over every row: the destination chosen scores within 2 gamma of the fp64 maximum, and node_max is within 2 gamma + 2^-22 of it.
Select is integer work on the device's own node_max: the tables equal the reference's exactly.  Merge / unmerge: one bf16 rounding of an fp32 result,
|err| <= 2^-8 |want| + 2^-8 s with s = (C + 16) 2^-16 max|summand| (i.e. (C + 16) 2^-24 of the largest summand: the fp32 error of the mean, the
variance and the sum of up to 1 + count rows, which matters only where the result cancels towards zero)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tome_ref
from oracle import sdxl_unet_ref as ref  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

# one k-chunk and one dst tile; Nsrc = 108, Ndst = 36: ragged source and dst tiles; non-square with the widest rows; a real level
SHAPES = [(2, 8, 8, 64), (2, 12, 12, 640), (1, 16, 24, 1280), (2, 32, 32, 1280)]


@pytest.fixture(scope="module")
def cases(cuda_device):
    """per shape: x (bf16, with an all-zero source row, an all-zero destination row, a duplicated destination and a source that is twice that
    destination), the fp64 scores and the reference tables at ratio 0.5 -- computed once"""
    out = {}
    for B, h, w, Cc in SHAPES:
        g = torch.Generator().manual_seed(h * 1000 + w + Cc)
        x = (torch.randn(B, h * w, Cc, generator=g) + 0.25 * torch.randn(B, 1, Cc, generator=g)).bfloat16()
        dst, src = tome_ref.sets(h, w, 2, 2)
        x[0, src[5]] = 0
        x[0, dst[2]] = 0
        x[0, dst[3]] = x[0, dst[1]]
        x[0, src[7]] = x[0, dst[1]] * 2
        s = tome_ref.scores(x, h, w, 2, 2)
        r = (h * w) // 2
        tables = tome_ref.select(*tome_ref.match(x, h, w, 2, 2), h, w, 2, 2, r)
        out[(B, h, w, Cc)] = dict(x=x, xd=x.cuda(), s=s, r=r, tables=tables)
    return out


def _dev_tables(tables, h, w, r):
    from sduss_amd import ops
    return ops.TomeTables(*(t.cuda().contiguous() for t in tables), h, w, 2, 2, r)


@pytest.mark.parametrize("B,h,w,Cc", SHAPES)
def test_match_properties(cases, B, h, w, Cc):
    from sduss_amd import ops
    c = cases[(B, h, w, Cc)]
    node_max, node_idx = (t.cpu() for t in ops.tome_match(c["xd"], h, w))
    s, gamma = c["s"], (Cc + 4) * 2.0 ** -24
    max64 = s.max(dim=-1).values
    assert node_idx.min() >= 0 and node_idx.max() < s.shape[-1]
    chosen = s.gather(-1, node_idx.long()[..., None])[..., 0]
    print(f"{B}x{h}x{w}x{Cc}: chosen score short of the maximum by {(max64 - chosen).max().item():.3e}, |node_max - max| {(node_max.double() - max64).abs().max().item():.3e}, gamma {gamma:.3e}")
    assert (chosen >= max64 - 2 * gamma).all()
    assert ((node_max.double() - max64).abs() <= 2 * gamma + 2.0 ** -22).all()
    assert node_max[0, 5] == 0 and node_idx[0, 5] == 0, "a zero source row scores 0 against everything: the lowest ordinal"
    assert node_idx[0, 7] == 1, "destinations 1 and 3 are the same row: the lower ordinal wins"


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("B,h,w,Cc,r", [s + ((s[1] * s[2]) // 2,) for s in SHAPES] + [(2, 8, 8, 64, 0), (2, 8, 8, 64, 48), (2, 12, 12, 640, 16)])
def test_select_tables(cases, B, h, w, Cc, r, ties):
    from sduss_amd import ops
    node_max, node_idx = ops.tome_match(cases[(B, h, w, Cc)]["xd"], h, w)
    if ties:                                     # few distinct values: ties everywhere, the r-th value included
        node_max = (node_max * 16).round() / 16
    t = ops.tome_select(node_max, node_idx, h, w, r)
    nm, n_unm = node_max.cpu(), node_max.shape[1] - r
    src = tome_ref.sets(h, w, 2, 2)[1]
    for b in range(B):
        merged = t.row_of[b].cpu()[src] >= n_unm
        assert merged.sum().item() == r
        if 0 < r < len(src):
            kth = nm[b].sort(descending=True).values[r - 1]
            assert merged[nm[b] > kth].all() and not merged[nm[b] < kth].any()
            eq = merged[nm[b] == kth].int()
            assert (eq[1:] <= eq[:-1]).all(), "equal values are taken in ascending source order"
    for got, want, name in zip(t[:4], tome_ref.select(nm, node_idx.cpu(), h, w, 2, 2, r), ops.TomeTables._fields):
        assert torch.equal(got.cpu(), want), name


@pytest.mark.parametrize("eps", [None, 1e-5])
@pytest.mark.parametrize("B,h,w,Cc", SHAPES)
def test_merge_against_fp64(cases, B, h, w, Cc, eps):
    from sduss_amd import ops
    c = cases[(B, h, w, Cc)]
    want = tome_ref.merge(c["x"], c["tables"], h, w, 2, 2, eps)
    got = ops.tome_merge(c["xd"], _dev_tables(c["tables"], h, w, c["r"]), eps).cpu().double()
    big = c["x"].double().abs().max() if eps is None else torch.nn.functional.layer_norm(c["x"].double(), (Cc,), eps=eps).abs().max()
    bound = 2.0 ** -8 * want.abs() + (Cc + 16) * 2.0 ** -24 * big
    print(f"{B}x{h}x{w}x{Cc} eps={eps}: max |err| {(got - want).abs().max().item():.3e}, worst excess over the bound {((got - want).abs() - bound).max().item():.3e}")
    assert got.shape == want.shape and ((got - want).abs() <= bound).all()


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("B,h,w,Cc", SHAPES)
def test_unmerge_against_fp64(cases, B, h, w, Cc, residual):
    from sduss_amd import ops
    c = cases[(B, h, w, Cc)]
    g = torch.Generator().manual_seed(7)
    o = torch.randn(B, h * w - c["r"], Cc, generator=g).bfloat16()
    res = torch.randn(B, h * w, Cc, generator=g).bfloat16() if residual else None
    got = ops.tome_unmerge(o.cuda(), _dev_tables(c["tables"], h, w, c["r"]), None if res is None else res.cuda()).cpu()
    want = tome_ref.unmerge(o, c["tables"], res)
    if res is None:
        assert torch.equal(got.double(), want), "the plain unmerge moves rows"
    else:
        assert ((got.double() - want).abs() <= 2.0 ** -8 * want.abs() + 2.0 ** -24 * (8 + want.abs())).all()


TOME = dict(ratio=0.5, sx=2, sy=2, max_downsample=4)
HW, BATCH = 64, 2             # attention levels 32 x 32 (1024 -> 512 rows, C = 128) and 16 x 16 (256 -> 128 rows, C = 256); on the CPU: e_bf16 0.034, moved 0.14


@pytest.fixture(scope="module")
def tiny(cuda_device):
    from sduss_amd.config import UNetConfig
    from sduss_amd.unet import MxUNet
    ocfg, P = ref.UNetConfig.tiny(), ref.init_params(ref.UNetConfig.tiny())
    cpu = ref.make_inputs(ocfg, BATCH, HW, seed=HW)
    return dict(ocfg=ocfg, P=P, net=MxUNet(UNetConfig.tiny(), P, device="cuda:0"), cpu=cpu)


def _dev(inputs):
    s, t, e, te, ti = inputs
    return s.cuda().to(torch.bfloat16), t.cuda(), e.cuda().to(torch.bfloat16), te.cuda(), ti.cuda()


def test_forward_identity_and_reference(tiny):
    """ratio 0 and disable_tome: the plain forward, bit for bit.  Ratio 0.5: both matching decisions are discrete, so the yardstick is the same graph in
    stock bf16 on the CPU: the HIP forward may be twice as far from the fp32 reference as that (a flipped match moves a whole token; it is no
    rounding).  Measured on MI355X (profiles/tome.txt): HIP 0.02978, stock bf16 0.03484, the plain fp32 forward 0.14106 away."""
    net, dev, P, ocfg, cpu = tiny["net"], _dev(tiny["cpu"]), tiny["P"], tiny["ocfg"], tiny["cpu"]
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()      # noqa: E731
    plain = net.forward_one(*dev)
    net.enable_tome(ratio=0)
    assert torch.equal(net.forward_one(*dev), plain), "enable_tome(ratio=0) must be the plain forward, bit for bit"
    net.enable_tome(**TOME)
    got = net.forward_one(*dev).cpu()
    net.disable_tome()
    assert torch.equal(net.forward_one(*dev), plain), "after disable_tome the forward must be the plain forward"
    want = tome_ref.unet_forward(P, ocfg, *cpu, tome=TOME)
    e_bf16 = rel(tome_ref.unet_forward(P, ocfg, *cpu, tome=TOME, dtype=torch.bfloat16), want)
    moved = rel(tome_ref.unet_forward(P, ocfg, *cpu), want)
    e_hip = rel(got, want)
    print(f"ToMe forward: rel L2 to the fp32 reference: HIP {e_hip:.5f}, stock bf16 {e_bf16:.5f}; the plain fp32 forward lies {moved:.5f} away")
    assert e_bf16 < 0.5 * moved, "the yardstick's own error hides what token merging changes: the comparison shows nothing"
    assert e_hip <= 2 * e_bf16


def test_refusals(tiny):
    from sduss_amd import lib
    from sduss_amd.block_cache import BlockSkipCache
    Always = type("Always", (), {"predict": lambda self, f: np.ones(len(f))})
    net, dev = tiny["net"], _dev(tiny["cpu"])
    pp = [net._handle] + [0 if a in (C.c_int, C.c_size_t) else None for a in lib.SYMBOLS["mx_unet_forward_pp"][1][1:]]
    two = [tiny["cpu"][0][:1].cuda().to(torch.bfloat16), torch.zeros(1, 4, 16, 16, dtype=torch.bfloat16, device="cuda")]
    net.enable_tome(**TOME)
    with pytest.raises(lib.MxError, match="ToMe"):
        net.forward_one_cached(BlockSkipCache(Always()), *dev, batch_key=3)
    assert net._lib.mx_unet_forward_pp(*pp) != 0 and b"ToMe" in net._lib.mx_last_error()
    with pytest.raises(lib.MxError, match="ToMe"):
        net.forward_mixed(two, *dev[1:])
    net.disable_tome()
    assert net._lib.mx_unet_forward_pp(*pp) != 0 and b"ToMe" not in net._lib.mx_last_error()       # (null operands: its own complaint)
