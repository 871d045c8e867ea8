"""FreeU on the GPU: mx_freeu against diffusers' FFT form in fp64 (tests/freeu_ref.py) under a derived per-element bound, the grouped launch, and
MxUNet.enable_freeu on UNetConfig.tiny() against the fp32 oracle forward with apply_freeu at every concatenation.

The bound, per element (the style of tests/norm_ref.py):   |y - ref| <= 2^-8 |ref| + |s - 1| * 4 * n * 2^-24 * mean|x| over the plane
  2^-8 |ref|: the one rounding of the fp32 value to bf16 (half an ulp is at most 2^-8 of the value);
  the rest:   each of the four bins is a sum of H W products whose fp32 error is at most n * 2^-24 * sum|x|, scaled by |s - 1| / (H W).
Summation order (freeu.hip): a thread adds the <= wseg pixels of an item left to right, folds its items one after the other, and the 64 pixel lanes are
added in a balanced tree of 6 levels: the longest chain is n = wseg + items per lane + 6 additions, a function of H and W alone (8 at 2 x 2, 71 at
64 x 64), reported by mx_freeu_route."""
import ctypes as C

import numpy as np
import pytest
import torch

import freeu_ref
from oracle import sdxl_unet_ref as ref  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

# the issue's seven shapes at C in {64, 320}, B = 3 (all on 16-channel slabs, staged); then both sides of every switch of the route: 64 x 66 is read
# twice, the wide launches take 32- and 64-channel slabs, 66 x 9 at slab 64 is read twice
SHAPES = [(3, h, w, c) for h, w in ((2, 2), (2, 8), (3, 5), (4, 6), (24, 24), (32, 32), (64, 64)) for c in (64, 320)]
SHAPES += [(3, 64, 66, 64), (8, 4, 6, 1024), (8, 4, 6, 2048), (2, 66, 9, 8192)]


def _inputs(B, H, W, C, seed=0):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + seed)
    return (torch.randn(B, H, W, C, generator=g) + 0.5).bfloat16(), torch.randn(B, H, W, 64, generator=g).bfloat16()


def _bound(x, want, s, n):          # x, want: [B, H, W, C]
    return 2.0 ** -8 * want.abs() + abs(s - 1) * 4 * n * 2.0 ** -24 * x.double().abs().mean(dim=(1, 2), keepdim=True)


@pytest.mark.parametrize("s", [0.2, 0.9])
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_operator_against_fft_fp64(cuda_device, B, H, W, C, s):
    from sduss_amd import ops
    b = 1.4
    x, hid = _inputs(B, H, W, C)
    n = ops.freeu_route([(B, H, W)], C)[2][0]
    want = freeu_ref.fourier_filter(x.permute(0, 3, 1, 2), 1, s).permute(0, 2, 3, 1)
    bound = _bound(x, want, s, n)
    if H > 2:       # (H = 2: bin +1 IS bin -1, the Nyquist row)  the reference alone separates a wrong diagonal bin on this input
        wrong = freeu_ref.filter_wrong_diagonal(x.permute(0, 3, 1, 2), s).permute(0, 2, 3, 1)
        assert ((wrong - want).abs() > bound).any(), "the input does not tell (+1, -1) from (-1, -1)"
    hd = hid.cuda()
    got = ops.freeu(hd, x.cuda(), s, b).cpu().double()
    excess = ((got - want).abs() - bound).max().item()
    print(f"{B}x{H}x{W}x{C} s={s}: n = {n}, max |err| {(got - want).abs().max().item():.3e}, worst excess over the bound {excess:.3e}")
    assert excess <= 0
    assert torch.equal(hd.cpu()[..., :32], (hid[..., :32].float() * b).bfloat16()), "the scaled half is bf16(fp32(x) * b), bit for bit"
    assert torch.equal(hd.cpu()[..., 32:], hid[..., 32:]), "the other half is untouched"


def test_grouped_launch_keeps_every_problems_bits(cuda_device):
    from sduss_amd import ops
    xs, hs = zip(*(_inputs(B, H, W, 320, seed=1) for B, H, W in ((2, 24, 24), (1, 3, 5), (3, 32, 32))))
    single = [ops.freeu(h.cuda(), x.cuda(), 0.2, 1.4) for x, h in zip(xs, hs)]
    hd = [h.cuda() for h in hs]
    grouped = ops.freeu(hd, [x.cuda() for x in xs], 0.2, 1.4)
    for g, h in enumerate(hs):
        assert torch.equal(grouped[g], single[g]), f"problem {g}"
        assert torch.equal(hd[g].cpu()[..., :32], (h[..., :32].float() * 1.4).bfloat16()) and torch.equal(hd[g].cpu()[..., 32:], h[..., 32:])


def test_bits_do_not_depend_on_the_slab_or_the_batch(cuda_device):
    """C = 1024 at batch 1 / 8 / 16 runs on 16- / 32- / 64-channel slabs: sample 0 keeps its bits"""
    from sduss_amd import ops
    x = _inputs(16, 24, 24, 1024, seed=2)[0].cuda()
    assert [ops.freeu_route([(B, 24, 24)], 1024)[0] for B in (1, 8, 16)] == [16, 32, 64]
    one = ops.freeu(None, x[:1], 0.2, 1.0)
    assert torch.equal(ops.freeu(None, x[:8], 0.2, 1.0)[:1], one) and torch.equal(ops.freeu(None, x, 0.2, 1.0)[:1], one)


FREEU = (0.9, 0.2, 1.3, 1.4)


@pytest.fixture(scope="module")
def tiny(cuda_device):
    from sduss_amd.config import UNetConfig
    from sduss_amd.unet import MxUNet
    ocfg, P = ref.UNetConfig.tiny(), ref.init_params(ref.UNetConfig.tiny())
    net = MxUNet(UNetConfig.tiny(), P, device="cuda:0")
    cpu = {hw: ref.make_inputs(ocfg, b, hw, seed=hw) for hw, b in ((16, 2), (32, 1))}
    want = {hw: freeu_ref.unet_forward(P, ocfg, *c, freeu=FREEU) for hw, c in cpu.items()}
    return dict(ocfg=ocfg, P=P, net=net, cpu=cpu, want=want)


def _dev(inputs):
    s, t, e, te, ti = inputs
    return s.cuda().to(torch.bfloat16), t.cuda(), e.cuda().to(torch.bfloat16), te.cuda(), ti.cuda()


def _check(got, want, plain, what):        # the bounds of tests/test_unet_gpu.py::_check for this config
    got = got.float().cpu()
    scale, err = want.abs().max().item(), (got - want).abs().max().item()
    l2, moved = ((got - want).norm() / want.norm()).item(), (got - plain.float().cpu()).abs().max().item()
    print(f"{what}: max err {err:.4f} ({err / scale:.4f} of max), rel L2 {l2:.4f}; moved by {moved:.4f} against the plain forward")
    assert err <= 0.04 * scale and l2 <= 0.02, f"{what}: max err {err} vs scale {scale}, rel L2 {l2}"
    assert moved > 0.04 * scale, f"{what}: FreeU moved the output by {moved}, inside the tolerance {0.04 * scale}: the comparison shows nothing"


def test_forward_identity_and_oracle(tiny):
    net, dev = tiny["net"], _dev(tiny["cpu"][16])
    plain = net.forward_one(*dev)
    net.enable_freeu(1, 1, 1, 1)
    assert torch.equal(net.forward_one(*dev), plain), "enable_freeu(1, 1, 1, 1) must be the plain forward, bit for bit"
    net.enable_freeu(*FREEU)
    got = net.forward_one(*dev)
    net.disable_freeu()
    _check(got, tiny["want"][16], plain, "FreeU forward")
    assert torch.equal(net.forward_one(*dev), plain), "after disable_freeu the forward must be the plain forward"


def test_mixed_batch_agrees_with_its_groups(tiny):
    net, cpu = tiny["net"], tiny["cpu"]
    cat = [torch.cat([a, b]) for a, b in zip(cpu[16][1:], cpu[32][1:])]
    args = ([cpu[hw][0].cuda().to(torch.bfloat16) for hw in (16, 32)], cat[0].cuda(), cat[1].cuda().to(torch.bfloat16), cat[2].cuda(), cat[3].cuda())
    plain = net.forward_mixed(*args)
    net.enable_freeu(*FREEU)
    got = net.forward_mixed(*args)
    alone = [net.forward_one(*_dev(cpu[hw])) for hw in (16, 32)]
    net.disable_freeu()
    for g, hw in enumerate((16, 32)):
        _check(got[g], tiny["want"][hw], plain[g], f"mixed group {g}")
        l2a = ((got[g].float() - alone[g].float()).norm().cpu() / tiny["want"][hw].norm()).item()
        print(f"mixed group {g}: rel L2 to its own forward {l2a:.4f}")
        assert l2a <= 0.02, "the bound tests/test_grouped_gpu.py sets between a mixed batch and its per-resolution sequences"


def test_refusals(tiny):
    from sduss_amd import lib
    from sduss_amd.block_cache import BlockSkipCache
    Always = type("Always", (), {"predict": lambda self, f: np.ones(len(f))})
    net, dev = tiny["net"], _dev(tiny["cpu"][16])
    plain = net.forward_one(*dev)
    pp = [net._handle] + [0 if a in (C.c_int, C.c_size_t) else None for a in lib.SYMBOLS["mx_unet_forward_pp"][1][1:]]
    net.enable_freeu(*FREEU)
    with pytest.raises(lib.MxError, match="FreeU"):
        net.forward_one_cached(BlockSkipCache(Always()), *dev, batch_key=3)
    assert net._lib.mx_unet_forward_pp(*pp) != 0 and b"FreeU" in net._lib.mx_last_error()
    net.disable_freeu()
    assert torch.equal(net.forward_one_cached(BlockSkipCache(Always()), *dev, batch_key=3), plain), "the cached entry point serves again"
    assert net._lib.mx_unet_forward_pp(*pp) != 0 and b"FreeU" not in net._lib.mx_last_error()       # (null operands: its own complaint)
