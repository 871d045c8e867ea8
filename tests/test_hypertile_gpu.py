"""HyperTile on the GPU: mx_attention_window against fp64 per window (kernel_ref.attention_ref's per-element bound), its refusals, and
MxUNet.enable_hypertile on UNetConfig.tiny() against tests/hypertile_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import hypertile_ref
import kernel_ref as R
from oracle import sdxl_unet_ref as ref  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

# (B, H, gh, gw, wh, ww): resident 2 x 2 windows; resident 80 keys (ragged key tile and query rows, 3 windows across, odd heads); one 64-key tile;
# streamed 336 keys (5 tiles + 16, ragged query block); streamed ww = 32; streamed 1024 keys (the L = 4096 level's form); one window = the whole grid
CASES = [(2, 2, 32, 32, 16, 16), (1, 3, 10, 48, 5, 16), (1, 2, 8, 48, 4, 16), (1, 1, 42, 32, 21, 16), (1, 2, 24, 64, 12, 32), (1, 1, 64, 32, 32, 32),
         (1, 1, 16, 32, 16, 32)]


def _operands(B, H, gh, gw, dev="cuda"):
    from sduss_amd import ops
    g = torch.Generator().manual_seed(gh * 1000 + gw * 10 + H)
    L, D = gh * gw, H * 64
    q = (torch.randn(B * L, D, generator=g) * ops.ATTN_QSCALE).bfloat16().to(dev)      # prescaled before its one rounding
    k, v = (torch.randn(B * L, D, generator=g).bfloat16().to(dev) for _ in range(2))
    ldvt = ops.vt_ld(L) + 8
    vt = torch.full((B, D, ldvt), float("nan"), dtype=torch.bfloat16, device=dev)
    vt[:, :, :ops.vt_ld(L)] = ops.pack_vt(v.reshape(B, L, D))
    return q, k, v, vt


@pytest.mark.parametrize("B,H,gh,gw,wh,ww", CASES)
def test_window_attention_against_fp64(cuda_device, B, H, gh, gw, wh, ww):
    from sduss_amd import ops
    L, D = gh * gw, H * 64
    q, k, v, vt = _operands(B, H, gh, gw)
    obuf, o = R.guarded(B * L, D, D + 4, torch.bfloat16, "cuda")
    ops.attention_window(q, k, vt, H, B, (gh, gw), (wh, ww), out=obuf)
    torch.cuda.synchronize()
    assert R.guard_violations(obuf, B * L, D) == 0, "the launch wrote outside O[:B*L, :H*64]"
    win = lambda t: hypertile_ref.to_windows(t.reshape(B, L, D), gh, gw, wh, ww)       # noqa: E731  [B windows, wh ww, D]
    qw, kw, vw, ow = win(q), win(k), win(v), win(o.contiguous())
    bad, worst = 0, 0.0
    for w in range(qw.shape[0]):
        for h in range(H):
            sl = slice(h * 64, h * 64 + 64)
            want, bound = R.attention_ref(qw[w, :, sl], kw[w, :, sl], vw[w, :, sl], 1.0)
            n, ratio = R.violations(ow[w, :, sl], want, bound)
            bad, worst = bad + n, max(worst, ratio)
    print(f"window {wh}x{ww} of {gh}x{gw}, B{B} H{H}: worst err / bound {worst:.3f}")
    assert bad == 0, f"{bad} elements outside their fp64 bound (worst err / bound {worst:.3g})"


@pytest.mark.parametrize("what,message", [("ww8", "multiple of 16"), ("gw", "divide the token grid"), ("null", "null operand"), ("misaligned", "16-byte aligned"),
                                          ("ldvt", "MX_VT_LD")])
def test_window_attention_refusals(cuda_device, what, message):
    from sduss_amd import lib
    l = lib.load()
    B, H, gh, gw = 1, 1, 16, 48
    q, k, _v, vt = _operands(B, H, gh, gw)
    o = torch.zeros(B * gh * gw + 1, 64, dtype=torch.bfloat16, device="cuda")
    before = o.clone()
    wh, ww = (8, 8) if what == "ww8" else (8, 32) if what == "gw" else (8, 16)
    rc = l.mx_attention_window(lib.current_stream(), None if what == "null" else q.data_ptr(), 64, k.data_ptr(), 64, vt.data_ptr(),
                               gh * gw - 16 if what == "ldvt" else vt.shape[2], 64 * vt.shape[2], o.data_ptr() + (8 if what == "misaligned" else 0), 64,
                               B, H, gh, gw, wh, ww)
    torch.cuda.synchronize()
    assert rc == 1 and message in l.mx_last_error().decode(), l.mx_last_error()
    assert torch.equal(o, before), "a refused call launched"


HW, BATCH = 64, 2             # attention levels 32 x 32 (tile 128: 2 x 2 windows of 16 x 16) and 16 x 16 (one window: plain)


@pytest.fixture(scope="module")
def tiny(cuda_device):
    from sduss_amd.config import UNetConfig
    from sduss_amd.unet import MxUNet
    ocfg, P = ref.UNetConfig.tiny(), ref.init_params(ref.UNetConfig.tiny())
    cpu = ref.make_inputs(ocfg, BATCH, HW, seed=HW)
    s, t, e, te, ti = cpu
    dev = (s.cuda().to(torch.bfloat16), t.cuda(), e.cuda().to(torch.bfloat16), te.cuda(), ti.cuda())
    return dict(ocfg=ocfg, P=P, net=MxUNet(UNetConfig.tiny(), P, device="cuda:0"), cpu=cpu, dev=dev)


def test_forward_identity_and_reference(tiny):
    """tile_size 0, disable_hypertile and a tile that covers every level: the plain forward, bit for bit.  On: no discrete decision is taken, so the
    yardstick is the forward tests' own (tests/test_unet_gpu.py _calibrated_all_rows): per sample, rel L2 to the fp32 reference <= 1.5 x that of the
    same graph in stock bf16 -- provided that error is below half of what HyperTile changes."""
    net, dev, P, ocfg, cpu = tiny["net"], tiny["dev"], tiny["P"], tiny["ocfg"], tiny["cpu"]
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()      # noqa: E731
    plain = net.forward_one(*dev)
    for tile in (0, 256):
        net.enable_hypertile(tile_size=tile)
        assert net.hypertile_windows(HW, HW) == [None, None]
        assert torch.equal(net.forward_one(*dev), plain), f"enable_hypertile(tile_size={tile}) must be the plain forward, bit for bit"
    net.enable_hypertile(tile_size=128)
    assert net.hypertile_windows(HW, HW) == [(32, 32, 16, 16), None]
    got = net.forward_one(*dev).cpu()
    net.disable_hypertile()
    assert torch.equal(net.forward_one(*dev), plain), "after disable_hypertile the forward must be the plain forward"
    want = hypertile_ref.unet_forward(P, ocfg, *cpu, tile_size=128)
    b16 = hypertile_ref.unet_forward(P, ocfg, *cpu, tile_size=128, dtype=torch.bfloat16)
    moved = hypertile_ref.unet_forward(P, ocfg, *cpu)
    for r in range(BATCH):
        e_hip, e_bf16, d = rel(got[r], want[r]), rel(b16[r], want[r]), rel(moved[r], want[r])
        print(f"HyperTile forward row {r}: rel L2 to the fp32 reference: HIP {e_hip:.5f}, stock bf16 {e_bf16:.5f}; the plain fp32 forward lies {d:.5f} away")
        assert e_bf16 < 0.5 * d, "the yardstick's own error hides what HyperTile changes: the comparison shows nothing"
        assert e_hip <= 1.5 * e_bf16


def test_refusals(tiny):
    from sduss_amd import lib
    from sduss_amd.block_cache import BlockSkipCache
    Always = type("Always", (), {"predict": lambda self, f: np.ones(len(f))})
    net, dev = tiny["net"], tiny["dev"]
    pp = [net._handle] + [0 if a in (C.c_int, C.c_size_t) else None for a in lib.SYMBOLS["mx_unet_forward_pp"][1][1:]]
    two = [tiny["cpu"][0][:1].cuda().to(torch.bfloat16), torch.zeros(1, 4, 16, 16, dtype=torch.bfloat16, device="cuda")]
    net.enable_hypertile(tile_size=128)
    with pytest.raises(lib.MxError, match="HyperTile"):
        net.forward_one_cached(BlockSkipCache(Always()), *dev, batch_key=3)
    assert net._lib.mx_unet_forward_pp(*pp) != 0 and b"HyperTile" in net._lib.mx_last_error()
    with pytest.raises(lib.MxError, match="HyperTile"):
        net.forward_mixed(two, *dev[1:])
    net.enable_tome(ratio=0.5)
    with pytest.raises(lib.MxError, match="HyperTile"):
        net.forward_one(*dev)
    net.disable_hypertile()
    net.forward_one(*dev)                                                                           # ToMe alone is served
    net.disable_tome()
    assert net._lib.mx_unet_forward_pp(*pp) != 0 and b"HyperTile" not in net._lib.mx_last_error()   # (null operands: its own complaint)
