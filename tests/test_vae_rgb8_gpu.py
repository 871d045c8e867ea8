"""The 8-bit image path on the GPU: mx_conv3x3_rgb8 (csrc/conv_rgb8.hip) on its own, mx_vae_decode_rgb8 at the plan level and post_inference's
output types.

The operator is checked two ways.  EXACT: inputs whose accumulator is exact in any summation order, so every byte must equal the header's formula
evaluated in fp32 by torch on the CPU -- y = acc + bias, t = y * 0.5 + 0.5, clamp to [0, 1] with NaN -> 0, round half to even of 255 t.  BOUNDED:
random bf16 operands; with the fp64 accumulator and its bound e from kernel_ref.conv_acc (+ 2^-24 |ref + bias| for the bias add) every byte must lie
in [ceil(255 clamp((ref - e) / 2 + 0.5) - 0.5 - d), floor(255 clamp((ref + e) / 2 + 0.5) + 0.5 + d)], d = 1e-4 levels for the three fp32 epilogue
operations (each at most 2^-24 relative on a value <= 255: 3 x 255 x 2^-24 = 4.6e-5).  Outputs sit between guard bytes that must come back unchanged,
inputs carry NaN rows behind them, weight row 3 and bias entry 3 (padding, never stored) are NaN, and every case runs twice into differently
pre-filled buffers and must return equal bytes."""
import math
from dataclasses import replace
from types import SimpleNamespace

import pytest
import torch

import kernel_ref as R

pytestmark = pytest.mark.gpu

from oracle import vae_ref as ref  # noqa: E402  (checker only)

GUARD = 64                 # guard bytes before and after an output (a multiple of 4: the output keeps its alignment)
GUARD_BYTE = 0x5A
DELTA = 1e-4               # levels: the three fp32 epilogue operations

# shape -> what it exercises
SHAPES = [
    pytest.param(1, 4, 16, 64, id="B1-H4-W16-Cin64"),        # one tile, one chunk
    pytest.param(2, 5, 17, 128, id="B2-H5-W17-Cin128"),      # ragged tiles both ways, byte stores, prefetch across chunks, tiles and images
    pytest.param(1, 8, 24, 128, id="B1-H8-W24-Cin128"),      # vector stores with a half-full right tile
    pytest.param(1, 256, 512, 64, id="B1-H256-W512-Cin64"),  # 2048 tiles: more than the launch starts workgroups
]


def formula_cpu(acc, bias):
    """the epilogue in fp32 on the CPU: acc [..., 3] fp32, bias [3] fp32 -> uint8"""
    assert acc.dtype == torch.float32 and bias.dtype == torch.float32 and acc.device.type == "cpu"
    y = acc + bias
    t = y * 0.5 + 0.5
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t).clamp(0.0, 1.0)
    return torch.round(t * 255.0).to(torch.uint8)           # torch.round: half to even


def launch_cap(cin):
    """workgroups one launch starts at most, by the launcher's rule: min(6, 160 KB / (LDS + 256)) per CU, whole groups of 8 CUs"""
    lds = ((3 * 9 * cin * 2 + 255) & ~255) + 6 * 18 * 144
    cus = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    return max(1, min(6, (160 * 1024) // (lds + 256))) * cus


def guarded_out(n, fill, offset=0):
    buf = torch.full((GUARD + offset + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    buf[GUARD + offset:GUARD + offset + n] = fill
    return buf


def guards_intact(buf, n, offset=0):
    return bool((buf[:GUARD + offset] == GUARD_BYTE).all()) and bool((buf[GUARD + offset + n:] == GUARD_BYTE).all())


def run_twice(x, w3, bias3, offset=0):
    """x [B, H, W, Cin] bf16, w3 [3, 9 Cin] bf16, bias3 [3] fp32 (CPU or GPU) -> uint8 [B, H, W, 3] on the CPU, after the guard, NaN and repeat checks"""
    from sduss_amd import ops
    B, H, W, Cin = x.shape
    xbuf, xv = R.nan_padded(x.reshape(-1, Cin).cuda(), Cin, extra_rows=R.GUARD_ROWS)
    w = torch.full((4, 9 * Cin), float("nan"), dtype=torch.bfloat16, device="cuda")
    w[:3] = w3.cuda()
    bias = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda")
    bias[:3] = bias3.cuda()
    n = B * H * W * 3
    outs = []
    for fill in (GUARD_BYTE, 0xA5):
        buf = guarded_out(n, fill, offset)
        view = buf[GUARD + offset:GUARD + offset + n].view(B, H, W, 3)
        got = ops.conv3x3_rgb8(xv.view(B, H, W, Cin), w, bias, out=view)
        torch.cuda.synchronize()
        assert got.data_ptr() == view.data_ptr()
        assert guards_intact(buf, n, offset), "guard bytes around the image changed"
        outs.append(view.cpu())
    assert torch.equal(outs[0], outs[1]), "two runs of the same launch returned different bytes"
    return outs[0]


def acc_on_device(x, w3):
    """kernel_ref.conv_acc on the GPU in fp64 -> (ref, bound) [B H W, 3] on the CPU"""
    acc, e = R.conv_acc(x.cuda(), w3.cuda(), x.shape[-1])
    return acc.cpu(), e.cpu()


# ---- 1. exact cases ----

def sweep_values():
    """>= 2^16 fp32 values: [-1.5, 1.5] densely, every rounding boundary of the 255 levels with its fp32 neighbours, and the special values"""
    dense = torch.linspace(-1.5, 1.5, 61441, dtype=torch.float64).float()
    k = torch.arange(255, dtype=torch.float64)
    mid = (((k + 0.5) / 255.0 - 0.5) * 2.0).float()                     # t * 255 = k + 0.5 up to rounding
    ulps = torch.arange(-8, 9, dtype=torch.int32)
    near = (mid.view(torch.int32)[:, None] + ulps[None, :]).view(torch.float32).reshape(-1)
    special = torch.tensor([math.inf, -math.inf, math.nan, 0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 1e-45, -1e-45, 3e38, -3e38, 1.0 - 2.0 ** -24, -1.0 + 2.0 ** -24],
                           dtype=torch.float32)
    v = torch.cat([dense, near, special])
    assert v.numel() >= 2 ** 16 and bool(torch.isinf(v).any()) and bool(torch.isnan(v).any())
    pad = (-v.numel()) % 3
    return torch.cat([v, torch.zeros(pad)])


def test_exact_bias_sweep(cuda_device):
    """(a) zero weights: the accumulator is 0 and y is the bias itself.  One [1, 2, 4, 64] image per bias triple, all into one guarded buffer."""
    from sduss_amd import lib as L
    l = L.load()
    vals = sweep_values()
    trip = vals.view(-1, 3)
    n_img, H, W, Cin = trip.shape[0], 2, 4, 64
    want = formula_cpu(torch.zeros_like(trip), trip)[:, None, :].expand(n_img, H * W, 3)
    assert int(want.min()) == 0 and int(want.max()) == 255 and want.unique().numel() == 256         # the sweep reaches every level
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-4, 5, (H * W, Cin), generator=g).to(torch.bfloat16)
    xbuf, xv = R.nan_padded(x.cuda(), Cin, extra_rows=R.GUARD_ROWS)
    w = torch.zeros((4, 9 * Cin), dtype=torch.bfloat16, device="cuda")
    w[3] = float("nan")
    bias = torch.full((n_img, 4), float("nan"), dtype=torch.float32, device="cuda")
    bias[:, :3] = trip.cuda()
    per = H * W * 3
    stream = L.current_stream()
    outs = []
    for fill in (GUARD_BYTE, 0xA5):
        buf = guarded_out(n_img * per, fill)
        xp, wp, bp, op = xv.data_ptr(), w.data_ptr(), bias.data_ptr(), buf.data_ptr() + GUARD
        for i in range(n_img):
            if l.mx_conv3x3_rgb8(stream, xp, wp, bp + 16 * i, op + per * i, 1, H, W, Cin):
                raise AssertionError(l.mx_last_error().decode())
        torch.cuda.synchronize()
        assert guards_intact(buf, n_img * per)
        outs.append(buf[GUARD:GUARD + n_img * per].view(n_img, H * W, 3).cpu())
    assert torch.equal(outs[0], outs[1])
    bad = (outs[0] != want).any(dim=1)
    assert not bool(bad.any()), f"{int(bad.sum())} bias values quantised wrongly, first: {trip[bad][:4].tolist()} -> {outs[0][bad][:4, 0].tolist()}"


def exact_operands(B, H, W, Cin):
    """(b) integer activations in [-4, 4]; weights multiples of 2^-6 with |w| <= 1/8 (one in eight non-zero, so that the sums stay near the interior);
    bias multiples of 2^-6: every product and every partial sum is a multiple of 2^-6 below 2^10 in magnitude, exact in fp32 in any order"""
    g = torch.Generator().manual_seed(1000 * H + W + Cin)
    x = torch.randint(-4, 5, (B, H, W, Cin), generator=g).to(torch.bfloat16)
    w = torch.randint(-8, 9, (3, 9 * Cin), generator=g).float() / 64.0
    w = (w * (torch.rand(3, 9 * Cin, generator=g) < 0.125)).to(torch.bfloat16)
    bias = torch.tensor([-0.25, 0.0, 0.171875])
    return x, w, bias


@pytest.mark.parametrize("B,H,W,Cin", SHAPES)
def test_exact_small_integers(cuda_device, B, H, W, Cin):
    x, w, bias = exact_operands(B, H, W, Cin)
    acc, _ = acc_on_device(x, w)
    assert bool((acc * 64 == (acc * 64).round()).all()) and float(acc.abs().max()) < 1024          # exact in fp32
    want = formula_cpu(acc.float(), bias).view(B, H, W, 3)
    # the span, on the reference alone: both saturated ends and the interior
    inside = ((want > 0) & (want < 255)).float().mean().item()
    assert bool((want == 0).any()) and bool((want == 255).any()) and inside >= 0.1 and want.unique().numel() >= 32, (inside, want.unique().numel())
    if H * W >= 256 * 512:
        tiles = B * ((H + 3) // 4) * ((W + 15) // 16)
        assert tiles > launch_cap(Cin), f"{tiles} tiles do not exceed the {launch_cap(Cin)} workgroups of a launch: the persistent loop is not tested"
    got = run_twice(x, w, bias)
    bad = got != want
    assert not bool(bad.any()), f"{int(bad.sum())} of {got.numel()} bytes differ from the fp32 formula (first at {bad.nonzero()[0].tolist()})"


def test_exact_unaligned_output(cuda_device):
    """W % 4 == 0 but the output starts one byte past a dword: the byte path, same bytes"""
    B, H, W, Cin = 1, 8, 24, 128
    x, w, bias = exact_operands(B, H, W, Cin)
    acc, _ = acc_on_device(x, w)
    want = formula_cpu(acc.float(), bias).view(B, H, W, 3)
    assert torch.equal(run_twice(x, w, bias, offset=1), want)


# ---- 1b. the two kernels of the shared staged body (csrc/conv_tile.h) against each other ----

def shared_body_operands(B, H, W, Cin):
    """integer activations in [-2, 2]; weights in {-1, 0, 1} x 2^-6, about half of them zero: every accumulator is k 2^-6 with a small integer k, exact
    in fp32 in any order AND a bf16 value, so the small-N kernel's bf16 output with a zero bias IS its accumulator.  The bias: one channel pushed to each
    clamp, one in the interior, each with a random fp32 offset (no multiple of 2^-6: the levels' rounding is exercised)."""
    g = torch.Generator().manual_seed(77 + 1000 * H + W + Cin)
    x = torch.randint(-2, 3, (B, H, W, Cin), generator=g).to(torch.bfloat16)
    w = torch.randint(-1, 2, (3, 9 * Cin), generator=g).float() / 64.0
    w = (w * (torch.rand(3, 9 * Cin, generator=g) < 0.75)).to(torch.bfloat16)          # zeros: 1/3 drawn + 1/4 of the rest = one half
    bias = torch.tensor([0.7, 0.0, -0.7]) + torch.randn(3, generator=g) * 0.05
    return x, w, bias


@pytest.mark.parametrize("B,H,W,Cin,offset", [
    pytest.param(1, 4, 16, 64, 0, id="B1-H4-W16-Cin64"),               # one tile, one chunk
    pytest.param(2, 5, 17, 128, 0, id="B2-H5-W17-Cin128"),             # ragged both ways, two chunks, prefetch across chunks, tiles and images, byte stores
    pytest.param(1, 8, 24, 128, 0, id="B1-H8-W24-Cin128"),             # dword stores with a half-full right tile
    pytest.param(2, 5, 17, 128, 1, id="B2-H5-W17-Cin128-unaligned"),   # the output one byte past a dword
])
def test_rgb8_is_the_small_n_accumulator_quantised(cuda_device, B, H, W, Cin, offset):
    """conv3x3_rgb8_kernel and conv3x3_small_n_kernel run one body: for the same operands the bytes of the first are the fp32 formula applied, on the CPU,
    to the accumulator the second returns (N = 4, rows 0..2 the rgb8 weights, row 3 and the bias zero; rgb8's own row 3 and bias[3] are NaN)."""
    from sduss_amd import ops
    x, w, bias = shared_body_operands(B, H, W, Cin)
    ref64, _ = acc_on_device(x, w)
    k = ref64 * 64
    assert bool((k == k.round()).all()) and float(k.abs().max()) < 256, float(k.abs().max())        # exact in any order, and a bf16 value
    assert float((w == 0).float().mean()) > 0.4
    w4 = torch.zeros((4, 9 * Cin), dtype=torch.bfloat16)
    w4[:3] = w
    acc = ops.conv3x3(x.cuda(), w4.cuda(), torch.zeros(4, device="cuda")).float().cpu()
    assert bool((acc[..., 3] == 0).all())
    assert torch.equal(acc[..., :3].reshape(-1, 3).double(), ref64), "the small-N kernel did not return the exact accumulator"
    want = formula_cpu(acc[..., :3].contiguous(), bias)
    inside = ((want > 0) & (want < 255)).float().mean().item()
    assert bool((want == 0).any()) and bool((want == 255).any()) and inside >= 0.1 and want.unique().numel() >= 32, (inside, want.unique().numel())
    got = run_twice(x, w, bias, offset=offset)
    bad = got != want
    assert not bool(bad.any()), f"{int(bad.sum())} of {got.numel()} bytes differ from the formula on the small-N accumulator (first at {bad.nonzero()[0].tolist()})"


# ---- 2. bounded cases ----

@pytest.mark.parametrize("B,H,W,Cin", SHAPES)
def test_bounded_random(cuda_device, B, H, W, Cin):
    g = torch.Generator().manual_seed(7 * H + W + Cin)
    x = torch.randn(B, H, W, Cin, generator=g).to(torch.bfloat16)
    # y ~ N(0, s^2) with P(y > 1) = P(y < -1) = 0.1: s = 1 / 1.2816
    w = (torch.randn(3, 9 * Cin, generator=g) * (0.78 / math.sqrt(9 * Cin))).to(torch.bfloat16)
    bias = torch.randn(3, generator=g) * 0.05
    acc, e = acc_on_device(x, w)
    v = acc + bias.double()
    e = e + R.U32 * v.abs()                                  # the fp32 add of the bias
    lo = torch.ceil(255.0 * ((v - e) / 2 + 0.5).clamp(0, 1) - 0.5 - DELTA).view(B, H, W, 3)
    hi = torch.floor(255.0 * ((v + e) / 2 + 0.5).clamp(0, 1) + 0.5 + DELTA).view(B, H, W, 3)
    assert bool((lo <= hi).all())
    sat0, sat1 = (hi == 0).float().mean().item(), (lo == 255).float().mean().item()
    print(f"rgb8 bounded B{B} H{H} W{W} Cin{Cin}: saturated low {sat0:.3f}, high {sat1:.3f}; intervals admitting more than one value: "
          f"{(hi > lo).float().mean().item():.5f}")
    assert 0.03 <= sat0 <= 0.25 and 0.03 <= sat1 <= 0.25                                           # "about a tenth" at each end
    if H * W >= 256 * 512:
        assert B * ((H + 3) // 4) * ((W + 15) // 16) > launch_cap(Cin)
    got = run_twice(x, w, bias).double()
    bad = ~((got >= lo) & (got <= hi))
    assert not bool(bad.any()), f"{int(bad.sum())} of {got.numel()} bytes outside their interval (first at {bad.nonzero()[0].tolist()})"


# ---- 4. plan level: the configs, seeds and latents of tests/test_vae_gpu.py ----

def _plan_case(name):
    from sduss_amd.vae import VAEConfig
    if name == "tiny-b2-16":
        return ref.VAEConfig.tiny(), VAEConfig.tiny(), (torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(16)) * 0.8).to(torch.bfloat16)
    if name == "tiny-b1-32":
        return ref.VAEConfig.tiny(), VAEConfig.tiny(), (torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(32)) * 0.8).to(torch.bfloat16)
    if name == "tiny-sd3":
        return (ref.VAEConfig.tiny_sd3(), replace(VAEConfig.sd3(), block_out_channels=(64, 64, 128), layers_per_block=1),
                (torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(8)) * 1.5).to(torch.bfloat16))
    assert name == "sdxl-widths-32"
    return ref.VAEConfig.sdxl(), VAEConfig.sdxl(), (torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(3)) * 0.8).to(torch.bfloat16)


def quantise(img01):
    """[n, 3, h, w] in [0, 1] -> uint8 [n, h, w, 3], as the host pass of the float path does"""
    return torch.round(img01.permute(0, 2, 3, 1) * 255.0).to(torch.uint8)


@pytest.mark.parametrize("name", ["tiny-b2-16", "tiny-b1-32", "tiny-sd3", "sdxl-widths-32"])
def test_decode_images(cuda_device, name):
    from sduss_amd.vae import MxVAEDecoder
    ocfg, cfg, lat = _plan_case(name)
    P = ref.init_params(ocfg)
    with torch.inference_mode():
        oracle = quantise(ref.postprocess(ref.decode(P, ocfg, lat.float())))
    vae = MxVAEDecoder(cfg, P, device="cuda:0")
    # first call of a fresh decoder: its workspace is exactly mx_vae_workspace_bytes, which must serve the 8-bit path as well
    got = vae.decode_images(lat.cuda())
    b, _c, h, w = lat.shape
    f = 2 ** (len(cfg.block_out_channels) - 1)
    assert got.shape == (b, f * h, f * w, 3) and got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous()      # (c)
    assert torch.equal(got, vae.decode_images(lat.cuda()))
    got = got.cpu().int()
    # (a) against the quantised float decode of the same build: one bf16 rounding of |y| <= 1 moves a level by at most 127.5 x 2^-8 < 0.5
    same = quantise((vae.decode(lat.cuda()).float().cpu() / 2 + 0.5).clamp(0, 1)).int()
    da = (got - same).abs()
    # (b) against the oracle: the 0.03-of-[0, 1] bound of test_post_inference_images (7.65 levels) plus the two roundings
    db = (got - oracle.int()).abs()
    print(f"decode_images {name}: vs own float decode max {int(da.max())} level(s), {float((da > 0).float().mean()):.4f} of the bytes differ; "
          f"vs oracle max {int(db.max())} levels")
    assert int(da.max()) <= 1
    assert int(db.max()) <= 8


# ---- 5. post_inference ----

def test_post_inference_output_types(cuda_device):
    from sduss_amd.vae import MxVAEDecoder, VAEConfig, post_inference
    ocfg = ref.VAEConfig.tiny()
    P = ref.init_params(ocfg)
    vae = MxVAEDecoder(VAEConfig.tiny(), P, device="cuda:0")

    def req(seed, hw):
        return SimpleNamespace(latents=(torch.randn(1, 4, hw, hw, generator=torch.Generator().manual_seed(seed)) * 0.8).to(torch.bfloat16).cuda())
    reqs = {"64": [req(0, 16), req(1, 16)], "128": [req(2, 32)], "256": []}          # (the tiny decoder has three levels: 4 x the latent size)
    lats = {res: torch.cat([r.latents for r in rs]) for res, rs in reqs.items() if rs}

    u8 = post_inference(vae, reqs, output_type="uint8")
    assert set(u8) == {"64", "128"}
    for res, lat in lats.items():
        n, px = lat.shape[0], int(res)
        assert u8[res].shape == (n, px, px, 3) and u8[res].dtype == torch.uint8 and u8[res].is_cuda
        assert torch.equal(u8[res], vae.decode_images(lat))

    pil = post_inference(vae, reqs, output_type="pil")
    assert set(pil) == {"64", "128"}
    # a second request through the same pinned buffer must not reach into the images already handed out
    post_inference(vae, {"64": [req(5, 16), req(6, 16)], "128": [req(7, 32)]}, output_type="pil")
    for res, imgs in pil.items():
        assert len(imgs) == lats[res].shape[0]
        for i, im in enumerate(imgs):
            assert im.mode == "RGB" and im.size == (int(res), int(res))
            assert im.tobytes() == u8[res][i].cpu().numpy().tobytes()

    pt = post_inference(vae, reqs)                          # the default: today's result, bit for bit
    pt2 = post_inference(vae, reqs, output_type="pt")
    for res, lat in lats.items():
        want = (vae.decode(lat) / 2 + 0.5).clamp(0, 1)
        assert pt[res].dtype == torch.float32 and pt[res].shape == (lat.shape[0], 3, int(res), int(res))
        assert torch.equal(pt[res], want) and torch.equal(pt2[res], want)
