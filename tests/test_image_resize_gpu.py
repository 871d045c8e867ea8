"""The image resize on the GPU (csrc/image_resize.hip): mx_resize_u8 against the numpy restatement of Pillow's resampler (tests/resize_ref.py) and
against Pillow's own bytes (tests/golden/resize_pillow.npz), compared with ``==``; then Denoiser.start_from_image / start_inpaint with ``size=`` on
the tiny configs of tests/test_vae_encode_gpu.py / tests/test_inpaint_gpu.py.

Every case runs with two different images (B = 2), with one and with three channels, and twice: into an output that starts on a 4-byte
boundary from an input that does (dword stores where a row allows them), and into one that starts one byte after a boundary from an input three
bytes after one (byte stores, dwords put together at the input's ends).  The two runs must give equal bytes, and the 0xA5 bytes either side of the
output must stay as they are.

| case (H x W)            | what it is there for                                              |
| 37x53 -> 16x24          | non-integer down, odd widths, rows that start at any alignment    |
| 9x11 -> 40x44           | up                                                                |
| 64x48 -> 64x40          | the vertical pass skipped                                         |
| 128x96 -> 17x96         | the horizontal pass skipped                                       |
| 7x5 -> 7x5              | a copy                                                            |
| 400x24 -> 8x24          | 301 vertical taps: more than one chunk of input rows              |
| 20x300 -> 24x200        | more than one column tile (600 output bytes a row, 128 a tile)    |
| 33x65 -> 32x64          | a scale just above 1                                              |
"""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import resize_ref as R
import vae_encode_ref as E

pytestmark = pytest.mark.gpu

from oracle import vae_ref  # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
FILL = 0xA5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "resize_pillow.npz"))


def run_placed(x: np.ndarray, size, resample: str, src_off: int, dst_off: int) -> np.ndarray:
    """mx_resize_u8 through the C ABI: the input ``src_off`` bytes and the output ``dst_off`` bytes after a 4-byte boundary, the output inside a
    buffer of guard bytes, which are checked"""
    from sduss_amd import lib
    l = lib.load()
    b, ih, iw = x.shape[:3]
    c = 3 if x.ndim == 4 else 1
    oh, ow = size
    n_out = b * oh * ow * c
    src_buf = torch.zeros(4 + x.size, dtype=torch.uint8, device="cuda")
    assert src_buf.data_ptr() % 4 == 0
    src = src_buf[src_off:src_off + x.size]
    src.copy_(torch.from_numpy(np.array(x).reshape(-1)))
    dst_buf = torch.full((GUARD + 4 + n_out + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    lo = GUARD + dst_off
    plan = l.mx_resize_create(ih, iw, oh, ow, R.FILTERS[resample])
    assert plan, l.mx_last_error()
    try:
        lib.check(l.mx_resize_u8(plan, lib.current_stream(), src.data_ptr(), dst_buf.data_ptr() + lo, b, c), "mx_resize_u8")
        torch.cuda.synchronize()
    finally:
        l.mx_resize_destroy(plan)
    host = dst_buf.cpu().numpy()
    assert (host[:lo] == FILL).all() and (host[lo + n_out:] == FILL).all(), "guard bytes were written"
    return host[lo:lo + n_out].reshape((b, oh, ow) + x.shape[3:])


def check_case(x: np.ndarray, size, resample: str, pillow: np.ndarray) -> None:
    from sduss_amd import ops
    want = R.resize(x, size, resample)
    first = run_placed(x, size, resample, 0, 0)
    second = run_placed(x, size, resample, 3, 1)
    assert (first == second).all(), "two runs differ"
    assert first.shape == want.shape and (first == want).all(), f"{int((first != want).sum())} bytes differ from the restatement"
    assert (first == pillow).all(), f"{int((first != pillow).sum())} bytes differ from Pillow"
    via_ops = ops.resize_u8(torch.from_numpy(np.array(x)).cuda(), size, resample)
    assert via_ops.dtype == torch.uint8 and (via_ops.cpu().numpy() == want).all()


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("resample", list(R.FILTERS))
@pytest.mark.parametrize("case", range(len(R.CASES)), ids=["%dx%d-%dx%d" % c for c in R.CASES])
def test_resize_equals_pillow(cuda_device, golden, case, resample, channels):
    ih, iw, oh, ow = R.CASES[case]
    x = golden[f"in_{case}"]
    assert x.shape == (2, ih, iw, 3) and not (x[0] == x[1]).all()
    if channels == 1:
        x = np.ascontiguousarray(x[..., 0])
    check_case(x, (oh, ow), resample, golden[f"out_{case}_{resample}_c{channels}"])


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("resample", list(R.FILTERS))
@pytest.mark.parametrize("case", range(len(R.EXTRA_CASES)), ids=["%dx%d-%dx%d" % c for c in R.EXTRA_CASES])
def test_resize_equals_pillow_on_the_steep_paths(cuda_device, golden, case, resample, channels):
    """resize_ref.EXTRA_CASES: coefficient tables too large for LDS (read from memory instead), one axis or both, and a row segment that makes the
    plan shrink the chunk and the tile"""
    ih, iw, oh, ow = R.EXTRA_CASES[case]
    x = R.case_input(ih, iw, seed=200 + case)
    if channels == 1:
        x = np.ascontiguousarray(x[..., 0])
    check_case(x, (oh, ow), resample, golden[f"out_x{case}_{resample}_c{channels}"])


@pytest.mark.parametrize("channels", [1, 3])
def test_overshoot_hits_both_ends_of_the_clip(cuda_device, golden, channels):
    """a 0 / 255 checkerboard and a 1-pixel stripe image: lanczos overshoots on both sides in both passes (tests/test_image_resize_cpu.py shows it
    on the restatement), so both ends of both clips are exercised"""
    x = golden["in_overshoot"]
    if channels == 1:
        x = np.ascontiguousarray(x[..., 0])
    want = golden[f"out_overshoot_lanczos_c{channels}"]
    assert (want == 0).any() and (want == 255).any()
    check_case(x, R.OVERSHOOT_CASE[2:], "lanczos", want)


def test_plans_are_kept_per_size_and_filter(cuda_device):
    from sduss_amd import ops
    x = torch.from_numpy(R.case_input(9, 11, seed=5)).cuda()
    plans = ops._resize_plans.setdefault(x.device.index, ops._ResizePlans())
    ops.resize_u8(x, (12, 10), "bicubic")
    n = len(plans._plans)
    a = ops.resize_u8(x, (12, 10), "bicubic")
    assert len(plans._plans) == n and (9, 11, 12, 10, R.FILTERS["bicubic"]) in plans._plans
    for k in range(ops._ResizePlans.CAPACITY + 2):                           # more sizes than the cache holds: the oldest plans leave
        ops.resize_u8(x, (4 + k, 6), "bilinear")
    assert len(plans._plans) == ops._ResizePlans.CAPACITY and (9, 11, 12, 10, R.FILTERS["bicubic"]) not in plans._plans
    assert torch.equal(ops.resize_u8(x, (12, 10), "bicubic"), a)             # and come back as good as new
    assert (a.cpu().numpy() == R.resize(x.cpu().numpy(), (12, 10), "bicubic")).all()


# ---- the requests: size= equals the same call given the restatement's resized image and mask ----

LAT = 16                     # the tiny VAEs have three levels: a 64 px image is a 16 x 16 latent, the latent of a "128" request
CLIENT = (90, 75)            # the client's image: neither axis a multiple of anything


@pytest.fixture(scope="module")
def sdxl(cuda_device):
    from oracle import sdxl_unet_ref
    from sduss_amd.config import UNetConfig
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    from sduss_amd.unet import MxUNet
    from sduss_amd.vae import MxVAEEncoder, VAEConfig
    net = MxUNet(UNetConfig.tiny(), sdxl_unet_ref.init_params(sdxl_unet_ref.UNetConfig.tiny()), device="cuda:0")
    enc = MxVAEEncoder(VAEConfig.tiny(), E.init_params(vae_ref.VAEConfig.tiny()), device="cuda:0")
    return (lambda: SDXLDenoiser(net, guidance_scale=5.0), lambda den, i: synthetic_request(i, 128, 10, UNetConfig.tiny(), den, "cuda:0"), enc)


@pytest.fixture(scope="module")
def sd3(cuda_device):
    from oracle import sd3_mmdit_ref
    from sduss_amd.config import MMDiTConfig
    from sduss_amd.pipeline_sd3 import SD3Denoiser, synthetic_sd3_request
    from sduss_amd.transformer_sd3 import MxSD3Transformer
    from sduss_amd.vae import MxVAEEncoder, VAEConfig
    net = MxSD3Transformer(MMDiTConfig.tiny(), sd3_mmdit_ref.init_params(sd3_mmdit_ref.MMDiTConfig.tiny()), device="cuda:0")
    cfg = replace(VAEConfig.sd3(), block_out_channels=(64, 64, 128), layers_per_block=1)
    enc = MxVAEEncoder(cfg, E.init_params(vae_ref.VAEConfig.tiny_sd3()), device="cuda:0")
    return (lambda: SD3Denoiser(net, guidance_scale=7.0), lambda den, i: synthetic_sd3_request(i, 128, 8, MMDiTConfig.tiny(), den, "cuda:0", ctx_len=21), enc)


@pytest.fixture(params=["sdxl", "sd3"])
def model(request):
    return request.getfixturevalue(request.param)


def client_image(seed):
    return torch.from_numpy(R.case_input(*CLIENT, seed=seed)[:1])


def client_mask():
    """uint8 [1, 90, 75]: the left part repainted with a soft edge, so that the resized mask has bytes either side of 128"""
    m = torch.zeros((1,) + CLIENT, dtype=torch.uint8)
    m[:, :, :40] = 255
    m[:, ::4, 30:45] = 128
    m[:, 10:20, 50:70] = 200
    return m


def fixed_noise(enc, seed=9):
    return torch.randn(1, enc.cfg.latent_channels, LAT, LAT, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).cuda()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                                                                     b.view(torch.int16) if b.dtype == torch.bfloat16 else b)


@pytest.mark.parametrize("resample", ["lanczos", "bicubic"])
def test_start_from_image_with_size(model, resample):
    make_den, make_req, enc = model
    den = make_den()
    size = (4 * LAT, 4 * LAT)
    img, noise = client_image(31), fixed_noise(enc)
    resized = torch.from_numpy(R.resize(img.numpy(), size, resample)).cuda()
    a, b = make_req(den, 0), make_req(den, 1)
    den.start_from_image(a, enc, img.cuda(), 0.6, start_noise=noise, size=size, resample=resample)
    den.start_from_image(b, enc, resized, 0.6, start_noise=noise)
    torch.cuda.synchronize()
    assert a.step_index == b.step_index > 0 and a.latents.shape == (1, enc.cfg.latent_channels, LAT, LAT) and same_bits(a.latents, b.latents)
    c = make_req(den, 2)
    den.start_from_image(c, enc, resized, 0.6, start_noise=noise, size=None, resample="bilinear")      # no size: the filter is not used
    assert same_bits(c.latents, b.latents)


def test_start_inpaint_with_size(model):
    from sduss_amd.lib import MxError
    make_den, make_req, enc = model
    den = make_den()
    size = (4 * LAT, 4 * LAT)
    img, mask, noise = client_image(32), client_mask(), fixed_noise(enc)
    img_r = torch.from_numpy(R.resize(img.numpy(), size, "lanczos")).cuda()
    mask_r = torch.from_numpy(R.resize(mask.numpy(), size, "lanczos")).cuda()
    assert 0 < int((mask_r >= 128).sum()) < mask_r.numel() and bool(((mask_r > 0) & (mask_r < 128)).any()) and bool(((mask_r >= 128) & (mask_r < 255)).any())
    a, b = make_req(den, 0), make_req(den, 1)
    den.start_inpaint(a, enc, img.cuda(), mask.cuda(), strength=0.5, noise=noise, paste=True, size=size)
    den.start_inpaint(b, enc, img_r, mask_r, strength=0.5, noise=noise, paste=True)
    torch.cuda.synchronize()
    s, t = a.inpaint, b.inpaint
    assert a.step_index == b.step_index and same_bits(a.latents, b.latents)
    assert torch.equal(s.image_u8, img_r) and torch.equal(s.mask_u8, mask_r) and s.paste and t.paste           # the request keeps the resized pair
    assert same_bits(s.init, t.init) and same_bits(s.noise, t.noise) and torch.equal(s.mask, t.mask) and 0 < int(s.mask.sum()) < LAT * LAT
    with pytest.raises(MxError, match="mask"):
        den.start_inpaint(make_req(den, 2), enc, img.cuda(), mask[:, :64].cuda(), size=size)                  # the mask is not the client image's size
    with pytest.raises(MxError, match="mask"):
        den.start_inpaint(make_req(den, 2), enc, img_r, mask.cuda())                                          # size=None: the refusal stays as it was
