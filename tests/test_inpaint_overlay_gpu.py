"""Inpainting only the masked region on the GPU (csrc/inpaint_overlay.hip): the mask blur, the bounding box and the overlay against the numpy
restatements (tests/overlay_ref.py) and Pillow's stored bytes (tests/golden/overlay_pillow.npz), then Denoiser.start_inpaint with ``blur`` and
``crop_pad`` through vae.finish_cropped on the tiny configs of tests/test_inpaint_gpu.py.

Every comparison is ``==`` on bytes.  Every kernel case runs twice, into an output that starts on a 4-byte boundary from inputs that do (dword
accesses where the shape allows them) and into one that starts one byte after a boundary from inputs that do not (byte accesses); the two runs
must give equal bytes, and the 0xA5 bytes either side of every output must stay as they are.

| blur case                         | what it is there for                                                               |
| the stored shapes x radii x kinds | r = 0 (radius 0.3 .. 1), odd widths, 17- and 5-wide lines under r = 39 (all clamp) |
| 300x520 at radius 4 and 33        | columns across many 16-row segments (the last one short), three column blocks      |
| 1024x1024 at radius 4 and 33      | a whole dword-path plane: 64 row segments x 4 column blocks, every row thread busy |
| 1x17 .. 40x17 at radius 40        | every tap of every pass clamps                                                     |
| B = 3                             | planes that differ: nothing leaks from one into the next                           |
"""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import overlay_ref as O
import resize_ref as R
import vae_encode_ref as E

pytestmark = pytest.mark.gpu

from oracle import vae_ref  # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
FILL = 0xA5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "overlay_pillow.npz"))


def put(x: np.ndarray, off: int) -> torch.Tensor:
    """x on the device as a contiguous view that starts ``off`` bytes after a 16-byte boundary"""
    x = np.ascontiguousarray(x)
    buf = torch.zeros(16 + x.nbytes, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + x.nbytes]
    view.copy_(torch.from_numpy(x.reshape(-1).view(np.uint8)))
    return view


def guarded(nbytes: int, off: int):
    """(buffer, address) of ``nbytes`` output bytes ``off`` after a 16-byte boundary inside guard bytes"""
    buf = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
    return buf, GUARD + off


def take(buf: torch.Tensor, lo: int, nbytes: int) -> np.ndarray:
    host = buf.cpu().numpy()
    assert (host[:lo] == FILL).all() and (host[lo + nbytes:] == FILL).all(), "guard bytes were written"
    return host[lo:lo + nbytes].copy()


def run_blur(x: np.ndarray, radius: float, off: int) -> np.ndarray:
    from sduss_amd import lib
    l = lib.load()
    b, h, w = x.shape
    src = put(x, off)
    dst, lo = guarded(x.size, off)
    tmp, tlo = guarded(x.size, off)
    lib.check(l.mx_gaussian_blur_u8(lib.current_stream(), src.data_ptr(), dst.data_ptr() + lo, tmp.data_ptr() + tlo if radius > 0 else None, b, h, w, radius),
              "mx_gaussian_blur_u8")
    torch.cuda.synchronize()
    take(tmp, tlo, x.size)                                                       # the scratch's guards
    assert (src.cpu().numpy() == x.reshape(-1)).all()
    return take(dst, lo, x.size).reshape(x.shape)


def check_blur(x: np.ndarray, radius: float, pillow=None) -> None:
    from sduss_amd import ops
    want = O.gaussian_blur(x, radius)
    first, second = run_blur(x, radius, 0), run_blur(x, radius, 1)
    assert (first == second).all(), "two runs differ"
    assert (first == want).all(), f"{int((first != want).sum())} bytes differ from the restatement"
    if pillow is not None:
        assert (first == pillow).all(), f"{int((first != pillow).sum())} bytes differ from Pillow"
    via_ops = ops.gaussian_blur_u8(torch.from_numpy(x).cuda(), radius)
    assert via_ops.dtype == torch.uint8 and (via_ops.cpu().numpy() == want).all()


@pytest.mark.parametrize("key,h,w,kind,seed", O.blur_cases(), ids=[c[0] for c in O.blur_cases()])
def test_blur_equals_pillow(cuda_device, golden, key, h, w, kind, seed):
    m = O.case_mask(h, w, kind, seed)
    for radius in O.radii_of(key):
        check_blur(m[None], radius, golden[f"blur_{key}_r{radius:g}"][None])


@pytest.mark.parametrize("radius", [4.0, 33.0])
def test_blur_of_a_whole_plane(cuda_device, radius):
    x = np.stack([O.case_mask(1024, 1024, "random", 41) // 2 + O.case_mask(1024, 1024, "rect", 42) // 2])
    check_blur(x, radius)


@pytest.mark.parametrize("h", [1, 7, 40])
def test_blur_where_every_tap_clamps(cuda_device, h):
    assert O.box_params(40.0)[0] + 1 >= 17
    check_blur(O.case_mask(h, 17, "random", 60 + h)[None], 40.0)


def test_blur_of_three_different_planes_and_the_copy(cuda_device):
    x = np.stack([O.case_mask(37, 53, kind, 70 + i) for i, kind in enumerate(O.KINDS)])
    assert not (x[0] == x[1]).all() and not (x[1] == x[2]).all()
    for radius in (0.5, 3.3, 12.5):
        check_blur(x, radius)
        one = np.stack([run_blur(x[i:i + 1], radius, 0)[0] for i in range(3)])
        assert (one == run_blur(x, radius, 0)).all()
    for radius in (0.0, -1.0):                                                  # radius <= 0 copies
        assert (run_blur(x, radius, 0) == x).all() and (run_blur(x, radius, 1) == x).all()


# ---- bounding box ----

def run_bbox(x: np.ndarray, off: int) -> np.ndarray:
    from sduss_amd import lib
    l = lib.load()
    b, h, w = x.shape
    src = put(x, off)
    box, lo = guarded(16 * b, 0)
    lib.check(l.mx_mask_bbox_u8(lib.current_stream(), src.data_ptr(), box.data_ptr() + lo, b, h, w), "mx_mask_bbox_u8")
    torch.cuda.synchronize()
    return take(box, lo, 16 * b).view(np.int32).reshape(b, 4)


def bbox_planes(h: int, w: int) -> np.ndarray:
    """an empty plane, one pixel in each corner, a full plane, a plane whose only non-zero byte is 1, a blob, two far pixels"""
    p = np.zeros((9, h, w), dtype=np.uint8)
    p[1, 0, 0] = p[2, 0, w - 1] = p[3, h - 1, 0] = p[4, h - 1, w - 1] = 255
    p[5] = 255
    p[6, h // 2, w // 3] = 1
    p[7, h // 4:h // 2 + 1, w // 3:w // 2 + 1] = 9
    p[8, h - 1, 0] = p[8, 0, w - 1] = 128
    return p


@pytest.mark.parametrize("h,w", [(5, 7), (16, 5), (64, 64), (37, 53), (300, 520), (1031, 2048)], ids=lambda v: str(v))
def test_bbox(cuda_device, h, w):
    """5x7, 37x53: the byte path; 64x64: 16-byte chunks that each lie in one row; 16x5: chunks that span four rows; 300x520: chunks that straddle two
    rows and more than one workgroup a plane; 1031x2048: many workgroups a plane"""
    from sduss_amd import ops
    x = bbox_planes(h, w)
    want = O.bbox(x)
    assert tuple(want[0]) == (w, h, 0, 0) and tuple(want[1]) == (0, 0, 1, 1) and tuple(want[4]) == (w - 1, h - 1, w, h) and tuple(want[5]) == (0, 0, w, h)
    assert tuple(want[6]) == (w // 3, h // 2, w // 3 + 1, h // 2 + 1) and tuple(want[8]) == (0, 0, w, h)
    first, second = run_bbox(x, 0), run_bbox(x, 3)
    assert (first == second).all() and (first == want).all(), (first, want)
    via_ops = ops.mask_bbox(torch.from_numpy(x).cuda())
    assert via_ops.dtype == torch.int32 and via_ops.is_cuda and (via_ops.cpu().numpy() == want).all()
    assert (run_bbox(x[:1], 0) == want[:1]).all() and (run_bbox(x[6:7], 1) == want[6:7]).all()


# ---- overlay ----

def run_overlay(dec: np.ndarray, orig: np.ndarray, mask: np.ndarray, x: int, y: int, off: int) -> np.ndarray:
    from sduss_amd import lib
    l = lib.load()
    b, hh, ww, _c = orig.shape
    h, w = dec.shape[1:3]
    d, o, m = put(dec, off), put(orig, off), put(mask, off)
    out, lo = guarded(orig.size, off)
    lib.check(l.mx_rgb8_overlay(lib.current_stream(), d.data_ptr(), o.data_ptr(), m.data_ptr(), out.data_ptr() + lo, b, hh, ww, x, y, w, h), "mx_rgb8_overlay")
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == orig.reshape(-1)).all() and (m.cpu().numpy() == mask.reshape(-1)).all()
    return take(out, lo, orig.size).reshape(orig.shape)


@pytest.fixture(scope="module")
def triples():
    """every (decoded, original, mask) byte triple as a 4096 x 4096 problem, and the restatement's answer: made once"""
    dec, orig, mask = O.triple_image()
    return dec, orig, mask, O.overlay(dec, orig, mask, 0, 0)


@pytest.mark.parametrize("off", [0, 1])
def test_overlay_of_every_byte_triple(cuda_device, triples, off):
    dec, orig, mask, want = triples
    got = run_overlay(dec, orig, mask, 0, 0, off)
    assert (got == want).all(), f"{int((got != want).sum())} bytes differ from the restatement"


def test_overlay_of_every_byte_triple_through_ops(cuda_device, triples, golden):
    from sduss_amd import ops
    dec, orig, mask, want = triples
    d, o, m = (torch.from_numpy(v).cuda() for v in (dec, orig, mask))
    first, second = ops.rgb8_overlay(d, o, m), ops.rgb8_overlay(d, o, m, 0, 0)
    assert first.data_ptr() not in (d.data_ptr(), o.data_ptr()) and torch.equal(first, second) and (first.cpu().numpy() == want).all()
    t = O.sample_triples()                                                     # Pillow's own bytes for a sample, as one row of pixels
    dec1 = np.repeat(t[None, None, :, 0:1], 3, axis=-1)
    orig1 = np.repeat(t[None, None, :, 1:2], 3, axis=-1)
    got = ops.rgb8_overlay(torch.from_numpy(dec1).cuda(), torch.from_numpy(orig1).cuda(), torch.from_numpy(np.ascontiguousarray(t[None, None, :, 2])).cuda())
    assert (got.cpu().numpy()[0, 0, :, 0] == golden["overlay_out"]).all() and (got[..., 0] == got[..., 2]).all()


@pytest.mark.parametrize("B", [1, 2])
def test_overlay_of_a_box_strictly_inside(cuda_device, B):
    """a 21 x 33 box at the odd offsets (7, 5) of a 50 x 70 image: outside it the original's bytes whatever the mask says, inside it the blend"""
    rng = np.random.default_rng(90 + B)
    hh, ww, h, w, x, y = 50, 70, 21, 33, 7, 5
    orig = rng.integers(0, 256, (B, hh, ww, 3), dtype=np.uint8)
    dec = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    mask = rng.integers(0, 256, (B, hh, ww), dtype=np.uint8)                    # non-zero outside the box too: the box decides there
    mask[:, y:y + 4, x:x + 8] = np.array([0, 255, 1, 254, 127, 128, 0, 255], dtype=np.uint8)
    want = O.overlay(dec, orig, mask, x, y)
    first, second = run_overlay(dec, orig, mask, x, y, 0), run_overlay(dec, orig, mask, x, y, 1)
    assert (first == second).all() and (first == want).all()
    inside = np.zeros((B, hh, ww), dtype=bool)
    inside[:, y:y + h, x:x + w] = True
    assert (first[~inside] == orig[~inside]).all() and not (first[inside] == orig[inside]).all()
    assert (first[inside] == O.overlay_bytes(dec, orig[:, y:y + h, x:x + w], mask[:, y:y + h, x:x + w, None]).reshape(-1, 3)).all()
    hard = np.where(mask >= 128, 255, 0).astype(np.uint8)                       # a 0 / 255 mask: the hard paste
    got = run_overlay(dec, orig, hard, x, y, 0)
    paste = orig.copy()
    sel = inside & (hard == 255)
    paste[sel] = dec[hard[:, y:y + h, x:x + w] == 255]
    assert (got == paste).all()


# ---- the request: blur, crop, repaint, overlay ----

LAT = 16                     # the tiny VAEs have three levels: a 64 px image is a 16 x 16 latent, the latent of a "128" request
RES = 4 * LAT                # the request's size in pixels
CLIENT = (96, 160)


@pytest.fixture(scope="module")
def sdxl(cuda_device):
    from oracle import sdxl_unet_ref
    from sduss_amd.config import UNetConfig
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    from sduss_amd.unet import MxUNet
    from sduss_amd.vae import MxVAEDecoder, MxVAEEncoder, VAEConfig
    net = MxUNet(UNetConfig.tiny(), sdxl_unet_ref.init_params(sdxl_unet_ref.UNetConfig.tiny()), device="cuda:0")
    enc = MxVAEEncoder(VAEConfig.tiny(), E.init_params(vae_ref.VAEConfig.tiny()), device="cuda:0")
    dec = MxVAEDecoder(VAEConfig.tiny(), vae_ref.init_params(vae_ref.VAEConfig.tiny()), device="cuda:0")
    return (lambda: SDXLDenoiser(net, guidance_scale=5.0), lambda den, i: synthetic_request(i, 128, 10, UNetConfig.tiny(), den, "cuda:0"), enc, dec)


@pytest.fixture(scope="module")
def sd3(cuda_device):
    from oracle import sd3_mmdit_ref
    from sduss_amd.config import MMDiTConfig
    from sduss_amd.pipeline_sd3 import SD3Denoiser, synthetic_sd3_request
    from sduss_amd.transformer_sd3 import MxSD3Transformer
    from sduss_amd.vae import MxVAEDecoder, MxVAEEncoder, VAEConfig
    net = MxSD3Transformer(MMDiTConfig.tiny(), sd3_mmdit_ref.init_params(sd3_mmdit_ref.MMDiTConfig.tiny()), device="cuda:0")
    cfg = replace(VAEConfig.sd3(), block_out_channels=(64, 64, 128), layers_per_block=1)
    enc = MxVAEEncoder(cfg, E.init_params(vae_ref.VAEConfig.tiny_sd3()), device="cuda:0")
    dec = MxVAEDecoder(cfg, vae_ref.init_params(vae_ref.VAEConfig.tiny_sd3()), device="cuda:0")
    return (lambda: SD3Denoiser(net, guidance_scale=7.0), lambda den, i: synthetic_sd3_request(i, 128, 8, MMDiTConfig.tiny(), den, "cuda:0", ctx_len=21), enc, dec)


@pytest.fixture(params=["sdxl", "sd3"])
def model(request):
    return request.getfixturevalue(request.param)


def client_image(seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (1,) + CLIENT + (3,), dtype=np.uint8))


def blob_mask():
    """uint8 [1, 96, 160]: an off-centre blob, 255 inside an ellipse around (58, 101)"""
    yy, xx = np.mgrid[:CLIENT[0], :CLIENT[1]]
    return torch.from_numpy((((yy - 58) / 15.0) ** 2 + ((xx - 101) / 22.0) ** 2 <= 1.0).astype(np.uint8)[None] * 255)


def fixed_noise(enc, seed=9):
    return torch.randn(1, enc.cfg.latent_channels, LAT, LAT, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).cuda()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                                                                     b.view(torch.int16) if b.dtype == torch.bfloat16 else b)


def test_crop_blur_repaint_overlay_end_to_end(model):
    from sduss_amd.lib import MxError
    from sduss_amd.vae import finish_cropped, post_inference
    make_den, make_req, enc, dec = model
    den = make_den()
    img, mask, noise = client_image(33), blob_mask(), fixed_noise(enc)
    # by hand, with the restatements: blur at the client's size, box, crop rule, crop, Pillow's resize of both
    soft = O.gaussian_blur(mask.numpy(), 4.0)
    box = O.bbox(soft)[0]
    region = O.crop_region(box, CLIENT[1], CLIENT[0], RES, RES, 8)
    x1, y1, x2, y2 = region
    assert 0 < x1 and x2 < CLIENT[1] and 0 < y1 and y2 <= CLIENT[0] and (x2 - x1, y2 - y1) != (RES, RES) and bool(((soft > 0) & (soft < 255)).any())
    img_c = torch.from_numpy(R.resize(np.ascontiguousarray(img.numpy()[:, y1:y2, x1:x2]), (RES, RES), "lanczos")).cuda()
    mask_c = torch.from_numpy(R.resize(np.ascontiguousarray(soft[:, y1:y2, x1:x2]), (RES, RES), "lanczos")).cuda()
    a, b = make_req(den, 0), make_req(den, 1)
    den.start_inpaint(a, enc, img.cuda(), mask.cuda(), strength=0.5, noise=noise, blur=4.0, crop_pad=8)
    den.start_inpaint(b, enc, img_c, mask_c, strength=0.5, noise=noise)
    torch.cuda.synchronize()
    s, t = a.inpaint, b.inpaint
    assert s.region == region and s.overlay and not s.paste and t.region is None and not t.overlay and t.full_image_u8 is None
    assert torch.equal(s.full_image_u8.cpu(), img) and (s.full_mask_u8.cpu().numpy() == soft).all()
    assert torch.equal(s.image_u8, img_c) and torch.equal(s.mask_u8, mask_c) and torch.equal(s.mask, t.mask) and 0 < int(s.mask.sum()) < LAT * LAT
    assert a.step_index == b.step_index and same_bits(s.init, t.init) and same_bits(a.latents, b.latents)
    with torch.inference_mode():
        for _ in range(2):
            den.denoising_step({"128": [a, b]})
    torch.cuda.synchronize()
    assert a.step_index == b.step_index and torch.isfinite(a.latents.float()).all()
    row = dec.decode_images(a.latents)
    full = finish_cropped(a, row)
    torch.cuda.synchronize()
    small = R.resize(row.cpu().numpy(), (y2 - y1, x2 - x1), "lanczos")
    want = O.overlay(small, img.numpy(), soft, x1, y1)
    assert full.shape == (1,) + CLIENT + (3,) and full.dtype == torch.uint8 and (full.cpu().numpy() == want).all()
    untouched = soft[0] == 0
    assert untouched.any() and (full.cpu().numpy()[0][untouched] == img.numpy()[0][untouched]).all() and not (full.cpu().numpy() == img.numpy()).all()
    # post_inference: "uint8" leaves the cropped request's row as decoded, "pil" returns it at the client's size
    out = post_inference(dec, {"128": [a, b]}, "uint8")["128"]
    assert torch.equal(out[0:1], row) and torch.equal(out[1:2], dec.decode_images(b.latents))
    pil = post_inference(dec, {"128": [a, b]}, "pil")["128"]
    assert pil[0].size == (CLIENT[1], CLIENT[0]) and pil[0].tobytes() == want.tobytes() and pil[1].size == (RES, RES)
    with pytest.raises(MxError, match="not started with crop_pad"):
        finish_cropped(b, row)
    # an empty mask has no region
    with pytest.raises(MxError, match="empty"):
        den.start_inpaint(make_req(den, 2), enc, img.cuda(), torch.zeros_like(mask).cuda(), crop_pad=8)


def test_overlay_without_a_region_and_the_parent_path(model):
    """``overlay`` alone blends at the request's size in post_inference; a request started without the new arguments is the parent commit's: no
    region, and the latents of the same call spelled without them"""
    from sduss_amd import ops
    from sduss_amd.vae import post_inference
    make_den, make_req, enc, dec = model
    den = make_den()
    img = torch.from_numpy(np.random.default_rng(34).integers(0, 256, (1, RES, RES, 3), dtype=np.uint8)).cuda()
    mask = blob_mask()[:, 20:20 + RES, 60:60 + RES].contiguous().cuda()
    noise = fixed_noise(enc)
    a, b, c = make_req(den, 0), make_req(den, 1), make_req(den, 2)
    den.start_inpaint(a, enc, img, mask, strength=0.5, noise=noise, blur=3.3, overlay=True)
    den.start_inpaint(b, enc, img, mask, strength=0.5, noise=noise)
    den.start_inpaint(c, enc, img, mask, strength=0.5, noise=noise, blur=0.0, crop_pad=None, overlay=False)
    soft = O.gaussian_blur(mask.cpu().numpy(), 3.3)
    assert a.inpaint.overlay and a.inpaint.region is None and (a.inpaint.mask_u8.cpu().numpy() == soft).all()
    for r in (b, c):
        assert r.inpaint.region is None and not r.inpaint.overlay and r.inpaint.full_image_u8 is None and torch.equal(r.inpaint.mask_u8, mask)
    assert same_bits(b.latents, c.latents) and same_bits(b.inpaint.init, c.inpaint.init) and torch.equal(b.inpaint.mask, c.inpaint.mask)
    assert same_bits(b.latents, ops.inpaint_renoise(enc.encode_images(img), noise, *den._inpaint_start_mix(b, b.step_index, 0.5)))
    with torch.inference_mode():
        den.denoising_step({"128": [a, b]})
    out = post_inference(dec, {"128": [a, b]}, "uint8")["128"]
    torch.cuda.synchronize()
    raw = dec.decode_images(torch.cat([a.latents, b.latents]))
    assert (out[0:1].cpu().numpy() == O.overlay(raw[0:1].cpu().numpy(), img.cpu().numpy(), soft, 0, 0)).all()
    assert torch.equal(out[1], raw[1]) and not torch.equal(out[0], raw[0])
    pil = post_inference(dec, {"128": [a, b]}, "pil")["128"]
    assert pil[0].tobytes() == out[0].cpu().numpy().tobytes()
