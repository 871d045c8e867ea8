"""Inpainting on the GPU (csrc/scheduler_step.hip, csrc/inpaint.hip): the masked scheduler steps, the start re-noising, the mask resize and the pixel paste on their own, then
Denoiser.start_inpaint / denoising_step / post_inference end to end for both models on the tiny configs of tests/test_vae_encode_gpu.py.

Every comparison is on the raw bits.  The stepped value must be what mx_cfg_euler_step / mx_cfg_flow_step leave (the same device functions); the kept
value keep * init + sigma_next * noise is a chain of separately rounded fp32 operations that torch evaluates identically on the CPU
(tests/inpaint_ref.py), rounded once to the io dtype; the byte kernels are integer selections."""
from dataclasses import replace

import pytest
import torch

import inpaint_ref as I
import vae_encode_ref as E
from step_operands import DTYPES, K, SLOTS, STEP_SHAPES, guards_intact, placed, same_bits

pytestmark = pytest.mark.gpu

from oracle import vae_ref  # noqa: E402  (checker only)

def step_operands(shape, dtype, flow, g):
    n, C, h, w = shape
    gen = torch.Generator().manual_seed(1000 * C + 10 * h + int(flow))
    pred = torch.randn((2 if g > 0 else 1) * n, C, h, w, generator=gen).to(dtype)
    lat = (torch.randn(n, C, h, w, generator=gen) * (1.0 if flow else 3.0)).to(dtype)
    sigma = torch.tensor([1.0, 0.7368, 0.3][:n] if flow else [14.6146, 3.1875, 0.9][:n])
    sigma_next = torch.tensor([0.9231, 0.5, 0.0][:n] if flow else [9.8123, 2.0625, 0.0][:n])
    init = torch.randn(K, C, h, w, generator=gen).to(dtype)
    noise = torch.randn(K, C, h, w, generator=gen).to(dtype)
    mask = torch.randint(0, 2, (K, h, w), generator=gen, dtype=torch.uint8) * torch.randint(1, 256, (K, h, w), generator=gen, dtype=torch.uint8)
    mask[0, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)            # non-zero is repaint, whatever the byte
    assert bool((mask == 0).any()) and bool((mask != 0).any())
    return pred, lat, sigma, sigma_next, init, noise, mask


def run_masked(flow, pred, lat, sigma, sigma_next, g, offset, slot=None, init=None, noise=None, mask=None):
    """one masked launch on fresh copies -> the latents it leaves, on the CPU (guards checked)"""
    from sduss_amd import ops
    fn = ops.cfg_flow_step_masked_ if flow else ops.cfg_euler_step_masked_
    pbuf, pv = placed(pred, offset)
    lbuf, lv = placed(lat, offset)
    rows, keepalive = [], []
    if init is not None:
        sbuf, sv = placed(torch.tensor(slot, dtype=torch.int32), 0)
        ibuf, iv = placed(init, offset)
        nbuf, nv = placed(noise, offset)
        mbuf, mv = placed(mask, offset)
        rows, keepalive = [sv, iv, nv, mv], [sbuf, ibuf, nbuf, mbuf]
    assert (lv.data_ptr() % 16 == 0) == (offset == 0)
    got = fn(pv, lv, sigma.cuda(), sigma_next.cuda(), g, *rows)
    torch.cuda.synchronize()
    assert got.data_ptr() == lv.data_ptr() and guards_intact(lbuf, lv) and torch.equal(pv.cpu(), pred)
    return lv.cpu()


def plain_step(flow, pred, lat, sigma, sigma_next, g):
    from sduss_amd import ops
    out = lat.cuda().clone()
    (ops.cfg_flow_step_ if flow else ops.cfg_euler_step_)(pred.cuda(), out, sigma.cuda(), sigma_next.cuda(), g)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("g", [5.0, 0.0], ids=["g5", "g0"])
@pytest.mark.parametrize("shape,offset", STEP_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flow", [False, True], ids=["euler", "flow"])
def test_masked_step(cuda_device, flow, dtype, shape, offset, g):
    pred, lat, sigma, sigma_next, init, noise, mask = step_operands(shape, dtype, flow, g)
    n = shape[0]
    plain = plain_step(flow, pred, lat, sigma, sigma_next, g)
    assert not same_bits(plain, lat)
    # no inpainting row: the plain step's bits
    assert same_bits(run_masked(flow, pred, lat, sigma, sigma_next, g, offset), plain)                                      # k = 0
    assert same_bits(run_masked(flow, pred, lat, sigma, sigma_next, g, offset, [-1] * n, init, noise, mask), plain)
    # mixed rows: repainted elements are the plain step's, kept ones the re-noised image's
    slot = SLOTS[n]
    got = run_masked(flow, pred, lat, sigma, sigma_next, g, offset, slot, init, noise, mask)
    want = I.masked_step(plain, flow, sigma_next, slot, init, noise, mask)
    assert not same_bits(want, plain)
    bad = I.bits(got) != I.bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {got.numel()} latents differ (first at {bad.nonzero()[0].tolist()})"
    for r, j in enumerate(slot):                                          # stated once more without the helper: a plain row is untouched by the rows beside it
        if j < 0:
            assert same_bits(got[r], plain[r])
    # a slot outside [0, k) is a plain row, never an index
    for wrong in (K, -7, 2 ** 31 - 1):
        bad_slot = [wrong if j == 0 else j for j in slot]
        got = run_masked(flow, pred, lat, sigma, sigma_next, g, offset, bad_slot, init, noise, mask)
        assert same_bits(got, I.masked_step(plain, flow, sigma_next, [-1 if j == wrong else j for j in bad_slot], init, noise, mask))
    # after the last step the kept region is the image's own latents, bit for bit
    zero = torch.zeros_like(sigma_next)
    plain0 = plain_step(flow, pred, lat, sigma, zero, g)
    got = run_masked(flow, pred, lat, sigma, zero, g, offset, slot, init, noise, mask)
    for r, j in enumerate(slot):
        keep = (mask[j] == 0)[None].expand_as(got[r]) if j >= 0 else torch.zeros_like(got[r], dtype=torch.bool)
        assert torch.equal(I.bits(got[r])[keep], I.bits(init[j] if j >= 0 else got[r])[keep])
        assert torch.equal(I.bits(got[r])[~keep], I.bits(plain0[r])[~keep])


@pytest.mark.parametrize("shape,offset", [pytest.param((3, 4, 5, 3), 0, id="3x60-elements"), pytest.param((2, 16, 16, 16), 0, id="2x4096-vectors"),
                                          pytest.param((2, 4, 8, 8), 1, id="2x256-offset-base")])
@pytest.mark.parametrize("dtype", DTYPES)
def test_inpaint_renoise(cuda_device, dtype, shape, offset):
    from sduss_amd import ops
    gen = torch.Generator().manual_seed(shape[1] + offset)
    init = torch.randn(shape, generator=gen).to(dtype)
    noise = torch.randn(shape, generator=gen).to(dtype)
    keep = torch.tensor([1.0, 0.3125 + 2.0 ** -20, 0.0][:shape[0]])
    sigma = torch.tensor([14.6146, 0.6875 - 2.0 ** -20, 1.0][:shape[0]])
    _ib, iv = placed(init, offset)
    _nb, nv = placed(noise, offset)
    got = ops.inpaint_renoise(iv, nv, keep, sigma)
    torch.cuda.synchronize()
    assert got.data_ptr() not in (iv.data_ptr(), nv.data_ptr()) and torch.equal(iv.cpu(), init) and torch.equal(nv.cpu(), noise)
    assert same_bits(got.cpu(), I.renoise(init, noise, keep, sigma))
    one = ops.inpaint_renoise(iv, nv, 1.0, 0.0)                           # scalars; sigma 0 gives the image's own latents back
    assert same_bits(one.cpu(), init)


@pytest.mark.parametrize("B,H,W,f", [(2, 24, 40, 8), (1, 8, 8, 8)])
def test_mask_to_latent(cuda_device, B, H, W, f):
    from sduss_amd import ops
    gen = torch.Generator().manual_seed(H + W)
    m = torch.randint(0, 256, (B, H, W), generator=gen, dtype=torch.uint8)
    m[:, ::f, ::f] = torch.where(torch.rand(B, H // f, W // f, generator=gen) < 0.5, 127, 128).to(torch.uint8)
    m[0, 0, 0] = 127
    m[0, H - f, W - f] = 128                                              # (one and the same pixel in the 8 x 8 case: 128 stands)
    got = ops.mask_to_latent(m.cuda(), f)
    torch.cuda.synchronize()
    want = I.latent_mask(m, f)
    assert got.shape == (B, H // f, W // f) and got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    assert int(want[0, -1, -1]) == 1 and (H == f or int(want[0, 0, 0]) == 0)


@pytest.mark.parametrize("B,H,W,offset", [pytest.param(2, 5, 7, 0, id="2x5x7"), pytest.param(1, 16, 16, 0, id="1x16x16"),
                                          pytest.param(1, 16, 16, 1, id="1x16x16-offset-base"), pytest.param(2, 5, 7, 3, id="2x5x7-offset-base")])
def test_rgb8_paste(cuda_device, B, H, W, offset):
    from sduss_amd import ops
    gen = torch.Generator().manual_seed(H * W + offset)
    dec = torch.randint(0, 256, (B, H, W, 3), generator=gen, dtype=torch.uint8)
    orig = torch.randint(0, 256, (B, H, W, 3), generator=gen, dtype=torch.uint8)
    mask = torch.randint(0, 256, (B, H, W), generator=gen, dtype=torch.uint8)
    mask.view(-1)[:8] = torch.tensor([127, 128, 0, 255, 128, 127, 127, 128], dtype=torch.uint8)
    mask.view(-1)[8:12] = 200                                             # a whole group repainted
    dbuf, dv = placed(dec, offset)
    _ob, ov = placed(orig, offset)
    _mb, mv = placed(mask, offset)
    got = ops.rgb8_paste_(dv, ov, mv)
    torch.cuda.synchronize()
    assert got.data_ptr() == dv.data_ptr() and guards_intact(dbuf, dv) and torch.equal(ov.cpu(), orig) and torch.equal(mv.cpu(), mask)
    want = I.paste(dec, orig, mask)
    assert not torch.equal(want, dec) and not torch.equal(want, orig)
    assert torch.equal(dv.cpu(), want)


# ---- end to end ----

LAT = 16                     # the tiny VAEs have three levels: a 64 px image is a 16 x 16 latent, the latent of a "128" request


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
    return (lambda: SDXLDenoiser(net, guidance_scale=5.0), lambda den, i: synthetic_request(i, 128, 10, UNetConfig.tiny(), den, "cuda:0"), enc, dec, 10)


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
    return (lambda: SD3Denoiser(net, guidance_scale=7.0), lambda den, i: synthetic_sd3_request(i, 128, 8, MMDiTConfig.tiny(), den, "cuda:0", ctx_len=21),
            enc, dec, 8)


@pytest.fixture(params=["sdxl", "sd3"])
def model(request):
    return request.getfixturevalue(request.param)


def client_image(seed):
    return torch.randint(0, 256, (1, 4 * LAT, 4 * LAT, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).cuda()


def fixed_noise(enc, seed=9):
    return torch.randn(1, enc.cfg.latent_channels, LAT, LAT, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).cuda()


def half_mask():
    """the left half repainted, with bytes either side of the threshold: uint8 [1, 64, 64]"""
    m = torch.full((1, 4 * LAT, 4 * LAT), 127, dtype=torch.uint8)
    m[:, :, :2 * LAT] = 128
    m[:, ::3, :2 * LAT] = 255
    m[:, ::5, 2 * LAT:] = 0
    return m.cuda()


def run_to_end(den, batch):
    with torch.inference_mode():
        while not all(r.done() for r in batch):
            den.denoising_step({"128": [r for r in batch if not r.done()]})
    torch.cuda.synchronize()


def test_start_inpaint_state(model):
    """what start_inpaint leaves on the request: one clean encode, the mask on the latent grid, the start latents of both strength regimes"""
    from sduss_amd import ops
    from sduss_amd.lib import MxError
    from sduss_amd.pipeline import start_step
    make_den, make_req, enc, _dec, steps = model
    den = make_den()
    img, mask, noise = client_image(21), half_mask(), fixed_noise(enc)
    a = make_req(den, 0)
    den.start_inpaint(a, enc, img, mask, strength=0.5, noise=noise, paste=True)
    t = start_step(steps, 0.5)
    s = a.inpaint
    assert a.step_index == t and s.paste and torch.equal(s.image_u8, img) and torch.equal(s.mask_u8, mask)
    assert same_bits(s.init, enc.encode_images(img)) and same_bits(s.noise, noise)
    assert torch.equal(s.mask.cpu(), I.latent_mask(mask.cpu(), 4)) and s.mask.shape == (1, LAT, LAT) and 0 < int(s.mask.sum()) < LAT * LAT
    keep, sigma = den._start_mix(a.sigmas[t])
    assert same_bits(a.latents.cpu(), I.renoise(s.init.cpu(), noise.cpu(), float(keep), float(sigma)))
    b = make_req(den, 1)
    den.start_inpaint(b, enc, img, mask, noise=noise)                        # strength 1: pure noise at the first sigma, nothing of the image
    scale = den.init_noise_sigma(steps) if hasattr(den, "init_noise_sigma") else 1.0
    assert b.step_index == 0 and not b.inpaint.paste
    assert same_bits(b.latents.cpu(), (noise.cpu().float() * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16))
    assert same_bits(b.latents, ops.inpaint_renoise(b.inpaint.init, noise, 0.0, scale))
    with pytest.raises(MxError, match="paste"):
        den.start_inpaint(make_req(den, 2), enc, E.preprocess_u8(img.cpu()).cuda(), mask, paste=True)
    with pytest.raises(MxError, match="mask"):
        den.start_inpaint(make_req(den, 2), enc, img, mask[:, :32])


def test_mask_all_ones_is_a_plain_request(model):
    make_den, make_req, enc, _dec, _steps = model
    den = make_den()
    a, b = make_req(den, 0), make_req(den, 1)
    den.start_inpaint(a, enc, client_image(22), torch.full((1, 4 * LAT, 4 * LAT), 255, dtype=torch.uint8).cuda(), strength=0.6, noise=fixed_noise(enc))
    b.latents, b.step_index = a.latents.clone(), a.step_index
    assert a.inpaint is not None and b.inpaint is None
    run_to_end(den, [a])
    run_to_end(den, [b])
    assert a.done() and b.done() and torch.isfinite(a.latents.float()).all() and same_bits(a.latents, b.latents)


def test_mask_all_zeros_returns_the_image_latents(model):
    make_den, make_req, enc, _dec, _steps = model
    den = make_den()
    a = make_req(den, 0)
    den.start_inpaint(a, enc, client_image(23), torch.zeros((1, 4 * LAT, 4 * LAT), dtype=torch.uint8).cuda(), strength=0.6, noise=fixed_noise(enc))
    assert not same_bits(a.latents, a.inpaint.init)
    run_to_end(den, [a])
    assert same_bits(a.latents, a.inpaint.init)


def test_half_mask_beside_a_plain_request(model):
    """a mixed batch: the plain request is untouched by its neighbour's mask; the kept half of the inpainting request ends as the image's latents"""
    make_den, make_req, enc, _dec, _steps = model
    img, mask, noise = client_image(24), half_mask(), fixed_noise(enc)
    finals = {}
    for inpaint in (True, False):
        den = make_den()
        a, p = make_req(den, 0), make_req(den, 1)
        den.start_inpaint(a, enc, img, mask, strength=0.6, noise=noise)
        if not inpaint:
            a.inpaint = None                                             # the same composition, the same starting latents, both requests plain
        p.step_index = 1                                                  # requests at different steps share the launch
        run_to_end(den, [a, p])
        finals[inpaint] = (a.latents.clone(), p.latents.clone(), a)
    assert same_bits(finals[True][1], finals[False][1])
    lat, _p, a = finals[True]
    init = a.inpaint.init
    kept = (a.inpaint.mask == 0)[:, None].expand_as(lat)
    assert 0 < int(kept.sum()) < kept.numel()
    assert torch.equal(I.bits(lat)[kept], I.bits(init)[kept])
    assert not bool((I.bits(lat)[~kept] == I.bits(init)[~kept]).all())
    assert not same_bits(lat, finals[False][0])


def test_post_inference_pastes_the_original_pixels(model):
    from sduss_amd.vae import post_inference
    make_den, make_req, enc, dec, _steps = model
    den = make_den()
    img, mask = client_image(25), half_mask()
    a, p = make_req(den, 0), make_req(den, 1)
    den.start_inpaint(a, enc, img, mask, strength=0.5, noise=fixed_noise(enc), paste=True)
    run_to_end(den, [a, p])
    out = post_inference(dec, {"128": [a, p]}, "uint8")["128"]
    torch.cuda.synchronize()
    raw = dec.decode_images(torch.cat([a.latents, p.latents]))
    assert out.shape == (2, 4 * LAT, 4 * LAT, 3) and out.dtype == torch.uint8
    assert torch.equal(out[0:1].cpu(), I.paste(raw[0:1].cpu(), img.cpu(), mask.cpu()))
    outside = (mask < 128)[0]
    assert torch.equal(out[0][outside], img[0][outside]) and not torch.equal(out[0], raw[0])
    assert torch.equal(out[1], raw[1])                                      # the plain request beside it: the decoder's bytes
    pil = post_inference(dec, {"128": [a, p]}, "pil")["128"]
    assert pil[0].tobytes() == out[0].cpu().numpy().tobytes()
    pt = post_inference(dec, {"128": [a, p]}, "pt")["128"]                  # the tensor stage is unchanged
    assert torch.equal(pt, (dec.decode(torch.cat([a.latents, p.latents])) / 2 + 0.5).clamp(0, 1))
