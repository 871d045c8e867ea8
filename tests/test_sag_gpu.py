"""Self-attention guidance on the GPU (csrc/sag.hip): mx_attention_colmass and mx_sag_degrade against tests/sag_ref.py in float64, the capture in
UNetConfig.tiny(), and one SDXLDenoiser.denoising_step with and without a SAG request."""
import pytest
import torch

import sag_ref
import sampler_ref as S
from oracle import sdxl_unet_ref as ref  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu


def _mass_bound(q, k, heads, batch, scale):
    """(fp64 mass, 16 x the error of the plain fp32 torch evaluation on the CPU)"""
    want = sag_ref.colmass(q.cpu(), k.cpu(), heads, batch, scale)
    return want, 16.0 * (sag_ref.colmass(q.cpu(), k.cpu(), heads, batch, scale, torch.float32).double() - want).abs().max().item()


def _check_mass(mass, mask, want, bound, what):
    err = (mass.double().cpu() - want).abs().max().item()
    sure = (want - 1.0).abs() > bound
    print(f"{what}: mass in [{want.min():.3f}, {want.max():.3f}], max err {err:.3g}, bound {bound:.3g}, {int((~sure).sum())} elements inside the band")
    assert err <= bound
    assert (~sure).sum() <= 0.01 * sure.numel()
    assert torch.equal(mask.cpu().bool()[sure], (want > 1.0)[sure])


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,L", [(1, 1, 64), (2, 2, 60), (1, 3, 200), (2, 2, 320)])
def test_colmass_against_fp64(cuda_device, B, H, L, prescaled):
    """One tile; a ragged single tile and two samples; two query blocks and four key tiles, both ragged, odd heads; three query blocks.  Inputs bf16
    N(0, 1), q times 3: masses over about 0.2 .. 3.2.  Bound: 16 x the error of the fp32 torch evaluation of the same inputs on the CPU, which measured
    4.4e-7, 3.1e-7, 3.2e-7, 4.6e-7 for the four shapes (bounds 7.0e-6, 4.9e-6, 5.1e-6, 7.3e-6; prescaled q is other data: 3e-7 .. 6e-7); no
    reference element lies inside the band around 1.  Two runs give the same bits."""
    from sduss_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + L)
    q, k = torch.randn(B * L, H * 64, generator=g) * 3, torch.randn(B * L, H * 64, generator=g).bfloat16().cuda()
    q = (q * ops.ATTN_QSCALE if prescaled else q).bfloat16().cuda()
    qk = torch.cat([q, k], dim=1)                                    # the q | k buffer of the step plan: row views with stride 2 H 64
    mass, mask = ops.attention_colmass(qk[:, :H * 64], qk[:, H * 64:], H, B, prescaled=prescaled)
    again = ops.attention_colmass(qk[:, :H * 64], qk[:, H * 64:], H, B, prescaled=prescaled)
    assert torch.equal(mass, again[0]) and torch.equal(mask, again[1])
    want, bound = _mass_bound(q, k, H, B, sag_ref.LN2 if prescaled else 0.125)
    _check_mass(mass, mask, want, bound, f"colmass B{B} H{H} L{L} prescaled={prescaled}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("h,w,hm,wm", [(8, 8, 2, 2), (12, 20, 3, 5), (5, 5, 1, 1), (40, 36, 5, 9)])
def test_degrade_against_fp64(cuda_device, h, w, hm, wm, dtype):
    """Reflect pad across most of the image; non-square; the smallest legal size; more than one tile with ragged ones.  Three rows of different
    sigmas: a random mask, all false, all true; one launch over rows (2, 0, 1).  Bound per element, u = 2^-24: the output rounding (half an ulp: at most
    2^-8 |ref| with bf16's 8-bit significand, u |ref| with fp32's 24 bits) plus u (20 blur|x0| + 2 blur(|x| + |n|) + 2 |n| + 2 |ref|) -- 18 fused taps over x0, whose own two roundings pass through
    the blur, then the product n = sigma eps and the last sum.  Unmasked elements equal ((x - n) + n) in fp32, rounded once, exactly."""
    from sduss_amd import ops
    g = torch.Generator().manual_seed(h * 100 + w)
    x, eps = (torch.randn(3, 4, h, w, generator=g) * s for s in (5.0, 1.0))
    x, eps = x.to(dtype), torch.cat([eps, torch.full((3, 4, h, w), float("nan"))]).to(dtype)          # (the conditional rows are never read)
    sigma = torch.tensor([14.6, 0.7, 3.1])
    mask = torch.stack([(torch.rand(hm, wm, generator=g) > 0.5), torch.zeros(hm, wm, dtype=torch.bool), torch.ones(hm, wm, dtype=torch.bool)]).to(torch.uint8)
    rows = [2, 0, 1]
    got = ops.sag_degrade(x.cuda(), eps.cuda(), sigma.cuda(), mask.cuda(), 1.0, rows=rows).cpu()
    want, x0, n = sag_ref.degrade(x, eps[:3], sigma, mask, 1.0)
    u, ab = 2.0 ** -24, lambda t: sag_ref.blur(t.abs(), 1.0)      # noqa: E731
    bound = (2.0 ** -8 if dtype == torch.bfloat16 else u) * want.abs() + u * (20 * ab(x0) + 2 * ab(x.double().abs() + n.abs()) + 2 * n.abs() + 2 * want.abs())
    ratio = ((got.double() - want[rows]).abs() / bound[rows]).max().item()
    print(f"degrade {h}x{w} {dtype}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0
    n32 = sigma.reshape(-1, 1, 1, 1) * eps[:3].float()
    plain = ((x.float() - n32) + n32).to(dtype)
    off = ~sag_ref.stretch(mask, h, w).expand_as(plain)
    assert torch.equal(got[off[rows]], plain[rows][off[rows]])
    assert not torch.equal(got[0], plain[2]), "the all-true row must be blurred"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_fold_against_fp32(cuda_device, dtype):
    """noise [6 rows] = [uncond ; cond], SAG rows (2, 0) of 3: the conditional rows 5 and 3 become eps_c + coef (eps_u - eps_d) in fp32 operations, rounded
    once, bit for bit; every other row keeps its bits."""
    from sduss_amd import ops
    g = torch.Generator().manual_seed(7)
    noise, eps_d = torch.randn(6, 4, 9, 7, generator=g).to(dtype), torch.randn(2, 4, 9, 7, generator=g).to(dtype)
    rows, coef = [2, 0], [0.15, -0.4]
    want = noise.clone()
    for i, r in enumerate(rows):
        want[3 + r] = (noise[3 + r].float() + torch.tensor(coef[i]) * (noise[r].float() - eps_d[i].float())).to(dtype)
    got = ops.sag_fold_(noise.cuda(), eps_d.cuda(), coef, rows=rows).cpu()
    assert torch.equal(got, want) and not torch.equal(got[3], noise[3])


HW, BATCH = 40, 4              # mid grid 10 x 10: L = 100, a ragged query block and a ragged second key tile; rows [u0, u1, c0, c1]


@pytest.fixture(scope="module")
def tiny(cuda_device):
    from sduss_amd.config import UNetConfig
    from sduss_amd.unet import MxUNet
    ocfg, P = ref.UNetConfig.tiny(), ref.init_params(ref.UNetConfig.tiny())
    s, t, e, te, ti = ref.make_inputs(ocfg, BATCH, HW, seed=HW)
    dev = (s.cuda().to(torch.bfloat16), t.cuda(), e.cuda().to(torch.bfloat16), te.cuda(), ti.cuda())
    return dict(net=MxUNet(UNetConfig.tiny(), P, device="cuda:0"), dev=dev)


def test_capture_in_the_tiny_unet(tiny):
    """The announced forward's output has the plain forward's bits, and the captured mass is that of rows [0, 2) of the q | k operand of
    mid_block.attentions.0.transformer_blocks.0.attn1 (traced; q prescaled, so softmax of q k^T ln 2) under test_colmass_against_fp64's rule.  The
    masses of the conditional rows [2, 4) and of transformer block 1 are checked to lie outside that bound: capturing either would fail."""
    net, dev = tiny["net"], tiny["dev"]
    heads, C = net.cfg.num_heads[-1], net.cfg.block_out_channels[-1]
    hm, wm = net.mid_grid(HW, HW)
    L, half = hm * wm, BATCH // 2
    plain = net.forward_one(*dev)
    mass = torch.full((half, L), float("nan"), device="cuda")
    mask = torch.full((half, L), 7, dtype=torch.uint8, device="cuda")
    net.set_attention_mass(mass, mask, half)
    assert torch.equal(net.forward_one(*dev), plain), "capture must leave the forward's bits alone"
    assert torch.equal(net.forward_one(*dev), plain) and net._mass_next is None      # one-shot
    block = "mid_block.attentions.0.transformer_blocks.%d.attn1.to_qkv"
    qk = net.forward_one(*dev, stage=block % 0, stage_shape=(BATCH * L, 2 * C))
    want, bound = _mass_bound(qk[:half * L, :C], qk[:half * L, C:], heads, half, sag_ref.LN2)
    _check_mass(mass, mask, want, bound, "captured mass")
    other = net.forward_one(*dev, stage=block % 1, stage_shape=(BATCH * L, 2 * C))
    for wrong in (qk[half * L:], other[:half * L]):
        assert (sag_ref.colmass(wrong[:, :C].cpu(), wrong[:, C:].cpu(), heads, half, sag_ref.LN2) - want).abs().max() > 100 * bound


@pytest.mark.parametrize("sampler,schedule", [("euler", "default"), ("dpmpp_2m", "karras")])
def test_denoising_step(cuda_device, sampler, schedule):
    """Requests A (set_sag 0.75) and B (none) in one step.  B's new latents have the bits of the step without SAG anywhere, and so has A with scale 0,
    which announces no capture.  A against float64: eps_u, eps_c from a direct forward of the step's rows with capture announced, x_deg from
    ops.sag_degrade (checked above), eps_d from a direct forward on it with A's negative prompt; eps = eps_u + g (eps_c - eps_u) + 0.75 (eps_u - eps_d)
    and the sampler's first step in float64 (sampler_ref's rows).  Bound: 4 x the error of the same composition in the step's working precision on the
    CPU -- the conditional row replaced in fp32 and rounded to bf16, sampler_ref's bf16 combine and fp32 step, the bf16 cast -- which measured
    0.099 (Euler) and 0.110 (dpmpp_2m) at latents of up to 24, bounds 0.395 and 0.438 (a bf16 ulp there is 0.125)."""
    from sduss_amd import ops
    from sduss_amd.config import UNetConfig
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    from sduss_amd.unet import MxUNet
    net = MxUNet(UNetConfig.tiny(), ref.init_params(ref.UNetConfig.tiny()), device="cuda:0")
    g, scale = 5.0, 0.75

    def run(sag):
        den = SDXLDenoiser(net, guidance_scale=g)
        reqs = [synthetic_request(i, 128, 6, UNetConfig.tiny(), den, "cuda:0", sampler=sampler, schedule=schedule) for i in range(2)]
        if sag is not None:
            den.set_sag(reqs[0], scale=sag)
        before = [r.latents.clone() for r in reqs]
        den.denoising_step({"128": reqs})
        return den, reqs, before

    _, base, _ = run(None)
    net._mass_live = None
    _, zero, _ = run(0.0)
    assert net._mass_live is None and all(torch.equal(a.latents, b.latents) for a, b in zip(zero, base))
    den, reqs, before = run(scale)
    assert torch.equal(reqs[1].latents, base[1].latents), "the request without SAG must keep its bits"
    assert not torch.equal(reqs[0].latents, base[0].latents)

    a, lat = reqs[0], torch.cat(before)
    sig = torch.tensor([float(r.sigmas[0]) for r in reqs], device="cuda")
    ts = torch.tensor([float(r.timesteps[0]) for r in reqs] * 2, device="cuda")
    hm, wm = net.mid_grid(16, 16)
    mass, mask = torch.empty(2, hm * wm, device="cuda"), torch.empty(2, hm * wm, dtype=torch.uint8, device="cuda")
    net.set_attention_mass(mass, mask, 2)
    noise = net.forward_one(ops.euler_scale_input(lat, sig, 4), ts, *SDXLDenoiser._cond(reqs, True))
    x_deg = ops.sag_degrade(lat, noise, sig, mask.view(2, hm, wm), 1.0, rows=[0])
    eps_d = net.forward_one(ops.euler_scale_input(x_deg, sig[:1], 1), ts[:1], a.negative_prompt_embeds, a.negative_pooled_prompt_embeds, a.negative_add_time_ids)
    eps_u, eps_c, eps_d, x = noise[0].cpu(), noise[2].cpu(), eps_d[0].cpu(), lat[0].cpu()
    folded = (eps_c.float() + (scale / g) * (eps_u.float() - eps_d.float())).bfloat16()
    m64, m_work = sag_ref.guided(eps_u, eps_c, eps_d, g, scale), S.guided(torch.stack([eps_u, folded]), 1, g)[0]
    s, sn = a.sigmas[0], a.sigmas[1]
    if sampler == "euler":
        step = lambda xx, mm: S.euler_row(xx, mm, s, sn, False)      # noqa: E731
    else:
        coef = S.step_coef(S.coeffs(S.DPMPP_2M, a.sigmas), 0, False)
        step = lambda xx, mm: S.multistep_row(S.DPMPP_2M, xx, mm, s, coef, None)[0]      # noqa: E731
    want, work = step(x.double(), m64), step(x.float(), m_work).bfloat16()
    bound = 4.0 * (work.double() - want).abs().max().item()
    moved = (step(x.double(), sag_ref.guided(eps_u, eps_c, eps_d, g, 0.0)) - want).abs().max().item()
    assert moved > 4.0 * bound, f"the SAG term moves the step by {moved:.3g}, not clear of the bound {bound:.3g}: a wrong sign or factor would pass"
    err = (a.latents[0].cpu().double() - want).abs().max().item()
    print(f"SAG step {sampler}: max err {err:.4g}, bound {bound:.4g}, the SAG term moves the step by {moved:.4g}, |latents| up to {want.abs().max():.1f}")
    assert err <= bound
