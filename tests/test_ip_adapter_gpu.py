"""The image-prompt adapter through MxUNet: UNetConfig.tiny(), batch 2, 32x32 latents, a random adapter, against oracle/sdxl_unet_ref.unet_forward
with basic_transformer_block replaced by ip_ref.block_with_image_term (fp32), within the bounds of tests/test_unet_gpu.py::_check; the output must
move against the plain forward by more than 3x its own error (an ignored adapter cannot pass).  Scale 0, clearing and no announcement: bit for bit."""
import pytest
import torch

import ip_ref

pytestmark = pytest.mark.gpu

from oracle import sdxl_unet_ref as ref  # noqa: E402  (checker only)

@pytest.fixture(scope="module")
def tiny(cuda_device):
    from sduss_amd.config import UNetConfig
    from sduss_amd.ip_adapter import IPAdapter
    from sduss_amd.unet import MxUNet
    cfg, ocfg, P = UNetConfig.tiny(), ref.UNetConfig.tiny(), ref.init_params(ref.UNetConfig.tiny())
    net = MxUNet(cfg, P, device="cuda:0")
    sd = ip_ref.random_adapter_sd(cfg, 31, n_img=4, embed_dim=64)
    cpu = s, t, e, te, ti = ref.make_inputs(ocfg, 2, 32)
    emb = torch.randn(3, 64, generator=torch.Generator().manual_seed(5)).bfloat16()       # row 2: the mixed batch's third sample
    dev = (s.cuda().to(torch.bfloat16), t.cuda(), e.cuda().to(torch.bfloat16), te.cuda(), ti.cuda())
    return dict(cfg=cfg, ocfg=ocfg, P=P, net=net, sd=sd, ad=IPAdapter.from_state_dict(cfg, sd), cpu=cpu, dev=dev, emb=emb, plain=_forward(net, dev))


def _forward(net, inputs, emb=None, scale=None):
    s, t, e, te, ti = inputs
    added = dict(text_embeds=te, time_ids=ti, **({} if emb is None else dict(image_embeds=emb, ip_scale=torch.tensor(scale))))
    return net.forward({"256": s}, t, e, added_cond_kwargs=added, return_dict=False, is_sliced=False, patch_size=256)[0]["256"].clone()


def _oracle(tiny, monkeypatch, P, cpu, emb, scale):
    block = ip_ref.block_with_image_term(ref, tiny["sd"], ip_ref.tokens_ref(tiny["cfg"], tiny["sd"], emb), torch.tensor(scale))
    monkeypatch.setattr(ref, "basic_transformer_block", block)
    return ref.unet_forward(P, tiny["ocfg"], *cpu)


def _check(got, want, plain, what):
    got = got.float().cpu()
    scale, err = want.abs().max().item(), (got - want).abs().max().item()
    l2, moved = ((got - want).norm() / want.norm()).item(), (got - plain.float().cpu()).abs().max().item()
    print(f"{what}: max err {err:.4f} ({err / scale:.4f} of max), rel L2 {l2:.4f}; moved by {moved:.4f} against the plain forward")
    assert err <= 0.04 * scale and l2 <= 0.02, f"{what}: max err {err} vs scale {scale}, rel L2 {l2}"
    assert moved > 3 * err, f"{what}: moved by {moved}, no more than 3x the error {err}: an ignored adapter would pass"


def test_forward_matches_oracle_with_image_term(tiny, monkeypatch):
    tiny["net"].set_ip_adapter(tiny["ad"])
    got = _forward(tiny["net"], tiny["dev"], tiny["emb"][:2].cuda(), [1.0, 0.7])
    _check(got, _oracle(tiny, monkeypatch, tiny["P"], tiny["cpu"], tiny["emb"][:2], [1.0, 0.7]), tiny["plain"], "image prompt")
    net, inputs, plain = tiny["net"], tiny["dev"], tiny["plain"]
    got = _forward(net, inputs, tiny["emb"][:2].cuda(), [0.0, 0.9])
    assert torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1]), "the scale-0 row must be the plain forward's row, bit for bit"
    assert torch.equal(_forward(net, inputs), plain), "a forward that was not announced must be the plain forward"
    net.clear_ip_adapter()
    assert torch.equal(_forward(net, inputs), plain), "after clear_ip_adapter the forward must be the plain forward"


def test_mixed_resolution_forward(tiny, monkeypatch):
    net, ocfg, scale = tiny["net"], tiny["ocfg"], [0.8, 1.0, 0.6]
    small, big = ref.make_inputs(ocfg, 1, 16, seed=3), tiny["cpu"]
    cat = [torch.cat([a, b]) for a, b in zip(small[1:], big[1:])]
    net.set_ip_adapter(tiny["ad"])
    dev = lambda x: x.cuda().to(torch.bfloat16)
    args = ([dev(small[0]), dev(big[0])], cat[0].cuda(), dev(cat[1]), cat[2].cuda(), cat[3].cuda())
    plain = net.forward_mixed(*args)
    net.set_image_tokens(tiny["ad"].project(tiny["emb"].cuda()), torch.tensor(scale))
    got = net.forward_mixed(*args)
    for g, (cpu, rows) in enumerate(((small, slice(0, 1)), (big, slice(1, 3)))):
        _check(got[g], _oracle(tiny, monkeypatch, tiny["P"], cpu, tiny["emb"][rows], scale[rows]), plain[g], f"mixed group {g}")


def test_lora_and_image_prompt_together(tiny, monkeypatch):
    import lora_ref
    from sduss_amd import lora
    net, inputs = tiny["net"], tiny["dev"]
    x = lora.LoraAdapter.from_state_dict(tiny["cfg"], lora_ref.random_adapter_sd(tiny["cfg"], 21))
    net.set_ip_adapter(tiny["ad"])
    net.set_adapters([(x, 0.1)])                 # must not drop the image-prompt adapter
    got = _forward(net, inputs, tiny["emb"][:2].cuda(), [1.0, 0.7])
    lora_only = _forward(net, inputs)
    _check(got, _oracle(tiny, monkeypatch, lora.merged_params(tiny["P"], [(x, 0.1)]), tiny["cpu"], tiny["emb"][:2], [1.0, 0.7]), lora_only, "LoRA + image prompt")
    net.clear_ip_adapter()                       # ... nor the reverse
    assert torch.equal(_forward(net, inputs), lora_only)
    net.clear_adapters()


def test_denoiser_mixes_requests_with_and_without_an_image_prompt(tiny):
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request      # two resolutions, ONE launch sequence
    net, emb, den = tiny["net"], tiny["emb"][:1].cuda(), SDXLDenoiser(tiny["net"])
    net.set_ip_adapter(tiny["ad"])

    def step(prompt):
        reqs = [synthetic_request(i, res, 4, tiny["cfg"], den, "cuda:0") for i, res in enumerate((128, 256))]
        if prompt:
            den.set_image_prompt(reqs[0], emb, 0.8)
        den.denoising_step({"128": reqs[:1], "256": reqs[1:]})
        return reqs
    plain, got = step(False), step(True)
    assert torch.equal(got[1].latents, plain[1].latents) and not torch.equal(got[0].latents, plain[0].latents)
    rows, scale = den._image_rows(got, True)                     # [uncond 0, uncond 1, cond 0, cond 1]
    want = tiny["ad"].project(torch.cat([torch.zeros_like(emb), emb]))
    assert scale.tolist() == pytest.approx([0.8, 0.0, 0.8, 0.0]) and not rows[1].any() and not rows[3].any()
    assert torch.equal(rows[0], want[0]) and torch.equal(rows[2], want[1]), "the unconditional row carries the tokens of ZERO embeddings"


@pytest.mark.parametrize("how", ["cached", "ctx_len_128", "no_adapter"])
def test_refusals(tiny, how):
    from sduss_amd.lib import MxError      # (the library's block-cache and patch-parallel entry points: tests/test_ip_adapter_cpu.py)
    net, (s, t, e, te, ti) = tiny["net"], tiny["dev"]
    if how == "ctx_len_128":
        e = torch.randn(2, 128, e.shape[2], device="cuda").to(torch.bfloat16)
    net.clear_ip_adapter() if how == "no_adapter" else net.set_ip_adapter(tiny["ad"])
    net.set_image_tokens(tiny["ad"].project(tiny["emb"][:2].cuda()), torch.ones(2))
    with pytest.raises(MxError, match="image"):
        net.forward_one_cached(object(), s, t, e, te, ti) if how == "cached" else _forward(net, (s, t, e, te, ti))
    assert torch.equal(_forward(net, tiny["dev"]), tiny["plain"]), "a refused announcement must not reach the next forward"
