"""Regional prompts through MxUNet and SDXLDenoiser: UNetConfig.tiny(), batch 2, 32x32 latents (token grids 16x16 and 8x8), row 0 with one prompt and row 1
with three, against oracle/sdxl_unet_ref.unet_forward with basic_transformer_block replaced by regions_ref.block_with_regions (fp32), judged as
tests/test_ip_adapter_gpu.py judges the image-prompt forward.  Counts of 1 everywhere: the plain forward bit for bit."""
import pytest
import torch

import regions_ref

pytestmark = pytest.mark.gpu

from oracle import sdxl_unet_ref as ref  # noqa: E402  (checker only)


@pytest.fixture(scope="module")
def tiny(cuda_device):
    from sduss_amd import regions
    from sduss_amd.config import UNetConfig
    from sduss_amd.unet import MxUNet
    cfg, ocfg, P = UNetConfig.tiny(), ref.UNetConfig.tiny(), ref.init_params(ref.UNetConfig.tiny())
    net = MxUNet(cfg, P, device="cuda:0")
    cpu = s, t, e, te, ti = ref.make_inputs(ocfg, 2, 32)
    dev = (s.cuda().to(torch.bfloat16), t.cuda(), e.cuda().to(torch.bfloat16), te.cuda(), ti.cuda())
    gen = torch.Generator().manual_seed(9)
    masks = torch.zeros(3, 32, 32)                 # base everywhere, a left band and an overlapping soft right band
    masks[0], masks[1, :, :14], masks[2, :, 9:] = 0.5, 1.0, torch.rand(32, 23, generator=gen)
    rg = regions.Regions(torch.randn(3, 77, e.shape[2], generator=gen).bfloat16(), masks, (32, 32))
    wide, counts, tables, seg = regions.batch_operands([None, rg], dev[2], 1, regions.token_grids(cfg, 32, 32))
    return dict(cfg=cfg, ocfg=ocfg, P=P, net=net, cpu=cpu, dev=dev, plain=_forward(net, dev), wide=wide, counts=counts, tables=tables, seg=seg)


def _forward(net, inputs, wide=None, counts=None, tables=None):
    s, t, e, te, ti = inputs
    added = dict(text_embeds=te, time_ids=ti, **({} if wide is None else dict(region_counts=counts, region_weights=tables)))
    return net.forward({"256": s}, t, e if wide is None else wide, added_cond_kwargs=added, return_dict=False, is_sliced=False, patch_size=256)[0]["256"].clone()


def _check(got, want, plain, what):                # tests/test_ip_adapter_gpu.py::_check
    got = got.float().cpu()
    scale, err = want.abs().max().item(), (got - want).abs().max().item()
    l2, moved = ((got - want).norm() / want.norm()).item(), (got - plain.float().cpu()).abs().max().item()
    print(f"{what}: max err {err:.4f} ({err / scale:.4f} of max), rel L2 {l2:.4f}; moved by {moved:.4f} against the plain forward")
    assert err <= 0.04 * scale and l2 <= 0.02, f"{what}: max err {err} vs scale {scale}, rel L2 {l2}"
    assert moved > 3 * err, f"{what}: moved by {moved}, no more than 3x the error {err}: ignored regions would pass"


def test_forward_matches_oracle_with_regions(tiny, monkeypatch):
    got = _forward(tiny["net"], tiny["dev"], tiny["wide"], tiny["counts"], tiny["tables"])
    block = regions_ref.block_with_regions(ref, tiny["counts"].cpu(), [t.cpu() for t in tiny["tables"]], tiny["seg"], 80)
    monkeypatch.setattr(ref, "basic_transformer_block", block)
    s, t, _e, te, ti = tiny["cpu"]
    _check(got, ref.unet_forward(tiny["P"], tiny["ocfg"], s, t, tiny["wide"].float().cpu(), te, ti), tiny["plain"], "regions")
    assert torch.equal(got[0], tiny["plain"][0]), "the one-prompt row must be the plain forward's row, bit for bit"
    assert torch.equal(_forward(tiny["net"], tiny["dev"]), tiny["plain"]), "a forward that was not announced must be the plain forward"
    got = _forward(tiny["net"], tiny["dev"], tiny["wide"], torch.ones_like(tiny["counts"]), tiny["tables"])
    assert torch.equal(got, tiny["plain"]), "announced with every count 1, the forward must be the plain forward on the same 77-token prompts"


@pytest.mark.parametrize("how", ["cached", "ctx_len", "mixed", "image_tokens"])
def test_refusals(tiny, how):
    from sduss_amd.lib import MxError      # (the library's block-cache and patch-parallel entry points: tests/test_regions_cpu.py)
    net, (s, t, e, te, ti) = tiny["net"], tiny["dev"]
    net.set_regions(tiny["counts"], tiny["tables"])
    with pytest.raises(MxError, match="image|region"):
        if how == "cached":
            net.forward_one_cached(object(), s, t, tiny["wide"], te, ti)
        elif how == "ctx_len":
            net.forward_one(s, t, e, te, ti)
        elif how == "mixed":
            net.set_regions(torch.cat([tiny["counts"]] * 2), [torch.cat([w] * 2) for w in tiny["tables"]])
            net.forward_mixed([s[:, :, :16, :16].contiguous(), s], torch.cat([t, t]), torch.cat([tiny["wide"]] * 2), torch.cat([te, te]), torch.cat([ti, ti]))
        else:
            net._ip_next = (torch.zeros(2, 16, e.shape[2], dtype=torch.bfloat16, device="cuda"), torch.ones(2, device="cuda"))
            net.forward_one(s, t, tiny["wide"], te, ti)
    assert torch.equal(_forward(net, tiny["dev"]), tiny["plain"]), "a refused announcement must not reach the next forward"


def test_denoiser_step_with_a_regional_and_a_plain_request(tiny):
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    den, gen = SDXLDenoiser(tiny["net"]), torch.Generator().manual_seed(3)
    embeds = torch.randn(2, 77, tiny["cfg"].cross_attention_dim, generator=gen).bfloat16()
    masks = torch.zeros(2, 32, 32, dtype=torch.bool)
    masks[0, :, :16], masks[1, :, 16:] = True, True

    def step(regional):
        reqs = [synthetic_request(i, 256, 4, tiny["cfg"], den, "cuda:0") for i in range(2)]
        if regional:
            den.set_regions(reqs[0], embeds, masks)
        den.denoising_step({"256": reqs})
        return reqs
    plain, got = step(False), step(True)
    assert torch.equal(got[1].latents, plain[1].latents) and not torch.equal(got[0].latents, plain[0].latents)
