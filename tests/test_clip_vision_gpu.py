"""The CLIP vision encoder on the device: mx_attention_d80 and mx_patch_embed_u8 one launch at a time against per-element fp64 bounds (kernel_ref.py),
the whole encoder against the fp64 restatement within twice the error of a stock bf16 evaluation of the same graph, and
Denoiser.set_image_prompt(image=..., encoder=...)."""
import types

import pytest
import torch

import clip_vision_ref as cref
import kernel_ref as kr

pytestmark = pytest.mark.gpu

HEADS, D = 3, 80


def _qkv(L, seed):
    """q, k, v as three column ranges of ONE [M, 3 * 240] buffer, the shape the encoder's q | k | v GEMM leaves"""
    buf = torch.randn(2 * L, 3 * HEADS * D, generator=torch.Generator().manual_seed(seed)).bfloat16().cuda()
    return buf, [buf[:, i * HEADS * D:(i + 1) * HEADS * D] for i in range(3)]


@pytest.mark.parametrize("L", [1, 15, 64, 65, 257, 480])     # single key, sub-tile, exact tile, one row over, the model's ragged length, the longest served
def test_attention_d80_vs_fp64(cuda_device, L):
    from sduss_amd import lib, ops
    assert lib.ATTN_D80_MAX_L == 480
    _buf, (q, k, v) = _qkv(L, L)
    guard, out = kr.guarded(2 * L, HEADS * D, HEADS * D, torch.bfloat16, "cuda")
    ops.attention_d80(q, k, v, HEADS, 2, out=out)
    assert kr.guard_violations(guard, 2 * L, HEADS * D) == 0, "rows after the last query row were written"
    for b in range(2):
        for h in range(HEADS):
            r, c = slice(b * L, (b + 1) * L), slice(h * D, (h + 1) * D)
            ref, bound = cref.attention_ref(q[r, c], k[r, c], v[r, c])
            kr.assert_within(out[r, c], ref, bound, f"L={L} batch {b} head {h}")


def test_attention_d80_refuses_longer_sequences(cuda_device):
    from sduss_amd import lib
    L = lib.ATTN_D80_MAX_L + 1
    _buf, (q, k, v) = _qkv(L, 7)
    guard, out = kr.guarded(2 * L, HEADS * D, HEADS * D, torch.bfloat16, "cuda")      # every row, the output's own included, keeps the guard pattern
    l = lib.load()
    assert l.mx_attention_d80(lib.current_stream(), q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), out.data_ptr(),
                              HEADS * D, 2, HEADS, L) != 0
    assert b"480" in l.mx_last_error()
    torch.cuda.synchronize()
    assert kr.guard_violations(guard, 0, HEADS * D) == 0, "a refused call must launch nothing"


@pytest.mark.parametrize("case", ["whole_tiles", "ragged_crop"])
def test_patch_embed_u8_vs_fp64(cuda_device, case):
    from sduss_amd import ops
    from sduss_amd.clip_vision import CLIP_MEAN, CLIP_STD
    from sduss_amd.weights import clip_vision_ldw
    g = torch.Generator().manual_seed(3)
    P, N, B = 14, 64, 2
    if case == "whole_tiles":                         # 224 x 224: 256 patches, whole 16-patch tiles
        img = torch.randint(0, 256, (B, 224, 224, 3), generator=g, dtype=torch.uint8).cuda()
    else:                                             # 42 x 70 (3 x 5 patches: a ragged tile) cut out of 60 x 100 whose margin is one sentinel byte
        big = torch.full((B, 60, 100, 3), 0xEE, dtype=torch.uint8)
        big[:, 7:49, 11:81] = torch.randint(0, 256, (B, 42, 70, 3), generator=g, dtype=torch.uint8)
        img = big.cuda()[:, 7:49, 11:81]
    T = 1 + (img.shape[1] // P) * (img.shape[2] // P)
    w = torch.zeros(N, clip_vision_ldw(P)).bfloat16()
    w[:, :3 * P * P] = (torch.randn(N, 3 * P * P, generator=g) * (3 * P * P) ** -0.5).bfloat16()
    cls, pos = torch.randn(N, generator=g).bfloat16().cuda(), torch.randn(T, N, generator=g).bfloat16().cuda()
    w = w.cuda()
    guard, out = kr.guarded(B * T, N, N, torch.bfloat16, "cuda")
    got = ops.patch_embed_u8(img, w, cls, pos, P, CLIP_MEAN, CLIP_STD, out=out.view(B, T, N))
    assert kr.guard_violations(guard, B * T, N) == 0
    a = cref.patches(cref.normalise(img, CLIP_MEAN, CLIP_STD), P)
    ref, bound = kr.epilogue_ref(*kr.gemm_acc(a, w[:, :3 * P * P]), residual=pos[1:].repeat(B, 1))
    kr.assert_within(got[:, 1:].reshape(-1, N), ref, bound, case)
    assert torch.equal(got[:, 0], (cls.float() + pos[0].float()).bfloat16().expand(B, N)), "the class row is one bf16 rounding of an fp32 sum"


@pytest.mark.parametrize("head_dim,act", [(80, "quick_gelu"), (80, "gelu"), (64, "quick_gelu"), (64, "gelu")])
def test_encoder_within_twice_the_stock_bf16_error(cuda_device, head_dim, act):
    from sduss_amd.clip_vision import CLIPVisionConfig, MxCLIPVision, synthetic_clip_vision_params
    cfg = CLIPVisionConfig.tiny(head_dim, act)
    P = synthetic_clip_vision_params(cfg)
    images = torch.randint(0, 256, (2, 56, 56, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    ours = MxCLIPVision(cfg, P).encode(images, hidden_states=True)
    ref = cref.vit_forward(cfg, P, images, torch.float64)
    stock = cref.vit_forward(cfg, P, images, torch.bfloat16)
    for name, o, r, s in zip(("image_embeds", "hidden_states[-2]"), ours, ref, stock):
        e_o, e_s = (o.double() - r).abs(), (s.double() - r).abs()
        fig = [e_o.max().item(), e_s.max().item(), e_o.square().mean().sqrt().item(), e_s.square().mean().sqrt().item()]
        print(f"heads of {head_dim}, {act}, {name}: max err ours {fig[0]:.3e} stock {fig[1]:.3e} (ratio {fig[0] / fig[1]:.2f}); "
              f"rms ours {fig[2]:.3e} stock {fig[3]:.3e} (ratio {fig[2] / fig[3]:.2f})")
        assert fig[0] <= 2 * fig[1] and fig[2] <= 2 * fig[3], f"{name}: further from fp64 than twice the stock bf16 evaluation"


def test_set_image_prompt_takes_the_image(cuda_device):
    import ip_ref
    from oracle import sdxl_unet_ref as ref
    from sduss_amd.clip_vision import CLIPVisionConfig, MxCLIPVision, synthetic_clip_vision_params
    from sduss_amd.config import UNetConfig
    from sduss_amd.ip_adapter import IPAdapter
    from sduss_amd.lib import MxError
    from sduss_amd.pipeline import SDXLDenoiser
    from sduss_amd.unet import MxUNet
    cfg, vcfg = UNetConfig.tiny(), CLIPVisionConfig.tiny()
    net = MxUNet(cfg, ref.init_params(ref.UNetConfig.tiny()), device="cuda:0")
    net.set_ip_adapter(IPAdapter.from_state_dict(cfg, ip_ref.random_adapter_sd(cfg, 31, n_img=4, embed_dim=vcfg.projection_dim)))
    den, enc = SDXLDenoiser(net), MxCLIPVision(vcfg, synthetic_clip_vision_params(vcfg))
    image = torch.randint(0, 256, (1, 90, 131, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).cuda()     # resized and cropped on the way
    a, b = types.SimpleNamespace(), types.SimpleNamespace()
    den.set_image_prompt(a, image=image, encoder=enc, scale=0.7)
    den.set_image_prompt(b, enc.encode_images(image), 0.7)
    assert torch.equal(a.image_tokens, b.image_tokens) and a.ip_scale == b.ip_scale == 0.7
    with pytest.raises(MxError, match="not both"):
        den.set_image_prompt(a, enc.encode_images(image), image=image, encoder=enc)
    with pytest.raises(MxError, match="encoder"):
        den.set_image_prompt(a, image=image)
