"""Host-side checks of the VAE encoder path: the rotation identity the plan rests on (through the packer's own rotated weights), the start step of an
image-to-image request, the conv_in packing, and the plan's weight inventory walked on the host.  No GPU."""
import ctypes as C

import pytest
import torch

import vae_encode_ref as E
from oracle import vae_ref


def unpack_encoder(cfg, packed):
    """packed tensors of pack_vae_encoder -> HF-shaped params again (still rotated: what the plan convolves with)"""
    m = 2 * cfg.latent_channels
    P = {}
    for name, t in packed:
        t = t.to(torch.float64)
        if name == "encoder.conv_in.weight":
            P[name] = t[:, :27].reshape(-1, 3, 3, 3).permute(0, 3, 1, 2)
        elif name.startswith("quant_conv."):
            P[name] = t[:m, :m].reshape(m, m, 1, 1) if t.ndim == 2 else t[:m]
        elif name.startswith("encoder.conv_out."):
            P[name] = t[:m].reshape(m, 3, 3, -1).permute(0, 3, 1, 2) if t.ndim == 2 else t[:m]
        elif name.endswith("conv_shortcut.weight"):
            P[name] = t.reshape(*t.shape, 1, 1)
        elif t.ndim == 2 and ".attentions." not in name:
            P[name] = t.reshape(t.shape[0], 3, 3, -1).permute(0, 3, 1, 2)
        else:
            P[name] = t
    return P


def test_rotated_plan_equals_the_plain_encoder():
    """conv(pad(x, (0, 1, 0, 1)), w, stride 2, pad 0) == rot(conv(rot(x), rot(w), stride 2, pad 1)) through the whole graph: the packer's rotated
    weights, unpacked, run with pad-1 downsamplers on the rotated image, give the rotated moments of the plain encoder.  Non-square, fp64, 1e-12."""
    from sduss_amd.vae import VAEConfig, pack_vae_encoder, rot180
    ocfg = vae_ref.VAEConfig.tiny()
    P = E.init_params(ocfg)
    x = torch.rand(2, 3, 24, 40, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 2 - 1
    want = E.moments(P, ocfg, x)
    assert want.shape == (2, 8, 6, 10) and want.dtype == torch.float64
    Pr = unpack_encoder(ocfg, pack_vae_encoder(VAEConfig.tiny(), P))
    assert set(Pr) == set(P) and all(Pr[k].shape == P[k].shape for k in P)
    got = rot180(E.moments(Pr, ocfg, rot180(x), pad1_downsample=True))
    assert float((got - want).abs().max()) <= 1e-12
    # the two ways to get it wrong must not pass: rotated weights without rotating the image back, and the pad-1 downsampler on plain weights
    assert float((rot180(got) - want).abs().max()) > 1e-3
    assert float((E.moments(P, ocfg, x, pad1_downsample=True) - want).abs().max()) > 1e-3


@pytest.mark.parametrize("steps,strength,want", [
    (50, 0.0, 50), (50, 1.0, 0), (50, 0.3, 35), (50, 0.5, 25), (30, 0.8, 6), (20, 0.05, 19), (10, 0.29, 8),   # int(2.9) = 2
    (50, 0.58, 22),            # 50 * 0.58 = 28.999999999999996: int() cuts to 28, as diffusers does
    (100, 0.29, 72),           # 100 * 0.29 = 28.999999999999996
    (7, 0.999, 1), (1, 0.99, 1), (1, 1.0, 0), (4, 1.5, 0),
])
def test_start_step_follows_get_timesteps(steps, strength, want):
    from sduss_amd.pipeline import start_step
    assert start_step(steps, strength) == want


def test_conv_in_pack_columns():
    from sduss_amd.vae import VAEConfig, conv_in_pack, pack_vae_encoder, rot180
    n = 16
    w = torch.arange(n * 27, dtype=torch.float32).reshape(n, 3, 3, 3)          # [O, I, kh, kw]
    p = conv_in_pack(w)
    assert p.shape == (n, 32) and p.is_contiguous()
    for o, c, ky, kx in ((0, 0, 0, 0), (3, 2, 1, 0), (15, 1, 2, 2), (7, 0, 2, 1)):
        assert p[o, (ky * 3 + kx) * 3 + c] == w[o, c, ky, kx]
    assert bool((p[:, 27:] == 0).all()) and sorted(p[:, :27].reshape(-1).tolist()) == w.reshape(-1).tolist()
    # in the packed encoder: the rotated weight, bf16, [N, 32]; tap (ky, kx) holds the plain weight's tap (2 - ky, 2 - kx)
    ocfg = vae_ref.VAEConfig.tiny()
    P = E.init_params(ocfg)
    packed = dict(pack_vae_encoder(VAEConfig.tiny(), P))
    q = packed["encoder.conv_in.weight"]
    assert q.dtype == torch.bfloat16 and q.shape == (64, 32) and bool((q[:, 27:] == 0).all())
    assert torch.equal(q.float(), conv_in_pack(rot180(P["encoder.conv_in.weight"])))
    assert q[5, (0 * 3 + 2) * 3 + 1].float() == P["encoder.conv_in.weight"][5, 1, 2, 0]


def test_encoder_plan_resolves_packed_weights_on_host():
    """mx_vae_encode_validate walks the encoder plan on the host: every name / size it asks for is what pack_vae_encoder produced, for the SDXL
    form (with quant_conv), the SD3 form (without) and the real widths; a missing tensor and the refusals are reported without a GPU."""
    from dataclasses import replace
    from sduss_amd import lib, weights
    from sduss_amd.vae import VAEConfig, _config_c, pack_vae_encoder
    l = lib.load()
    cases = ((VAEConfig.tiny(), vae_ref.VAEConfig.tiny()), (VAEConfig.sdxl(), vae_ref.VAEConfig.sdxl()),
             (replace(VAEConfig.sd3(), block_out_channels=(64, 64, 128), layers_per_block=1), vae_ref.VAEConfig.tiny_sd3()))
    for cfg, ocfg in cases:
        P = {k: torch.zeros(v) for k, v in E.param_shapes(ocfg).items()}
        packed = pack_vae_encoder(cfg, P)
        pw = weights.PackedWeights(packed, "cpu")
        h = l.mx_vae_create(C.byref(_config_c(cfg)))
        assert h and l.mx_vae_set_weights(h, pw.blob.data_ptr(), pw.blob.numel(), pw.table, len(pw.names)) == 0
        f = 2 ** (len(cfg.block_out_channels) - 1)
        assert l.mx_vae_encode_validate(h, 2, 8 * f, 16 * f) == 0, l.mx_last_error()
        assert l.mx_vae_encode_workspace_bytes(h, 2, 8 * f, 16 * f) > 0
        assert l.mx_vae_encode_validate(h, 1, 8 * f + f // 2, 16 * f) != 0 and b"multiples of" in l.mx_last_error()
        assert l.mx_vae_encode_workspace_bytes(h, 1, 8 * f, 16 * f + 1) == 0
        bad = [e for e in packed if e[0] != "encoder.mid_block.attentions.0.to_k.bias"]
        pw2 = weights.PackedWeights(bad, "cpu")
        assert l.mx_vae_set_weights(h, pw2.blob.data_ptr(), pw2.blob.numel(), pw2.table, len(pw2.names)) == 0
        assert l.mx_vae_encode_validate(h, 1, 8 * f, 8 * f) != 0 and b"to_k.bias" in l.mx_last_error()
        l.mx_vae_destroy(h)
    # an image has three channels
    cc = _config_c(replace(VAEConfig.tiny(), out_channels=4))
    h = l.mx_vae_create(C.byref(cc))
    assert h and l.mx_vae_encode_workspace_bytes(h, 1, 32, 32) == 0 and b"out_channels == 3" in l.mx_last_error()
    l.mx_vae_destroy(h)
    # SDXL VAE encoder: 34.2 M parameters
    total = sum(torch.Size(v).numel() for v in E.param_shapes(vae_ref.VAEConfig.sdxl()).values())
    assert 34.0e6 < total < 34.5e6, total


def test_operators_refuse_bad_arguments_without_a_launch():
    from sduss_amd import lib
    l = lib.load()
    ok = 4096                # any aligned non-null address: nothing is dereferenced before the refusal
    for args, msg in (((None, 0, ok, ok, ok, 1, 4, 16, 64, 0), b"null"), ((ok, 0, ok, ok, ok, 1, 0, 16, 64, 0), b"positive"),
                      ((ok, 0, ok, ok, ok, 1, 4, 16, 72, 0), b"multiple of 16"), ((ok, 2, ok, ok, ok, 1, 4, 16, 64, 0), b"image_format"),
                      ((ok, 0, ok, ok, ok, 1, 4, 16, 64, 2), b"rotate"), ((ok, 0, ok + 8, ok, ok, 1, 4, 16, 64, 0), b"aligned"),
                      ((ok, 1, ok, ok, ok, 1, 4, 16, 64, 0), None), ((ok + 2, 1, ok, ok, ok, 1, 4, 16, 64, 0), b"4-byte"),
                      ((ok, 0, ok, ok, ok, 4, 16384, 16384, 64, 0), b"32-bit")):
        if msg is None:
            continue         # (a well-formed call would launch: not made here)
        assert l.mx_conv3x3_rgb_in(None, *args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    for args, msg in (((None, 64, ok, 2, 1, 4, 3, 5, 1.0, 0.0, None, None, None, None, 0), b"null"),
                      ((ok, 7, ok, 2, 1, 4, 3, 5, 1.0, 0.0, None, None, None, None, 0), b"ld must"),
                      ((ok, 64, ok, 2, 1, 4, 3, 5, 1.0, 0.0, None, ok, None, None, 0), b"keep and sigma"),
                      ((ok, 64, ok, 2, 0, 4, 3, 5, 1.0, 0.0, None, None, None, None, 0), b"positive"),
                      ((ok, 64, ok, 2, 1, 4, 3, 5, 1.0, 0.0, None, None, None, None, 3), b"rotate")):
        assert l.mx_vae_latent_finish(None, *args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
