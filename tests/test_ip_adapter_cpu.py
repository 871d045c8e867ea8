"""Host side of the image-prompt adapter: IPAdapter.from_state_dict and project, and the step plan's dry walks with an adapter set.  No GPU."""
import ctypes as C

import pytest
import torch

import ip_ref
from oracle import sdxl_unet_ref as ref  # (parameters only)
from sduss_amd import lib, weights
from sduss_amd.config import UNetConfig
from sduss_amd.ip_adapter import IPAdapter, cross_attention_layers
from sduss_amd.unet import config_c

CFG = UNetConfig.tiny()
K0 = "down_blocks.1.attentions.0.transformer_blocks.0.attn2.processor.to_k_ip.0.weight"


@pytest.mark.parametrize("prefix", ["unet.", ""])
def test_packed_layers_follow_the_text_projection_order(prefix):
    """an adapter whose to_k_ip / to_v_ip ARE the net's attn2.to_k / to_v must pack to the net's own attn2_kv_all tensors"""
    P = ref.init_params(ref.UNetConfig.tiny())
    sd = ip_ref.random_adapter_sd(CFG, 1, prefix=prefix)
    for b, _dim in cross_attention_layers(CFG):
        for nm in ("k", "v"):
            sd[f"{prefix}{b}.attn2.processor.to_{nm}_ip.0.weight"] = P[f"{b}.attn2.to_{nm}.weight"]
    ad = IPAdapter.from_state_dict(CFG, sd)
    text = {n: t for n, t in weights.pack(CFG, P) if n.startswith("attn2_kv_all.")}
    assert ad.n_img == 4 and [n for n, _ in ad.packed] == [n.replace("attn2_kv_all", "ip_kv_all") for n in text]
    for n, t in ad.packed:
        assert t.dtype == torch.bfloat16 and torch.equal(t, text[n.replace("ip_kv_all", "attn2_kv_all")])


@pytest.mark.parametrize("how,exc", [("missing", KeyError), ("shape", ValueError), ("tokens", ValueError)])
def test_from_state_dict_refuses_naming_the_tensor(how, exc):
    sd = ip_ref.random_adapter_sd(CFG, 2, n_img=17 if how == "tokens" else 4, prefix="")
    if how == "missing":
        del sd[K0]
    if how == "shape":
        sd[K0] = sd[K0][:, :-1]
    with pytest.raises(exc, match="image_embeds.weight" if how == "tokens" else "to_k_ip"):
        IPAdapter.from_state_dict(CFG, sd)


def test_project_pads_caller_made_tokens():
    ad = IPAdapter.from_state_dict(CFG, ip_ref.random_adapter_sd(CFG, 3, n_img=4))
    tok = torch.randn(3, 4, CFG.cross_attention_dim)
    out = ad.project(tok)
    assert out.shape == (3, 16, CFG.cross_attention_dim) and torch.equal(out[:, :4], tok.bfloat16()) and not out[:, 4:].any()
    with pytest.raises(ValueError):
        ad.project(torch.randn(3, 5, CFG.cross_attention_dim))


def test_dry_walks_account_for_the_adapter():
    l, pw = lib.load(), weights.PackedWeights(weights.pack(CFG, ref.init_params(ref.UNetConfig.tiny())), "cpu")
    h = l.mx_unet_create(C.byref(config_c(CFG)))
    assert h and l.mx_unet_set_weights(h, pw.blob.data_ptr(), pw.blob.numel(), pw.table, len(pw.names)) == 0
    plain = l.mx_unet_workspace_bytes(h, 2, 32, 32, 77)
    ad = IPAdapter.from_state_dict(CFG, ip_ref.random_adapter_sd(CFG, 4))
    ip = weights.PackedWeights(ad.packed, "cpu")
    assert l.mx_unet_set_ip_adapter(h, ip.blob.data_ptr(), ip.blob.numel(), ip.table, len(ip.names), ad.n_img) == 0
    assert l.mx_unet_validate(h, 2, 32, 32, 77) == 0, l.mx_last_error()
    assert l.mx_unet_workspace_bytes(h, 2, 32, 32, 77) > plain > 0
    assert l.mx_unet_set_ip_adapter(h, ip.blob.data_ptr(), ip.blob.numel(), ip.table, 1, ad.n_img) == 0      # a table that lacks a width: the walk names it
    assert l.mx_unet_validate(h, 2, 32, 32, 77) != 0 and b"ip_kv_all.256.weight" in l.mx_last_error()
    for name in ("mx_unet_forward_cached", "mx_unet_forward_cached_mixed", "mx_unet_forward_pp", "mx_unet_forward_pp_stale"):      # announced: refused at once
        assert l.mx_unet_set_image_tokens(h, 4096, 4096) == 0
        args = [h] + [0 if a in (C.c_int, C.c_size_t) else None for a in lib.SYMBOLS[name][1][1:]]
        assert getattr(l, name)(*args) != 0 and b"image prompt" in l.mx_last_error(), name
    assert l.mx_unet_set_ip_adapter(h, None, 0, None, 0, 0) == 0 and l.mx_unet_workspace_bytes(h, 2, 32, 32, 77) == plain
    l.mx_unet_destroy(h)
