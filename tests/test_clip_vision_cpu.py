"""The CLIP vision encoder's host side, no GPU: pack_clip_vision, the refusals of mx_clip_vision_create, the dry sizing / validating walks."""
import ctypes as C

import pytest
import torch

from sduss_amd import lib
from sduss_amd.clip_vision import CLIPVisionConfig, synthetic_clip_vision_params
from sduss_amd.weights import PackedWeights, clip_vision_ldw, pack_clip_vision


def _config_c(cfg, heads=None):
    cc = lib.CLIPVisionConfigC()
    cc.hidden_size, cc.intermediate_size, cc.num_hidden_layers, cc.num_attention_heads = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, heads or cfg.num_attention_heads
    cc.image_size, cc.patch_size, cc.projection_dim, cc.layer_norm_eps, cc.hidden_act = cfg.image_size, cfg.patch_size, cfg.projection_dim, cfg.layer_norm_eps, 0
    cc.image_mean, cc.image_std = (C.c_float * 3)(*cfg.image_mean), (C.c_float * 3)(*cfg.image_std)
    return cc


def test_pack_names_shapes_and_patch_order():
    cfg = CLIPVisionConfig.tiny()
    P = synthetic_clip_vision_params(cfg)
    packed = dict(pack_clip_vision(cfg, P))
    h, p, layer = cfg.hidden_size, cfg.patch_size, "vision_model.encoder.layers.1."
    want = {"vision_model.embeddings.class_embedding": ((h,), torch.bfloat16), "vision_model.embeddings.position_embedding.weight": ((cfg.tokens, h), torch.bfloat16),
            "vision_model.embeddings.patch_embedding.weight": ((h, clip_vision_ldw(p)), torch.bfloat16), "vision_model.pre_layrnorm.bias": ((h,), torch.float32),
            layer + "self_attn.qkv_proj.weight": ((3 * h, h), torch.bfloat16), layer + "self_attn.qkv_proj.bias": ((3 * h,), torch.float32),
            layer + "mlp.fc1.weight": ((cfg.intermediate_size, h), torch.bfloat16), "visual_projection.weight": ((cfg.projection_dim, h), torch.bfloat16)}
    for name, (shape, dtype) in want.items():
        assert tuple(packed[name].shape) == shape and packed[name].dtype == dtype, name
    assert not any("q_proj" in n or "position_ids" in n for n in packed) and len(packed) == len(P) - 4 * cfg.num_hidden_layers
    a = layer + "self_attn."
    assert torch.equal(packed[a + "qkv_proj.weight"].float(), torch.cat([P[a + n + "_proj.weight"] for n in "qkv"]))      # bf16-exact values: nothing re-rounded
    # the flattening order: one random patch convolved both ways in fp64; the padding exactly zero
    w, flat = P["vision_model.embeddings.patch_embedding.weight"].double(), packed["vision_model.embeddings.patch_embedding.weight"].double()
    patch = torch.randn(p, p, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))                          # (row, column, channel): interleaved RGB
    conv = torch.nn.functional.conv2d(patch.permute(2, 0, 1)[None], w)[0, :, 0, 0]
    assert (flat[:, :3 * p * p] @ patch.reshape(-1) - conv).abs().max() <= 1e-12
    assert clip_vision_ldw(14) == 608 and not flat[:, 3 * p * p:].any()


@pytest.mark.parametrize("heads", [2, 8, 10])        # 320 / heads = 160, 40, 32
def test_create_refuses_other_head_widths(heads):
    l = lib.load()
    assert not l.mx_clip_vision_create(C.byref(_config_c(CLIPVisionConfig.tiny(), heads)))
    assert f"heads of {320 // heads}".encode() in l.mx_last_error()


@pytest.mark.parametrize("head_dim", [80, 64])
def test_dry_walks_need_no_device(head_dim):
    l, cfg = lib.load(), CLIPVisionConfig.tiny(head_dim)
    h = l.mx_clip_vision_create(C.byref(_config_c(cfg)))
    assert h, l.mx_last_error()
    w = PackedWeights(pack_clip_vision(cfg, synthetic_clip_vision_params(cfg)), "cpu")
    assert l.mx_clip_vision_set_weights(h, w.blob.data_ptr(), w.blob.numel(), w.table, len(w.names)) == 0
    assert l.mx_clip_vision_validate(h, 2) == 0, l.mx_last_error()
    one, two = l.mx_clip_vision_workspace_bytes(h, 1), l.mx_clip_vision_workspace_bytes(h, 2)
    assert 0 < one < two
    assert l.mx_clip_vision_set_weights(h, w.blob.data_ptr(), w.blob.numel(), w.table, len(w.names) - 1) == 0     # a table that lacks a tensor: the walk names it
    assert l.mx_clip_vision_validate(h, 2) != 0 and b"missing weight" in l.mx_last_error()
    l.mx_clip_vision_destroy(h)
