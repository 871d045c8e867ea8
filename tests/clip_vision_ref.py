"""Plain torch restatement of transformers' CLIPVisionModelWithProjection and of softmax(Q K^T / sqrt d) V, for tests/test_clip_vision_*.py.  Evaluated in
float64 it is the reference; evaluated in bfloat16 it is the stock evaluation of the same graph whose error is the yardstick.
Both start from the values the kernels receive: bf16-representable weights and the image normalised in fp32, operation by operation, rounded once."""
import math

import torch
import torch.nn.functional as F

from kernel_ref import U32


def normalise(images, mean, std):
    """uint8 [B, H, W, 3] -> bf16: (u / 255 - mean) / std, every operand a tensor so that each step is one fp32 operation"""
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=images.device)
    return ((images.float() / t(255.0) - t(mean)) / t(std)).bfloat16()


def patches(x, p):
    """[B, H, W, 3] -> [B * (H/p) * (W/p), 3 p p], columns in (row, column, channel) order"""
    b, h, w, _ = x.shape
    return x.reshape(b, h // p, p, w // p, p, 3).permute(0, 1, 3, 2, 4, 5).reshape(b * (h // p) * (w // p), 3 * p * p)


def vit_forward(cfg, P, images, dtype):
    """(image_embeds [B, projection_dim], hidden_states[-2] [B, tokens, H]) in ``dtype``"""
    P = {k: v.to(device=images.device, dtype=dtype) for k, v in P.items()}
    vm, eps, h = "vision_model.", cfg.layer_norm_eps, cfg.hidden_size
    ln = lambda x, n: F.layer_norm(x, (h,), P[n + ".weight"], P[n + ".bias"], eps)
    lin = lambda x, n: F.linear(x, P[n + ".weight"], P[n + ".bias"])
    act = (lambda x: x * torch.sigmoid(1.702 * x)) if cfg.hidden_act == "quick_gelu" else F.gelu
    xn = normalise(images, cfg.image_mean, cfg.image_std).to(dtype).permute(0, 3, 1, 2)
    x = F.conv2d(xn, P[vm + "embeddings.patch_embedding.weight"], stride=cfg.patch_size).flatten(2).transpose(1, 2)
    x = torch.cat([P[vm + "embeddings.class_embedding"].expand(x.shape[0], 1, h), x], dim=1) + P[vm + "embeddings.position_embedding.weight"]
    x = ln(x, vm + "pre_layrnorm")
    states = [x]
    for l in range(cfg.num_hidden_layers):
        p = f"{vm}encoder.layers.{l}."
        y = ln(x, p + "layer_norm1")
        q, k, v = (lin(y, p + f"self_attn.{n}_proj").unflatten(2, (cfg.num_attention_heads, -1)).transpose(1, 2) for n in "qkv")
        x = x + lin(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).flatten(2), p + "self_attn.out_proj")
        x = x + lin(act(lin(ln(x, p + "layer_norm2"), p + "mlp.fc1")), p + "mlp.fc2")
        states.append(x)
    return F.linear(ln(x[:, 0], vm + "post_layernorm"), P["visual_projection.weight"]), states[-2]


def attention_ref(q, k, v):
    """softmax(q k^T / sqrt d) v of one head in fp64 from bf16 q, k, v [L, d], with kernel_ref.attention_ref's per-element bound for d products per score:
    P rounded to bf16 before P V (2^-7 P |V|), fp32 scores in the log2 domain (2 ln 2 d 2^-23 c max_j |q_i| |k_j| P |V|), the bf16 output rounding."""
    q64, k64, v64 = q.double(), k.double(), v.double()
    d = q.shape[1]
    c = math.log2(math.e) / math.sqrt(d)
    p = torch.softmax(q64 @ k64.t() / math.sqrt(d), dim=1)
    ref, pv = p @ v64, p @ v64.abs()
    e_score = d * 2 * U32 * c * (q64.abs() @ k64.abs().t()).max(dim=1, keepdim=True).values
    e = 2.0 ** -7 * pv + 2.0 * math.log(2.0) * e_score * pv
    return ref, e + 2.0 ** -8 * (ref.abs() + e)
