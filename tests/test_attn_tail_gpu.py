"""The attention tail of a BasicTransformerBlock (attn1.to_out + residual -> norm2 folded into attn2.to_q -> the 77-key cross-attention -> attn2.to_out +
residual; modules/transformer.py:204-262, modules/attention.py:59-110) as the step plan issues it: four launches, the first projection's slab statistics
feeding the folded norm2, the last writing slab (and, on 256-row tiles, finalised) statistics.  A torch fp32 evaluation of the same four ops bounds the
arithmetic."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rt(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _problem(b, heads, L, ctx_len=77, seed=0):
    from sduss_amd import ops
    from sduss_amd.weights import fold_layernorm
    g = torch.Generator().manual_seed(seed + b + heads + L)
    c = heads * 64
    m = b * L
    ao = _rt(torch.randn(m, c, generator=g))
    y = _rt(torch.randn(m, c, generator=g) * (0.5 + torch.rand(m, 1, generator=g)) + 0.5 * torch.randn(m, 1, generator=g))
    lin = lambda: (_rt(torch.randn(c, c, generator=g) * c ** -0.5), 0.1 * torch.randn(c, generator=g))
    (w1, b1), (wq, bq), (w2, b2) = lin(), lin(), lin()
    gamma, beta = 1.0 + 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    wqf, colsum, bqf = fold_layernorm(wq, bq, gamma, beta)
    k = _rt(torch.randn(b, ctx_len, c, generator=g))
    v = _rt(torch.randn(b, ctx_len, c, generator=g))
    dev = lambda t: t.cuda()
    bf = lambda t: t.to(torch.bfloat16).cuda()
    host = dict(ao=ao, y=y, w1=w1, b1=b1, wq=wq, bq=bq, gamma=gamma, beta=beta, w2=w2, b2=b2, k=k, v=v)
    args = dict(ao=bf(ao), y=bf(y), w1=bf(w1), b1=dev(b1), wq=wqf.cuda(), bq=dev(bqf), colsum_q=dev(colsum), k=bf(k.reshape(b * ctx_len, c)),
                vt=ops.pack_vt(bf(v), pad=float("nan")), w2=bf(w2), b2=dev(b2), heads=heads, L=L, ctx_len=ctx_len)
    return host, args


@pytest.mark.parametrize("b,heads,L,finalise", [(8, 20, 1024, True),      # the 60 layers at 32 x 32 of the headline batch: 256 x 160 tiles, slab + finalised statistics
                                                (8, 10, 4096, True),      # the 10 layers at 64 x 64: 256 x 160 tiles, slab + finalised statistics
                                                (2, 20, 1024, False)])    # one request: M 2048 on 128-row tiles, the split statistics path
def test_attn_tail_within_fp32_bound(cuda_device, b, heads, L, finalise):
    from sduss_amd import ops
    host, args = _problem(b, heads, L)
    y, _st, _final, _q2, _ao2 = ops.attn_tail(**args, finalise=finalise)
    # the arithmetic itself against torch fp32 (the bound of three bf16-stored linears and one attention: 2^-6 of the range)
    c = heads * 64
    y1 = host["ao"] @ host["w1"].t() + host["b1"] + host["y"]
    y1 = _rt(y1)
    q2 = F.layer_norm(y1, (c,), host["gamma"], host["beta"], 1e-5) @ host["wq"].t() + host["bq"]
    qh = q2.reshape(b, L, heads, 64).transpose(1, 2)
    kh = host["k"].reshape(b, -1, heads, 64).transpose(1, 2)
    vh = host["v"].reshape(b, -1, heads, 64).transpose(1, 2)
    a2 = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(b * L, c)
    want = a2 @ host["w2"].t() + host["b2"] + y1
    err = (y.float().cpu() - want).abs().max().item() / want.abs().max().item()
    print(f"attn_tail B{b} H{heads} L{L}: max err vs torch fp32 {err:.5f} of range")
    assert err <= 2.0 ** -6
