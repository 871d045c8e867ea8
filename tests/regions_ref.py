"""Checker side of the regional-prompt tests: the blend of kernel_ref.attention_ref over a sample's sets with its per-element bound, and the oracle's
BasicTransformerBlock with a regional attn2 in fp32 (installed over oracle.sdxl_unet_ref.basic_transformer_block with pytest's monkeypatch)."""
import torch
import torch.nn.functional as F

import kernel_ref as R


def blend_ref(q, ks, vs, ws):
    """sum_r w_r[:, None] * attention(q, k_r, v_r) and the bound sum_r |w_r| * bound_r; q [Lq, 64], ks / vs lists of [seg, 64] bf16, ws fp32 [len, Lq]"""
    terms = [R.attention_ref(q, k, v, 1.0) for k, v in zip(ks, vs)]
    w = ws.double().unsqueeze(2)
    return sum(w[r] * t[0] for r, t in enumerate(terms)), sum(w[r].abs() * t[1] for r, t in enumerate(terms))


def block_with_regions(ref, counts, tables, seg_len, seg_ld):      # attn2 = sum_r w_r softmax(q k_r^T) v_r on the sets of the wide context; w by token count
    by_tokens = {t.shape[2]: t for t in tables}

    def block(P, b, x, ctx, heads, cfg):
        dim, eps = x.shape[-1], cfg.layer_norm_eps
        ln = lambda i: F.layer_norm(x, (dim,), P[f"{b}.norm{i}.weight"], P[f"{b}.norm{i}.bias"], eps)
        n = ln(1)
        a = ref.attention(F.linear(n, P[f"{b}.attn1.to_q.weight"]), F.linear(n, P[f"{b}.attn1.to_k.weight"]), F.linear(n, P[f"{b}.attn1.to_v.weight"]), heads)
        x = F.linear(a, P[f"{b}.attn1.to_out.0.weight"], P[f"{b}.attn1.to_out.0.bias"]) + x
        q, w = F.linear(ln(2), P[f"{b}.attn2.to_q.weight"]), by_tokens[x.shape[1]].to(x)
        a = torch.zeros_like(q)
        for r in range(int(counts.max())):
            c = ctx[:, r * seg_ld:r * seg_ld + seg_len]
            live = (counts > r).to(x).view(-1, 1, 1)
            wr = torch.where(counts.view(-1, 1) > 1, w[:, r], torch.full_like(w[:, r], float(r == 0))).unsqueeze(2)      # count 1: the plain attention on set 0
            a = a + live * wr * ref.attention(q, F.linear(c, P[f"{b}.attn2.to_k.weight"]), F.linear(c, P[f"{b}.attn2.to_v.weight"]), heads)
        x = F.linear(a, P[f"{b}.attn2.to_out.0.weight"], P[f"{b}.attn2.to_out.0.bias"]) + x
        hid, gate = F.linear(ln(3), P[f"{b}.ff.net.0.proj.weight"], P[f"{b}.ff.net.0.proj.bias"]).chunk(2, dim=-1)
        return F.linear(hid * F.gelu(gate), P[f"{b}.ff.net.2.weight"], P[f"{b}.ff.net.2.bias"]) + x
    return block
