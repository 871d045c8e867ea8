"""LoRA adapters on the host: the packing algebra, the key parsing, the term table's checks (no GPU).

Packing algebra.  ``pack(cfg, P + s f B A)`` (the only route before the merge kernel; f = alpha / r) against the device formula of tests/lora_ref.py
applied to ``pack(cfg, P)`` with the adapter's placed factors.  Both routes end in ONE bf16 rounding of (almost) the same real number
x = (W + s f B A) g  (g = the folded LayerNorm's gamma, 1 elsewhere), so with D = |s f| (|B| @ |A g|) the roundings that separate them are

    base      the device route starts from bf16(W g):                                        2^-8 |W g|
    factors   it multiplies bf16(B) by bf16(A g): (1 + 2^-8)^2 - 1 = 2^-7 + 2^-16 relative:     (2^-7 + 2^-16) D
    fp32      P + s f B A is formed in fp32 by the pack route (r products, a scale, an add, the multiplication by g): (r + 4) 2^-24 (|W g| + D)
    final     each route rounds its own value once: 2^-8 |x| for the pack route, 2^-8 (|x| + E) for the device route, E = the three lines above

    bound = E + 2^-8 (2 |x| + E)        per element; EVERY element of every targeted matrix is compared.

The deltas are as large as W itself (|B A| ~ 2 |W|), so a wrong row permutation, layer offset, q / k / v range or a missing gamma (|g - 1| ~ 0.1)
is off by many bounds on most elements.  colsum is the fp32 row sum of the rounded matrix on both routes: they differ by at most the sum of the
row's bounds plus K 2^-24 sum |out|.  bias' = bias + (W + s f B A) beta on the pack route, (bias + W beta) + s f B (A beta) on the device route, all
fp32: (K + r + 4) 2^-23 (|bias| + (|W| + |s f| |B| |A|) |beta|).  Tensors no adapter targets must be bit-equal."""
import os
import subprocess

import pytest
import torch

from sduss_amd import lib as _lib
from sduss_amd import lora, ops, weights
from sduss_amd.config import UNetConfig, param_shapes

import lora_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, U24 = 2.0 ** -8, 2.0 ** -24          # unit roundoffs of bf16 (8 significant bits) and fp32


_adapter_sd = lora_ref.random_adapter_sd


@pytest.fixture(scope="module")
def tiny_packed():
    cfg = UNetConfig.tiny()
    P = weights.synthetic_params(cfg)
    entries = weights.pack(cfg, P)
    layout = lora.LoraLayout(cfg, lora.blob_table(entries), lora.norm_params(P), "cpu")
    return cfg, P, dict(entries), layout


def test_targets_cover_every_linear_and_fit_the_tiling():
    for cfg in (UNetConfig.tiny(), UNetConfig.sdxl_base()):
        targets = lora.lora_targets(cfg)
        shapes = {k[:-len(".weight")]: v for k, v in param_shapes(cfg).items()
                  if k.endswith(".weight") and len(v) == 2 and (".transformer_blocks." in k or ".proj_in." in k or ".proj_out." in k)}
        assert set(targets) == set(shapes)
        for m, t in targets.items():
            assert (t.rows, t.K) == shapes[m], m
            assert t.rows % 16 == 0 and t.row0 % 16 == 0 and t.K % 64 == 0 and t.row0 + t.rows <= t.N, (m, t)


def test_packing_algebra_every_target_kind(tiny_packed):
    cfg, P, packed, layout = tiny_packed
    s = -0.9
    adapter = lora.LoraAdapter.from_state_dict(cfg, _adapter_sd(cfg, 1))
    assert len(adapter.modules) == len(lora.lora_targets(cfg)) and not adapter.skipped
    want = dict(weights.pack(cfg, lora.merged_params(P, [(adapter, s)])))
    terms = lora.scaled_terms(layout, [(adapter, s)])
    ops.lora_merge_validate([{**t, "up": 0x1000, "down_t": 0x2000, "dbias": 0x3000 if "dbias" in t else None, "R": t["up"].shape[1]} for t in terms],
                            sum(v.numel() * v.element_size() + 256 for v in packed.values()))
    got = lora_ref.apply_terms(packed, terms)
    assert set(got) == {n for n in packed if not torch.equal(packed[n], want[n])}, "the formula touched other tensors than the pack route"
    for n in packed:
        if n not in got:
            assert torch.equal(packed[n], want[n]), f"{n}: untargeted, yet the pack route changed it"
    f64 = torch.float64
    for m, tg in lora.lora_targets(cfg).items():
        a, b, factor = adapter.modules[m]
        sf = lora_ref.f32_scale(s * factor)
        w = P[f"{m}.weight"].to(f64).reshape(tg.rows, tg.K)
        bias = P.get(f"{m}.bias")
        a, b = a.to(f64), b.to(f64)
        if tg.geglu:
            w, b = weights._geglu_interleave(w), weights._geglu_interleave(b)
            bias = weights._geglu_interleave(bias)
        gam = P[f"{tg.norm}.weight"].to(f64) if tg.norm else torch.ones(tg.K, dtype=f64)
        x = (w + sf * (b @ a)) * gam[None, :]
        wg, D = (w * gam[None, :]).abs(), abs(sf) * (b.abs() @ (a * gam[None, :]).abs())
        r = a.shape[0]
        E = U8 * wg + (2.0 ** -7 + 2.0 ** -16) * D + (r + 4) * U24 * (wg + D)
        bound = E + U8 * (2 * x.abs() + E)
        rows = slice(tg.row0, tg.row0 + tg.rows)
        g_, w_ = got[f"{tg.packed}.weight"][rows].to(f64), want[f"{tg.packed}.weight"][rows].to(f64)
        bad = (g_ - w_).abs() > bound
        assert not bool(bad.any()), f"{m}: {int(bad.sum())} of {bad.numel()} elements off, worst {float(((g_ - w_).abs() / bound).max()):.1f} bounds"
        assert not bool(((w_ - x).abs() > U8 * x.abs() + (r + 4) * U24 * (wg + D)).any()), f"{m}: the pack route is not where the fp64 value is"
        if tg.norm:
            cs_g, cs_w = got[f"{tg.packed}.colsum"][rows].to(f64), want[f"{tg.packed}.colsum"][rows].to(f64)
            cs_bound = bound.sum(dim=1) + tg.K * U24 * (g_.abs().sum(dim=1) + w_.abs().sum(dim=1))
            assert bool(((cs_g - cs_w).abs() <= cs_bound).all()), f"{m}: colsum"
            beta = P[f"{tg.norm}.bias"].to(f64)
            b_bound = (tg.K + r + 4) * 2.0 ** -23 * ((bias.to(f64).abs() if bias is not None else 0) + (w.abs() + abs(sf) * (b.abs() @ a.abs())) @ beta.abs())
            b_g, b_w = got[f"{tg.packed}.bias"][rows].to(f64), want[f"{tg.packed}.bias"][rows].to(f64)
            assert bool(((b_g - b_w).abs() <= b_bound).all()), f"{m}: folded bias off by {float((b_g - b_w).abs().max()):.3g}"
            assert float((b_g - packed[f"{tg.packed}.bias"][rows].to(f64)).abs().max()) > 100 * float(b_bound.max()), f"{m}: the bias did not move"


def test_stacked_adapters_add_in_set_order(tiny_packed):
    cfg, P, packed, layout = tiny_packed
    m = "mid_block.attentions.0.transformer_blocks.1.attn1.to_k"
    x = lora.LoraAdapter.from_state_dict(cfg, _adapter_sd(cfg, 2, modules={m}))
    y = lora.LoraAdapter.from_state_dict(cfg, _adapter_sd(cfg, 3, ranks=(24,), modules={m}))
    terms = lora.scaled_terms(layout, [(x, 0.8), (y, -1.3)])
    assert [t["up"].shape[1] for t in terms] == [32, 32] and [t["row0"] for t in terms] == [256, 256]
    got = lora_ref.apply_terms(packed, terms)
    want = dict(weights.pack(cfg, lora.merged_params(P, [(x, 0.8), (y, -1.3)])))
    name = "mid_block.attentions.0.transformer_blocks.1.attn1.to_qkv.weight"
    diff = (got[name].double() - want[name].double()).abs()
    assert float(diff.max()) <= 2.0 ** -6 * float(want[name].double().abs().max())
    assert torch.equal(got[name][:256], packed[name][:256]) and torch.equal(got[name][512:], packed[name][512:])


def test_key_parsing(tiny_packed):
    cfg, _P, _packed, layout = tiny_packed
    m = "down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_v"
    t = lora.lora_targets(cfg)[m]
    a, b = torch.randn(4, t.K), torch.randn(t.rows, 4)
    plain = lora.LoraAdapter.from_state_dict(cfg, {f"{m}.lora_A.weight": a, f"{m}.lora_B.weight": b})
    assert plain.modules[m][2] == 1.0, "without alpha the factor is 1"
    with_alpha = lora.LoraAdapter.from_state_dict(cfg, {f"unet.{m}.lora_A.weight": a, f"unet.{m}.lora_B.weight": b, f"unet.{m}.alpha": torch.tensor(2.0)})
    assert with_alpha.modules[m][2] == 0.5, "alpha / r"
    old = lora.LoraAdapter.from_state_dict(cfg, {f"{m}.lora.down.weight": a, f"{m}.lora.up.weight": b})
    assert torch.equal(old.modules[m][0], plain.modules[m][0]) and torch.equal(old.modules[m][1], plain.modules[m][1])
    # ranks 4 and 24 are zero-padded to 32; the layer's offset inside attn2_kv_all
    for r in (4, 24):
        ad = lora.LoraAdapter.from_state_dict(cfg, {f"{m}.lora_A.weight": torch.randn(r, t.K), f"{m}.lora_B.weight": torch.randn(t.rows, r)})
        (term,) = ad.placed(layout)
        assert term["up"].shape == (t.rows, 32) and term["down_t"].shape == (t.K, 32)
        assert not term["up"][:, r:].any() and not term["down_t"][:, r:].any() and term["up"][:, :r].any()
        assert term["packed"] == "attn2_kv_all.128" and term["row0"] == 128 and term["N"] == 5 * 2 * 128 and "dbias" not in term
        assert ad.placed(layout) is ad.placed(layout), "placed once per layout"
    # keys without a place
    conv = {"down_blocks.0.resnets.0.conv1.lora_A.weight": torch.randn(4, 64, 3, 3), "down_blocks.0.resnets.0.conv1.lora_B.weight": torch.randn(64, 4, 1, 1),
            "down_blocks.0.resnets.0.time_emb_proj.lora_A.weight": torch.randn(4, 256), "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight": torch.randn(4, 8)}
    sd = {f"{m}.lora_A.weight": a, f"{m}.lora_B.weight": b, **conv}
    with pytest.raises(ValueError, match="conv1.lora_A.weight") as e:
        lora.LoraAdapter.from_state_dict(cfg, sd)
    assert all(k in str(e.value) for k in conv)
    lenient = lora.LoraAdapter.from_state_dict(cfg, sd, strict=False)
    assert lenient.skipped == sorted(conv) and list(lenient.modules) == [m]
    with pytest.raises(ValueError, match="do not fit"):
        lora.LoraAdapter.from_state_dict(cfg, {f"{m}.lora_A.weight": torch.randn(4, t.K + 1), f"{m}.lora_B.weight": b})
    with pytest.raises(ValueError, match="both factors"):
        lora.LoraAdapter.from_state_dict(cfg, {f"{m}.lora_A.weight": a})


def _term(**kw):
    t = dict(w_off=4096, N=128, K=128, row0=0, rows=128, up=0x10000, down_t=0x20000, R=32, scale=0.5)
    t.update(kw)
    return t


def test_validate_accepts_a_good_table():
    blob = 1 << 20
    ops.lora_merge_validate([], blob)
    ops.lora_merge_validate([_term(), _term(up=0x30000, R=64), _term(w_off=65536, N=384, row0=128, rows=128),
                             _term(w_off=65536, N=384, row0=256, rows=128, colsum_off=300000, bias_off=304096, dbias=0x40000)], blob)
    assert _lib.load().mx_lora_table_bytes(4) >= 4 * 32


@pytest.mark.parametrize("terms,message", [
    ([_term(w_off=(1 << 20) - 4096)], "outside the blob"),
    ([_term(colsum_off=(1 << 20) - 256, bias_off=0)], "derived vector lies outside the blob"),
    ([_term(row0=64)], "does not lie inside the matrix"),
    ([_term(rows=24)], "multiples of 16"),
    ([_term(row0=8, rows=16)], "multiples of 16"),
    ([_term(K=96)], "multiple of 64"),
    ([_term(R=16)], "multiple of 32"),
    ([_term(R=48)], "multiple of 32"),
    ([_term(w_off=4100)], "misaligned matrix offset"),
    ([_term(up=0x10008)], "misaligned factor"),
    ([_term(colsum_off=300002, bias_off=304096)], "misaligned vector offset"),
    ([_term(), _term(row0=64, rows=64)], "overlaps that of term 0 without being identical"),
    ([_term(rows=96), _term(row0=64, rows=64)], "overlaps"),
    ([_term(R=512), _term(R=32)], "MX_LORA_MAX_RANK"),
    ([_term(scale=float("inf"))], "not finite"),
])
def test_validate_refuses(terms, message):
    with pytest.raises(_lib.MxError, match=message):
        ops.lora_merge_validate(terms, 1 << 20)


def test_term_table_under_address_and_ub_sanitizers():
    """tests/lora_terms_walk.cpp: a program of its own over csrc/lora_terms.cpp, compiled with -fsanitize=address,undefined and run on the CPU as
    a child process: good tables and the device table they become, and every refused kind of table."""
    csrc = os.path.join(ROOT, "sduss_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "lora_walk"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "LORA_TERMS_WALK_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
