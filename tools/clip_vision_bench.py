"""Cost and parity of the CLIP vision encoder (OpenCLIP ViT-H/14, random weights): the whole encode and its two own kernels beside stock torch -- the
same graph in bf16 with scaled_dot_product_attention (tests/clip_vision_ref.py) -- on the same GPU in the same process.
Usage, on a machine with the GPU: python tools/clip_vision_bench.py [--out profiles/clip_vision.txt] [--reps 30] [--tiny]
Both sides alternate window by window (same clocks, same thermal state), device events around each window, after a warm-up of both; reported: median
and p10 .. p90 of each side and the ratio of the medians.  A kernel window is 20 back-to-back launches between one pair of events.
  parity:  the tiny test configurations, max and RMS error against the fp64 restatement, ours and stock bf16;
  kernels: mx_attention_d80 against SDPA (B x 16 heads x 257 x 80) and mx_patch_embed_u8 against normalise + conv2d + cat + add (B x 224 x 224);
  encode:  MxCLIPVision.encode against vit_forward in bf16, B = 1 and 8."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_vision_ref as cref  # noqa: E402
from sduss_amd import ops  # noqa: E402
from sduss_amd.clip_vision import CLIPVisionConfig, MxCLIPVision, synthetic_clip_vision_params  # noqa: E402
from sduss_amd.weights import pack_clip_vision  # noqa: E402


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(ours, stock, reps, per_window=1):
    for _ in range(3):
        ours(); stock()
    torch.cuda.synchronize()
    o, s = [], []
    for _ in range(reps):
        o.append(event_ms(ours, per_window))
        s.append(event_ms(stock, per_window))
    return o, s


def report(say, what, o, s, unit=1e3, name="us"):
    def side(x):
        q = statistics.quantiles(x, n=10)
        return f"{statistics.median(x) * unit:9.1f} {name} [p10 {q[0] * unit:.1f} .. p90 {q[-1] * unit:.1f}]"
    say(f"  {what:28s} ours {side(o)}   stock torch {side(s)}   ours / stock {statistics.median(o) / statistics.median(s):.3f}  ({len(o)} alternating windows each)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--tiny", action="store_true", help="the tiny configuration throughout: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clip_vision_bench needs the GPU: a time taken elsewhere says nothing"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev, bf = "cuda:0", torch.bfloat16
    g = torch.Generator().manual_seed(1)
    say(f"# CLIP vision encoder on {torch.cuda.get_device_name(0)}{' (tiny rehearsal)' if args.tiny else ''}")
    say("parity: error against the fp64 restatement, 2 images of 56x56, hidden 4 heads x width, 2 layers")
    for width, act in ((80, "quick_gelu"), (80, "gelu"), (64, "quick_gelu"), (64, "gelu")):
        cfg = CLIPVisionConfig.tiny(width, act)
        P = synthetic_clip_vision_params(cfg)
        images = torch.randint(0, 256, (2, 56, 56, 3), generator=g, dtype=torch.uint8).to(dev)
        ours, ref, stock = MxCLIPVision(cfg, P).encode(images, hidden_states=True), cref.vit_forward(cfg, P, images, torch.float64), cref.vit_forward(cfg, P, images, bf)
        for name, o, r, s in zip(("image_embeds", "hidden_states[-2]"), ours, ref, stock):
            eo, es = (o.double() - r).abs(), (s.double() - r).abs()
            say(f"  heads of {width} {act:10s} {name:17s} max ours {eo.max():.3e} stock {es.max():.3e} ratio {eo.max() / es.max():.2f}   "
                f"rms ours {eo.square().mean().sqrt():.3e} stock {es.square().mean().sqrt():.3e} ratio {eo.square().mean().sqrt() / es.square().mean().sqrt():.2f}")
    cfg = CLIPVisionConfig.tiny() if args.tiny else CLIPVisionConfig.vit_h_14()
    P = synthetic_clip_vision_params(cfg)
    enc = MxCLIPVision(cfg, P)
    Pd = {k: v.to(dev, bf) for k, v in P.items()}
    H, heads, S, L = cfg.hidden_size, cfg.num_attention_heads, cfg.image_size, cfg.tokens
    packed = {n: t.to(dev) for n, t in pack_clip_vision(cfg, P) if "embeddings" in n}
    pw, cls, pos = (packed["vision_model.embeddings." + n] for n in ("patch_embedding.weight", "class_embedding", "position_embedding.weight"))
    conv_w = Pd["vision_model.embeddings.patch_embedding.weight"]
    for B in (1, 8):
        say(f"B = {B}: ViT-H/14, {L} tokens, {heads} heads of {H // heads}" if not args.tiny else f"B = {B}: tiny")
        images = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
        qkv = torch.randn(B * L, 3 * H, device=dev).to(bf)
        q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
        q4, k4, v4 = (t.reshape(B, L, heads, -1).transpose(1, 2) for t in (q, k, v))
        out = torch.empty(B * L, H, dtype=bf, device=dev)
        o, s = alternate(lambda: ops.attention_d80(q, k, v, heads, B, out=out), lambda: torch.nn.functional.scaled_dot_product_attention(q4, k4, v4), args.reps, 20)
        report(say, "mx_attention_d80", o, s)
        if B == 1:
            say(f"    (one launch is {heads} heads x {-(-L // 64)} query blocks = {heads * -(-L // 64)} workgroups: far from filling the chip, and not tuned for)")
        x = torch.empty(B, L, H, dtype=bf, device=dev)

        def stock_embed():
            xn = cref.normalise(images, cfg.image_mean, cfg.image_std).permute(0, 3, 1, 2)
            y = torch.nn.functional.conv2d(xn, conv_w, stride=cfg.patch_size).flatten(2).transpose(1, 2)
            return torch.cat([Pd["vision_model.embeddings.class_embedding"].expand(B, 1, H), y], dim=1) + Pd["vision_model.embeddings.position_embedding.weight"]
        o, s = alternate(lambda: ops.patch_embed_u8(images, pw, cls, pos, cfg.patch_size, cfg.image_mean, cfg.image_std, out=x), stock_embed, args.reps, 20)
        report(say, "mx_patch_embed_u8", o, s)
        with torch.inference_mode():
            o, s = alternate(lambda: enc.encode(images), lambda: cref.vit_forward(cfg, Pd, images, bf), max(args.reps // 2, 5))
        report(say, "whole encode", o, s, unit=1.0, name="ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
