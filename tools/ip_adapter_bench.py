"""Cost of the image-prompt (IP-Adapter) term: mx_attention_cross_ip beside the plain mx_attention_cross_prescaled launch, and the whole SDXL-base
step with the adapter on every row beside the plain step.
Usage, on a machine with the GPU: python tools/ip_adapter_bench.py [--out profiles/ip_adapter.txt] [--reps 30] [--tiny]
Both legs alternate the two sides call by call in ONE process (same clocks, same thermal state), device events around each call, after a
warm-up of both; reported: median, min, max of each side and the ratio of the medians.  A launch window is 50 back-to-back launches between one pair of events.
  launch: the step's two cross-attention shapes (B8 H10 Lq4096, B8 H20 Lq1024; Lk 77) at n_img 4 and 16, every ip_scale 1;
  step:   MxUNet.forward_one, batch 8 at 128x128 latents, with image tokens announced for every row (scale 1) and without."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd import ops  # noqa: E402
from sduss_amd.config import UNetConfig  # noqa: E402
from sduss_amd.ip_adapter import IPAdapter, cross_attention_layers  # noqa: E402
from sduss_amd.unet import MxUNet  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(plain, with_ip, reps, per_window=1):
    """alternating timed windows of ``per_window`` back-to-back calls each (a single 30 us launch between two events is mostly launch overhead);
    times per call"""
    def window(fn):
        def run():
            for _ in range(per_window):
                fn()
        return event_ms(run) / per_window
    for _ in range(3):
        plain(); with_ip()
    torch.cuda.synchronize()
    p, w = [], []
    for _ in range(reps):
        p.append(window(plain))
        w.append(window(with_ip))
    return p, w


def report(say, what, p, w, unit=1e3, name="us"):
    mp, mw = statistics.median(p), statistics.median(w)
    say(f"  {what:34s} plain {mp * unit:9.1f} {name} [{min(p) * unit:.1f} .. {max(p) * unit:.1f}]   with image term {mw * unit:9.1f} {name} "
        f"[{min(w) * unit:.1f} .. {max(w) * unit:.1f}]   ratio {mw / mp:.3f}  ({len(p)} alternating windows each)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--tiny", action="store_true", help="UNetConfig.tiny() and small launches: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ip_adapter_bench needs the GPU: a time taken elsewhere says nothing"
    from oracle import sdxl_unet_ref as ref
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev, bf = "cuda:0", torch.bfloat16
    say(f"# image-prompt adapter on {torch.cuda.get_device_name(0)}{' (tiny rehearsal)' if args.tiny else ''}")
    say("launch: mx_attention_cross_ip against mx_attention_cross_prescaled, Lk 77")
    for B, H, Lq in ((2, 2, 256),) if args.tiny else ((8, 10, 4096), (8, 20, 1024)):
        D = H * 64
        q = (torch.randn(B * Lq, D, device=dev) * ops.ATTN_QSCALE).to(bf)
        k, vt = torch.randn(B * 77, D, device=dev).to(bf), ops.pack_vt(torch.randn(B, 77, D, device=dev).to(bf))
        k_ip, vt_ip = torch.randn(B * 16, D, device=dev).to(bf), ops.pack_vt(torch.randn(B, 16, D, device=dev).to(bf))
        one = torch.ones(B, device=dev)
        for n_img in (4, 16):
            p, w = alternate(lambda: ops.attention_cross(q, k, vt, H, Lq, 77),
                             lambda: ops.attention_cross_ip(q, k, vt, k_ip, vt_ip, n_img, one, H, Lq, 77), args.reps, per_window=50)
            report(say, f"B{B} H{H} Lq{Lq} n_img {n_img}", p, w)
    cfg, ocfg = (UNetConfig.tiny(), ref.UNetConfig.tiny()) if args.tiny else (UNetConfig.sdxl_base(), ref.UNetConfig.sdxl_base())
    net = MxUNet(cfg, ref.fast_params(ocfg), device=dev)
    g = torch.Generator().manual_seed(1)
    ctx = cfg.cross_attention_dim
    sd = {f"{b}.attn2.processor.{nm}.0.weight": torch.randn(dim, ctx, generator=g) * ctx ** -0.5 for b, dim in cross_attention_layers(cfg) for nm in ("to_k_ip", "to_v_ip")}
    ad = IPAdapter.from_state_dict(cfg, sd, n_img=4)
    net.set_ip_adapter(ad)
    batch, hw = (2, 32) if args.tiny else (8, 128)
    s, t, e, te, ti = (x.to(dev) for x in ref.make_inputs(ocfg, batch, hw))
    s, e = s.to(bf), e.to(bf)
    tokens, one = ad.project(torch.randn(batch, 4, ctx, device=dev)), torch.ones(batch, device=dev)

    def with_ip():
        net.set_image_tokens(tokens, one)
        net.forward_one(s, t, e, te, ti)
    say(f"step: MxUNet.forward_one, batch {batch}, {hw}x{hw} latents, n_img 4, the adapter on every row")
    p, w = alternate(lambda: net.forward_one(s, t, e, te, ti), with_ip, max(args.reps // 3, 5))
    report(say, "UNet forward", p, w, unit=1.0, name="ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
