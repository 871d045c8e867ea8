"""Cost of regional prompts: mx_attention_cross_regions at the shapes an SDXL-base step of four 1024 px requests under CFG gets (8 samples), beside the
plain short-key launch on the same rows and the naive route (one plain launch per prompt plus a torch blend), and the whole denoising step with 0, 1 and
4 regional requests.
Usage, on a machine with the GPU: python tools/regions_bench.py [--out profiles/regions.txt] [--reps 30] [--tiny]
Every comparison alternates its sides window by window in ONE process (same clocks, same thermal state), device events around each window, after a
warm-up of all of them; reported: median [p10 .. p90] per call.  A launch window is 20 back-to-back launches between one pair of events.
  launch: 8 samples x 20 heads x 1024 tokens (32 x 32 grid) and 8 x 10 x 4096 (64 x 64), 77-token prompts, every sample regional:
          halves (left / right, n_sets 2) and bands (a base prompt everywhere + three vertical bands, n_sets 4);
  step:   SDXLDenoiser.denoising_step, four 1024 px requests under CFG, of which 0, 1 or 4 carry the bands' regions.
The weights are random, so nothing here says what the regions do to an image: only times are reported.
The file's last section ("headline step ...") is not measured here: it is the ms_per_step of `python bench.py --gpus 1 --steps 20 --warmup 3` in this
tree and in a checkout of the parent commit, alternating in one session.  A run with --out keeps it as it is."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd import ops  # noqa: E402
from sduss_amd.config import UNetConfig  # noqa: E402
from sduss_amd.regions import mask_weights  # noqa: E402
from sduss_amd.unet import MxUNet  # noqa: E402


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns, reps, per_window):
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(times, fns):
            t.append(event_ms(f, per_window))
    return times


def fmt(t, unit, name):
    q = statistics.quantiles(t, n=10)
    return f"{statistics.median(t) * unit:8.1f} {name} [{q[0] * unit:.1f} .. {q[-1] * unit:.1f}]"


def masks_of(kind, hw):
    """halves: left / right; bands: a base prompt everywhere and three vertical bands (a token of a band is shared half and half with the base)"""
    if kind == "halves":
        m = torch.zeros(2, hw, hw)
        m[0, :, :hw // 2], m[1, :, hw // 2:] = 1.0, 1.0
        return m
    m = torch.zeros(4, hw, hw)
    m[0] = 1.0
    for r in range(3):
        m[r + 1, :, r * hw // 3:(r + 1) * hw // 3] = 1.0
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--tiny", action="store_true", help="UNetConfig.tiny() and small launches: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "regions_bench needs the GPU: a time taken elsewhere says nothing"
    from oracle import sdxl_unet_ref as ref
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev, bf, seg = "cuda:0", torch.bfloat16, 77
    seg_ld = ops.vt_ld(seg)
    say(f"# regional prompts on {torch.cuda.get_device_name(0)}{' (tiny rehearsal)' if args.tiny else ''}")
    B, levels = (2, [(16, 2)]) if args.tiny else (8, [(32, 20), (64, 10)])
    say(f"launch: {B} samples, {seg}-token prompts; median [p10 .. p90] over {args.reps} windows of 20 launches, the launches of a row alternating")
    for hw, H in levels:
        L, D = hw * hw, H * 64
        q = (torch.randn(B * L, D, device=dev) * 0.18).to(bf)
        o = torch.empty_like(q)
        for kind in ("halves", "bands"):
            w1 = mask_weights(masks_of(kind, hw), (hw, hw))
            n = w1.shape[0]
            k = torch.randn(B * n * seg_ld, D, device=dev).to(bf)
            v = torch.randn(B, n * seg_ld, D, device=dev).to(bf)
            vt = ops.pack_vt(v)
            w = w1.to(dev).unsqueeze(0).repeat(B, 1, 1).contiguous()
            counts = torch.full((B,), n, dtype=torch.int32, device=dev)
            ks = [k.view(B, n, seg_ld, D)[:, r, :seg].reshape(B * seg, D).contiguous() for r in range(n)]
            vts = [ops.pack_vt(v.view(B, n, seg_ld, D)[:, r, :seg].contiguous()) for r in range(n)]

            def naive():
                acc = None
                for r in range(n):
                    t = ops.attention_cross(q, ks[r], vts[r], H, L, seg).view(B, L, D).float() * w[:, r].unsqueeze(2)
                    acc = t if acc is None else acc + t
                return acc.to(bf)
            fns = [lambda: ops.attention_cross_regions(q, k, vt, w, counts, H, L, n, seg, out=o), lambda: ops.attention_cross(q, ks[0], vts[0], H, L, seg), naive]
            times = alternate(fns, args.reps, 20)
            names = ("regions, one launch", "plain launch, one prompt", f"naive: {n} plain launches + torch blend")
            say(f"  {hw}x{hw} H {H} {kind} (n_sets {n}): " + "   ".join(f"{nm} {fmt(t, 1e3, 'us')}" for nm, t in zip(names, times)))
    cfg, ocfg = (UNetConfig.tiny(), ref.UNetConfig.tiny()) if args.tiny else (UNetConfig.sdxl_base(), ref.UNetConfig.sdxl_base())
    net = MxUNet(cfg, ref.fast_params(ocfg), device=dev)
    den, res, n_req = SDXLDenoiser(net), (256 if args.tiny else 1024), 4
    embeds = torch.randn(4, seg, cfg.cross_attention_dim, device=dev).to(bf)
    masks = masks_of("bands", res // 8)

    def batch(regional):
        reqs = [synthetic_request(i, res, 1000, cfg, den, dev) for i in range(n_req)]
        for r in reqs[:regional]:
            den.set_regions(r, embeds, masks)
        return lambda: den.denoising_step({str(res): reqs})
    modes = [0, 1, 4]
    reps = max(args.reps // 3, 5)
    say(f"step: SDXLDenoiser.denoising_step, {n_req} requests at {res} px under CFG; median [p10 .. p90] over {reps} alternating steps")
    times = alternate([batch(m) for m in modes], reps, 1)
    base = statistics.median(times[0])
    for m, tt in zip(modes, times):
        say(f"  {m} regional requests (bands, 4 prompts): {fmt(tt, 1.0, 'ms')}   {statistics.median(tt) - base:+.2f} ms, ratio {statistics.median(tt) / base:.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if os.path.exists(args.out):       # the section that is not this tool's (docstring) stays
            old = open(args.out).read().splitlines()
            at = next((i for i, ln in enumerate(old) if ln.startswith("headline step")), len(old))
            lines += old[at:]
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
