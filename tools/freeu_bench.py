"""Cost of FreeU: the six mx_freeu applications of an SDXL-base forward at 8 x 1024 px beside their HBM floor and beside the torch fp32 FFT form on
the same tensors, and the whole step with FreeU on and off.
Usage, on a machine with the GPU: python tools/freeu_bench.py [--out profiles/freeu.txt] [--reps 30] [--tiny]
Every comparison alternates its two sides window by window in ONE process (same clocks, same thermal state), device events around each window, after
a warm-up of both; reported: median [min .. max] per call.  A launch window is 20 back-to-back launches between one pair of events.
  floor: the skip read and written once and half the hidden state read and written once, at 8 TB/s;
  FFT:   fftn / fftshift / 2 x 2 box / ifftshift / ifftn(...).real in fp32 over the NHWC tensor's plane axes, cast to bf16, and the hidden half scaled in place;
  step:  MxUNet.forward_one, batch 8 at 128 x 128 latents, enable_freeu(0.9, 0.2, 1.3, 1.4) against disable_freeu().
The file's last section, "headline step, FreeU off ... against the parent commit", is not measured here (it needs two built trees): it is the
ms_per_step of `python bench.py --gpus 1 --steps 20 --warmup 3` run three times in each of the two checkouts, alternating, in one session on one
GPU, written in by hand.  A run with --out keeps that section of an existing file as it is."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd import ops  # noqa: E402
from sduss_amd.config import UNetConfig  # noqa: E402
from sduss_amd.unet import MxUNet  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(f, g, reps, per_window):
    for _ in range(3):
        f(); g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(event_ms(f, per_window))
        tg.append(event_ms(g, per_window))
    return tf, tg


def fmt(t, unit, name):
    return f"{statistics.median(t) * unit:9.1f} {name} [{min(t) * unit:.1f} .. {max(t) * unit:.1f}]"


def fft_form(hidden, skip, s, b):
    x = torch.fft.fftshift(torch.fft.fftn(skip.float(), dim=(1, 2)), dim=(1, 2))
    H, W = skip.shape[1], skip.shape[2]
    mask = torch.ones((1, H, W, 1), device=skip.device)
    mask[:, H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    out = torch.fft.ifftn(torch.fft.ifftshift(x * mask, dim=(1, 2)), dim=(1, 2)).real.to(skip.dtype)
    half = hidden.shape[3] // 2
    hidden[..., :half] = hidden[..., :half] * b
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--tiny", action="store_true", help="UNetConfig.tiny() and small launches: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "freeu_bench needs the GPU: a time taken elsewhere says nothing"
    from oracle import sdxl_unet_ref as ref
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev, bf = "cuda:0", torch.bfloat16
    say(f"# FreeU on {torch.cuda.get_device_name(0)}{' (tiny rehearsal)' if args.tiny else ''}")
    # (H = W, skip channels, hidden channels, s, b) of the six applications in plan order: up block 0, then up block 1 (whose first hidden state is
    # the 1280-wide output of up block 0's upsampler)
    apps = [(32, 1280, 1280), (32, 1280, 1280), (32, 640, 1280), (64, 640, 1280), (64, 640, 640), (64, 320, 640)]
    B = 8
    if args.tiny:
        apps, B = [(4, 256, 256), (8, 128, 256)], 2
    say(f"launch: mx_freeu, batch {B}; floor = (2 x skip + hidden) bytes at {HBM_BYTES_PER_S / 1e12:.0f} TB/s; FFT = the torch fp32 form on the same tensors")
    for hw, cs, chid in apps:
        skip = (torch.randn(B, hw, hw, cs, device=dev) + 0.5).to(bf)
        hidden = torch.randn(B, hw, hw, chid, device=dev).to(bf)
        slab, staged, _ = ops.freeu_route([(B, hw, hw)], cs)
        nbytes = 2 * skip.numel() * 2 + hidden.numel() * 2
        floor_us = nbytes / HBM_BYTES_PER_S * 1e6
        # b = 1 in the timed calls: the in-place product must not drift towards inf / 0 over hundreds of calls; the traffic is the same
        k, f = alternate(lambda: ops.freeu(hidden, skip, 0.9, 1.0), lambda: fft_form(hidden, skip, 0.9, 1.0), args.reps, 20)
        mk = statistics.median(k)
        say(f"  {hw}x{hw} skip {cs:4d} hidden {chid:4d} (slab {slab}, {'LDS' if staged[0] else 'read twice'}): mx_freeu {fmt(k, 1e3, 'us')}  floor {floor_us:6.1f} us "
            f"({floor_us / (mk * 1e3):.2f} of it, {nbytes / (mk * 1e-3) / 1e12:.2f} TB/s)   FFT {fmt(f, 1e3, 'us')}  ratio {statistics.median(f) / mk:.1f}x")
    cfg, ocfg = (UNetConfig.tiny(), ref.UNetConfig.tiny()) if args.tiny else (UNetConfig.sdxl_base(), ref.UNetConfig.sdxl_base())
    net = MxUNet(cfg, ref.fast_params(ocfg), device=dev)
    batch, hw = (2, 32) if args.tiny else (8, 128)
    s, t, e, te, ti = (x.to(dev) for x in ref.make_inputs(ocfg, batch, hw))
    s, e = s.to(bf), e.to(bf)

    def off():
        net.disable_freeu()
        net.forward_one(s, t, e, te, ti)

    def on():
        net.enable_freeu(0.9, 0.2, 1.3, 1.4)
        net.forward_one(s, t, e, te, ti)
    say(f"step: MxUNet.forward_one, batch {batch}, {hw}x{hw} latents")
    p, w = alternate(off, on, max(args.reps // 3, 5), 1)
    say(f"  UNet forward   FreeU off {fmt(p, 1.0, 'ms')}   on {fmt(w, 1.0, 'ms')}   ratio {statistics.median(w) / statistics.median(p):.4f}")
    net.disable_freeu()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if os.path.exists(args.out):       # the comparison against the parent commit (docstring) is not this tool's: it stays
            old = open(args.out).read().splitlines()
            at = next((i for i, ln in enumerate(old) if ln.startswith("headline step")), len(old))
            lines += old[at:]
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
