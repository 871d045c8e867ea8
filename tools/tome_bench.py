"""Cost and gain of token merging: the four launches of tome.hip at the two attention levels of an SDXL-base forward at 8 x 1024 px, and the whole
step with token merging off and on.
Usage, on a machine with the GPU: python tools/tome_bench.py [--out profiles/tome.txt] [--reps 30] [--tiny]
Every comparison alternates its sides window by window in ONE process (same clocks, same thermal state), device events around each window, after a
warm-up of all of them; reported: median [p10 .. p90] per call.  A launch window is 20 back-to-back launches between one pair of events.
  match:  2 B Nsrc Ndst C floating-point operations over its time (the norms and the running maximum are not counted);
  step:   MxUNet.forward_one, batch 8 at 128 x 128 latents, disable_tome() against enable_tome(ratio, max_downsample=2 | 4).
The weights are random, so nothing here says what token merging does to an image: only times are reported.
The file's last sections ("accuracy ...", "headline step ...") are not measured here: the first is the printed line of
tests/test_tome_gpu.py::test_forward_identity_and_reference, the second the ms_per_step of `python bench.py --gpus 1 --steps 20 --warmup 3` run in
this tree and in a checkout of the parent commit, alternating, in one session on one GPU.  A run with --out keeps them as they are."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--tiny", action="store_true", help="UNetConfig.tiny() and small launches: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tome_bench needs the GPU: a time taken elsewhere says nothing"
    from oracle import sdxl_unet_ref as ref
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev, bf = "cuda:0", torch.bfloat16
    say(f"# Token merging on {torch.cuda.get_device_name(0)}{' (tiny rehearsal)' if args.tiny else ''}")
    B, levels = (2, [(16, 128)]) if args.tiny else (8, [(64, 640), (32, 1280)])
    say(f"launch: batch {B}, cells 2 x 2; median [p10 .. p90] over {args.reps} windows of 20 launches, the four kernels alternating")
    for hw, Cc in levels:
        x = torch.randn(B, hw * hw, Cc, device=dev).to(bf)
        for ratio in (0.5, 0.75):
            ndst, nsrc, r, lm = ops.tome_sizes(hw, hw, 2, 2, ratio)
            node_max, node_idx = ops.tome_match(x, hw, hw)
            tables = ops.tome_select(node_max, node_idx, hw, hw, r)
            o = ops.tome_merge(x, tables, 1e-5)
            tm, ts, tg, tu = alternate([lambda: ops.tome_match(x, hw, hw), lambda: ops.tome_select(node_max, node_idx, hw, hw, r),
                                        lambda: ops.tome_merge(x, tables, 1e-5), lambda: ops.tome_unmerge(o, tables, x)], args.reps, 20)
            tflops = 2.0 * B * nsrc * ndst * Cc / (statistics.median(tm) * 1e-3) / 1e12
            say(f"  {hw}x{hw}x{Cc} ratio {ratio} (r {r}, Lm {lm}): match {fmt(tm, 1e3, 'us')} {tflops:6.1f} TFLOP/s   select {fmt(ts, 1e3, 'us')}   "
                f"merge {fmt(tg, 1e3, 'us')}   unmerge+add {fmt(tu, 1e3, 'us')}")
    cfg, ocfg = (UNetConfig.tiny(), ref.UNetConfig.tiny()) if args.tiny else (UNetConfig.sdxl_base(), ref.UNetConfig.sdxl_base())
    net = MxUNet(cfg, ref.fast_params(ocfg), device=dev)
    batch, hw = (2, 64) if args.tiny else (8, 128)
    s, t, e, te, ti = (v.to(dev) for v in ref.make_inputs(ocfg, batch, hw))
    s, e = s.to(bf), e.to(bf)
    modes = [None, (0.5, 2), (0.5, 4), (0.75, 2), (0.75, 4)]

    def step(mode):
        def run():
            if mode is None:
                net.disable_tome()
            else:
                net.enable_tome(ratio=mode[0], max_downsample=mode[1])
            net.forward_one(s, t, e, te, ti)
        return run
    say(f"step: MxUNet.forward_one, batch {batch}, {hw}x{hw} latents; median [p10 .. p90] over {max(args.reps // 3, 5)} alternating forwards")
    times = alternate([step(m) for m in modes], max(args.reps // 3, 5), 1)
    base = statistics.median(times[0])
    for m, tt in zip(modes, times):
        name = "ToMe off" if m is None else f"ratio {m[0]} max_downsample {m[1]}"
        say(f"  {name:32s} {fmt(tt, 1.0, 'ms')}   {statistics.median(tt) - base:+.2f} ms, ratio {statistics.median(tt) / base:.4f}")
    net.disable_tome()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if os.path.exists(args.out):       # the sections that are not this tool's (docstring) stay
            old = open(args.out).read().splitlines()
            at = next((i for i, ln in enumerate(old) if ln.startswith("accuracy")), len(old))
            lines += old[at:]
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
