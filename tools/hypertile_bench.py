"""Cost and gain of HyperTile: mx_attention_window at the shapes an SDXL-base forward at 8 x 1024 px gets beside the plain self-attention launches it
replaces, and the whole step with HyperTile off and on.
Usage, on a machine with the GPU: python tools/hypertile_bench.py [--out profiles/hypertile.txt] [--reps 30] [--tiny] [--streamed-lib PATH]
Every comparison alternates its sides window by window in ONE process (same clocks, same thermal state), device events around each window, after a
warm-up of all of them; reported: median [p10 .. p90] per call.  A launch window is 20 back-to-back launches between one pair of events.
  launch: batch 8; level 64 x 64 (H 10) and 32 x 32 (H 20): the plain launch (mx_attention_prescaled, L keys) against 16 x 16 windows (tile 128, both
          levels) and 32 x 32 windows (tile 256, the first level; at the second the window is the whole grid and the level runs plain);
  step:   MxUNet.forward_one, batch 8 at 128 x 128 latents, disable_hypertile() against enable_hypertile(128) and (256).
--streamed-lib: a second build of the library with -DMX_WIN_RESIDENT_MAX=0 on attention_window.hip, whose streamed form serves every window: the
16 x 16 windows are then timed on both forms, alternating.
The weights are random, so nothing here says what HyperTile does to an image: only times are reported.
The file's last sections ("accuracy ...", "headline step ...") are not measured here: the first is the printed lines of
tests/test_hypertile_gpu.py::test_forward_identity_and_reference, the second the ms_per_step of `python bench.py --gpus 1 --steps 20 --warmup 3` in this
tree and in a checkout of the parent commit.  A run with --out keeps them as they are."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd import lib as _lib, ops  # noqa: E402
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
    ap.add_argument("--streamed-lib", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hypertile_bench needs the GPU: a time taken elsewhere says nothing"
    from oracle import sdxl_unet_ref as ref
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev, bf = "cuda:0", torch.bfloat16
    say(f"# HyperTile on {torch.cuda.get_device_name(0)}{' (tiny rehearsal)' if args.tiny else ''}")
    B, levels = (2, [(32, 2, (16,))]) if args.tiny else (8, [(64, 10, (16, 32)), (32, 20, (16,))])
    other = None
    if args.streamed_lib:
        other = C.CDLL(os.path.abspath(args.streamed_lib))
        other.mx_attention_window.restype, other.mx_attention_window.argtypes = _lib.SYMBOLS["mx_attention_window"]
    say(f"launch: batch {B}; median [p10 .. p90] over {args.reps} windows of 20 launches, the launches of a level alternating")
    for hw, H, wins in levels:
        L, D = hw * hw, H * 64
        q, k = (torch.randn(B * L, D, device=dev).to(bf) for _ in range(2))
        vt = ops.pack_vt(torch.randn(B, L, D, device=dev).to(bf))
        o = torch.empty(B * L, D, dtype=bf, device=dev)
        names, fns = [f"plain L={L}"], [lambda: ops.attention(q, k, vt, H, L, L, prescaled=True)]
        for w in wins:
            names.append(f"window {w}x{w}")
            fns.append(lambda w=w: ops.attention_window(q, k, vt, H, B, (hw, hw), (w, w), out=o))
            if other is not None and w * w <= 256:
                names.append(f"window {w}x{w} streamed form")
                fns.append(lambda w=w: other.mx_attention_window(_lib.current_stream(), q.data_ptr(), D, k.data_ptr(), D, vt.data_ptr(), vt.shape[2],
                                                                 D * vt.shape[2], o.data_ptr(), D, B, H, hw, hw, w, w))
        times = alternate(fns, args.reps, 20)
        say(f"  {hw}x{hw} H {H}: " + "   ".join(f"{n} {fmt(t, 1e3, 'us')}" for n, t in zip(names, times)))
    cfg, ocfg = (UNetConfig.tiny(), ref.UNetConfig.tiny()) if args.tiny else (UNetConfig.sdxl_base(), ref.UNetConfig.sdxl_base())
    net = MxUNet(cfg, ref.fast_params(ocfg), device=dev)
    batch, hw = (2, 64) if args.tiny else (8, 128)
    s, t, e, te, ti = (v.to(dev) for v in ref.make_inputs(ocfg, batch, hw))
    s, e = s.to(bf), e.to(bf)
    modes = [0, 128, 256]

    def step(tile):
        def run():
            net.enable_hypertile(tile_size=tile)
            net.forward_one(s, t, e, te, ti)
        return run
    say(f"step: MxUNet.forward_one, batch {batch}, {hw}x{hw} latents; median [p10 .. p90] over {max(args.reps // 3, 5)} alternating forwards")
    times = alternate([step(m) for m in modes], max(args.reps // 3, 5), 1)
    base = statistics.median(times[0])
    for m, tt in zip(modes, times):
        net.enable_hypertile(tile_size=m)
        name = "HyperTile off" if m == 0 else f"tile_size {m}: windows {net.hypertile_windows(hw, hw)}"
        say(f"  {name:72s} {fmt(tt, 1.0, 'ms')}   {statistics.median(tt) - base:+.2f} ms, ratio {statistics.median(tt) / base:.4f}")
    net.disable_hypertile()
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
