"""Per-shape A/B of the 3x3 conv entries at the stride-1 shapes of the SDXL headline step (batch 4 with guidance = 8 images): mx_conv3x3
(tap-major, the 256 x 160 tile of gemm_bf16_v5.hip) against the staged entry that serves the descriptor -- mx_conv3x3_halo at the 32 and 64 wide
levels, mx_conv3x3_halfrow at the 128 wide level (both conv_halo.hip).
Usage, on a machine with the GPU: python tools/conv_halo_bench.py [--reps 60] [--widths 32,64,128] [--out FILE]
One process, random data, device events around every launch, the two entries alternating; a launch rotates through NSETS operand sets so that
neither entry finds its weights warm from its own last launch.  Reports median and p10..p90 per entry and shape.  A shape counts as FASTER only
when the new median beats the old one by more than the old entry's own p10..p90 width.  Also prints the largest difference between the two
outputs relative to the largest output (the orders of summation differ: last bits)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd import lib as L  # noqa: E402

BATCH = 8
# (H = W, Cin, N, launches per step): the stride-1, not upsampled conv rows of profiles/r04_a_shape_profile_b4.txt at the 32, 64 and 128 wide levels
# (128: 320 -> 320 is down block 0 (4, conv1 and conv2 alike) and conv2 of up block 2 (3); 640 / 960 -> 320 are the conv1 of up block 2)
SHAPES = ((32, 1280, 1280, 10), (32, 2560, 1280, 2), (32, 1920, 1280, 1), (32, 640, 1280, 1),
          (64, 640, 640, 6), (64, 1920, 640, 1), (64, 1280, 640, 1), (64, 960, 640, 1), (64, 320, 640, 1),
          (128, 320, 320, 7), (128, 640, 320, 2), (128, 960, 320, 1))
NSETS = 4
WARM = 3


def _event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3


def _stats(ts):
    q = statistics.quantiles(ts, n=10)
    return statistics.median(ts), q[0], q[-1]


def _operands(hw, cin, n, form, g):
    """form 'conv1': bias + per-sample row bias (the time embedding); 'conv2': bias + residual"""
    bf = torch.bfloat16
    m = BATCH * hw * hw
    x = torch.randn((m, cin), generator=g).to(bf).cuda()
    w = (torch.randn((n, 9 * cin), generator=g) * (9 * cin) ** -0.5).to(bf).cuda()
    bias = torch.randn(n, generator=g).cuda()
    extra = torch.randn((BATCH, n), generator=g).cuda() if form == "conv1" else torch.randn((m, n), generator=g).to(bf).cuda()
    out = torch.empty((m, n), dtype=bf, device="cuda")
    d = L.GemmDesc()
    d.a, d.w, d.c, d.bias = x.data_ptr(), w.data_ptr(), out.data_ptr(), bias.data_ptr()
    d.M, d.N, d.K, d.ldc, d.ldr = m, n, 9 * cin, n, n
    d.rows_per_batch = hw * hw
    d.B, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride = BATCH, hw, hw, cin, hw, hw, 1
    if form == "conv1":
        d.rowbias, d.ldrb = extra.data_ptr(), n
    else:
        d.residual = extra.data_ptr()
    return d, out, (x, w, bias, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--widths", default="32,64,128", help="image widths to run, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    widths = {int(v) for v in a.widths.split(",")}
    assert a.reps >= 20 and torch.cuda.is_available(), "needs a GPU and at least 20 repetitions"
    lib = L.load()
    s = L.current_stream()
    g = torch.Generator().manual_seed(11)
    lines = [f"conv_halo_bench: batch {BATCH}, {a.reps} repetitions per entry, alternating, {NSETS} operand sets in rotation; times in us (device events)",
             f"{'H=W':>4} {'Cin':>5} {'N':>5} {'form':>6} {'n/step':>6} | {'old med':>8} {'p10':>8} {'p90':>8} | {'new med':>8} {'p10':>8} {'p90':>8} | {'gain':>7} {'old width':>9}  verdict   max|new-old|/max|old|"]
    saved = 0.0
    for hw, cin, n, per_step in SHAPES:
        if hw not in widths:
            continue
        for form in ("conv1", "conv2") if cin == n else ("conv1",):
            sets = [_operands(hw, cin, n, form, g) for _ in range(NSETS)]
            d0 = sets[0][0]
            assert L.gemm_kernels_of(d0, True)[0].startswith("gemm_v5_kernel<160"), (hw, cin, n)
            if lib.mx_conv3x3_halo_serves(C.byref(d0)):
                entry, entry_name = lib.mx_conv3x3_halo, "mx_conv3x3_halo"
            elif lib.mx_conv3x3_halfrow_serves(C.byref(d0)):
                entry, entry_name = lib.mx_conv3x3_halfrow, "mx_conv3x3_halfrow"
            else:                                                  # a shape an earlier run of this comparison excluded
                lines.append(f"{hw:>4} {cin:>5} {n:>5} {form:>6} {per_step:>6} | not served by mx_conv3x3_halo / mx_conv3x3_halfrow (their _serves)")
                continue
            old = lambda k: L.check(lib.mx_conv3x3(s, C.byref(sets[k][0])), "mx_conv3x3")
            new = lambda k: L.check(entry(s, C.byref(sets[k][0])), entry_name)
            old(0); ref = sets[0][1].float().clone()
            new(0); diff = (sets[0][1].float() - ref).abs().max().item() / ref.abs().max().item()
            for _ in range(WARM):                       # every operand set through both entries: code objects, clocks, allocator
                for k in range(NSETS):
                    old(k); new(k)
            t_old, t_new = [], []
            for r in range(a.reps):
                k = r % NSETS
                t_old.append(_event_us(lambda: old(k)))
                t_new.append(_event_us(lambda: new(k)))
            (mo, lo, ho), (mn, ln, hn) = _stats(t_old), _stats(t_new)
            faster = mo - mn > ho - lo
            if faster and form == "conv1":
                saved += (mo - mn) * per_step
            lines.append(f"{hw:>4} {cin:>5} {n:>5} {form:>6} {per_step:>6} | {mo:8.1f} {lo:8.1f} {ho:8.1f} | {mn:8.1f} {ln:8.1f} {hn:8.1f} | {mo - mn:7.1f} {ho - lo:9.1f}  "
                         f"{'FASTER' if faster else 'not faster':<10} {diff:.2e}")
            del sets
            torch.cuda.empty_cache()
    lines.append(f"sum over the shapes that count as faster of gain x launches per step (conv1 rows): {saved / 1e3:.2f} ms per step")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
