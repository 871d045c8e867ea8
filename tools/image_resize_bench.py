"""Cost of resizing a client's image to the request's resolution on the device (mx_resize_u8) beside what callers do without it: Pillow's resize on
a host core plus the copy of its result to the device.  Three shapes, RGB, lanczos (diffusers' default): 2048^2 -> 1024^2, 1536 x 1024 -> 1024^2
(H x W; only the vertical pass does work), 640 x 480 -> 512^2 (W x H as a camera names it: 480 x 640 here).
Usage, on a machine with the GPU: python tools/image_resize_bench.py [--out profiles/image_resize_mi355x.txt]
Legs per shape, alternating inside every repetition, medians:
  (a)  mx_resize_u8 through ctypes with prepared arguments, device events around a run of launches on ONE input: the time per launch as a stream of
       them runs.  The input and the tables stay in the 256 MB Infinity Cache, so this is not an HBM figure;
  (a') the same launches walking a ring of inputs larger than the Infinity Cache, so that every launch reads its image from HBM;
  (b)  Image.resize on the host + torch's copy of the result to the device, a host clock around work that ends in a device synchronise; only where
       Pillow imports -- otherwise the file says it was not measured.
Beside each time: the bytes the resize has to move (input read once, output written once) over the time, and the HBM floor of those bytes at DESIGN.md
section 4's rates.  Before timing, the device's result is compared byte for byte with Pillow's (where Pillow imports)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd import lib  # noqa: E402

SHAPES = ((2048, 2048, 1024, 1024), (1536, 1024, 1024, 1024), (480, 640, 512, 512))      # in_h, in_w, out_h, out_w
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12          # the peak, and the rate its floors are quoted at
RING_BYTES = 640 << 20                         # inputs of leg (a'): more than twice the Infinity Cache

try:
    import PIL
    from PIL import Image
except ImportError:
    PIL = Image = None


def _run_us(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def shape_legs(ih, iw, oh, ow, reps, launches, warm, emit):
    l, stream = lib.load(), lib.current_stream()
    rng = np.random.RandomState(ih + ow)
    host = rng.randint(0, 256, size=(ih, iw, 3)).astype(np.uint8)
    n_in, n_out = host.size, oh * ow * 3
    ring_n = max(2, RING_BYTES // n_in)
    ring = torch.from_numpy(host).cuda().reshape(1, -1).repeat(ring_n, 1).contiguous()          # the same image ring_n times, at distinct addresses
    out = torch.empty((1, oh, ow, 3), dtype=torch.uint8, device="cuda")
    plan = l.mx_resize_create(ih, iw, oh, ow, lib.RESIZE_FILTERS["lanczos"])
    assert plan, l.mx_last_error()
    src = [ring[i].data_ptr() for i in range(ring_n)]
    dst = out.data_ptr()
    assert l.mx_resize_u8(plan, stream, src[0], dst, 1, 3) == 0, l.mx_last_error()
    torch.cuda.synchronize()
    compared = "not compared (Pillow does not import)"
    if Image is not None:
        want = np.asarray(Image.fromarray(host).resize((ow, oh), resample=Image.Resampling.LANCZOS))
        assert np.array_equal(out[0].cpu().numpy(), want), "the device's bytes differ from Pillow's"
        compared = "equal to Pillow's, byte for byte"

    legs = [("(a)  mx_resize_u8, one input (cache-resident)", lambda: _run_us(lambda i: l.mx_resize_u8(plan, stream, src[0], dst, 1, 3), launches)),
            (f"(a') mx_resize_u8, ring of {ring_n} inputs = {ring_n * n_in >> 20} MiB", lambda: _run_us(lambda i: l.mx_resize_u8(plan, stream, src[i % ring_n], dst, 1, 3), launches))]
    if Image is not None:
        def pillow_leg():
            t0 = time.perf_counter()
            r = torch.from_numpy(np.asarray(Image.fromarray(host).resize((ow, oh), resample=Image.Resampling.LANCZOS))).cuda()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            del r
            return dt * 1e6
        legs.append(("(b)  Pillow on the host + copy to the device", pillow_leg))
    for _ in range(warm):
        for _n, fn in legs:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in legs]
    for _ in range(reps):
        for i, (_n, fn) in enumerate(legs):
            times[i].append(fn())
    l.mx_resize_destroy(plan)
    moved = n_in + n_out
    emit(f"{ih} x {iw} -> {oh} x {ow} RGB lanczos: {n_in / 1e6:.2f} MB read once + {n_out / 1e6:.2f} MB written once = {moved / 1e6:.2f} MB; HBM floor "
         f"{moved / HBM_PEAK * 1e6:.2f} us at 8 TB/s, {moved / HBM_STREAM * 1e6:.2f} us at 6.3 TB/s; the device's bytes: {compared}")
    emit(f"  {reps} repetitions, legs alternating, after {warm} warm-ups; (a), (a'): device events around {launches} launches, us per launch; (b): host clock, us per image")
    for (n, _fn), ts in zip(legs, times):
        q = statistics.quantiles(ts, n=10)
        med = statistics.median(ts)
        emit(f"  {n:52s}: median {med:10.2f}  p10 {q[0]:10.2f}  p90 {q[-1]:10.2f}   {moved / med / 1e6:7.3f} TB/s of the bytes above")
    if Image is None:
        emit("  (b)  Pillow on the host + copy to the device: not measured (Pillow does not import here)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_resize_mi355x.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "image_resize_bench needs the GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"tools/image_resize_bench.py on {torch.cuda.get_device_name(0)}" + (f", Pillow {PIL.__version__}" if Image is not None else ", without Pillow"))
    for shape in SHAPES:
        shape_legs(*shape, a.reps, a.launches, a.warmup, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
