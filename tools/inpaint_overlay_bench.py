"""Cost of the three device operations around a request that repaints a crop of a client's photo -- the mask blur (mx_gaussian_blur_u8, radius 33),
the mask's bounding box (mx_mask_bbox_u8) and the overlay of the repainted crop (mx_rgb8_overlay) -- beside the same Pillow calls on a host core plus
the two copies they need (the device's bytes to the host and the result back).  Planes of 1024^2 and 4096^2.
Usage, on a machine with the GPU: python tools/inpaint_overlay_bench.py [--out profiles/inpaint_overlay.txt]
Legs per operation and size, alternating inside every repetition, medians:
  (a) the entry through ctypes with prepared arguments, device events around a run of calls on one input: the time per call as a stream of them
      runs (the blur is four launches a call, the bounding box a memset and a launch).  The operands stay in the 256 MB Infinity Cache at 1024^2;
  (b) copy to the host + the Pillow call + copy of the result to the device, a host clock around work that ends in a device synchronise; only where
      Pillow imports -- otherwise the file says it was not measured.  The bounding box returns four numbers: its leg (b) has one copy.
Before timing, the device's result is compared byte for byte with Pillow's (where Pillow imports).  A per-request cost, recorded, not asserted."""
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

SIZES = (1024, 4096)
RADIUS = 33.0
HBM_STREAM = 6.3e12                            # the rate its floors are quoted at

try:
    import PIL
    from PIL import Image, ImageFilter, ImageOps
except ImportError:
    PIL = Image = None


def _run_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def _host_us(fn):
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del r
    return dt * 1e6


def pillow_overlay(dec, orig, mask):
    """diffusers' apply_overlay without crop_coords, call for call"""
    init_image, image = Image.fromarray(orig, "RGB"), Image.fromarray(dec, "RGB")
    masked = Image.new("RGBa", (init_image.width, init_image.height))
    masked.paste(init_image.convert("RGBA").convert("RGBa"), mask=ImageOps.invert(Image.fromarray(mask, "L")))
    image = image.convert("RGBA")
    image.alpha_composite(masked.convert("RGBA"))
    return np.asarray(image.convert("RGB"))


def size_legs(n, reps, calls, warm, emit):
    l, stream = lib.load(), lib.current_stream()
    rng = np.random.RandomState(n)
    yy, xx = np.mgrid[:n, :n]
    hard = ((((yy - 0.55 * n) / (0.2 * n)) ** 2 + ((xx - 0.6 * n) / (0.25 * n)) ** 2) <= 1.0).astype(np.uint8) * 255      # an off-centre blob
    orig_h = rng.randint(0, 256, size=(n, n, 3)).astype(np.uint8)
    dec_h = rng.randint(0, 256, size=(n, n, 3)).astype(np.uint8)
    mask, orig, dec = torch.from_numpy(hard).cuda(), torch.from_numpy(orig_h).cuda(), torch.from_numpy(dec_h).cuda()
    soft, tmp, out = torch.empty_like(mask), torch.empty_like(mask), torch.empty_like(orig)
    box = torch.empty(4, dtype=torch.int32, device="cuda")

    def blur():
        return l.mx_gaussian_blur_u8(stream, mask.data_ptr(), soft.data_ptr(), tmp.data_ptr(), 1, n, n, RADIUS)

    def bbox():
        return l.mx_mask_bbox_u8(stream, soft.data_ptr(), box.data_ptr(), 1, n, n)

    def overlay():
        return l.mx_rgb8_overlay(stream, dec.data_ptr(), orig.data_ptr(), soft.data_ptr(), out.data_ptr(), 1, n, n, 0, 0, n, n)
    for fn in (blur, bbox, overlay):
        assert fn() == 0, l.mx_last_error()
    torch.cuda.synchronize()
    compared = "not compared (Pillow does not import)"
    if Image is not None:
        soft_h = np.asarray(Image.fromarray(hard, "L").filter(ImageFilter.GaussianBlur(RADIUS)))
        assert np.array_equal(soft.cpu().numpy(), soft_h), "the blurred mask differs from Pillow's"
        assert tuple(box.tolist()) == Image.fromarray(soft_h, "L").getbbox(), "the bounding box differs from Pillow's"
        assert np.array_equal(out.cpu().numpy(), pillow_overlay(dec_h, orig_h, soft_h)), "the overlay differs from Pillow's"
        compared = "equal to Pillow's, byte for byte"
    ops = [("blur r=33", blur, 2 * n * n, 8 * n * n), ("bbox", bbox, n * n, n * n), ("overlay", overlay, 10 * n * n, 10 * n * n)]
    legs = [(f"(a) {name}: device", (lambda fn=fn: _run_us(fn, calls)), floor, moved) for name, fn, floor, moved in ops]
    if Image is not None:
        legs.append(("(b) blur r=33: copy + Pillow + copy", lambda: _host_us(
            lambda: torch.from_numpy(np.asarray(Image.fromarray(mask.cpu().numpy(), "L").filter(ImageFilter.GaussianBlur(RADIUS)))).cuda()), 0, 0))
        legs.append(("(b) bbox: copy + Pillow", lambda: _host_us(lambda: Image.fromarray(soft.cpu().numpy(), "L").getbbox()), 0, 0))
        legs.append(("(b) overlay: copies + Pillow + copy", lambda: _host_us(
            lambda: torch.from_numpy(pillow_overlay(dec.cpu().numpy(), orig.cpu().numpy(), soft.cpu().numpy())).cuda()), 0, 0))
    for _ in range(warm):
        for leg in legs:
            leg[1]()
    torch.cuda.synchronize()
    times = [[] for _ in legs]
    for _ in range(reps):
        for i, leg in enumerate(legs):
            times[i].append(leg[1]())
    emit(f"{n} x {n}: mask {n * n / 1e6:.2f} MB, RGB image {3 * n * n / 1e6:.2f} MB; the device's bytes: {compared}")
    emit(f"  {reps} repetitions, legs alternating, after {warm} warm-ups; (a): device events around {calls} calls, us per call; (b): host clock, us per call")
    for (name, _fn, floor, moved), ts in zip(legs, times):
        q = statistics.quantiles(ts, n=10)
        med = statistics.median(ts)
        tail = f"   {floor / HBM_STREAM * 1e6:6.2f} us for its {floor / 1e6:.1f} MB of operands at 6.3 TB/s; moves {moved / 1e6:.1f} MB as built" if floor else ""
        emit(f"  {name:40s}: median {med:11.2f}  p10 {q[0]:11.2f}  p90 {q[-1]:11.2f}{tail}")
    if Image is None:
        emit("  (b) the Pillow legs: not measured (Pillow does not import here)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_overlay.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "inpaint_overlay_bench needs the GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"tools/inpaint_overlay_bench.py on {torch.cuda.get_device_name(0)}" + (f", Pillow {PIL.__version__}" if Image is not None else ", without Pillow"))
    for n in SIZES:
        size_legs(n, a.reps, a.calls, a.warmup, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
