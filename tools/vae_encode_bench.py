"""Latency of the VAE encoder (mx_vae_encode) and of its first launch (mx_conv3x3_rgb_in) at the SDXL widths, random-init weights.
Usage, on a machine with the GPU: python tools/vae_encode_bench.py
  1. conv_in: conv3x3_rgb_in_kernel (8-bit image in, rotated) against the route it replaces on the same tree -- the image written as NHWC bf16
     zero-padded to 64 channels (a torch copy into a zeroed buffer stands in for the prep launch) followed by mx_conv3x3 with cin_valid = 3 --
     device events around each launch, alternating repetitions, medians, beside the output-write floor.
  2. whole encode (encode_images, mode) beside whole decode (decode_images) in the same process, host clock between device synchronises."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sduss_amd import ops  # noqa: E402
from sduss_amd.vae import MxVAEDecoder, MxVAEEncoder, VAEConfig, conv_in_pack  # noqa: E402
from sduss_amd.weights import _conv_pack  # noqa: E402

SHAPES = ((512, 1), (1024, 1), (1024, 4))
HBM_TBS = 6.3        # the ceiling the write floor is set beside (TB/s)


def _event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _med(ts):
    q = statistics.quantiles(ts, n=10)
    return f"median {statistics.median(ts):9.1f}  p10 {q[0]:9.1f}  p90 {q[-1]:9.1f}"


def conv_in_leg(n=128, reps=20, warm=3):
    g = torch.Generator().manual_seed(2)
    w4 = (torch.randn(n, 3, 3, 3, generator=g) * 27 ** -0.5)
    w32 = conv_in_pack(w4).to(torch.bfloat16).cuda()
    w64 = _conv_pack(w4, 64).to(torch.bfloat16).cuda()
    bias = torch.zeros(n, device="cuda")
    for res, batch in SHAPES:
        img = torch.randint(0, 256, (batch, res, res, 3), generator=g, dtype=torch.uint8).cuda()
        y = torch.empty((batch, res, res, n), dtype=torch.bfloat16, device="cuda")
        xpad = torch.zeros((batch, res, res, 64), dtype=torch.bfloat16, device="cuda")

        def new():
            ops.conv3x3_rgb_in(img, w32, bias, rotate=True, out=y)

        def prep():
            xpad[..., :3] = img.flip(1, 2).float().div_(255.0).mul_(2.0).sub_(1.0)

        def old():
            return ops.conv3x3(xpad, w64, bias, cin_valid=3)

        for _ in range(warm):
            new(); prep(); y_old = old()
        torch.cuda.synchronize()
        same = float((y.float() - y_old.float()).abs().max())
        del y_old
        tn, tp, to = [], [], []
        for _ in range(reps):
            tn.append(_event_us(new)); tp.append(_event_us(prep)); to.append(_event_us(old))
        out_mb = batch * res * res * n * 2 / 1e6
        floor = out_mb / HBM_TBS            # MB / (TB/s) = us
        print(f"conv_in {res}x{res} batch {batch}, N = {n}: output {out_mb:.0f} MB, write floor at {HBM_TBS} TB/s {floor:.1f} us; "
              f"{reps} alternating repetitions after {warm} warm-ups, device events, us:")
        print(f"  conv3x3_rgb_in_kernel (uint8 in)           : {_med(tn)}   ({out_mb / statistics.median(tn):.2f} TB/s written)")
        print(f"  replaced route, mx_conv3x3 cin_valid = 3   : {_med(to)}")
        print(f"  replaced route, pad-to-64 prep (torch ops) : {_med(tp)}")
        print(f"  max |new - replaced route| over the outputs: {same:.4f}", flush=True)
        del img, y, xpad
        torch.cuda.empty_cache()


def _params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    P = {}
    for k, s in shapes.items():
        if len(s) > 1:
            fan = 1
            for d in s[1:]:
                fan *= d
            P[k] = torch.randn(s, generator=g) * fan ** -0.5
        else:
            P[k] = (1.0 if k.endswith("weight") else 0.0) + 0.05 * torch.randn(s, generator=g)
    return P


def encode_leg(reps=10, warm=2):
    import vae_bench
    import vae_encode_ref
    from oracle import vae_ref
    cfg = VAEConfig.sdxl()
    enc = MxVAEEncoder(cfg, _params(vae_encode_ref.param_shapes(vae_ref.VAEConfig.sdxl()), 1), device="cuda:0")
    dec = MxVAEDecoder(cfg, _params(vae_bench.shapes(cfg), 1), device="cuda:0")
    for res, batch in SHAPES:
        g = torch.Generator().manual_seed(res + batch)
        img = torch.randint(0, 256, (batch, res, res, 3), generator=g, dtype=torch.uint8).cuda()
        lat = torch.randn(batch, 4, res // 8, res // 8, generator=g).to(torch.bfloat16).cuda()
        for _ in range(warm):
            out = enc.encode_images(img); dec.decode_images(lat)
        te, td = [], []
        for _ in range(reps):
            te.append(_host_ms(lambda: enc.encode_images(img))); td.append(_host_ms(lambda: dec.decode_images(lat)))
        me, md = statistics.median(te), statistics.median(td)
        print(f"vae {res}x{res} batch {batch}, {reps} alternating repetitions after {warm} warm-ups, host clock between synchronises, ms:")
        print(f"  mx_vae_encode (uint8 image -> latents, mode) : median {me:8.3f}  min {min(te):8.3f}  max {max(te):8.3f}   {me / batch:8.3f} ms/image, finite {bool(torch.isfinite(out.float()).all())}")
        print(f"  mx_vae_decode_rgb8 (latents -> uint8 image)  : median {md:8.3f}  min {min(td):8.3f}  max {max(td):8.3f}   {md / batch:8.3f} ms/image", flush=True)
        del img, lat
        torch.cuda.empty_cache()


if __name__ == "__main__":
    conv_in_leg()
    encode_leg()
