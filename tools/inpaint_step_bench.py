"""Cost of the masked scheduler step (mx_cfg_euler_step_masked / mx_cfg_flow_step_masked) beside the plain one it extends, at the latents of a batch
of eight 1024 px requests: 8 x 4 x 128 x 128 (SDXL) and 8 x 16 x 128 x 128 (SD3), bf16, CFG on.
Usage, on a machine with the GPU: python tools/inpaint_step_bench.py [--out profiles/inpaint_step.txt]
Legs per model: the plain step, and the masked step with 0, half and all rows inpainting (random half-zero masks, so nearly every vector of an
inpainting row reads init and noise).  The entries are called through ctypes with prepared arguments, so a launch costs the host a few
microseconds; device events around runs of launches, the legs alternating inside every repetition, medians: the time per launch as a stream of them
runs, an upper bound on the kernel's own time where the host or the launch path is the slower side.  Beside each
time: the bytes the leg has to move (prediction, latents read and written, and for inpainting rows init + noise + mask) and that over the time.
sigma_next = sigma in every launch, so the in-place latents stay what they are however often the step runs."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd import lib  # noqa: E402

N_LAT, HW = 8, 128
STEP_MS = 55.0        # the denoising step these launches end (bench.py's flagship batch), for the share


def _run_us(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def model_legs(name, C, plain, masked, g, reps, launches, warm, emit):
    gen = torch.Generator().manual_seed(C)
    dt = torch.bfloat16
    pred = torch.randn(2 * N_LAT, C, HW, HW, generator=gen).to(dt).cuda()
    lat = torch.randn(N_LAT, C, HW, HW, generator=gen).to(dt).cuda()
    sigma = torch.linspace(0.9, 0.2, N_LAT).cuda()
    init = torch.randn(N_LAT, C, HW, HW, generator=gen).to(dt).cuda()
    noise = torch.randn(N_LAT, C, HW, HW, generator=gen).to(dt).cuda()
    mask = torch.randint(0, 2, (N_LAT, HW, HW), generator=gen, dtype=torch.uint8).cuda()
    elems = C * HW * HW
    base_bytes = (2 * N_LAT + 2 * N_LAT) * elems * 2
    l, stream, code = lib.load(), lib.current_stream(), lib.torch_dtype_code(dt)
    plain_fn, masked_fn = getattr(l, plain), getattr(l, masked)
    head = (stream, pred.data_ptr(), lat.data_ptr(), sigma.data_ptr(), sigma.data_ptr(), g, N_LAT)
    legs = [("plain step", lambda: plain_fn(*head, elems, code), base_bytes)]
    keepalive = []
    for k in (0, N_LAT // 2, N_LAT):
        slot = torch.tensor([i // 2 if (i % 2 == 0 and i // 2 < k) else -1 for i in range(N_LAT)] if k < N_LAT else list(range(N_LAT)), dtype=torch.int32).cuda()
        assert int((slot >= 0).sum()) == k
        rows = lib.InpaintRows()
        if k:
            rows.k, rows.slot, rows.init, rows.noise, rows.mask = k, slot.data_ptr(), init.data_ptr(), noise.data_ptr(), mask.data_ptr()
        keepalive.append((slot, rows))
        legs.append((f"masked step, {k} of {N_LAT} rows inpainting", (lambda rows=rows: masked_fn(*head, C, HW * HW, code, lib.C.byref(rows))),
                     base_bytes + k * (2 * elems * 2 + HW * HW)))
    for _n, fn, _b in legs:
        assert fn() == 0, l.mx_last_error()
    for _ in range(warm):
        for _n, fn, _b in legs:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in legs]
    for _ in range(reps):
        for i, (_n, fn, _b) in enumerate(legs):
            times[i].append(_run_us(fn, launches))
    emit(f"{name}: latents {N_LAT} x {C} x {HW} x {HW} bf16, guidance {g}; {reps} repetitions of {launches} launches per leg, legs alternating, after {warm} "
         f"warm-ups; device events, us per launch")
    t_plain = statistics.median(times[0])
    for (n, _fn, nbytes), ts in zip(legs, times):
        q = statistics.quantiles(ts, n=10)
        med = statistics.median(ts)
        emit(f"  {n:38s}: median {med:8.2f}  p10 {q[0]:8.2f}  p90 {q[-1]:8.2f}   {nbytes / 1e6:7.1f} MB -> {nbytes / med / 1e6:5.2f} TB/s   "
             f"{med - t_plain:+7.2f} us on the plain step = {100.0 * (med - t_plain) / (STEP_MS * 1e3):+.4f} % of a {STEP_MS:.0f} ms step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_step.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "inpaint_step_bench needs the GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"tools/inpaint_step_bench.py on {torch.cuda.get_device_name(0)}")
    model_legs("SDXL, mx_cfg_euler_step vs mx_cfg_euler_step_masked", 4, "mx_cfg_euler_step", "mx_cfg_euler_step_masked", 5.0, a.reps, a.launches, a.warmup, emit)
    model_legs("SD3, mx_cfg_flow_step vs mx_cfg_flow_step_masked", 16, "mx_cfg_flow_step", "mx_cfg_flow_step_masked", 7.0, a.reps, a.launches, a.warmup, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
