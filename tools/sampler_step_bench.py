"""Cost of the multistep scheduler launch (mx_cfg_multistep_step) beside the plain step it stands in for, at the latents of a batch of eight 1024 px
requests: 8 x 4 x 128 x 128 (SDXL) and 8 x 16 x 128 x 128 (SD3), bf16, CFG on.
Usage, on a machine with the GPU: python tools/sampler_step_bench.py [--out profiles/sampler_step.txt]
Legs per model: the plain step, and the multistep launch with all rows Euler (kind 0: the history is not touched), half of the rows multistep and
all rows multistep (DPM-Solver++ 2M rows for SDXL, AB2 rows for SD3, second order: the fp32 history is read and written, 4 more bytes per element
each way).  The entries are called through ctypes with prepared arguments; device events around runs of launches, the legs alternating inside every
repetition, medians -- the method of tools/inpaint_step_bench.py.  Beside each time: the bytes the leg has to move and that over the time.
sigma_next = sigma and the multistep coefficients (1, 0, 1e-30) in every launch, so the in-place latents stay what they are however often the step
runs, while c1 != 0 keeps the history read.  Nothing is asserted beyond the launches' status.
The stochastic leg (--out-stochastic profiles/stochastic_step.txt): mx_cfg_stochastic_step, every row a second-order kind-1 row with noise made in the
launch, beside the only alternative without it -- mx_cfg_multistep_step, then torch.randn of the latents' shape, then one in-place scaled add
(addcmul_) -- at the two shapes above and at 128 x 16 x 128 x 128 bf16, whose operands (0.6 GB) leave the caches.  cn = 1e-3, so the latents stay
finite over the run.  --only multistep | stochastic runs one of the two."""
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


def model_legs(name, C, plain, flow, kind, g, reps, launches, warm, emit):
    gen = torch.Generator().manual_seed(C)
    dt = torch.bfloat16
    pred = torch.randn(2 * N_LAT, C, HW, HW, generator=gen).to(dt).cuda()
    lat = torch.randn(N_LAT, C, HW, HW, generator=gen).to(dt).cuda()
    hist = torch.randn(N_LAT, C, HW, HW, generator=gen).cuda()
    sigma = torch.linspace(0.9, 0.2, N_LAT).cuda()
    coef = torch.tensor([[1.0, 0.0, 1e-30]] * N_LAT, dtype=torch.float32).cuda()
    elems = C * HW * HW
    base_bytes = (2 * N_LAT + 2 * N_LAT) * elems * 2
    l, stream, code = lib.load(), lib.current_stream(), lib.torch_dtype_code(dt)
    plain_fn, multi_fn = getattr(l, plain), l.mx_cfg_multistep_step
    head = (stream, pred.data_ptr(), lat.data_ptr(), sigma.data_ptr(), sigma.data_ptr(), g, N_LAT)
    legs = [("plain step", lambda: plain_fn(*head, elems, code), base_bytes)]
    keepalive = []
    for k in (0, N_LAT // 2, N_LAT):
        kinds = torch.tensor([kind if (i % 2 == 0 and i // 2 < k) or k == N_LAT else 0 for i in range(N_LAT)], dtype=torch.int32).cuda()
        assert int((kinds != 0).sum()) == k
        ms = lib.MultistepRows()
        ms.kind, ms.coef, ms.hist = kinds.data_ptr(), coef.data_ptr(), hist.data_ptr()
        keepalive.append((kinds, ms))
        legs.append((f"multistep launch, {k} of {N_LAT} rows multistep", (lambda ms=ms: multi_fn(*head, C, HW * HW, code, flow, lib.C.byref(ms), None)),
                     base_bytes + k * 2 * elems * 4))
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
        emit(f"  {n:40s}: median {med:8.2f}  p10 {q[0]:8.2f}  p90 {q[-1]:8.2f}   {nbytes / 1e6:7.1f} MB -> {nbytes / med / 1e6:5.2f} TB/s   "
             f"{med - t_plain:+7.2f} us on the plain step = {100.0 * (med - t_plain) / (STEP_MS * 1e3):+.4f} % of a {STEP_MS:.0f} ms step")
    assert bool(torch.isfinite(lat.float()).all()) and bool(torch.isfinite(hist).all())


def stochastic_legs(n_lat, C, reps, launches, warm, emit):
    gen = torch.Generator().manual_seed(C + n_lat)
    dt = torch.bfloat16
    g = 5.0
    pred = torch.randn(2 * n_lat, C, HW, HW, generator=gen).to(dt).cuda()
    lat = torch.randn(n_lat, C, HW, HW, generator=gen).to(dt).cuda()
    hist = torch.randn(n_lat, C, HW, HW, generator=gen).cuda()
    sigma = torch.linspace(0.9, 0.2, n_lat).cuda()
    coef = torch.tensor([[1.0, 0.0, 1e-30]] * n_lat, dtype=torch.float32).cuda()
    kinds = torch.full((n_lat,), lib.MX_SAMPLER_DPMPP_2M, dtype=torch.int32).cuda()
    cn = torch.full((n_lat,), 1e-3, dtype=torch.float32).cuda()
    cn_rows = cn.to(dt).reshape(n_lat, 1, 1, 1)
    seed = torch.arange(1, n_lat + 1, dtype=torch.int64).cuda()
    step = torch.zeros(n_lat, dtype=torch.int32).cuda()
    elems = C * HW * HW
    l, stream, code = lib.load(), lib.current_stream(), lib.torch_dtype_code(dt)
    ms, nz = lib.MultistepRows(), lib.NoiseRows()
    ms.kind, ms.coef, ms.hist = kinds.data_ptr(), coef.data_ptr(), hist.data_ptr()
    nz.cn, nz.seed, nz.step = cn.data_ptr(), seed.data_ptr(), step.data_ptr()
    head = (stream, pred.data_ptr(), lat.data_ptr(), sigma.data_ptr(), sigma.data_ptr(), g, n_lat, C, HW * HW, code, 0, lib.C.byref(ms), None)

    def fused():
        return l.mx_cfg_stochastic_step(*head, lib.C.byref(nz))

    def unfused():
        status = l.mx_cfg_multistep_step(*head)
        lat.addcmul_(torch.randn(lat.shape, device=lat.device, dtype=dt), cn_rows)
        return status
    step_bytes = (2 * n_lat + 2 * n_lat) * elems * 2 + n_lat * 2 * elems * 4
    legs = [("mx_cfg_stochastic_step", fused, step_bytes), ("mx_cfg_multistep_step + torch.randn + addcmul_", unfused, step_bytes + 4 * n_lat * elems * 2)]
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
    emit(f"stochastic step: latents {n_lat} x {C} x {HW} x {HW} bf16, guidance {g}, every row second order with noise; {reps} repetitions of {launches} "
         f"steps per leg, legs alternating, after {warm} warm-ups; device events, us per step")
    t_fused = statistics.median(times[0])
    for (n, _fn, nbytes), ts in zip(legs, times):
        q = statistics.quantiles(ts, n=10)
        med = statistics.median(ts)
        emit(f"  {n:48s}: median {med:8.2f}  p10 {q[0]:8.2f}  p90 {q[-1]:8.2f}   {nbytes / 1e6:7.1f} MB -> {nbytes / med / 1e6:5.2f} TB/s   "
             f"{med - t_fused:+8.2f} us on the fused launch")
    assert bool(torch.isfinite(lat.float()).all()) and bool(torch.isfinite(hist).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_step.txt"))
    ap.add_argument("--out-stochastic", default=os.path.join(ROOT, "profiles", "stochastic_step.txt"))
    ap.add_argument("--only", choices=("multistep", "stochastic"), default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sampler_step_bench needs the GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def write(path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        lines.clear()
    if a.only != "stochastic":
        emit(f"tools/sampler_step_bench.py on {torch.cuda.get_device_name(0)}")
        model_legs("SDXL, mx_cfg_euler_step vs mx_cfg_multistep_step (DPM-Solver++ 2M rows)", 4, "mx_cfg_euler_step", 0, lib.MX_SAMPLER_DPMPP_2M, 5.0,
                   a.reps, a.launches, a.warmup, emit)
        model_legs("SD3, mx_cfg_flow_step vs mx_cfg_multistep_step (AB2 rows)", 16, "mx_cfg_flow_step", 1, lib.MX_SAMPLER_AB2, 7.0, a.reps, a.launches, a.warmup,
                   emit)
        write(a.out)
    if a.only != "multistep":
        emit(f"tools/sampler_step_bench.py, the stochastic leg, on {torch.cuda.get_device_name(0)}")
        for n_lat, C in ((N_LAT, 4), (N_LAT, 16), (128, 16)):
            stochastic_legs(n_lat, C, a.reps, a.launches, a.warmup, emit)
        write(a.out_stochastic)


if __name__ == "__main__":
    main()
