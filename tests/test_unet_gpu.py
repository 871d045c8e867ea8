"""GPU parity of the whole UNet step plan (outer boundary) against the CPU oracle, tiny SDXL-topology config with
seeded synthetic weights shared bit-for-bit by both sides (bf16-representable).

Tolerance: activations are stored in bf16 between ~40 fused kernels (2^-9 relative rounding each, fp32 accumulate);
the oracle is fp32 end to end.  Bound used: max|hip - oracle| <= 4% of max|oracle| and relative L2 <= 2%."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import patch_ref, sdxl_unet_ref as ref  # noqa: E402  (checker only)


@pytest.fixture(scope="module")
def tiny(cuda_device):
    from sduss_amd.config import UNetConfig
    from sduss_amd.unet import MxUNet
    ocfg = ref.UNetConfig.tiny()
    P = ref.init_params(ocfg)
    net = MxUNet(UNetConfig.tiny(), P, device="cuda:0")
    return ocfg, P, net


def _check(got, want, what, max_rel=0.04, l2_rel=0.02):
    got = got.float().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    l2 = ((got - want).norm() / want.norm()).item()
    print(f"{what}: max err {err:.4f} ({err / scale:.4f} of max), rel L2 {l2:.4f}")
    assert err <= max_rel * scale, f"{what}: max err {err} vs scale {scale}"
    assert l2 <= l2_rel, f"{what}: rel L2 {l2}"


@pytest.mark.parametrize("batch,hw", [(2, 32), (1, 16), (3, 24)])
def test_unet_unsliced(tiny, batch, hw):
    ocfg, P, net = tiny
    if hw % 4:
        pytest.skip("latent must be divisible by 4")
    s, t, e, te, ti = ref.make_inputs(ocfg, batch, hw)
    want = ref.unet_forward(P, ocfg, s, t, e, te, ti)
    key = str(hw * 8)
    out = net.forward({key: s.cuda().to(torch.bfloat16)}, t.cuda(), e.cuda(), added_cond_kwargs={"text_embeds": te.cuda(), "time_ids": ti.cuda()},
                      return_dict=False, is_sliced=False, patch_size=hw * 8, input_indices={key: [str(i) for i in range(batch)]})[0]
    assert list(out.keys()) == [key] and out[key].shape == s.shape
    _check(out[key], want, f"unet unsliced b{batch} {hw}x{hw}")


@pytest.mark.parametrize("patch_px", [128, 64])
def test_unet_sliced_matches_reference_patch_pipeline(tiny, patch_px):
    """is_sliced=True: the whole-image HIP plan must equal the reference's literal patch pipeline (split_sample ->
    per-patch convs on halo'd patches with the native op's corner semantics -> patch-averaged GroupNorm -> regrouped
    attention -> concat_sample), restated in oracle/patch_ref.py."""
    ocfg, P, net = tiny
    s, t, e, te, ti = ref.make_inputs(ocfg, 2, 32)
    want = patch_ref.unet_forward_sliced(P, ocfg, {"256": s}, t, e, te, ti, patch_size=patch_px)["256"]
    exact = ref.unet_forward(P, ocfg, s, t, e, te, ti)
    out = net.forward({"256": s.cuda().to(torch.bfloat16)}, t.cuda(), e.cuda(), added_cond_kwargs={"text_embeds": te.cuda(), "time_ids": ti.cuda()},
                      return_dict=False, is_sliced=True, patch_size=patch_px, input_indices={"256": ["0", "1"]})[0]["256"]
    _check(out, want, f"unet sliced patch {patch_px}")
    # and the sliced result is measurably NOT the unsliced one (the approximation is reproduced, not ignored)
    assert (out.float().cpu() - exact).abs().max() > 3 * (out.float().cpu() - want).abs().max()


def test_unet_mixed_resolutions_sliced(tiny):
    """Two resolutions in one call, conditioning rows concatenated in ascending-resolution order (pipeline :275-339)."""
    ocfg, P, net = tiny
    s1, t1, e1, te1, ti1 = ref.make_inputs(ocfg, 1, 16, seed=1)
    s2, t2, e2, te2, ti2 = ref.make_inputs(ocfg, 2, 32, seed=2)
    t = torch.cat([t1, t2]); e = torch.cat([e1, e2]); te = torch.cat([te1, te2]); ti = torch.cat([ti1, ti2])
    want = patch_ref.unet_forward_sliced(P, ocfg, {"128": s1, "256": s2}, t, e, te, ti, patch_size=64)
    out = net.forward({"128": s1.cuda().to(torch.bfloat16), "256": s2.cuda().to(torch.bfloat16)}, t.cuda(), e.cuda(),
                      added_cond_kwargs={"text_embeds": te.cuda(), "time_ids": ti.cuda()}, return_dict=False, is_sliced=True,
                      patch_size=64, input_indices={"128": ["0"], "256": ["1", "2"]})[0]
    for k in ("128", "256"):
        _check(out[k], want[k], f"mixed-res sliced {k}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_unet_io_dtypes(tiny, dtype):
    """The reference hands fp16 latents; the boundary converts at the edge kernels."""
    ocfg, P, net = tiny
    s, t, e, te, ti = ref.make_inputs(ocfg, 1, 16)
    want = ref.unet_forward(P, ocfg, s, t, e, te, ti)
    out = net.forward_one(s.cuda().to(dtype), t.cuda(), e.cuda(), te.cuda(), ti.cuda())
    assert out.dtype == dtype
    _check(out, want, f"unet io {dtype}")


def test_denoising_step_two_steps(tiny):
    """pipeline.denoising_step (gather -> scale+CFG dup -> UNet -> CFG combine -> Euler) vs the same sequence built from
    the oracle pieces, two consecutive steps on two requests."""
    from oracle import scheduler_ref
    from sduss_amd.config import UNetConfig
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    ocfg, P, net = tiny
    cfg = UNetConfig.tiny()
    den = SDXLDenoiser(net, guidance_scale=5.0)
    reqs = [synthetic_request(i, 128, 4, cfg, den, "cuda:0", dtype=torch.bfloat16) for i in range(2)]
    lat = torch.cat([r.latents for r in reqs]).float().cpu()
    pe = reqs[0].prompt_embeds.float().cpu(); ne = reqs[0].negative_prompt_embeds.float().cpu()
    pp = reqs[0].pooled_prompt_embeds.float().cpu(); npp = reqs[0].negative_pooled_prompt_embeds.float().cpu()
    tid = reqs[0].add_time_ids.float().cpu()
    ts, sig, _ = scheduler_ref.sdxl_euler_tables(4)
    for step in range(2):
        den.denoising_step({"128": reqs})
        x2 = scheduler_ref.scale_model_input(torch.cat([lat, lat]), sig[[step] * 4])
        noise = ref.unet_forward(P, ocfg, x2, ts[[step] * 4], torch.cat([ne, ne, pe, pe]), torch.cat([npp, npp, pp, pp]), tid.repeat(4, 1))
        lat = scheduler_ref.euler_step(scheduler_ref.cfg_combine(noise, 5.0), lat, sig[[step] * 2], sig[[step + 1] * 2])
        lat = lat.to(torch.bfloat16).float()      # the requests keep their latents in the model dtype between steps
    got = torch.cat([r.latents for r in reqs])
    assert all(r.step_index == 2 for r in reqs)
    # two chained forwards + CFG (guidance 5 amplifies the uncond/cond difference): twice the single-forward bound
    _check(got, lat, "denoising_step x2", max_rel=0.06, l2_rel=0.04)


def test_unet_full_width_sdxl(full_width_sdxl):
    """The real SDXL-base widths (320/640/1280, 70 transformer layers, 2.57 B params) on a 256x256-pixel latent, batch 2:
    exercises the BN=64 tile (N=320), channels-per-group 10/20/30/40/60/80, K=2880..23040 and the 10/20-head attention."""
    ocfg, P, _held, net = full_width_sdxl
    s, t, e, te, ti = ref.make_inputs(ocfg, 2, 32)
    with torch.inference_mode():
        want = ref.unet_forward(P, ocfg, s, t, e, te, ti)
    got = net.forward_one(s.cuda().to(torch.bfloat16), t.cuda(), e.cuda(), te.cuda(), ti.cuda())
    _check(got, want, "unet full width 32x32", max_rel=0.05, l2_rel=0.03)


def test_unet_full_width_sdxl_batch8(full_width_sdxl):
    """the same widths at UNet batch 8 (M = 8192 tokens at the 640-wide level, 2048 at the 1280-wide one): both LayerNorm routes of the
    step plan in one forward -- a normalisation pass in front of the 256 x 256 kernel where the batch makes it the tile of choice, row
    statistics from the producing GEMM's epilogue elsewhere -- against the oracle on the weights as the device holds them"""
    ocfg, P, held, net = full_width_sdxl
    s, t, e, te, ti = ref.make_inputs(ocfg, 8, 32)
    s = s + 0.3 * torch.randn(s.shape, generator=torch.Generator().manual_seed(8))      # eight different samples
    rows = [0, 3, 7]                            # samples are independent: the oracle answers three of the eight rows (the fp32 forward costs seconds per row)
    with torch.inference_mode():
        want = ref.unet_forward(held, ocfg, s[rows], t[rows], e[rows], te[rows], ti[rows])
        want_orig = ref.unet_forward(P, ocfg, s[rows], t[rows], e[rows], te[rows], ti[rows])
    got = net.forward_one(s.cuda().to(torch.bfloat16), t.cuda(), e.cuda(), te.cuda(), ti.cuda())
    assert (got[1].float() - got[0].float()).abs().max() > 0.05 * got[0].float().abs().max()       # the rows differ: a row mix-up cannot pass
    _calibrated_all_rows(got, held, ocfg, (s, t, e, te, ti), "unet full width 32x32 batch 8")
    got = got[rows]
    _check(got, want, "unet full width 32x32 batch 8", max_rel=0.05, l2_rel=0.03)
    # ... and against the ORIGINAL weights: real checkpoints have gamma != 1, so the fold's one extra weight rounding (bf16(W * gamma)) belongs
    # inside the stated end-to-end tolerance too (1.9 % -> 2.4 % rel L2 on the full forward)
    _check(got, want_orig, "unet full width 32x32 batch 8, original weights", max_rel=0.06, l2_rel=0.035)


def test_unet_full_width_sdxl_finalised_statistics(full_width_sdxl):
    """the same widths at UNet batch 32 on a 64 x 64 latent (M = 32768 tokens at the 640-wide level, 8192 at the 1280-wide one: the token counts of the
    benchmark's step): the smallest batch at which the step plan takes the FINALISED row statistics -- norm3 at both widths and norm1 at the 1280-wide
    level reach their consumers on the 256 x 256 kernel as (mean, rstd) per row from the producing launch (tests/test_ln_routes_cpu.py pins the routes
    of these token counts), which no other forward of the suite does"""
    ocfg, _P, held, net = full_width_sdxl
    inputs = ref.make_inputs(ocfg, 32, 64)
    s = inputs[0] + 0.3 * torch.randn(inputs[0].shape, generator=torch.Generator().manual_seed(32))      # thirty-two different samples
    inputs = (s,) + tuple(inputs[1:])
    got = net.forward_one(s.cuda().to(torch.bfloat16), *(x.cuda() for x in inputs[1:]))
    assert (got[1].float() - got[0].float()).abs().max() > 0.05 * got[0].float().abs().max()       # the rows differ: a row mix-up cannot pass
    # samples are independent: the oracle answers the first, the middle and the last of the 32 rows (its two evaluations of all 32 take 120 s on the
    # GPU; over all 32 the ratio to the stock bf16 figure came out at 0.33 .. 0.90)
    rows = [0, 15, 31]
    _calibrated_all_rows(got[rows], held, ocfg, tuple(x[rows] for x in inputs), "unet full width 64x64 batch 32, rows 0 / 15 / 31")


def _calibrated_all_rows(got, P, ocfg, inputs, what, ratio=1.5):
    """Round 5 (advisor: "the oracle now checks only the first and last rows"; verdict: calibrate the tolerances): EVERY row against the fp32 oracle evaluated on
    the GPU (the oracle's code by stock torch ops: seconds; agrees with the CPU oracle to 1e-5, tests/test_headline_shapes_gpu.py), and the bound is relative to
    what a stock bf16 evaluation of the same graph loses on the same inputs: rel L2 per row <= ratio x the stock bf16 figure of that row.
    P = the weights AS THE DEVICE HOLDS THEM (weights.params_as_held: the folded linears carry bf16(W * gamma), rounded once), handed to the oracle and to the stock
    evaluation alike: the synthetic parameters are bf16-exact, so on the ORIGINAL ones the stock path would multiply by rounding-free weights -- an advantage no real
    checkpoint gives it -- while the HIP path's one rounding of W * gamma acts as a coherent perturbation that the final conv_out amplifies (measured on this batch,
    tools/exp/stage_calibration.py: per stage the HIP path is 0.6-0.9 x the stock error up to the last resnet, and 0.36-1.01 x at the output on equal weights)."""
    s, t, e, te, ti = inputs
    with torch.inference_mode():
        o32 = ref.unet_forward(P, ocfg, s, t, e, te, ti, device="cuda").cpu()
        b16 = ref.unet_forward(P, ocfg, s, t, e, te, ti, compute_dtype=torch.bfloat16, device="cuda", sdpa=True).float().cpu()
    g = got.float().cpu()
    for r in range(s.shape[0]):
        l2 = ((g[r] - o32[r]).norm() / o32[r].norm()).item()
        sl2 = ((b16[r] - o32[r]).norm() / o32[r].norm()).item()
        print(f"{what} row {r}: HIP rel L2 {l2:.4f}, stock bf16 {sl2:.4f}, ratio {l2 / sl2:.2f}")
        assert l2 <= ratio * sl2, f"{what} row {r}: HIP rel L2 {l2:.4f} > {ratio} x stock bf16 {sl2:.4f}"


@pytest.mark.parametrize("batch,hw", [(3, 24), (5, 40), (1, 48)])
def test_unet_full_width_sdxl_ragged(full_width_sdxl, batch, hw):
    """the real widths on token counts that are not multiples of the GEMM tiles (batch 3 x 24 x 24 latents: M = 1728 / 432 tokens; 5 x 40 x 40:
    8000 / 2000; 1 x 48 x 48: 2304 / 576): the last row tile of every GEMM is partial, so the producers' row statistics and the consumers'
    folded LayerNorm run on tiles that end inside a tile; odd image sizes for the convs and the GroupNorm tiles"""
    ocfg, P, held, net = full_width_sdxl
    s, t, e, te, ti = ref.make_inputs(ocfg, batch, hw)
    rows = sorted({0, batch - 1})               # the oracle answers the first and the last row (independent samples)
    with torch.inference_mode():
        want = ref.unet_forward(held, ocfg, s[rows], t[rows], e[rows], te[rows], ti[rows])
        want_orig = ref.unet_forward(P, ocfg, s[rows], t[rows], e[rows], te[rows], ti[rows])
    got_all = net.forward_one(s.cuda().to(torch.bfloat16), t.cuda(), e.cuda(), te.cuda(), ti.cuda())
    _calibrated_all_rows(got_all, held, ocfg, (s, t, e, te, ti), f"unet full width {hw}x{hw} batch {batch}")
    got = got_all[rows]
    _check(got, want, f"unet full width {hw}x{hw} batch {batch}", max_rel=0.05, l2_rel=0.03)
    # (round 4: 3.4 % -> 3.53 % at 48 x 48 batch 1 when the small convs of this shape moved to split-K -- another summation order; bound 4 %)
    _check(got, want_orig, f"unet full width {hw}x{hw} batch {batch}, original weights", max_rel=0.06, l2_rel=0.04)


def test_unet_graph_replay_follows_buffer_contents(tiny):
    """The forward is captured into a hipGraph keyed by its argument pointers (graph_cache.h) and replayed: a replay must read
    the CURRENT contents of the caller's buffers, and equal inputs must give bit-identical outputs on capture and replay."""
    ocfg, P, net = tiny
    s1, t, e, te, ti = ref.make_inputs(ocfg, 2, 32, seed=5)
    s2 = ref.make_inputs(ocfg, 2, 32, seed=6)[0]
    sg, tg, eg, teg, tig = s1.cuda().to(torch.bfloat16), t.cuda(), e.cuda(), te.cuda(), ti.cuda()
    outs = []
    for k in range(4):                      # same tensors (same pointers) every call: capture, then replays
        if k == 2:
            sg.copy_(s2.to(torch.bfloat16))   # new contents, same address
        outs.append(net.forward_one(sg, tg, eg, teg, tig).float().cpu())
    assert torch.equal(outs[0], outs[1]), "replay differs from the captured run"
    assert torch.equal(outs[2], outs[3])
    assert not torch.equal(outs[1], outs[2]), "replay ignored the new buffer contents"
    _check(outs[2], ref.unet_forward(P, ocfg, s2.to(torch.bfloat16).float(), t, e, te, ti), "graph replay with new contents")


def test_graph_replay_path_in_subprocess(cuda_device):
    """MX_GRAPH is read once per process, so the opt-in hipGraph replay path (graph_cache.h) is exercised in a child process:
    same tensors four times (capture + three replays, new contents before the third call) must behave like the eager path."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys, torch
sys.path.insert(0, %r)
from oracle import sdxl_unet_ref as ref
from sduss_amd.config import UNetConfig
from sduss_amd.unet import MxUNet
ocfg = ref.UNetConfig.tiny(); P = ref.init_params(ocfg)
net = MxUNet(UNetConfig.tiny(), P, device="cuda:0")
s1, t, e, te, ti = ref.make_inputs(ocfg, 2, 32, seed=5); s2 = ref.make_inputs(ocfg, 2, 32, seed=6)[0]
sg, tg, eg, teg, tig = s1.cuda().to(torch.bfloat16), t.cuda(), e.cuda(), te.cuda(), ti.cuda()
outs = []
for k in range(4):
    if k == 2: sg.copy_(s2.to(torch.bfloat16))
    outs.append(net.forward_one(sg, tg, eg, teg, tig).float().cpu())
want = ref.unet_forward(P, ocfg, s2.to(torch.bfloat16).float(), t, e, te, ti)
err = (outs[3] - want).abs().max().item() / want.abs().max().item()
assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]) and not torch.equal(outs[1], outs[2]), "replay mismatch"
assert err < 0.04, err
del net
print("GRAPH_OK", err)
''' % root
    env = dict(os.environ, MX_GRAPH="1", MX_GRAPH_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "replays 3 captures 1" in r.stderr, "the graph path did not replay: " + r.stderr[-500:]


def test_denoising_step_mixed_resolutions_concurrent_equals_serial(tiny):
    """resolutions of a mixed batch run on separate streams (pipeline.py): the result must be bit-identical to running them one
    after the other, over several steps (latents produced on one stream are consumed on another at the next step)."""
    from sduss_amd.config import UNetConfig
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    ocfg, P, net = tiny
    cfg = UNetConfig.tiny()
    outs = []
    net.mixed_one_sequence = False              # this test is about the per-resolution sequences on side streams (the single mixed sequence:
    for concurrent in (False, True):            # tests/test_grouped_gpu.py)
        den = SDXLDenoiser(net, guidance_scale=5.0)
        den.concurrent_resolutions = concurrent
        reqs = {"128": [synthetic_request(0, 128, 6, cfg, den, "cuda:0")],
                "256": [synthetic_request(1, 256, 6, cfg, den, "cuda:0"), synthetic_request(2, 256, 6, cfg, den, "cuda:0")],
                "384": [synthetic_request(3, 384, 6, cfg, den, "cuda:0")]}
        for step in range(4):
            if step == 2:                       # change the set of resolutions -> streams are re-assigned
                reqs = {k: v for k, v in reqs.items() if k != "128"}
            den.denoising_step(reqs, is_sliced=True, patch_size=128)
        torch.cuda.synchronize()
        outs.append({k: torch.cat([r.latents for r in v]).float().cpu() for k, v in reqs.items()})
    net.mixed_one_sequence = True
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), f"concurrent != serial at {k}"


def test_plumbing_config0_four_steps_512(tiny):
    """BASELINE configs[0] (the reference's CPU-runnable plumbing case): one prompt, 4 denoising steps at 512 x 512 (latent
    64 x 64, UNet batch 2 under CFG) -- the whole loop (scale -> UNet -> CFG combine -> Euler) against the oracle chain, tiny
    SDXL-topology weights.  Four chained forwards with guidance 5: max error <= 10 % of range, relative L2 <= 6 %."""
    from oracle import scheduler_ref
    from sduss_amd.config import UNetConfig
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    ocfg, P, net = tiny
    cfg = UNetConfig.tiny()
    den = SDXLDenoiser(net, guidance_scale=5.0)
    req = synthetic_request(0, 512, 4, cfg, den, "cuda:0", dtype=torch.bfloat16)
    lat = req.latents.float().cpu()
    pe, ne = req.prompt_embeds.float().cpu(), req.negative_prompt_embeds.float().cpu()
    pp, npp = req.pooled_prompt_embeds.float().cpu(), req.negative_pooled_prompt_embeds.float().cpu()
    tid = req.add_time_ids.float().cpu()
    ts, sig, _ = scheduler_ref.sdxl_euler_tables(4)
    for step in range(4):
        den.denoising_step({"512": [req]})
        x2 = scheduler_ref.scale_model_input(torch.cat([lat, lat]), sig[[step] * 2])
        noise = ref.unet_forward(P, ocfg, x2, ts[[step] * 2], torch.cat([ne, pe]), torch.cat([npp, pp]), tid.repeat(2, 1))
        lat = scheduler_ref.euler_step(scheduler_ref.cfg_combine(noise, 5.0), lat, sig[[step]], sig[[step + 1]])
        lat = lat.to(torch.bfloat16).float()
    assert req.done()
    _check(req.latents, lat, "config0 plumbing: 4 steps at 512x512", max_rel=0.10, l2_rel=0.06)


def test_unet_per_stage_error_budget(tiny):
    """The end-to-end bound of the tests above, broken down: every block output of the step plan (mx_unet_forward_trace) against the
    same stage of the fp32 oracle.  Budget: each fused stage stores its result in bf16 (relative rounding 2^-9 per element, ~0.2 % rms)
    and reads inputs that already carry the error of the stages before, so the relative L2 error after n stages is allowed
    0.35 % * sqrt(n) (independent roundings add in quadrature; GroupNorm / LayerNorm keep the scale at 1 so the error neither dies out
    nor compounds) and no single stage may add more than 1 % on top of its input's error.  A kernel that is wrong in one stage shows as a
    jump at that stage instead of hiding in a 4 % end-to-end bound."""
    ocfg, P, net = tiny
    s, t, e, te, ti = ref.make_inputs(ocfg, 2, 32)
    tr = {}
    ref.unet_forward(P, ocfg, s, t, e, te, ti, trace=tr)
    x = s.cuda().to(torch.bfloat16)
    prev = 0.0
    rows = []
    for k, (name, want) in enumerate(tr.items()):
        if want.ndim != 4:
            continue
        b, c, h, w = want.shape
        got = net.forward_one(x, t.cuda(), e.cuda(), te.cuda(), ti.cuda(), stage=name, stage_shape=(b, h, w, c))
        got = got.float().cpu().permute(0, 3, 1, 2)
        l2 = ((got - want).norm() / want.norm()).item()
        rows.append((name, l2))
        budget = 0.0035 * (len(rows) ** 0.5) + 0.002
        assert l2 <= budget, f"stage {name} (#{len(rows)}): rel L2 {l2:.4f} > budget {budget:.4f}; previous stage {prev:.4f}"
        assert l2 <= prev + 0.01, f"stage {name} adds {l2 - prev:.4f} to the relative error in one step"
        prev = l2
    print("per-stage rel L2:", ", ".join(f"{n.split('.')[-3] if n.count('.') > 2 else n}={v:.4f}" for n, v in rows[:6]), "...", f"{rows[-1][0]}={rows[-1][1]:.4f}")
    assert len(rows) >= 20


def test_unet_context_key_store_is_bit_identical(tiny):
    """mx_unet_set_context_key: a forward announced with a composition key reads the cross-attention K / V^T its first forward stored -- the same
    bits as projecting them again; a new key (new embeddings) projects anew; an unannounced forward never reads the store; two streams may share an entry."""
    ocfg, P, net = tiny
    s, t, e, te, ti = ref.make_inputs(ocfg, 2, 32, seed=5)
    _s2, _t2, e2, _te2, _ti2 = ref.make_inputs(ocfg, 2, 32, seed=6)
    sc, tc, tec, tic = s.cuda().to(torch.bfloat16), t.cuda(), te.cuda(), ti.cuda()
    ec, e2c = e.cuda().to(torch.bfloat16), e2.cuda().to(torch.bfloat16)

    def fwd(ehs, key=0, sample=sc):
        net.set_context_key(key)
        return net.forward({"256": sample}, tc, ehs, added_cond_kwargs={"text_embeds": tec, "time_ids": tic}, return_dict=False,
                           is_sliced=False, patch_size=256, input_indices={"256": ["0", "1"]})[0]["256"].clone()
    h0, m0 = net.context_stats()
    plain, plain2 = fwd(ec), fwd(e2c)
    assert net.context_stats() == (h0, m0), "an unannounced forward must not touch the store"
    assert not torch.equal(plain, plain2)
    first = fwd(ec, key=1001)            # miss: projects into the store
    # the hit must not read encoder_hidden_states at all: hand it garbage under the SAME key (the caller's promise is what the key means)
    again = fwd(torch.full_like(ec, float("nan")), key=1001)
    assert net.context_stats() == (h0 + 1, m0 + 1)
    assert torch.equal(first, plain) and torch.equal(again, plain)
    other = fwd(e2c, key=1002)           # a new composition
    assert torch.equal(other, plain2)
    assert torch.equal(fwd(ec, key=1001), plain), "the first composition is still stored (4 entries)"
    # a different sample under a stored key: only the conditioning is reused
    s3 = (sc.float() * 0.5).to(torch.bfloat16)
    assert torch.equal(fwd(ec, key=1001, sample=s3), fwd(ec, sample=s3))
    # another stream reads the entry the first one wrote
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = fwd(ec, key=1001)
    side.synchronize()
    assert torch.equal(on_side, plain)
    # more compositions than entries: the least recently used one is projected again, results unchanged
    for k in range(2001, 2006):
        assert torch.equal(fwd(e2c, key=k), plain2)
    assert torch.equal(fwd(ec, key=1001), plain)
