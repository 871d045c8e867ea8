"""The multistep samplers on the GPU (csrc/scheduler_step.hip): the step launch on its own, then Denoiser.denoising_step over requests of different
samplers -- with a stub in the model slot, so that every step can be replayed on the CPU, and with the tiny models of tests/test_inpaint_gpu.py.

Every comparison of a step is on the raw bits: a multistep row is a chain of separately rounded fp32 operations that torch evaluates identically on
the CPU (tests/sampler_ref.py), rounded once to the io dtype; an Euler row must be what mx_cfg_euler_step / mx_cfg_flow_step leave.  The
coefficients of the loop tests are the library's own (mx_sampler_coeffs, held to the fp64 rules within 1 ulp by tests/test_sampler_cpu.py)."""
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import inpaint_ref as I
import sampler_ref as S
import vae_encode_ref as E
from step_operands import DTYPES, K, SLOTS, STEP_SHAPES, guards_intact, placed, same_bits

pytestmark = pytest.mark.gpu

from oracle import vae_ref  # noqa: E402  (checker only)

KINDS = {3: [2, 0, 1], 2: [1, 2]}                                             # permuted: row != kind


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = I.bits(got) != I.bits(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {got.numel()} differ (first at {bad.nonzero()[0].tolist()})"


def step_operands(shape, dtype, flow, g):
    n, C, h, w = shape
    gen = torch.Generator().manual_seed(2000 * C + 10 * h + int(flow))
    pred = torch.randn((2 if g > 0 else 1) * n, C, h, w, generator=gen).to(dtype)
    lat = (torch.randn(n, C, h, w, generator=gen) * (1.0 if flow else 3.0)).to(dtype)
    hist = torch.randn(n, C, h, w, generator=gen) * 2.0
    sigma = torch.tensor([1.0, 0.7368, 0.3][:n] if flow else [14.6146, 3.1875, 0.9][:n])
    sigma_next = torch.tensor([0.9231, 0.5, 0.0][:n] if flow else [9.8123, 2.0625, 0.0][:n])
    init = torch.randn(K, C, h, w, generator=gen).to(dtype)
    noise = torch.randn(K, C, h, w, generator=gen).to(dtype)
    mask = torch.randint(0, 2, (K, h, w), generator=gen, dtype=torch.uint8) * torch.randint(1, 256, (K, h, w), generator=gen, dtype=torch.uint8)
    mask[0, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)
    return pred, lat, hist, sigma, sigma_next, init, noise, mask


def coefs(n, second):
    """fp32 [n, 3] of plausible magnitudes (a DPM-Solver++ row, an AB2 row, ...); ``second``: per row, whether c1 != 0"""
    rows = [(0.6713867, 0.5432129, -0.2145996), (1.0, -0.1977539, 0.0834961), (0.25, 1.125, -0.375)][:n]
    return torch.tensor([(cx, c0, c1 if s else 0.0) for (cx, c0, c1), s in zip(rows, second)], dtype=torch.float32)


def run_multistep(flow, pred, lat, hist, sigma, sigma_next, g, offset, kind, coef, slot=None, init=None, noise=None, mask=None):
    """one launch on fresh copies -> (latents, hist) it leaves, on the CPU (guards of both checked, the prediction unchanged)"""
    from sduss_amd import ops
    pbuf, pv = placed(pred, offset)
    lbuf, lv = placed(lat, offset)
    hbuf, hv = placed(hist, offset)
    rows, keepalive = [], []
    if init is not None:
        sbuf, sv = placed(torch.tensor(slot, dtype=torch.int32), 0)
        ibuf, iv = placed(init, offset)
        nbuf, nv = placed(noise, offset)
        mbuf, mv = placed(mask, offset)
        rows, keepalive = [sv, iv, nv, mv], [sbuf, ibuf, nbuf, mbuf]
    assert (lv.data_ptr() % 16 == 0) == (offset == 0) and (hv.data_ptr() % 16 == 0) == (offset == 0)
    got = ops.cfg_multistep_step_(pv, lv, sigma.cuda(), sigma_next.cuda(), g, torch.tensor(kind, dtype=torch.int32).cuda(), coef.cuda(), hv, flow, *rows)
    torch.cuda.synchronize()
    assert got.data_ptr() == lv.data_ptr() and guards_intact(lbuf, lv) and guards_intact(hbuf, hv) and torch.equal(pv.cpu(), pred)
    return lv.cpu(), hv.cpu()


def plain_step(flow, pred, lat, sigma, sigma_next, g):
    from sduss_amd import ops
    out = lat.cuda().clone()
    (ops.cfg_flow_step_ if flow else ops.cfg_euler_step_)(pred.cuda(), out, sigma.cuda(), sigma_next.cuda(), g)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("g", [5.0, 0.0], ids=["g5", "g0"])
@pytest.mark.parametrize("shape,offset", STEP_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flow", [False, True], ids=["euler", "flow"])
def test_multistep_step(cuda_device, flow, dtype, shape, offset, g):
    pred, lat, hist, sigma, sigma_next, _init, _noise, _mask = step_operands(shape, dtype, flow, g)
    n = shape[0]
    plain = plain_step(flow, pred, lat, sigma, sigma_next, g)
    # rows of kinds 0, 1, 2 permuted, first-order and second-order rows mixed, then the orders swapped
    for second in ([True, False, False][:n], [False, True, True][:n], [True] * n):
        kind, coef = KINDS[n], coefs(n, second)
        got, got_hist = run_multistep(flow, pred, lat, hist, sigma, sigma_next, g, offset, kind, coef)
        want, want_hist = S.multistep_step(pred, lat, sigma, sigma_next, g, kind, coef, hist, flow)
        assert_bits(got, want, f"latents, second order {second}")
        assert_bits(got_hist, want_hist, f"hist, second order {second}")
        for r, k in enumerate(kind):
            if k == 0:                                                    # an Euler row beside multistep rows: the plain step's bits, its history untouched
                assert same_bits(got[r], plain[r]) and same_bits(got_hist[r], hist[r])
            else:
                assert not same_bits(got[r], plain[r]) and not same_bits(got_hist[r], hist[r])
    # kind 0 and every unknown kind: the plain step, bit for bit, and no history written
    for kind in ([0] * n, [7, -1, 3][:n], [2 ** 31 - 1, -2 ** 31, 0][:n]):
        got, got_hist = run_multistep(flow, pred, lat, hist, sigma, sigma_next, g, offset, kind, coefs(n, [True] * n))
        assert_bits(got, plain, f"kinds {kind}")
        assert_bits(got_hist, hist, f"hist under kinds {kind}")


@pytest.mark.parametrize("shape,offset", STEP_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_order_rows_never_read_the_history(cuda_device, dtype, shape, offset):
    """on a request's first step the history is uninitialised memory: all NaN here, and nothing of it reaches the latents or the new history"""
    pred, lat, hist, sigma, sigma_next, *_ = step_operands(shape, dtype, False, 5.0)
    n = shape[0]
    nan_hist = torch.full_like(hist, float("nan"))
    kind = [1, 2, 1][:n]
    got, got_hist = run_multistep(False, pred, lat, nan_hist, sigma, sigma_next, 5.0, offset, kind, coefs(n, [False] * n))
    assert bool(torch.isfinite(got.float()).all()) and bool(torch.isfinite(got_hist).all())
    want, want_hist = S.multistep_step(pred, lat, sigma, sigma_next, 5.0, kind, coefs(n, [False] * n), hist, False)
    assert_bits(got, want, "latents")
    assert_bits(got_hist, want_hist, "hist")


@pytest.mark.parametrize("shape,offset", STEP_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flow", [False, True], ids=["euler", "flow"])
def test_multistep_step_with_inpainting_rows(cuda_device, flow, dtype, shape, offset):
    pred, lat, hist, sigma, sigma_next, init, noise, mask = step_operands(shape, dtype, flow, 5.0)
    n = shape[0]
    kind, slot, coef = KINDS[n], SLOTS[n], coefs(n, [True, True, False][:n])
    free, free_hist = run_multistep(flow, pred, lat, hist, sigma, sigma_next, 5.0, offset, kind, coef)
    got, got_hist = run_multistep(flow, pred, lat, hist, sigma, sigma_next, 5.0, offset, kind, coef, slot, init, noise, mask)
    want, want_hist = S.multistep_step(pred, lat, sigma, sigma_next, 5.0, kind, coef, hist, flow, slot, init, noise, mask)
    assert_bits(got, want, "latents")
    assert_bits(got_hist, want_hist, "hist")
    assert_bits(got_hist, free_hist, "hist: the unmasked D")              # diffusers does not mask its model_outputs either
    keep = I.step_keep(flow, sigma_next)
    for r, j in enumerate(slot):                                          # stated once more without the helper
        if j < 0:
            assert same_bits(got[r], free[r])
            continue
        kept = (mask[j] == 0)[None].expand_as(got[r])
        assert 0 < int(kept.sum()) < kept.numel()
        renoised = I.renoise(init[j:j + 1], noise[j:j + 1], keep[r], sigma_next[r])[0]
        assert torch.equal(I.bits(got[r])[kept], I.bits(renoised)[kept]) and torch.equal(I.bits(got[r])[~kept], I.bits(free[r])[~kept])
    # no inpainting row (every slot -1, k = 0 rows): the launch without them
    none, none_hist = run_multistep(flow, pred, lat, hist, sigma, sigma_next, 5.0, offset, kind, coef, [-1] * n, init, noise, mask)
    assert same_bits(none, free) and same_bits(none_hist, free_hist)


@pytest.mark.parametrize("dtype", DTYPES)
def test_last_step_returns_the_data_prediction(cuda_device, dtype):
    """sigma_next = 0 with (cx, c0, c1) = (0, 1, 0): the latents are D = x - sigma m, rounded once to the io dtype"""
    shape = (3, 16, 16, 16)
    pred, lat, hist, sigma, _sn, *_ = step_operands(shape, dtype, False, 5.0)
    coef = torch.tensor([[0.0, 1.0, 0.0]] * 3)
    got, got_hist = run_multistep(False, pred, lat, hist, sigma, torch.zeros(3), 5.0, 0, [1, 1, 1], coef)
    D = lat.float() - sigma.reshape(3, 1, 1, 1) * S.guided(pred, 3, 5.0)
    assert_bits(got_hist, D, "hist")
    assert torch.equal(got.float(), D.to(dtype).float())                  # by value: 0 * x + 1 * D may give a zero of D the other sign


# ---- the denoising loop ----

LAT = 16                     # a "128" request of the tiny models: 16 x 16 latents
RES = "128"


class Counter:
    """the stub predictions of a run: a fixed seeded tensor per call, kept on the CPU for the replay"""
    def __init__(self, seed):
        self.seed, self.preds = seed, []

    def next(self, shape, dtype):
        p = torch.randn(shape, generator=torch.Generator().manual_seed(self.seed + len(self.preds))).to(dtype)
        self.preds.append(p)
        return p


def stub_denoiser(base, counter, guidance_scale=5.0):
    """a Denoiser of the model's kind whose model slot returns ``counter``'s tensors"""
    class Stub(base):
        def _forward(self, x, ts, cond, **kwargs):
            return {res: counter.next(tuple(t.shape), t.dtype).to(t.device) for res, t in x.items()}
    return Stub(SimpleNamespace(device=torch.device("cuda:0"), set_context_key=lambda uid: None), guidance_scale)


@pytest.fixture(scope="module")
def sdxl(cuda_device):
    from oracle import sdxl_unet_ref
    from sduss_amd.config import UNetConfig
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    from sduss_amd.unet import MxUNet
    from sduss_amd.vae import MxVAEDecoder, MxVAEEncoder, VAEConfig
    enc = MxVAEEncoder(VAEConfig.tiny(), E.init_params(vae_ref.VAEConfig.tiny()), device="cuda:0")
    dec = MxVAEDecoder(VAEConfig.tiny(), vae_ref.init_params(vae_ref.VAEConfig.tiny()), device="cuda:0")

    def net():
        return MxUNet(UNetConfig.tiny(), sdxl_unet_ref.init_params(sdxl_unet_ref.UNetConfig.tiny()), device="cuda:0")

    def make_req(den, i, steps, sampler="euler", schedule="default", dtype=torch.bfloat16):
        return synthetic_request(i, 128, steps, UNetConfig.tiny(), den, "cuda:0", dtype=dtype, sampler=sampler, schedule=schedule)
    return SimpleNamespace(name="sdxl", base=SDXLDenoiser, flow=False, g=5.0, make_req=make_req, enc=enc, dec=dec, net=net,
                           second=("dpmpp_2m", "karras"), third=("ab2", "default"))


@pytest.fixture(scope="module")
def sd3(cuda_device):
    from oracle import sd3_mmdit_ref
    from sduss_amd.config import MMDiTConfig
    from sduss_amd.pipeline_sd3 import SD3Denoiser, synthetic_sd3_request
    from sduss_amd.transformer_sd3 import MxSD3Transformer
    from sduss_amd.vae import MxVAEDecoder, MxVAEEncoder, VAEConfig
    cfg = replace(VAEConfig.sd3(), block_out_channels=(64, 64, 128), layers_per_block=1)
    enc = MxVAEEncoder(cfg, E.init_params(vae_ref.VAEConfig.tiny_sd3()), device="cuda:0")
    dec = MxVAEDecoder(cfg, vae_ref.init_params(vae_ref.VAEConfig.tiny_sd3()), device="cuda:0")

    def net():
        return MxSD3Transformer(MMDiTConfig.tiny(), sd3_mmdit_ref.init_params(sd3_mmdit_ref.MMDiTConfig.tiny()), device="cuda:0")

    def make_req(den, i, steps, sampler="euler", schedule="default", dtype=torch.bfloat16):
        return synthetic_sd3_request(i, 128, steps, MMDiTConfig.tiny(), den, "cuda:0", dtype=dtype, ctx_len=21, sampler=sampler, schedule=schedule)
    return SimpleNamespace(name="sd3", base=SD3Denoiser, flow=True, g=7.0, make_req=make_req, enc=enc, dec=dec, net=net,
                           second=("ab2", "default"), third=("ab2", "default"))


@pytest.fixture(params=["sdxl", "sd3"])
def model(request):
    return request.getfixturevalue(request.param)


def client_image(seed):
    return torch.randint(0, 256, (1, 4 * LAT, 4 * LAT, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).cuda()


def fixed_noise(enc, seed=9):
    return torch.randn(1, enc.cfg.latent_channels, LAT, LAT, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).cuda()


def half_mask():
    m = torch.full((1, 4 * LAT, 4 * LAT), 127, dtype=torch.uint8)
    m[:, :, :2 * LAT] = 128
    return m.cuda()


class Replay:
    """the CPU's copy of one request: its latents, its history and the step that left it, stepped by tests/sampler_ref.py"""
    def __init__(self, req, flow):
        from sduss_amd import ops
        self.req, self.flow = req, flow
        self.lat = req.latents.cpu().clone()
        self.step = req.step_index
        self.kind = S.KIND[req.sampler]
        self.tab = ops.sampler_coeffs(req.sampler, req.sigmas, flow) if self.kind else None
        self.hist, self.hist_step = None, -1
        s = req.inpaint
        self.inpaint = None if s is None else (s.init.cpu(), s.noise.cpu(), s.mask.cpu())

    def second(self):
        return self.kind != 0 and self.hist is not None and self.hist_step == self.step - 1


def replay_step(rows, pred, g, flow):
    """one scheduler step of the batch ``rows`` (Replay objects in batch order) from the model's output ``pred``"""
    n = len(rows)
    sig = torch.tensor([float(r.req.sigmas[r.step]) for r in rows])
    sig_next = torch.tensor([float(r.req.sigmas[r.step + 1]) for r in rows])
    coef = torch.zeros(n, 3)
    for i, r in enumerate(rows):
        if r.kind:
            coef[i] = torch.tensor([float(c) for c in S.step_coef(r.tab, r.step, r.second())])
    hist = torch.cat([r.hist if r.second() else torch.full_like(r.lat, float("nan"), dtype=torch.float32) for r in rows])
    inp = [r for r in rows if r.inpaint is not None]
    extra = ()
    if inp:
        order = iter(range(len(inp)))
        extra = ([next(order) if r.inpaint is not None else -1 for r in rows], *(torch.cat([r.inpaint[k] for r in inp]) for k in range(3)))
    lat, new_hist = S.multistep_step(pred, torch.cat([r.lat for r in rows]), sig, sig_next, g, [r.kind for r in rows], coef, hist, flow, *extra)
    for i, r in enumerate(rows):
        r.lat = lat[i:i + 1]
        if r.kind:
            r.hist, r.hist_step = new_hist[i:i + 1], r.step
        r.step += 1


def run_and_replay(den, counter, reqs, flow, g, max_steps=None):
    """steps ``reqs`` to the end (or ``max_steps`` steps) on the device and on the CPU, comparing every request's latents after every step"""
    rows = {id(r): Replay(r, flow) for r in reqs}
    done = 0
    while not all(r.done() for r in reqs) and (max_steps is None or done < max_steps):
        active = [r for r in reqs if not r.done()]
        den.denoising_step({RES: active})
        torch.cuda.synchronize()
        replay_step([rows[id(r)] for r in active], counter.preds[-1], g, flow)
        for r in active:
            assert r.step_index == rows[id(r)].step
            assert_bits(r.latents.cpu(), rows[id(r)].lat, f"request {r.request_id} ({r.sampler}) after step {r.step_index - 1}")
        done += 1
    return rows


def three_requests(model, den, samplers):
    """an Euler request, an image-to-image request at strength 0.5 and an inpainting request with a half mask, of different lengths"""
    (s1, sch1), (s2, sch2) = samplers
    a = model.make_req(den, 0, 6)
    b = model.make_req(den, 1, 8, s1, sch1)
    c = model.make_req(den, 2, 7, s2, sch2)
    den.start_from_image(b, model.enc, client_image(31), 0.5, start_noise=fixed_noise(model.enc, 5))
    den.start_inpaint(c, model.enc, client_image(32), half_mask(), strength=1.0, noise=fixed_noise(model.enc, 6))
    assert (b.sampler, c.sampler) == (s1, s2) and b.step_index == 4 and c.step_index == 0 and b.history is None
    return [a, b, c]


def test_loop_equals_the_cpu_replay(model):
    """requests of three samplers in one resolution, one of them image-to-image and one inpainting, leaving the batch at different steps"""
    finals = {}
    for samplers in ((model.second, model.third), (("euler", "default"), ("euler", "default"))):
        counter = Counter(100)
        den = stub_denoiser(model.base, counter, model.g)
        reqs = three_requests(model, den, samplers)
        if samplers[0][0] != "euler":
            from sduss_amd.pipeline import karras_tables
            assert model.flow or np.array_equal(reqs[1].sigmas, karras_tables(8)[1])
        rows = run_and_replay(den, counter, reqs, model.flow, model.g)
        assert all(r.done() for r in reqs) and len(counter.preds) == 7            # one model call per step of the longest request
        for r in reqs:
            assert bool(torch.isfinite(r.latents.float()).all())
            if r.sampler != "euler":
                assert r.history is not None and r.history.dtype == torch.float32 and r.history_step == r.num_inference_steps - 1
                assert_bits(r.history.cpu(), rows[id(r)].hist, f"history of request {r.request_id}")
            else:
                assert r.history is None and r.history_step == -1
        kept = (reqs[2].inpaint.mask == 0)[:, None].expand_as(reqs[2].latents)
        assert torch.equal(I.bits(reqs[2].latents)[kept], I.bits(reqs[2].inpaint.init)[kept])      # sigma_next = 0: the image's own latents
        finals[samplers[0][0]] = [r.latents.clone() for r in reqs]
    multi, euler = finals[model.second[0]], finals["euler"]
    assert same_bits(multi[0], euler[0])                                  # the Euler request does not see its neighbours' samplers
    assert not same_bits(multi[1], euler[1]) and not same_bits(multi[2], euler[2])


def two_requests(model, den):
    return [model.make_req(den, 0, 7, *model.second), model.make_req(den, 1, 6, "ab2", "default")]


def test_history_travels_on_the_request(model):
    """a fresh Denoiser (no step cache, no history buffer) takes the requests over after 3 steps: the same final bits"""
    finals = []
    for hand_over in (False, True):
        counter = Counter(200)
        den = stub_denoiser(model.base, counter, model.g)
        reqs = two_requests(model, den)
        run_and_replay(den, counter, reqs, model.flow, model.g, max_steps=3)
        assert all(r.step_index == 3 and r.history_step == 2 for r in reqs)
        if hand_over:
            den = stub_denoiser(model.base, counter, model.g)
        while not all(r.done() for r in reqs):
            den.denoising_step({RES: [r for r in reqs if not r.done()]})
        torch.cuda.synchronize()
        finals.append([r.latents.clone() for r in reqs])
    assert all(same_bits(a, b) for a, b in zip(*finals))


def test_rewound_request_steps_first_order(model):
    """bench.py refills its batch by resetting step_index: the stale history must not enter the step"""
    counter = Counter(300)
    den = stub_denoiser(model.base, counter, model.g)
    reqs = two_requests(model, den)
    rows = run_and_replay(den, counter, reqs, model.flow, model.g, max_steps=3)
    a, b = reqs
    a.step_index = 0                                                      # a keeps history_step = 2; b goes on in second order
    before = a.latents.cpu().clone()
    den.denoising_step({RES: reqs})
    torch.cuda.synchronize()
    ra, rb = rows[id(a)], rows[id(b)]
    tab = ra.tab
    sig = torch.tensor([float(a.sigmas[0])])
    want, want_hist = S.multistep_step(torch.cat([counter.preds[-1][0:1], counter.preds[-1][2:3]]), before, sig, torch.tensor([float(a.sigmas[1])]), model.g,
                                       [ra.kind], torch.tensor([[float(c) for c in S.step_coef(tab, 0, False)]]),
                                       torch.full_like(before, float("nan"), dtype=torch.float32), model.flow)
    assert a.step_index == 1 and a.history_step == 0
    assert_bits(a.latents.cpu(), want, "the rewound request")
    assert_bits(a.history.cpu(), want_hist, "its history")
    ra.lat, ra.step, ra.hist, ra.hist_step = before, 0, None, -1          # and the neighbour is untouched by it: the replay of both rows
    replay_step([ra, rb], counter.preds[-1], model.g, model.flow)
    assert_bits(b.latents.cpu(), rb.lat, "the neighbour")
    assert_bits(a.latents.cpu(), ra.lat, "the rewound request, replayed")


def test_convergence_on_the_device(model):
    """the analytic denoiser of Gaussian data in the model slot (fp32 latents, no guidance): at 20 steps the multistep sampler ends closer to the
    ODE's exact solution than Euler at 40 steps on the same schedule"""
    schedule = "default" if model.flow else "karras"
    sampler = "ab2" if model.flow else "dpmpp_2m"

    class Analytic(model.base):
        def _gather(self, res, reqs, cfg):
            self.part = super()._gather(res, reqs, cfg)
            return self.part

        def _forward(self, x, ts, cond, **kwargs):
            lat, s = self.part.latents.double(), self.part.sigma.double().reshape(-1, 1, 1, 1)
            out = (lat * (s - (1 - s) * S.SD ** 2) / ((1 - s) ** 2 * S.SD ** 2 + s ** 2)) if model.flow else lat * s / (S.SD ** 2 + s ** 2)
            return {RES: out.float()}
    den = Analytic(SimpleNamespace(device=torch.device("cuda:0"), set_context_key=lambda uid: None), model.g)
    slow = model.make_req(den, 0, 40, "euler", schedule, dtype=torch.float32)
    fast = model.make_req(den, 1, 20, sampler, schedule, dtype=torch.float32)
    fast.latents = slow.latents.clone()
    x0 = slow.latents.cpu().double().numpy()
    # (the first sigma of a 20-step and of a 40-step schedule differ: each request's exact solution starts from x0 at its own)
    want = {r.sampler: S.exact_final(x0, r.sigmas[0], model.flow) for r in (slow, fast)}
    reqs = [slow, fast]
    while not all(r.done() for r in reqs):
        den.denoising_step({RES: [r for r in reqs if not r.done()]}, do_classifier_free_guidance=False)
    torch.cuda.synchronize()
    err = {r.sampler: S.rel_max_err(r.latents.cpu().double().numpy(), want[r.sampler]) for r in reqs}
    print(model.name, err)
    assert err[sampler] < err["euler"]
    # and each is where the fp64 loop of the restatement ends, to fp32 accuracy: at most 40 steps of at most 16 roundings of 2^-24 each, every
    # one relative to the sample, which the linear ODE carries to the end unchanged in relative size
    for r in reqs:
        ref = S.sample_loop(S.KIND[r.sampler], r.sigmas, S.v_model if model.flow else S.eps_model, x0, model.flow)
        assert S.rel_max_err(r.latents.cpu().double().numpy(), ref) <= 40 * 2.0 ** -20, r.sampler


def test_end_to_end_with_the_real_model(model):
    from sduss_amd.vae import post_inference
    sampler, schedule = model.second
    net = model.net()
    finals = {}
    for multi in (True, False):
        den = model.base(net, guidance_scale=model.g)
        a = model.make_req(den, 0, 6, *((sampler, schedule) if multi else ("euler", "default")))
        p = model.make_req(den, 1, 6)
        while not all(r.done() for r in (a, p)):
            den.denoising_step({RES: [a, p]})
        torch.cuda.synchronize()
        assert bool(torch.isfinite(a.latents.float()).all()) and bool(torch.isfinite(p.latents.float()).all())
        assert (a.history is not None) == multi and p.history is None
        out = post_inference(model.dec, {RES: [a, p]}, "uint8")[RES]
        torch.cuda.synchronize()
        assert out.shape == (2, 4 * LAT, 4 * LAT, 3) and out.dtype == torch.uint8
        finals[multi] = (a.latents.clone(), p.latents.clone())
    assert same_bits(finals[True][1], finals[False][1])                   # the Euler neighbour: the bits of the all-Euler run of the same composition
    assert not same_bits(finals[True][0], finals[False][0])
