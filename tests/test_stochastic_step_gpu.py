"""The stochastic samplers on the GPU (csrc/scheduler_step.hip NOISY, mx_cfg_stochastic_step): the fused launch against the unfused restatement
(tests/stochastic_ref.py) fed the noise ops.seeded_noise writes, bit for bit; then Denoiser.denoising_step over requests of four samplers in one
resolution -- with a stub in the model slot whose prediction for a request depends on that request alone, so that every step can be replayed on
the CPU and a request can be run again alone -- and the variance the SDE sampler ends with on the analytic Gaussian problem."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import inpaint_ref as I
import noise_ref as N
import sampler_ref as S
import stochastic_ref as R
import vae_encode_ref as E
from step_operands import DTYPES, K, SLOTS, STEP_SHAPES, guards_intact, placed, same_bits

pytestmark = pytest.mark.gpu

from oracle import vae_ref  # noqa: E402  (checker only)

SHAPES = STEP_SHAPES + [pytest.param((2, 3, 3, 3), 0, id="2x3x3x3-partial-group")]
KINDS = {3: [2, 0, 1], 2: [1, 2]}                         # the device kinds: a noisy AB2-form row, an Euler row, a noisy DPM-Solver++-form row
CN = [0.8359375, 0.5, 1.71875]                            # the Euler row's is not read
SEEDS = [0xDEADBEEF12345678, 2 ** 64 - 1, 3]
NSTEPS = [0, 5, 19]
NAN64, NAN32 = 0x7FF8000000000000, 0x7FC00000            # the bits of a NaN: poison for buffers that must not be read


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = I.bits(got) != I.bits(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {got.numel()} differ (first at {bad.nonzero()[0].tolist()})"


def step_operands(shape, dtype, g=5.0):
    n, C, h, w = shape
    gen = torch.Generator().manual_seed(3000 * C + 10 * h)
    pred = torch.randn((2 if g > 0 else 1) * n, C, h, w, generator=gen).to(dtype)
    lat = (torch.randn(n, C, h, w, generator=gen) * 3.0).to(dtype)
    hist = torch.randn(n, C, h, w, generator=gen) * 2.0
    sigma = torch.tensor([14.6146, 3.1875, 0.9][:n])
    sigma_next = torch.tensor([9.8123, 2.0625, 0.0][:n])
    init = torch.randn(K, C, h, w, generator=gen).to(dtype)
    noise = torch.randn(K, C, h, w, generator=gen).to(dtype)
    mask = torch.randint(0, 2, (K, h, w), generator=gen, dtype=torch.uint8) * torch.randint(1, 256, (K, h, w), generator=gen, dtype=torch.uint8)
    mask[0, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)
    return pred, lat, hist, sigma, sigma_next, init, noise, mask


def coefs(n, second):
    rows = [(1.0, -0.1977539, 0.0834961), (0.25, 1.125, -0.375), (0.6713867, 0.5432129, -0.2145996)][:n]
    return torch.tensor([(cx, c0, c1 if s else 0.0) for (cx, c0, c1), s in zip(rows, second)], dtype=torch.float32)


def run_step(pred, lat, hist, sigma, sigma_next, g, offset, kind, coef, cn=None, seeds=None, steps=None, inpaint=None):
    """one launch on fresh copies -> (latents, hist) it leaves, on the CPU; cn None: mx_cfg_multistep_step.  Guards checked, the prediction unchanged"""
    from sduss_amd import ops
    pbuf, pv = placed(pred, offset)
    lbuf, lv = placed(lat, offset)
    hbuf, hv = placed(hist, offset)
    rows, keepalive = [], []
    if inpaint is not None:
        slot, init, noise, mask = inpaint
        sbuf, sv = placed(torch.tensor(slot, dtype=torch.int32), 0)
        ibuf, iv = placed(init, offset)
        nbuf, nv = placed(noise, offset)
        mbuf, mv = placed(mask, offset)
        rows, keepalive = [sv, iv, nv, mv], [sbuf, ibuf, nbuf, mbuf]
    assert (lv.data_ptr() % 16 == 0) == (offset == 0)
    kd = torch.tensor(kind, dtype=torch.int32).cuda()
    if cn is None:
        got = ops.cfg_multistep_step_(pv, lv, sigma.cuda(), sigma_next.cuda(), g, kd, coef.cuda(), hv, False, *rows)
    else:
        n = lat.shape[0]
        sd, st = ops._seeds_and_steps("test", n, list(seeds[:n]), list(steps[:n]), "cuda")
        got = ops.cfg_stochastic_step_(pv, lv, sigma.cuda(), sigma_next.cuda(), g, kd, coef.cuda(), hv, False, torch.tensor(cn[:n], dtype=torch.float32).cuda(),
                                       sd, st, *rows)
    torch.cuda.synchronize()
    assert got.data_ptr() == lv.data_ptr() and guards_intact(lbuf, lv) and guards_intact(hbuf, hv) and torch.equal(pv.cpu(), pred)
    return lv.cpu(), hv.cpu()


def step_noise(shape, seeds, steps):
    """z of every row, fp32 on the CPU: what ops.seeded_noise writes for (seed, step) of the row at the step domain (held to noise_ref by
    tests/test_noise_gpu.py)"""
    from sduss_amd import ops
    n = shape[0]
    z = ops.seeded_noise(shape, list(seeds[:n]), list(steps[:n]), N.STEP, dtype=torch.float32)
    torch.cuda.synchronize()
    return z.cpu()


@pytest.mark.parametrize("g", [5.0, 0.0], ids=["g5", "g0"])
@pytest.mark.parametrize("shape,offset", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_is_the_unfused_one(cuda_device, dtype, shape, offset, g):
    pred, lat, hist, sigma, sigma_next, *_ = step_operands(shape, dtype, g)
    n = shape[0]
    kind, cn = KINDS[n], torch.tensor(CN[:n])
    z = step_noise(shape, SEEDS, NSTEPS)
    elems = z[0].numel()
    assert np.abs(z[n - 1].reshape(-1).double().numpy() - N.normals(SEEDS[n - 1], NSTEPS[n - 1], N.STEP, elems)).max() <= 4e-6      # idx is the row's own
    plain = lat.cuda().clone()
    from sduss_amd import ops
    ops.cfg_euler_step_(pred.cuda(), plain, sigma.cuda(), sigma_next.cuda(), g)
    plain = plain.cpu()
    for second in ([True, False, False][:n], [False, True, True][:n], [True] * n):          # first- and second-order rows, mixed and swapped
        coef = coefs(n, second)
        got, got_hist = run_step(pred, lat, hist, sigma, sigma_next, g, offset, kind, coef, CN, SEEDS, NSTEPS)
        want, want_hist = R.stochastic_step(pred, lat, sigma, sigma_next, g, kind, coef, hist, False, cn, z)
        assert_bits(got, want, f"latents, second order {second}")
        assert_bits(got_hist, want_hist, f"hist, second order {second}")
        quiet, quiet_hist = run_step(pred, lat, hist, sigma, sigma_next, g, offset, kind, coef)
        assert_bits(got_hist, quiet_hist, "hist: D carries no noise")
        for r, k in enumerate(kind):
            if k == 0:                                                    # a kind-0 row beside noisy rows: the plain step's bits, its cn never read
                assert same_bits(got[r], plain[r]) and same_bits(got_hist[r], hist[r])
            else:
                assert not same_bits(got[r], quiet[r])
    # every cn zero: the bits of mx_cfg_multistep_step, with seed and step buffers full of NaN bits (poisoned memory that must not matter)
    coef = coefs(n, [True, False, True][:n])
    quiet, quiet_hist = run_step(pred, lat, hist, sigma, sigma_next, g, offset, kind, coef)
    for seeds, steps in ((SEEDS, NSTEPS), ([NAN64] * 3, [NAN32] * 3)):
        got, got_hist = run_step(pred, lat, hist, sigma, sigma_next, g, offset, kind, coef, [0.0, 0.0, -0.0], seeds, steps)
        assert_bits(got, quiet, "latents with cn = 0")
        assert_bits(got_hist, quiet_hist, "hist with cn = 0")
    # one noisy row among rows without noise whose seeds and steps are poison: the noisy row as before, the others the multistep launch's
    noisy_row = n - 1
    cn1 = [CN[r] if r == noisy_row else 0.0 for r in range(n)]
    seeds1 = [SEEDS[r] if r == noisy_row else NAN64 for r in range(n)]
    steps1 = [NSTEPS[r] if r == noisy_row else NAN32 for r in range(n)]
    got, _h = run_step(pred, lat, hist, sigma, sigma_next, g, offset, kind, coef, cn1, seeds1, steps1)
    full, _h = run_step(pred, lat, hist, sigma, sigma_next, g, offset, kind, coef, CN, SEEDS, NSTEPS)
    for r in range(n):
        assert same_bits(got[r], full[r] if r == noisy_row else quiet[r]), r
    assert bool(torch.isfinite(got.float()).all())


@pytest.mark.parametrize("shape,offset", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_with_inpainting_rows(cuda_device, dtype, shape, offset):
    pred, lat, hist, sigma, sigma_next, init, noise, mask = step_operands(shape, dtype)
    n = shape[0]
    kind, slot, coef, cn = KINDS[n], SLOTS[n], coefs(n, [True, True, False][:n]), torch.tensor(CN[:n])
    z = step_noise(shape, SEEDS, NSTEPS)
    free, free_hist = run_step(pred, lat, hist, sigma, sigma_next, 5.0, offset, kind, coef, CN, SEEDS, NSTEPS)
    got, got_hist = run_step(pred, lat, hist, sigma, sigma_next, 5.0, offset, kind, coef, CN, SEEDS, NSTEPS, (slot, init, noise, mask))
    want, want_hist = R.stochastic_step(pred, lat, sigma, sigma_next, 5.0, kind, coef, hist, False, cn, z, slot, init, noise, mask)
    assert_bits(got, want, "latents")
    assert_bits(got_hist, want_hist, "hist")
    assert_bits(got_hist, free_hist, "hist: the unmasked D")
    for r, j in enumerate(slot):                                          # the put-back runs after the noise: kept elements carry none of it
        if j < 0:
            assert same_bits(got[r], free[r])
            continue
        kept = (mask[j] == 0)[None].expand_as(got[r])
        assert 0 < int(kept.sum()) < kept.numel()
        renoised = I.renoise(init[j:j + 1], noise[j:j + 1], 1.0, sigma_next[r])[0]
        assert torch.equal(I.bits(got[r])[kept], I.bits(renoised)[kept]) and torch.equal(I.bits(got[r])[~kept], I.bits(free[r])[~kept])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_requests_step_noise_does_not_see_the_batch(cuda_device, dtype):
    """the same row (latents, prediction, seed, step) stepped alone, as row 0 of 3 and as row 2 of 3: bit-equal, on the vector path, from an offset
    base and with 27-element rows"""
    for row_shape, offset in (((16, 16, 16), 0), ((4, 8, 8), 1), ((3, 3, 3), 0)):
        pred3, lat3, hist3, *_ = step_operands((3,) + row_shape, dtype, 0.0)
        s, sn = torch.tensor([3.1875]), torch.tensor([2.0625])
        coef = coefs(3, [True] * 3)[2:3]
        alone, alone_hist = run_step(pred3[0:1], lat3[0:1], hist3[0:1], s, sn, 0.0, offset, [1], coef, [CN[0]], [SEEDS[0]], [7])
        for pos in (0, 2):
            order = [0, 1, 2] if pos == 0 else [1, 2, 0]                  # batch row -> operand row; the request is operand row 0
            got, got_hist = run_step(pred3[order], lat3[order], hist3[order], s.expand(3), sn.expand(3), 0.0, offset, [1, 1, 1], coef.expand(3, 3).contiguous(),
                                     [CN[0]] * 3, [SEEDS[0] if o == 0 else 100 + o for o in order], [7 if o == 0 else o for o in order])
            assert same_bits(got[pos:pos + 1], alone) and same_bits(got_hist[pos:pos + 1], alone_hist), (row_shape, offset, pos)


# ---- the denoising loop ----

LAT = 16                     # a "128" request of the tiny models: 16 x 16 latents
RES = "128"


class PerRequestStub:
    """the stub predictions of a run: for a request at a step a fixed seeded tensor pair (unconditional, conditional) that depends on the request's
    id and step alone -- not on the batch -- so that a request run again alone sees the same model; every batch prediction is kept for the replay"""
    def __init__(self, seed):
        self.seed, self.preds = seed, []

    def batch(self, reqs, row_shape, dtype, cfg):
        def one(r, half):
            g = torch.Generator().manual_seed(self.seed + 1000 * r.request_id + 2 * r.step_index + half)
            return torch.randn((1,) + tuple(row_shape), generator=g).to(dtype)
        p = torch.cat([one(r, half) for half in ((0, 1) if cfg else (0,)) for r in reqs])
        self.preds.append(p)
        return p


def stub_denoiser(stub, guidance_scale=5.0):
    from sduss_amd.pipeline import SDXLDenoiser

    class Stub(SDXLDenoiser):
        def _gather(self, res, reqs, cfg):
            self.part, self.cfg = super()._gather(res, reqs, cfg), cfg
            return self.part

        def _forward(self, x, ts, cond, **kwargs):
            return {res: stub.batch(self.part.reqs, t.shape[1:], t.dtype, self.cfg).to(t.device) for res, t in x.items()}
    return Stub(SimpleNamespace(device=torch.device("cuda:0"), set_context_key=lambda uid: None), guidance_scale)


@pytest.fixture(scope="module")
def sdxl(cuda_device):
    from sduss_amd.config import UNetConfig
    from sduss_amd.pipeline import synthetic_request
    from sduss_amd.vae import MxVAEEncoder, VAEConfig
    enc = MxVAEEncoder(VAEConfig.tiny(), E.init_params(vae_ref.VAEConfig.tiny()), device="cuda:0")

    def make_req(den, i, steps, sampler="euler", schedule="default", dtype=torch.bfloat16, res=128, seed=None, eta=1.0):
        r = synthetic_request(i, res, steps, UNetConfig.tiny(), den, "cuda:0", dtype=dtype)
        if seed is not None:
            den.seed_request(r, seed)
        den.set_timesteps(r, sampler=sampler, schedule=schedule, eta=eta)
        return r
    return SimpleNamespace(make_req=make_req, enc=enc)


def client_image(seed):
    return torch.randint(0, 256, (1, 4 * LAT, 4 * LAT, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).cuda()


def half_mask():
    m = torch.full((1, 4 * LAT, 4 * LAT), 127, dtype=torch.uint8)
    m[:, :, :2 * LAT] = 128
    return m.cuda()


class Replay:
    """the CPU's copy of one request: its latents, its history and the step that left it, stepped by tests/stochastic_ref.py"""
    def __init__(self, req):
        from sduss_amd import ops
        self.req = req
        self.lat = req.latents.cpu().clone()
        self.step = req.step_index
        self.kind = R.DEVICE_KIND[req.sampler]
        self.noisy = req.sampler in R.KIND
        self.tab = None
        if self.noisy:
            self.tab = ops.sampler_coeffs(req.sampler, req.sigmas, False, eta=req.eta)
        elif self.kind:
            self.tab = ops.sampler_coeffs(req.sampler, req.sigmas, False)
        self.hist, self.hist_step = None, -1
        s = req.inpaint
        self.inpaint = None if s is None else (s.init.cpu(), s.noise.cpu(), s.mask.cpu())

    def second(self):
        return self.kind != 0 and self.hist is not None and self.hist_step == self.step - 1


def replay_step(rows, pred, g):
    """one scheduler step of the batch ``rows`` (Replay objects in batch order) from the model's output ``pred``"""
    n = len(rows)
    sig = torch.tensor([float(r.req.sigmas[r.step]) for r in rows])
    sig_next = torch.tensor([float(r.req.sigmas[r.step + 1]) for r in rows])
    coef, cn = torch.zeros(n, 3), torch.zeros(n)
    for i, r in enumerate(rows):
        if r.kind:
            coef[i] = torch.tensor([float(c) for c in S.step_coef(r.tab, r.step, r.second())])
        if r.noisy:
            cn[i] = float(r.tab[r.step, 4])
    z = step_noise(tuple(torch.cat([r.lat for r in rows]).shape), [r.req.seed or 0 for r in rows], [r.step for r in rows])
    hist = torch.cat([r.hist if r.second() else torch.full_like(r.lat, float("nan"), dtype=torch.float32) for r in rows])
    inp = [r for r in rows if r.inpaint is not None]
    extra = ()
    if inp:
        order = iter(range(len(inp)))
        extra = ([next(order) if r.inpaint is not None else -1 for r in rows], *(torch.cat([r.inpaint[k] for r in inp]) for k in range(3)))
    lat, new_hist = R.stochastic_step(pred, torch.cat([r.lat for r in rows]), sig, sig_next, g, [r.kind for r in rows], coef, hist, False, cn, z, *extra)
    for i, r in enumerate(rows):
        r.lat = lat[i:i + 1]
        if r.kind:
            r.hist, r.hist_step = new_hist[i:i + 1], r.step
        r.step += 1


def run_and_replay(den, stub, reqs, g):
    """steps ``reqs`` to the end on the device and on the CPU, comparing every request's latents after every step"""
    rows = {id(r): Replay(r) for r in reqs}
    while not all(r.done() for r in reqs):
        active = [r for r in reqs if not r.done()]
        den.denoising_step({RES: active})
        torch.cuda.synchronize()
        replay_step([rows[id(r)] for r in active], stub.preds[-1], g)
        for r in active:
            assert r.step_index == rows[id(r)].step
            assert_bits(r.latents.cpu(), rows[id(r)].lat, f"request {r.request_id} ({r.sampler}) after step {r.step_index - 1}")
    return rows


def four_requests(model, den):
    """an Euler request, a DPM-Solver++ 2M Karras request, an inpainting Euler-ancestral request and an image-to-image DPM++ 2M SDE Karras request at
    strength 0.5, of different lengths; the two from images draw their start noise from their seed"""
    a = model.make_req(den, 0, 6)
    b = model.make_req(den, 1, 8, "dpmpp_2m", "karras")
    c = model.make_req(den, 2, 7, "euler_a", "default", seed=0xC0FFEE0000000007)
    d = model.make_req(den, 3, 9, "dpmpp_2m_sde", "karras", seed=11, eta=0.75)
    den.start_inpaint(c, model.enc, client_image(32), half_mask(), strength=1.0)
    den.start_from_image(d, model.enc, client_image(31), 0.5)
    assert (c.sampler, d.sampler, d.eta) == ("euler_a", "dpmpp_2m_sde", 0.75) and c.step_index == 0 and d.step_index == 5 and d.history is None
    return [a, b, c, d]


def test_loop_equals_the_cpu_replay(sdxl):
    from sduss_amd import ops
    from sduss_amd.lib import MxError
    from sduss_amd.pipeline import karras_tables
    g = 5.0
    stub = PerRequestStub(100)
    den = stub_denoiser(stub, g)
    reqs = four_requests(sdxl, den)
    a, b, c, d = reqs
    assert np.array_equal(d.sigmas, karras_tables(9)[1])
    # the seeded starts: the initial latents of seed_request, and the kept-region noise of the inpainting request, are the request's own noise
    fresh = sdxl.make_req(den, 9, 7, seed=c.seed)
    want0 = ops.seeded_noise((1, 4, LAT, LAT), c.seed, 0, N.INIT, dtype=torch.bfloat16, scale=den.init_noise_sigma(7))
    assert same_bits(fresh.latents, want0) and fresh.seed == c.seed
    assert same_bits(c.inpaint.noise, ops.seeded_noise((1, 4, LAT, LAT), c.seed, 0, N.START, dtype=torch.bfloat16))
    start = {id(r): (r.latents.clone(), r.step_index) for r in reqs}
    rows = run_and_replay(den, stub, reqs, g)
    assert all(r.done() for r in reqs) and len(stub.preds) == 8              # one model call per step of the longest request
    finals = [r.latents.clone() for r in reqs]
    for r in reqs:
        assert bool(torch.isfinite(r.latents.float()).all())
        if r.sampler != "euler":
            assert r.history is not None and r.history.dtype == torch.float32 and r.history_step == r.num_inference_steps - 1
            assert_bits(r.history.cpu(), rows[id(r)].hist, f"history of request {r.request_id}")
    kept = (c.inpaint.mask == 0)[:, None].expand_as(c.latents)
    assert torch.equal(I.bits(c.latents)[kept], I.bits(c.inpaint.init)[kept])                      # sigma_next = 0: the image's own latents
    # the same seeded requests run alone, by a fresh Denoiser, end in the same bits; and so does each after a rewind, beside a stranger
    for i, r in ((2, c), (3, d)):
        alone = stub_denoiser(PerRequestStub(100), g)
        r.latents, r.step_index = start[id(r)][0].clone(), start[id(r)][1]
        while not r.done():
            alone.denoising_step({RES: [r]})
        torch.cuda.synchronize()
        assert_bits(r.latents.cpu(), finals[i].cpu(), f"request {r.request_id} ({r.sampler}) run alone")
        r.latents, r.step_index = start[id(r)][0].clone(), start[id(r)][1]         # rewound: its history is stale, its counter is its step index
        other = sdxl.make_req(den, 20 + i, 12, "euler_a", "karras", seed=5)
        while not r.done():
            den.denoising_step({RES: [other, r]})
        torch.cuda.synchronize()
        assert_bits(r.latents.cpu(), finals[i].cpu(), f"request {r.request_id} ({r.sampler}) rewound and re-run")
    # another seed is another image
    c2 = sdxl.make_req(den, 2, 7, "euler_a", "default", seed=c.seed + 1)
    den.start_inpaint(c2, sdxl.enc, client_image(32), half_mask(), strength=1.0)
    lone = stub_denoiser(PerRequestStub(100), g)
    while not c2.done():
        lone.denoising_step({RES: [c2]})
    torch.cuda.synchronize()
    assert not same_bits(c2.latents.cpu(), finals[2].cpu())
    # refusals: an unseeded request has no stochastic sampler, by set_timesteps or by a sampler written onto the request
    plain = sdxl.make_req(den, 30, 4)
    for sampler in R.KIND:
        with pytest.raises(MxError, match="needs a seeded request"):
            den.set_timesteps(plain, sampler=sampler)
    plain.sampler = "euler_a"
    before = plain.latents.clone()
    with pytest.raises(MxError, match="needs a seeded request"):
        den.denoising_step({RES: [plain]})
    assert same_bits(plain.latents, before) and plain.step_index == 0


def test_sd3_and_patch_parallelism_refuse(cuda_device):
    from sduss_amd.lib import MxError
    from sduss_amd.patch_parallel import PatchParallelDenoiser
    from sduss_amd.pipeline_sd3 import SD3Denoiser
    sd3 = SD3Denoiser(SimpleNamespace(device=torch.device("cuda:0")))
    den = PatchParallelDenoiser.__new__(PatchParallelDenoiser)
    for sampler in R.KIND:
        with pytest.raises(MxError, match="sampler must be one of"):
            sd3.set_timesteps(SimpleNamespace(num_inference_steps=8, seed=1), sampler=sampler)
        with pytest.raises(MxError, match="not available under patch parallelism"):
            den.step(SimpleNamespace(inpaint=None, sampler=sampler, seed=1))


def test_variance_on_the_device(sdxl):
    """The analytic denoiser of Gaussian data in the model slot (fp32 latents 1 x 4 x 64 x 64, no guidance), dpmpp_2m_sde at 20 Karras steps, eta 1:
    the sample variance of the 16384 final latents lies within 5 sqrt(2 / 16384) = 0.0552 relative of the variance the covariance recursion
    (stochastic_ref.final_variance) predicts from Var(x_0) = init_noise_sigma^2 -- five standard deviations of the sample variance of 16384
    independent normals.  Seed 1: the fp64 CPU replay of this run (noise_ref's normals through the same steps) ends 0.0096 from the prediction
    (variance 0.259623 against 0.262143), and so did the device when this was written."""
    from sduss_amd import ops
    from sduss_amd.pipeline import SDXLDenoiser

    class Analytic(SDXLDenoiser):
        def _gather(self, res, reqs, cfg):
            self.part = super()._gather(res, reqs, cfg)
            return self.part

        def _forward(self, x, ts, cond, **kwargs):
            lat, s = self.part.latents.double(), self.part.sigma.double().reshape(-1, 1, 1, 1)
            return {res: (lat * s / (S.SD ** 2 + s ** 2)).float() for res in x}
    den = Analytic(SimpleNamespace(device=torch.device("cuda:0"), set_context_key=lambda uid: None), 5.0)
    r = sdxl.make_req(den, 0, 20, "dpmpp_2m_sde", "karras", dtype=torch.float32, res=512, seed=1)
    assert r.latents.shape == (1, 4, 64, 64) and r.latents.dtype == torch.float32
    init = den.init_noise_sigma(20)
    x = init * N.normals(1, 0, N.INIT, 16384)
    assert np.abs(r.latents.cpu().double().numpy().reshape(-1) - x).max() <= init * 4e-6 + 2.0 ** -24 * init * 5.77
    tab = ops.sampler_coeffs("dpmpp_2m_sde", r.sigmas, False, eta=1.0)
    want = R.final_variance(tab, r.sigmas, init ** 2)
    prev = None
    for i in range(20):                                                    # the CPU replay in fp64
        D = S.SD ** 2 / (S.SD ** 2 + float(r.sigmas[i]) ** 2) * x
        cx, c0, c1 = (float(c) for c in S.step_coef(tab, i, prev is not None))
        x = cx * x + c0 * D + (c1 * prev if prev is not None else 0.0) + float(tab[i, 4]) * N.normals(1, i, N.STEP, 16384)
        prev = D
    while not r.done():
        den.denoising_step({"512": [r]}, do_classifier_free_guidance=False)
    torch.cuda.synchronize()
    got = r.latents.cpu().double().numpy().reshape(-1)
    bound = 5.0 * math.sqrt(2.0 / 16384)
    print(f"variance: device {got.var():.6f}, CPU replay {x.var():.6f}, recursion {want:.6f}; sd^2 {S.SD ** 2}")
    assert abs(x.var() / want - 1.0) <= bound and abs(got.var() / want - 1.0) <= bound
    # and element by element the device is the replay to fp32 accuracy: 20 steps of at most 8 roundings of 2^-24 and a 4e-6 noise error each,
    # every one relative to a sample of magnitude at most 6 init_noise_sigma, none of them amplified (every |cx + c0 a| <= 1)
    assert np.abs(got - x).max() <= 20 * (8 * 2.0 ** -24 + 4e-6) * 6 * init
