"""Host-side checks of the multistep samplers (csrc/scheduler_step.hip, sampler_coeffs.cpp; pipeline.karras_tables; the request state): the entries
are declared, exported and bound and refuse bad arguments before any launch; mx_sampler_coeffs against the fp64 restatement; the variance-exploding
form of DPM-Solver++ 2M against diffusers' variance-preserving one; the order of every sampler on the analytic Gaussian problem; the fp32 element
chain against fp64; the Karras schedule; the request fields and the refusals.  No GPU: the library loads without a device."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sampler_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 4096                    # any aligned non-null address: nothing is dereferenced before a refusal
STEPS = (1, 2, 10, 50)


def _tables(n):
    """{name: (sigmas f32 [n + 1], flow)} of the three schedules at n steps"""
    from sduss_amd.pipeline import euler_tables, karras_tables
    from sduss_amd.pipeline_sd3 import flow_match_tables
    return {"sdxl": (euler_tables(n)[1], False), "karras": (karras_tables(n)[1], False), "flow": (flow_match_tables(n)[1], True)}


def test_entries_are_declared_exported_and_bound():
    from sduss_amd import lib
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "mxdenoise.h")).read()
    declared = set(re.findall(r"\b(mx_[a-z0-9_]+)\s*\(", hdr))
    for name in ("mx_cfg_multistep_step", "mx_sampler_coeffs"):
        assert name in declared and name in lib.SYMBOLS and hasattr(l, name)
        assert getattr(l, name).argtypes == lib.SYMBOLS[name][1]
    assert "} mx_multistep_rows;" in hdr and "enum { MX_SAMPLER_EULER = 0, MX_SAMPLER_DPMPP_2M = 1, MX_SAMPLER_AB2 = 2 };" in hdr
    assert [f[0] for f in lib.MultistepRows._fields_] == ["kind", "coef", "hist"]
    assert lib.SAMPLERS == {"euler": 0, "dpmpp_2m": 1, "ab2": 2} == S.KIND


def _ms(kind=OK, coef=OK, hist=1 << 30):
    from sduss_amd import lib
    m = lib.MultistepRows()
    m.kind, m.coef, m.hist = kind, coef, hist
    return m


def _rows(k=0, slot=None, init=None, noise=None, mask=None):
    from sduss_amd import lib
    r = lib.InpaintRows()
    r.k, r.slot, r.init, r.noise, r.mask = k, slot, init, noise, mask
    return r


def test_multistep_step_refuses_without_a_launch():
    from sduss_amd import lib
    fn = lib.load().mx_cfg_multistep_step
    FAR = 1 << 30                                                        # the history, far from the latents (OK) and the prediction (2 OK)
    good, none = _ms(hist=FAR), _rows()
    full = dict(slot=OK, init=OK, noise=OK, mask=OK)
    P, L = 2 * OK, OK                                                    # 2 x 4 x 16 bf16 latents = 256 bytes, the prediction 512
    cases = [((None, L, OK, OK, 5.0, 2, 4, 16, 2, 0, good, none), b"null"), ((P, None, OK, OK, 5.0, 2, 4, 16, 2, 0, good, none), b"null"),
             ((P, L, None, OK, 5.0, 2, 4, 16, 2, 0, good, none), b"null"), ((P, L, OK, None, 5.0, 2, 4, 16, 2, 0, good, none), b"null"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, None, none), b"null"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(kind=None, hist=FAR), none), b"null"), ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(coef=None, hist=FAR), none), b"null"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(hist=None), none), b"null"),
             ((P, L, OK, OK, 5.0, 0, 4, 16, 2, 0, good, none), b"positive"), ((P, L, OK, OK, 5.0, 2, -1, 16, 2, 1, good, none), b"positive"),
             ((P, L, OK, OK, 5.0, 2, 4, 0, 2, 0, good, none), b"positive"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 3, 0, good, none), b"bad dtype"), ((P, L, OK, OK, 5.0, 2, 4, 16, -1, 1, good, none), b"bad dtype"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(hist=L), none), b"alias"), ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 1, _ms(hist=P), none), b"alias"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(hist=L + 252), none), b"alias"),          # the last latent's bytes
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(hist=P + 508), none), b"alias"),          # the last conditional prediction's
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(hist=L - 508), none), b"alias"),          # the history's own last bytes reach the latents
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, good, _rows(k=-1, **full)), b"negative")]
    for missing in full:
        cases.append(((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, good, _rows(k=1, **{**full, missing: None})), b"need slot, init, noise and mask"))
    for args, msg in cases:
        ms, rows = args[-2], args[-1]
        status = fn(None, *args[:-2], C.byref(ms) if ms is not None else None, C.byref(rows))
        assert status != 0 and msg in lib.load().mx_last_error(), (args, lib.load().mx_last_error())


def test_sampler_coeffs_refusals():
    from sduss_amd import lib, ops
    from sduss_amd.lib import MxError
    l = lib.load()
    good = np.array([2.0, 1.0, 0.0], dtype=np.float32)
    out = np.zeros((2, 4), dtype=np.float32)
    assert l.mx_sampler_coeffs(2, 0, good.ctypes.data, 2, out.ctypes.data) == 0
    for args, msg in (((2, 0, None, 2, out.ctypes.data), b"null"), ((2, 0, good.ctypes.data, 2, None), b"null"),
                      ((2, 0, good.ctypes.data, 0, out.ctypes.data), b"n_steps"), ((0, 0, good.ctypes.data, 2, out.ctypes.data), b"Euler"),
                      ((3, 0, good.ctypes.data, 2, out.ctypes.data), b"unknown sampler"), ((-1, 1, good.ctypes.data, 2, out.ctypes.data), b"unknown sampler"),
                      ((1, 1, good.ctypes.data, 2, out.ctypes.data), b"flow")):
        assert l.mx_sampler_coeffs(*args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    assert b"worse than Euler" in l.mx_last_error() and b"infinity" in l.mx_last_error()       # the flow refusal says why
    for bad, msg in (([2.0, 2.0, 0.0], "strictly decreasing"), ([1.0, 2.0, 0.0], "strictly decreasing"), ([2.0, 1.0, -1.0], "negative"),
                     ([1.0, 0.0, 0.0], "strictly decreasing"), ([float("nan"), 1.0, 0.0], "negative")):
        for sampler in ("dpmpp_2m", "ab2"):
            with pytest.raises(MxError, match=msg):
                ops.sampler_coeffs(sampler, bad, False)
    with pytest.raises(MxError, match="sampler must be one of"):
        ops.sampler_coeffs("plms", good, False)
    with pytest.raises(MxError, match="Euler"):
        ops.sampler_coeffs("euler", good, False)


def _ulps(a: np.ndarray, b: np.ndarray) -> int:
    """the largest distance of two fp32 arrays in units in the last place (neither holds a NaN; -0 and +0 count as one apart at most)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max())


@pytest.mark.parametrize("n", STEPS)
def test_sampler_coeffs_match_the_restatement(n):
    from sduss_amd import ops
    for name, (sig, flow) in _tables(n).items():
        for sampler in ("ab2",) if flow else ("dpmpp_2m", "ab2"):
            got = ops.sampler_coeffs(sampler, sig, flow)
            want = S.coeffs(S.KIND[sampler], sig)
            assert got.shape == (n, 4) and got.dtype == np.float32 and np.isfinite(got).all()
            assert _ulps(got, want.astype(np.float32)) <= 1, (name, sampler, got, want)
            # c1 == 0 exactly where the history must not be read, and nowhere else; the first-order pair repeated there
            for i in range(n):
                first_only = i == 0 or (sampler == "dpmpp_2m" and sig[i + 1] == 0)
                assert (got[i, 3] == 0.0) == first_only and (not first_only or got[i, 2] == got[i, 1]), (name, sampler, i, got[i])
            if sampler == "dpmpp_2m":
                assert sig[n] == 0 and got[n - 1].tolist() == [0.0, 1.0, 1.0, 0.0]
            else:
                assert (got[:, 0] == 1.0).all() and (n < 2 or got[n - 1, 3] != 0.0)               # AB2's final step stays second order


@pytest.mark.parametrize("schedule", ["sdxl", "karras"])
def test_variance_exploding_form_equals_diffusers_variance_preserving_form(schedule):
    x0 = np.random.default_rng(3).standard_normal(64)
    for n in (2, 10, 20, 50):
        sig = _tables(n)[schedule][0]
        x = x0 * float(sig[0])
        ve = S.sample_loop(S.DPMPP_2M, sig, S.eps_model, x, False)
        vp = S.dpmpp_2m_vp_loop(sig, S.eps_model, x)
        assert np.abs(ve - vp).max() <= 1e-12 * np.abs(vp).max(), (n, np.abs(ve - vp).max() / np.abs(vp).max())


def _err(sampler, schedule, n):
    sig, flow = _tables(n)[schedule]
    x = np.random.default_rng(5).standard_normal(256) * (1.0 if flow else np.sqrt(S.SD ** 2 + float(sig[0]) ** 2))
    got = S.sample_loop(sampler, sig, S.v_model if flow else S.eps_model, x, flow)
    return S.rel_max_err(got, S.exact_final(x, sig[0], flow))


def test_order_on_the_analytic_problem():
    """the restatement alone (the library's coefficients are its own to 1 ulp): second order where it is claimed, first order for Euler"""
    e = {(s, sch, n): _err(S.KIND[s], sch, n) for s, sch in (("euler", "karras"), ("dpmpp_2m", "karras"), ("euler", "flow"), ("ab2", "flow"))
         for n in (20, 40)}
    print({k: f"{v:.3g}" for k, v in e.items()})
    assert e["dpmpp_2m", "karras", 20] < e["euler", "karras", 40]
    assert e["ab2", "flow", 20] < e["euler", "flow", 40]
    for s, sch in (("dpmpp_2m", "karras"), ("ab2", "flow")):
        assert e[s, sch, 20] / e[s, sch, 40] >= 3.0, (s, e[s, sch, 20] / e[s, sch, 40])
    for sch in ("karras", "flow"):
        assert e["euler", sch, 20] / e["euler", sch, 40] <= 2.5, (sch, e["euler", sch, 20] / e["euler", sch, 40])
    # the sampler is refused on the flow model because it is worse than Euler there, and gains little without the Karras schedule
    assert _err(S.DPMPP_2M, "flow", 20) > e["euler", "flow", 20]
    assert _err(S.DPMPP_2M, "sdxl", 20) > 5 * e["dpmpp_2m", "karras", 20]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_fp32_chain_against_fp64(dtype):
    """Before the cast, the chain of separately rounded fp32 operations is within 6 * 2^-24 * (|cx x| + |c0| (|x| + |sigma m|) + |c1 hist|) of its
    exact evaluation on the same fp32 operands, for DPM-Solver++ 2M: five roundings (sigma m, the difference, two products counted with the sums
    they enter, the sums), each at most 2^-24 of a term of that sum.  AB2's D is m itself, so the term of c0 is |c0 m|."""
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for n in (10, 20, 50):
        for name, (sig, flow) in _tables(n).items():
            for sampler in (S.AB2,) if flow else (S.DPMPP_2M, S.AB2):
                tab = S.coeffs(sampler, sig).astype(np.float32)
                for i in range(n):
                    x = (torch.randn(512, generator=g) * float(np.sqrt(1 + sig[i] ** 2))).to(dtype).float()
                    m = torch.randn(512, generator=g).to(dtype).float()
                    hist = torch.randn(512, generator=g) * (1.0 if sampler == S.AB2 else 2.0)
                    for second in (False, True) if i > 0 else (False,):
                        cx, c0, c1 = S.step_coef(tab, i, second)
                        acc, D = S.multistep_row(sampler, x, m, np.float32(sig[i]), (cx, c0, c1), hist)
                        assert acc.dtype == torch.float32 and D.dtype == torch.float32
                        xd, md, hd, s = x.double(), m.double(), hist.double(), float(np.float32(sig[i]))
                        Dd = xd - s * md if sampler == S.DPMPP_2M else md
                        exact = float(cx) * xd + float(c0) * Dd + float(c1) * hd
                        term = (xd.abs() + (s * md).abs()) if sampler == S.DPMPP_2M else md.abs()
                        bound = 6 * 2.0 ** -24 * ((float(cx) * xd).abs() + abs(float(c0)) * term + (float(c1) * hd).abs())
                        share = float(((acc.double() - exact).abs() / bound).max())
                        worst = max(worst, share)
                        assert share <= 1.0, (name, sampler, n, i, second, share)
    print(f"largest share of the bound: {worst:.3f}")


@pytest.mark.parametrize("n", [1, 2, 3, 10, 20, 50])
def test_karras_tables(n):
    from sduss_amd.pipeline import euler_tables, karras_tables
    ets, esig, einit = euler_tables(n)
    ts, sig, init = karras_tables(n)
    assert ts.dtype == np.float32 and sig.dtype == np.float32 and ts.shape == (n,) and sig.shape == (n + 1,)
    assert sig[0] == esig[0] and sig[n] == 0.0 and init == einit
    assert sig[n - 1] == esig[n - 1]                                    # through the rho-th root and back in fp64, rounded once
    assert (np.diff(sig.astype(np.float64)) < 0).all()
    assert (ts >= 0).all() and (ts <= 999).all() and (np.diff(ts.astype(np.float64)) <= 0).all()
    assert abs(float(ts[0]) - float(ets[0])) <= 1e-3                    # sigma max sits on its training step
    rts, rsig = S.karras_tables(esig)
    assert np.array_equal(sig, rsig) and np.abs(ts.astype(np.float64) - rts).max() <= 1e-3
    if n == 10:                                                         # rho 7 packs the steps at the low sigmas
        assert sig[5] < esig[5]


def _denoisers():
    from sduss_amd.pipeline import SDXLDenoiser
    from sduss_amd.pipeline_sd3 import SD3Denoiser
    model = SimpleNamespace(device="cpu")
    return SDXLDenoiser(model), SD3Denoiser(model)


def test_requests_construct_as_before_and_set_timesteps_defaults_are_todays():
    from sduss_amd.pipeline import Request, euler_tables, karras_tables
    from sduss_amd.pipeline_sd3 import SD3Request, flow_match_tables
    sdxl, sd3 = _denoisers()
    t = torch.zeros(1)
    a, b = Request(0, 128, 10, t, t, t, t, t, t, t), SD3Request(1, 128, 8, t, t, t, t, t)
    for r in (a, b):
        assert r.sampler == "euler" and r.history is None and r.history_step == -1 and r.inpaint is None and r.step_index == 0
    a.step_index = b.step_index = 3
    sdxl.set_timesteps(a)
    sd3.set_timesteps(b)
    assert np.array_equal(a.timesteps, euler_tables(10)[0]) and np.array_equal(a.sigmas, euler_tables(10)[1])
    assert np.array_equal(b.timesteps, flow_match_tables(8)[0]) and np.array_equal(b.sigmas, flow_match_tables(8)[1])
    for r in (a, b):
        assert r.step_index == 0 and r.sampler == "euler" and r.history is None and r.history_step == -1
    assert sdxl._multistep_rows([a, a]) is None and sd3._multistep_rows([b]) is None           # all Euler: today's launch
    a.history, a.history_step = t, 4
    sdxl.set_timesteps(a, sampler="dpmpp_2m", schedule="karras")
    assert a.sampler == "dpmpp_2m" and a.history is None and a.history_step == -1
    assert np.array_equal(a.sigmas, karras_tables(10)[1]) and np.array_equal(a.timesteps, karras_tables(10)[0])
    assert sdxl.init_noise_sigma(10) == euler_tables(10)[2]
    sd3.set_timesteps(b, sampler="ab2")
    assert b.sampler == "ab2" and np.array_equal(b.sigmas, flow_match_tables(8)[1])
    # the rows of a mixed resolution: kinds in batch order, the library's coefficients per request, zeros for the Euler row
    c = Request(2, 128, 6, t, t, t, t, t, t, t)
    sdxl.set_timesteps(c, sampler="ab2")
    e = Request(3, 128, 4, t, t, t, t, t, t, t)
    sdxl.set_timesteps(e)
    kinds, tab = sdxl._multistep_rows([e, a, c])
    from sduss_amd import ops
    assert kinds == [0, 1, 2] and tab.shape == (3, 10, 4) and not tab[0].any() and not tab[2, 6:].any()
    assert np.array_equal(tab[1], ops.sampler_coeffs("dpmpp_2m", a.sigmas, False)) and np.array_equal(tab[2, :6], ops.sampler_coeffs("ab2", c.sigmas, False))
    kinds, tab = sd3._multistep_rows([b])
    assert kinds == [2] and np.array_equal(tab[0], ops.sampler_coeffs("ab2", b.sigmas, True))


def test_refusals_of_samplers_and_schedules():
    from sduss_amd.lib import MxError
    from sduss_amd.patch_parallel import PatchParallelDenoiser
    sdxl, sd3 = _denoisers()
    req = SimpleNamespace(num_inference_steps=8)
    with pytest.raises(MxError, match="dpmpp_2m is refused on the flow model"):
        sd3.set_timesteps(req, sampler="dpmpp_2m")
    with pytest.raises(MxError, match="karras"):
        sd3.set_timesteps(req, schedule="karras")
    with pytest.raises(MxError, match="sampler must be one of"):
        sd3.set_timesteps(req, sampler="plms")
    with pytest.raises(MxError, match="sampler must be one of"):
        sdxl.set_timesteps(req, sampler="heun")
    with pytest.raises(MxError, match="schedule must be"):
        sdxl.set_timesteps(req, schedule="exponential")
    assert not hasattr(req, "sigmas")                                   # a refusal leaves the request as it was
    den = PatchParallelDenoiser.__new__(PatchParallelDenoiser)          # the refusal comes before anything of the model is touched
    for sampler in ("dpmpp_2m", "ab2"):
        with pytest.raises(MxError, match="multistep samplers are not available under patch parallelism"):
            den.step(SimpleNamespace(inpaint=None, sampler=sampler))


def test_wrapper_checks_shapes_and_dtypes():
    from sduss_amd import ops
    from sduss_amd.lib import MxError
    lat = torch.zeros(2, 4, 4, 4, dtype=torch.bfloat16)
    pred = torch.zeros(4, 4, 4, 4, dtype=torch.bfloat16)
    sg = torch.ones(2)
    kind = torch.tensor([1, 2], dtype=torch.int32)
    coef = torch.zeros(2, 3)
    hist = torch.zeros(2, 4, 4, 4)
    fn = ops.cfg_multistep_step_
    with pytest.raises(MxError, match="prediction"):
        fn(pred[:3], lat, sg, sg, 5.0, kind, coef, hist, False)
    with pytest.raises(MxError, match="kind must"):
        fn(pred, lat, sg, sg, 5.0, kind.long(), coef, hist, False)
    with pytest.raises(MxError, match="coef must"):
        fn(pred, lat, sg, sg, 5.0, kind, torch.zeros(2, 4), hist, False)
    with pytest.raises(MxError, match="hist must"):
        fn(pred, lat, sg, sg, 5.0, kind, coef, hist.to(torch.bfloat16), True)
    with pytest.raises(MxError, match="hist must"):
        fn(pred, lat, sg, sg, 5.0, kind, coef, hist[:1], True)
    with pytest.raises(MxError, match="one value per latent row"):
        fn(pred, lat, sg[:1], sg, 5.0, kind, coef, hist, False)
    with pytest.raises(MxError, match="need slot"):
        fn(pred, lat, sg, sg, 5.0, kind, coef, hist, False, init=torch.zeros(1, 4, 4, 4, dtype=torch.bfloat16))


def test_sampler_walk_builds_and_passes():
    """the coefficient tables under AddressSanitizer + UBSan, as a program of its own (tests/sampler_coeffs_walk.cpp)"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "sduss_amd", "csrc"), "sampler_walk"], capture_output=True, text=True)
    assert out.returncode == 0 and "SAMPLER_COEFFS_WALK_OK 20 tables" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
