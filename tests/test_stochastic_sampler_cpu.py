"""Host-side checks of the stochastic samplers (csrc/sampler_coeffs.cpp mx_sampler_coeffs_eta, csrc/scheduler_step.hip mx_cfg_stochastic_step,
the request's seed): the entries are declared, exported and bound and refuse bad arguments before any launch; the coefficients against the fp64
restatement of k-diffusion's two rules (tests/stochastic_ref.py); eta = 0 against the deterministic samplers; the variance each sampler ends with
on the analytic Gaussian problem; the request fields and the refusals of set_timesteps.  No GPU: the library loads without a device."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sampler_ref as S
import stochastic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 4096                    # any aligned non-null address: nothing is dereferenced before a refusal
NAMES = ("euler_a", "dpmpp_2m_sde")


def _tables():
    """the two tables of the coefficient checks: a 10-step Karras table and the default SDXL table (50 steps)"""
    from sduss_amd.pipeline import euler_tables, karras_tables
    return {"karras 10": karras_tables(10)[1], "sdxl 50": euler_tables(50)[1]}


def _ulps(a: np.ndarray, b: np.ndarray) -> int:
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max())


def test_entries_are_declared_exported_and_bound():
    from sduss_amd import lib
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "mxdenoise.h")).read()
    declared = set(re.findall(r"\b(mx_[a-z0-9_]+)\s*\(", hdr))
    for name in ("mx_cfg_stochastic_step", "mx_sampler_coeffs_eta"):
        assert name in declared and name in lib.SYMBOLS and hasattr(l, name)
        assert getattr(l, name).argtypes == lib.SYMBOLS[name][1]
    assert "} mx_noise_rows;" in hdr and "enum { MX_SAMPLER_EULER_A = 3, MX_SAMPLER_DPMPP_2M_SDE = 4 };" in hdr
    assert [f[0] for f in lib.NoiseRows._fields_] == ["cn", "seed", "step"]
    assert lib.STOCHASTIC_SAMPLERS == {"euler_a": 3, "dpmpp_2m_sde": 4} == R.KIND
    assert not set(lib.STOCHASTIC_SAMPLERS) & set(lib.SAMPLERS)          # SAMPLERS stays the kinds of a row of the step launch


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0, 1.3])
def test_coefficients_match_the_restatement(eta):
    """to one float rounding: the library's doubles are the restatement's up to the last place of exp / expm1 / log / sqrt compositions, each
    coefficient rounded to float once -- at most 1 ulp apart, as tests/test_sampler_cpu.py holds the deterministic samplers"""
    from sduss_amd import ops
    for name, sig in _tables().items():
        n = len(sig) - 1
        for sampler in NAMES:
            got = ops.sampler_coeffs(sampler, sig, False, eta=eta)
            want = R.coeffs(R.KIND[sampler], sig, eta)
            assert got.shape == (n, 5) and got.dtype == np.float32 and np.isfinite(got).all()
            assert _ulps(got, want.astype(np.float32)) <= 1, (name, sampler, got, want)
            assert got[n - 1].tolist() == [0.0, 1.0, 1.0, 0.0, 0.0]                        # sigma_next = 0: the data prediction, no noise
            assert (got[:, 4] >= 0).all() and ((got[:n - 1, 4] > 0) == (eta > 0)).all()
            if sampler == "euler_a":
                assert (got[:, 3] == 0).all() and np.array_equal(got[:, 1], got[:, 2])     # c1 = 0 always: the history is never read
            else:
                assert got[0, 3] == 0 and (got[1:n - 1, 3] != 0).all()
            # the noise level of the next sigma is met exactly by both: cx^2 s^2 + cn^2 = sn^2
            s, sn = sig[:-1].astype(np.float64), sig[1:].astype(np.float64)
            assert np.abs(got[:, 0].astype(np.float64) ** 2 * s ** 2 + got[:, 4].astype(np.float64) ** 2 - sn ** 2).max() <= 1e-6 * float(s.max()) ** 2


def test_eta_zero_is_the_deterministic_sampler():
    from sduss_amd import ops
    g = torch.Generator().manual_seed(4)
    for name, sig in _tables().items():
        sde, ode = ops.sampler_coeffs("dpmpp_2m_sde", sig, False, eta=0.0), ops.sampler_coeffs("dpmpp_2m", sig, False)
        assert np.array_equal(sde[:, :4].view(np.int32), ode.view(np.int32)) and not sde[:, 4].any(), name      # the bits of DPM-Solver++ 2M
        for sampler in ("dpmpp_2m", "ab2"):                              # the deterministic samplers through the same entry: their bits, cn = 0
            five = ops.sampler_coeffs(sampler, sig, False, eta=0.7)
            assert np.array_equal(five[:, :4].view(np.int32), ops.sampler_coeffs(sampler, sig, False).view(np.int32)) and not five[:, 4].any()
        ea = ops.sampler_coeffs("euler_a", sig, False, eta=0.0).astype(np.float64)
        assert not ea[:, 4].any() and np.abs(ea[:, 0] + ea[:, 1] - 1.0).max() <= 2.0 ** -24       # two roundings of values below 1
        for i in range(len(sig) - 1):                                    # and it steps as Euler: x + (sn - s) (x - D) / s
            s, sn = float(sig[i]), float(sig[i + 1])
            x = torch.randn(256, generator=g, dtype=torch.float64) * (1 + s * s) ** 0.5
            D = torch.randn(256, generator=g, dtype=torch.float64)
            euler = x + (sn - s) * (x - D) / s
            mine = ea[i, 0] * x + ea[i, 1] * D
            assert float((mine - euler).abs().max()) <= 1e-6 * float(euler.abs().max()), (name, i)


def test_coefficient_refusals():
    from sduss_amd import lib, ops
    from sduss_amd.lib import MxError
    l = lib.load()
    good = np.array([2.0, 1.0, 0.0], dtype=np.float32)
    out = np.zeros((2, 5), dtype=np.float32)
    for sampler in (3, 4):
        assert l.mx_sampler_coeffs_eta(sampler, 0, good.ctypes.data, 2, 1.0, out.ctypes.data) == 0
        for args, msg in (((sampler, 1, good.ctypes.data, 2, 1.0, out.ctypes.data), b"flow"), ((sampler, 0, good.ctypes.data, 2, -1e-9, out.ctypes.data), b"eta"),
                          ((sampler, 0, good.ctypes.data, 2, float("nan"), out.ctypes.data), b"eta"), ((sampler, 0, None, 2, 1.0, out.ctypes.data), b"null"),
                          ((sampler, 0, good.ctypes.data, 2, 1.0, None), b"null"), ((sampler, 0, good.ctypes.data, 0, 1.0, out.ctypes.data), b"n_steps")):
            assert l.mx_sampler_coeffs_eta(*args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    for args, msg in (((0, 0, good.ctypes.data, 2, 1.0, out.ctypes.data), b"Euler"), ((5, 0, good.ctypes.data, 2, 1.0, out.ctypes.data), b"unknown sampler"),
                      ((1, 1, good.ctypes.data, 2, 1.0, out.ctypes.data), b"flow")):
        assert l.mx_sampler_coeffs_eta(*args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    for sampler in NAMES:
        for bad, msg in (([2.0, 2.0, 0.0], "strictly decreasing"), ([2.0, 1.0, -1.0], "negative")):
            with pytest.raises(MxError, match=msg):
                ops.sampler_coeffs(sampler, bad, False, eta=1.0)
        with pytest.raises(MxError, match="flow"):
            ops.sampler_coeffs(sampler, good, True, eta=1.0)
        with pytest.raises(MxError, match="eta"):
            ops.sampler_coeffs(sampler, good, False, eta=-1.0)
        with pytest.raises(MxError, match="sampler must be one of"):     # without eta: the four-column entry, which does not know them
            ops.sampler_coeffs(sampler, good, False)


def test_the_sampler_is_the_right_one():
    """The analytic denoiser of Gaussian data (sd 0.5): every step is linear, so the covariance of (x, D_prev) goes through
    the steps exactly (stochastic_ref.final_variance, fp64) from Var(x) = sd^2 + sigma_max^2.  |Var(x_final) / sd^2 - 1| at 10 / 20 / 40 Karras steps
    and eta = 1, with the library's own coefficients, shrinks with the step count for both samplers.  The figures, as measured:
        euler_a        0.4404   0.2735   0.1569
        dpmpp_2m_sde   0.1240   0.0486   0.0077
    (a wrong cn, a wrong sign of c1 or noise that is not fresh every step shows here: the variance then does not approach sd^2 at all)"""
    from sduss_amd import ops
    from sduss_amd.pipeline import karras_tables
    err = {}
    for sampler in NAMES:
        for n in (10, 20, 40):
            sig = karras_tables(n)[1]
            tab = ops.sampler_coeffs(sampler, sig, False, eta=1.0)
            var = R.final_variance(tab, sig, S.SD ** 2 + float(sig[0]) ** 2)
            err[sampler, n] = abs(var / S.SD ** 2 - 1.0)
            # the restatement's own fp64 coefficients end at the same variance: the library's are theirs within 1 ulp (2^-23 relative), a variance
            # takes each step's twice (squared), and the history term of opposite sign amplifies the relative error by (|c0| + |c1|) / (c0 + c1) < 2
            ref = R.final_variance(R.coeffs(R.KIND[sampler], sig, 1.0), sig, S.SD ** 2 + float(sig[0]) ** 2)
            assert abs(var - ref) <= 4 * n * 2.0 ** -23 * ref, (sampler, n, var, ref)
    print({k: f"{v:.4f}" for k, v in err.items()})
    for sampler in NAMES:
        assert err[sampler, 10] > err[sampler, 20] > err[sampler, 40], (sampler, err)
    # without noise in the recursion the stochastic coefficients contract too much: the noise term is what carries the variance
    sig = karras_tables(20)[1]
    tab = ops.sampler_coeffs("dpmpp_2m_sde", sig, False, eta=1.0).copy()
    tab[:, 4] = 0.0
    assert abs(R.final_variance(tab, sig, S.SD ** 2 + float(sig[0]) ** 2) / S.SD ** 2 - 1.0) > 5 * err["dpmpp_2m_sde", 20]


def _ms(kind=OK, coef=OK, hist=1 << 30):
    from sduss_amd import lib
    m = lib.MultistepRows()
    m.kind, m.coef, m.hist = kind, coef, hist
    return m


def _nz(cn=OK, seed=OK, step=OK):
    from sduss_amd import lib
    z = lib.NoiseRows()
    z.cn, z.seed, z.step = cn, seed, step
    return z


def test_stochastic_step_refuses_without_a_launch():
    from sduss_amd import lib
    l = lib.load()
    fn = l.mx_cfg_stochastic_step
    rows = lib.InpaintRows()
    P, L, FAR = 2 * OK, OK, 1 << 30
    good, noise = _ms(hist=FAR), _nz()
    cases = [((None, L, OK, OK, 5.0, 2, 4, 16, 2, 0, good, noise), b"null"), ((P, None, OK, OK, 5.0, 2, 4, 16, 2, 0, good, noise), b"null"),
             ((P, L, None, OK, 5.0, 2, 4, 16, 2, 0, good, noise), b"null"), ((P, L, OK, None, 5.0, 2, 4, 16, 2, 0, good, noise), b"null"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, None, noise), b"null"), ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(kind=None, hist=FAR), noise), b"null"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(hist=None), noise), b"null"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, good, _nz(cn=None)), b"null cn, seed or step"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, good, _nz(seed=None)), b"null cn, seed or step"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, good, _nz(step=None)), b"null cn, seed or step"),
             ((P, L, OK, OK, 5.0, 0, 4, 16, 2, 0, good, noise), b"positive"), ((P, L, OK, OK, 5.0, 2, 4, 0, 2, 0, good, noise), b"positive"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 3, 0, good, noise), b"bad dtype"),
             ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(hist=L), noise), b"alias"), ((P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, _ms(hist=P + 508), noise), b"alias")]
    for args, msg in cases:
        ms, nz = args[-2], args[-1]
        status = fn(None, *args[:-2], C.byref(ms) if ms is not None else None, C.byref(rows), C.byref(nz))
        assert status != 0 and msg in l.mx_last_error() and b"cfg_stochastic_step" in l.mx_last_error(), (args, l.mx_last_error())
    bad = lib.InpaintRows()
    bad.k = -1
    assert fn(None, P, L, OK, OK, 5.0, 2, 4, 16, 2, 0, C.byref(good), C.byref(bad), C.byref(noise)) != 0 and b"negative" in l.mx_last_error()


def _denoisers():
    from sduss_amd.pipeline import SDXLDenoiser
    from sduss_amd.pipeline_sd3 import SD3Denoiser
    model = SimpleNamespace(device="cpu")
    return SDXLDenoiser(model), SD3Denoiser(model)


def test_request_seed_and_set_timesteps():
    from sduss_amd import ops
    from sduss_amd.lib import MxError
    from sduss_amd.patch_parallel import PatchParallelDenoiser
    from sduss_amd.pipeline import Request, karras_tables
    sdxl, sd3 = _denoisers()
    t = torch.zeros(1)
    a = Request(0, 128, 10, t, t, t, t, t, t, t)
    assert a.seed is None and a.eta == 0.0
    for sampler in NAMES:
        with pytest.raises(MxError, match="needs a seeded request"):     # an unseeded request cannot be reproduced: refused, nothing set
            sdxl.set_timesteps(a, sampler=sampler)
        assert a.sigmas is None and a.sampler == "euler"
        with pytest.raises(MxError, match="sampler must be one of"):     # the flow model has no stochastic sampler
            sd3.set_timesteps(SimpleNamespace(num_inference_steps=8, seed=3), sampler=sampler)
    a.seed = 2 ** 64 - 5
    with pytest.raises(MxError, match="eta must not be negative"):
        sdxl.set_timesteps(a, sampler="euler_a", eta=-0.1)
    for schedule, tables in (("default", sdxl._table(10)), ("karras", karras_tables(10))):       # both work on either schedule
        for sampler in NAMES:
            a.history, a.history_step, a.step_index = t, 4, 3
            sdxl.set_timesteps(a, sampler=sampler, schedule=schedule, eta=0.75)
            assert (a.sampler, a.eta, a.step_index, a.history, a.history_step) == (sampler, 0.75, 0, None, -1)
            assert np.array_equal(a.sigmas, tables[1]) and np.array_equal(a.timesteps, tables[0])
    # the rows of a mixed resolution: both stochastic samplers are kind-1 rows on the device; cn and seed per row, zeros for the others
    b = Request(1, 128, 6, t, t, t, t, t, t, t, seed=7)
    sdxl.set_timesteps(b, sampler="euler_a")
    e = Request(2, 128, 4, t, t, t, t, t, t, t)
    sdxl.set_timesteps(e)
    d = Request(3, 128, 5, t, t, t, t, t, t, t)
    sdxl.set_timesteps(d, sampler="dpmpp_2m", schedule="karras")
    assert b.eta == 1.0 and e.eta == 0.0
    kinds, tab, (cn, seeds) = sdxl._multistep_rows([e, a, b, d])
    fa, fb = ops.sampler_coeffs("dpmpp_2m_sde", a.sigmas, False, eta=0.75), ops.sampler_coeffs("euler_a", b.sigmas, False, eta=1.0)
    assert kinds == [0, 1, 1, 1] and tab.shape == (4, 10, 4) and cn.shape == (4, 10) and seeds == [0, 2 ** 64 - 5, 7, 0]
    assert np.array_equal(tab[1], fa[:, :4]) and np.array_equal(cn[1], fa[:, 4]) and np.array_equal(tab[2, :6], fb[:, :4]) and np.array_equal(cn[2, :6], fb[:, 4])
    assert not tab[0].any() and not cn[0].any() and not cn[3].any() and not cn[2, 6:].any()
    assert np.array_equal(tab[3, :5], ops.sampler_coeffs("dpmpp_2m", d.sigmas, False))
    assert len(sdxl._multistep_rows([e, d])) == 2                       # no stochastic request: the multistep launch of before
    b.seed = None
    with pytest.raises(MxError, match="needs a seeded request"):
        sdxl._multistep_rows([b])
    den = PatchParallelDenoiser.__new__(PatchParallelDenoiser)          # the refusal comes before anything of the model is touched
    for sampler in NAMES:
        with pytest.raises(MxError, match="multistep samplers are not available under patch parallelism"):
            den.step(SimpleNamespace(inpaint=None, sampler=sampler, seed=1))


def test_stochastic_walk_builds_and_passes():
    """the five-column tables under AddressSanitizer + UBSan, as a program of its own (tests/stochastic_coeffs_walk.cpp)"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "sduss_amd", "csrc"), "stochastic_walk"], capture_output=True, text=True)
    assert out.returncode == 0 and "STOCHASTIC_COEFFS_WALK_OK 64 tables" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
