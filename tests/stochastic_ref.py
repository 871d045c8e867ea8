"""Restatements of the stochastic samplers (csrc/sampler_coeffs.cpp mx_sampler_coeffs_eta, csrc/scheduler_step.hip NOISY) for
tests/test_stochastic_sampler_cpu.py and tests/test_stochastic_step_gpu.py, in the style of tests/sampler_ref.py: the two k-diffusion rules in fp64
(sample_euler_ancestral; sample_dpmpp_2m_sde with solver_type "midpoint", s_noise 1), the per-element chain in fp32 with one torch op per operation,
and the exact propagation of the covariance of (x, D_prev) through a sampler's steps on the analytic Gaussian problem.  Everything runs on the CPU."""
from __future__ import annotations

import math

import numpy as np
import torch

import sampler_ref as S

EULER_A, DPMPP_2M_SDE = 3, 4
KIND = {"euler_a": EULER_A, "dpmpp_2m_sde": DPMPP_2M_SDE}
DEVICE_KIND = {"euler": 0, "dpmpp_2m": 1, "ab2": 2, "euler_a": 1, "dpmpp_2m_sde": 1}      # both step on D = x - sigma m


# ---- the coefficients (mx_sampler_coeffs_eta) ----

def coeffs(sampler: int, sigmas, eta: float) -> np.ndarray:
    """fp64 [n, 5] = (cx, c0 first order, c0 second order, c1 second order, cn) of every step, written as k-diffusion steps:
    Euler ancestral   x' = x + (x - D) / s * (sd - s) + su z                 = (sd / s) x + (1 - sd / s) D + su z
    2M SDE, midpoint  x' = sn / s exp(-eta h) x + E D + 0.5 E / r (D - D_prev) + sn sqrt(-expm1(-2 eta h)) z,   E = -expm1(-h - eta h)"""
    sig = [float(s) for s in np.asarray(sigmas)]
    out = np.zeros((len(sig) - 1, 5), dtype=np.float64)
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        if sn == 0.0:
            out[i] = (0.0, 1.0, 1.0, 0.0, 0.0)
        elif sampler == EULER_A:
            su = min(sn, eta * math.sqrt(sn ** 2 * (s ** 2 - sn ** 2) / s ** 2))      # get_ancestral_step
            sd = math.sqrt(sn ** 2 - su ** 2)
            out[i] = (sd / s, 1.0 - sd / s, 1.0 - sd / s, 0.0, su)
        else:
            assert sampler == DPMPP_2M_SDE
            t, t_next = -math.log(s), -math.log(sn)
            h = t_next - t
            eta_h = eta * h
            E = -math.expm1(-h - eta_h)
            out[i] = (sn / s * math.exp(-eta_h), E, E, 0.0, sn * math.sqrt(-math.expm1(-2.0 * eta_h)))
            if i > 0:
                r = (t - (-math.log(sig[i - 1]))) / h                                 # h_last / h
                out[i, 2:4] = (E + 0.5 * E / r, -0.5 * E / r)
    return out


# ---- the element chain of mx_cfg_stochastic_step, fp32 op by op ----

def stochastic_step(pred, lat, sigma, sigma_next, g, kind, coef, hist, flow, cn, z, slot=None, init=None, noise=None, mask=None):
    """what mx_cfg_stochastic_step leaves: (latents in lat's dtype, hist fp32).  kind: the device kinds per row; cn fp32 [n]; z fp32 like lat: the
    step noise of every row (ops.seeded_noise in fp32, or noise_ref).  A kind-1 / kind-2 row with cn != 0: acc = acc + (cn * z) behind the multistep
    update, both rounded on their own, then the cast; every other row as S.multistep_step; the put-back of inpainting rows after."""
    import inpaint_ref as I
    n = lat.shape[0]
    m = S.guided(pred, n, g)
    x = lat.to(torch.float32)
    out, new_hist = lat.clone(), hist.clone()
    for r in range(n):
        if kind[r] in (S.DPMPP_2M, S.AB2):
            acc, D = S.multistep_row(kind[r], x[r], m[r], sigma[r], coef[r], hist[r])
            if float(cn[r]) != 0.0:
                acc = acc + (cn[r].to(torch.float32) * z[r].to(torch.float32))
            out[r], new_hist[r] = acc.to(lat.dtype), D
        else:
            out[r] = S.euler_row(x[r], m[r], sigma[r], sigma_next[r], flow).to(lat.dtype)
    if init is not None:
        out = I.masked_step(out, flow, sigma_next.to(torch.float32), slot, init, noise, mask)
    return out, new_hist


# ---- the analytic problem: the covariance of (x, D_prev), exactly ----

def final_variance(table: np.ndarray, sigmas, var0: float) -> float:
    """Var(x) per element after every step of a sampler with the [n, >= 4] coefficient ``table`` (a fifth column: cn) on the analytic Gaussian
    problem (data N(0, SD^2), D = a x with a = SD^2 / (SD^2 + sigma^2)), from x ~ N(0, var0) at sigmas[0].  Every step is linear,
        (x', D') = A (x, D_prev) + (cn z, 0),   A = [[cx + c0 a, c1], [a, 0]],
    second order from the second step on (c1 of a first-order table row is 0), so the covariance P goes P' = A P A^T + diag(cn^2, 0) in fp64."""
    sig = np.asarray(sigmas, dtype=np.float64)
    P = np.array([[var0, 0.0], [0.0, 0.0]])
    for i in range(len(sig) - 1):
        a = S.SD ** 2 / (S.SD ** 2 + sig[i] ** 2)
        cx, c0, c1 = S.step_coef(np.asarray(table, dtype=np.float64), i, i > 0)
        cn = float(table[i][4]) if len(table[i]) > 4 else 0.0
        A = np.array([[cx + c0 * a, c1], [a, 0.0]])
        P = A @ P @ A.T + np.array([[cn * cn, 0.0], [0.0, 0.0]])
    return float(P[0, 0])
