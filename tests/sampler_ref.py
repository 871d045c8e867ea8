"""Torch / numpy restatements of the multistep samplers (csrc/scheduler_step.hip, sampler_coeffs.cpp, pipeline.karras_tables) for
tests/test_sampler_cpu.py and tests/test_sampler_gpu.py: the coefficient rules in fp64, the Karras schedule, the per-element chain in fp32 (one torch
op per operation, one cast at the end, as in inpaint_ref.py: the kernel must return the same bits), the fp64 loop of every sampler, diffusers'
variance-preserving form of DPM-Solver++ 2M, and the analytic Gaussian problem with its closed-form solution.  Everything here runs on the CPU."""
from __future__ import annotations

import math

import numpy as np
import torch

import inpaint_ref as I

EULER, DPMPP_2M, AB2 = 0, 1, 2
KIND = {"euler": EULER, "dpmpp_2m": DPMPP_2M, "ab2": AB2}


# ---- the coefficients (mx_sampler_coeffs) ----

def coeffs(sampler: int, sigmas) -> np.ndarray:
    """fp64 [n, 4] = (cx, c0 first order, c0 second order, c1 second order) of every step of the schedule ``sigmas`` [n + 1]"""
    sig = [float(s) for s in np.asarray(sigmas)]
    out = np.zeros((len(sig) - 1, 4), dtype=np.float64)
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        if sampler == DPMPP_2M:
            if sn == 0.0:
                out[i] = (0.0, 1.0, 1.0, 0.0)
                continue
            lam, lam_next = -math.log(s), -math.log(sn)
            h = lam_next - lam
            E = -math.expm1(-h)
            out[i] = (sn / s, E, E, 0.0)
            if i > 0:
                r = (lam - (-math.log(sig[i - 1]))) / h
                out[i, 2:] = (E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r))
        else:
            assert sampler == AB2
            h = sn - s
            out[i] = (1.0, h, h, 0.0)
            if i > 0:
                w = h / (2.0 * (s - sig[i - 1]))
                out[i, 2:] = (h * (1.0 + w), -h * w)
    return out


def step_coef(table: np.ndarray, step: int, second: bool) -> tuple:
    """(cx, c0, c1) of one step in one order, from a [n, 4] table"""
    cx, c0a, c0b, c1 = (table[step, j] for j in range(4))
    return (cx, c0b, c1) if second else (cx, c0a, type(c1)(0.0))


# ---- the schedules ----

def train_sigmas() -> np.ndarray:
    """the 1000 training sigmas of the SDXL scheduler config (scaled-linear betas in fp32, as diffusers computes them), ascending"""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0)
    return (((1 - ac) / ac) ** 0.5).numpy()


def karras_tables(euler_sigmas, rho: float = 7.0):
    """(timesteps f32 [n], sigmas f32 [n + 1]) of the Karras schedule between the first and the last non-zero of ``euler_sigmas`` [n + 1]"""
    n = len(euler_sigmas) - 1
    hi, lo = float(euler_sigmas[0]) ** (1.0 / rho), float(euler_sigmas[n - 1]) ** (1.0 / rho)
    sig = np.array([(hi + (i / (n - 1) if n > 1 else 0.0) * (lo - hi)) ** rho for i in range(n)], dtype=np.float64)
    log_train = np.log(train_sigmas().astype(np.float64))
    ts = []
    for s in sig:                                          # diffusers' _sigma_to_t, one sigma at a time
        ls = math.log(s)
        below = np.nonzero(log_train <= ls)[0]
        low = min(int(below[-1]) if len(below) else 0, 998)
        w = min(max((log_train[low] - ls) / (log_train[low] - log_train[low + 1]), 0.0), 1.0)
        ts.append((1.0 - w) * low + w * (low + 1))
    return np.array(ts, dtype=np.float64).astype(np.float32), np.concatenate([sig, [0.0]]).astype(np.float32)


# ---- the element chain of mx_cfg_multistep_step, fp32 op by op ----

def guided(pred: torch.Tensor, n: int, g: float) -> torch.Tensor:
    """m of every latent row in fp32: the CFG combine in the model dtype, one rounding per operation (pred = [uncond rows ; cond rows]), or the
    plain prediction for g <= 0"""
    if g <= 0:
        return pred[:n].to(torch.float32)
    u, t = pred[:n], pred[n:2 * n]
    return (u + g * (t - u)).to(torch.float32)


def _f32(v) -> torch.Tensor:
    return torch.tensor(float(v), dtype=torch.float32)


def euler_row(x: torch.Tensor, m: torch.Tensor, s, sn, flow: bool) -> torch.Tensor:
    """the model's own step of one row in fp32 (step_math.h euler_update / flow_update), before the cast"""
    s, sn = _f32(s), _f32(sn)
    if flow:
        return x + ((sn - s) * m)
    pred_x0 = x - (s * m)
    d = (x - pred_x0) / s
    return x + (d * (sn - s))


def multistep_row(kind: int, x: torch.Tensor, m: torch.Tensor, s, coef, hist) -> tuple:
    """(acc, D) of one multistep row in fp32, before the cast: D = x - (s*m) or m; acc = (cx*x) + (c0*D), + (c1*hist) only where c1 != 0"""
    cx, c0, c1 = (_f32(c) for c in coef)
    D = x - (_f32(s) * m) if kind == DPMPP_2M else m.clone()
    acc = (cx * x) + (c0 * D)
    if float(c1) != 0.0:
        acc = acc + (c1 * hist)
    return acc, D


def multistep_step(pred, lat, sigma, sigma_next, g, kind, coef, hist, flow, slot=None, init=None, noise=None, mask=None):
    """what mx_cfg_multistep_step leaves: (latents in lat's dtype, hist fp32).  kind: a list of ints per row; coef fp32 [n, 3]; hist fp32 like lat"""
    n = lat.shape[0]
    m = guided(pred, n, g)
    x = lat.to(torch.float32)
    out, new_hist = lat.clone(), hist.clone()
    for r in range(n):
        if kind[r] in (DPMPP_2M, AB2):
            acc, D = multistep_row(kind[r], x[r], m[r], sigma[r], coef[r], hist[r])
            out[r], new_hist[r] = acc.to(lat.dtype), D
        else:
            out[r] = euler_row(x[r], m[r], sigma[r], sigma_next[r], flow).to(lat.dtype)
    if init is not None:
        out = I.masked_step(out, flow, sigma_next.to(torch.float32), slot, init, noise, mask)
    return out, new_hist


# ---- the fp64 loops ----

def sample_loop(sampler: int, sigmas, model, x, flow: bool) -> np.ndarray:
    """every step of one sampler in fp64 from x at sigmas[0]; ``model(x, sigma)`` is eps (flow False) or v (flow True)"""
    sig = np.asarray(sigmas, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if sampler == EULER:
        for i in range(len(sig) - 1):
            x = x + (sig[i + 1] - sig[i]) * model(x, sig[i])          # d = (x - x0) / sigma = eps for the epsilon model, v for the flow model
        return x
    tab = coeffs(sampler, sigmas)
    prev = None
    for i in range(len(sig) - 1):
        m = model(x, sig[i])
        D = x - sig[i] * m if sampler == DPMPP_2M else m
        cx, c0, c1 = step_coef(tab, i, prev is not None)
        x = cx * x + c0 * D + (c1 * prev if c1 != 0.0 else 0.0)
        prev = D
    return x


def dpmpp_2m_vp_loop(sigmas, model, x) -> np.ndarray:
    """diffusers' DPMSolverMultistepScheduler (algorithm dpmsolver++, order 2, midpoint, lower_order_final, final sigma zero) in its own
    variance-preserving variables, fp64: alpha = 1 / sqrt(1 + sigma^2), sigma_t = sigma alpha, lambda = log alpha - log sigma_t, the sample
    x alpha.  ``x`` is the Euler-scaled sample at sigmas[0]; returns the final sample (alpha = 1 at sigma 0)."""
    sig = np.asarray(sigmas, dtype=np.float64)
    n = len(sig) - 1

    def avl(s):
        a = 1.0 / math.sqrt(1.0 + s * s)
        return a, s * a, (math.log(a) - math.log(s * a)) if s > 0 else math.inf

    y = np.asarray(x, dtype=np.float64) * avl(sig[0])[0]
    outs = []                                                       # model_outputs: the data predictions
    for i in range(n):
        a_s, st_s, lam_s = avl(sig[i])
        a_t, st_t, lam_t = avl(sig[i + 1])
        eps = model(y / a_s, sig[i])                                # the analytic model is a function of the Euler-scaled sample y / alpha
        outs.append((y - st_s * eps) / a_s)
        first = i == 0 or i == n - 1                                # lower_order_final with final_sigmas_type "zero": the last step is first order
        h = lam_t - lam_s
        em = math.expm1(-h) if math.isfinite(h) else -1.0
        if first:
            y = (st_t / st_s) * y - (a_t * em) * outs[-1]
        else:
            lam_p = avl(sig[i - 1])[2]
            r0 = (lam_s - lam_p) / h
            D0, D1 = outs[-1], (1.0 / r0) * (outs[-1] - outs[-2])
            y = (st_t / st_s) * y - (a_t * em) * D0 - 0.5 * (a_t * em) * D1
    return y / avl(sig[n])[0]


# ---- the analytic problem: data N(0, sd^2) per element ----

SD = 0.5


def eps_model(x, sigma):
    return x * sigma / (SD * SD + sigma * sigma)


def v_model(x, sigma):
    return x * (sigma - (1.0 - sigma) * SD * SD) / ((1.0 - sigma) ** 2 * SD * SD + sigma * sigma)


def exact_final(x, sigma_max, flow: bool) -> np.ndarray:
    """the ODE's solution at sigma 0 from x at sigma_max (the flow schedule starts at sigma 1)"""
    x = np.asarray(x, dtype=np.float64)
    return x * SD if flow else x * SD / math.sqrt(SD * SD + float(sigma_max) ** 2)


def rel_max_err(got, want) -> float:
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())
