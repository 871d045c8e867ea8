// The step coefficients of the multistep samplers (scheduler_step.hip), built on the host: DPM-Solver++ 2M in k-diffusion's variance-exploding form
// (sample_dpmpp_2m) and the second-order Adams-Bashforth step on a non-uniform sigma grid; with a noise coefficient cn beside them, the stochastic
// samplers Euler ancestral (sample_euler_ancestral) and DPM-Solver++ 2M SDE (sample_dpmpp_2m_sde, midpoint), whose eta = 0 is DPM-Solver++ 2M by
// the same code.  Host only and plain C++: nothing of HIP is included, so
// tests/sampler_coeffs_walk.cpp links this file alone.  Everything is double precision, each coefficient rounded to float once; this file is
// compiled without FMA contraction (Makefile), so the Python restatement of the tests computes the same doubles.
#include <cmath>
#include <string>

#include "../../include/mxdenoise.h"

#pragma STDC FP_CONTRACT OFF

namespace mx {
void set_error(const std::string& msg);   // capi.cpp (the walk brings its own)

// every entry's table: `cols` = 4 (cx, c0 first order, c0 second order, c1) or 5 (+ cn) per step
static int sampler_coeffs(const std::string& what, int sampler, int flow, const float* sigmas, int n_steps, double eta, float* out, int cols) {
  if (!sigmas || !out) { set_error(what + ": null table"); return 1; }
  if (n_steps < 1) { set_error(what + ": n_steps must be at least 1"); return 1; }
  if (sampler == MX_SAMPLER_EULER) { set_error(what + ": the Euler step has no coefficients (its rows are kind 0 of the step launch)"); return 1; }
  const bool stochastic = cols == 5 && (sampler == MX_SAMPLER_EULER_A || sampler == MX_SAMPLER_DPMPP_2M_SDE);
  if (sampler != MX_SAMPLER_DPMPP_2M && sampler != MX_SAMPLER_AB2 && !stochastic) { set_error(what + ": unknown sampler"); return 1; }
  if (sampler == MX_SAMPLER_DPMPP_2M && flow) {
    set_error(what + ": DPM-Solver++ 2M is refused for the flow model: its log-SNR is -infinity at sigma = 1 and on the analytic Gaussian "
                     "problem it is worse than Euler at 10, 20 and 40 steps (0.59 / 0.36 / 0.12 against 0.285 / 0.143 / 0.072); use AB2");
    return 1;
  }
  if (stochastic && flow) { set_error(what + ": the stochastic samplers are refused for the flow model"); return 1; }
  if (stochastic && !(eta >= 0.0)) { set_error(what + ": eta must not be negative (or NaN)"); return 1; }
  if (!stochastic) eta = 0.0;                            // DPM-Solver++ 2M is its SDE form without noise
  for (int i = 0; i <= n_steps; ++i) {
    if (!(sigmas[i] >= 0.0f)) { set_error(what + ": sigmas must not be negative (or NaN)"); return 1; }
    if (i > 0 && !(sigmas[i] < sigmas[i - 1])) { set_error(what + ": sigmas must be strictly decreasing"); return 1; }
  }
  if (!std::isfinite(sigmas[0])) { set_error(what + ": sigmas must be finite"); return 1; }
  for (int i = 0; i < n_steps; ++i) {
    const double s = sigmas[i], sn = sigmas[i + 1];
    double cx, c0_first, c0_second, c1, cn = 0.0;
    if (sampler == MX_SAMPLER_DPMPP_2M || sampler == MX_SAMPLER_DPMPP_2M_SDE) {
      if (sn == 0.0) {                                   // the last step to sigma 0: the data prediction itself, first order whatever came before
        cx = 0.0; c0_first = c0_second = 1.0; c1 = 0.0;
      } else {
        const double lam = -std::log(s), lam_next = -std::log(sn);
        const double h = lam_next - lam;
        const double eta_h = eta * h;                    // eta = 0: -h - 0 is -h, exp(-0) is 1 and expm1(-0) is -0, so the bits of the ODE form
        const double E = -std::expm1(-h - eta_h);
        cx = (sn / s) * std::exp(-eta_h);
        c0_first = c0_second = E;
        c1 = 0.0;
        if (i > 0) {
          const double r = (lam - (-std::log((double)sigmas[i - 1]))) / h;
          c0_second = E * (1.0 + 1.0 / (2.0 * r));
          c1 = -E / (2.0 * r);
        }
        cn = sn * std::sqrt(-std::expm1(-2.0 * eta_h));
      }
    } else if (sampler == MX_SAMPLER_EULER_A) {
      if (sn == 0.0) {
        cx = 0.0; c0_first = c0_second = 1.0; c1 = 0.0;
      } else {
        const double su = std::fmin(sn, eta * std::sqrt(sn * sn * (s * s - sn * sn) / (s * s)));
        const double sd = std::sqrt(sn * sn - su * su);
        cx = sd / s;
        c0_first = c0_second = 1.0 - sd / s;
        c1 = 0.0;
        cn = su;
      }
    } else {
      const double h = sn - s;
      cx = 1.0;
      c0_first = c0_second = h;
      c1 = 0.0;
      if (i > 0) {
        const double w = h / (2.0 * (s - (double)sigmas[i - 1]));
        c0_second = h * (1.0 + w);
        c1 = -h * w;
      }
    }
    float* o = out + cols * (long)i;
    o[0] = (float)cx; o[1] = (float)c0_first; o[2] = (float)c0_second; o[3] = (float)c1;
    if (cols == 5) o[4] = (float)cn;
  }
  return 0;
}
}  // namespace mx

extern "C" int mx_sampler_coeffs(int sampler, int flow, const float* sigmas, int n_steps, float* out) {
  return mx::sampler_coeffs("sampler_coeffs", sampler, flow, sigmas, n_steps, 0.0, out, 4);
}

extern "C" int mx_sampler_coeffs_eta(int sampler, int flow, const float* sigmas, int n_steps, double eta, float* out) {
  return mx::sampler_coeffs("sampler_coeffs_eta", sampler, flow, sigmas, n_steps, eta, out, 5);
}
