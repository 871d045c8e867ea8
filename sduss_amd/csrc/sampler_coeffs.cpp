// The step coefficients of the multistep samplers (scheduler_step.hip), built on the host: DPM-Solver++ 2M in k-diffusion's variance-exploding form
// (sample_dpmpp_2m) and the second-order Adams-Bashforth step on a non-uniform sigma grid.  Host only and plain C++: nothing of HIP is included, so
// tests/sampler_coeffs_walk.cpp links this file alone.  Everything is double precision, each coefficient rounded to float once; this file is
// compiled without FMA contraction (Makefile), so the Python restatement of the tests computes the same doubles.
#include <cmath>
#include <string>

#include "../../include/mxdenoise.h"

#pragma STDC FP_CONTRACT OFF

namespace mx {
void set_error(const std::string& msg);   // capi.cpp (the walk brings its own)
}  // namespace mx

extern "C" int mx_sampler_coeffs(int sampler, int flow, const float* sigmas, int n_steps, float* out) {
  if (!sigmas || !out) { mx::set_error("sampler_coeffs: null table"); return 1; }
  if (n_steps < 1) { mx::set_error("sampler_coeffs: n_steps must be at least 1"); return 1; }
  if (sampler == MX_SAMPLER_EULER) { mx::set_error("sampler_coeffs: the Euler step has no coefficients (its rows are kind 0 of the step launch)"); return 1; }
  if (sampler != MX_SAMPLER_DPMPP_2M && sampler != MX_SAMPLER_AB2) { mx::set_error("sampler_coeffs: unknown sampler"); return 1; }
  if (sampler == MX_SAMPLER_DPMPP_2M && flow) {
    mx::set_error("sampler_coeffs: DPM-Solver++ 2M is refused for the flow model: its log-SNR is -infinity at sigma = 1 and on the analytic Gaussian "
                  "problem it is worse than Euler at 10, 20 and 40 steps (0.59 / 0.36 / 0.12 against 0.285 / 0.143 / 0.072); use AB2");
    return 1;
  }
  for (int i = 0; i <= n_steps; ++i) {
    if (!(sigmas[i] >= 0.0f)) { mx::set_error("sampler_coeffs: sigmas must not be negative (or NaN)"); return 1; }
    if (i > 0 && !(sigmas[i] < sigmas[i - 1])) { mx::set_error("sampler_coeffs: sigmas must be strictly decreasing"); return 1; }
  }
  if (!std::isfinite(sigmas[0])) { mx::set_error("sampler_coeffs: sigmas must be finite"); return 1; }
  for (int i = 0; i < n_steps; ++i) {
    const double s = sigmas[i], sn = sigmas[i + 1];
    double cx, c0_first, c0_second, c1;
    if (sampler == MX_SAMPLER_DPMPP_2M) {
      if (sn == 0.0) {                                   // the last step to sigma 0: the data prediction itself, first order whatever came before
        cx = 0.0; c0_first = c0_second = 1.0; c1 = 0.0;
      } else {
        const double lam = -std::log(s), lam_next = -std::log(sn);
        const double h = lam_next - lam;
        const double E = -std::expm1(-h);
        cx = sn / s;
        c0_first = c0_second = E;
        c1 = 0.0;
        if (i > 0) {
          const double r = (lam - (-std::log((double)sigmas[i - 1]))) / h;
          c0_second = E * (1.0 + 1.0 / (2.0 * r));
          c1 = -E / (2.0 * r);
        }
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
    float* o = out + 4 * (long)i;
    o[0] = (float)cx; o[1] = (float)c0_first; o[2] = (float)c0_second; o[3] = (float)c1;
  }
  return 0;
}
