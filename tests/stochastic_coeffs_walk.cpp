// The stochastic samplers' coefficient tables (sduss_amd/csrc/sampler_coeffs.cpp, mx_sampler_coeffs_eta) under AddressSanitizer + UBSan, on the CPU:
// a program of its own, built by `make -C sduss_amd/csrc stochastic_walk` from that one source file.  It builds the five-column tables of the SDXL
// schedule and of its Karras form at 1, 2, 10 and 50 steps and eta 0, 0.5, 1 and 1.5 into exactly sized arrays and checks what the step launch
// relies on: every coefficient finite; cn >= 0, and cn == 0 exactly at eta 0 and on the step to sigma 0, which is (0, 1, 1, 0, 0); c1 == 0 where
// the history must not be read; a latent equal to a constant data prediction stays there in the mean (cx + c0 + c1 == 1); the variance rule of each
// sampler (Euler ancestral: cx^2 s^2 + cn^2 == sn^2; 2M SDE: cx^2 s^2 + cn^2 == sn^2 as well, the noise level of the next sigma); eta 0 of the SDE
// sampler equal to mx_sampler_coeffs(DPMPP_2M) bit for bit; the deterministic samplers through the same entry with cn == 0; and the refusals.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/mxdenoise.h"

static std::string last_error;
namespace mx {
void set_error(const std::string& msg) { last_error = msg; }
}  // namespace mx

#define REQUIRE(cond)                                                                                                                                  \
  do {                                                                                                                                                 \
    if (!(cond)) { std::fprintf(stderr, "stochastic_coeffs_walk: %s failed at line %d (%s, %d steps, step %d, eta %g): %s\n", #cond, __LINE__, what, n, \
                                step, eta, last_error.c_str()); return 1; }                                                                            \
  } while (0)

static std::vector<float> sdxl_sigmas(int n) {
  std::vector<double> sig(1000);
  const double b0 = std::sqrt(0.00085), b1 = std::sqrt(0.012);
  double prod = 1.0;
  for (int i = 0; i < 1000; ++i) {
    const double b = b0 + (b1 - b0) * i / 999.0;
    prod *= 1.0 - b * b;
    sig[i] = std::sqrt((1.0 - prod) / prod);
  }
  std::vector<float> out;
  for (int i = n - 1; i >= 0; --i) out.push_back((float)sig[i * (1000 / n) + 1]);
  out.push_back(0.0f);
  return out;
}

static std::vector<float> karras_sigmas(int n) {
  const std::vector<float> base = sdxl_sigmas(n);
  const double hi = std::pow((double)base[0], 1.0 / 7.0), lo = std::pow((double)base[n - 1], 1.0 / 7.0);
  std::vector<float> out;
  for (int i = 0; i < n; ++i) out.push_back((float)std::pow(n == 1 ? hi : hi + (double)i / (n - 1) * (lo - hi), 7.0));
  out.push_back(0.0f);
  return out;
}

static int walk(const char* what, int sampler, const std::vector<float>& sig, double eta) {
  const int n = (int)sig.size() - 1;
  int step = -1;
  std::vector<float> out((size_t)n * 5), ode((size_t)n * 4);
  REQUIRE(mx_sampler_coeffs_eta(sampler, 0, sig.data(), n, eta, out.data()) == 0);
  REQUIRE(mx_sampler_coeffs(MX_SAMPLER_DPMPP_2M, 0, sig.data(), n, ode.data()) == 0);
  for (step = 0; step < n; ++step) {
    const float* o = &out[(size_t)step * 5];
    const double s = sig[step], sn = sig[step + 1];
    for (int j = 0; j < 5; ++j) REQUIRE(std::isfinite(o[j]));
    REQUIRE(o[4] >= 0.0f && (o[4] == 0.0f) == (eta == 0.0 || sn == 0.0));
    if (sn == 0.0) REQUIRE(o[0] == 0.0f && o[1] == 1.0f && o[2] == 1.0f && o[3] == 0.0f);
    const bool first_only = step == 0 || sn == 0.0 || sampler == MX_SAMPLER_EULER_A;
    if (first_only) REQUIRE(o[3] == 0.0f && o[2] == o[1]);
    else REQUIRE(o[3] != 0.0f);
    REQUIRE(std::fabs((double)o[0] + (double)o[1] - 1.0) <= 1e-6 && std::fabs((double)o[0] + (double)o[2] + (double)o[3] - 1.0) <= 1e-6);
    REQUIRE(std::fabs((double)o[0] * o[0] * s * s + (double)o[4] * o[4] - sn * sn) <= 1e-5 * s * s);
    REQUIRE(o[0] >= 0.0f && o[1] > 0.0f && (double)o[0] <= sn / s + 1e-6);
    if (sampler == MX_SAMPLER_DPMPP_2M_SDE && eta == 0.0) REQUIRE(std::memcmp(o, &ode[(size_t)step * 4], 4 * sizeof(float)) == 0);
  }
  return 0;
}

int main() {
  int tables = 0;
  for (int n : {1, 2, 10, 50})
    for (double eta : {0.0, 0.5, 1.0, 1.5}) {
      if (walk("sdxl euler_a", MX_SAMPLER_EULER_A, sdxl_sigmas(n), eta)) return 1;
      if (walk("karras euler_a", MX_SAMPLER_EULER_A, karras_sigmas(n), eta)) return 1;
      if (walk("sdxl dpmpp_2m_sde", MX_SAMPLER_DPMPP_2M_SDE, sdxl_sigmas(n), eta)) return 1;
      if (walk("karras dpmpp_2m_sde", MX_SAMPLER_DPMPP_2M_SDE, karras_sigmas(n), eta)) return 1;
      tables += 4;
    }
  {
    const char* what = "the deterministic samplers and the refusals";
    const int n = 2, step = -1;
    const double eta = 1.0;
    const std::vector<float> good = {2.0f, 1.0f, 0.0f};
    std::vector<float> out(10), four(8);
    for (int sampler : {MX_SAMPLER_DPMPP_2M, MX_SAMPLER_AB2}) {
      REQUIRE(mx_sampler_coeffs_eta(sampler, 0, good.data(), n, eta, out.data()) == 0 && mx_sampler_coeffs(sampler, 0, good.data(), n, four.data()) == 0);
      for (int i = 0; i < n; ++i) REQUIRE(std::memcmp(&out[5 * i], &four[4 * i], 4 * sizeof(float)) == 0 && out[5 * i + 4] == 0.0f);
    }
    for (int sampler : {MX_SAMPLER_EULER_A, MX_SAMPLER_DPMPP_2M_SDE}) {
      REQUIRE(mx_sampler_coeffs_eta(sampler, 1, good.data(), n, eta, out.data()) != 0 && last_error.find("flow") != std::string::npos);
      REQUIRE(mx_sampler_coeffs_eta(sampler, 0, good.data(), n, -0.5, out.data()) != 0 && last_error.find("eta") != std::string::npos);
      REQUIRE(mx_sampler_coeffs_eta(sampler, 0, good.data(), n, std::nan(""), out.data()) != 0 && last_error.find("eta") != std::string::npos);
      REQUIRE(mx_sampler_coeffs_eta(sampler, 0, nullptr, n, eta, out.data()) != 0 && mx_sampler_coeffs_eta(sampler, 0, good.data(), n, eta, nullptr) != 0);
      REQUIRE(mx_sampler_coeffs_eta(sampler, 0, good.data(), 0, eta, out.data()) != 0);
      REQUIRE(mx_sampler_coeffs(sampler, 0, good.data(), n, four.data()) != 0 && last_error.find("unknown sampler") != std::string::npos);
      const std::vector<float> flat = {2.0f, 2.0f, 0.0f}, rising = {1.0f, 2.0f, 0.0f}, negative = {2.0f, 1.0f, -1.0f};
      for (const auto* bad : {&flat, &rising, &negative}) REQUIRE(mx_sampler_coeffs_eta(sampler, 0, bad->data(), n, eta, out.data()) != 0);
    }
    REQUIRE(mx_sampler_coeffs_eta(MX_SAMPLER_EULER, 0, good.data(), n, eta, out.data()) != 0 && mx_sampler_coeffs_eta(5, 0, good.data(), n, eta, out.data()) != 0);
  }
  std::printf("STOCHASTIC_COEFFS_WALK_OK %d tables\n", tables);
  return 0;
}
