// The multistep samplers' coefficient tables (sduss_amd/csrc/sampler_coeffs.cpp) under AddressSanitizer + UBSan, on the CPU: a program of its own,
// built by `make -C sduss_amd/csrc sampler_walk` from that one source file.  It builds the tables of the SDXL schedule (scaled-linear betas, leading
// spacing), of its Karras form (rho 7) and of the flow-match schedule (shift 3) at 1, 2, 10 and 50 steps into exactly sized arrays and checks what
// the step launch relies on: every coefficient finite, c1 == 0 exactly on the rows that must not read the history (step 0; DPM-Solver++'s step to
// sigma 0, which is (0, 1, 1, 0)), a constant D reproduced in both orders (DPM-Solver++: cx == sn / s and c0 + c1 == 1 - sn / s, so a latent equal to
// a constant data prediction stays there; AB2: cx == 1 and c0 + c1 == sn - s), and the refusals.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../include/mxdenoise.h"

static std::string last_error;
namespace mx {
void set_error(const std::string& msg) { last_error = msg; }
}  // namespace mx

#define REQUIRE(cond)                                                                                                                             \
  do {                                                                                                                                            \
    if (!(cond)) { std::fprintf(stderr, "sampler_coeffs_walk: %s failed at line %d (%s, %d steps, step %d): %s\n", #cond, __LINE__, what, n, step, \
                                last_error.c_str()); return 1; }                                                                                  \
  } while (0)

// the 1000 training sigmas of the SDXL scheduler config, ascending
static std::vector<double> train_sigmas() {
  std::vector<double> sig(1000);
  const double b0 = std::sqrt(0.00085), b1 = std::sqrt(0.012);
  double prod = 1.0;
  for (int i = 0; i < 1000; ++i) {
    const double b = b0 + (b1 - b0) * i / 999.0;
    prod *= 1.0 - b * b;
    sig[i] = std::sqrt((1.0 - prod) / prod);
  }
  return sig;
}

static std::vector<float> sdxl_sigmas(int n) {
  const std::vector<double> sig = train_sigmas();
  std::vector<float> out;
  for (int i = n - 1; i >= 0; --i) out.push_back((float)sig[i * (1000 / n) + 1]);     // 'leading' spacing, steps_offset 1
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

static std::vector<float> flow_sigmas(int n) {
  std::vector<float> out;
  for (int i = 0; i < n; ++i) {
    const double t = n == 1 ? 1.0 : 1.0 + (double)i / (n - 1) * (0.001 - 1.0);
    out.push_back((float)(3.0 * t / (1.0 + 2.0 * t)));
  }
  out.push_back(0.0f);
  return out;
}

static int walk(const char* what, int sampler, int flow, const std::vector<float>& sig) {
  const int n = (int)sig.size() - 1;
  int step = -1;
  std::vector<float> out((size_t)n * 4);
  REQUIRE(mx_sampler_coeffs(sampler, flow, sig.data(), n, out.data()) == 0);
  for (step = 0; step < n; ++step) {
    const float* o = &out[(size_t)step * 4];
    const double s = sig[step], sn = sig[step + 1];
    for (int j = 0; j < 4; ++j) REQUIRE(std::isfinite(o[j]));
    const bool first_only = step == 0 || (sampler == MX_SAMPLER_DPMPP_2M && sn == 0.0);
    if (first_only) REQUIRE(o[3] == 0.0f && o[2] == o[1]);
    else REQUIRE(o[3] != 0.0f);
    if (sampler == MX_SAMPLER_DPMPP_2M) {
      if (sn == 0.0) REQUIRE(o[0] == 0.0f && o[1] == 1.0f && o[2] == 1.0f && o[3] == 0.0f);
      REQUIRE(std::fabs((double)o[0] - sn / s) <= 1e-6);
      REQUIRE(std::fabs((double)o[1] - (1.0 - sn / s)) <= 1e-6 && std::fabs((double)o[2] + (double)o[3] - (1.0 - sn / s)) <= 1e-6);
      REQUIRE(std::fabs((double)o[0] + (double)o[2] + (double)o[3] - 1.0) <= 1e-6);      // a latent equal to a constant data prediction stays
      REQUIRE(o[1] > 0.0f && o[2] >= o[1] && o[3] <= 0.0f);
    } else {
      REQUIRE(o[0] == 1.0f && o[1] == (float)(sn - s));
      REQUIRE(std::fabs((double)o[2] + (double)o[3] - (sn - s)) <= 1e-6 * s);             // a constant derivative is integrated exactly
      REQUIRE(o[1] < 0.0f && o[2] <= o[1] && o[3] >= 0.0f);
    }
  }
  return 0;
}

int main() {
  int tables = 0;
  for (int n : {1, 2, 10, 50}) {
    if (walk("sdxl dpmpp_2m", MX_SAMPLER_DPMPP_2M, 0, sdxl_sigmas(n))) return 1;
    if (walk("karras dpmpp_2m", MX_SAMPLER_DPMPP_2M, 0, karras_sigmas(n))) return 1;
    if (walk("sdxl ab2", MX_SAMPLER_AB2, 0, sdxl_sigmas(n))) return 1;
    if (walk("karras ab2", MX_SAMPLER_AB2, 0, karras_sigmas(n))) return 1;
    if (walk("flow ab2", MX_SAMPLER_AB2, 1, flow_sigmas(n))) return 1;
    tables += 5;
  }
  {
    const char* what = "refusals";
    const int n = 2, step = -1;
    const std::vector<float> good = {2.0f, 1.0f, 0.0f};
    std::vector<float> out(8);
    REQUIRE(mx_sampler_coeffs(MX_SAMPLER_DPMPP_2M, 1, good.data(), n, out.data()) != 0 && last_error.find("flow") != std::string::npos);
    REQUIRE(mx_sampler_coeffs(MX_SAMPLER_EULER, 0, good.data(), n, out.data()) != 0 && mx_sampler_coeffs(3, 0, good.data(), n, out.data()) != 0);
    REQUIRE(mx_sampler_coeffs(-1, 0, good.data(), n, out.data()) != 0 && mx_sampler_coeffs(MX_SAMPLER_AB2, 0, good.data(), 0, out.data()) != 0);
    REQUIRE(mx_sampler_coeffs(MX_SAMPLER_AB2, 0, nullptr, n, out.data()) != 0 && mx_sampler_coeffs(MX_SAMPLER_AB2, 0, good.data(), n, nullptr) != 0);
    const std::vector<float> flat = {2.0f, 2.0f, 0.0f}, rising = {1.0f, 2.0f, 0.0f}, negative = {2.0f, 1.0f, -1.0f}, two_zeros = {1.0f, 0.0f, 0.0f};
    for (const auto* bad : {&flat, &rising, &negative, &two_zeros})
      for (int sampler : {MX_SAMPLER_DPMPP_2M, MX_SAMPLER_AB2}) REQUIRE(mx_sampler_coeffs(sampler, 0, bad->data(), n, out.data()) != 0);
  }
  std::printf("SAMPLER_COEFFS_WALK_OK %d tables\n", tables);
  return 0;
}
