// The coefficient tables of the 8-bit image resize (image_resize.hip), built on the host: Pillow's precompute_coeffs + normalize_coeffs_8bpc
// (src/libImaging/Resample.c) restated.  Host only and plain C++: nothing of HIP is included, so tests/resize_coeffs_walk.cpp links this file alone.
// The device never evaluates a filter: the host's and the device's sin may differ in the last place, and one flipped coefficient breaks bit equality
// with Pillow.  Everything is double precision in Pillow's order of operations; this file is compiled without FMA contraction (Makefile).
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mxdenoise.h"

#pragma STDC FP_CONTRACT OFF

namespace mx {
void set_error(const std::string& msg);   // capi.cpp (the walk brings its own)

static double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
static double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
static double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * 3.14159265358979323846;
  return std::sin(x) / x;
}
static double lanczos_filter(double x) { return (-3.0 <= x && x < 3.0) ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }

static bool filter_of(int filter, double (**fn)(double), double* support) {
  switch (filter) {
    case MX_RESIZE_LANCZOS: *fn = lanczos_filter; *support = 3.0; return true;
    case MX_RESIZE_BICUBIC: *fn = bicubic_filter; *support = 2.0; return true;
    case MX_RESIZE_BILINEAR: *fn = bilinear_filter; *support = 1.0; return true;
  }
  return false;
}
}  // namespace mx

extern "C" int mx_resize_coeffs(int in, int out, int filter, int32_t* bounds, int32_t* k, int cap) {
  double (*fn)(double) = nullptr;
  double fsupport = 0.0;
  if (in <= 0 || out <= 0 || in > MX_RESIZE_MAX_SIZE || out > MX_RESIZE_MAX_SIZE) { mx::set_error("resize_coeffs: sizes must be positive and at most 2^24"); return -1; }
  if (!mx::filter_of(filter, &fn, &fsupport)) { mx::set_error("resize_coeffs: unknown filter"); return -1; }
  const double scale = (double)in / out;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = fsupport * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  if (!bounds && !k) return ksize;                                    // the size query
  if (!bounds || !k) { mx::set_error("resize_coeffs: null table"); return -1; }
  if ((int64_t)out * ksize > (int64_t)cap) { mx::set_error("resize_coeffs: k holds fewer than out * ksize entries"); return -1; }
  const double ss = 1.0 / filterscale;                               // Pillow multiplies by the reciprocal
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    int32_t* row = k + (int64_t)xx * ksize;
    double ww = 0.0;
    // the weights pass through the int32 row's place twice in Pillow (double, then fixed point); here a first pass sums and a second one rounds
    for (int j = 0; j < n; ++j) ww += fn((j + xmin - center + 0.5) * ss);
    for (int j = 0; j < n; ++j) {
      double w = fn((j + xmin - center + 0.5) * ss);
      if (ww != 0.0) w /= ww;
      row[j] = w < 0 ? (int32_t)(-0.5 + w * (double)(1 << MX_RESIZE_PRECISION_BITS)) : (int32_t)(0.5 + w * (double)(1 << MX_RESIZE_PRECISION_BITS));
    }
    for (int j = n; j < ksize; ++j) row[j] = 0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
  return ksize;
}
