// The resize coefficient tables (sduss_amd/csrc/resize_coeffs.cpp) under AddressSanitizer + UBSan, on the CPU: a program of its own, built by
// `make -C sduss_amd/csrc resize_walk` from that one source file.  It builds both tables for every (in, out, filter) of the resize tests plus the
// edge sizes (in = 1, out = 1, 4096 -> 1) into exactly sized arrays and checks what the kernel relies on when it turns them into addresses:
// xmin >= 0, xmin + n <= in, 0 <= n <= ksize, xmin and xmin + n never decreasing, zero tail entries, and the refusals.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../include/mxdenoise.h"

static std::string last_error;
namespace mx {
void set_error(const std::string& msg) { last_error = msg; }
}  // namespace mx

#define REQUIRE(cond)                                                                                              \
  do {                                                                                                             \
    if (!(cond)) { std::fprintf(stderr, "resize_coeffs_walk: %s failed at line %d (in %d, out %d, filter %d): %s\n", #cond, __LINE__, in, out, \
                                filter, last_error.c_str()); return 1; }                                           \
  } while (0)

static int walk(int in, int out, int filter) {
  const int ksize = mx_resize_coeffs(in, out, filter, nullptr, nullptr, 0);
  REQUIRE(ksize >= 3 && ksize % 2 == 1);
  std::vector<int32_t> bounds((size_t)out * 2), k((size_t)out * ksize);
  REQUIRE(mx_resize_coeffs(in, out, filter, bounds.data(), k.data(), out * ksize) == ksize);
  int prev_min = 0, prev_max = 0;
  for (int x = 0; x < out; ++x) {
    const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
    REQUIRE(xmin >= 0 && n >= 0 && n <= ksize && xmin + n <= in);
    REQUIRE(xmin >= prev_min && xmin + n >= prev_max);
    prev_min = xmin; prev_max = xmin + n;
    int64_t sum = 0;
    for (int j = 0; j < ksize; ++j) {
      if (j >= n) REQUIRE(k[(size_t)x * ksize + j] == 0);
      sum += k[(size_t)x * ksize + j];
    }
    REQUIRE(n > 0 && sum > (1 << MX_RESIZE_PRECISION_BITS) - ksize && sum < (1 << MX_RESIZE_PRECISION_BITS) + ksize);   // normalised: each entry rounds by < 1
  }
  REQUIRE(mx_resize_coeffs(in, out, filter, bounds.data(), k.data(), out * ksize - 1) == -1);                          // one entry short: refused, nothing written past it
  REQUIRE(mx_resize_coeffs(in, out, filter, bounds.data(), nullptr, out * ksize) == -1);
  return 0;
}

int main() {
  const int pairs[][2] = {{37, 16}, {53, 24}, {9, 40}, {11, 44}, {64, 64}, {48, 40}, {128, 17}, {96, 96}, {7, 7}, {5, 5}, {400, 8}, {24, 24}, {20, 24},
                          {300, 200}, {33, 32}, {65, 64}, {1, 1}, {1, 7}, {7, 1}, {1, 4096}, {4096, 1}, {2, 3}, {3, 2}, {2048, 1024}, {640, 512}, {1536, 1024}};
  const int filters[] = {MX_RESIZE_LANCZOS, MX_RESIZE_BILINEAR, MX_RESIZE_BICUBIC};
  int n = 0;
  for (const auto& p : pairs)
    for (int f : filters) {
      if (walk(p[0], p[1], f)) return 1;
      ++n;
    }
  {
    const int in = 8, out = 8, filter = 0;
    REQUIRE(mx_resize_coeffs(0, 8, MX_RESIZE_LANCZOS, nullptr, nullptr, 0) == -1 && mx_resize_coeffs(8, -1, MX_RESIZE_LANCZOS, nullptr, nullptr, 0) == -1);
    REQUIRE(mx_resize_coeffs(in, out, filter, nullptr, nullptr, 0) == -1 && mx_resize_coeffs(in, out, 4, nullptr, nullptr, 0) == -1);
    REQUIRE(mx_resize_coeffs(MX_RESIZE_MAX_SIZE + 1, 8, MX_RESIZE_LANCZOS, nullptr, nullptr, 0) == -1);
  }
  std::printf("RESIZE_COEFFS_WALK_OK %d tables\n", n);
  return 0;
}
