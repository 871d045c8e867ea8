// The host arithmetic of inpainting only the masked region (inpaint_overlay.hip): the box parameters of Pillow's GaussianBlur
// (src/libImaging/BoxBlur.c: _gaussian_blur_radius and the ww / fw of one box pass) and diffusers' crop rule
// (VaeImageProcessor.get_crop_region after the bounding box), restated.  Host only and plain C++, as resize_coeffs.cpp: nothing of HIP is included.
// The blur parameters are single precision, the crop ratios double, each in the order the originals evaluate them; this file is compiled
// without FMA contraction (Makefile), which would change `l (l + 1) - 3 sigma2` and `(y2 - y1) ratio - (x2 - x1)`.
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mxdenoise.h"

#pragma STDC FP_CONTRACT OFF

namespace mx {
void set_error(const std::string& msg);   // capi.cpp
}  // namespace mx

#define REGION_CHECK(cond, msg)                       \
  do {                                                \
    if (!(cond)) { mx::set_error(msg); return 1; }    \
  } while (0)

extern "C" int mx_blur_box_params(float radius, int* r, uint32_t* ww, uint32_t* fw) {
  REGION_CHECK(r && ww && fw, "blur_box_params: null result");
  REGION_CHECK(radius > 0.0f && radius <= (float)MX_BLUR_MAX_RADIUS, "blur_box_params: the radius must be positive and at most MX_BLUR_MAX_RADIUS");
  // three passes: the box whose threefold convolution has the variance radius^2 (Gwosdek et al., Pillow's reference)
  const float sigma2 = radius * radius / 3.0f;
  const float L = std::sqrt(12.0f * sigma2 + 1.0f);
  const float l = std::floor((L - 1.0f) / 2.0f);
  const float a = (2.0f * l + 1.0f) * (l * (l + 1.0f) - 3.0f * sigma2) / (6.0f * (sigma2 - (l + 1.0f) * (l + 1.0f)));
  const float fr = l + a;
  const int ri = (int)fr;
  const uint32_t w = (uint32_t)((float)(1 << 24) / (fr * 2.0f + 1.0f));
  // (2 ri + 1) w <= 2^24 because 2 ri + 1 <= 2 fr + 1; checked, not assumed: fw is an unsigned weight on the device
  REGION_CHECK(ri >= 0 && (uint64_t)(2 * ri + 1) * w <= (1u << 24), "blur_box_params: the box weights do not fit 24 bits");
  *r = ri;
  *ww = w;
  *fw = ((1u << 24) - (uint32_t)(2 * ri + 1) * w) / 2u;
  return 0;
}

extern "C" int mx_crop_region(int x1, int y1, int x2, int y2, int mask_w, int mask_h, int width, int height, int pad, int32_t* out) {
  REGION_CHECK(out, "crop_region: null result");
  REGION_CHECK(mask_w > 0 && mask_h > 0 && width > 0 && height > 0, "crop_region: sizes must be positive");
  REGION_CHECK(pad >= 0 && pad <= MX_RESIZE_MAX_SIZE, "crop_region: pad must not be negative");
  REGION_CHECK(x2 > x1 && y2 > y1, "crop_region: the box is empty (an empty mask has no region)");
  REGION_CHECK(x1 >= 0 && y1 >= 0 && x2 <= mask_w && y2 <= mask_h, "crop_region: the box must lie inside the mask");
  // 2. pad, clipped to the mask
  x1 = x1 - pad > 0 ? x1 - pad : 0;
  y1 = y1 - pad > 0 ? y1 - pad : 0;
  x2 = (int64_t)x2 + pad < mask_w ? x2 + pad : mask_w;
  y2 = (int64_t)y2 + pad < mask_h ? y2 + pad : mask_h;
  // 3. grow the short side to the aspect of the image to be processed
  const double ratio_crop = (double)(x2 - x1) / (double)(y2 - y1);
  const double ratio_proc = (double)width / (double)height;
  if (ratio_crop > ratio_proc) {
    const double desired = (double)(x2 - x1) / ratio_proc;
    const double d = desired - (double)(y2 - y1);
    REGION_CHECK(d < 2147483647.0, "crop_region: the grown box does not fit an int");
    const int diff = (int)d;                               // Python's int(): towards zero
    y1 -= diff / 2;
    y2 += diff - diff / 2;
    if (y2 >= mask_h) { const int over = y2 - mask_h; y2 -= over; y1 -= over; }
    if (y1 < 0) { y2 -= y1; y1 = 0; }
    if (y2 >= mask_h) y2 = mask_h;
  } else {
    const double desired = (double)(y2 - y1) * ratio_proc;
    const double d = desired - (double)(x2 - x1);
    REGION_CHECK(d < 2147483647.0, "crop_region: the grown box does not fit an int");
    const int diff = (int)d;
    x1 -= diff / 2;
    x2 += diff - diff / 2;
    if (x2 >= mask_w) { const int over = x2 - mask_w; x2 -= over; x1 -= over; }
    if (x1 < 0) { x2 -= x1; x1 = 0; }
    if (x2 >= mask_w) x2 = mask_w;
  }
  out[0] = x1; out[1] = y1; out[2] = x2; out[3] = y2;
  return 0;
}
