// pil_resize.cpp -- the host side of the Pillow resize filters: the CPU
// statement of their arithmetic (mxd_pil_resize_u8) in plain C++, over the
// tables taps.cpp builds.  The kernel is pil_resize.hip's.
#include "capi_internal.h"

static_assert(mxd::kPilPrecisionShift == mxd::kPilPrecisionBits, "the kernel shifts by the tables' fraction bits");

namespace {

inline uint8_t clip8(int32_t acc) {
  const int32_t v = acc >> mxd::kPilPrecisionBits;  // arithmetic shift, as Pillow's
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

}  // namespace

// Pillow's ImagingResample for 8 bits per channel: the horizontal pass over
// the source rows the window's vertical taps reach, rounded and clamped to
// bytes, then the vertical pass over those bytes.
extern "C" int mxd_pil_resize_u8(const uint8_t* src, int64_t src_stride, int32_t src_w, int32_t src_h, int32_t channels,
                                 int32_t filter, int32_t resize_w, int32_t resize_h, int32_t crop_x, int32_t crop_y,
                                 int32_t crop_w, int32_t crop_h, int32_t flip, uint8_t* dst, int64_t dst_stride) {
  using mxd::capi::fail;
  if (!src || !dst) return fail(MXD_ERR_INVALID, "mxd_pil_resize_u8: null src/dst pointer");
  if (!mxd::filter_is_pil(filter))
    return fail(MXD_ERR_INVALID, "mxd_pil_resize_u8: filter " + std::to_string(filter) + " is not a Pillow filter");
  if (channels != 1 && channels != 3)
    return fail(MXD_ERR_UNSUPPORTED, "mxd_pil_resize_u8: the Pillow filters take 1 or 3 channels");
  if (src_w <= 0 || src_h <= 0 || resize_w <= 0 || resize_h <= 0 || crop_w <= 0 || crop_h <= 0 || crop_x < 0 ||
      crop_y < 0 || crop_x + crop_w > resize_w || crop_y + crop_h > resize_h ||
      src_stride < (int64_t)src_w * channels || dst_stride < (int64_t)crop_w * channels)
    return fail(MXD_ERR_INVALID, "mxd_pil_resize_u8: invalid geometry");
  mxd::AxisTaps xt, yt;
  if (!mxd::build_axis_taps(src_w, resize_w, crop_x, crop_w, &xt, filter) ||
      !mxd::build_axis_taps(src_h, resize_h, crop_y, crop_h, &yt, filter))
    return fail(MXD_ERR_INVALID, "mxd_pil_resize_u8: invalid geometry");
  const int32_t c = channels, y_lo = yt.lo(), y_hi = yt.hi();
  // H pass: rows y_lo .. y_hi, the window's columns.
  std::vector<uint8_t> tmp((size_t)(y_hi - y_lo + 1) * crop_w * c);
  for (int32_t y = y_lo; y <= y_hi; y++) {
    const uint8_t* row = src + (int64_t)y * src_stride;
    for (int32_t x = 0; x < crop_w; x++) {
      const int32_t* k = &xt.coef[(size_t)x * xt.width];
      for (int32_t ch = 0; ch < c; ch++) {
        int32_t acc = 1 << (mxd::kPilPrecisionBits - 1);
        for (int32_t t = 0; t < xt.count[x]; t++) acc += (int32_t)row[(size_t)(xt.first[x] + t) * c + ch] * k[t];
        tmp[((size_t)(y - y_lo) * crop_w + x) * c + ch] = clip8(acc);
      }
    }
  }
  // V pass on those bytes; the flip mirrors the window's columns.
  for (int32_t y = 0; y < crop_h; y++) {
    const int32_t* k = &yt.coef[(size_t)y * yt.width];
    uint8_t* out = dst + (int64_t)y * dst_stride;
    for (int32_t x = 0; x < crop_w; x++) {
      const int32_t sx = flip ? crop_w - 1 - x : x;
      for (int32_t ch = 0; ch < c; ch++) {
        int32_t acc = 1 << (mxd::kPilPrecisionBits - 1);
        for (int32_t t = 0; t < yt.count[y]; t++)
          acc += (int32_t)tmp[((size_t)(yt.first[y] + t - y_lo) * crop_w + sx) * c + ch] * k[t];
        out[(size_t)x * c + ch] = clip8(acc);
      }
    }
  }
  return MXD_OK;
}
