// enhance.cpp -- the per-image enhance operations (mxd_enhance,
// capi_internal.h): the CPU statement of the arithmetic (mxd_enhance_apply_u8)
// in plain C++, and the validation of the _enhance calls.  The arithmetic is
// Pillow's ImageEnhance.Sharpness / Color / Brightness, bit for bit (DESIGN.md
// section 2).  The device side is enhance.hip; the two share no code.
// Host only.
#include "capi_internal.h"

#pragma clang fp contract(off)

namespace mxd {
namespace capi {
namespace {

int enhance_check(const mxd_enhance& e, int32_t i) {
  auto at = [i](const std::string& msg) {
    return fail(MXD_ERR_INVALID, "mxd_enhance: " + msg + " (image " + std::to_string(i) + ")");
  };
  if (e.op < MXD_ENHANCE_NONE || e.op > MXD_ENHANCE_BRIGHTNESS) return at("unknown op " + std::to_string(e.op));
  if (e.reserved[0] != 0 || e.reserved[1] != 0) return at("reserved must be 0");
  if (e.op != MXD_ENHANCE_NONE && !(std::isfinite(e.factor) && e.factor >= 0.0f && e.factor <= 1e6f))
    return at("factor must be finite and in 0..1e6");
  return MXD_OK;
}

// Image.blend(degenerate, image, f) of one byte: each operation a float32
// operation, correctly rounded (volatile: none is contracted or carried in a
// wider type).
inline uint8_t blend(int d, int q, float f) {
  volatile float diff = (float)(q - d);
  volatile float fd = f * diff;
  volatile float x = (float)d + fd;
  const float y = x;
  if (f >= 0.0f && f <= 1.0f) return (uint8_t)(int)y;
  return y <= 0.0f ? 0 : y >= 255.0f ? 255 : (uint8_t)(int)y;
}

}  // namespace

int enhance_validate(const mxd_image* images, const mxd_enhance* enhances, int32_t n) {
  if (n > 0 && !enhances) return fail(MXD_ERR_INVALID, "mxd: null enhances");
  for (int32_t i = 0; i < n; i++) {
    if (images && images[i].channels != 3)
      return fail(MXD_ERR_INVALID, "mxd_enhance: channels must be 3 (image " + std::to_string(i) + ")");
    if (int rc = enhance_check(enhances[i], i)) return rc;
  }
  return MXD_OK;
}

}  // namespace capi
}  // namespace mxd

using namespace mxd::capi;

extern "C" int mxd_enhance_validate(const mxd_enhance* enh) { return enhance_validate(nullptr, enh, 1); }

extern "C" int mxd_enhance_apply_u8(const uint8_t* rgb, int32_t w, int32_t h, int64_t stride, const mxd_enhance* enh,
                                    uint8_t* out, int64_t out_stride) {
  if (int rc = mxd_enhance_validate(enh)) return rc;
  if (w < 0 || h < 0) return fail(MXD_ERR_INVALID, "mxd: bad size");
  if (w > 0 && h > 0 && (!rgb || !out)) return fail(MXD_ERR_INVALID, "mxd: null pixels");
  if (w == 0 || h == 0) return MXD_OK;
  if (stride < (int64_t)w * 3 || out_stride < (int64_t)w * 3) return fail(MXD_ERR_INVALID, "mxd: stride smaller than a row");
  const uint8_t* const in_end = rgb + (int64_t)(h - 1) * stride + (int64_t)w * 3;
  const uint8_t* const out_end = out + (int64_t)(h - 1) * out_stride + (int64_t)w * 3;
  if (rgb < out_end && out < in_end) return fail(MXD_ERR_INVALID, "mxd_enhance: out overlaps rgb");
  auto src = [&](int y, int x) { return rgb + (int64_t)y * stride + (int64_t)x * 3; };
  auto dst = [&](int y, int x) { return out + (int64_t)y * out_stride + (int64_t)x * 3; };
  const int op = enh->op;
  const float f = enh->factor;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const uint8_t* q = src(y, x);
      uint8_t* o = dst(y, x);
      if (op == MXD_ENHANCE_NONE) {
        std::memcpy(o, q, 3);
      } else if (op == MXD_ENHANCE_BRIGHTNESS) {
        for (int c = 0; c < 3; c++) o[c] = blend(0, q[c], f);
      } else if (op == MXD_ENHANCE_COLOR) {
        const int l = (int)((19595u * q[0] + 38470u * q[1] + 7471u * q[2] + 32768u) >> 16);
        for (int c = 0; c < 3; c++) o[c] = blend(l, q[c], f);
      } else {
        const bool ring = x == 0 || y == 0 || x == w - 1 || y == h - 1;  // (every pixel when w < 3 or h < 3)
        for (int c = 0; c < 3; c++) {
          int d = q[c];
          if (!ring) {
            int s = 4 * q[c];
            for (int dy = -1; dy <= 1; dy++)
              for (int dx = -1; dx <= 1; dx++) s += src(y + dy, x + dx)[c];
            d = (2 * s + 13) / 26;
          }
          o[c] = blend(d, q[c], f);
        }
      }
    }
  return MXD_OK;
}
