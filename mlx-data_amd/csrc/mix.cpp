// mix.cpp -- MixUp and CutMix across the images of a call (mxd_mix,
// capi_internal.h): the CPU statement of the arithmetic (mxd_mix_apply_u8) in
// plain C++, and the validation of the _mix calls.  The arithmetic is timm's
// FastCollateMixup on uint8 images, that is NumPy's
//   a.astype(float32) * lam + b.astype(float32) * (1 - lam), then rint
// bit for bit.  The device side is mix.hip; the two
// share no code.  Host only.
#include "capi_internal.h"

#pragma clang fp contract(off)

namespace mxd {
namespace capi {
namespace {

int fail_at(int32_t i, const std::string& msg) {
  return fail(MXD_ERR_INVALID, "mxd_mix: " + msg + " (image " + std::to_string(i) + ")");
}

// What one entry says by itself.  w, h: the image's crop window (< 0: unknown,
// the box's upper bounds are not checked).
int mix_check(const mxd_mix& m, int32_t i, int32_t w, int32_t h) {
  if (m.op < MXD_MIX_NONE || m.op > MXD_MIX_CUTMIX) return fail_at(i, "unknown op " + std::to_string(m.op));
  if (m.reserved[0] != 0 || m.reserved[1] != 0) return fail_at(i, "reserved must be 0");
  if (m.op == MXD_MIX_MIXUP) {
    if (!(std::isfinite(m.w_self) && m.w_self >= 0.0f && m.w_self <= 1.0f))
      return fail_at(i, "w_self must be finite and in 0..1");
    if (!(std::isfinite(m.w_other) && m.w_other >= 0.0f && m.w_other <= 1.0f))
      return fail_at(i, "w_other must be finite and in 0..1");
  }
  if (m.op == MXD_MIX_CUTMIX) {
    if (!(0 <= m.x0 && m.x0 <= m.x1 && (w < 0 || m.x1 <= w)))
      return fail_at(i, "box needs 0 <= x0 <= x1 <= crop_w, got x0 " + std::to_string(m.x0) + " x1 " +
                            std::to_string(m.x1) + (w < 0 ? "" : " crop_w " + std::to_string(w)));
    if (!(0 <= m.y0 && m.y0 <= m.y1 && (h < 0 || m.y1 <= h)))
      return fail_at(i, "box needs 0 <= y0 <= y1 <= crop_h, got y0 " + std::to_string(m.y0) + " y1 " +
                            std::to_string(m.y1) + (h < 0 ? "" : " crop_h " + std::to_string(h)));
  }
  return MXD_OK;
}

// One byte of a MixUp: each operation a float32 operation, correctly rounded
// (volatile: none is contracted or carried in a wider type), then round half
// to even.
inline uint8_t mixup(uint8_t q, uint8_t r, float w_self, float w_other) {
  volatile float a = (float)q * w_self;
  volatile float b = (float)r * w_other;
  volatile float x = a + b;
  const float y = std::nearbyintf(x);  // (the default rounding mode: to nearest, ties to even)
  return (uint8_t)(y >= 255.0f ? 255 : (int)y);
}

}  // namespace

int mix_validate(const mxd_image* images, const mxd_mix* mixes, int32_t n) {
  if (n > 0 && !mixes) return fail(MXD_ERR_INVALID, "mxd: null mixes");
  for (int32_t i = 0; i < n; i++) {
    if (images && images[i].channels != 3) return fail_at(i, "channels must be 3");
    const mxd_mix& m = mixes[i];
    if (int rc = mix_check(m, i, images ? images[i].crop_w : -1, images ? images[i].crop_h : -1)) return rc;
    if (m.op == MXD_MIX_NONE) continue;
    if (m.partner < 0 || m.partner >= n)
      return fail_at(i, "partner " + std::to_string(m.partner) + " outside 0.." + std::to_string(n - 1));
    if (images && (images[m.partner].crop_w != images[i].crop_w || images[m.partner].crop_h != images[i].crop_h))
      return fail_at(i, "partner " + std::to_string(m.partner) + "'s crop size " + std::to_string(images[m.partner].crop_w) +
                            " x " + std::to_string(images[m.partner].crop_h) + " differs from " +
                            std::to_string(images[i].crop_w) + " x " + std::to_string(images[i].crop_h));
  }
  return MXD_OK;
}

}  // namespace capi
}  // namespace mxd

using namespace mxd::capi;

extern "C" int mxd_mix_validate(const mxd_image* images, const mxd_mix* mixes, int32_t n) {
  if (n < 0) return fail(MXD_ERR_INVALID, "mxd: bad image array");
  return mix_validate(images, mixes, n);
}

extern "C" int mxd_mix_apply_u8(const uint8_t* own, int64_t own_stride, const uint8_t* partner, int64_t partner_stride,
                                int32_t w, int32_t h, const mxd_mix* mix, uint8_t* out, int64_t out_stride) {
  if (!mix) return fail(MXD_ERR_INVALID, "mxd: null mixes");
  if (w < 0 || h < 0) return fail(MXD_ERR_INVALID, "mxd: bad size");
  if (int rc = mix_check(*mix, 0, w, h)) return rc;
  if (w == 0 || h == 0) return MXD_OK;
  if (!own || !out || (mix->op != MXD_MIX_NONE && !partner)) return fail(MXD_ERR_INVALID, "mxd: null pixels");
  const int64_t row = (int64_t)w * 3;
  if (own_stride < row || out_stride < row || (mix->op != MXD_MIX_NONE && partner_stride < row))
    return fail(MXD_ERR_INVALID, "mxd: stride smaller than a row");
  const int op = mix->op;
  for (int y = 0; y < h; y++) {
    const uint8_t* q = own + (int64_t)y * own_stride;
    const uint8_t* r = op == MXD_MIX_NONE ? q : partner + (int64_t)y * partner_stride;
    uint8_t* o = out + (int64_t)y * out_stride;
    if (op == MXD_MIX_MIXUP) {
      for (int64_t k = 0; k < row; k++) o[k] = mixup(q[k], r[k], mix->w_self, mix->w_other);
    } else {
      const bool in_rows = op == MXD_MIX_CUTMIX && y >= mix->y0 && y < mix->y1;
      for (int x = 0; x < w; x++) {
        const uint8_t* s = in_rows && x >= mix->x0 && x < mix->x1 ? r : q;
        for (int c = 0; c < 3; c++) o[3 * x + c] = s[3 * x + c];
      }
    }
  }
  return MXD_OK;
}
