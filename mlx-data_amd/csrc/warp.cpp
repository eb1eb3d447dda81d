// warp.cpp -- the per-image affine warps (mxd_warp, capi_internal.h): the CPU
// statement of the arithmetic (mxd_warp_apply_u8) in plain C++, and the
// validation of the _warp calls.  The arithmetic is Pillow's
// Image.transform(size, AFFINE, m, resample, fillcolor=fill), bit for bit
// (DESIGN.md section 2).  The device side is warp.hip; the two share no code.
// Host only.
#include "capi_internal.h"

#pragma clang fp contract(off)

namespace mxd {
namespace capi {
namespace {

int warp_check(const mxd_warp& wp, int32_t w, int32_t h, int32_t i) {
  auto at = [i](const std::string& msg) {
    return fail(MXD_ERR_INVALID, "mxd_warp: " + msg + " (image " + std::to_string(i) + ")");
  };
  if (wp.mode < MXD_WARP_NONE || wp.mode > MXD_WARP_BILINEAR) return at("unknown mode " + std::to_string(wp.mode));
  if (wp.mode == MXD_WARP_NONE) return MXD_OK;
  for (int k = 0; k < 6; k++)
    if (!std::isfinite(wp.m[k])) return at("m[" + std::to_string(k) + "] is not finite");
  // Pillow's condition for its fixed-point path, here for every mode: the four
  // corners map within +-32768, so every double-to-int conversion is in range.
  const double xs[2] = {0.0, (double)w}, ys[2] = {0.0, (double)h};
  for (int cy = 0; cy < 2; cy++)
    for (int cx = 0; cx < 2; cx++) {
      const double sx = xs[cx] * wp.m[0] + ys[cy] * wp.m[1] + wp.m[2];
      const double sy = xs[cx] * wp.m[3] + ys[cy] * wp.m[4] + wp.m[5];
      if (!(std::fabs(sx) < 32768.0 && std::fabs(sy) < 32768.0))
        return at("matrix maps a corner to a source coordinate of magnitude >= 32768");
    }
  return MXD_OK;
}

inline int floor_i(double v) { return v < 0.0 ? (int)std::floor(v) : (int)v; }
inline int coord_i(double v) { return v < 0.0 ? -1 : (int)v; }
inline int clamp_i(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

}  // namespace

int warp_validate(const mxd_image* images, const mxd_warp* warps, int32_t n) {
  if (n > 0 && !warps) return fail(MXD_ERR_INVALID, "mxd: null warps");
  for (int32_t i = 0; i < n; i++) {
    if (images && images[i].channels != 3)
      return fail(MXD_ERR_INVALID, "mxd_warp: channels must be 3 (image " + std::to_string(i) + ")");
    if (images)
      if (int rc = warp_check(warps[i], images[i].crop_w, images[i].crop_h, i)) return rc;
  }
  return MXD_OK;
}

int warp_validate_one(const mxd_warp& warp, int32_t w, int32_t h) { return warp_check(warp, w, h, 0); }

}  // namespace capi
}  // namespace mxd

using namespace mxd::capi;

extern "C" int mxd_warp_validate(const mxd_warp* warp, int32_t w, int32_t h) {
  if (!warp) return fail(MXD_ERR_INVALID, "mxd: null warps");
  if (w < 0 || h < 0) return fail(MXD_ERR_INVALID, "mxd: bad size");
  return warp_validate_one(*warp, w, h);
}

extern "C" int mxd_warp_apply_u8(const uint8_t* rgb, int32_t w, int32_t h, int64_t stride, const mxd_warp* warp,
                                 uint8_t* out, int64_t out_stride) {
  if (int rc = mxd_warp_validate(warp, w, h)) return rc;
  if (w > 0 && h > 0 && (!rgb || !out)) return fail(MXD_ERR_INVALID, "mxd: null pixels");
  if (w == 0 || h == 0) return MXD_OK;
  if (stride < (int64_t)w * 3 || out_stride < (int64_t)w * 3) return fail(MXD_ERR_INVALID, "mxd: stride smaller than a row");
  auto src = [&](int y, int x) { return rgb + (int64_t)y * stride + (int64_t)x * 3; };
  auto dst = [&](int y, int x) { return out + (int64_t)y * out_stride + (int64_t)x * 3; };
  if (warp->mode == MXD_WARP_NONE) {
    for (int y = 0; y < h; y++) std::memmove(dst(y, 0), src(y, 0), (size_t)w * 3);
    return MXD_OK;
  }
  // (the source is read after the fill is written: work from a copy when the two overlap)
  std::vector<uint8_t> copy;
  const uint8_t* const in_end = rgb + (int64_t)(h - 1) * stride + (int64_t)w * 3;
  const uint8_t* const out_end = out + (int64_t)(h - 1) * out_stride + (int64_t)w * 3;
  if (rgb < out_end && out < in_end) {
    copy.resize((size_t)w * 3 * h);
    for (int y = 0; y < h; y++) std::memcpy(copy.data() + (size_t)y * w * 3, src(y, 0), (size_t)w * 3);
    rgb = copy.data();
    stride = (int64_t)w * 3;
  }
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) std::memcpy(dst(y, x), warp->fill, 3);
  const double* a = warp->m;
  if (warp->mode == MXD_WARP_NEAREST && a[1] == 0.0 && a[3] == 0.0) {
    // the scale path: index tables by sequential accumulation in double
    std::vector<int> xt(w), yt(h);
    volatile double xo = a[2] + a[0] * 0.5;
    for (int x = 0; x < w; x++) {
      xt[x] = coord_i(xo);
      xo = xo + a[0];
    }
    volatile double yo = a[5] + a[4] * 0.5;
    for (int y = 0; y < h; y++) {
      yt[y] = coord_i(yo);
      yo = yo + a[4];
    }
    for (int y = 0; y < h; y++) {
      if (yt[y] < 0 || yt[y] >= h) continue;
      for (int x = 0; x < w; x++)
        if (xt[x] >= 0 && xt[x] < w) std::memcpy(dst(y, x), src(yt[y], xt[x]), 3);
    }
    return MXD_OK;
  }
  if (warp->mode == MXD_WARP_NEAREST) {
    // 16.16 fixed point
    // (Pillow's FIX in 64 bits: the same value wherever Pillow's int holds it)
    auto fix = [](double v) { return (int64_t)std::floor(v * 65536.0 + 0.5); };
    const int64_t a0 = fix(a[0]), a1 = fix(a[1]), a3 = fix(a[3]), a4 = fix(a[4]);
    const int64_t a2 = fix(a[2] + a[0] * 0.5 + a[1] * 0.5), a5 = fix(a[5] + a[3] * 0.5 + a[4] * 0.5);
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        const int64_t xin = (a2 + a1 * y + a0 * x) >> 16, yin = (a5 + a4 * y + a3 * x) >> 16;
        if (xin >= 0 && xin < w && yin >= 0 && yin < h) std::memcpy(dst(y, x), src((int)yin, (int)xin), 3);
      }
    return MXD_OK;
  }
  // BILINEAR: double, every product and sum rounded, none fused
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      volatile double t0 = a[0] * (x + 0.5), t1 = a[1] * (y + 0.5);
      volatile double t2 = t0 + t1;
      double sx = t2 + a[2];
      volatile double u0 = a[3] * (x + 0.5), u1 = a[4] * (y + 0.5);
      volatile double u2 = u0 + u1;
      double sy = u2 + a[5];
      if (sx < 0.0 || sx >= (double)w || sy < 0.0 || sy >= (double)h) continue;
      sx -= 0.5;
      sy -= 0.5;
      const int X = floor_i(sx), Y = floor_i(sy);
      const double dx = sx - X, dy = sy - Y;
      const int x0 = clamp_i(X, 0, w - 1), x1 = clamp_i(X + 1, 0, w - 1), yc = clamp_i(Y, 0, h - 1);
      const bool below = Y + 1 >= 0 && Y + 1 < h;
      for (int c = 0; c < 3; c++) {
        const double p0 = src(yc, x0)[c], p1 = src(yc, x1)[c];
        volatile double d1 = (p1 - p0) * dx;
        volatile double v1 = p0 + d1;
        double v2 = v1;
        if (below) {
          const double q0 = src(Y + 1, x0)[c], q1 = src(Y + 1, x1)[c];
          volatile double d2 = (q1 - q0) * dx;
          volatile double r2 = q0 + d2;
          v2 = r2;
        }
        volatile double d3 = (v2 - v1) * dy;
        volatile double r = v1 + d3;
        dst(y, x)[c] = (uint8_t)(int)r;
      }
    }
  return MXD_OK;
}
