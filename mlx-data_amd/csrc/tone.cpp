// tone.cpp -- the per-image tone operations (mxd_tone, capi_internal.h): the
// CPU statement of the tables (mxd_tone_table_u8, mxd_tone_apply_u8) in plain
// C++, and the validation of the _tone calls.  The device side is
// row_stage.hip; the two share no code.  Host only.
#include "capi_internal.h"

namespace mxd {
namespace capi {
namespace {

int tone_check(const mxd_tone& t, int32_t i) {
  auto at = [i](const std::string& msg) {
    return fail(MXD_ERR_INVALID, "mxd_tone: " + msg + " (image " + std::to_string(i) + ")");
  };
  if (t.op < MXD_TONE_NONE || t.op > MXD_TONE_CONTRAST) return at("unknown op " + std::to_string(t.op));
  if (t.reserved != 0) return at("reserved must be 0");
  if (t.op == MXD_TONE_POSTERIZE && (t.arg < 1 || t.arg > 8)) return at("arg (posterize bits) must be in 1..8");
  if (t.op == MXD_TONE_SOLARIZE && (t.arg < 0 || t.arg > 256)) return at("arg (solarize threshold) must be in 0..256");
  if (t.op == MXD_TONE_CONTRAST && !(std::isfinite(t.factor) && t.factor >= 0.0f && t.factor <= 1e6f))
    return at("factor (contrast) must be finite and in 0..1e6");
  return MXD_OK;
}

}  // namespace

int tone_validate(const mxd_image* images, const mxd_tone* tones, int32_t n) {
  if (n > 0 && !tones) return fail(MXD_ERR_INVALID, "mxd: null tones");
  for (int32_t i = 0; i < n; i++) {
    if (images && images[i].channels != 3)
      return fail(MXD_ERR_INVALID, "mxd_tone: channels must be 3 (image " + std::to_string(i) + ")");
    if (int rc = tone_check(tones[i], i)) return rc;
  }
  return MXD_OK;
}

}  // namespace capi
}  // namespace mxd

using namespace mxd::capi;

extern "C" int mxd_tone_table_u8(const uint8_t* rgb, int64_t npixels, const mxd_tone* tone, uint8_t table[768]) {
  if (!table) return fail(MXD_ERR_INVALID, "mxd: null table");
  if (npixels < 0 || (npixels > 0 && !rgb)) return fail(MXD_ERR_INVALID, "mxd: null pixels");
  if (int rc = tone_validate(nullptr, tone, 1)) return rc;
  for (int c = 0; c < 3; c++)
    for (int v = 0; v < 256; v++) table[256 * c + v] = (uint8_t)v;
  const int op = tone->op;
  if (op == MXD_TONE_POSTERIZE) {
    const int mask = (0xff << (8 - tone->arg)) & 0xff;
    for (int k = 0; k < 768; k++) table[k] = (uint8_t)((k & 255) & mask);
    return MXD_OK;
  }
  if (op == MXD_TONE_SOLARIZE) {
    for (int k = 0; k < 768; k++) table[k] = (uint8_t)((k & 255) < tone->arg ? (k & 255) : 255 - (k & 255));
    return MXD_OK;
  }
  if (op == MXD_TONE_NONE || npixels == 0) return MXD_OK;
  if (op == MXD_TONE_CONTRAST) {
    int64_t sum = 0;
    for (int64_t i = 0; i < npixels; i++) {
      const uint32_t q0 = rgb[3 * i], q1 = rgb[3 * i + 1], q2 = rgb[3 * i + 2];
      sum += (19595u * q0 + 38470u * q1 + 7471u * q2 + 32768u) >> 16;
    }
    volatile double mean = (double)sum / (double)npixels;
    const int m = (int)(mean + 0.5);
    const float f = tone->factor;
    for (int v = 0; v < 256; v++) {
      // each operation a float32 operation, correctly rounded (volatile: none
      // is contracted or carried in a wider type)
      volatile float d = (float)(v - m);
      volatile float fd = f * d;
      volatile float x = (float)m + fd;
      const float y = x;
      uint8_t b;
      if (f >= 0.0f && f <= 1.0f) b = (uint8_t)(int)y;
      else b = y <= 0.0f ? 0 : y >= 255.0f ? 255 : (uint8_t)(int)y;
      table[v] = table[256 + v] = table[512 + v] = b;
    }
    return MXD_OK;
  }
  for (int c = 0; c < 3; c++) {
    std::vector<int64_t> hist(256, 0);
    for (int64_t i = 0; i < npixels; i++) hist[rgb[3 * i + c]]++;
    int lo = 256, hi = -1, bins = 0;
    for (int v = 0; v < 256; v++)
      if (hist[v]) {
        lo = std::min(lo, v);
        hi = v;
        bins++;
      }
    uint8_t* t = table + 256 * c;
    if (op == MXD_TONE_AUTOCONTRAST) {
      if (hi <= lo) continue;
      volatile double scale = 255.0 / (double)(hi - lo);
      volatile double offset = (double)(-lo) * scale;
      for (int v = 0; v < 256; v++) {
        volatile double prod = (double)v * scale;
        volatile double x = prod + offset;
        const int ix = (int)x;
        t[v] = (uint8_t)(ix < 0 ? 0 : ix > 255 ? 255 : ix);
      }
    } else {  // MXD_TONE_EQUALIZE
      if (bins <= 1) continue;
      const int64_t step = (npixels - hist[hi]) / 255;
      if (step == 0) continue;
      int64_t acc = step / 2;
      for (int v = 0; v < 256; v++) {
        t[v] = (uint8_t)std::min<int64_t>(255, acc / step);
        acc += hist[v];
      }
    }
  }
  return MXD_OK;
}

extern "C" int mxd_tone_apply_u8(const uint8_t* rgb, int64_t npixels, const mxd_tone* tone, uint8_t* out) {
  if (npixels < 0 || (npixels > 0 && (!rgb || !out))) return fail(MXD_ERR_INVALID, "mxd: null pixels");
  uint8_t table[768];
  if (int rc = mxd_tone_table_u8(rgb, npixels, tone, table)) return rc;
  for (int64_t i = 0; i < npixels; i++)
    for (int c = 0; c < 3; c++) out[3 * i + c] = table[256 * c + rgb[3 * i + c]];
  return MXD_OK;
}
