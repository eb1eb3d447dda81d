// enhance.cpp -- the per-image enhance operations (mxd_enhance,
// capi_internal.h): the CPU statement of the arithmetic (mxd_enhance_apply_u8)
// in plain C++, and the validation of the _enhance calls.  The arithmetic is
// Pillow's ImageEnhance.Sharpness / Color / Brightness, bit for bit, and for
// GAUSSIAN_BLUR a separable Gaussian with torchvision's kernel and reflect
// padding, and for PIL_GAUSSIAN_BLUR / PIL_BOX_BLUR Pillow's fixed-point box
// passes, and for PIL_HUE Pillow's RGB -> HSV -> RGB round trip with the hue
// shifted.  The device side is enhance.hip, blur.hip,
// pilblur.hip and hue.hip; the two sides share no code.
// Host only.
#include "capi_internal.h"

#include <algorithm>
#include <vector>

#pragma clang fp contract(off)

namespace mxd {
namespace capi {

std::atomic<int32_t> g_blur_seg_rows{0}, g_blur_step{0};

namespace {

int enhance_check(const mxd_enhance& e, int32_t i) {
  auto at = [i](const std::string& msg) {
    return fail(MXD_ERR_INVALID, "mxd_enhance: " + msg + " (image " + std::to_string(i) + ")");
  };
  if (e.op == MXD_ENHANCE_GAUSSIAN_BLUR) {
    if (e.reserved[1] != 0) return at("reserved[1] must be 0");
    if (e.reserved[0] < 3 || e.reserved[0] > 33 || e.reserved[0] % 2 == 0)
      return at("reserved[0] (the kernel size) must be odd and in 3..33");
    if (!(std::isfinite(e.factor) && e.factor > 0.0f && e.factor <= 1e6f))
      return at("factor (sigma) must be finite, > 0 and at most 1e6");
    return MXD_OK;
  }
  if (e.op == MXD_ENHANCE_PIL_GAUSSIAN_BLUR || e.op == MXD_ENHANCE_PIL_BOX_BLUR) {
    if (e.reserved[0] != 0 || e.reserved[1] != 0) return at("reserved must be 0");
    if (!(std::isfinite(e.factor) && e.factor >= 0.0f)) return at("factor (the radius) must be finite and not negative");
    if (!(pil_blur_params(e.op, e.factor).fr < (float)mxd::kBlurMaxR))
      return at("factor (the radius) is too large: its box radius must stay below " + std::to_string(mxd::kBlurMaxR));
    return MXD_OK;
  }
  if (e.op == MXD_ENHANCE_PIL_HUE) {
    if (e.reserved[0] < 0 || e.reserved[0] > 255) return at("hue shift must be in 0..255");
    if (e.reserved[1] != 0) return at("reserved must be 0");
    if (!(e.factor == 0.0f)) return at("factor must be 0");
    return MXD_OK;
  }
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

// torch / NumPy "reflect" of index i into 0..n-1: the mirror without the edge
// repeated, period 2 (n - 1).
inline int reflect(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// GAUSSIAN_BLUR (mxd_amd.h): the H pass of every row into float32, then the V
// pass, each operation rounded on its own.
void gaussian_blur(const uint8_t* rgb, int w, int h, int64_t stride, const float* wt, int R, uint8_t* out,
                   int64_t out_stride) {
  const int n = w * 3;
  std::vector<float> hp((size_t)h * n);
  std::vector<int> xl(w * (R + 1)), xr(w * (R + 1));
  for (int x = 0; x < w; x++)
    for (int d = 0; d <= R; d++) xl[x * (R + 1) + d] = reflect(x - d, w), xr[x * (R + 1) + d] = reflect(x + d, w);
  for (int y = 0; y < h; y++) {
    const uint8_t* q = rgb + (int64_t)y * stride;
    for (int x = 0; x < w; x++)
      for (int c = 0; c < 3; c++) {
        volatile float a = wt[R] * (float)q[3 * x + c];
        for (int d = 1; d <= R; d++) {
          volatile float t = wt[R + d] * (float)((int)q[3 * xl[x * (R + 1) + d] + c] + (int)q[3 * xr[x * (R + 1) + d] + c]);
          a = a + t;
        }
        hp[(size_t)y * n + 3 * x + c] = a;
      }
  }
  for (int y = 0; y < h; y++)
    for (int i = 0; i < n; i++) {
      volatile float a = wt[R] * hp[(size_t)y * n + i];
      for (int d = 1; d <= R; d++) {
        volatile float s = hp[(size_t)reflect(y - d, h) * n + i] + hp[(size_t)reflect(y + d, h) * n + i];
        volatile float t = wt[R + d] * s;
        a = a + t;
      }
      const float r = std::nearbyint((float)a);  // half to even in the default rounding mode
      out[(int64_t)y * out_stride + i] = (uint8_t)(r <= 0.0f ? 0.0f : r >= 255.0f ? 255.0f : r);
    }
}

// One pass of Pillow's extended box blur over n bytes `step` apart.
void box_pass(const uint8_t* in, uint8_t* out, int n, int64_t step, int R, uint32_t ww, uint32_t fw) {
  auto at = [&](int i) { return (uint32_t)in[(int64_t)std::min(std::max(i, 0), n - 1) * step]; };
  for (int x = 0; x < n; x++) {
    uint32_t sum = 0;
    for (int d = -R; d <= R; d++) sum += at(x + d);
    out[(int64_t)x * step] = (uint8_t)((ww * sum + fw * (at(x - R - 1) + at(x + R + 1)) + (1u << 23)) >> 24);
  }
}

// PIL_GAUSSIAN_BLUR / PIL_BOX_BLUR (mxd_amd.h): the passes over every row,
// then over every column of the result, each on the bytes of the one before.
void pil_blur(const uint8_t* rgb, int w, int h, int64_t stride, const PilBlurParams& p, uint8_t* out, int64_t out_stride) {
  const int n = w * 3, R = (int)p.fr;
  std::vector<uint8_t> a((size_t)h * n), b((size_t)h * n);
  for (int y = 0; y < h; y++) std::memcpy(&a[(size_t)y * n], rgb + (int64_t)y * stride, n);
  for (int pass = 0; pass < 2 * p.passes && p.fr != 0.0f; pass++) {
    if (pass < p.passes) {
      for (int y = 0; y < h; y++)
        for (int c = 0; c < 3; c++) box_pass(&a[(size_t)y * n + c], &b[(size_t)y * n + c], w, 3, R, p.ww, p.fw);
    } else {
      for (int i = 0; i < n; i++) box_pass(&a[i], &b[i], h, n, R, p.ww, p.fw);
    }
    a.swap(b);
  }
  for (int y = 0; y < h; y++) std::memcpy(out + (int64_t)y * out_stride, &a[(size_t)y * n], n);
}

// PIL_HUE (mxd_amd.h) of one pixel: Pillow's rgb2hsv, the shift of H modulo
// 256, Pillow's hsv2rgb.  A float is a float32 and a double a float64; every
// operation is rounded where it stands.
inline void pil_hue(const uint8_t* q, int shift, uint8_t* o) {
  const int r = q[0], g = q[1], b = q[2];
  const int maxc = std::max(r, std::max(g, b)), minc = std::min(r, std::min(g, b));
  int H = 0, S = 0;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)std::fmod((double)h / 6.0 + 1.0, 1.0);
    H = std::min(std::max((int)((double)h * 255.0), 0), 255);
    S = std::min(std::max((int)((double)s * 255.0), 0), 255);
  }
  H = (H + shift) & 255;
  if (S == 0) {
    o[0] = o[1] = o[2] = (uint8_t)maxc;
    return;
  }
  const double hf = (double)(float)H * 6.0 / 255.0;
  const double fl = std::floor(hf);
  const float f = (float)(hf - fl);
  const float fs = (float)((double)S / 255.0);
  const float fsf = fs * f;
  const double V = (double)maxc;
  auto byte = [](double x) { return (uint8_t)std::min(std::max(std::round(x), 0.0), 255.0); };
  const uint8_t v = (uint8_t)maxc;
  const uint8_t p = byte(V * (1.0 - (double)fs));
  const uint8_t qq = byte(V * (1.0 - (double)fsf));
  const uint8_t t = byte(V * (1.0 - (double)fs * (1.0 - (double)f)));
  switch ((int)fl % 6) {
    case 0: o[0] = v, o[1] = t, o[2] = p; break;
    case 1: o[0] = qq, o[1] = v, o[2] = p; break;
    case 2: o[0] = p, o[1] = v, o[2] = t; break;
    case 3: o[0] = p, o[1] = qq, o[2] = v; break;
    case 4: o[0] = t, o[1] = p, o[2] = v; break;
    default: o[0] = v, o[1] = p, o[2] = qq; break;
  }
}

}  // namespace

// Pillow's _gaussian_blur_radius and the weights of ImagingLineBoxBlur8: all
// float32 (volatile: no operation is contracted or carried wider) but the
// square root.
PilBlurParams pil_blur_params(int32_t op, float radius) {
  PilBlurParams p{};
  p.passes = op == MXD_ENHANCE_PIL_GAUSSIAN_BLUR ? 3 : 1;
  volatile float fr = radius;
  if (op == MXD_ENHANCE_PIL_GAUSSIAN_BLUR) {
    volatile float s2 = radius * radius;
    s2 = s2 / 3.0f;
    volatile float L = (float)std::sqrt(12.0 * (double)s2 + 1.0);
    volatile float l = std::floor((L - 1.0f) / 2.0f);
    volatile float t = l * (l + 1.0f);
    volatile float u = 3.0f * s2;
    t = t - u;
    volatile float a = (2.0f * l + 1.0f) * t;
    volatile float l1 = (l + 1.0f) * (l + 1.0f);
    volatile float den = s2 - l1;
    den = 6.0f * den;
    a = a / den;
    fr = l + a;
  }
  p.fr = fr;
  if (!(p.fr >= 0.0f && p.fr < 1e6f)) return p;  // (not valid: the caller refuses it)
  volatile float span = p.fr * 2.0f;
  span = span + 1.0f;
  volatile float q = (float)(1 << 24) / span;
  p.ww = (uint32_t)q;
  p.fw = ((1u << 24) - (2u * (uint32_t)(int)p.fr + 1u) * p.ww) / 2u;
  return p;
}

int gaussian_weights(float sigma, int32_t k, float* out) {
  const int R = (k - 1) / 2;
  double p[33], sum = 0.0;
  for (int j = 0; j < k; j++) {
    const double x = (double)(j - R) / (double)sigma;
    p[j] = std::exp(-0.5 * (x * x));
    sum += p[j];
  }
  for (int j = 0; j < k; j++) {
    const float w = (float)(p[j] / sum);
    out[j] = std::fabs(w) < 0x1p-126f ? 0.0f : w;
  }
  return MXD_OK;
}

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

extern "C" int mxd_blur_shape(int32_t seg_rows, int32_t step) {
  if (seg_rows < 0 || (step != 0 && step != 4 && step != 8)) return fail(MXD_ERR_INVALID, "mxd_blur_shape: bad shape");
  g_blur_seg_rows = seg_rows;
  g_blur_step = step;
  return MXD_OK;
}

extern "C" int mxd_pil_blur_params(int32_t op, float radius, float* fr, uint32_t* ww, uint32_t* fw, int32_t* passes) {
  if (op != MXD_ENHANCE_PIL_GAUSSIAN_BLUR && op != MXD_ENHANCE_PIL_BOX_BLUR)
    return fail(MXD_ERR_INVALID, "mxd_pil_blur_params: op must be MXD_ENHANCE_PIL_GAUSSIAN_BLUR or MXD_ENHANCE_PIL_BOX_BLUR");
  const mxd_enhance e{op, radius, {0, 0}};
  if (int rc = mxd_enhance_validate(&e)) return rc;
  const PilBlurParams p = pil_blur_params(op, radius);
  if (fr) *fr = p.fr;
  if (ww) *ww = p.ww;
  if (fw) *fw = p.fw;
  if (passes) *passes = p.passes;
  return MXD_OK;
}

extern "C" int mxd_gaussian_weights(float sigma, int32_t k, float* out) {
  const mxd_enhance e{MXD_ENHANCE_GAUSSIAN_BLUR, sigma, {k, 0}};
  if (int rc = mxd_enhance_validate(&e)) return rc;
  if (!out) return fail(MXD_ERR_INVALID, "mxd: null weights");
  return gaussian_weights(sigma, k, out);
}

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
  if (op == MXD_ENHANCE_GAUSSIAN_BLUR) {
    float wt[33];
    gaussian_weights(f, enh->reserved[0], wt);
    gaussian_blur(rgb, w, h, stride, wt, (enh->reserved[0] - 1) / 2, out, out_stride);
    return MXD_OK;
  }
  if (op == MXD_ENHANCE_PIL_GAUSSIAN_BLUR || op == MXD_ENHANCE_PIL_BOX_BLUR) {
    pil_blur(rgb, w, h, stride, pil_blur_params(op, f), out, out_stride);
    return MXD_OK;
  }
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const uint8_t* q = src(y, x);
      uint8_t* o = dst(y, x);
      if (op == MXD_ENHANCE_NONE) {
        std::memcpy(o, q, 3);
      } else if (op == MXD_ENHANCE_PIL_HUE) {
        pil_hue(q, enh->reserved[0], o);
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
