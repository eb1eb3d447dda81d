// color.cpp -- the per-image colour transform (mxd_color, capi_internal.h):
// the twist matrix (brightness, contrast, saturation, hue), the CPU statement
// of the map on result bytes, and the validation of the _color calls.  The
// device side is row_stage.hip.  Host only.
#include "capi_internal.h"

namespace mxd {
namespace capi {
namespace {

using M3 = std::array<std::array<double, 3>, 3>;
// A 3 x 4 affine map [A | t] of a column vector [r g b 1].
struct Affine {
  M3 a{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}};
  std::array<double, 3> t{0, 0, 0};
};

M3 mul(const M3& x, const M3& y) {
  M3 r{};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r[i][j] = x[i][0] * y[0][j] + x[i][1] * y[1][j] + x[i][2] * y[2][j];
  return r;
}

// x after y.
Affine after(const Affine& x, const Affine& y) {
  Affine r;
  r.a = mul(x.a, y.a);
  for (int i = 0; i < 3; i++) r.t[i] = x.a[i][0] * y.t[0] + x.a[i][1] * y.t[1] + x.a[i][2] * y.t[2] + x.t[i];
  return r;
}

// Inverse by cofactors (the YIQ matrix is far from singular).
M3 inverse(const M3& m) {
  M3 c{};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      c[j][i] = m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];  // adjugate: transposed cofactors
    }
  const double det = m[0][0] * c[0][0] + m[0][1] * c[1][0] + m[0][2] * c[2][0];
  for (auto& row : c)
    for (double& v : row) v /= det;
  return c;
}

const M3 kYiq{{{0.299, 0.587, 0.114}, {0.595716, -0.274453, -0.321263}, {0.211456, -0.522591, 0.311135}}};

// The one encode of the project: (uint8) trunc(clamp(v + 0.5f, 0, 255)).
uint8_t encode(float v) {
  volatile float x = v + 0.5f;
  float y = x;
  y = y < 0.0f ? 0.0f : y > 255.0f ? 255.0f : y;
  return (uint8_t)y;
}

}  // namespace

float color_entry(float m) { return std::fabs(m) < 0x1p-100f ? 0.0f : m; }

int color_validate(const mxd_image* images, const mxd_color* colors, int32_t n) {
  if (n > 0 && !colors) return fail(MXD_ERR_INVALID, "mxd: null colors");
  for (int32_t i = 0; i < n; i++) {
    if (images && images[i].channels != 3)
      return fail(MXD_ERR_INVALID, "mxd_color: channels must be 3 (image " + std::to_string(i) + ")");
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 4; k++) {
        const float v = colors[i].m[r][k];
        if (!std::isfinite(v) || std::fabs(v) > 1e6f)
          return fail(MXD_ERR_INVALID, "mxd_color: m[" + std::to_string(r) + "][" + std::to_string(k) +
                                           "] is not finite or larger than 1e6 (image " + std::to_string(i) + ")");
      }
  }
  return MXD_OK;
}

}  // namespace capi
}  // namespace mxd

using namespace mxd::capi;

extern "C" int mxd_color_twist_matrix(double brightness, double contrast, double saturation, double hue_degrees,
                                      mxd_color* out) {
  if (!out) return fail(MXD_ERR_INVALID, "mxd: null output");
  const double f[3] = {brightness, contrast, saturation};
  const char* names[3] = {"brightness", "contrast", "saturation"};
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(f[k]) || f[k] < 0.0)
      return fail(MXD_ERR_INVALID, std::string("mxd_color_twist_matrix: ") + names[k] + " must be finite and >= 0");
  if (!std::isfinite(hue_degrees)) return fail(MXD_ERR_INVALID, "mxd_color_twist_matrix: hue must be finite");
  // M = B . C . S . H: hue first, brightness last; a default factor adds no matrix.
  Affine m;
  if (hue_degrees != 0.0) {
    const double a = hue_degrees * 3.14159265358979323846 / 180.0, cs = std::cos(a), sn = std::sin(a);
    const M3 rot{{{1, 0, 0}, {0, cs, -sn}, {0, sn, cs}}};
    Affine h;
    h.a = mul(inverse(kYiq), mul(rot, kYiq));
    m = after(h, m);
  }
  if (saturation != 1.0) {
    Affine s;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) s.a[i][j] = (i == j ? saturation : 0.0) + (1.0 - saturation) * kYiq[0][j];
    m = after(s, m);
  }
  if (contrast != 1.0) {
    Affine c;
    for (int i = 0; i < 3; i++) c.a[i][i] = contrast, c.t[i] = 0.5 * (1.0 - contrast);
    m = after(c, m);
  }
  if (brightness != 1.0) {
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) m.a[i][j] *= brightness;
      m.t[i] *= brightness;
    }
  }
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) out->m[i][j] = (float)m.a[i][j];
    out->m[i][3] = (float)(m.t[i] * 255.0);
  }
  return MXD_OK;
}

extern "C" int mxd_color_apply_u8(const uint8_t* rgb, int64_t npixels, const mxd_color* color, uint8_t* out) {
  if (npixels < 0 || (npixels > 0 && (!rgb || !out))) return fail(MXD_ERR_INVALID, "mxd: null pixels");
  if (int rc = color_validate(nullptr, color, 1)) return rc;
  float m[3][4];
  for (int c = 0; c < 3; c++)
    for (int k = 0; k < 4; k++) m[c][k] = color_entry(color->m[c][k]);
  for (int64_t i = 0; i < npixels; i++) {
    const float q0 = rgb[3 * i], q1 = rgb[3 * i + 1], q2 = rgb[3 * i + 2];
    uint8_t o[3];
    for (int c = 0; c < 3; c++) {
      // each operation a float32 operation, correctly rounded (volatile: none
      // is contracted or carried in a wider type)
      volatile float a = m[c][0] * q0;
      volatile float b = m[c][1] * q1;
      volatile float ab = a + b;
      volatile float d = m[c][2] * q2;
      volatile float abd = ab + d;
      volatile float v = abd + m[c][3];
      o[c] = encode(v);
    }
    out[3 * i] = o[0], out[3 * i + 1] = o[1], out[3 * i + 2] = o[2];
  }
  return MXD_OK;
}
