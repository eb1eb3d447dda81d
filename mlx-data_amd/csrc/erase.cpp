// erase.cpp -- Random Erasing behind the output form (mxd_erase,
// capi_internal.h): the validation of the _erase calls, the fills as element
// bits (erase_fill, which the batch layout puts into its records) and the CPU
// statement (mxd_erase_apply) in plain C++.  The noise is erase_noise.h's, the
// header the kernel (erase.hip) includes too: both sides run the same float32
// operations, so they agree bit for bit.  Compiled with
// -ffp-contract=off.  Host only.
#include "capi_internal.h"
#include "erase_noise.h"

#pragma clang fp contract(off)

namespace mxd {
namespace capi {
namespace {

int fail_at(int32_t i, const std::string& msg) {
  return fail(MXD_ERR_INVALID, "mxd_erase: " + msg + " (image " + std::to_string(i) + ")");
}

// What one entry says by itself.  w, h: the image's crop window (< 0: unknown,
// the boxes' upper bounds are not checked).
int erase_check(const mxd_erase& e, int32_t i, int32_t w, int32_t h, int32_t elem) {
  for (int32_t r : e.reserved)
    if (r != 0) return fail_at(i, "reserved must be 0");
  if (e.count < 0 || e.count > MXD_ERASE_MAX_BOXES)
    return fail_at(i, "count " + std::to_string(e.count) + " outside 0.." + std::to_string(MXD_ERASE_MAX_BOXES));
  if (e.count == 0) return MXD_OK;
  if (e.mode < MXD_ERASE_CONST || e.mode > MXD_ERASE_PIXEL) return fail_at(i, "unknown mode " + std::to_string(e.mode));
  if (e.mode != MXD_ERASE_CONST && elem == MXD_ERASE_U8)
    return fail_at(i, "mode COLOR / PIXEL needs a float element type, the call writes u8");
  if (e.mode == MXD_ERASE_CONST)
    for (int c = 0; c < 3; c++) {
      const float v = e.value[c];
      if (!std::isfinite(v)) return fail_at(i, "value[" + std::to_string(c) + "] is not finite");
      if (elem == MXD_ERASE_U8 && !(v >= 0.0f && v <= 255.0f && v == std::floor(v)))
        return fail_at(i, "value[" + std::to_string(c) + "] must be an integer in 0..255 for u8 elements");
    }
  for (int32_t b = 0; b < e.count; b++) {
    const int32_t* bx = e.box[b];
    const std::string name = "box[" + std::to_string(b) + "]";
    if (!(0 <= bx[0] && bx[0] <= bx[2] && (w < 0 || bx[2] <= w)))
      return fail_at(i, name + " needs 0 <= x0 <= x1 <= crop_w, got x0 " + std::to_string(bx[0]) + " x1 " +
                            std::to_string(bx[2]) + (w < 0 ? "" : " crop_w " + std::to_string(w)));
    if (!(0 <= bx[1] && bx[1] <= bx[3] && (h < 0 || bx[3] <= h)))
      return fail_at(i, name + " needs 0 <= y0 <= y1 <= crop_h, got y0 " + std::to_string(bx[1]) + " y1 " +
                            std::to_string(bx[3]) + (h < 0 ? "" : " crop_h " + std::to_string(h)));
  }
  return MXD_OK;
}

void put(uint8_t* p, int32_t es, uint32_t bits) { std::memcpy(p, &bits, (size_t)es); }  // (little endian)

}  // namespace

int32_t erase_elem(const mxd_out_format* fmt, int32_t out_dtype) {
  return fmt ? fmt->elem + 1 : out_dtype == MXD_F32_DIV255 ? MXD_ERASE_F32 : MXD_ERASE_U8;
}

int erase_validate(const mxd_image* images, const mxd_erase* erases, int32_t n, int32_t elem) {
  if (n > 0 && !erases) return fail(MXD_ERR_INVALID, "mxd: null erases");
  if (elem < MXD_ERASE_U8 || elem > MXD_ERASE_BF16) return fail(MXD_ERR_INVALID, "mxd_erase: unknown elem " + std::to_string(elem));
  for (int32_t i = 0; i < n; i++) {
    if (images && images[i].channels != 3) return fail_at(i, "channels must be 3");
    if (int rc = erase_check(erases[i], i, images ? images[i].crop_w : -1, images ? images[i].crop_h : -1, elem)) return rc;
  }
  return MXD_OK;
}

void erase_fill(const mxd_erase& e, int32_t b, int32_t elem, uint32_t fill[3]) {
  float z[4] = {e.value[0], e.value[1], e.value[2], 0.0f};
  if (e.mode == MXD_ERASE_COLOR) mxd::noise::color_normals(e.seed[0], e.seed[1], (uint32_t)b, z);
  for (int c = 0; c < 3; c++)
    fill[c] = e.mode == MXD_ERASE_PIXEL ? 0u : elem == MXD_ERASE_U8 ? (uint32_t)z[c] : mxd::noise::elem_bits(z[c], elem);
}

}  // namespace capi
}  // namespace mxd

using namespace mxd::capi;

extern "C" int mxd_erase_validate(const mxd_image* images, const mxd_erase* erases, int32_t n, int32_t elem) {
  if (n < 0) return fail(MXD_ERR_INVALID, "mxd: bad image array");
  return erase_validate(images, erases, n, elem);
}

extern "C" int mxd_erase_normals(const uint32_t counter[4], const uint32_t key[2], float out[4], uint32_t* words) {
  if (!counter || !key || !out) return fail(MXD_ERR_INVALID, "mxd: null argument");
  uint32_t w[4] = {counter[0], counter[1], counter[2], counter[3]};
  mxd::noise::philox4x32_10(w, key[0], key[1]);
  if (words) std::memcpy(words, w, sizeof w);
  float z[4];
  mxd::noise::normals4(w, z);
  std::memcpy(out, z, sizeof z);
  return MXD_OK;
}

extern "C" int mxd_erase_apply(void* dst, int64_t dst_stride, int64_t plane_stride, int32_t w, int32_t h, int32_t elem,
                               int32_t layout, const mxd_erase* erase) {
  if (!erase) return fail(MXD_ERR_INVALID, "mxd: null erases");
  if (w < 0 || h < 0) return fail(MXD_ERR_INVALID, "mxd: bad size");
  if (layout != MXD_LAYOUT_HWC && layout != MXD_LAYOUT_CHW)
    return fail(MXD_ERR_INVALID, "mxd_erase: unknown layout " + std::to_string(layout));
  if (int rc = erase_validate(nullptr, erase, 1, elem)) return rc;
  if (int rc = erase_check(*erase, 0, w, h, elem)) return rc;
  if (erase->count == 0 || w == 0 || h == 0) return MXD_OK;
  if (!dst) return fail(MXD_ERR_INVALID, "mxd: null pixels");
  const bool chw = layout == MXD_LAYOUT_CHW;
  const int32_t es = elem == MXD_ERASE_U8 ? 1 : elem == MXD_ERASE_F32 ? 4 : 2;
  if (dst_stride < (int64_t)w * es * (chw ? 1 : 3)) return fail(MXD_ERR_INVALID, "mxd: stride smaller than a row");
  if (chw && plane_stride < (int64_t)h * dst_stride) return fail(MXD_ERR_INVALID, "mxd: plane_stride smaller than a plane");
  const mxd_erase& e = *erase;
  uint8_t* const base = static_cast<uint8_t*>(dst);
  // Boxes in order: a later box overwrites an earlier one, which is the rule
  // "the highest-numbered box that contains the element wins".
  for (int32_t b = 0; b < e.count; b++) {
    const int32_t* bx = e.box[b];
    uint32_t fill[3];
    erase_fill(e, b, elem, fill);
    for (int32_t y = bx[1]; y < bx[3]; y++)
      for (int32_t c = 0; c < 3; c++) {
        float z[4] = {0, 0, 0, 0};
        for (int32_t x = bx[0]; x < bx[2]; x++) {
          uint32_t bits = fill[c];
          if (e.mode == MXD_ERASE_PIXEL) {
            if (x == bx[0] || (x & 3) == 0)
              mxd::noise::pixel_normals(e.seed[0], e.seed[1], (uint32_t)b, (uint32_t)c, (uint32_t)y, (uint32_t)(x >> 2), z);
            bits = mxd::noise::elem_bits(z[x & 3], elem);
          }
          uint8_t* p = chw ? base + c * plane_stride + y * dst_stride + (int64_t)x * es
                           : base + y * dst_stride + ((int64_t)x * 3 + c) * es;
          put(p, es, bits);
        }
      }
  }
  return MXD_OK;
}
