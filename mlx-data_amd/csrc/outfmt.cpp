// outfmt.cpp -- formatted outputs (mxd_out_format, capi_internal.h): the
// table of the 256 elements a format assigns to the result bytes of each
// channel (the one place those values are computed: the kernels look them
// up), its cached device copies, and the validation of the _fmt calls.
// Host only.
#include <array>

#include "capi_internal.h"

namespace mxd {
namespace capi {
namespace {

uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

float float_of(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// float32 -> float16, round to nearest even (subnormal results through one
// float addition whose rounding is the half's).
uint16_t to_f16(float v) {
  uint32_t f = bits_of(v);
  const uint32_t sign = f & 0x80000000u;
  f ^= sign;
  const uint32_t inf32 = 255u << 23, max16 = (127u + 16u) << 23, magic = ((127u - 15u) + (23u - 10u) + 1u) << 23;
  uint32_t o;
  if (f >= max16) {
    o = f > inf32 ? 0x7e00u : 0x7c00u;
  } else if (f < (113u << 23)) {
    o = bits_of(float_of(f) + float_of(magic)) - magic;
  } else {
    const uint32_t odd = (f >> 13) & 1u;
    f += ((15u - 127u) << 23) + 0xfffu;
    f += odd;
    o = f >> 13;
  }
  return (uint16_t)(o | (sign >> 16));
}

// float32 -> bfloat16, round to nearest even.
uint16_t to_bf16(float v) {
  const uint32_t f = bits_of(v);
  if ((f & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;  // NaN
  return (uint16_t)((f + 0x7fffu + ((f >> 16) & 1u)) >> 16);
}

}  // namespace

int32_t fmt_elem_size(const mxd_out_format& fmt) { return fmt.elem == MXD_ELEM_F32 ? 4 : 2; }

int fmt_validate(const mxd_out_format* fmt, int32_t channels) {
  if (!fmt) return fail(MXD_ERR_INVALID, "mxd: null fmt");
  if (fmt->elem != MXD_ELEM_F32 && fmt->elem != MXD_ELEM_F16 && fmt->elem != MXD_ELEM_BF16)
    return fail(MXD_ERR_INVALID, "mxd_out_format: unknown elem " + std::to_string(fmt->elem));
  if (fmt->layout != MXD_LAYOUT_HWC && fmt->layout != MXD_LAYOUT_CHW)
    return fail(MXD_ERR_INVALID, "mxd_out_format: unknown layout " + std::to_string(fmt->layout));
  if (fmt->normalize)
    for (int32_t c = 0; c < channels && c < 4; c++) {
      if (!std::isfinite(fmt->std[c]) || fmt->std[c] == 0.0f)
        return fail(MXD_ERR_INVALID, "mxd_out_format: std[" + std::to_string(c) + "] is zero or not finite");
      if (!std::isfinite(fmt->mean[c]))
        return fail(MXD_ERR_INVALID, "mxd_out_format: mean[" + std::to_string(c) + "] is not finite");
    }
  return MXD_OK;
}

int fmt_validate_images(const mxd_image* images, int32_t n, const mxd_out_format& fmt) {
  const int64_t es = fmt_elem_size(fmt);
  const bool chw = fmt.layout == MXD_LAYOUT_CHW;
  if (chw && fmt.plane_stride % es != 0)
    return fail(MXD_ERR_INVALID, "mxd_out_format: plane_stride is not a multiple of the element size");
  for (int32_t i = 0; i < n; i++) {
    const mxd_image& im = images[i];
    const std::string at = " (image " + std::to_string(i) + ")";
    if (int rc = fmt_validate(&fmt, im.channels)) return rc;
    if (reinterpret_cast<uintptr_t>(im.dst) % es != 0)
      return fail(MXD_ERR_INVALID, "mxd: dst is not a multiple of the element size" + at);
    if (im.dst_stride % es != 0)
      return fail(MXD_ERR_INVALID, "mxd: dst_stride is not a multiple of the element size" + at);
    if (im.dst_stride < (int64_t)im.crop_w * (chw ? 1 : im.channels) * es)
      return fail(MXD_ERR_INVALID, "mxd: dst_stride smaller than an output row" + at);
    if (chw && im.channels != images[0].channels)
      return fail(MXD_ERR_INVALID, "mxd: channels differ within a CHW call" + at);
    if (chw && fmt.plane_stride < (int64_t)im.crop_h * im.dst_stride)
      return fail(MXD_ERR_INVALID, "mxd_out_format: plane_stride smaller than crop_h * dst_stride" + at);
  }
  return MXD_OK;
}

void fmt_table(const mxd_out_format& fmt, int32_t channels, void* table) {
  for (int32_t c = 0; c < channels; c++)
    for (int32_t q = 0; q < 256; q++) {
      // each operation a float32 operation, correctly rounded (volatile: none
      // is contracted or carried in a wider type)
      volatile float x = (float)q / 255.0f;
      volatile float y = x;
      if (fmt.normalize) {
        volatile float d = x - fmt.mean[c];
        y = d / fmt.std[c];
      }
      const size_t i = (size_t)c * 256 + q;
      if (fmt.elem == MXD_ELEM_F32) static_cast<float*>(table)[i] = y;
      else if (fmt.elem == MXD_ELEM_F16) static_cast<uint16_t*>(table)[i] = to_f16(y);
      else static_cast<uint16_t*>(table)[i] = to_bf16(y);
    }
}

// Device copies of the tables, one per (device, element type, channels,
// normalisation constants), built on first use like the tap tables.  Entries
// live for the process (a launch in flight may read one, so none is freed):
// at most 4 KB each, for callers with a handful of formats.  A caller that
// draws new constants per call (jittered statistics) grows this by one entry
// per distinct set; INTEGRATION.md states the limit.
int fmt_device_table(int32_t device, const mxd_out_format& fmt, int32_t channels, const void** out) {
  static std::mutex mu;
  static auto* cache = new std::map<std::array<uint32_t, 12>, void*>();
  std::array<uint32_t, 12> key{};
  key[0] = (uint32_t)device, key[1] = (uint32_t)fmt.elem, key[2] = (uint32_t)channels, key[3] = fmt.normalize ? 1u : 0u;
  if (fmt.normalize)
    for (int32_t c = 0; c < channels; c++) key[4 + c] = bits_of(fmt.mean[c]), key[8 + c] = bits_of(fmt.std[c]);
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache->find(key);
  if (it != cache->end()) {
    *out = it->second;
    return MXD_OK;
  }
  std::vector<uint32_t> host((size_t)channels * 256);
  fmt_table(fmt, channels, host.data());
  const size_t bytes = (size_t)channels * 256 * fmt_elem_size(fmt);
  DeviceGuard g(device);
  void* dev = nullptr;
  MXD_HIP(hipMalloc(&dev, bytes));
  MXD_HIP(hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice));
  (*cache)[key] = dev;
  *out = dev;
  return MXD_OK;
}

}  // namespace capi
}  // namespace mxd

using namespace mxd::capi;

extern "C" int mxd_out_format_table(const mxd_out_format* fmt, int32_t channels, void* table) {
  if (channels < 1 || channels > 4) return fail(MXD_ERR_INVALID, "verifyImage: channels must be 0 <= c <= 4");
  if (int rc = fmt_validate(fmt, channels)) return rc;
  if (!table) return fail(MXD_ERR_INVALID, "mxd: null table");
  fmt_table(*fmt, channels, table);
  return MXD_OK;
}
