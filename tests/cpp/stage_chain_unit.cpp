// stage_chain_unit.cpp -- dumps the batch layout (mlx-data_amd/csrc/
// batch_layout.cpp) of every combination of the five things that can follow
// the resize (format, colours, tones, warps, enhances) under two kernel
// policies, in the device-free environment (host_env) through
// capi_internal.h, linked against the in-tree libmxd_amd.so; no device call.
// One line per layout: the uploaded bytes as a digest (as built, and once the
// scratch offsets are addresses), the scratch offsets and every launch
// parameter.  Built and run by tests/test_stage_chain.py, which compares the
// lines with tests/golden/stage_chain_layouts.txt: the upload and the
// launches of a call are a fixed function of the call.
#include <cstdio>
#include <cstdlib>

#include "capi_internal.h"

using namespace mxd::capi;

// Fixed fake addresses (never dereferenced), so the bytes do not depend on
// where the process is loaded.
static const uint8_t* const kSrc = reinterpret_cast<const uint8_t*>(uintptr_t(3) << 33);

static mxd_image image(int sw, int sh, int rw, int rh, int cx, int cy, int cw, int ch, int filter, int64_t stride) {
  mxd_image m{};
  m.src = kSrc;
  m.src_stride = stride;
  m.src_w = sw, m.src_h = sh, m.channels = 3;
  m.resize_w = rw, m.resize_h = rh;
  m.crop_x = cx, m.crop_y = cy, m.crop_w = cw, m.crop_h = ch;
  m.dst = reinterpret_cast<void*>((uintptr_t(1) << 20) + 64 * (uintptr_t)sw + 1);
  m.dst_stride = (int64_t)cw * 3 * 2;
  m.filter = filter;
  return m;
}

static mxd_warp warp(int32_t mode, double m0, double m1, double m2, double m3, double m4, double m5) {
  mxd_warp w{};
  w.mode = mode;
  w.fill[0] = 124, w.fill[1] = 116, w.fill[2] = 104;
  const double m[6] = {m0, m1, m2, m3, m4, m5};
  for (int k = 0; k < 6; k++) w.m[k] = m[k];
  return w;
}

static uint64_t digest(const std::vector<mxd::ImgDev>& descs) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(descs.data());
  uint64_t h = 1469598103934665603ull;  // FNV-1a
  for (size_t k = 0; k < descs.size() * sizeof(mxd::ImgDev); k++) h = (h ^ p[k]) * 1099511628211ull;
  return h;
}

int main() {
  // enhance_layout_unit.cpp's mixed batch (general, wave, general, Catmull-Rom
  // wave, wave, wave / band, general).
  std::vector<mxd_image> imgs = {
      image(101, 99, 75, 70, 3, 2, 61, 33, 0, 101 * 3),
      image(500, 375, 341, 256, 58, 16, 224, 224, 0, 1504),
      image(680, 680, 40, 40, 0, 0, 40, 40, 0, 2048),
      image(500, 375, 341, 256, 58, 16, 224, 224, 1, 1504),
      image(500, 375, 341, 256, 57, 15, 223, 221, 0, 1504),
      image(600, 600, 40, 40, 0, 0, 40, 40, 0, 1808),
      image(101, 99, 75, 70, 0, 0, 16, 16, 0, 101 * 3),
  };
  const int32_t n = (int32_t)imgs.size();
  const std::vector<mxd_enhance> enh = {
      {MXD_ENHANCE_SHARPNESS, 1.9f, 0, 0}, {MXD_ENHANCE_NONE, 9.0f, 0, 0},      {MXD_ENHANCE_COLOR, 0.25f, 0, 0},
      {MXD_ENHANCE_BRIGHTNESS, 2.0f, 0, 0}, {MXD_ENHANCE_SHARPNESS, 0.0f, 0, 0}, {MXD_ENHANCE_COLOR, 1.0f, 0, 0},
      {MXD_ENHANCE_BRIGHTNESS, 0.5f, 0, 0},
  };
  const std::vector<mxd_warp> warps = {
      warp(MXD_WARP_NONE, 5, 6, 7, 8, 9, 10),              // (nothing of it is read)
      warp(MXD_WARP_NEAREST, 1.2, 0, 3, 0, 0.9, -2),       // table path
      warp(MXD_WARP_NEAREST, 1, 0.3, 0, -0.1, 1, 0),       // fixed point
      warp(MXD_WARP_BILINEAR, 0.9, -0.2, 4, 0.2, 0.9, 1),
      warp(MXD_WARP_NEAREST, 1, 0, -7.5, 0, 1, 2.25),      // table path
      warp(MXD_WARP_BILINEAR, 1, 0, 0.5, 0, 1, 0),
      warp(MXD_WARP_NEAREST, 0.8, 0.6, 1, -0.6, 0.8, 3),   // fixed point
  };
  const std::vector<mxd_tone> tones = {
      {MXD_TONE_EQUALIZE, 0, 0.0f, 0},     {MXD_TONE_POSTERIZE, 3, 0.0f, 0}, {MXD_TONE_NONE, 0, 0.0f, 0},
      {MXD_TONE_AUTOCONTRAST, 0, 0.0f, 0}, {MXD_TONE_EQUALIZE, 0, 0.0f, 0},  {MXD_TONE_SOLARIZE, 128, 0.0f, 0},
      {MXD_TONE_CONTRAST, 0, 1.5f, 0},
  };
  std::vector<mxd_color> colors(n);
  for (int32_t i = 0; i < n; i++)
    for (int k = 0; k < 12; k++) colors[i].m[k / 4][k % 4] = i == 2 ? (k % 5 == 0 ? 1.0f : 0.0f) : (float)(100 * i + k) / 64;
  mxd_out_format fmt{};
  fmt.elem = MXD_ELEM_BF16;
  fmt.layout = MXD_LAYOUT_HWC;
  const LayoutEnv env = host_env(64, 4096);
  const int32_t policies[2] = {MXD_POLICY_AUTO, MXD_POLICY_PREFER_BAND};
  for (int pol = 0; pol < 2; pol++)
    for (int combo = 0; combo < 32; combo++) {
      const PostOps ops{combo & 1 ? &fmt : nullptr, combo & 2 ? colors.data() : nullptr, combo & 4 ? tones.data() : nullptr,
                        combo & 8 ? warps.data() : nullptr, combo & 16 ? enh.data() : nullptr};
      mxd_set_kernel_policy(policies[pol]);
      BatchLayout L;
      if (build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, ops, &L) != MXD_OK) {
        std::printf("FAIL policy %d combo %d: %s\n", policies[pol], combo, mxd_last_error());
        return 1;
      }
      const uint64_t built = digest(L.descs);
      if (L.scratch_bytes > 0) L.add_scratch(reinterpret_cast<uint8_t*>(uintptr_t(1) << 32));
      std::printf("policy=%d fmt=%d colors=%d tones=%d warps=%d enhances=%d descs=%zu built=%016llx placed=%016llx scratch=%zu",
                  policies[pol], combo & 1, combo >> 1 & 1, combo >> 2 & 1, combo >> 3 & 1, combo >> 4 & 1, L.descs.size(),
                  (unsigned long long)built, (unsigned long long)digest(L.descs), L.scratch_bytes);
      std::printf(" pass_at=%zu warp_at=%zu enhance_at=%zu b_at=%zu tab_at=%zu tone_ws_at=%zu", L.fmt_at, L.warp_at(),
                  L.enhance_at(), L.b_at, L.warp_tab_at, L.tone_ws_at);
      std::printf(" pass=%d matrix=%d entries=%d blocks=%d hist_blocks=%d stat_bytes=%zu warp_tiles=%d tabs=%d enhance_tiles=%d",
                  (int)L.pass, L.matrix ? 1 : 0, L.fmt_count(), L.fmt_blocks(), L.tone_hist_blocks(), L.tone_stat_bytes,
                  L.warp_tiles(), L.warp_tab_count(), L.enhance_tiles());
      std::printf(" ws=%llx tab=%llx launches=", (unsigned long long)reinterpret_cast<uintptr_t>(L.tone_ws),
                  (unsigned long long)reinterpret_cast<uintptr_t>(L.warp_tab));
      for (const BatchLayout::Launch& l : L.launches) std::printf("(%d,%lld)", l.kind, (long long)l.units);
      std::printf("\n");
    }
  mxd_set_kernel_policy(MXD_POLICY_AUTO);
  return 0;
}
