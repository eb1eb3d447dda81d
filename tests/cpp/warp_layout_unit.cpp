// warp_layout_unit.cpp -- CPU unit test of a warp call's batch layout
// (mlx-data_amd/csrc/batch_layout.cpp) in the device-free environment
// (host_env) through capi_internal.h, linked against the in-tree
// libmxd_amd.so; no device call.  Built and run by tests/test_warp.py.
// Prints "ok <n>" or the first failure.
#include <cstdio>
#include <cstdlib>

#include "capi_internal.h"

using namespace mxd::capi;

static int g_checks = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    g_checks++;                                                      \
    if (!(c)) {                                                      \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

static uint8_t g_dummy[64];

static mxd_image image(int sw, int sh, int rw, int rh, int cx, int cy, int cw, int ch, int filter, int64_t stride) {
  mxd_image m{};
  m.src = g_dummy;
  m.src_stride = stride;
  m.src_w = sw, m.src_h = sh, m.channels = 3;
  m.resize_w = rw, m.resize_h = rh;
  m.crop_x = cx, m.crop_y = cy, m.crop_w = cw, m.crop_h = ch;
  m.dst = reinterpret_cast<void*>((uintptr_t(1) << 20) + 64 * (uintptr_t)sw + 1);
  m.dst_stride = (int64_t)cw * 3 * 2;
  m.filter = filter;
  return m;
}

static mxd_warp warp(int32_t mode, uint8_t r, uint8_t g, uint8_t b, double m0, double m1, double m2, double m3, double m4,
                     double m5) {
  mxd_warp w{};
  w.mode = mode;
  w.fill[0] = r, w.fill[1] = g, w.fill[2] = b;
  const double m[6] = {m0, m1, m2, m3, m4, m5};
  for (int k = 0; k < 6; k++) w.m[k] = m[k];
  return w;
}

int main() {
  // tone_layout_unit.cpp's mixed batch (general, wave, general, Catmull-Rom
  // wave, wave, wave / band, general) with every code path: a copy, two
  // table images (a translate, a scale), fixed point, bilinear.
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
  std::vector<mxd_warp> warps = {
      warp(MXD_WARP_BILINEAR, 1, 2, 3, 1, 0.3, 0, 0, 1, 0),   warp(MXD_WARP_NONE, 9, 9, 9, 5, 5, 5, 5, 5, 5),
      warp(MXD_WARP_NEAREST, 4, 5, 6, 1, 0, 2.5, 0, 1, -1.25), warp(MXD_WARP_NEAREST, 7, 8, 9, 1, 0.3, 0, -0.1, 1, 0),
      warp(MXD_WARP_BILINEAR, 0, 0, 0, 1, 0, 2.5, 0, 1, -1.25), warp(MXD_WARP_NEAREST, 255, 254, 253, 0.7, 0, 1, 0, 1.4, 0),
      warp(MXD_WARP_BILINEAR, 10, 20, 30, 0.5, 0.5, 1, -0.5, 0.5, 2),
  };
  const int32_t paths[7] = {mxd::kWarpBilinear, mxd::kWarpCopy,     mxd::kWarpTable, mxd::kWarpFixed,
                            mxd::kWarpBilinear, mxd::kWarpTable, mxd::kWarpBilinear};
  std::vector<mxd_tone> tones(n, mxd_tone{MXD_TONE_EQUALIZE, 0, 0.0f, 0});
  std::vector<mxd_color> colors(n);
  for (int32_t i = 0; i < n; i++)
    for (int k = 0; k < 12; k++) colors[i].m[k / 4][k % 4] = (float)(100 * i + k);
  mxd_out_format fmt{};
  fmt.elem = MXD_ELEM_BF16;
  fmt.layout = MXD_LAYOUT_HWC;
  const LayoutEnv env = host_env(64, 4096);
  for (int pass = 0; pass < 16; pass++) {
    const mxd_out_format* f = pass & 1 ? &fmt : nullptr;
    const bool prefer_band = (pass & 2) != 0;
    const mxd_color* cols = pass & 4 ? colors.data() : nullptr;
    const mxd_tone* tn = pass & 8 ? tones.data() : nullptr;
    const bool follows = f || cols || tn;
    mxd_set_kernel_policy(prefer_band ? MXD_POLICY_PREFER_BAND : MXD_POLICY_AUTO);
    BatchLayout L, Q;
    CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{f, cols, tn, warps.data()}, &L) == MXD_OK);
    CHECK(L.warped() && L.n == n);
    // what follows the warp: pixel_rows in a tone or colour call's layout (a format alone: identity matrices), or nothing
    CHECK(L.pass == (tn ? SecondPass::Tone : follows ? SecondPass::Color : SecondPass::None));
    // the routes and the resize descriptors are those of the same call without warps, all of them into scratch rows A
    CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, colors.data()}, &Q) == MXD_OK);
    CHECK(L.fmt_at == Q.fmt_at && std::memcmp(L.descs.data(), Q.descs.data(), L.fmt_at * sizeof(ImgDev)) == 0);
    for (const auto& g : L.waves) CHECK(g.cfg.f32 == 0 && mxd::wave_has_kernel(g.cfg));
    size_t a_end = 0;
    for (int32_t k = 0; k < n; k++) {
      const int32_t i = L.image_of[k];
      const uintptr_t off = reinterpret_cast<uintptr_t>(L.descs[k].dst);
      CHECK(off % 256 == 0 && L.descs[k].dst_stride % 16 == 0 && L.descs[k].dst_stride >= imgs[i].crop_w * 3);
      a_end = std::max<size_t>(a_end, off + (size_t)L.descs[k].dst_stride * imgs[i].crop_h);
      const mxd::WarpRowDev& e = L.warp_entry(i);
      CHECK(reinterpret_cast<uintptr_t>(e.src) == off && e.src_stride == L.descs[k].dst_stride);
      if (follows) {
        // scratch rows B: the same rows, b_at further on, read by the second pass
        CHECK(reinterpret_cast<uintptr_t>(e.dst) == off + L.b_at && e.dst_stride == e.src_stride);
        CHECK(reinterpret_cast<uintptr_t>(L.entry(i).src) == off + L.b_at && L.entry(i).src_stride == e.src_stride);
        CHECK(L.entry(i).dst == imgs[i].dst && L.entry(i).dst_stride == imgs[i].dst_stride);
      } else {
        CHECK(e.dst == imgs[i].dst && e.dst_stride == imgs[i].dst_stride);  // no B: the caller's destination
      }
    }
    if (follows) CHECK(L.b_at % 256 == 0 && L.b_at >= a_end && L.fmt_count() == n);
    else CHECK(L.b_at == 0 && L.fmt_count() == 0 && L.fmt_blocks() == 0);
    const size_t b_end = follows ? L.b_at + a_end : a_end;
    // the tables: behind B, before the tone workspace, one w + h int32 block per table image
    CHECK(L.warp_tab_count() == 2 && L.warp_tab_at % 256 == 0 && L.warp_tab_at >= b_end);
    const size_t tab_end = L.warp_tab_at + (40 + 40) * 4 * 2;
    if (tn) CHECK(L.tone_ws_at % 256 == 0 && L.tone_ws_at >= tab_end && L.scratch_bytes > L.tone_ws_at);
    else CHECK(L.scratch_bytes == tab_end);
    CHECK(L.warp_at() >= L.fmt_at + ((size_t)L.fmt_count() * L.entry_size() + sizeof(ImgDev) - 1) / sizeof(ImgDev));
    CHECK(L.descs.size() == L.warp_at() + ((size_t)n * sizeof(mxd::WarpRowDev) + sizeof(ImgDev) - 1) / sizeof(ImgDev));
    int32_t tiles = 0, tabs = 0;
    for (int32_t i = 0; i < n; i++) {
      const mxd::WarpRowDev& e = L.warp_entry(i);
      CHECK(e.w == imgs[i].crop_w && e.h == imgs[i].crop_h && e.path == paths[i]);
      CHECK(e.tile_begin == tiles && e.tiles_x == (e.w + mxd::kWarpTileW - 1) / mxd::kWarpTileW);
      tiles += e.tiles_x * ((e.h + mxd::kWarpTileH - 1) / mxd::kWarpTileH);
      CHECK(e.fill == ((uint32_t)warps[i].fill[0] | (uint32_t)warps[i].fill[1] << 8 | (uint32_t)warps[i].fill[2] << 16));
      for (int k = 0; k < 6; k++) CHECK(e.m[k] == (e.path == mxd::kWarpCopy ? 0.0 : warps[i].m[k]));
      if (e.path == mxd::kWarpTable) {
        CHECK(e.tab_index == tabs && e.tab_off == tabs * (40 + 40) * 4 && e.tab_off % 16 == 0);
        tabs++;
      } else {
        CHECK(e.tab_index == -1);
      }
    }
    CHECK(L.warp_tiles() == tiles && tabs == 2);
    // scratch offsets become addresses
    uint8_t* base = reinterpret_cast<uint8_t*>(uintptr_t(1) << 32);
    std::vector<uintptr_t> offs(n);
    for (int32_t k = 0; k < n; k++) offs[k] = reinterpret_cast<uintptr_t>(L.descs[k].dst);
    L.add_scratch(base);
    for (int32_t k = 0; k < n; k++) {
      const int32_t i = L.image_of[k];
      CHECK(L.descs[k].dst == base + offs[k] && L.warp_entry(i).src == base + offs[k]);
      if (follows) CHECK(L.warp_entry(i).dst == base + offs[k] + L.b_at && L.entry(i).src == L.warp_entry(i).dst);
      else CHECK(L.warp_entry(i).dst == imgs[i].dst);
    }
    CHECK(L.warp_tab == base + L.warp_tab_at);
    if (tn) CHECK(L.tone_ws == base + L.tone_ws_at);
  }
  mxd_set_kernel_policy(MXD_POLICY_AUTO);
  // no table image: no table bytes
  {
    std::vector<mxd_warp> w2 = warps;
    w2[2].mode = MXD_WARP_BILINEAR, w2[5].m[1] = 0.25;
    BatchLayout L;
    CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, w2.data()}, &L) == MXD_OK);
    CHECK(L.warp_tab_count() == 0 && L.warp_entry(5).path == mxd::kWarpFixed);
    size_t a_end = 0;
    for (int32_t k = 0; k < n; k++)
      a_end = std::max<size_t>(a_end, reinterpret_cast<uintptr_t>(L.descs[k].dst) +
                                          (size_t)L.descs[k].dst_stride * imgs[L.image_of[k]].crop_h);
    CHECK(L.scratch_bytes >= a_end && L.scratch_bytes < a_end + 256);
  }
  // another matrix, fill or mode, another upload: the cached descriptor slot is keyed by them
  BatchLayout A, B, C, D;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, warps.data()}, &A) == MXD_OK);
  warps[0].m[1] = 0.31;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, warps.data()}, &B) == MXD_OK);
  warps[3].fill[2] = 10;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, warps.data()}, &C) == MXD_OK);
  warps[6].mode = MXD_WARP_NEAREST;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, warps.data()}, &D) == MXD_OK);
  const BatchLayout* all[4] = {&A, &B, &C, &D};
  for (int a = 0; a < 4; a++)
    for (int b = a + 1; b < 4; b++) {
      CHECK(all[a]->descs.size() == all[b]->descs.size() && all[a]->warp_at() == all[b]->warp_at());
      CHECK(std::memcmp(all[a]->descs.data(), all[b]->descs.data(), A.descs.size() * sizeof(ImgDev)) != 0);
      CHECK(std::memcmp(all[a]->descs.data(), all[b]->descs.data(), A.warp_at() * sizeof(ImgDev)) == 0);
    }
  // what MXD_WARP_NONE does not read does not reach the upload
  warps[1].m[0] = 77.0, warps[1].fill[0] = 1;
  BatchLayout E;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, warps.data()}, &E) == MXD_OK);
  CHECK(std::memcmp(E.warp_entry(1).m, D.warp_entry(1).m, sizeof E.warp_entry(1).m) == 0);
  // without warps the layouts are what they were
  BatchLayout K, P;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, colors.data()}, &K) == MXD_OK);
  CHECK(!K.warped() && K.b_at == 0 && K.warp_tiles() == 0 && K.descs.size() == K.fmt_at + ((size_t)n * sizeof(mxd::ColorRowDev) + sizeof(ImgDev) - 1) / sizeof(ImgDev));
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{}, &P) == MXD_OK);
  CHECK(!P.warped() && P.pass == SecondPass::None && P.scratch_bytes == 0 && P.descs.size() == P.fmt_at);
  std::printf("ok %d\n", g_checks);
  return 0;
}
