// tone_layout_unit.cpp -- CPU unit test of a tone call's batch layout
// (mlx-data_amd/csrc/batch_layout.cpp) in the device-free environment
// (host_env) through capi_internal.h, linked against the in-tree
// libmxd_amd.so; no device call.  Built and run by tests/test_tone.py.
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
  m.dst = reinterpret_cast<void*>((uintptr_t(1) << 20) + 64 * (uintptr_t)sw);
  m.dst_stride = (int64_t)cw * 3 * 2;
  m.filter = filter;
  return m;
}

// Entry j of a tone call's layout (it starts with the head L.entry(j) returns).
static const mxd::ToneRowDev& tone_entry(BatchLayout& L, int32_t j) {
  return reinterpret_cast<const mxd::ToneRowDev&>(L.entry(j));
}

int main() {
  // color_layout_unit.cpp's mixed batch (general, wave, general, Catmull-Rom
  // wave, wave, wave / band) and a seventh image, with all six ops: images 1
  // and 6 (NONE, SOLARIZE) and 3 (POSTERIZE) need no statistics.
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
  std::vector<mxd_tone> tones = {
      {MXD_TONE_EQUALIZE, 0, 0.0f, 0},  {MXD_TONE_NONE, 0, 0.0f, 0},         {MXD_TONE_CONTRAST, 0, 1.75f, 0},
      {MXD_TONE_POSTERIZE, 3, 0.0f, 0}, {MXD_TONE_AUTOCONTRAST, 0, 0.0f, 0}, {MXD_TONE_CONTRAST, 0, 0.5f, 0},
      {MXD_TONE_SOLARIZE, 200, 0.0f, 0},
  };
  const bool stats[7] = {true, false, true, false, true, true, false};
  std::vector<mxd_color> colors(n);
  for (int32_t i = 0; i < n; i++)
    for (int k = 0; k < 12; k++) colors[i].m[k / 4][k % 4] = (float)(100 * i + k);
  mxd_out_format fmt{};
  fmt.elem = MXD_ELEM_BF16;
  fmt.layout = MXD_LAYOUT_HWC;
  const LayoutEnv env = host_env(64, 4096);
  const size_t stat_block = mxd::kToneStatWords * sizeof(uint32_t);
  for (int pass = 0; pass < 8; pass++) {
    const mxd_out_format* f = pass & 1 ? &fmt : nullptr;
    const bool prefer_band = (pass & 2) != 0;
    const mxd_color* cols = pass & 4 ? colors.data() : nullptr;
    mxd_set_kernel_policy(prefer_band ? MXD_POLICY_PREFER_BAND : MXD_POLICY_AUTO);
    BatchLayout L;
    CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{f, cols, tones.data()}, &L) == MXD_OK);
    CHECK(L.pass == SecondPass::Tone && L.entry_size() == sizeof(mxd::ToneRowDev) && L.n == n && (int32_t)L.image_of.size() == n);
    CHECK(L.matrix == (cols != nullptr));
    // the routes are those of a plain u8 call
    CHECK(!L.plans[0].wave && !L.plans[0].band && !L.plans[2].wave && !L.plans[2].band);
    if (!prefer_band) CHECK(L.plans[1].wave && L.plans[3].wave && L.plans[3].s == 4 && L.plans[4].wave && L.bands.empty());
    else CHECK(L.plans[5].band && !L.bands.empty());
    for (const auto& g : L.waves) CHECK(g.cfg.f32 == 0 && mxd::wave_has_kernel(g.cfg));
    // every image is in scratch at a 256-byte aligned offset, below the workspace
    size_t end_max = 0;
    for (int32_t k = 0; k < n; k++) {
      const int32_t i = L.image_of[k];
      const uintptr_t off = reinterpret_cast<uintptr_t>(L.descs[k].dst);
      CHECK(off % 256 == 0 && off < L.tone_ws_at);
      CHECK(L.descs[k].dst_stride % 16 == 0 && L.descs[k].dst_stride >= imgs[i].crop_w * 3);
      end_max = std::max<size_t>(end_max, off + (size_t)L.descs[k].dst_stride * imgs[i].crop_h);
      const mxd::FmtRowDev& r = L.entry(i);
      CHECK(reinterpret_cast<uintptr_t>(r.src) == off && r.src_stride == L.descs[k].dst_stride);
    }
    CHECK(end_max <= L.tone_ws_at && L.tone_ws_at % 256 == 0);
    // the workspace: one statistics block per image that needs one, then a table per image
    CHECK(L.tone_stat_bytes == 4 * stat_block);
    CHECK(L.scratch_bytes == L.tone_ws_at + L.tone_stat_bytes + (size_t)n * mxd::kToneLutBytes);
    CHECK(L.fmt_count() == n);
    CHECK(L.descs.size() >= L.fmt_at + ((size_t)n * sizeof(mxd::ToneRowDev) + sizeof(ImgDev) - 1) / sizeof(ImgDev));
    int32_t blocks = 0, hist = 0, nstat = 0;
    for (int32_t i = 0; i < n; i++) {
      const mxd::ToneRowDev& r = tone_entry(L, i);
      const mxd::FmtRowDev& h = r.color.head;
      CHECK(&h == &L.entry(i));
      CHECK(h.dst == imgs[i].dst && h.dst_stride == imgs[i].dst_stride);
      CHECK(h.crop_w == imgs[i].crop_w && h.crop_h == imgs[i].crop_h && h.channels == 3);
      CHECK(r.op == tones[i].op && r.arg == tones[i].arg && r.factor == tones[i].factor);
      for (int k = 0; k < 12; k++) CHECK(r.color.m[k] == (cols ? (float)(100 * i + k) : k % 5 == 0 ? 1.0f : 0.0f));
      CHECK(h.blk_begin == blocks && r.hist_begin == hist);
      CHECK(mxd::tone_needs_stats(r.op) == stats[i]);
      if (stats[i]) {
        CHECK(r.stat_off == (int32_t)(nstat * stat_block));
        nstat++;
        hist += (imgs[i].crop_h + mxd::kToneHistRows - 1) / mxd::kToneHistRows;
      } else {
        CHECK(r.stat_off == -1);  // and no tone_hist workgroup: hist stays
      }
      CHECK(r.lut_off == (int32_t)(L.tone_stat_bytes + (size_t)i * mxd::kToneLutBytes) && r.lut_off % 256 == 0);
      CHECK((size_t)r.lut_off + mxd::kToneLutBytes <= L.scratch_bytes - L.tone_ws_at);
      blocks += (imgs[i].crop_h + mxd::kPixelRows - 1) / mxd::kPixelRows;
    }
    CHECK(L.fmt_blocks() == blocks && L.tone_hist_blocks() == hist && hist > 0);
    // tone_hist's search (the last image whose hist_begin <= block) finds an image with statistics
    for (int32_t blk = 0; blk < hist; blk++) {
      int32_t found = 0;
      for (int32_t i = 0; i < n; i++)
        if (tone_entry(L, i).hist_begin <= blk) found = i;
      CHECK(stats[found]);
      const int32_t y0 = (blk - tone_entry(L, found).hist_begin) * mxd::kToneHistRows;
      CHECK(y0 >= 0 && y0 < imgs[found].crop_h);
    }
    // scratch offsets become addresses for every descriptor and entry, and the workspace gets its own
    uint8_t* base = reinterpret_cast<uint8_t*>(uintptr_t(1) << 32);
    std::vector<uintptr_t> offs(n);
    for (int32_t k = 0; k < n; k++) offs[k] = reinterpret_cast<uintptr_t>(L.descs[k].dst);
    L.add_scratch(base);
    for (int32_t k = 0; k < n; k++) {
      CHECK(L.descs[k].dst == base + offs[k]);
      CHECK(L.entry(L.image_of[k]).src == base + offs[k]);
    }
    CHECK(L.tone_ws == base + L.tone_ws_at);
  }
  mxd_set_kernel_policy(MXD_POLICY_AUTO);
  // only ops without statistics: no tone_hist workgroup, no statistics bytes
  {
    std::vector<mxd_tone> flat(n, mxd_tone{MXD_TONE_POSTERIZE, 4, 0.0f, 0});
    flat[2].op = MXD_TONE_NONE;
    BatchLayout L;
    CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, flat.data()}, &L) == MXD_OK);
    CHECK(L.tone_hist_blocks() == 0 && L.tone_stat_bytes == 0 && L.fmt_blocks() > 0);
    for (int32_t i = 0; i < n; i++) CHECK(tone_entry(L, i).stat_off == -1 && tone_entry(L, i).hist_begin == 0);
  }
  // other ops or parameters, other upload: the cached descriptor slot is keyed by them
  BatchLayout A, B, C, D;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, tones.data()}, &A) == MXD_OK);
  tones[5].factor = 0.75f;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, tones.data()}, &B) == MXD_OK);
  tones[3].arg = 4;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, tones.data()}, &C) == MXD_OK);
  tones[6].op = MXD_TONE_NONE;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, tones.data()}, &D) == MXD_OK);
  const BatchLayout* all[4] = {&A, &B, &C, &D};
  for (int a = 0; a < 4; a++)
    for (int b = a + 1; b < 4; b++) {
      CHECK(all[a]->descs.size() == all[b]->descs.size());
      CHECK(std::memcmp(all[a]->descs.data(), all[b]->descs.data(), A.descs.size() * sizeof(ImgDev)) != 0);
      CHECK(std::memcmp(all[a]->descs.data(), all[b]->descs.data(), A.fmt_at * sizeof(ImgDev)) == 0);
    }
  // without tones the layouts are the colour call's and the plain call's
  BatchLayout K, P;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, colors.data()}, &K) == MXD_OK);
  CHECK(K.pass == SecondPass::Color && K.tone_stat_bytes == 0 && K.tone_ws_at == 0 && K.fmt_count() == n);
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{}, &P) == MXD_OK);
  CHECK(P.pass == SecondPass::None && P.fmt_count() == 0 && P.scratch_bytes == 0 && P.descs.size() == P.fmt_at);
  std::printf("ok %d\n", g_checks);
  return 0;
}
