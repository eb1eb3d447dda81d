// enhance_layout_unit.cpp -- CPU unit test of an enhance call's batch layout
// (mlx-data_amd/csrc/batch_layout.cpp) in the device-free environment
// (host_env) through capi_internal.h, linked against the in-tree
// libmxd_amd.so; no device call.  Built and run by tests/test_enhance.py.
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

static mxd_enhance enhance(int32_t op, float factor) {
  mxd_enhance e{};
  e.op = op, e.factor = factor;
  return e;
}

static uintptr_t off_of(const void* p) { return reinterpret_cast<uintptr_t>(p); }

int main() {
  // warp_layout_unit.cpp's mixed batch (general, wave, general, Catmull-Rom
  // wave, wave, wave / band, general) with every op.
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
  std::vector<mxd_enhance> enh = {
      enhance(MXD_ENHANCE_SHARPNESS, 1.5f), enhance(MXD_ENHANCE_NONE, 9.0f),      enhance(MXD_ENHANCE_COLOR, 0.25f),
      enhance(MXD_ENHANCE_BRIGHTNESS, 2.0f), enhance(MXD_ENHANCE_SHARPNESS, 0.0f), enhance(MXD_ENHANCE_COLOR, 1.0f),
      enhance(MXD_ENHANCE_BRIGHTNESS, 0.5f),
  };
  std::vector<mxd_warp> warps(n);
  for (int32_t i = 0; i < n; i++) {
    warps[i] = mxd_warp{};
    warps[i].mode = i % 2 ? MXD_WARP_BILINEAR : MXD_WARP_NEAREST;
    const double m[6] = {1, 0.3, 0, -0.1, 1, 0};  // (no table image)
    for (int k = 0; k < 6; k++) warps[i].m[k] = m[k];
  }
  std::vector<mxd_tone> tones(n, mxd_tone{MXD_TONE_EQUALIZE, 0, 0.0f, 0});
  std::vector<mxd_color> colors(n);
  for (int32_t i = 0; i < n; i++)
    for (int k = 0; k < 12; k++) colors[i].m[k / 4][k % 4] = (float)(100 * i + k);
  mxd_out_format fmt{};
  fmt.elem = MXD_ELEM_BF16;
  fmt.layout = MXD_LAYOUT_HWC;
  const LayoutEnv env = host_env(64, 4096);
  for (int pass = 0; pass < 32; pass++) {
    const mxd_out_format* f = pass & 1 ? &fmt : nullptr;
    const bool prefer_band = (pass & 2) != 0;
    const mxd_color* cols = pass & 4 ? colors.data() : nullptr;
    const mxd_tone* tn = pass & 8 ? tones.data() : nullptr;
    const mxd_warp* wp = pass & 16 ? warps.data() : nullptr;
    const bool follows = f || cols || tn;
    mxd_set_kernel_policy(prefer_band ? MXD_POLICY_PREFER_BAND : MXD_POLICY_AUTO);
    BatchLayout L, Q;
    CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{f, cols, tn, wp, enh.data()}, &L) == MXD_OK);
    CHECK(L.enhanced() && L.warped() == (wp != nullptr) && L.n == n);
    // what follows the stage: pixel_rows in a tone or colour call's layout (a format alone: identity matrices), or nothing
    CHECK(L.pass == (tn ? SecondPass::Tone : follows ? SecondPass::Color : SecondPass::None));
    // the routes and the resize descriptors are those of the same call without the stages, all of them into scratch rows A
    CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, colors.data()}, &Q) == MXD_OK);
    CHECK(L.fmt_at == Q.fmt_at && std::memcmp(L.descs.data(), Q.descs.data(), L.fmt_at * sizeof(ImgDev)) == 0);
    // rows B exist when a second pass follows, or when the warp stage has to hand its rows to this one
    const bool has_b = follows || wp;
    size_t a_end = 0;
    for (int32_t k = 0; k < n; k++) {
      const int32_t i = L.image_of[k];
      const uintptr_t off = off_of(L.descs[k].dst);
      CHECK(off % 256 == 0 && L.descs[k].dst_stride % 16 == 0 && L.descs[k].dst_stride >= imgs[i].crop_w * 3);
      a_end = std::max<size_t>(a_end, off + (size_t)L.descs[k].dst_stride * imgs[i].crop_h);
      const mxd::EnhanceRowDev& e = L.enhance_entry(i);
      CHECK(e.src_stride == L.descs[k].dst_stride);
      // the stage cannot run in place
      CHECK(off_of(e.src) != off_of(e.dst));
      if (wp) {
        // the warp writes B (always: this stage reads it), this stage reads B and writes A or the destinations
        const mxd::WarpRowDev& w = L.warp_entry(i);
        CHECK(off_of(w.src) == off && off_of(w.dst) == off + L.b_at && w.dst_stride == w.src_stride);
        CHECK(off_of(e.src) == off + L.b_at);
        if (follows) {
          CHECK(off_of(e.dst) == off && e.dst_stride == e.src_stride);
          CHECK(off_of(L.entry(i).src) == off && L.entry(i).src_stride == e.src_stride);
        }
      } else {
        // this stage reads A and writes B or the destinations
        CHECK(off_of(e.src) == off);
        if (follows) {
          CHECK(off_of(e.dst) == off + L.b_at && e.dst_stride == e.src_stride);
          CHECK(off_of(L.entry(i).src) == off + L.b_at && L.entry(i).src_stride == e.src_stride);
        }
      }
      if (follows) CHECK(L.entry(i).dst == imgs[i].dst && L.entry(i).dst_stride == imgs[i].dst_stride);
      else CHECK(e.dst == imgs[i].dst && e.dst_stride == imgs[i].dst_stride);
    }
    if (has_b) CHECK(L.b_at % 256 == 0 && L.b_at >= a_end);
    else CHECK(L.b_at == 0);
    if (follows) CHECK(L.fmt_count() == n);
    else CHECK(L.fmt_count() == 0 && L.fmt_blocks() == 0);
    // no third scratch: A, B, then the tone workspace
    const size_t b_end = has_b ? L.b_at + a_end : a_end;
    if (tn) CHECK(L.tone_ws_at % 256 == 0 && L.tone_ws_at >= b_end && L.tone_ws_at < b_end + 512 && L.scratch_bytes > L.tone_ws_at);
    else CHECK(L.scratch_bytes >= b_end && L.scratch_bytes < b_end + 512);
    // the entries: behind the second pass's and the warp stage's
    const size_t fmt_end = L.fmt_at + ((size_t)L.fmt_count() * L.entry_size() + sizeof(ImgDev) - 1) / sizeof(ImgDev);
    if (wp) CHECK(L.warp_at() >= fmt_end && L.enhance_at() == L.warp_at() + ((size_t)n * sizeof(mxd::WarpRowDev) + sizeof(ImgDev) - 1) / sizeof(ImgDev));
    else CHECK(L.enhance_at() >= fmt_end);
    CHECK(L.descs.size() == L.enhance_at() + ((size_t)n * sizeof(mxd::EnhanceRowDev) + sizeof(ImgDev) - 1) / sizeof(ImgDev));
    int32_t tiles = 0;
    for (int32_t i = 0; i < n; i++) {
      const mxd::EnhanceRowDev& e = L.enhance_entry(i);
      CHECK(e.w == imgs[i].crop_w && e.h == imgs[i].crop_h && e.op == enh[i].op);
      CHECK(e.factor == (enh[i].op == MXD_ENHANCE_NONE ? 0.0f : enh[i].factor));
      CHECK(e.tile_begin == tiles && e.tiles_x == (e.w + mxd::kEnhTileW - 1) / mxd::kEnhTileW);
      tiles += e.tiles_x * ((e.h + mxd::kEnhTileH - 1) / mxd::kEnhTileH);
    }
    CHECK(L.enhance_tiles() == tiles);
    // scratch offsets become addresses
    uint8_t* base = reinterpret_cast<uint8_t*>(uintptr_t(1) << 32);
    std::vector<uintptr_t> offs(n);
    for (int32_t k = 0; k < n; k++) offs[k] = off_of(L.descs[k].dst);
    L.add_scratch(base);
    for (int32_t k = 0; k < n; k++) {
      const int32_t i = L.image_of[k];
      const mxd::EnhanceRowDev& e = L.enhance_entry(i);
      CHECK(L.descs[k].dst == base + offs[k]);
      CHECK(e.src == base + offs[k] + (wp ? L.b_at : 0));
      if (wp) CHECK(L.warp_entry(i).src == base + offs[k] && L.warp_entry(i).dst == e.src);
      if (follows) CHECK(e.dst == base + offs[k] + (wp ? 0 : L.b_at) && L.entry(i).src == e.dst);
      else CHECK(e.dst == imgs[i].dst);
    }
    if (tn) CHECK(L.tone_ws == base + L.tone_ws_at);
  }
  mxd_set_kernel_policy(MXD_POLICY_AUTO);
  // another op or factor, another upload: the cached descriptor slot is keyed by them
  BatchLayout A, B, C;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, nullptr, enh.data()}, &A) == MXD_OK);
  enh[0].factor = 1.51f;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, nullptr, enh.data()}, &B) == MXD_OK);
  enh[6].op = MXD_ENHANCE_COLOR;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, nullptr, enh.data()}, &C) == MXD_OK);
  const BatchLayout* all[3] = {&A, &B, &C};
  for (int a = 0; a < 3; a++)
    for (int b = a + 1; b < 3; b++) {
      CHECK(all[a]->descs.size() == all[b]->descs.size() && all[a]->enhance_at() == all[b]->enhance_at());
      CHECK(std::memcmp(all[a]->descs.data(), all[b]->descs.data(), A.descs.size() * sizeof(ImgDev)) != 0);
      CHECK(std::memcmp(all[a]->descs.data(), all[b]->descs.data(), A.enhance_at() * sizeof(ImgDev)) == 0);
    }
  // what MXD_ENHANCE_NONE does not read does not reach the upload
  enh[1].factor = 77.0f;
  BatchLayout E;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, nullptr, nullptr, nullptr, enh.data()}, &E) == MXD_OK);
  CHECK(E.descs.size() == C.descs.size() && std::memcmp(E.descs.data(), C.descs.data(), C.descs.size() * sizeof(ImgDev)) == 0);
  // a host-path chunk's slice
  const PostOps whole{&fmt, colors.data(), tones.data(), warps.data(), enh.data()};
  const PostOps part = whole.at(3);
  CHECK(part.fmt == &fmt && part.colors == colors.data() + 3 && part.tones == tones.data() + 3);
  CHECK(part.warps == warps.data() + 3 && part.enhances == enh.data() + 3);
  CHECK(PostOps{}.at(2).enhances == nullptr && !PostOps{}.any());
  // without enhance ops the layouts are what they were
  BatchLayout W, K, P;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{&fmt, nullptr, nullptr, warps.data()}, &W) == MXD_OK);
  CHECK(!W.enhanced() && W.enhance_tiles() == 0 && W.enhance_at() == 0);
  CHECK(W.descs.size() == W.warp_at() + ((size_t)n * sizeof(mxd::WarpRowDev) + sizeof(ImgDev) - 1) / sizeof(ImgDev));
  CHECK(off_of(W.entry(0).src) == off_of(W.warp_entry(0).dst));
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, colors.data()}, &K) == MXD_OK);
  CHECK(!K.enhanced() && !K.warped() && K.b_at == 0 &&
        K.descs.size() == K.fmt_at + ((size_t)n * sizeof(mxd::ColorRowDev) + sizeof(ImgDev) - 1) / sizeof(ImgDev));
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{}, &P) == MXD_OK);
  CHECK(!P.enhanced() && P.pass == SecondPass::None && P.scratch_bytes == 0 && P.descs.size() == P.fmt_at);
  std::printf("ok %d\n", g_checks);
  return 0;
}
