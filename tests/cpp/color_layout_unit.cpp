// color_layout_unit.cpp -- CPU unit test of a colour call's batch layout
// (mlx-data_amd/csrc/batch_layout.cpp) in the device-free environment
// (host_env) through capi_internal.h, linked against the in-tree
// libmxd_amd.so; no device call.  Built and run by tests/test_color.py.
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

static mxd_image image(int sw, int sh, int rw, int rh, int cx, int cy, int cw, int ch, int filter, int64_t stride,
                       uintptr_t src_off) {
  mxd_image m{};
  m.src = g_dummy + src_off;
  m.src_stride = stride;
  m.src_w = sw, m.src_h = sh, m.channels = 3;
  m.resize_w = rw, m.resize_h = rh;
  m.crop_x = cx, m.crop_y = cy, m.crop_w = cw, m.crop_h = ch;
  m.dst = reinterpret_cast<void*>((uintptr_t(1) << 20) + 64 * (uintptr_t)sw);
  m.dst_stride = (int64_t)cw * 3 * 2;
  m.filter = filter;
  return m;
}

int main() {
  // A mixed batch: the general kernel (packed rows of 101 pixels: not 4-byte
  // aligned), a triangle wave image, a 680 -> 40 image (34 taps: past every
  // wave bucket and band class, the general kernel again), a Catmull-Rom wave
  // image, a second wave image of the first one's shape, a 600 -> 40 image
  // (a wave kernel, or the band kernel under MXD_POLICY_PREFER_BAND).
  std::vector<mxd_image> imgs = {
      image(101, 99, 75, 70, 3, 2, 61, 33, 0, 101 * 3, 0),
      image(500, 375, 341, 256, 58, 16, 224, 224, 0, 1504, 0),
      image(680, 680, 40, 40, 0, 0, 40, 40, 0, 2048, 0),
      image(500, 375, 341, 256, 58, 16, 224, 224, 1, 1504, 0),
      image(500, 375, 341, 256, 57, 15, 223, 221, 0, 1504, 0),
      image(600, 600, 40, 40, 0, 0, 40, 40, 0, 1808, 0),
  };
  const int32_t n = (int32_t)imgs.size();
  std::vector<mxd_color> colors(n);
  for (int32_t i = 0; i < n; i++)
    for (int k = 0; k < 12; k++) colors[i].m[k / 4][k % 4] = (float)(100 * i + k);
  colors[2].m[1][2] = 1e-42f;  // stored as zero
  mxd_out_format fmt{};
  fmt.elem = MXD_ELEM_BF16;
  fmt.layout = MXD_LAYOUT_HWC;
  const LayoutEnv env = host_env(64, 4096);
  for (int pass = 0; pass < 4; pass++) {
    const mxd_out_format* f = pass & 1 ? &fmt : nullptr;
    const bool prefer_band = pass >= 2;
    mxd_set_kernel_policy(prefer_band ? MXD_POLICY_PREFER_BAND : MXD_POLICY_AUTO);
    BatchLayout L;
    CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{f, colors.data()}, &L) == MXD_OK);
    CHECK(L.pass == SecondPass::Color && L.matrix && L.entry_size() == sizeof(mxd::ColorRowDev) && L.n == n && (int32_t)L.image_of.size() == n);
    // the routes are those of a plain u8 call: all three kernel families
    CHECK(!L.plans[0].wave && !L.plans[0].band && !L.plans[2].wave && !L.plans[2].band);
    CHECK(L.general.nimgs == 2);
    if (!prefer_band) {
      CHECK(L.plans[1].wave && L.plans[3].wave && L.plans[3].s == 4 && L.plans[4].wave && L.plans[5].wave);
      CHECK(L.bands.empty() && L.waves.size() >= 3);
    } else {
      CHECK(L.plans[5].band && !L.bands.empty());
    }
    for (const auto& g : L.waves) CHECK(g.cfg.f32 == 0 && mxd::wave_has_kernel(g.cfg));
    // every image is in scratch at a 256-byte aligned offset, none overlapping
    std::vector<bool> seen(n, false);
    size_t end_max = 0;
    for (int32_t k = 0; k < n; k++) {
      const int32_t i = L.image_of[k];
      CHECK(i >= 0 && i < n && !seen[i]);
      seen[i] = true;
      const uintptr_t off = reinterpret_cast<uintptr_t>(L.descs[k].dst);
      CHECK(off % 256 == 0 && off < L.scratch_bytes);
      CHECK(L.descs[k].dst_stride % 16 == 0 && L.descs[k].dst_stride >= imgs[i].crop_w * 3);
      end_max = std::max<size_t>(end_max, off + (size_t)L.descs[k].dst_stride * imgs[i].crop_h);
      // the entry of image i reads what descriptor k writes
      const mxd::FmtRowDev& r = L.entry(i);
      CHECK(reinterpret_cast<uintptr_t>(r.src) == off && r.src_stride == L.descs[k].dst_stride);
    }
    CHECK(end_max <= L.scratch_bytes);
    // one entry per image, in batch order, with the image's own matrix and destination
    CHECK(L.fmt_count() == n);
    CHECK(L.descs.size() >= L.fmt_at + ((size_t)n * sizeof(mxd::ColorRowDev) + sizeof(ImgDev) - 1) / sizeof(ImgDev));
    int32_t blocks = 0;
    for (int32_t i = 0; i < n; i++) {
      const mxd::FmtRowDev& r = L.entry(i);
      const mxd::ColorRowDev& c = reinterpret_cast<const mxd::ColorRowDev&>(r);
      CHECK(r.dst == imgs[i].dst && r.dst_stride == imgs[i].dst_stride);
      CHECK(r.crop_w == imgs[i].crop_w && r.crop_h == imgs[i].crop_h && r.channels == 3);
      for (int k = 0; k < 12; k++) {
        const float want = i == 2 && k == 6 ? 0.0f : (float)(100 * i + k);
        CHECK(c.m[k] == want);
      }
      CHECK(r.blk_begin == blocks);
      blocks += (imgs[i].crop_h + mxd::kPixelRows - 1) / mxd::kPixelRows;
    }
    CHECK(L.fmt_blocks() == blocks);
    // scratch offsets become addresses for every descriptor and every entry
    uint8_t* base = reinterpret_cast<uint8_t*>(uintptr_t(1) << 32);
    std::vector<uintptr_t> offs(n);
    for (int32_t k = 0; k < n; k++) offs[k] = reinterpret_cast<uintptr_t>(L.descs[k].dst);
    L.add_scratch(base);
    for (int32_t k = 0; k < n; k++) {
      CHECK(L.descs[k].dst == base + offs[k]);
      CHECK(L.entry(L.image_of[k]).src == base + offs[k]);
    }
  }
  mxd_set_kernel_policy(MXD_POLICY_AUTO);
  // other matrices, other upload: the cached descriptor slot is keyed by them
  BatchLayout A, B;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, colors.data()}, &A) == MXD_OK);
  colors[4].m[2][3] += 1.0f;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{nullptr, colors.data()}, &B) == MXD_OK);
  CHECK(A.descs.size() == B.descs.size());
  CHECK(std::memcmp(A.descs.data(), B.descs.data(), A.descs.size() * sizeof(ImgDev)) != 0);
  CHECK(std::memcmp(A.descs.data(), B.descs.data(), A.fmt_at * sizeof(ImgDev)) == 0);
  // without colours the layout is the plain call's
  BatchLayout P;
  CHECK(build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, PostOps{}, &P) == MXD_OK);
  CHECK(P.pass == SecondPass::None && P.fmt_count() == 0 && P.scratch_bytes == 0 && P.descs.size() == P.fmt_at);
  std::printf("ok %d\n", g_checks);
  return 0;
}
