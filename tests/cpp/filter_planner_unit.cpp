// filter_planner_unit.cpp -- CPU unit tests of the host planner for the
// resize filters (mlx-data_amd/csrc/plan.cpp, batch_layout.cpp), in the
// device-free environment (host_env) through capi_internal.h, linked against
// the in-tree libmxd_amd.so; no device call.  Built and run by
// tests/test_filters.py.  Prints "ok <n>" or the first failure.
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

static mxd_image center(int sw, int sh, int size, int crop, bool f32, int filter) {
  mxd_image m{};
  int64_t rw = 0, rh = 0, cx = 0, cy = 0;
  mxd_resize_smallest_side_dims(sw, sh, size, &rw, &rh);
  mxd_center_crop_origin(rw, rh, crop, crop, &cx, &cy);
  static uint8_t dummy[64];
  m.src = dummy;
  m.src_stride = ((int64_t)sw * 3 + 15) / 16 * 16;
  m.src_w = sw;
  m.src_h = sh;
  m.channels = 3;
  m.resize_w = (int32_t)rw;
  m.resize_h = (int32_t)rh;
  m.crop_x = (int32_t)cx;
  m.crop_y = (int32_t)cy;
  m.crop_w = crop;
  m.crop_h = crop;
  m.dst = reinterpret_cast<void*>(uintptr_t(1) << 20);
  m.dst_stride = (int64_t)crop * 3 * (f32 ? 4 : 1);
  m.filter = filter;
  return m;
}

static ImgPlan plan(const mxd_image& m) {
  ImgPlan p;
  CHECK(host_tables().get(0, m.src_w, m.resize_w, &p.xt, m.filter) == MXD_OK);
  CHECK(host_tables().get(0, m.src_h, m.resize_h, &p.yt, m.filter) == MXD_OK);
  return p;
}

// Filter 0 through the defaulted table lookup and through the field: the
// plans planner_unit.cpp pins (C2 scatter S 2 / DMAX 4, 12 MP the 24-tap
// bucket at depth 12, 48 MP no wave kernel), from the same table objects.
static void test_triangle_unchanged() {
  const mxd_image c2 = center(1280, 960, 256, 224, true, 0);
  ImgPlan p;
  CHECK(host_tables().get(0, c2.src_w, c2.resize_w, &p.xt) == MXD_OK);
  CHECK(host_tables().get(0, c2.src_h, c2.resize_h, &p.yt) == MXD_OK);
  const ImgPlan named = plan(c2);
  CHECK(named.xt == p.xt && named.yt == p.yt && p.yt->filter == 0);
  plan_wave(c2, whole(c2), MXD_F32_DIV255, p);
  CHECK(p.wave && p.kind == 2 && p.s == 2 && p.dmax == 4);
  const mxd_image big = center(4032, 3024, 256, 224, true, 0);
  ImgPlan q = plan(big);
  plan_wave(big, whole(big), MXD_F32_DIV255, q);
  CHECK(q.wave && q.kind == 2 && q.bucket == 24 && q.dmax == 12 && q.s == 2);
  const mxd_image huge = center(8000, 6000, 256, 224, true, 0);
  ImgPlan h = plan(huge);
  plan_wave(huge, whole(huge), MXD_F32_DIV255, h);
  CHECK(!h.wave);
  // A triangle window whose scatter shape has four slots (an upscale, rows
  // 91..163 of 167 -> 256) keeps the gather kernel: the S = 4 scatter kernels
  // are the cubic filters' alone, also for a JPEG plane source (none at all).
  mxd_image up = center(417, 167, 256, 224, false, 0);
  up.resize_w = 639, up.resize_h = 256, up.crop_x = 305, up.crop_y = 91, up.crop_w = 28, up.crop_h = 73;
  up.dst_stride = 28 * 3;
  ImgPlan u = plan(up);
  CHECK(scatter_shape(*u.yt, up.crop_y, up.crop_h).s == 4);
  plan_wave(up, whole(up), MXD_U8, u);
  CHECK(u.wave && u.kind == 0 && u.bucket == 2);
  mxd::YccDev ycc{};
  Stored planes = whole(up);
  planes.ycc = &ycc;
  ImgPlan y = plan(up);
  plan_wave(up, planes, MXD_U8, y);
  CHECK(!y.wave);
}

// Cubic tables are objects of their own, the identity axis is shared, and an
// unknown filter is refused.
static void test_tables(int filter) {
  const DevTable *t0 = nullptr, *tf = nullptr, *i0 = nullptr, *ifl = nullptr;
  CHECK(host_tables().get(0, 960, 256, &t0) == MXD_OK);
  CHECK(host_tables().get(0, 960, 256, &tf, filter) == MXD_OK);
  CHECK(t0 != tf && tf->filter == filter && tf->width == 15 && t0->width == 8);
  CHECK(host_tables().get(0, 256, 256, &i0) == MXD_OK);
  CHECK(host_tables().get(0, 256, 256, &ifl, filter) == MXD_OK);
  CHECK(i0 == ifl && i0->width == 1);
  CHECK(host_tables().get(0, 960, 256, &tf, 99) == MXD_ERR_INVALID);
  // the footprint of the same window is wider than the triangle's
  CHECK(tf != nullptr);
  const DevTable* c = nullptr;
  CHECK(host_tables().get(0, 960, 256, &c, filter) == MXD_OK);
  CHECK(c->first[100] < t0->first[100] && c->first[100] + c->count[100] > t0->first[100] + t0->count[100]);
}

// Cubic C2 and C4 shapes take a scatter wave kernel with four accumulator
// slots, in the u8 and f32 modes; upsampling the 4-tap gather kernel; a
// 2160 -> 256 image (34 taps) no wave kernel and, with no band class of four
// slots, the general kernel.
static void test_cubic_routes(int filter) {
  for (bool f32 : {false, true}) {
    const int32_t dt = f32 ? MXD_F32_DIV255 : MXD_U8;
    const mxd_image c2 = center(1280, 960, 256, 224, f32, filter);
    ImgPlan p = plan(c2);
    plan_wave(c2, whole(c2), dt, p);
    CHECK(p.wave && p.kind == 2 && p.s == 4 && p.dmax == 4 && p.bucket == 17);
    CHECK(mxd::wave_has_kernel(mxd::WaveCfg{3, f32 ? 1 : 0, p.bucket, 0, 0, 2, p.s, p.dmax, p.q, p.shift, p.pp}));
    for (int sw : {500, 333}) {
      const mxd_image c4 = sw == 500 ? center(500, 375, 256, 224, f32, filter) : center(333, 500, 256, 224, f32, filter);
      ImgPlan q = plan(c4);
      plan_wave(c4, whole(c4), dt, q);
      CHECK(q.wave && q.kind == 2 && q.s == 4 && q.dmax == 2 && q.bucket == 6);
    }
    const mxd_image up = center(300, 200, 256, 224, f32, filter);
    ImgPlan u = plan(up);
    plan_wave(up, whole(up), dt, u);
    CHECK(u.wave && u.kind == 0 && u.bucket == 4);
    const mxd_image far = center(3840, 2160, 256, 224, f32, filter);
    ImgPlan h = plan(far);
    CHECK(h.yt->width == 34);
    plan_wave(far, whole(far), dt, h);
    CHECK(!h.wave);
    plan_band(far, whole(far), dt, h);
    CHECK(!h.band);
  }
}

// build_layout of a mixed batch: triangle and cubic images of one geometry
// plan apart (the filter is part of the plan key) and launch as two wave
// groups; a formatted call keeps the triangle image on its wave kernel and
// sends the cubic one through u8 scratch rows (format_rows); the schedules of
// two cubic filters with one shape are different objects.
static void test_layout() {
  mxd_image imgs[3] = {center(1280, 960, 256, 224, false, 0), center(1280, 960, 256, 224, false, 1),
                       center(1280, 960, 256, 224, false, 2)};
  const LayoutEnv env = host_env(64, 4096);
  BatchLayout L;
  CHECK(build_layout(env, 0, imgs, 3, nullptr, MXD_U8, nullptr, &L) == MXD_OK);
  CHECK(L.plans[0].wave && L.plans[0].s == 2 && L.plans[1].wave && L.plans[1].s == 4 && L.plans[2].s == 4);
  CHECK(L.waves.size() == 2 && L.bands.empty() && L.general.nimgs == 0);
  CHECK(L.plans[1].yt != L.plans[2].yt);
  for (const auto& g : L.waves) CHECK(mxd::wave_has_kernel(g.cfg));
  // every cubic schedule row is reached: the descriptors carry schedules of S = 4 entries
  mxd_out_format fmt{};
  fmt.elem = MXD_ELEM_BF16;
  fmt.layout = MXD_LAYOUT_HWC;
  for (auto& m : imgs) m.dst_stride = 224 * 3 * 2;
  BatchLayout F;
  CHECK(build_layout(env, 0, imgs, 3, nullptr, MXD_U8, &fmt, &F) == MXD_OK);
  CHECK(F.plans[0].wave && !F.plans[1].wave && !F.plans[2].wave);
  CHECK(F.fmt_count() == 2 && F.scratch_bytes > 0);
  // large sources: triangle groups take streaming loads, cubic groups the default policy
  std::vector<mxd_image> many(400, center(1280, 960, 256, 224, false, 0));
  for (size_t i = 200; i < many.size(); i++) many[i].filter = 1;
  BatchLayout M;
  CHECK(build_layout(env, 0, many.data(), (int32_t)many.size(), nullptr, MXD_U8, nullptr, &M) == MXD_OK);
  CHECK(M.waves.size() == 2);
  for (const auto& g : M.waves) {
    CHECK(g.cfg.nt == (g.cfg.s == 2 ? 1 : 0));
    CHECK(mxd::wave_has_kernel(g.cfg));
  }
}

int main() {
  test_triangle_unchanged();
  for (int f = 1; f <= 3; f++) {
    test_tables(f);
    test_cubic_routes(f);
  }
  test_layout();
  std::printf("ok %d\n", g_checks);
  return 0;
}
