// planner_unit.cpp -- CPU unit tests of the fused stage's host planning
// (mlx-data_amd/csrc/plan.cpp, band_plan.cpp) and of what build_layout
// (batch_layout.cpp) assembles from it, in the device-free environment
// (host_env), through capi_internal.h, linked
// against the in-tree libmxd_amd.so; no device call.  Built and run by
// tests/test_planner_unit.py.  Prints "ok <n>" or the first failure.
#include <cmath>
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

static mxd_image center(int sw, int sh, int size, int crop, bool f32) {
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
  return m;
}

static ImgPlan plan(const mxd_image& m) {
  ImgPlan p;
  CHECK(host_tables().get(0, m.src_w, m.resize_w, &p.xt) == MXD_OK);
  CHECK(host_tables().get(0, m.src_h, m.resize_h, &p.yt) == MXD_OK);
  return p;
}

// band_rows: the fewest "rounds" of `capacity` units whose band height stays
// within the cap, units never above rounds * capacity, at least one row.
static void test_band_rows() {
  auto units = [](const std::vector<std::pair<int32_t, int32_t>>& s, int32_t ty) {
    int64_t u = 0;
    for (auto& x : s) u += (int64_t)x.first * ((x.second + std::min(ty, x.second) - 1) / std::min(ty, x.second));
    return u;
  };
  const std::vector<std::pair<int32_t, int32_t>> c2(256, {1, 224});
  CHECK(band_rows(c2, 1024, 64) == 56);  // one round: 4 bands x 256 images
  CHECK(units(c2, 56) == 1024);
  CHECK(band_rows(c2, 1024, 16) == 14);  // 4 rounds of 16 bands
  CHECK(units(c2, 14) == 4096);
  for (int cap : {1, 7, 100, 1024, 4096})
    for (int mx : {8, 16, 64, 128}) {
      std::vector<std::pair<int32_t, int32_t>> mixed;
      for (int i = 0; i < 37; i++) mixed.push_back({1 + i % 3, 1 + (i * 53) % 400});
      const int32_t ty = band_rows(mixed, cap, mx);
      CHECK(ty >= 1);
      const int64_t u = units(mixed, ty);
      const int64_t rounds = (u + cap - 1) / cap;
      CHECK(ty <= std::max(mx, 8) || ty >= 400);
      // no smaller height fits the same rounds
      if (ty > 8) CHECK(units(mixed, ty - 1) > rounds * cap || ty - 1 < 8);
    }
}

// plan_wave: C2 takes a scatter wave kernel; a 12 MP photo takes the 24-tap
// bucket with a depth-12 schedule, a 48 MP one (31:1) none.
static void test_plan_wave() {
  const mxd_image c2 = center(1280, 960, 256, 224, true);
  ImgPlan p = plan(c2);
  plan_wave(c2, whole(c2), MXD_F32_DIV255, p);
  CHECK(p.wave);
  CHECK(p.kind == 2);  // scatter
  CHECK(p.s == 2 && p.dmax == 4);
  CHECK(p.nstrips >= 1 && p.tx * p.nstrips >= 224);
  const mxd_image big = center(4032, 3024, 256, 224, true);
  ImgPlan q = plan(big);
  plan_wave(big, whole(big), MXD_F32_DIV255, q);
  CHECK(q.wave && q.kind == 2 && q.bucket == 24 && q.dmax == 12 && q.s == 2);
  const mxd_image huge = center(8000, 6000, 256, 224, true);
  ImgPlan h = plan(huge);
  plan_wave(huge, whole(huge), MXD_F32_DIV255, h);
  CHECK(!h.wave);
  // an odd row stride leaves the wave kernels (4-byte aligned rows only)
  mxd_image odd = c2;
  odd.src_stride = 1280 * 3 + 1;
  ImgPlan r = plan(odd);
  plan_wave(odd, whole(odd), MXD_F32_DIV255, r);
  CHECK(!r.wave);
}

// plan_band + band_schedule: class, strips, and a schedule whose groups bring
// every tap row of every output row exactly once per band, complete the rows
// in order, and carry each row's weights.
static void test_band_schedule(int sw, int sh, int ty) {
  const mxd_image m = center(sw, sh, 256, 224, true);
  ImgPlan p = plan(m);
  plan_band(m, whole(m), MXD_F32_DIV255, p);
  CHECK(p.band);
  const mxd::AxisView yv = axis_view(*p.yt);
  std::vector<int32_t> w;
  int32_t bw = 0;
  const int32_t min_groups = p.bp.la + 2;
  CHECK(mxd::band_schedule(yv, m.crop_y, m.crop_h, ty, p.bp.db, p.bp.s, min_groups, &w, &bw));
  const int E = mxd::kBandEntryWords, gw = (1 + p.bp.db) * E;
  const int nb = (m.crop_h + ty - 1) / ty;
  CHECK((int64_t)w.size() == (int64_t)nb * bw);
  for (int b = 0; b < nb; b++) {
    const int32_t* band = w.data() + (size_t)b * bw;
    const int ng = band[0];
    CHECK(ng >= min_groups && E + ng * gw <= bw);
    const int y0 = b * ty, n = std::min(ty, m.crop_h - y0);
    std::vector<double> sum(n, 0.0);
    std::vector<int> seen(n, 0);
    int done = 0;
    for (int g = 0; g < ng; g++) {
      const int32_t* gr = band + E + g * gw;
      for (int j = 0; j < p.bp.db; j++) {
        const int32_t* e = gr + (1 + j) * E;
        if (e[0] < 0) continue;
        for (int s = 0; s < p.bp.s; s++) {
          float wt;
          std::memcpy(&wt, &e[1 + s], 4);
          if (wt == 0.0f) continue;
          const int u = done + s;
          CHECK(u < n);
          const int r = e[0], f = yv.first[m.crop_y + y0 + u];
          CHECK(r >= f && r < f + yv.count[m.crop_y + y0 + u]);
          CHECK(wt == yv.w[(size_t)(m.crop_y + y0 + u) * yv.width + (r - f)]);
          sum[u] += wt;
          seen[u]++;
        }
      }
      if (gr[0] & mxd::kBandRowDone) done++;
    }
    CHECK(done == n);
    for (int u = 0; u < n; u++) {
      // nonzero taps of the row, each once
      int nz = 0;
      for (int k = 0; k < yv.count[m.crop_y + y0 + u]; k++)
        nz += yv.w[(size_t)(m.crop_y + y0 + u) * yv.width + k] != 0.0f;
      CHECK(seen[u] == nz);
      CHECK(std::fabs(sum[u] - 1.0) < 1e-4);
    }
  }
}

// scatter_schedule_words, with the shape plan_wave picks: every nonzero tap of
// every output row of every band once, with its weight, in an accumulator
// slot < S; loaded rows inside the band's tap rows; weights summing to 1;
// word 0 of an iteration = the row loaded `la` iterations later.
static void test_scatter_schedule(int sw, int sh, int ty) {
  const mxd_image m = center(sw, sh, 256, 224, true);
  ImgPlan p = plan(m);
  plan_wave(m, whole(m), MXD_F32_DIV255, p);
  CHECK(p.wave && p.kind == 2);
  const ScatterShape shape{p.s, p.dmax, p.p, p.pp == 16 ? 16 : p.pp * 3};
  const int S = shape.s, D = shape.dmax, P = shape.p, E = mxd::scatter_entry_words(S);
  const int la = mxd::scatter_ring_slots(D, shape.lane_bytes) - 1;
  std::vector<int32_t> w;
  int32_t bw = 0, eo = 0;
  CHECK(scatter_schedule_words(*p.yt, m.crop_y, m.crop_h, ty, shape, &w, &bw, &eo));
  const DevTable& yt = *p.yt;
  const int nb = (m.crop_h + ty - 1) / ty, iters = (bw - eo) / E;
  CHECK(S <= E - 2 && (bw - eo) % E == 0 && (int64_t)w.size() == (int64_t)nb * bw);
  auto first = [&](int y) { return yt.first[m.crop_y + y]; };
  auto last = [&](int y) { return yt.first[m.crop_y + y] + yt.count[m.crop_y + y] - 1; };
  for (int b = 0; b < nb; b++) {
    const int32_t* band = w.data() + (size_t)b * bw;
    const int32_t* ent = band + eo;
    const int y0 = b * ty, n = std::min(ty, m.crop_h - y0);
    CHECK(band[0] >= P + n && band[0] * D + la <= iters);
    // group g completes output row g - P of the band
    for (int g = 0; g < band[0]; g++) CHECK(band[1 + g] == (g >= P && g - P < n ? y0 + g - P : -1));
    std::vector<double> sum(n, 0.0);
    std::vector<int> seen(n, 0);
    for (int i = 0; i < iters; i++) {
      const int32_t* e = ent + (size_t)i * E;
      CHECK(e[0] == (i + la < iters ? ent[(size_t)(i + la) * E + 1] : -1));
      const int r = e[1], g = i / D;
      if (r < 0) {
        for (int k = 2; k < E; k++) CHECK(e[k] == 0);
        continue;
      }
      CHECK(r >= first(y0) && r <= last(y0 + n - 1));
      for (int k = 0; k < E - 2; k++) {
        float wt;
        std::memcpy(&wt, &e[2 + k], 4);
        if (wt == 0.0f) continue;
        CHECK(k < S);
        const int u = g - P + k;
        CHECK(u >= 0 && u < n);
        CHECK(r >= first(y0 + u) && r <= last(y0 + u));
        CHECK(wt == yt.w[(size_t)(m.crop_y + y0 + u) * yt.width + (r - first(y0 + u))]);
        sum[u] += wt;
        seen[u]++;
      }
    }
    for (int u = 0; u < n; u++) {
      int nz = 0;
      for (int k = 0; k < yt.count[m.crop_y + y0 + u]; k++)
        nz += yt.w[(size_t)(m.crop_y + y0 + u) * yt.width + k] != 0.0f;
      CHECK(seen[u] == nz);
      CHECK(std::fabs(sum[u] - 1.0) < 1e-4);
    }
  }
}

// The mixed RGB batch of the layout tests: every wave or band group gets at
// least two images.  Distinct addresses, as a caller's buffers have.
static std::vector<mxd_image> mixed_batch(bool f32) {
  std::vector<mxd_image> v;
  auto add = [&](mxd_image m, int src_shift = 0) {
    m.src = reinterpret_cast<const uint8_t*>(((uintptr_t)(v.size() + 1) << 28) + src_shift);
    m.dst = reinterpret_cast<void*>(((uintptr_t)(v.size() + 1) << 28) + ((uintptr_t)1 << 27));
    v.push_back(m);
  };
  for (int rep = 0; rep < 2; rep++) {
    add(center(1280, 960, 256, 224, f32));   // C2: scatter
    add(center(640, 480, 256, 224, f32));    // narrow lanes
    add(center(300, 200, 256, 224, f32));    // 2-tap bucket
    add(center(200, 150, 512, 448, f32));    // upsampling: a gather wave kernel under either policy
    add(center(1280, 960, 256, 224, f32), 1);  // a base off the 4-byte grid: the band kernel under either policy
    add(center(4032, 3024, 256, 224, f32));  // 24-tap bucket
    mxd_image crop = center(6000, 4000, 256, 64, f32);  // PREFER_BAND: band kernel
    add(crop);
    crop.crop_h = 40 + 16 * rep;  // one group, two unit counts: a unit table
    add(crop);
  }
  mxd_image odd = center(1280, 960, 256, 224, f32);
  odd.src_stride = 1280 * 3 + 1;  // no 4-byte aligned rows: general kernel
  add(odd);
  return v;
}

static int units_of(const ImgDev& d) { return d.nstrips * ((d.crop_h + d.ty - 1) / d.ty); }

// What build_layout assembles from the planner's leaves.  Returns the number
// of (band groups, band groups with a unit table, wave groups, general images).
static std::array<int, 4> check_layout(const BatchLayout& L, const std::vector<mxd_image>& imgs, bool formatted) {
  const int n = (int)imgs.size();
  CHECK(L.n == n && (int)L.plans.size() == n && (int)L.image_of.size() == n && L.tables_at == (size_t)n);
  std::vector<int> hit(n, 0);
  for (int k = 0; k < n; k++) hit[L.image_of[k]]++;
  for (int i = 0; i < n; i++) CHECK(hit[i] == 1);
  // band, then wave, then general; groups contiguous, one per kernel key, batch order inside
  int at = 0;
  auto bkey = [&](int k) {
    const mxd::BandPlan& b = L.plans[L.image_of[k]].bp;
    return std::make_tuple(b.cls, b.nq, b.la);
  };
  auto wkey = [&](int k) {
    const ImgPlan& p = L.plans[L.image_of[k]];
    return std::make_tuple(p.kind, p.bucket, p.s, p.dmax, p.q, p.shift, p.pp, p.ycc);
  };
  auto check_group = [&](int first, int count, int units, int nunits, int nimgs, int per_img, int ty_cap) {
    CHECK(first == at && count >= 1 && nimgs == count);
    int sum = 0, same = -1;
    // one unit height per group, cut to each image's rows (band groups: the tallest unit's)
    for (int k = first; k < first + count && ty_cap <= 0; k++) ty_cap = std::max(ty_cap, L.descs[k].ty);
    for (int k = first; k < first + count; k++) {
      const ImgDev& d = L.descs[k];
      const mxd_image& im = imgs[L.image_of[k]];
      if (k > first) CHECK(L.image_of[k] > L.image_of[k - 1]);
      CHECK(d.tile_begin == sum);
      CHECK(d.crop_h == im.crop_h && d.crop_w == im.crop_w && d.ty >= 1 && d.ty <= im.crop_h);
      CHECK(d.ty == std::min(ty_cap, im.crop_h));
      // the 4-byte aligned base, its byte shift in flip bits 8 and up
      CHECK((reinterpret_cast<uintptr_t>(d.src) & 3) == 0 && d.src + (d.flip >> 8) == im.src && (d.flip >> 8) < 4);
      CHECK((d.flip & 1) == (im.flip ? 1 : 0));
      if (!formatted) CHECK(d.dst == im.dst && d.dst_stride == im.dst_stride);
      same = k == first ? units_of(d) : (same == units_of(d) ? same : 0);
      sum += units_of(d);
    }
    CHECK(units == sum && nunits == sum && per_img == same);
    at += count;
  };
  int ntables = 0, table_words = 0;
  for (size_t gi = 0; gi < L.bands.size(); gi++) {
    const BatchLayout::BandGroup& g = L.bands[gi];
    check_group(g.first, g.count, g.units, g.cfg.nunits, g.cfg.nimgs, g.cfg.per_img, 0);
    for (int k = g.first; k < g.first + g.count; k++) {
      const ImgPlan& p = L.plans[L.image_of[k]];
      CHECK(p.band && bkey(k) == bkey(g.first) && L.descs[k].nstrips == p.bp.nstrips && L.descs[k].tx == p.bp.tx);
    }
    if (gi > 0) CHECK(bkey(L.bands[gi - 1].first) < bkey(g.first));
    CHECK(g.cfg.grid >= 1 && g.cfg.grid <= g.units);
    CHECK((g.cfg.per_img == 0) == (g.table >= 0));
    if (g.table < 0) continue;
    // the unit table names image j units_of(j) times, then zeros to a whole ImgDev block
    CHECK(g.table == table_words);
    const int32_t* t = L.unit_tables() + g.table;
    int w = 0;
    for (int k = g.first; k < g.first + g.count; k++)
      for (int u = 0; u < units_of(L.descs[k]); u++) CHECK(t[w++] == k - g.first);
    const int block = sizeof(ImgDev) / 4;
    for (; w % block; w++) CHECK(t[w] == 0);
    table_words += w;
    ntables++;
  }
  for (size_t gi = 0; gi < L.waves.size(); gi++) {
    const BatchLayout::WaveGroup& g = L.waves[gi];
    check_group(g.first, g.count, g.units, g.cfg.nunits, g.cfg.nimgs, g.cfg.per_img, g.ty);
    for (int k = g.first; k < g.first + g.count; k++) {
      const ImgPlan& p = L.plans[L.image_of[k]];
      CHECK(p.wave && !p.band && wkey(k) == wkey(g.first) && L.descs[k].nstrips == p.nstrips && L.descs[k].tx == p.tx);
    }
    if (gi > 0) CHECK(wkey(L.waves[gi - 1].first) < wkey(g.first));
    CHECK((g.cfg.f32 == mxd::kWaveOutFmt) == formatted && g.cfg.kind == L.plans[L.image_of[g.first]].kind);
  }
  CHECK(L.general_at == at && L.general.nimgs == n - at);
  int tiles = 0;
  for (int k = at; k < n; k++) {
    const ImgPlan& p = L.plans[L.image_of[k]];
    CHECK(!p.band && !p.wave && L.descs[k].tile_begin == tiles);
    if (k > at) CHECK(L.image_of[k] > L.image_of[k - 1]);
    tiles += units_of(L.descs[k]);
  }
  CHECK(L.general.ntiles == tiles);
  CHECK((size_t)table_words * 4 == (L.fmt_at - L.tables_at) * sizeof(ImgDev));
  // launch order: every launch once, by units descending (a band unit counts 4), ties in
  // the order band groups, wave groups, general
  CHECK(L.launches.size() == L.bands.size() + L.waves.size() + (n > at ? 1 : 0));
  std::vector<int> launched(L.launches.size(), 0);
  for (size_t k = 0; k < L.launches.size(); k++) {
    const BatchLayout::Launch& l = L.launches[k];
    const int64_t u = l.kind == 0 ? 4 * (int64_t)L.bands[l.group].units : l.kind == 1 ? L.waves[l.group].units : tiles;
    CHECK(l.units == u);
    const size_t id = l.kind == 0 ? l.group : l.kind == 1 ? L.bands.size() + l.group : L.launches.size() - 1;
    CHECK(id < launched.size() && launched[id]++ == 0);
    if (k > 0) {
      const BatchLayout::Launch& q = L.launches[k - 1];
      CHECK(q.units > l.units || (q.units == l.units && std::make_pair(q.kind, q.group) < std::make_pair(l.kind, l.group)));
    }
  }
  return {(int)L.bands.size(), ntables, (int)L.waves.size(), n - at};
}

static void test_layout(bool f32) {
  const std::vector<mxd_image> imgs = mixed_batch(f32);
  const int32_t dtype = f32 ? MXD_F32_DIV255 : MXD_U8;
  const LayoutEnv env = host_env(1024, 7);
  BatchLayout L;
  CHECK(build_layout(env, 0, imgs.data(), (int32_t)imgs.size(), nullptr, dtype, nullptr, &L) == MXD_OK);
  const std::array<int, 4> a = check_layout(L, imgs, false);
  // the shifted pair on the band kernel, the other pairs on five wave kernels at least, the odd stride general
  CHECK(a[0] >= 1 && a[2] >= 5 && a[3] == 1);
  for (const BatchLayout::BandGroup& g : L.bands) CHECK(g.count >= 2);
  for (const BatchLayout::WaveGroup& g : L.waves) CHECK(g.count >= 2);
  int kinds[3] = {0, 0, 0};
  for (const BatchLayout::WaveGroup& g : L.waves) kinds[g.cfg.kind]++;
  CHECK(kinds[0] >= 1 && kinds[2] >= 2);  // gather and scatter
  const int32_t before = mxd_set_kernel_policy(MXD_POLICY_PREFER_BAND);
  BatchLayout B;
  CHECK(build_layout(env, 0, imgs.data(), (int32_t)imgs.size(), nullptr, dtype, nullptr, &B) == MXD_OK);
  mxd_set_kernel_policy(before);
  const std::array<int, 4> b = check_layout(B, imgs, false);
  CHECK(b[0] >= 4 && b[1] >= 1 && b[2] >= 1 && b[3] == 1);  // band groups, one with a unit table
  for (const BatchLayout::BandGroup& g : B.bands) CHECK(g.count >= 2);
  for (const BatchLayout::WaveGroup& g : B.waves) CHECK(g.count >= 2);
  // gather kernels have no schedule: group 1, the vertical tap table
  for (const BatchLayout::WaveGroup& g : B.waves)
    if (g.cfg.kind == 0) CHECK(B.descs[g.first].group == 1 && B.descs[g.first].ywidth == B.plans[B.image_of[g.first]].yt->padded);
  for (int k = 0; k < B.n; k++)
    if (imgs[B.image_of[k]].src_w == 6000) CHECK(B.plans[B.image_of[k]].band);
  // the device-free form: table and schedule pointers are null plus their offsets
  for (int k = 0; k < L.n; k++) {
    const mxd_image& im = imgs[L.image_of[k]];
    CHECK(reinterpret_cast<uintptr_t>(L.descs[k].xtab) == (size_t)im.crop_x * (mxd::kTapHeader + L.descs[k].xwidth) * 4);
  }
}

// A formatted call (f16 CHW) of the same batch: wave images keep the caller's
// destinations, the others get scratch rows and a format_rows entry.
static void test_layout_formatted(int32_t policy) {
  std::vector<mxd_image> imgs = mixed_batch(false);
  mxd_out_format fmt{};
  fmt.elem = MXD_ELEM_F16;
  fmt.layout = MXD_LAYOUT_CHW;
  fmt.plane_stride = 224 * 224 * 2;
  for (mxd_image& m : imgs) m.dst_stride = m.crop_w * 2;
  const int32_t before = mxd_set_kernel_policy(policy);
  BatchLayout L;
  CHECK(build_layout(host_env(1024, 7), 0, imgs.data(), (int32_t)imgs.size(), nullptr, MXD_U8, &fmt, &L) == MXD_OK);
  mxd_set_kernel_policy(before);
  check_layout(L, imgs, true);
  const int n = L.n;
  std::vector<std::pair<size_t, size_t>> ranges;  // scratch (offset, size) by batch index order
  std::vector<const ImgDev*> desc_of(n);
  for (int k = 0; k < n; k++) desc_of[L.image_of[k]] = &L.descs[k];
  size_t need = 0;
  int rows = 0, blocks = 0;
  CHECK(L.fmt_at >= L.tables_at && L.fmt_at <= L.descs.size());
  for (int i = 0; i < n; i++) {
    const ImgDev& d = *desc_of[i];
    if (L.plans[i].wave) {
      CHECK(d.dst == imgs[i].dst && d.dst_stride == imgs[i].dst_stride);
      continue;
    }
    const size_t off = reinterpret_cast<uintptr_t>(d.dst);
    const size_t size = ((size_t)d.dst_stride * d.crop_h + 255) & ~(size_t)255;
    CHECK(d.dst_stride % 16 == 0 && d.dst_stride >= (int64_t)d.crop_w * 3 && off % 256 == 0);
    for (auto& r : ranges) CHECK(off >= r.first + r.second || off + size <= r.first);
    ranges.push_back({off, size});
    need += size;
    CHECK(rows < L.fmt_count());
    const mxd::FmtRowDev& e = L.entry(rows++);
    CHECK(e.src == d.dst && e.src_stride == d.dst_stride && e.dst == imgs[i].dst && e.dst_stride == imgs[i].dst_stride);
    CHECK(e.crop_w == d.crop_w && e.crop_h == d.crop_h && e.channels == 3 && e.blk_begin == blocks);
    blocks += (d.crop_h + mxd::kFmtRows - 1) / mxd::kFmtRows;
  }
  CHECK(rows == L.fmt_count() && blocks == L.fmt_blocks() && need == L.scratch_bytes);
  for (auto& r : ranges) CHECK(r.first + r.second <= need);
  CHECK(rows >= 1);
  CHECK(L.descs.size() == L.fmt_at + ((size_t)rows * sizeof(mxd::FmtRowDev) + sizeof(ImgDev) - 1) / sizeof(ImgDev));
  // add_scratch turns the offsets into addresses
  uint8_t* const base = reinterpret_cast<uint8_t*>((uintptr_t)1 << 40);
  const uintptr_t off0 = reinterpret_cast<uintptr_t>(L.entry(0).src);
  L.add_scratch(base);
  CHECK(L.entry(0).src == base + off0);
  for (int i = 0; i < n; i++) CHECK(L.plans[i].wave ? desc_of[i]->dst == imgs[i].dst : desc_of[i]->dst >= (void*)base);
}

// split_batch: one sub-batch per channel count in ascending order, RGBA split
// by alpha mode (weighted first), batch order inside, stored entries following.
static void test_split_batch() {
  const int chans[] = {1, 3, 4, 3, 1, 4, 4};
  const int weighted[] = {0, 1, 0, 0, 1, 1, 0};
  std::vector<mxd_image> imgs;
  std::vector<Stored> stored;
  for (int i = 0; i < 7; i++) {
    mxd_image m = center(640, 480, 256, 224, false);
    m.channels = chans[i];
    m.rgba_weighted = weighted[i];
    m.src_w = 100 + i;  // tags the image
    imgs.push_back(m);
    stored.push_back(Stored{nullptr, 0, i, 0, 0});
  }
  auto tags = [](const SubBatch& s) {
    std::vector<int> t;
    for (size_t k = 0; k < s.images.size(); k++) {
      CHECK(s.stored.size() == s.images.size() && s.stored[k].x0 == s.images[k].src_w - 100);
      t.push_back(s.images[k].src_w - 100);
    }
    return t;
  };
  // 1, 3, 4, 3, 1 with one alpha mode among the RGBA images
  std::vector<SubBatch> s = split_batch(imgs.data(), 5, stored.data());
  CHECK(s.size() == 3 && tags(s[0]) == std::vector<int>({0, 4}) && tags(s[1]) == std::vector<int>({1, 3}) &&
        tags(s[2]) == std::vector<int>({2}));
  // both alpha modes: weighted RGBA first
  s = split_batch(imgs.data(), 7, stored.data());
  CHECK(s.size() == 4 && tags(s[0]) == std::vector<int>({0, 4}) && tags(s[1]) == std::vector<int>({1, 3}) &&
        tags(s[2]) == std::vector<int>({5}) && tags(s[3]) == std::vector<int>({2, 6}));
  // RGBA only, both modes; and without stored entries
  s = split_batch(imgs.data() + 5, 2, nullptr);
  CHECK(s.size() == 2 && s[0].stored.empty() && s[0].images[0].src_w == 105 && s[1].images[0].src_w == 106);
  // launchable as it is: nothing to split (rgba_weighted means nothing below four channels)
  CHECK(split_batch(imgs.data() + 5, 1, nullptr).empty());
  const mxd_image rgb[2] = {imgs[1], imgs[3]};
  CHECK(split_batch(rgb, 2, nullptr).empty());
}

int main() {
  test_band_rows();
  test_plan_wave();
  test_split_batch();
  for (int ty : {1, 8, 14, 56, 224}) {
    test_scatter_schedule(1280, 960, ty);
    test_scatter_schedule(4032, 3024, ty);
    test_scatter_schedule(6000, 4000, ty);
  }
  for (bool f32 : {false, true}) test_layout(f32);
  test_layout_formatted(MXD_POLICY_AUTO);
  test_layout_formatted(MXD_POLICY_PREFER_BAND);
  for (int ty : {1, 3, 8, 14, 16, 224}) {
    test_band_schedule(1280, 960, ty);   // 3.75:1, one group per row
    test_band_schedule(4032, 3024, ty);  // 11.8:1, two groups per row
    test_band_schedule(6000, 4000, ty);  // 15.6:1
    test_band_schedule(300, 200, ty);    // upsampling, rows with no new source row
  }
  std::printf("ok %d\n", g_checks);
  return 0;
}
