// batch_layout.cpp -- build_layout (capi_internal.h): the plans, descriptors,
// launch groups and launch order of one launchable batch.  No device call of
// its own: tables, schedules and capacities come through the LayoutEnv.
#include "capi_internal.h"

namespace mxd {
namespace capi {
namespace {

// A call whose wave-kernel sources total at least this many bytes loads them
// with the streaming (nt) policy (half the 256 MB Infinity Cache).
constexpr int64_t kNtSourceBytes = (int64_t)128 << 20;

// A u8 scratch image's rows: 16-byte aligned, so the band and general
// kernels plan it as they plan an aligned destination.
int64_t scratch_stride(const mxd_image& im) { return ((int64_t)im.crop_w * im.channels + 15) & ~(int64_t)15; }
size_t scratch_size(const mxd_image& im) { return (size_t)(im.dst_stride * im.crop_h + 255) & ~(size_t)255; }

// One build_layout call.
struct Batch {
  const LayoutEnv& env;
  int32_t device;
  const mxd_image* images;  // formatted call: L.images
  const Stored* stored;
  int32_t n, channels, out_dtype;
  bool formatted;
  BatchLayout& L;
  // Images of one geometry, layout and alignment share a plan and a
  // schedule: rep[i] = the first image with image i's key.
  std::vector<int32_t> rep;
  Stored at(int32_t i) const { return stored ? stored[i] : whole(images[i]); }
  int32_t f32() const { return out_dtype == MXD_F32_DIV255 ? 1 : 0; }
};

// Planning walks tap tables, and a batch rarely holds more than a few shapes.
int plan_images(Batch& b) {
  const bool no_wave = (g_policy.load() & MXD_POLICY_NO_WAVE) != 0;
  b.L.plans.assign(b.n, ImgPlan{});
  b.rep.resize(b.n);
  std::unordered_map<PlanKey, int32_t, PlanKeyHash> first_of;
  first_of.reserve(16);
  for (int32_t i = 0; i < b.n; i++) {
    const mxd_image& im = b.images[i];
    const Stored st = b.at(i);
    const auto ins = first_of.emplace(plan_key(im, st), i);
    b.rep[i] = ins.first->second;
    ImgPlan& p = b.L.plans[i];
    if (!ins.second) {
      p = b.L.plans[b.rep[i]];
      continue;
    }
    if (int rc = b.env.tables->get(b.device, im.src_w, im.resize_w, &p.xt, im.filter)) return rc;
    if (int rc = b.env.tables->get(b.device, im.src_h, im.resize_h, &p.yt, im.filter)) return rc;
    if (st.ycc) {
      // JPEG planes (the host path checked ycc_plan_ok): a wave kernel or nothing
      plan_wave(im, st, b.out_dtype, p);
      if (!p.wave) return fail(MXD_ERR_UNSUPPORTED, "mxd: no wave kernel for a JPEG plane source");
    } else if (!no_wave) {
      if (g_policy.load() & MXD_POLICY_PREFER_BAND) {
        plan_band(im, st, b.out_dtype, p);
        if (!p.band) plan_wave(im, st, b.out_dtype, p);
      } else {
        plan_wave(im, st, b.out_dtype, p);
        if (!p.wave) plan_band(im, st, b.out_dtype, p);
      }
      // A formatted call keeps a wave kernel only where its formatted form
      // exists (every shape of wave.hip; not the cubic filters' shapes): the
      // others are resized into u8 scratch rows by the band or general kernel.
      if (b.formatted && p.wave &&
          !mxd::wave_has_kernel(mxd::WaveCfg{b.channels, mxd::kWaveOutFmt, p.bucket, 0, 0, p.kind, p.s, p.dmax, p.q,
                                             p.shift, p.pp})) {
        p.wave = false;
        plan_band(im, st, b.out_dtype, p);
      }
    }
  }
  return MXD_OK;
}

// Appends the images of one kernel family to the descriptor order, grouped
// by kernel key (batch order within a key), and starts a group per key.
template <class Group, class Pick, class Key, class Cfg>
void order_family(Batch& b, std::vector<Group>& groups, Pick pick, Key key, Cfg cfg) {
  std::vector<int32_t>& of = b.L.image_of;
  const size_t at = of.size();
  for (int32_t i = 0; i < b.n; i++)
    if (pick(b.L.plans[i])) of.push_back(i);
  std::stable_sort(of.begin() + at, of.end(),
                   [&](int32_t x, int32_t y) { return key(b.L.plans[x]) < key(b.L.plans[y]); });
  for (size_t k = at; k < of.size(); k++) {
    const ImgPlan& p = b.L.plans[of[k]];
    if (groups.empty() || key(b.L.plans[of[groups.back().first]]) != key(p)) {
      groups.push_back(Group{});
      groups.back().first = (int32_t)k;
      groups.back().cfg = cfg(p);
    }
    groups.back().count++;
  }
}

void fill(const Batch& b, int32_t i, ImgDev& d) {
  const mxd_image& im = b.images[i];
  const ImgPlan& p = b.L.plans[i];
  const Stored st = b.at(i);
  d = ImgDev{};
  d.src = st.base;
  d.src_stride = st.stride;
  d.src_w = im.src_w;
  d.src_h = st.rows;
  d.src_x0 = st.x0;
  d.src_y0 = st.y0;
  d.dst = im.dst;
  d.dst_stride = im.dst_stride;
  d.xwidth = p.xt->padded;
  d.ywidth = p.yt->padded;
  d.xtab = p.xt->ptr + (size_t)im.crop_x * (mxd::kTapHeader + p.xt->padded);
  d.ytab = p.yt->ptr + (size_t)im.crop_y * (mxd::kTapHeader + p.yt->padded);
  d.crop_w = im.crop_w;
  d.crop_h = im.crop_h;
  d.flip = im.flip ? 1 : 0;
  d.ycc = st.ycc;
}

// (nstrips, crop_h) of a group's images: what band_rows sizes the units by.
template <class Group>
std::vector<std::pair<int32_t, int32_t>> group_strips(const Batch& b, const Group& g, bool band) {
  std::vector<std::pair<int32_t, int32_t>> strips;
  for (int32_t k = g.first; k < g.first + g.count; k++) {
    const ImgPlan& p = b.L.plans[b.L.image_of[k]];
    strips.push_back({band ? p.bp.nstrips : p.nstrips, b.images[b.L.image_of[k]].crop_h});
  }
  return strips;
}

// The descriptors of a band or wave group whose units are ty rows high:
// 4-byte aligned base with the byte shift in flip bits 8.., the schedule of
// the image's geometry (sched(i, ty, &out); gather kernels have none), the
// image's units numbered from tile_begin.  per_img: the unit count of every
// image when all agree, else 0.
template <class Group, class Sched>
int unit_descs(Batch& b, Group& g, bool band, int32_t ty, Sched sched) {
  std::unordered_map<int32_t, const DevSched*> sched_of;  // by rep[] (one geometry, one band height)
  for (int32_t k = g.first; k < g.first + g.count; k++) {
    const int32_t i = b.L.image_of[k];
    const mxd_image& im = b.images[i];
    const ImgPlan& p = b.L.plans[i];
    ImgDev& d = b.L.descs[k];
    fill(b, i, d);
    const uintptr_t a = reinterpret_cast<uintptr_t>(d.src);
    d.src = reinterpret_cast<const uint8_t*>(a & ~(uintptr_t)3);
    d.flip |= (int32_t)(a & 3) << 8;
    d.ty = std::min(ty, im.crop_h);
    d.group = 1;
    if (band || p.kind == 2) {
      const DevSched*& sc = sched_of[b.rep[i]];
      if (!sc)
        if (int rc = sched(i, d.ty, &sc)) return rc;
      d.ytab = reinterpret_cast<const float*>(sc->ptr);
      d.ywidth = sc->band_words;
      d.group = sc->entry_off;
    }
    d.tile_begin = g.units;
    d.nstrips = band ? p.bp.nstrips : p.nstrips;
    d.tx = band ? p.bp.tx : p.tx;
    const int32_t u = d.nstrips * ((im.crop_h + d.ty - 1) / d.ty);
    g.cfg.per_img = k == g.first ? u : (g.cfg.per_img == u ? u : 0);
    g.units += u;
  }
  g.cfg.nunits = g.units;
  return MXD_OK;
}

// Band launches: one per (class, window KiB, lookahead).
int band_groups(Batch& b) {
  const int32_t channels = b.channels, f32 = b.f32();
  order_family(
      b, b.L.bands, [](const ImgPlan& p) { return p.band; },
      [](const ImgPlan& p) { return std::make_tuple(p.bp.cls, p.bp.nq, p.bp.la); },
      [=](const ImgPlan& p) {
        return mxd::BandCfg{channels, f32, p.bp.nq, p.bp.taps, p.bp.s, p.bp.db, p.bp.la, 0, 0, 0, 0};
      });
  for (BatchLayout::BandGroup& g : b.L.bands) {
    g.cfg.nimgs = g.count;
    const int32_t forced = g_tune[MXD_TUNE_BAND_ROWS].load();
    const int32_t capacity = b.env.band_capacity >= 0 ? b.env.band_capacity : band_capacity_cached(g.cfg, b.device);
    const int32_t ty = forced > 0 ? forced : band_rows(group_strips(b, g, true), capacity, kBandMaxRows);
    auto sched = [&](int32_t i, int32_t rows, const DevSched** out) {
      const mxd_image& im = b.images[i];
      const mxd::BandPlan& bp = b.L.plans[i].bp;
      return band_schedule_dev(*b.env.scheds, b.device, *b.L.plans[i].yt, im.src_h, im.resize_h, im.crop_y, im.crop_h,
                               rows, bp.db, bp.s, bp.la + 2, out);
    };
    if (int rc = unit_descs(b, g, true, ty, sched)) return rc;
    // A persistent grid: as many workgroups as the device holds at once,
    // each running an equal share of units (measured on C2 / 12 MP / 24 MP:
    // 0.158 / 0.195 / 0.367 ms against 0.17-0.19 / 0.224 / 0.383 with one
    // workgroup per unit); MXD_TUNE_BAND_GRID overrides.
    const int32_t knob = g_tune[MXD_TUNE_BAND_GRID].load();
    int32_t grid = knob == 1 ? g.units : knob > 1 ? knob : (capacity > 0 ? capacity : 1024);
    grid = std::max(1, std::min(g.units, grid));
    g.cfg.grid = (g.units + (g.units + grid - 1) / grid - 1) / ((g.units + grid - 1) / grid);
  }
  return MXD_OK;
}

// Wave launches: one per kernel (kind, tap bucket, scatter shape, q, shift).
int wave_groups(Batch& b) {
  const int32_t channels = b.channels, mode = b.formatted ? mxd::kWaveOutFmt : b.f32();
  const size_t at = b.L.image_of.size();
  order_family(
      b, b.L.waves, [](const ImgPlan& p) { return p.wave; },
      [](const ImgPlan& p) { return std::make_tuple(p.kind, p.bucket, p.s, p.dmax, p.q, p.shift, p.pp, p.ycc); },
      [=](const ImgPlan& p) {
        return mxd::WaveCfg{channels, mode, p.bucket, 0, 0, p.kind, p.s, p.dmax, p.q, p.shift, p.pp, 0, 1, p.ycc ? 1 : 0};
      });
  // Source load policy (wave.hip LAUX): streaming (nt) loads when the
  // call's sources are far past what the 256 MB Infinity Cache could hold
  // for a re-read (sources just written by a decode or a copy stay there,
  // and nt loads would bypass them: C4's 128 small images measured 45 %
  // slower with nt, C2 / C3 / C5 2-7 % faster; profiles/r06/README.md).
  // MXD_TUNE_LOAD_POLICY: 1 = default policy always, 2 = nt always.
  int64_t src_bytes = 0;
  for (size_t k = at; k < b.L.image_of.size(); k++) {
    const mxd_image& im = b.images[b.L.image_of[k]];
    src_bytes += (int64_t)im.src_w * im.src_h * im.channels;
  }
  const int32_t load_knob = g_tune[MXD_TUNE_LOAD_POLICY].load();
  const int32_t nt = load_knob == 2 ? 1 : load_knob == 1 ? 0 : src_bytes >= kNtSourceBytes ? 1 : 0;
  for (BatchLayout::WaveGroup& g : b.L.waves) {
    g.cfg.nimgs = g.count;
    g.cfg.nt = g.cfg.ycc ? 0 : nt;
    if (g.cfg.nt && !mxd::wave_has_kernel(g.cfg)) g.cfg.nt = 0;  // shapes built with the default policy only
    const int32_t capacity = b.env.wave_capacity >= 0 ? b.env.wave_capacity : wave_capacity_cached(g.cfg, b.device);
    g.ty = band_rows(group_strips(b, g, false), capacity);
    auto sched = [&](int32_t i, int32_t rows, const DevSched** out) {
      const mxd_image& im = b.images[i];
      const ImgPlan& p = b.L.plans[i];
      const int32_t lane_bytes = p.ycc ? mxd::kYccLaneBytes : p.pp == 16 ? 16 : p.pp * channels;
      return scatter_schedule(*b.env.scheds, b.device, *p.yt, im.src_h, im.resize_h, im.crop_y, im.crop_h, rows,
                              ScatterShape{p.s, p.dmax, p.p, lane_bytes}, out);
    };
    if (int rc = unit_descs(b, g, false, g.ty, sched)) return rc;
  }
  return MXD_OK;
}

// General path (any alignment, any tap count): workgroup tiles, resample.hip.
int general_group(Batch& b) {
  BatchLayout& L = b.L;
  L.general_at = (int32_t)L.image_of.size();
  for (int32_t i = 0; i < b.n; i++)
    if (!L.plans[i].band && !L.plans[i].wave) L.image_of.push_back(i);
  if (L.general_at == b.n) return MXD_OK;
  // The tile kernel addresses rows from the image's row 0: a staged
  // footprint is reached through the (never dereferenced) address its
  // row 0 would have; the kernel only reads footprint rows and columns.
  auto base0 = [&](int32_t i) {
    const Stored st = b.at(i);
    return st.base - (int64_t)st.y0 * st.stride - (int64_t)st.x0 * b.images[i].channels;
  };
  bool aligned16 = true;
  for (int32_t k = L.general_at; k < b.n; k++) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(base0(L.image_of[k])) | (uintptr_t)b.at(L.image_of[k]).stride;
    aligned16 = aligned16 && (a & 15) == 0;
  }
  const int32_t channels = b.channels, vec = aligned16 ? 16 : 1;
  LaunchCfg& cfg = L.general;
  cfg.vec = vec;
  cfg.channels = channels;
  cfg.alpha = channels == 4 && b.images[L.image_of[L.general_at]].rgba_weighted ? 1 : 0;
  cfg.f32 = b.f32();
  cfg.nimgs = b.n - L.general_at;
  int32_t tiles = 0;
  for (int32_t k = L.general_at; k < b.n; k++) {
    const int32_t i = L.image_of[k];
    const mxd_image& im = b.images[i];
    const DevTable* xt = L.plans[i].xt;
    const DevTable* yt = L.plans[i].yt;
    const bool flip = im.flip != 0;
    // Column strips: enough that one strip row's footprint is ~kStripBytes.
    const int32_t full = strip_chunks(*xt, im.crop_x, im.crop_w, 0, im.crop_w, flip, channels, 1);
    int32_t nstrips = std::max<int32_t>(1, (full + kStripBytes - 1) / kStripBytes);
    int32_t tx = (im.crop_w + nstrips - 1) / nstrips;
    tx = std::min<int32_t>(im.crop_w, (tx + 3) & ~3);
    nstrips = (im.crop_w + tx - 1) / tx;
    int32_t max_chunks = 0;
    for (int32_t s = 0; s < nstrips; s++) {
      const int32_t ox0 = s * tx, ox1 = std::min(ox0 + tx, im.crop_w);
      max_chunks = std::max(max_chunks, strip_chunks(*xt, im.crop_x, im.crop_w, ox0, ox1, flip, channels, vec));
    }
    const int32_t vw = (max_chunks * vec + 3) & ~3;
    const int32_t ty = std::min(kTileRows, im.crop_h);
    int32_t group = std::max<int32_t>(1, std::min<int32_t>(8, 512 / std::max(1, max_chunks)));
    group = std::max<int32_t>(1, std::min<int32_t>(group, kLdsBudget / (vw * 4)));
    group = std::min(group, ty);
    const int32_t nbands = (im.crop_h + ty - 1) / ty;
    ImgDev& d = L.descs[k];
    fill(b, i, d);
    d.src = base0(i);
    d.src_h = im.src_h;
    d.src_x0 = d.src_y0 = 0;
    d.tile_begin = tiles;
    d.nstrips = nstrips;
    d.ty = ty;
    d.tx = tx;
    d.group = group;
    tiles += nbands * nstrips;
    cfg.max_tx = std::max(cfg.max_tx, tx);
    cfg.max_ty = std::max(cfg.max_ty, ty);
    cfg.max_xw = std::max(cfg.max_xw, xt->padded);
    cfg.max_yw = std::max(cfg.max_yw, yt->padded);
    cfg.max_vw = std::max(cfg.max_vw, vw);
    cfg.max_group = std::max(cfg.max_group, group);
  }
  cfg.ntiles = tiles;
  if (mxd::resample_smem_bytes(cfg) > 160 * 1024) return fail(MXD_ERR_UNSUPPORTED, "mxd: tile does not fit in LDS");
  return MXD_OK;
}

// Whether the second pass reads image i (from scratch rows): every image,
// but a formatted call's wave images, which the resize launch formats.
bool second_pass_reads(const Batch& b, int32_t i) { return !(b.formatted && b.L.plans[i].wave); }

// The images the second pass reads get their scratch rows (at 256-byte
// aligned offsets: add_scratch); the others keep the caller's destination.
void place_scratch(Batch& b, const mxd_image* callers) {
  size_t at = 0;
  for (int32_t i = 0; i < b.n; i++) {
    mxd_image& im = b.L.images[i];
    if (second_pass_reads(b, i)) {
      im.dst = reinterpret_cast<void*>(at);
      at += scratch_size(im);
    } else {
      im.dst = callers[i].dst;
      im.dst_stride = callers[i].dst_stride;
    }
  }
  b.L.scratch_bytes = at;
}

// The chain of a call (the rule: capi_internal.h, above PostOps): which
// stages follow the resize, and which rows each reads and writes.
void derive_chain(const PostOps& ops, BatchLayout& L) {
  L.pass = ops.pass();
  if (ops.warps) L.chain[L.nstages++].kind = StageKind::Warp;
  if (ops.enhances) L.chain[L.nstages++].kind = StageKind::Enhance;
  if (L.pass != SecondPass::None) L.chain[L.nstages++].kind = StageKind::Pass;
  if (ops.mixes) L.chain[L.nstages++].kind = StageKind::Mix;
  for (int32_t s = 0; s < L.nstages; s++) {
    BatchLayout::Stage& st = L.chain[s];
    st.reads = s % 2 ? Rows::B : Rows::A;
    st.writes = s == L.nstages - 1 ? Rows::Dst : s % 2 ? Rows::A : Rows::B;
    st.entry_size = st.kind == StageKind::Warp       ? sizeof(mxd::WarpRowDev)
                    : st.kind == StageKind::Enhance  ? sizeof(mxd::EnhanceRowDev)
                    : st.kind == StageKind::Mix      ? sizeof(mxd::MixRowDev)
                    : L.pass == SecondPass::Tone     ? sizeof(mxd::ToneRowDev)
                    : L.pass == SecondPass::Color    ? sizeof(mxd::ColorRowDev)
                                                     : sizeof(mxd::FmtRowDev);
  }
}

// Whether a warp takes the table path: Pillow's scale path of NEAREST.
bool warp_tabled(const mxd_warp& w) { return w.mode == MXD_WARP_NEAREST && w.m[1] == 0.0 && w.m[3] == 0.0; }
size_t warp_tab_size(const mxd_image& im) { return (((size_t)im.crop_w + im.crop_h) * 4 + 15) & ~(size_t)15; }

// A stage's entries at the end of the upload (zeroed), their heads written:
// one per image the stage reads, in batch order.
void append_stage(Batch& b, const mxd_image* callers, BatchLayout::Stage& st) {
  BatchLayout& L = b.L;
  const bool every = st.kind != StageKind::Pass;
  for (int32_t i = 0; i < b.n; i++) st.count += every || second_pass_reads(b, i) ? 1 : 0;
  st.at = L.descs.size();
  L.descs.resize(st.at + ((size_t)st.count * st.entry_size + sizeof(ImgDev) - 1) / sizeof(ImgDev));
  for (int32_t i = 0, j = 0; i < b.n; i++) {
    if (!every && !second_pass_reads(b, i)) continue;
    const mxd_image& im = L.images[i];
    const bool out = st.writes == Rows::Dst;
    const mxd::RowHead h{static_cast<const uint8_t*>(im.dst) + (st.reads == Rows::B ? L.b_at : 0),
                         out ? callers[i].dst : static_cast<uint8_t*>(im.dst) + (st.writes == Rows::B ? L.b_at : 0),
                         im.dst_stride, out ? callers[i].dst_stride : im.dst_stride, im.crop_w, im.crop_h};
    std::memcpy(L.head(st, j++), &h, sizeof h);
  }
}

// The warp stage's own fields: modes, fills and matrices are part of the
// upload's bytes, so a cached slot is reused only for the same ones.
void fill_warps(Batch& b, BatchLayout::Stage& st, const PostOps& ops) {
  BatchLayout& L = b.L;
  size_t tab_at = L.warp_tab_at;
  for (int32_t i = 0; i < b.n; i++) {
    const mxd_image& im = L.images[i];
    const mxd_warp& wp = ops.warps[i];
    mxd::WarpRowDev& e = L.warp_entry(i);
    e.tile_begin = st.blocks;
    e.tiles_x = (im.crop_w + mxd::kWarpTileW - 1) / mxd::kWarpTileW;
    st.blocks += e.tiles_x * ((im.crop_h + mxd::kWarpTileH - 1) / mxd::kWarpTileH);
    e.path = wp.mode == MXD_WARP_NONE       ? mxd::kWarpCopy
             : warp_tabled(wp)              ? mxd::kWarpTable
             : wp.mode == MXD_WARP_NEAREST  ? mxd::kWarpFixed
                                            : mxd::kWarpBilinear;
    e.fill = (uint32_t)wp.fill[0] | (uint32_t)wp.fill[1] << 8 | (uint32_t)wp.fill[2] << 16;
    e.tab_off = 0, e.tab_index = -1;
    if (e.path == mxd::kWarpTable) {
      e.tab_off = (int32_t)(tab_at - L.warp_tab_at);
      e.tab_index = st.pre_blocks++;
      tab_at += warp_tab_size(im);
    }
    // (MXD_WARP_NONE reads nothing of the matrix: zeros, so equal calls make equal bytes)
    for (int k = 0; k < 6; k++) e.m[k] = e.path == mxd::kWarpCopy ? 0.0 : wp.m[k];
  }
}

// The enhance stage's own fields: ops and factors are part of the upload's
// bytes, so a cached slot is reused only for the same ones.
void fill_enhances(Batch& b, BatchLayout::Stage& st, const PostOps& ops) {
  BatchLayout& L = b.L;
  for (int32_t i = 0; i < b.n; i++) {
    const mxd_image& im = L.images[i];
    const mxd_enhance& en = ops.enhances[i];
    mxd::EnhanceRowDev& e = L.enhance_entry(i);
    e.tile_begin = st.blocks;
    e.tiles_x = (im.crop_w + mxd::kEnhTileW - 1) / mxd::kEnhTileW;
    st.blocks += e.tiles_x * ((im.crop_h + mxd::kEnhTileH - 1) / mxd::kEnhTileH);
    e.op = en.op;
    // (MXD_ENHANCE_NONE reads no factor: zero, so equal calls make equal bytes)
    e.factor = en.op == MXD_ENHANCE_NONE ? 0.0f : en.factor;
  }
}

// The mix stage's own fields: partners, ops, weights and boxes are part of the
// upload's bytes, so a cached slot is reused only for equal mixes.  The
// partner's rows are those the partner's own entry reads (an offset into the
// scratch until add_scratch).
void fill_mixes(Batch& b, BatchLayout::Stage& st, const PostOps& ops) {
  BatchLayout& L = b.L;
  for (int32_t i = 0; i < b.n; i++) {
    const mxd_image& im = L.images[i];
    const mxd_mix& mx = ops.mixes[i];
    mxd::MixRowDev& e = L.mix_entry(i);
    e.blk_begin = st.blocks;
    st.blocks += (im.crop_h + mxd::kMixRows - 1) / mxd::kMixRows;
    e.op = mx.op;
    // (MXD_MIX_NONE reads nothing else: zeros, so equal calls make equal bytes)
    if (mx.op == MXD_MIX_NONE) continue;
    const mxd::MixRowDev& p = L.mix_entry(mx.partner);
    e.psrc = p.src;
    e.psrc_stride = p.src_stride;
    if (mx.op == MXD_MIX_MIXUP) e.w_self = mx.w_self, e.w_other = mx.w_other;
    if (mx.op == MXD_MIX_CUTMIX) e.x0 = mx.x0, e.y0 = mx.y0, e.x1 = mx.x1, e.y1 = mx.y1;
  }
}

// After every descriptor, in ImgDev-sized blocks: the unit -> image tables of
// the band launches whose images differ in unit count (int32 each), then the
// stages' entries (append_stages).
void append_tables(Batch& b) {
  BatchLayout& L = b.L;
  std::vector<int32_t> unit_tables;
  for (BatchLayout::BandGroup& g : L.bands) {
    if (g.cfg.per_img > 0) continue;
    g.table = (int32_t)unit_tables.size();
    for (int32_t k = g.first; k < g.first + g.count; k++) {
      const ImgDev& d = L.descs[k];
      unit_tables.insert(unit_tables.end(), d.nstrips * ((d.crop_h + d.ty - 1) / d.ty), k - g.first);
    }
    unit_tables.resize((unit_tables.size() * 4 + sizeof(ImgDev) - 1) / sizeof(ImgDev) * sizeof(ImgDev) / 4, 0);
  }
  L.tables_at = L.descs.size();
  L.descs.resize(L.tables_at + unit_tables.size() * 4 / sizeof(ImgDev));
  if (!unit_tables.empty())
    std::memcpy(reinterpret_cast<void*>(L.descs.data() + L.tables_at), unit_tables.data(), unit_tables.size() * 4);
  L.fmt_at = L.descs.size();
}

// The second pass's own fields (matrices, ops and parameters: part of the
// upload's bytes like the rows), and a tone call's workspace behind
// everything else of the scratch: statistics first.
void fill_second_pass(Batch& b, BatchLayout::Stage& st, const PostOps& ops) {
  BatchLayout& L = b.L;
  const int32_t block_rows = L.pass == SecondPass::Format ? mxd::kFmtRows : mxd::kPixelRows;
  int32_t stats = 0;
  for (int32_t i = 0, j = 0; i < b.n; i++) {
    if (!second_pass_reads(b, i)) continue;
    const mxd_image& im = L.images[i];
    mxd::FmtRowDev& head = L.entry(j++);
    head.channels = im.channels;
    head.blk_begin = st.blocks;
    st.blocks += (im.crop_h + block_rows - 1) / block_rows;
    if (L.pass == SecondPass::Format) continue;
    mxd::ColorRowDev& c = reinterpret_cast<mxd::ColorRowDev&>(head);
    for (int k = 0; k < 12; k++) c.m[k] = ops.colors ? color_entry(ops.colors[i].m[k / 4][k % 4]) : k % 5 == 0 ? 1.0f : 0.0f;
    if (L.pass == SecondPass::Color) continue;
    // The workspace follows the scratch rows: statistics first.
    mxd::ToneRowDev& t = reinterpret_cast<mxd::ToneRowDev&>(head);
    t.op = ops.tones[i].op, t.arg = ops.tones[i].arg, t.factor = ops.tones[i].factor;
    t.hist_begin = st.pre_blocks;
    t.stat_off = -1;
    if (mxd::tone_needs_stats(t.op)) {
      t.stat_off = stats * (int32_t)(mxd::kToneStatWords * sizeof(uint32_t));
      stats++;
      st.pre_blocks += (im.crop_h + mxd::kToneHistRows - 1) / mxd::kToneHistRows;
    }
  }
  if (L.pass != SecondPass::Tone) return;
  L.tone_stat_bytes = (size_t)stats * mxd::kToneStatWords * sizeof(uint32_t);
  for (int32_t i = 0; i < b.n; i++)
    reinterpret_cast<mxd::ToneRowDev&>(L.entry(i)).lut_off = (int32_t)(L.tone_stat_bytes + (size_t)i * mxd::kToneLutBytes);
  L.tone_ws_at = (L.scratch_bytes + 255) & ~(size_t)255;
  L.scratch_bytes = L.tone_ws_at + L.tone_stat_bytes + (size_t)b.n * mxd::kToneLutBytes;
}

// The chain's scratch behind rows A, then its entries behind the tables: the
// second pass's first, then the warp stage's, the enhance stage's, the mix
// stage's.
void append_stages(Batch& b, const mxd_image* callers, const PostOps& ops) {
  BatchLayout& L = b.L;
  if (L.nstages >= 2) {
    L.b_at = (L.scratch_bytes + 255) & ~(size_t)255;
    L.scratch_bytes = L.b_at + L.scratch_bytes;
  }
  if (ops.warps) {
    L.warp_tab_at = (L.scratch_bytes + 255) & ~(size_t)255;
    size_t tab_bytes = 0;
    for (int32_t i = 0; i < b.n; i++) tab_bytes += warp_tabled(ops.warps[i]) ? warp_tab_size(L.images[i]) : 0;
    if (tab_bytes > 0) L.scratch_bytes = L.warp_tab_at + tab_bytes;
  }
  for (StageKind kind : {StageKind::Pass, StageKind::Warp, StageKind::Enhance, StageKind::Mix}) {
    BatchLayout::Stage* st = L.stage(kind);
    if (!st) continue;
    append_stage(b, callers, *st);
    if (kind == StageKind::Pass) fill_second_pass(b, *st, ops);
    if (kind == StageKind::Warp) fill_warps(b, *st, ops);
    if (kind == StageKind::Enhance) fill_enhances(b, *st, ops);
    if (kind == StageKind::Mix) fill_mixes(b, *st, ops);
  }
}

}  // namespace

LayoutEnv device_env() { return LayoutEnv{&tables(), &schedules(), -1, -1}; }
LayoutEnv host_env(int32_t band_capacity, int32_t wave_capacity) {
  return LayoutEnv{&host_tables(), &host_schedules(), band_capacity, wave_capacity};
}

void BatchLayout::add_scratch(uint8_t* base) {
  for (int32_t k = 0; k < n; k++)
    if (pass != SecondPass::Format || !plans[image_of[k]].wave) descs[k].dst = base + reinterpret_cast<uintptr_t>(descs[k].dst);
  for (int32_t s = 0; s < nstages; s++)
    for (int32_t j = 0; j < chain[s].count; j++) {
      mxd::RowHead h;
      std::memcpy(&h, head(chain[s], j), sizeof h);
      h.src = base + reinterpret_cast<uintptr_t>(h.src);
      if (chain[s].writes != Rows::Dst) h.dst = base + reinterpret_cast<uintptr_t>(h.dst);
      std::memcpy(head(chain[s], j), &h, sizeof h);
      // the partner's rows, an offset like src (a NONE entry has none)
      if (chain[s].kind == StageKind::Mix && mix_entry(j).op != MXD_MIX_NONE)
        mix_entry(j).psrc = base + reinterpret_cast<uintptr_t>(mix_entry(j).psrc);
    }
  if (pass == SecondPass::Tone) tone_ws = base + tone_ws_at;
  if (warped()) warp_tab = base + warp_tab_at;
}

int build_layout(const LayoutEnv& env, int32_t device, const mxd_image* images, int32_t n, const Stored* stored,
                 int32_t out_dtype, const PostOps& ops, BatchLayout* out) {
  *out = BatchLayout{};
  BatchLayout& L = *out;
  L.n = n;
  derive_chain(ops, L);
  L.matrix = ops.colors != nullptr;
  // A formatted call plans its kernels as a u8 call does: the wave kernels
  // exist in the same shapes in every output mode and write any element
  // alignment, and an image they do not take is resized into u8 scratch rows
  // (16-byte aligned; placed once the plans are known).
  const mxd_image* const callers = images;
  // A colour or tone call plans every image so, and keeps every u8 kernel a
  // plain u8 call has (the cubic filters' and JPEG plane sources' wave
  // kernels too).
  if (ops.any()) {
    out_dtype = MXD_U8;
    L.images.assign(images, images + n);
    for (mxd_image& im : L.images) {
      im.dst = reinterpret_cast<void*>((uintptr_t)4096);
      im.dst_stride = scratch_stride(im);
    }
    images = L.images.data();
  }
  Batch b{env, device, images, stored, n, images[0].channels, out_dtype, ops.resize_formats(), L, {}};
  if (int rc = plan_images(b)) return rc;
  if (ops.any()) place_scratch(b, callers);
  // Descriptors of one upload: band-kernel images first, then wave-kernel
  // images, then the general kernel's.
  L.descs.resize(n);
  L.image_of.reserve(n);
  if (int rc = band_groups(b)) return rc;
  if (int rc = wave_groups(b)) return rc;
  if (int rc = general_group(b)) return rc;
  append_tables(b);
  append_stages(b, callers, ops);
  // Largest first (a band unit is a workgroup, ~4 wave units).
  for (size_t g = 0; g < L.bands.size(); g++) L.launches.push_back({4 * (int64_t)L.bands[g].units, 0, (int32_t)g});
  for (size_t g = 0; g < L.waves.size(); g++) L.launches.push_back({L.waves[g].units, 1, (int32_t)g});
  if (L.general.nimgs > 0) L.launches.push_back({L.general.ntiles, 2, -1});
  std::stable_sort(L.launches.begin(), L.launches.end(),
                   [](const BatchLayout::Launch& x, const BatchLayout::Launch& y) { return x.units > y.units; });
  return MXD_OK;
}

}  // namespace capi
}  // namespace mxd
