// mix_layout_unit.cpp -- the batch layout (mlx-data_amd/csrc/batch_layout.cpp)
// of a mix call: every combination of the five other things that can follow
// the resize (format, colours, tones, warps, enhances) with mixes, under two
// kernel policies, in the device-free environment (host_env) through
// capi_internal.h, linked against the in-tree libmxd_amd.so; no device call.
// Checks the chain's invariants (the mix stage last, rows alternating A, B, A,
// B, the last stage writing the destinations, a second pass only with tones
// or colours and never the formatting one, rows B iff two stages) and that
// every entry's partner address is the partner's own source row address, in
// the rows the stage reads, before and after add_scratch.  Prints one line
// per layout and "ok"; exits non-zero at the first violation.  Built and run
// by tests/test_mix_chain.py.
#include <cstdio>
#include <cstdlib>

#include "capi_internal.h"

using namespace mxd::capi;

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
  const double m[6] = {m0, m1, m2, m3, m4, m5};
  for (int k = 0; k < 6; k++) w.m[k] = m[k];
  return w;
}

static int g_combo = 0, g_policy_now = 0;
#define CHECK(cond)                                                                                          \
  do {                                                                                                       \
    if (!(cond)) {                                                                                           \
      std::printf("FAIL policy %d combo %d line %d: %s\n", g_policy_now, g_combo, __LINE__, #cond);          \
      return 1;                                                                                              \
    }                                                                                                        \
  } while (0)

static mxd_mix mixup(int partner, float ws, float wo) {
  mxd_mix m{};
  m.op = MXD_MIX_MIXUP, m.partner = partner, m.w_self = ws, m.w_other = wo;
  return m;
}
static mxd_mix cutmix(int partner, int x0, int y0, int x1, int y1) {
  mxd_mix m{};
  m.op = MXD_MIX_CUTMIX, m.partner = partner, m.x0 = x0, m.y0 = y0, m.x1 = x1, m.y1 = y1;
  return m;
}

static int check_entries(BatchLayout& L, const std::vector<mxd_image>& imgs, const std::vector<mxd_mix>& mixes,
                         uintptr_t base) {
  const BatchLayout::Stage& st = *L.stage(StageKind::Mix);
  const int32_t n = (int32_t)imgs.size();
  CHECK(st.count == n && st.entry_size == sizeof(mxd::MixRowDev));
  const uintptr_t rows_at = base + (st.reads == Rows::B ? L.b_at : 0);
  const size_t rows_size = L.b_at ? L.b_at : L.scratch_bytes;  // rows A (and B) come first in the scratch
  int32_t blocks = 0;
  for (int32_t i = 0; i < n; i++) {
    const mxd::MixRowDev& e = L.mix_entry(i);
    const uintptr_t src = reinterpret_cast<uintptr_t>(e.src);
    // the image's rows in the rows the stage reads: where the resize kernels put them in A, plus b_at for B
    CHECK(src == rows_at + reinterpret_cast<uintptr_t>(L.images[i].dst));
    CHECK(src >= rows_at && src + (size_t)e.src_stride * imgs[i].crop_h <= rows_at + rows_size + 255);
    CHECK(e.src_stride == L.images[i].dst_stride && e.src_stride % 16 == 0 && src % 256 == 0);
    CHECK(e.dst == imgs[i].dst && e.dst_stride == imgs[i].dst_stride);
    CHECK(e.w == imgs[i].crop_w && e.h == imgs[i].crop_h);
    CHECK(e.blk_begin == blocks && e.op == mixes[i].op);
    blocks += (imgs[i].crop_h + mxd::kMixRows - 1) / mxd::kMixRows;
    if (e.op == MXD_MIX_NONE) {
      // nothing else of the entry is set: equal calls upload equal bytes
      CHECK(e.psrc == nullptr && e.psrc_stride == 0 && e.w_self == 0 && e.w_other == 0);
      CHECK(e.x0 == 0 && e.y0 == 0 && e.x1 == 0 && e.y1 == 0);
      continue;
    }
    const mxd::MixRowDev& p = L.mix_entry(mixes[i].partner);
    CHECK(e.psrc == p.src && e.psrc_stride == p.src_stride);
    CHECK(p.w == e.w && p.h == e.h);
    if (e.op == MXD_MIX_MIXUP) CHECK(e.w_self == mixes[i].w_self && e.w_other == mixes[i].w_other && e.x1 == 0 && e.y1 == 0);
    if (e.op == MXD_MIX_CUTMIX)
      CHECK(e.x0 == mixes[i].x0 && e.y0 == mixes[i].y0 && e.x1 == mixes[i].x1 && e.y1 == mixes[i].y1 && e.w_self == 0);
    CHECK(e.pad[0] == 0 && e.pad[1] == 0);
  }
  CHECK(st.blocks == blocks);
  return 0;
}

int main() {
  // stage_chain_unit.cpp's mixed batch (general, wave, general, Catmull-Rom
  // wave, wave, wave / band, general): the windows of 1 and 3 and of 2 and 5
  // are equal, so those pair up.
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
  const std::vector<mxd_mix> mixes = {
      mixup(0, 0.25f, 0.75f),         // its own partner
      mixup(3, 0.3f, (float)(1.0 - 0.3)),
      cutmix(5, 3, 0, 17, 40),
      cutmix(1, 0, 0, 224, 224),      // a chain 3 -> 1 -> 3
      mxd_mix{},                      // NONE
      mixup(2, 1.0f, 0.0f),
      cutmix(6, 5, 5, 5, 9),          // an empty box
  };
  const std::vector<mxd_enhance> enh(n, mxd_enhance{MXD_ENHANCE_COLOR, 0.25f, {0, 0}});
  std::vector<mxd_warp> warps(n, warp(MXD_WARP_BILINEAR, 0.9, -0.2, 4, 0.2, 0.9, 1));
  warps[1] = warp(MXD_WARP_NEAREST, 1.2, 0, 3, 0, 0.9, -2);  // table path
  const std::vector<mxd_tone> tones(n, mxd_tone{MXD_TONE_EQUALIZE, 0, 0.0f, 0});
  std::vector<mxd_color> colors(n);
  for (int32_t i = 0; i < n; i++)
    for (int k = 0; k < 12; k++) colors[i].m[k / 4][k % 4] = (float)(100 * i + k) / 64;
  mxd_out_format fmt{};
  fmt.elem = MXD_ELEM_BF16;
  fmt.layout = MXD_LAYOUT_HWC;
  if (mxd_mix_validate(imgs.data(), mixes.data(), n) != MXD_OK) {
    std::printf("FAIL validate: %s\n", mxd_last_error());
    return 1;
  }
  const LayoutEnv env = host_env(64, 4096);
  const int32_t policies[2] = {MXD_POLICY_AUTO, MXD_POLICY_PREFER_BAND};
  for (int pol = 0; pol < 2; pol++)
    for (int combo = 0; combo < 32; combo++) {
      g_combo = combo, g_policy_now = policies[pol];
      const PostOps ops{combo & 1 ? &fmt : nullptr, combo & 2 ? colors.data() : nullptr, combo & 4 ? tones.data() : nullptr,
                        combo & 8 ? warps.data() : nullptr, combo & 16 ? enh.data() : nullptr, mixes.data()};
      mxd_set_kernel_policy(policies[pol]);
      BatchLayout L;
      if (build_layout(env, 0, imgs.data(), n, nullptr, MXD_U8, ops, &L) != MXD_OK) {
        std::printf("FAIL policy %d combo %d: %s\n", policies[pol], combo, mxd_last_error());
        return 1;
      }
      // the chain: warp, enhance, a second pass only with tones or colours, the mix stage last
      const bool second = (combo & 6) != 0;
      const int32_t want = (combo & 8 ? 1 : 0) + (combo & 16 ? 1 : 0) + (second ? 1 : 0) + 1;
      CHECK(L.nstages == want && want <= 4);
      int32_t s = 0;
      if (combo & 8) CHECK(L.chain[s++].kind == StageKind::Warp);
      if (combo & 16) CHECK(L.chain[s++].kind == StageKind::Enhance);
      if (second) CHECK(L.chain[s++].kind == StageKind::Pass);
      CHECK(L.chain[s].kind == StageKind::Mix && s == L.nstages - 1);
      for (s = 0; s < L.nstages; s++) {
        CHECK(L.chain[s].reads == (s % 2 ? Rows::B : Rows::A));
        CHECK(L.chain[s].writes == (s == L.nstages - 1 ? Rows::Dst : s % 2 ? Rows::A : Rows::B));
        CHECK(L.chain[s].count == n);
      }
      // the second pass is pixel_rows (its u8 form is the launcher's: it does not write the destinations)
      CHECK(L.pass == (combo & 4 ? SecondPass::Tone : combo & 2 ? SecondPass::Color : SecondPass::None));
      CHECK(!ops.resize_formats());
      for (const BatchLayout::WaveGroup& g : L.waves) CHECK(g.cfg.f32 == 0);  // the resize kernels' u8 mode
      for (const BatchLayout::BandGroup& g : L.bands) CHECK(g.cfg.f32 == 0);
      CHECK((L.b_at > 0) == (L.nstages >= 2));
      CHECK(L.scratch_bytes > 0 && L.b_at % 256 == 0);
      if (check_entries(L, imgs, mixes, 0)) return 1;
      const uintptr_t base = uintptr_t(1) << 32;
      L.add_scratch(reinterpret_cast<uint8_t*>(base));
      if (check_entries(L, imgs, mixes, base)) return 1;
      std::printf("policy=%d combo=%d stages=%d reads=%c b_at=%zu scratch=%zu mix_at=%zu blocks=%d\n", policies[pol], combo,
                  L.nstages, L.stage(StageKind::Mix)->reads == Rows::B ? 'B' : 'A', L.b_at, L.scratch_bytes, L.mix_at(),
                  L.mix_blocks());
    }
  mxd_set_kernel_policy(MXD_POLICY_AUTO);
  std::printf("ok\n");
  return 0;
}
