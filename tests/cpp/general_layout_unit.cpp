// general_layout_unit.cpp -- prints how general_group (mlx-data_amd/csrc/
// batch_layout.cpp) tiles the launches it reads from stdin, in the device-free
// environment (host_env) through capi_internal.h, linked against the in-tree
// libmxd_amd.so; no device call.  Every launch runs under MXD_POLICY_NO_WAVE:
// neither a wave nor a band kernel takes an image, all are the general
// kernel's.  Built and run by tests/test_general_shapes.py, which writes the
// launches from tests/general_shapes.py (one table) and compares the lines
// with that module's restatement of the tiling.
//
// Input, whitespace separated: per launch `f32 n`, then n images of
//   src_w src_h channels resize_w resize_h crop_x crop_y crop_w crop_h flip
//   src_offset src_stride dst_offset dst_stride rgba_weighted filter
// (the offsets are bytes past a 4096-byte aligned fake address).
// Output: per launch one line `launch rc=0 vec= channels= alpha= f32= nimgs=
// ntiles= smem= max_vw=` followed by one line per image `image nstrips= tx= ty=
// group= vw= tile_begin= xwidth= ywidth=`, or `launch rc=<code> error=<message>`;
// `ok` at the end.  The layout keeps no per-image vw: an image's figure is
// this program's own strip_chunks over the layout's strips, max_vw the
// planner's (LaunchCfg::max_vw).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "capi_internal.h"

using namespace mxd::capi;

// Fixed fake addresses (never dereferenced).
static const uintptr_t kSrc = uintptr_t(3) << 33, kDst = uintptr_t(5) << 33;

int main() {
  const LayoutEnv env = host_env(64, 4096);
  mxd_set_kernel_policy(MXD_POLICY_NO_WAVE);
  int f32 = 0, n = 0;
  while (std::scanf("%d %d", &f32, &n) == 2) {
    if (n <= 0 || n > 4096) return 2;
    std::vector<mxd_image> imgs(n);
    for (mxd_image& m : imgs) {
      long long src_off = 0, src_stride = 0, dst_off = 0, dst_stride = 0;
      int v[10], weighted = 0, filter = 0;
      for (int& x : v)
        if (std::scanf("%d", &x) != 1) return 2;
      if (std::scanf("%lld %lld %lld %lld %d %d", &src_off, &src_stride, &dst_off, &dst_stride, &weighted, &filter) != 6)
        return 2;
      m = mxd_image{};
      m.src = reinterpret_cast<const uint8_t*>(kSrc + (uintptr_t)src_off);
      m.src_stride = src_stride;
      m.src_w = v[0], m.src_h = v[1], m.channels = v[2];
      m.resize_w = v[3], m.resize_h = v[4];
      m.crop_x = v[5], m.crop_y = v[6], m.crop_w = v[7], m.crop_h = v[8];
      m.flip = v[9];
      m.dst = reinterpret_cast<void*>(kDst + (uintptr_t)dst_off);
      m.dst_stride = dst_stride;
      m.rgba_weighted = weighted;
      m.filter = filter;
    }
    for (int i = 0; i < n; i++)
      if (validate(imgs[i], i) != MXD_OK) {
        std::printf("FAIL %s\n", mxd_last_error());
        return 1;
      }
    BatchLayout L;
    const int rc = build_layout(env, 0, imgs.data(), n, nullptr, f32 ? MXD_F32_DIV255 : MXD_U8, PostOps{}, &L);
    if (rc != MXD_OK) {
      std::printf("launch rc=%d error=%s\n", rc, mxd_last_error());
      continue;
    }
    const LaunchCfg& cfg = L.general;
    if (L.general_at != 0 || cfg.nimgs != n || !L.bands.empty() || !L.waves.empty() || L.launches.size() != 1 ||
        L.launches[0].kind != 2 || L.launches[0].units != cfg.ntiles) {
      std::printf("FAIL not one general launch\n");
      return 1;
    }
    std::printf("launch rc=0 vec=%d channels=%d alpha=%d f32=%d nimgs=%d ntiles=%d smem=%d max_vw=%d\n", cfg.vec,
                cfg.channels, cfg.alpha, cfg.f32, cfg.nimgs, cfg.ntiles, mxd::resample_smem_bytes(cfg), cfg.max_vw);
    for (int k = 0; k < n; k++) {
      const int i = L.image_of[k];
      const mxd_image& im = imgs[i];
      const ImgDev& d = L.descs[k];
      int32_t chunks = 0;
      for (int32_t s = 0; s < d.nstrips; s++)
        chunks = std::max(chunks, strip_chunks(*L.plans[i].xt, im.crop_x, im.crop_w, s * d.tx,
                                               std::min(s * d.tx + d.tx, im.crop_w), im.flip != 0, im.channels, cfg.vec));
      std::printf("image index=%d nstrips=%d tx=%d ty=%d group=%d vw=%d tile_begin=%d xwidth=%d ywidth=%d\n", i, d.nstrips,
                  d.tx, d.ty, d.group, (chunks * cfg.vec + 3) & ~3, d.tile_begin, d.xwidth, d.ywidth);
    }
  }
  mxd_set_kernel_policy(MXD_POLICY_AUTO);
  std::printf("ok\n");
  return 0;
}
