// warp.hip -- the warp stage (resample.h): per-image affine warps of u8 RGB
// scratch rows, between the resize launches and the second pass of a warp
// call.  One launch covers every image of a call; no kernel waits on another
// workgroup (warp_tab is ordered before warp_rows by the stream).
//
// warp_tab   one workgroup per image that takes Pillow's scale path (NEAREST
//            with m[1] == m[3] == 0): lane 0 builds xt[w], lane 64 (another
//            wave) yt[h] by the sequential double accumulation of the
//            definition, once per image.
// warp_rows  pixmap.hip's measured shape: a workgroup of 256 lanes owns a 64 x
//            16 pixel output tile, a lane four adjacent pixels of a row and
//            one 12-byte store where the destination is 4-byte aligned
//            (element stores for row tails and misaligned destinations).  The
//            image's entry is read through a uniform (scalar) address and its
//            code path chosen by a uniform branch: a copy (MXD_WARP_NONE), the
//            table lookup, 16.16 fixed point in 64-bit integers, or the double
//            bilinear.  Every source pixel is fetched with one 8-byte load at a
//            4-byte aligned address clamped to end inside the image's own
//            rows (16-byte aligned base, stride a multiple of 16, so
//            stride * h bytes are the image's); indices are clamped or
//            rejected before the address is formed, and a rejected pixel takes
//            the fill without a load.
//
// Arithmetic: Pillow's, bit for bit; the CPU statement
// is warp.cpp's.  Every double operation is correctly rounded and none fused,
// so this file is compiled with -ffp-contract=off and says so again below.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "resample.h"

#pragma clang fp contract(off)

namespace mxd {
namespace {

constexpr int kThreads = 256;
constexpr int kGroups = kWarpTileW / 4;  // lanes per tile row
static_assert(kGroups * kWarpTileH == kThreads, "a lane per four pixels of the tile");

using WarpRowK = const __attribute__((address_space(4))) WarpRowDev;

// The three bytes of the pixel at byte offset o (0 <= o <= limit - 3) of an
// image whose rows take `limit` bytes (a multiple of 16, >= 16) from base.
__device__ __forceinline__ uint32_t fetch(const uint8_t* base, int64_t limit, int64_t o) {
  const int64_t a = min(o & ~(int64_t)3, limit - 8);
  const uint32_t* p = reinterpret_cast<const uint32_t*>(base + a);
  const uint64_t v = (uint64_t)p[0] | (uint64_t)p[1] << 32;
  return (uint32_t)(v >> (8 * (int)(o - a))) & 0xffffffu;
}

__device__ __forceinline__ int64_t fix16(double v) {
  const double t = v * 65536.0 + 0.5;
  return (int64_t)floor(t);
}

__device__ __forceinline__ double lerp(double a, double b, double d) {
  const double diff = b - a;
  const double prod = diff * d;
  return a + prod;
}

__global__ __launch_bounds__(kThreads) void warp_tab(const WarpRowDev* __restrict__ rows, int nimgs, uint8_t* ws) {
  __shared__ int img;
  for (int i = threadIdx.x; i < nimgs; i += kThreads)
    if (rows[i].tab_index == (int)blockIdx.x) img = i;  // (exactly one)
  __syncthreads();
  const WarpRowDev& e = rows[img];
  int32_t* const xt = reinterpret_cast<int32_t*>(ws + e.tab_off);
  if (threadIdx.x == 0) {
    double xo = e.m[2] + e.m[0] * 0.5;
    for (int x = 0; x < e.w; x++) {
      xt[x] = xo < 0.0 ? -1 : (int32_t)xo;
      xo = xo + e.m[0];
    }
  } else if (threadIdx.x == 64) {
    int32_t* const yt = xt + e.w;
    double yo = e.m[5] + e.m[4] * 0.5;
    for (int y = 0; y < e.h; y++) {
      yt[y] = yo < 0.0 ? -1 : (int32_t)yo;
      yo = yo + e.m[4];
    }
  }
}

__global__ __launch_bounds__(kThreads) void warp_rows(const void* __restrict__ rows, int nimgs,
                                                      const uint8_t* __restrict__ ws) {
  WarpRowK* rk = (WarpRowK*)rows;
  const int blk = blockIdx.x;
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rk[mid].tile_begin <= blk) lo = mid; else hi = mid - 1;
  }
  WarpRowK& e = rk[lo];
  const int w = e.w, h = e.h;
  const int t = blk - e.tile_begin;
  const int tyb = t / e.tiles_x;
  const int y = tyb * kWarpTileH + (int)threadIdx.x / kGroups;
  const int x0 = (t - tyb * e.tiles_x) * kWarpTileW + ((int)threadIdx.x % kGroups) * 4;
  if (y >= h || x0 >= w) return;
  const int cnt = min(4, w - x0);
  const uint8_t* const src = e.src;
  const int64_t sstride = e.src_stride;
  const int64_t limit = sstride * h;
  const uint32_t fill = e.fill;
  uint32_t px[4] = {fill, fill, fill, fill};
  const int path = e.path;
  if (path == kWarpCopy) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < cnt) px[k] = fetch(src, limit, (int64_t)y * sstride + 3 * (x0 + k));
  } else if (path == kWarpTable) {
    const int32_t* const xt = reinterpret_cast<const int32_t*>(ws + e.tab_off);
    const int yin = xt[w + y];
    if (yin >= 0 && yin < h) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (k >= cnt) continue;
        const int xin = xt[x0 + k];
        if (xin >= 0 && xin < w) px[k] = fetch(src, limit, (int64_t)yin * sstride + 3 * xin);
      }
    }
  } else if (path == kWarpFixed) {
    const double m0 = e.m[0], m1 = e.m[1], m3 = e.m[3], m4 = e.m[4];
    const int64_t a0 = fix16(m0), a1 = fix16(m1), a3 = fix16(m3), a4 = fix16(m4);
    const double c2 = (e.m[2] + m0 * 0.5) + m1 * 0.5;
    const double c5 = (e.m[5] + m3 * 0.5) + m4 * 0.5;
    const int64_t bx = fix16(c2) + a1 * y, by = fix16(c5) + a4 * y;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (k >= cnt) continue;
      const int64_t xin = (bx + a0 * (x0 + k)) >> 16, yin = (by + a3 * (x0 + k)) >> 16;
      if (xin >= 0 && xin < w && yin >= 0 && yin < h) px[k] = fetch(src, limit, yin * sstride + 3 * xin);
    }
  } else {
    const double m0 = e.m[0], m2 = e.m[2], m3 = e.m[3], m5 = e.m[5];
    const double yc5 = (double)y + 0.5;
    const double ty = e.m[1] * yc5, uy = e.m[4] * yc5;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (k >= cnt) continue;
      const double xc5 = (double)(x0 + k) + 0.5;
      const double px0 = m0 * xc5, py0 = m3 * xc5;
      const double s1 = px0 + ty, s2 = py0 + uy;
      double sx = s1 + m2, sy = s2 + m5;
      if (sx < 0.0 || sx >= (double)w || sy < 0.0 || sy >= (double)h) continue;
      sx = sx - 0.5;
      sy = sy - 0.5;
      const double fx = floor(sx), fy = floor(sy);
      const int X = (int)fx, Y = (int)fy;
      const double dx = sx - fx, dy = sy - fy;
      const int xa = min(max(X, 0), w - 1), xb = min(max(X + 1, 0), w - 1), yc = min(max(Y, 0), h - 1);
      const uint32_t p00 = fetch(src, limit, (int64_t)yc * sstride + 3 * xa);
      const uint32_t p01 = fetch(src, limit, (int64_t)yc * sstride + 3 * xb);
      const bool below = Y + 1 >= 0 && Y + 1 < h;
      const int yb = below ? Y + 1 : yc;  // (a row of the image either way; not used unless below)
      const uint32_t p10 = fetch(src, limit, (int64_t)yb * sstride + 3 * xa);
      const uint32_t p11 = fetch(src, limit, (int64_t)yb * sstride + 3 * xb);
      uint32_t o = 0;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double v1 = lerp((double)((p00 >> (8 * c)) & 255u), (double)((p01 >> (8 * c)) & 255u), dx);
        const double r2 = lerp((double)((p10 >> (8 * c)) & 255u), (double)((p11 >> (8 * c)) & 255u), dx);
        const double v2 = below ? r2 : v1;
        const double v = lerp(v1, v2, dy);
        o |= ((uint32_t)(int)v & 255u) << (8 * c);
      }
      px[k] = o;
    }
  }
  uint8_t* const d = e.dst + (int64_t)y * e.dst_stride + 3 * (int64_t)x0;
  const bool wide = ((reinterpret_cast<uint64_t>(e.dst) | (uint64_t)e.dst_stride) & 3) == 0;
  if (wide && cnt == 4) {
    uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
    d4[0] = px[0] | px[1] << 24;
    d4[1] = px[1] >> 8 | px[2] << 16;
    d4[2] = px[2] >> 16 | px[3] << 8;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (k >= cnt) continue;
      d[3 * k] = (uint8_t)px[k], d[3 * k + 1] = (uint8_t)(px[k] >> 8), d[3 * k + 2] = (uint8_t)(px[k] >> 16);
    }
  }
}

}  // namespace

int launch_warp(const WarpRowDev* rows, int nimgs, int ntiles, int tab_rows, uint8_t* ws, void* stream) {
  if (nimgs <= 0 || ntiles <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (tab_rows > 0) hipLaunchKernelGGL(warp_tab, dim3(tab_rows), dim3(kThreads), 0, s, rows, nimgs, ws);
  hipLaunchKernelGGL(warp_rows, dim3(ntiles), dim3(kThreads), 0, s, static_cast<const void*>(rows), nimgs,
                     static_cast<const uint8_t*>(ws));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
