// warp_cubic.hip -- the bicubic images of the warp stage (resample.h,
// MXD_WARP_BICUBIC): Pillow's Image.transform(AFFINE, BICUBIC), bit for bit.
// warp.hip's tiles and entries, another data path: a bicubic pixel reads a
// 4 x 4 neighbourhood and neighbouring pixels share almost all of it, so a
// workgroup brings its tile's source box into LDS once and the taps are LDS
// reads.
//
// warp_cubic_rows  launched over the tiles from the first bicubic image's
//            first to the last one's last, behind warp_rows on the same
//            stream; a workgroup whose image is not bicubic returns on the
//            uniform path word (as warp_rows does for a bicubic one), and no
//            kernel waits on another workgroup.  A workgroup of 256 lanes owns
//            a 64 x 16 output tile, a lane four adjacent pixels of a row and
//            one 12-byte store where the destination is 4-byte aligned.
//   the box  the source positions of the tile's four corner pixels bound
//            every pixel's (the map is affine); floored, widened by -1 / +2
//            for the taps and by 1 more against rounding, clamped to the
//            image, the left edge moved down to a multiple of 4 pixels.  The
//            taps' indices are clamped into the image, so they lie in the
//            clamped box.  An empty box: every pixel of the tile is fill,
//            nothing is loaded.
//   staging  a box of at most kBoxDwords pixels goes to LDS as one dword per
//            pixel, rows a multiple of 4 dwords apart: a lane takes four
//            pixels -- 12 source bytes at a 4-byte aligned address (16-byte
//            aligned rows, a multiple of 4 pixels in) -- and writes them with
//            one 16-byte LDS store; consecutive lanes take consecutive groups
//            of a box row.  A dword that would start past the row's own stride
//            bytes is not loaded (its pixels lie past the image's width).
//   taps     a row's four taps are adjacent dwords unless the clamp folds
//            them.  A lane whose taps are not all inside the staged box, and
//            every lane when the box does not fit (strong minification), reads
//            them with fetch_rgb from global memory, like warp_rows: indices
//            are clamped or rejected before an address is formed, and nothing
//            outside the image's stride * h bytes is read.  Both routes give
//            the same bytes.
//
// Arithmetic: the CPU statement is warp.cpp's (mxd_warp_apply_u8).  Every
// double operation is correctly rounded and none fused, so this file is
// compiled with -ffp-contract=off and says so again below.
// -DMXD_WARP_CUBIC_NO_LDS (diagnostic builds): nothing is staged.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "resample.h"

#pragma clang fp contract(off)

namespace mxd {
namespace {

constexpr int kThreads = 256;
constexpr int kGroups = kWarpTileW / 4;  // lanes per tile row
static_assert(kGroups * kWarpTileH == kThreads, "a lane per four pixels of the tile");
// 20 KiB: eight workgroups, the 32 waves a compute unit holds, fit its 160 KiB;
// a tile rotated by 45 degrees needs 61 rows of 64 dwords.
#ifdef MXD_WARP_CUBIC_NO_LDS
constexpr int kBoxDwords = 4;
#else
constexpr int kBoxDwords = 5120;
#endif

using WarpRowK = const __attribute__((address_space(4))) WarpRowDev;
using dev::fetch_rgb;

// Pillow's BICUBIC macro: the cubic convolution with a = -1.
__device__ __forceinline__ double cub(double v1, double v2, double v3, double v4, double d) {
  const double p2 = -v1 + v3;
  const double p3 = ((2.0 * (v1 - v2)) + v3) - v4;
  const double p4 = ((-v1 + v2) - v3) + v4;
  return v2 + d * (p2 + d * (p3 + d * p4));
}

__device__ __forceinline__ double chan(uint32_t p, int c) { return (double)((p >> (8 * c)) & 255u); }

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(kThreads) void warp_cubic_rows(const void* __restrict__ rows, int nimgs, int tile_first) {
  __shared__ __attribute__((aligned(16))) uint32_t box[kBoxDwords];
  WarpRowK* rk = (WarpRowK*)rows;
  const int blk = (int)blockIdx.x + tile_first;
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rk[mid].tile_begin <= blk) lo = mid; else hi = mid - 1;
  }
  WarpRowK& e = rk[lo];
  if (e.path != kWarpCubic) return;  // warp_rows' image (uniform)
  const int w = e.w, h = e.h;
  const int t = blk - e.tile_begin;
  const int tyb = t / e.tiles_x;
  const int ty0 = tyb * kWarpTileH, tx0 = (t - tyb * e.tiles_x) * kWarpTileW;
  const uint8_t* const src = e.src;
  const int64_t sstride = e.src_stride;
  const int64_t limit = sstride * h;
  const double m0 = e.m[0], m1 = e.m[1], m2 = e.m[2], m3 = e.m[3], m4 = e.m[4], m5 = e.m[5];

  // ---- the tile's source box --------------------------------------------------------------
  const double cx[2] = {(double)tx0 + 0.5, (double)min(tx0 + kWarpTileW - 1, w - 1) + 0.5};
  const double cy[2] = {(double)ty0 + 0.5, (double)min(ty0 + kWarpTileH - 1, h - 1) + 0.5};
  double xmin = 0.0, xmax = 0.0, ymin = 0.0, ymax = 0.0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const double sx = ((m0 * cx[c & 1]) + (m1 * cy[c >> 1])) + m2;
    const double sy = ((m3 * cx[c & 1]) + (m4 * cy[c >> 1])) + m5;
    xmin = c == 0 ? sx : fmin(xmin, sx), xmax = c == 0 ? sx : fmax(xmax, sx);
    ymin = c == 0 ? sy : fmin(ymin, sy), ymax = c == 0 ? sy : fmax(ymax, sy);
  }
  // (validation bounds every position by 32768: the conversions are in range)
  const int lox = uniform((int)floor(xmin - 0.5) - 2), hix = uniform((int)floor(xmax - 0.5) + 3);
  const int loy = uniform((int)floor(ymin - 0.5) - 2), hiy = uniform((int)floor(ymax - 0.5) + 3);
  const int bx0 = max(lox, 0) & ~3, bx1 = min(hix, w - 1);
  const int by0 = max(loy, 0), by1 = min(hiy, h - 1);
  const int S = (bx1 - bx0 + 4) & ~3;  // the box's row in LDS: dwords, a multiple of 4
  bool staged = hix >= 0 && lox <= w - 1 && hiy >= 0 && loy <= h - 1 &&
                (int64_t)S * (by1 - by0 + 1) <= (int64_t)kBoxDwords;
#ifdef MXD_WARP_CUBIC_NO_LDS
  staged = false;
#endif

  // ---- staging ---------------------------------------------------------------------------
  if (staged) {
    const int G = S >> 2, items = G * (by1 - by0 + 1);
    for (int it = (int)threadIdx.x; it < items; it += kThreads) {
      const int r = it / G, g = it - r * G;
      // pixels bx0 + 4 g .. + 3 of row by0 + r: the first is inside the image (bx0 + 4 g <= bx1)
      const int64_t off = 3 * (int64_t)bx0 + 12 * (int64_t)g;  // a multiple of 4, < stride
      const uint32_t* const p = reinterpret_cast<const uint32_t*>(src + (int64_t)(by0 + r) * sstride + off);
      uint32_t d0 = p[0], d1 = 0, d2 = 0;
      if (off + 8 <= sstride) d1 = p[1];
      if (off + 12 <= sstride) d2 = p[2];
      uint4 v;
      v.x = d0 & 0xffffffu;
      v.y = (d0 >> 24 | d1 << 8) & 0xffffffu;
      v.z = (d1 >> 16 | d2 << 16) & 0xffffffu;
      v.w = d2 >> 8;
      *reinterpret_cast<uint4*>(&box[r * S + 4 * g]) = v;
    }
  }
  __syncthreads();

  // ---- the lane's four pixels -----------------------------------------------------------
  const int y = ty0 + (int)threadIdx.x / kGroups;
  const int x0 = tx0 + ((int)threadIdx.x % kGroups) * 4;
  if (y >= h || x0 >= w) return;
  const int cnt = min(4, w - x0);
  const uint32_t fill = e.fill;
  uint32_t px[4] = {fill, fill, fill, fill};
  const double yc5 = (double)y + 0.5;
  const double ty = m1 * yc5, uy = m4 * yc5;
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
    const double dx = sx - fx, dy = sy - fy;
    const int X = (int)fx - 1, Y = (int)fy - 1;
    int xk[4];
#pragma unroll
    for (int i = 0; i < 4; i++) xk[i] = min(max(X + i, 0), w - 1);
    // (the clamped columns do not decrease: the first and the last bound them)
    const bool cols_in = staged && xk[0] >= bx0 && xk[3] <= bx1;
    double r[4][3];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool have = j == 0 || (Y + j >= 0 && Y + j < h);
      if (have) {
        const int yy = j == 0 ? min(max(Y, 0), h - 1) : Y + j;
        uint32_t tp[4];
        if (cols_in && yy >= by0 && yy <= by1) {
          const int at = (yy - by0) * S - bx0;
#pragma unroll
          for (int i = 0; i < 4; i++) tp[i] = box[at + xk[i]];
        } else {
#pragma unroll
          for (int i = 0; i < 4; i++) tp[i] = fetch_rgb(src, limit, (int64_t)yy * sstride + 3 * xk[i]);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) r[j][c] = cub(chan(tp[0], c), chan(tp[1], c), chan(tp[2], c), chan(tp[3], c), dx);
      } else {
#pragma unroll
        for (int c = 0; c < 3; c++) r[j][c] = r[j - 1][c];  // (j >= 1: row 0 is always there)
      }
    }
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double v = cub(r[0][c], r[1][c], r[2][c], r[3][c], dy);
      const uint32_t b = v <= 0.0 ? 0u : v >= 255.0 ? 255u : (uint32_t)(int)v;
      o |= b << (8 * c);
    }
    px[k] = o;
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

int launch_warp_cubic(const WarpRowDev* rows, int nimgs, int tile_first, int tile_end, void* stream) {
  if (nimgs <= 0 || tile_end <= tile_first) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(warp_cubic_rows, dim3(tile_end - tile_first), dim3(kThreads), 0, s, static_cast<const void*>(rows),
                     nimgs, tile_first);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
