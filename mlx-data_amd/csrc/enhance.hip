// enhance.hip -- the enhance stage (resample.h): Pillow's ImageEnhance
// Sharpness / Color / Brightness of u8 RGB scratch rows, behind the resize
// launches (and the warp stage) and before the second pass of an enhance call.
// One launch covers every image of a call; no kernel waits on another
// workgroup.
//
// enhance_rows  warp_rows' shape: a workgroup of 256 lanes owns a 64 x 16 pixel
//               output tile, a lane four adjacent pixels of a row (12 bytes,
//               three aligned dwords of the scratch row) and one 12-byte store
//               where the destination is 4-byte aligned (element stores for row
//               tails and misaligned destinations).  The image's entry is read
//               through a uniform (scalar) address and its op chosen by a
//               uniform branch.
//               SHARPNESS reads the 3 x 3 neighbourhoods of its four
//               pixels as 3 rows x 5 aligned dwords (the lane's twelve bytes,
//               the dword before and the dword after) straight from the scratch
//               rows, through L1 / L2: each row is clamped to the window and
//               each offset into the row, so no address outside the image's own
//               stride x h bytes is formed (a clamped dword is read by ring
//               pixels only, which do not use it), and the twelve sums are
//               integer.  -DMXD_ENH_LDS builds the form that stages the tile
//               and its one-pixel halo in LDS first (18 rows of 50 dwords, one
//               barrier that no lane leaves before): measured 3 % (C2) to 5 %
//               (C4) slower per call, kept for that
//               comparison.
//               COLOR, BRIGHTNESS and NONE load their three dwords only.
//
// Arithmetic: Pillow's, bit for bit; the CPU statement
// is enhance.cpp's.  Every float operation of the blend is correctly rounded
// and none fused, so this file is compiled with -ffp-contract=off and says so
// again below.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "resample.h"

#pragma clang fp contract(off)

namespace mxd {
namespace {

constexpr int kThreads = 256;
constexpr int kGroups = kEnhTileW / 4;               // lanes per tile row
#ifdef MXD_ENH_LDS
constexpr int kHaloRows = kEnhTileH + 2;             // the tile's rows, one above, one below
constexpr int kHaloWords = (kEnhTileW * 3 + 8) / 4;  // the tile's bytes, the dword before, the dword after
#endif
static_assert(kGroups * kEnhTileH == kThreads, "a lane per four pixels of the tile");
static_assert((kEnhTileW * 3) % 4 == 0, "a tile row starts at a dword of the scratch row");

using EnhRowK = const __attribute__((address_space(4))) EnhanceRowDev;

// Byte k of the little-endian dwords v.
__device__ __forceinline__ int byte_of(const uint32_t* v, int k) { return (int)((v[k >> 2] >> (8 * (k & 3))) & 255u); }

// Image.blend(degenerate, image, f) of one byte, float32, nothing fused.
// unit: 0 <= f <= 1, where Pillow does not clip (x lies between d and q).
__device__ __forceinline__ uint32_t blend(int d, int q, float f, bool unit) {
  const float diff = (float)(q - d);
  const float fd = f * diff;
  const float x = (float)d + fd;
  const float c = unit ? x : fminf(fmaxf(x, 0.0f), 255.0f);
  return (uint32_t)(int)c;
}

__global__ __launch_bounds__(kThreads) void enhance_rows(const void* __restrict__ rows, int nimgs) {
#ifdef MXD_ENH_LDS
  __shared__ uint32_t halo[kHaloRows * kHaloWords];
#endif
  EnhRowK* rk = (EnhRowK*)rows;
  const int blk = blockIdx.x;
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rk[mid].tile_begin <= blk) lo = mid; else hi = mid - 1;
  }
  EnhRowK& e = rk[lo];
  const int w = e.w, h = e.h;
  const int t = blk - e.tile_begin;
  const int tyb = t / e.tiles_x, txb = t - tyb * e.tiles_x;
  const int gy = (int)threadIdx.x / kGroups, gx = (int)threadIdx.x % kGroups;
  const int y = tyb * kEnhTileH + gy;
  const int x0 = txb * kEnhTileW + gx * 4;
  const bool active = y < h && x0 < w;
  const int cnt = min(4, w - x0);
  const uint8_t* const src = e.src;
  const int64_t sstride = e.src_stride;
  const int op = e.op;
  const float f = e.factor;
  const bool unit = f >= 0.0f && f <= 1.0f;
  uint32_t out[3] = {0, 0, 0};  // the lane's twelve result bytes
  if (op == kEnhSharpness) {
    const int64_t bx = (int64_t)txb * (kEnhTileW * 3) - 4;
    // bytes 0..19 of the three rows from the dword before the lane's pixels; its own are 4..15
    uint32_t r0[5], r1[5], r2[5];
#ifdef MXD_ENH_LDS
    for (int i = (int)threadIdx.x; i < kHaloRows * kHaloWords; i += kThreads) {
      const int r = i / kHaloWords, c = i - r * kHaloWords;
      const int yy = min(max(tyb * kEnhTileH - 1 + r, 0), h - 1);
      const int64_t o = min(max(bx + 4 * c, (int64_t)0), sstride - 4);
      halo[i] = *reinterpret_cast<const uint32_t*>(src + (int64_t)yy * sstride + o);
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int j = 0; j < 5; j++) {
        r0[j] = halo[gy * kHaloWords + 3 * gx + j];
        r1[j] = halo[(gy + 1) * kHaloWords + 3 * gx + j];
        r2[j] = halo[(gy + 2) * kHaloWords + 3 * gx + j];
      }
#else
    if (active) {
      const int64_t ya = (int64_t)max(y - 1, 0) * sstride, yb = (int64_t)y * sstride;
      const int64_t yc = (int64_t)min(y + 1, h - 1) * sstride;
#pragma unroll
      for (int j = 0; j < 5; j++) {
        const int64_t o = min(max(bx + 4 * (3 * gx + j), (int64_t)0), sstride - 4);
        r0[j] = *reinterpret_cast<const uint32_t*>(src + ya + o);
        r1[j] = *reinterpret_cast<const uint32_t*>(src + yb + o);
        r2[j] = *reinterpret_cast<const uint32_t*>(src + yc + o);
      }
#endif
      int col[20];
#pragma unroll
      for (int k = 1; k < 19; k++) col[k] = byte_of(r0, k) + byte_of(r1, k) + byte_of(r2, k);
      const bool yring = y == 0 || y == h - 1;
#pragma unroll
      for (int k = 0; k < 12; k++) {
        const int x = x0 + k / 3;
        const int qc = byte_of(r1, k + 4);
        const int s = col[k + 1] + col[k + 4] + col[k + 7] + 4 * qc;
        const bool ring = yring || x == 0 || x >= w - 1;  // (x >= w: a tail pixel, not stored)
        const int d = ring ? qc : (2 * s + 13) / 26;
        out[k >> 2] |= blend(d, qc, f, unit) << (8 * (k & 3));
      }
    }
  } else if (active) {
    const int64_t limit = sstride * h;
    const int64_t ro = (int64_t)y * sstride + 3 * (int64_t)x0;
    uint32_t q[3];
#pragma unroll
    for (int j = 0; j < 3; j++) q[j] = *reinterpret_cast<const uint32_t*>(src + min(ro + 4 * j, limit - 4));
    if (op == kEnhNone) {
      out[0] = q[0], out[1] = q[1], out[2] = q[2];
    } else {
#pragma unroll
      for (int p = 0; p < 4; p++) {
        const int q0 = byte_of(q, 3 * p), q1 = byte_of(q, 3 * p + 1), q2 = byte_of(q, 3 * p + 2);
        const int d = op == kEnhColor
                          ? (int)((19595u * (uint32_t)q0 + 38470u * (uint32_t)q1 + 7471u * (uint32_t)q2 + 32768u) >> 16)
                          : 0;
        const int qs[3] = {q0, q1, q2};
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const int k = 3 * p + c;
          out[k >> 2] |= blend(d, qs[c], f, unit) << (8 * (k & 3));
        }
      }
    }
  }
  if (!active) return;
  uint8_t* const d = e.dst + (int64_t)y * e.dst_stride + 3 * (int64_t)x0;
  const bool wide = ((reinterpret_cast<uint64_t>(e.dst) | (uint64_t)e.dst_stride) & 3) == 0;
  if (wide && cnt == 4) {
    uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
    d4[0] = out[0];
    d4[1] = out[1];
    d4[2] = out[2];
  } else {
#pragma unroll
    for (int k = 0; k < 12; k++)
      if (k < 3 * cnt) d[k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
  }
}

}  // namespace

int launch_enhance(const EnhanceRowDev* rows, int nimgs, int ntiles, void* stream) {
  if (nimgs <= 0 || ntiles <= 0) return 0;
  hipLaunchKernelGGL(enhance_rows, dim3(ntiles), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const void*>(rows), nimgs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
