// color_rows.hip -- the second pass of a colour call (mxd_color): u8 RGB
// scratch rows -> the per-image 3 x 4 map of the result bytes -> the call's
// output form (u8, or the elements of an mxd_out_format table, HWC or CHW).
// One launch covers every image of a call.  A workgroup takes kColorRows rows
// of one image, reads the image's matrix through a uniform (scalar) address
// and, when the output has a table, copies it into LDS once.  A lane owns four
// adjacent pixels: 12 source bytes as three dwords (scratch rows start at
// 16-byte multiples of 256-byte aligned bases, so the lanes of a wave read
// contiguous bytes), the 12 new bytes computed in registers, then the widest
// nontemporal stores the destination's alignment allows -- tested once per
// workgroup on the image's base and strides, so the branch is uniform.  A
// row's last w mod 4 pixels and misaligned destinations take element stores.
//
// Arithmetic: float32 operations, each correctly
// rounded, none fused -- this file is compiled with -ffp-contract=off and says
// so again below, because the CPU statement (mxd_color_apply_u8) and NumPy
// round every product and sum.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "resample.h"

#pragma clang fp contract(off)

namespace mxd {
namespace {

constexpr int kThreads = 256;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4a8 __attribute__((aligned(8)));

using ColorRowK = const __attribute__((address_space(4))) ColorRowDev;

template <class T>
__device__ __forceinline__ void nt(char* p, T v) {
  __builtin_nontemporal_store(v, MXD_GLOBAL_PTR(T, p));
}

// The twelve bytes of four pixels -> their twelve new bytes.
__device__ __forceinline__ void twist(const float (&m)[12], const uint32_t (&in)[3], uint32_t (&out)[12]) {
  float q[12];
#pragma unroll
  for (int k = 0; k < 12; k++) q[k] = (float)((in[k >> 2] >> (8 * (k & 3))) & 0xffu);
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float v = ((m[4 * c] * q[3 * p] + m[4 * c + 1] * q[3 * p + 1]) + m[4 * c + 2] * q[3 * p + 2]) + m[4 * c + 3];
      out[3 * p + c] = (uint32_t)dev::encode(v);
    }
}

// ES: bytes per output element (1: u8, no table); CHW: channel planes.
template <int ES, bool CHW>
__global__ __launch_bounds__(kThreads) void color_rows(const ColorRowDev* __restrict__ rows, int nimgs, OutFmtDev fmt) {
  __shared__ uint32_t tab[ES > 1 ? 3 * 256 : 1];
  const int blk = blockIdx.x;
  ColorRowK* rk = (ColorRowK*)rows;
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rk[mid].blk_begin <= blk) lo = mid; else hi = mid - 1;
  }
  ColorRowK& im = rk[lo];
  float m[12];
#pragma unroll
  for (int k = 0; k < 12; k++) m[k] = im.m[k];
  const int w = im.crop_w, h = im.crop_h;
  if constexpr (ES > 1) {
    for (int i = threadIdx.x; i < 3 * 256; i += kThreads)
      tab[i] = ES == 2 ? (uint32_t)static_cast<const uint16_t*>(fmt.table)[i] : static_cast<const uint32_t*>(fmt.table)[i];
    __syncthreads();
  }
  const int y0 = (blk - im.blk_begin) * kColorRows;
  const int nrows = min(kColorRows, h - y0);
  const int nq = (w + 3) >> 2;  // lanes per row
  const int64_t sstride = im.src_stride, dstride = im.dst_stride;
  const uint8_t* const sbase = im.src + (int64_t)y0 * sstride;
  char* const dbase = static_cast<char*>(im.dst) + (int64_t)y0 * dstride;
  // widest store of a lane: 4 bytes (u8), 16 (f32), 8 (16-bit elements)
  constexpr int kAlign = ES == 1 ? 4 : ES == 4 ? 16 : 8;
  const uint64_t bits = reinterpret_cast<uint64_t>(im.dst) | (uint64_t)dstride | (CHW ? (uint64_t)fmt.plane_stride : 0);
  const bool wide = (bits & (kAlign - 1)) == 0;
  for (int it = threadIdx.x; it < nrows * nq; it += kThreads) {
    const int r = it / nq, qx = it - r * nq;
    const int npx = min(4, w - 4 * qx);
    const uint8_t* s = sbase + r * sstride + 12 * qx;
    uint32_t in[3] = {0, 0, 0};
    if (npx == 4) {
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
      in[0] = s4[0], in[1] = s4[1], in[2] = s4[2];
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++)
        if (k < 3 * npx) in[k >> 2] |= (uint32_t)s[k] << (8 * (k & 3));
    }
    uint32_t o[12];
    twist(m, in, o);
    char* d = dbase + r * dstride;
    if constexpr (ES == 1) {
      d += 12 * qx;
      if (wide && npx == 4) {
#pragma unroll
        for (int k = 0; k < 3; k++)
          nt<uint32_t>(d + 4 * k, o[4 * k] | o[4 * k + 1] << 8 | o[4 * k + 2] << 16 | o[4 * k + 3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 12; k++)
          if (k < 3 * npx) nt<uint8_t>(d + k, (uint8_t)o[k]);
      }
    } else {
      uint32_t e[12];
#pragma unroll
      for (int k = 0; k < 12; k++) e[k] = tab[(k % 3) * 256 + o[k]];
      if constexpr (!CHW) {
        d += 12 * ES * qx;
        if (wide && npx == 4) {
          if constexpr (ES == 4) {
#pragma unroll
            for (int k = 0; k < 3; k++) nt<u32x4>(d + 16 * k, u32x4{e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3]});
          } else {
            nt<u32x4a8>(d, u32x4a8{e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16});
            nt<u32x2>(d + 16, u32x2{e[8] | e[9] << 16, e[10] | e[11] << 16});
          }
        } else {
#pragma unroll
          for (int k = 0; k < 12; k++) {
            if (k >= 3 * npx) break;
            if constexpr (ES == 4) nt<uint32_t>(d + 4 * k, e[k]);
            else nt<uint16_t>(d + 2 * k, (uint16_t)e[k]);
          }
        }
      } else {
        d += 4 * ES * qx;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          char* p = d + c * fmt.plane_stride;
          if (wide && npx == 4) {
            if constexpr (ES == 4) nt<u32x4>(p, u32x4{e[c], e[3 + c], e[6 + c], e[9 + c]});
            else nt<u32x2>(p, u32x2{e[c] | e[3 + c] << 16, e[6 + c] | e[9 + c] << 16});
          } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
              if (k >= npx) break;
              if constexpr (ES == 4) nt<uint32_t>(p + 4 * k, e[3 * k + c]);
              else nt<uint16_t>(p + 2 * k, (uint16_t)e[3 * k + c]);
            }
          }
        }
      }
    }
  }
}

}  // namespace

int launch_color_rows(const ColorRowDev* rows, int nimgs, int nblocks, const OutFmtDev& fmt, void* stream) {
  if (nimgs <= 0 || nblocks <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(nblocks), block(kThreads);
  if (!fmt.table) hipLaunchKernelGGL((color_rows<1, false>), grid, block, 0, s, rows, nimgs, fmt);
  else if (fmt.elem16 && fmt.chw) hipLaunchKernelGGL((color_rows<2, true>), grid, block, 0, s, rows, nimgs, fmt);
  else if (fmt.elem16) hipLaunchKernelGGL((color_rows<2, false>), grid, block, 0, s, rows, nimgs, fmt);
  else if (fmt.chw) hipLaunchKernelGGL((color_rows<4, true>), grid, block, 0, s, rows, nimgs, fmt);
  else hipLaunchKernelGGL((color_rows<4, false>), grid, block, 0, s, rows, nimgs, fmt);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
