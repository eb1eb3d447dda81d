// mix.hip -- the mix stage (resample.h): the last stage of a mix call.  u8 RGB
// scratch rows of two images of the call -> MixUp / CutMix of their bytes ->
// the call's output form (u8, or the elements of an mxd_out_format table, HWC
// or CHW).  One launch covers every image of the call.
//
// mix_rows     a workgroup takes kMixRows rows of one image, found by
//              image_of_block over blk_begin, reads the image's entry through
//              a uniform (scalar) address and copies the format's table into
//              LDS once.  A lane owns four adjacent pixels: 12 own bytes as
//              three dwords and, unless the op is NONE, the partner's 12 bytes
//              at the same place as three more (both from scratch rows that
//              start at 16-byte multiples of 256-byte aligned bases, so the
//              lanes of a wave read contiguous bytes), the 12 new bytes
//              computed in registers, then pixel_rows' store forms: packed
//              dwords for u8, the widest nontemporal stores the destination's
//              alignment allows for f32 / 16-bit elements, HWC and CHW --
//              tested once per workgroup on the image's base and strides, so
//              the branch is uniform.  A row's last w mod 4 pixels and
//              misaligned destinations take element stores.  The op is uniform
//              per workgroup; CutMix selects per pixel (a box edge falls inside
//              a lane's quad) and loads the partner's bytes only in the lanes
//              whose quad meets the box.
//
// The kernel waits on no other workgroup.  Both images' rows were written by
// the launch before it on the same stream, and nothing in this launch writes
// them: every image reads unmixed bytes, whatever the order of the workgroups.
//
// Arithmetic: x = (float)q * w_self + (float)r * w_other
// in float32, each operation correctly rounded and none fused, then round
// half to even (v_rndne_f32) -- NumPy's, and the CPU statement's
// (mxd_mix_apply_u8).  So this file is compiled with -ffp-contract=off and
// says so again below.  (The store forms restate row_stage.hip's pixel_rows:
// that kernel stays as it is.)
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

using MixRowK = const __attribute__((address_space(4))) MixRowDev;

template <class T>
__device__ __forceinline__ void nt(char* p, T v) {
  __builtin_nontemporal_store(v, MXD_GLOBAL_PTR(T, p));
}

// The image of workgroup blk: the last of nimgs whose first workgroup is <= blk.
__device__ __forceinline__ int image_of_block(MixRowK* rows, int nimgs, int blk) {
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].blk_begin <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The twelve bytes of a lane's four pixels (npx of them exist) into `in`,
// which the caller zeroed.
__device__ __forceinline__ void load_px(const uint8_t* s, int npx, uint32_t (&in)[3]) {
  if (npx == 4) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
    in[0] = s4[0], in[1] = s4[1], in[2] = s4[2];
  } else {
#pragma unroll
    for (int k = 0; k < 9; k++)
      if (k < 3 * npx) in[k >> 2] |= (uint32_t)s[k] << (8 * (k & 3));
  }
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&in)[3], int k) { return (in[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// ES: bytes per output element (1: u8, no format table); CHW: channel planes.
template <int ES, bool CHW>
__global__ __launch_bounds__(kThreads) void mix_rows(const MixRowDev* __restrict__ rows, int nimgs, OutFmtDev fmt) {
  __shared__ uint32_t tab[ES > 1 ? 3 * 256 : 1];
  const int blk = blockIdx.x;
  MixRowK* rk = (MixRowK*)rows;
  MixRowK& im = rk[image_of_block(rk, nimgs, blk)];
  if constexpr (ES > 1) {
    for (int i = threadIdx.x; i < 3 * 256; i += kThreads)
      tab[i] = ES == 2 ? (uint32_t)static_cast<const uint16_t*>(fmt.table)[i] : static_cast<const uint32_t*>(fmt.table)[i];
    __syncthreads();
  }
  const int w = im.w, h = im.h;
  const int op = im.op;
  const float ws = im.w_self, wo = im.w_other;
  const int bx0 = im.x0, bx1 = im.x1, by0 = im.y0, by1 = im.y1;
  const int y0 = (blk - im.blk_begin) * kMixRows;
  const int nrows = min(kMixRows, h - y0);
  const int nq = (w + 3) >> 2;  // lanes per row
  const int64_t sstride = im.src_stride, pstride = im.psrc_stride, dstride = im.dst_stride;
  const uint8_t* const sbase = im.src + (int64_t)y0 * sstride;
  const uint8_t* const pbase = im.psrc + (int64_t)y0 * pstride;  // (kMixNone: never read)
  char* const dbase = static_cast<char*>(im.dst) + (int64_t)y0 * dstride;
  // widest store of a lane: 4 bytes (u8), 16 (f32), 8 (16-bit elements)
  constexpr int kAlign = ES == 1 ? 4 : ES == 4 ? 16 : 8;
  const uint64_t bits = reinterpret_cast<uint64_t>(im.dst) | (uint64_t)dstride | (CHW ? (uint64_t)fmt.plane_stride : 0);
  const bool wide = (bits & (kAlign - 1)) == 0;
  for (int it = threadIdx.x; it < nrows * nq; it += kThreads) {
    const int r = it / nq, qx = it - r * nq;
    const int npx = min(4, w - 4 * qx);
    uint32_t in[3] = {0, 0, 0};
    load_px(sbase + r * sstride + 12 * qx, npx, in);
    uint32_t o[12];
    if (op == kMixMixup) {
      uint32_t pin[3] = {0, 0, 0};
      load_px(pbase + r * pstride + 12 * qx, npx, pin);
#pragma unroll
      for (int k = 0; k < 12; k++) {
        const float a = (float)byte_of(in, k) * ws;
        const float b = (float)byte_of(pin, k) * wo;
        const float x = a + b;
        o[k] = (uint32_t)fminf(__builtin_rintf(x), 255.0f);
      }
    } else if (op == kMixCutmix) {
      const int y = y0 + r, x = 4 * qx;
      const bool touches = y >= by0 && y < by1 && x < bx1 && x + npx > bx0;
      uint32_t pin[3] = {0, 0, 0};
      if (touches) load_px(pbase + r * pstride + 12 * qx, npx, pin);
#pragma unroll
      for (int k = 0; k < 12; k++) {
        const bool inside = touches && x + k / 3 >= bx0 && x + k / 3 < bx1;
        o[k] = inside ? byte_of(pin, k) : byte_of(in, k);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 12; k++) o[k] = byte_of(in, k);
    }
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

int launch_mix(const MixRowDev* rows, int nimgs, int nblocks, const OutFmtDev& fmt, void* stream) {
  if (nimgs <= 0 || nblocks <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(nblocks), block(kThreads);
  if (!fmt.table) hipLaunchKernelGGL((mix_rows<1, false>), grid, block, 0, s, rows, nimgs, fmt);
  else if (fmt.elem16 && fmt.chw) hipLaunchKernelGGL((mix_rows<2, true>), grid, block, 0, s, rows, nimgs, fmt);
  else if (fmt.elem16) hipLaunchKernelGGL((mix_rows<2, false>), grid, block, 0, s, rows, nimgs, fmt);
  else if (fmt.chw) hipLaunchKernelGGL((mix_rows<4, true>), grid, block, 0, s, rows, nimgs, fmt);
  else hipLaunchKernelGGL((mix_rows<4, false>), grid, block, 0, s, rows, nimgs, fmt);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
