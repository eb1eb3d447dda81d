// hue.hip -- Pillow's HSV hue shift of the enhance stage (resample.h): the
// images of an enhance call whose op is MXD_ENHANCE_PIL_HUE, the hue part of
// torchvision's ColorJitter on a PIL image: convert("HSV"), H += shift modulo
// 256, convert("RGB"), byte for byte (mxd_amd.h).
// hue_rows runs in the enhance stage's slot of the chain, behind enhance_rows,
// blur_rows and pilblur_rows on the same stream, reads and writes the rows
// that stage does (the images' own EnhanceRowDev entries) and takes the images
// none of the three has a unit for.  One launch covers every such image of a
// call; no workgroup waits on another.
//
// hue_rows  pixel_rows' shape: the op is pointwise, so a workgroup of 256 lanes
//           takes kHueRows whole rows of one image, found from blockIdx by the
//           binary search over unit_begin, and a lane four adjacent pixels at a
//           time: three aligned dwords of the scratch row in, twelve bytes out
//           as three dword stores where the destination base and stride are
//           4-byte aligned (tested once per workgroup), element loads and
//           stores for a row's tail and element stores for a misaligned
//           destination.  No address outside a row's own 3 w bytes is formed.
//
//           tables  the second conversion's sector i mod 6 and fraction f
//                   depend on H' only, and its fs on S only.  Once per
//                   workgroup lane v computes all three for the byte v into
//                   256-entry LDS tables (one barrier, before any lane leaves):
//                   the two float64 divisions by 255 and the floor leave the
//                   per-pixel path.  The tables do not depend on the shift,
//                   which is added to H per pixel.
//           pixel   RGB -> HSV is three float32 divisions (s and the two of
//                   rc, gc, bc that the branch of the maximum reads: the third
//                   is 0 or unused), one float64 sum rounded to float32 -- the
//                   float32 difference bc - gc of the red branch is the same
//                   rounding of the same exact double difference, so the three
//                   branches are one instruction stream with selected
//                   operands --, the float64 division by 6 and two truncations.
//                   HSV -> RGB reads f, fs and the sector from LDS and needs p
//                   and only one of q and t (odd sectors read q, even ones t):
//                   two float64 products and two roundings, then selects.
//                   A grey pixel (V == min) takes the same stream with its
//                   divisors replaced by 1: its S is 0, and the S == 0 select
//                   at the end returns (V, V, V).  No divergent branch.
//
// Matrix instructions do not fit: the work is per pixel, divisions and
// roundings at prescribed precisions, with no product shared between pixels.
// Every float operation is rounded where the statement says and none is fused,
// so this file is compiled with -ffp-contract=off and says so again below;
// float32 division is the correctly rounded one (no fast-math switch).  The
// CPU statement is enhance.cpp's; the two share no code.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "resample.h"

#pragma clang fp contract(off)

namespace mxd {
namespace {

constexpr int kThreads = 256;

using EnhRowK = const __attribute__((address_space(4))) EnhanceRowDev;
using HueRecK = const __attribute__((address_space(4))) HueRecDev;

// What H' and S mean to hsv2rgb, for every byte.
struct HueTables {
  float f[256];     // f32(hf - floor(hf)), hf = f32(H') 6 / 255
  int sector[256];  // floor(hf) mod 6
  float fs[256];    // f32(S / 255)
};

// One pixel: q = r | g << 8 | b << 16 -> the same packing of the result.
__device__ __forceinline__ uint32_t hue_pixel(uint32_t q, int shift, const HueTables& tab) {
  const int r = (int)(q & 255u), g = (int)((q >> 8) & 255u), b = (int)((q >> 16) & 255u);
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  const bool grey = maxc == minc;
  // rgb2hsv
  const float cr = grey ? 1.0f : (float)(maxc - minc);
  const float s = (float)(maxc - minc) / (grey ? 1.0f : (float)maxc);
  const bool rmax = r == maxc, gmax = g == maxc;
  const int n1 = maxc - (rmax ? b : gmax ? r : g), n2 = maxc - (rmax ? g : gmax ? b : r);
  const double off = rmax ? 0.0 : gmax ? 2.0 : 4.0;
  const float c1 = (float)n1 / cr, c2 = (float)n2 / cr;
  const float h6 = (float)(off + (double)c1 - (double)c2);  // (both sums exact in double: one rounding)
  const double x = (double)h6 / 6.0 + 1.0;                  // in [5/6, 11/6]: x - floor(x) is fmod(x, 1)
  const float h = (float)(x - floor(x));
  const int H = min((int)((double)h * 255.0), 255);
  const int S = min((int)((double)s * 255.0), 255);
  // the shift, then hsv2rgb
  const int Hs = (H + shift) & 255;
  const float f = tab.f[Hs], fs = tab.fs[S];
  const int sector = tab.sector[Hs];
  const double V = (double)maxc;
  const bool odd = (sector & 1) != 0;
  const float fsf = fs * f;
  const double mix = odd ? (double)fsf : (double)fs * (1.0 - (double)f);
  const int p = min((int)round(V * (1.0 - (double)fs)), 255);
  const int m = min((int)round(V * (1.0 - mix)), 255);  // q in odd sectors, t in even ones
  // sectors 0..5: (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q)
  int R = sector == 0 || sector == 5 ? maxc : sector == 1 || sector == 4 ? m : p;
  int G = sector == 1 || sector == 2 ? maxc : sector == 0 || sector == 3 ? m : p;
  int B = sector == 3 || sector == 4 ? maxc : sector == 2 || sector == 5 ? m : p;
  if (S == 0) R = G = B = maxc;
  return (uint32_t)R | (uint32_t)G << 8 | (uint32_t)B << 16;
}

__global__ __launch_bounds__(kThreads) void hue_rows(const void* __restrict__ rows, const void* __restrict__ recs,
                                                     int nrecs) {
  __shared__ HueTables tab;
  {
    const int v = (int)threadIdx.x;
    const double hf = (double)(float)v * 6.0 / 255.0;
    const double fl = floor(hf);
    tab.f[v] = (float)(hf - fl);
    tab.sector[v] = (int)fl % 6;  // (H' = 255: floor(hf) = 6, sector 0)
    tab.fs[v] = (float)((double)v / 255.0);
  }
  __syncthreads();
  HueRecK* hk = (HueRecK*)recs;
  const int blk = blockIdx.x;
  int lo = 0, hi = nrecs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (hk[mid].unit_begin <= blk) lo = mid; else hi = mid - 1;
  }
  HueRecK& rec = hk[lo];
  EnhRowK& e = ((EnhRowK*)rows)[rec.entry];
  const int w = e.w, h = e.h;
  const int shift = rec.shift & 255;
  const int y0 = (blk - rec.unit_begin) * kHueRows;
  const int nrows = min(kHueRows, h - y0);
  const int nq = (w + 3) >> 2;  // lanes per row
  const int64_t sstride = e.src_stride, dstride = e.dst_stride;
  const uint8_t* const sbase = e.src + (int64_t)y0 * sstride;
  uint8_t* const dbase = e.dst + (int64_t)y0 * dstride;
  const bool wide = ((reinterpret_cast<uint64_t>(e.dst) | (uint64_t)dstride) & 3) == 0;
  for (int it = (int)threadIdx.x; it < nrows * nq; it += kThreads) {
    const int r = it / nq, qx = it - r * nq;
    const int npx = min(4, w - 4 * qx);
    const uint8_t* const s = sbase + r * sstride + 12 * qx;
    uint32_t in[3] = {0, 0, 0};
    if (npx == 4) {  // (a scratch row starts at a multiple of 16 bytes)
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
      in[0] = s4[0], in[1] = s4[1], in[2] = s4[2];
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++)
        if (k < 3 * npx) in[k >> 2] |= (uint32_t)s[k] << (8 * (k & 3));
    }
    // the four pixels out of the twelve bytes, and back
    const uint32_t o0 = hue_pixel(in[0] & 0xffffffu, shift, tab);
    const uint32_t o1 = hue_pixel((in[0] >> 24 | in[1] << 8) & 0xffffffu, shift, tab);
    const uint32_t o2 = hue_pixel((in[1] >> 16 | in[2] << 16) & 0xffffffu, shift, tab);
    const uint32_t o3 = hue_pixel(in[2] >> 8, shift, tab);
    const uint32_t out[3] = {o0 | o1 << 24, o1 >> 8 | o2 << 16, o2 >> 16 | o3 << 8};
    uint8_t* const d = dbase + r * dstride + 12 * qx;
    if (wide && npx == 4) {
      uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
      d4[0] = out[0];
      d4[1] = out[1];
      d4[2] = out[2];
    } else {
#pragma unroll
      for (int k = 0; k < 12; k++)
        if (k < 3 * npx) d[k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
    }
  }
}

}  // namespace

int launch_hue(const EnhanceRowDev* rows, const HueRecDev* recs, int nrecs, int nunits, void* stream) {
  if (nrecs <= 0 || nunits <= 0) return 0;
  hipLaunchKernelGGL(hue_rows, dim3(nunits), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const void*>(rows), static_cast<const void*>(recs), nrecs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
