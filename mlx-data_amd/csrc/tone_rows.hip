// tone_rows.hip -- the second pass of a tone call (mxd_tone): per-image
// statistics of the u8 RGB scratch rows, a 3 x 256 byte table per image, and
// the rows looked up, mapped through the colour matrix (when the call has
// one) and written in the call's output form.  Three kernels, ordered by the
// stream alone; none waits on another workgroup.
//
// tone_hist   a workgroup takes kToneHistRows rows of one image whose op needs
//             statistics, counts its bytes into LDS histograms with LDS
//             atomics (q0, q1, q2, and the luma byte for MXD_TONE_CONTRAST) and
//             adds the non-zero bins to the image's block of the workspace with
//             global atomics.
// tone_lut    one workgroup of 256 lanes per image: lane v builds t[c][v].
// tone_rows   color_rows.hip's structure: a lane owns four adjacent pixels
//             (three dwords), the image's table sits in LDS beside the format
//             table, stores are as wide as the destination's alignment allows.
//
// Arithmetic (the CPU statement is tone.cpp's): Pillow's
// -- truncation, not the project's +0.5 encode.  Every float and double
// operation is correctly rounded and none is fused: this file is compiled
// with -ffp-contract=off and says so again below.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "resample.h"

#pragma clang fp contract(off)

namespace mxd {
namespace {

constexpr int kThreads = 256;
// tone_hist merges the equal adjacent values of a lane's four pixels before
// the LDS atomics (measured against one atomic per byte: DESIGN.md section 5i)
constexpr bool kLaneMerge = true;
// mxd_tone_op (include/mxd_amd.h)
constexpr int kPosterize = 1, kSolarize = 2, kAutocontrast = 3, kEqualize = 4, kContrast = 5;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4a8 __attribute__((aligned(8)));

using ToneRowK = const __attribute__((address_space(4))) ToneRowDev;

template <class T>
__device__ __forceinline__ void nt(char* p, T v) {
  __builtin_nontemporal_store(v, MXD_GLOBAL_PTR(T, p));
}

// The twelve source bytes of a lane's four pixels (npx of them exist).
__device__ __forceinline__ void load_px(const uint8_t* s, int npx, uint32_t (&in)[3]) {
  in[0] = in[1] = in[2] = 0;
  if (npx == 4) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
    in[0] = s4[0], in[1] = s4[1], in[2] = s4[2];
  } else {
#pragma unroll
    for (int k = 0; k < 9; k++)
      if (k < 3 * npx) in[k >> 2] |= (uint32_t)s[k] << (8 * (k & 3));
  }
}

__global__ __launch_bounds__(kThreads) void tone_hist(const ToneRowDev* __restrict__ rows, int nimgs, uint8_t* ws) {
  __shared__ uint32_t h[kToneStatWords];
  const int blk = blockIdx.x;
  ToneRowK* rk = (ToneRowK*)rows;
  // the last image whose hist_begin <= blk: images without workgroups carry the next image's
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rk[mid].hist_begin <= blk) lo = mid; else hi = mid - 1;
  }
  ToneRowK& im = rk[lo];
  if (im.stat_off < 0) return;  // (uniform; the host gives such an image no workgroup)
  const bool luma = im.op == kContrast;
  const int nbins = luma ? 4 * 256 : 3 * 256;
  for (int i = threadIdx.x; i < nbins; i += kThreads) h[i] = 0;
  __syncthreads();
  const int w = im.crop_w;
  const int y0 = (blk - im.hist_begin) * kToneHistRows;
  const int nrows = min(kToneHistRows, im.crop_h - y0);
  const int nq = (w + 3) >> 2;
  const int64_t sstride = im.src_stride;
  const uint8_t* const sbase = im.src + (int64_t)y0 * sstride;
  for (int it = threadIdx.x; it < nrows * nq; it += kThreads) {
    const int r = it / nq, qx = it - r * nq;
    const int npx = min(4, w - 4 * qx);
    uint32_t in[3];
    load_px(sbase + r * sstride + 12 * qx, npx, in);
    // a lane's equal neighbours go out as one add (flat areas: a quarter of the atomics)
    uint32_t q[4][4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int k = 3 * p + c;
        q[p][c] = (in[k >> 2] >> (8 * (k & 3))) & 0xffu;
      }
      q[p][3] = (19595u * q[p][0] + 38470u * q[p][1] + 7471u * q[p][2] + 32768u) >> 16;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (c == 3 && !luma) break;
      uint32_t run = 1;
#pragma unroll
      for (int p = 0; p < 4; p++) {
        if (p >= npx) break;
        if (kLaneMerge && p + 1 < npx && q[p + 1][c] == q[p][c]) {
          run++;
        } else {
          atomicAdd(&h[c * 256 + q[p][c]], run);
          run = 1;
        }
      }
    }
  }
  __syncthreads();
  uint32_t* stat = reinterpret_cast<uint32_t*>(ws + im.stat_off);
  for (int i = threadIdx.x; i < nbins; i += kThreads)
    if (h[i]) atomicAdd(stat + i, h[i]);
}

__global__ __launch_bounds__(kThreads) void tone_lut(const ToneRowDev* __restrict__ rows, uint8_t* ws) {
  // H_c, then for EQUALIZE its inclusive prefix sums (two buffers: the scan ping-pongs)
  __shared__ uint32_t cum[2][3 * 256];
  __shared__ unsigned long long nz[3][kThreads / 64];  // the non-empty bins of a channel, one mask per wave (gfx950: 64 lanes)
  __shared__ unsigned long long sum_s;
  ToneRowK& im = ((ToneRowK*)rows)[blockIdx.x];
  const int v = threadIdx.x;
  const int op = im.op;
  uint8_t* const lut = ws + im.lut_off;
  const uint32_t* stat = im.stat_off >= 0 ? reinterpret_cast<const uint32_t*>(ws + im.stat_off) : nullptr;
  uint8_t t[3] = {(uint8_t)v, (uint8_t)v, (uint8_t)v};
  if (op == kPosterize) {
    t[0] = t[1] = t[2] = (uint8_t)(v & ((0xff << (8 - im.arg)) & 0xff));
  } else if (op == kSolarize) {
    t[0] = t[1] = t[2] = (uint8_t)(v < im.arg ? v : 255 - v);
  } else if (op == kAutocontrast || op == kEqualize) {
#pragma unroll
    for (int c = 0; c < 3; c++) cum[0][c * 256 + v] = stat[c * 256 + v];
    __syncthreads();
    uint32_t own[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      own[c] = cum[0][c * 256 + v];
      const unsigned long long mask = __ballot(own[c] != 0);
      if ((v & 63) == 0) nz[c][v >> 6] = mask;
    }
    __syncthreads();
    // smallest / largest non-empty bin and their number, per channel
    int lo_s[3], hi_s[3], bins_s[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      lo_s[c] = 256, hi_s[c] = -1, bins_s[c] = 0;
#pragma unroll
      for (int k = 0; k < kThreads / 64; k++) {
        const unsigned long long mask = nz[c][k];
        if (!mask) continue;
        if (lo_s[c] == 256) lo_s[c] = 64 * k + __ffsll(mask) - 1;
        hi_s[c] = 64 * k + 63 - __clzll(mask);
        bins_s[c] += __popcll(mask);
      }
    }
    if (op == kAutocontrast) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int lo = lo_s[c], hi = hi_s[c];
        if (hi > lo) {
          const double scale = 255.0 / (double)(hi - lo);
          const double offset = (double)(-lo) * scale;
          const double prod = (double)v * scale;
          const double x = prod + offset;
          const int ix = (int)x;
          t[c] = (uint8_t)(ix < 0 ? 0 : ix > 255 ? 255 : ix);
        }
      }
    } else {
      // the three channels' inclusive prefix sums: eight doubling steps over 256 lanes
      uint32_t last[3];
#pragma unroll
      for (int c = 0; c < 3; c++) last[c] = hi_s[c] >= 0 ? cum[0][c * 256 + hi_s[c]] : 0;
      int cur = 0;
#pragma unroll
      for (int d = 1; d < 256; d <<= 1) {
#pragma unroll
        for (int c = 0; c < 3; c++)
          cum[cur ^ 1][c * 256 + v] = cum[cur][c * 256 + v] + (v >= d ? cum[cur][c * 256 + v - d] : 0u);
        cur ^= 1;
        __syncthreads();
      }
      const uint32_t npix = (uint32_t)im.crop_w * (uint32_t)im.crop_h;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const uint32_t step = (npix - last[c]) / 255u;
        if (bins_s[c] > 1 && step != 0) {
          const uint32_t e = (step / 2 + (cum[cur][c * 256 + v] - own[c])) / step;
          t[c] = (uint8_t)(e > 255u ? 255u : e);
        }
      }
    }
  } else if (op == kContrast) {
    if (v == 0) sum_s = 0;
    __syncthreads();
    const uint32_t nl = stat[768 + v];
    if (nl && v) atomicAdd(&sum_s, (unsigned long long)v * nl);
    __syncthreads();
    const double npix = (double)((int64_t)im.crop_w * im.crop_h);
    const double mean = (double)sum_s / npix;
    const int m = (int)(mean + 0.5);
    const float f = im.factor;
    const float d = (float)(v - m);
    const float fd = f * d;
    const float x = (float)m + fd;
    uint8_t b;
    if (f >= 0.0f && f <= 1.0f) b = (uint8_t)(int)x;
    else b = x <= 0.0f ? 0 : x >= 255.0f ? 255 : (uint8_t)(int)x;
    t[0] = t[1] = t[2] = b;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) lut[c * 256 + v] = t[c];
}

// The twelve looked-up bytes of four pixels -> their twelve new bytes
// (color_rows' arithmetic).
__device__ __forceinline__ void twist(const float (&m)[12], const uint32_t (&b)[12], uint32_t (&out)[12]) {
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float v = ((m[4 * c] * (float)b[3 * p] + m[4 * c + 1] * (float)b[3 * p + 1]) + m[4 * c + 2] * (float)b[3 * p + 2]) +
                      m[4 * c + 3];
      out[3 * p + c] = (uint32_t)dev::encode(v);
    }
}

// ES: bytes per output element (1: u8, no table); CHW: channel planes; MAT:
// the colour matrix is applied.
template <int ES, bool CHW, bool MAT>
__global__ __launch_bounds__(kThreads) void tone_rows(const ToneRowDev* __restrict__ rows, int nimgs, OutFmtDev fmt,
                                                      const uint8_t* __restrict__ ws) {
  __shared__ uint32_t tab[ES > 1 ? 3 * 256 : 1];
  __shared__ uint32_t lut4[kToneLutBytes / 4];
  const uint8_t* const lut = reinterpret_cast<const uint8_t*>(lut4);
  const int blk = blockIdx.x;
  ToneRowK* rk = (ToneRowK*)rows;
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rk[mid].blk_begin <= blk) lo = mid; else hi = mid - 1;
  }
  ToneRowK& im = rk[lo];
  float m[12];
  if constexpr (MAT) {
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = im.m[k];
  }
  const int w = im.crop_w, h = im.crop_h;
  // (tables lie at multiples of 256 bytes in the workspace)
  if (threadIdx.x < kToneLutBytes / 4) lut4[threadIdx.x] = reinterpret_cast<const uint32_t*>(ws + im.lut_off)[threadIdx.x];
  if constexpr (ES > 1) {
    for (int i = threadIdx.x; i < 3 * 256; i += kThreads)
      tab[i] = ES == 2 ? (uint32_t)static_cast<const uint16_t*>(fmt.table)[i] : static_cast<const uint32_t*>(fmt.table)[i];
  }
  __syncthreads();
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
    uint32_t in[3];
    load_px(sbase + r * sstride + 12 * qx, npx, in);
    uint32_t o[12];
    {
      uint32_t b[12];
#pragma unroll
      for (int k = 0; k < 12; k++) b[k] = lut[(k % 3) * 256 + ((in[k >> 2] >> (8 * (k & 3))) & 0xffu)];
      if constexpr (MAT) {
        twist(m, b, o);
      } else {
#pragma unroll
        for (int k = 0; k < 12; k++) o[k] = b[k];
      }
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

template <bool MAT>
void launch_rows(const ToneRowDev* rows, int nimgs, int nblocks, const OutFmtDev& fmt, const uint8_t* ws, hipStream_t s) {
  const dim3 grid(nblocks), block(kThreads);
  if (!fmt.table) hipLaunchKernelGGL((tone_rows<1, false, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
  else if (fmt.elem16 && fmt.chw) hipLaunchKernelGGL((tone_rows<2, true, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
  else if (fmt.elem16) hipLaunchKernelGGL((tone_rows<2, false, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
  else if (fmt.chw) hipLaunchKernelGGL((tone_rows<4, true, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
  else hipLaunchKernelGGL((tone_rows<4, false, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
}

}  // namespace

int launch_tone(const ToneRowDev* rows, int nimgs, int hist_blocks, int row_blocks, const OutFmtDev& fmt, uint8_t* ws,
                bool matrix, void* stream) {
  if (nimgs <= 0 || row_blocks <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hist_blocks > 0) hipLaunchKernelGGL(tone_hist, dim3(hist_blocks), dim3(kThreads), 0, s, rows, nimgs, ws);
  hipLaunchKernelGGL(tone_lut, dim3(nimgs), dim3(kThreads), 0, s, rows, ws);
  if (matrix) launch_rows<true>(rows, nimgs, row_blocks, fmt, ws, s);
  else launch_rows<false>(rows, nimgs, row_blocks, fmt, ws, s);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
