// row_stage.hip -- the row stage (resample.h): the second pass behind the
// resize launches of a formatted, colour or tone call.  u8 scratch rows ->
// the call's output form (u8, or the elements of an mxd_out_format table, HWC
// or CHW), through the per-image byte table of a tone call and the per-image
// 3 x 4 map of a colour call.  One launch covers every image of a call; none
// of the kernels waits on another workgroup.
//
// format_rows  a formatted call's band / general images, 1-4 channels: a
//              workgroup takes kFmtRows rows of one image and looks every
//              byte up in the format's table, so the elements equal the table
//              by construction -- the same values the wave kernels store
//              (wave_fmt.hip).
// tone_hist    a workgroup takes kToneHistRows rows of one image whose op needs
//              statistics, counts its bytes into LDS histograms with LDS
//              atomics (q0, q1, q2, and the luma byte for MXD_TONE_CONTRAST) and
//              adds the non-zero bins to the image's block of the workspace with
//              global atomics.
// tone_lut     one workgroup of 256 lanes per image: lane v builds t[c][v].
// pixel_rows   the colour and the tone call's rows.  A workgroup takes
//              kPixelRows rows of one image, reads the image's entry through a
//              uniform (scalar) address and copies the tables it needs (the
//              image's, the format's) into LDS once.  A lane owns four adjacent
//              pixels: 12 source bytes as three dwords (scratch rows start at
//              16-byte multiples of 256-byte aligned bases, so the lanes of a
//              wave read contiguous bytes), the 12 new bytes computed in
//              registers, then the widest nontemporal stores the destination's
//              alignment allows -- tested once per workgroup on the image's
//              base and strides, so the branch is uniform.  A row's last
//              w mod 4 pixels and misaligned destinations take element stores.
//
// Arithmetic.  The colour map: float32 operations, each
// correctly rounded, none fused, because its CPU statement (mxd_color_apply_u8)
// and NumPy round every product and sum.  The tone tables (the CPU statement
// is tone.cpp's): Pillow's -- truncation, not the project's +0.5 encode; every
// float and double operation correctly rounded and none fused.  So this file
// is compiled with -ffp-contract=off and says so again below.
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

using ColorRowK = const __attribute__((address_space(4))) ColorRowDev;
using ToneRowK = const __attribute__((address_space(4))) ToneRowDev;
__device__ __forceinline__ ColorRowK& color_of(ColorRowK& e) { return e; }
__device__ __forceinline__ ColorRowK& color_of(ToneRowK& e) { return e.color; }

template <class T>
__device__ __forceinline__ void nt(char* p, T v) {
  __builtin_nontemporal_store(v, MXD_GLOBAL_PTR(T, p));
}

// The image of workgroup blk: the last of nimgs whose first workgroup,
// begin(i), is <= blk (an image without workgroups carries the next image's).
template <class Begin>
__device__ __forceinline__ int image_of_block(int nimgs, int blk, Begin begin) {
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begin(mid) <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The first n elements of the format's table into LDS, a dword each (the
// caller's barrier follows).
__device__ __forceinline__ void stage_table(const OutFmtDev& fmt, bool elem16, int n, uint32_t* tab) {
  for (int i = threadIdx.x; i < n; i += kThreads)
    tab[i] = elem16 ? (uint32_t)static_cast<const uint16_t*>(fmt.table)[i] : static_cast<const uint32_t*>(fmt.table)[i];
}

// The twelve source bytes of a lane's four pixels (npx of them exist) into
// `in`, which the caller zeroed.
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

// The twelve bytes of four pixels -> their twelve new bytes.
__device__ __forceinline__ void twist(const float (&m)[12], const uint32_t (&b)[12], uint32_t (&out)[12]) {
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float q0 = (float)b[3 * p], q1 = (float)b[3 * p + 1], q2 = (float)b[3 * p + 2];
      const float v = ((m[4 * c] * q0 + m[4 * c + 1] * q1) + m[4 * c + 2] * q2) + m[4 * c + 3];
      out[3 * p + c] = (uint32_t)dev::encode(v);
    }
}

__global__ __launch_bounds__(kThreads) void format_rows(const FmtRowDev* __restrict__ rows, int nimgs, OutFmtDev fmt) {
  __shared__ uint32_t tab[4 * 256];
  const int blk = blockIdx.x;
  const FmtRowDev& im = rows[image_of_block(nimgs, blk, [&](int i) { return rows[i].blk_begin; })];
  const int c = im.channels, w = im.crop_w, h = im.crop_h;
  const int e16 = fmt.elem16, chw = fmt.chw;
  stage_table(fmt, e16, c * 256, tab);
  __syncthreads();
  const int y0 = (blk - im.blk_begin) * kFmtRows;
  const int y1 = min(y0 + kFmtRows, h);
  const int n = w * c;
  for (int y = y0; y < y1; y++) {
    const uint8_t* s = im.src + (int64_t)y * im.src_stride;
    char* d = static_cast<char*>(im.dst) + (int64_t)y * im.dst_stride;
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const int x = i / c, ch = i - x * c;
      const uint32_t v = tab[ch * 256 + s[i]];
      // element index in the row (CHW: in the row of plane ch)
      char* p = chw ? d + ch * fmt.plane_stride : d;
      const int e = chw ? x : i;
      if (e16) __builtin_nontemporal_store((uint16_t)v, MXD_GLOBAL_PTR(uint16_t, p) + e);
      else __builtin_nontemporal_store(v, MXD_GLOBAL_PTR(uint32_t, p) + e);
    }
  }
}

__global__ __launch_bounds__(kThreads) void tone_hist(const ToneRowDev* __restrict__ rows, int nimgs, uint8_t* ws) {
  __shared__ uint32_t h[kToneStatWords];
  const int blk = blockIdx.x;
  ToneRowK* rk = (ToneRowK*)rows;
  ToneRowK& im = rk[image_of_block(nimgs, blk, [&](int i) { return rk[i].hist_begin; })];
  if (im.stat_off < 0) return;  // (uniform; the host gives such an image no workgroup)
  const bool luma = im.op == kContrast;
  const int nbins = luma ? 4 * 256 : 3 * 256;
  for (int i = threadIdx.x; i < nbins; i += kThreads) h[i] = 0;
  __syncthreads();
  const int w = im.color.head.crop_w;
  const int y0 = (blk - im.hist_begin) * kToneHistRows;
  const int nrows = min(kToneHistRows, im.color.head.crop_h - y0);
  const int nq = (w + 3) >> 2;
  const int64_t sstride = im.color.head.src_stride;
  const uint8_t* const sbase = im.color.head.src + (int64_t)y0 * sstride;
  for (int it = threadIdx.x; it < nrows * nq; it += kThreads) {
    const int r = it / nq, qx = it - r * nq;
    const int npx = min(4, w - 4 * qx);
    uint32_t in[3] = {0, 0, 0};
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
  const int crop_w = im.color.head.crop_w, crop_h = im.color.head.crop_h;
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
      const uint32_t npix = (uint32_t)crop_w * (uint32_t)crop_h;
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
    const double npix = (double)((int64_t)crop_w * crop_h);
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

// ES: bytes per output element (1: u8, no format table); CHW: channel planes;
// TAB: a tone call (ToneRowDev entries; every byte goes through the image's
// table in the workspace ws), else a colour call (ColorRowDev entries); MAT:
// the entries' matrices are applied.
template <int ES, bool CHW, bool TAB, bool MAT>
__global__ __launch_bounds__(kThreads) void pixel_rows(const void* __restrict__ rows, int nimgs, OutFmtDev fmt,
                                                       const uint8_t* __restrict__ ws) {
  using EntryK = typename std::conditional<TAB, ToneRowK, ColorRowK>::type;
  __shared__ uint32_t tab[ES > 1 ? 3 * 256 : 1];
  __shared__ uint32_t lut4[TAB ? kToneLutBytes / 4 : 1];
  const uint8_t* const lut = reinterpret_cast<const uint8_t*>(lut4);
  const int blk = blockIdx.x;
  EntryK* rk = (EntryK*)rows;
  EntryK& entry = rk[image_of_block(nimgs, blk, [&](int i) { return color_of(rk[i]).head.blk_begin; })];
  ColorRowK& im = color_of(entry);
  float m[12];
  if constexpr (MAT) {
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = im.m[k];
  }
  const int w = im.head.crop_w, h = im.head.crop_h;
  if constexpr (TAB) {
    // (tables lie at multiples of 256 bytes in the workspace)
    if (threadIdx.x < kToneLutBytes / 4) lut4[threadIdx.x] = reinterpret_cast<const uint32_t*>(ws + entry.lut_off)[threadIdx.x];
  }
  if constexpr (ES > 1) stage_table(fmt, ES == 2, 3 * 256, tab);
  if constexpr (TAB || ES > 1) __syncthreads();
  const int y0 = (blk - im.head.blk_begin) * kPixelRows;
  const int nrows = min(kPixelRows, h - y0);
  const int nq = (w + 3) >> 2;  // lanes per row
  const int64_t sstride = im.head.src_stride, dstride = im.head.dst_stride;
  const uint8_t* const sbase = im.head.src + (int64_t)y0 * sstride;
  char* const dbase = static_cast<char*>(im.head.dst) + (int64_t)y0 * dstride;
  // widest store of a lane: 4 bytes (u8), 16 (f32), 8 (16-bit elements)
  constexpr int kAlign = ES == 1 ? 4 : ES == 4 ? 16 : 8;
  const uint64_t bits = reinterpret_cast<uint64_t>(im.head.dst) | (uint64_t)dstride | (CHW ? (uint64_t)fmt.plane_stride : 0);
  const bool wide = (bits & (kAlign - 1)) == 0;
  for (int it = threadIdx.x; it < nrows * nq; it += kThreads) {
    const int r = it / nq, qx = it - r * nq;
    const int npx = min(4, w - 4 * qx);
    uint32_t in[3] = {0, 0, 0};
    load_px(sbase + r * sstride + 12 * qx, npx, in);
    uint32_t o[12];
    {
      uint32_t b[12];
#pragma unroll
      for (int k = 0; k < 12; k++) {
        b[k] = (in[k >> 2] >> (8 * (k & 3))) & 0xffu;
        if constexpr (TAB) b[k] = lut[(k % 3) * 256 + b[k]];
      }
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

// The instantiation of the call's output form.
template <bool TAB, bool MAT>
void launch_pixel_rows(const void* rows, int nimgs, int nblocks, const OutFmtDev& fmt, const uint8_t* ws, hipStream_t s) {
  const dim3 grid(nblocks), block(kThreads);
  if (!fmt.table) hipLaunchKernelGGL((pixel_rows<1, false, TAB, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
  else if (fmt.elem16 && fmt.chw) hipLaunchKernelGGL((pixel_rows<2, true, TAB, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
  else if (fmt.elem16) hipLaunchKernelGGL((pixel_rows<2, false, TAB, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
  else if (fmt.chw) hipLaunchKernelGGL((pixel_rows<4, true, TAB, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
  else hipLaunchKernelGGL((pixel_rows<4, false, TAB, MAT>), grid, block, 0, s, rows, nimgs, fmt, ws);
}

}  // namespace

int launch_format_rows(const FmtRowDev* rows, int nimgs, int nblocks, const OutFmtDev& fmt, void* stream) {
  if (nimgs <= 0 || nblocks <= 0) return 0;
  hipLaunchKernelGGL(format_rows, dim3(nblocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), rows, nimgs,
                     fmt);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_color_rows(const ColorRowDev* rows, int nimgs, int nblocks, const OutFmtDev& fmt, void* stream) {
  if (nimgs <= 0 || nblocks <= 0) return 0;
  launch_pixel_rows<false, true>(rows, nimgs, nblocks, fmt, nullptr, reinterpret_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_tone(const ToneRowDev* rows, int nimgs, int hist_blocks, int row_blocks, const OutFmtDev& fmt, uint8_t* ws,
                bool matrix, void* stream) {
  if (nimgs <= 0 || row_blocks <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hist_blocks > 0) hipLaunchKernelGGL(tone_hist, dim3(hist_blocks), dim3(kThreads), 0, s, rows, nimgs, ws);
  hipLaunchKernelGGL(tone_lut, dim3(nimgs), dim3(kThreads), 0, s, rows, ws);
  if (matrix) launch_pixel_rows<true, true>(rows, nimgs, row_blocks, fmt, ws, s);
  else launch_pixel_rows<true, false>(rows, nimgs, row_blocks, fmt, ws, s);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
