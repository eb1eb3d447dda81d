// pil_resize.hip -- Pillow's 8-bit resize (Resample.c ImagingResampleHorizontal_8bpc
// then ImagingResampleVertical_8bpc) + crop (+ hflip) (+ u8 -> f32 / 255) for
// gfx950: the kernel of mxd_filter 16..18.
//
// Pillow's arithmetic is not the float kernels': 8.22 fixed-point coefficients
// (taps.cpp pil_axis_taps), int32 sums from 2^21, an arithmetic shift by 22 and
// a clamp to a byte -- once after the horizontal pass and once after the
// vertical pass, which runs on the horizontal pass's bytes.  The clamp between
// the passes is observable (bicubic and Lanczos lobes overshoot), so the
// kernel keeps Pillow's order: horizontal first.
//
// Work decomposition: one 256-lane workgroup per tile = (image, kPilTY output
// rows, kPilTX output columns), tiles numbered through ImgDev::tile_begin.  The
// tile's horizontal tap entries are staged in LDS once.  Its source rows
// first_y[tile's first row] .. last_y[tile's last row] then stream through the
// workgroup kPilG at a time:
//   load    the bytes of the kPilG rows that the tile's columns touch, global ->
//           LDS, as dwords where the row stride allows it (a dword is loaded
//           whole only when every byte of it lies in the footprint; the ragged
//           ends and unaligned strides go byte by byte), so no byte outside the
//           footprint -- past src_stride, or outside a staged region -- is read;
//   H pass  one lane per (row of the group, output column): count_x taps from
//           the LDS bytes into C int32 sums by 24-bit multiply-adds (a byte
//           times a coefficient below 2^23), rounded, shifted, clamped and
//           written as bytes into an LDS ring of H-resampled rows;
//   V pass  every output row whose last tap row the ring now holds: one wave per
//           ready row (its tap entry is wave-uniform, read by scalar loads), one
//           lane per 4 output bytes, count_y taps down the ring, rounded,
//           shifted, clamped, stored as a dword (u8) or four floats (q / 255).
// The ring holds max count_y + kPilG rows: an output row is emitted at most
// kPilG - 1 rows after its last tap row arrives, so its first is still there.
// The horizontal flip is applied where the tap entries are staged (output
// column ox takes the entry of crop_w - 1 - ox): mirrored interleaved pixels
// are not mirrored dwords, so a flip at the store would cost the dword stores.
// Matrix instructions do not fit: a product is u8 x signed 23 bits and must be
// exact in int32, which no MFMA input type holds.
#include <hip/hip_runtime.h>

#include "pil_resize.h"

namespace mxd {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
static_assert(kPilG * kPilTX == kThreads, "H pass: one lane per (row of the group, output column)");
static_assert((kPilTX * 3) / 4 <= kWave && kPilTX % 4 == 0, "V pass: one wave covers a ring row in dwords");

// Exact f32 q/255.0f for q in 0..255 (resample.hip's, checked for all 256 values).
__device__ __forceinline__ float div255(float q) {
  const float inv = 1.0f / 255.0f;
  const float r = q * inv;
  const float e = __builtin_fmaf(-r, 255.0f, q);
  return __builtin_fmaf(e, inv, r);
}

// Pillow's clip8 of a sum that started from 2^21.
__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> kPilPrecisionShift, 0), 255); }

template <int C, bool F32>
__global__ __launch_bounds__(kThreads) void pil_resize_rows(const ImgDev* __restrict__ imgs, int nimgs, int xs, int seg,
                                                            int ring_rows) {
  extern __shared__ __attribute__((aligned(16))) int32_t smem[];
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {  // image owning tile t
    const int mid = (lo + hi + 1) >> 1;
    if (imgs[mid].tile_begin <= t) lo = mid; else hi = mid - 1;
  }
  const ImgDev im = imgs[lo];
  const int local = t - im.tile_begin;
  const int band = local / im.nstrips;
  const int strip = local - band * im.nstrips;
  const int oy0 = band * kPilTY, oy1 = min(oy0 + kPilTY, im.crop_h);
  const int ox0 = strip * kPilTX, ox1 = min(ox0 + kPilTX, im.crop_w);
  const int tw = ox1 - ox0;
  const int xstride = kTapHeader + im.xwidth, ystride = kTapHeader + im.ywidth;
  const int32_t* __restrict__ xtab = reinterpret_cast<const int32_t*>(im.xtab);
  const int32_t* __restrict__ ytab = reinterpret_cast<const int32_t*>(im.ytab);

  // The tile's source footprint: first and last are monotone in the output index.
  const int xa = im.flip ? im.crop_w - ox1 : ox0;
  const int xb = im.flip ? im.crop_w - 1 - ox0 : ox1 - 1;
  const int px_lo = xtab[(size_t)xa * xstride];
  const int px_hi = xtab[(size_t)xb * xstride] + xtab[(size_t)xb * xstride + 1] - 1;
  const int y_lo = ytab[(size_t)oy0 * ystride];
  const int y_hi = ytab[(size_t)(oy1 - 1) * ystride] + ytab[(size_t)(oy1 - 1) * ystride + 1] - 1;
  const int nbytes = (px_hi - px_lo + 1) * C;
  const int64_t sstride = im.src_stride;
  const uint8_t* __restrict__ seg0 = im.src + (int64_t)px_lo * C;  // the footprint's first byte in row 0
  // Dword loads need every row's footprint at one phase m of a dword: a row
  // stride that is a multiple of 4.  LDS byte m + b of a row is footprint byte b.
  const bool dwords = (sstride & 3) == 0;
  const int m = dwords ? (int)(reinterpret_cast<uintptr_t>(seg0) & 3) : 0;
  const int ndw = (m + nbytes + 3) >> 2;

  int32_t* __restrict__ xinf = smem;                                   // [kPilTX][xs]
  uint32_t* __restrict__ srcw = reinterpret_cast<uint32_t*>(smem + kPilTX * xs);  // [kPilG][seg / 4]
  const uint8_t* __restrict__ srcb = reinterpret_cast<const uint8_t*>(srcw);
  uint8_t* __restrict__ ring = reinterpret_cast<uint8_t*>(srcw) + kPilG * seg;  // [ring_rows][pitch]
  constexpr int kPitch = pil_ring_pitch(C);
  const uint32_t* __restrict__ ringw = reinterpret_cast<const uint32_t*>(ring);

  // Stage the tile's horizontal entries: word 0 becomes the LDS byte of
  // (first tap, channel 0), then the count and the coefficients (xs is the
  // launch's widest entry: nothing is read past this image's own).
  for (int i = tid; i < tw * xs; i += kThreads) {
    const int xl = i / xs, k = i - xl * xs;
    const int ox = ox0 + xl;
    const int x = im.flip ? im.crop_w - 1 - ox : ox;
    const int32_t* e = xtab + (size_t)x * xstride;
    xinf[i] = k == 0 ? (e[0] - px_lo) * C + m : k < xstride ? e[k] : 0;
  }

  const int nout = tw * C;
  const int nq = (nout + 3) >> 2;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & (kWave - 1);
  int oy = oy0;  // the next output row to emit
  for (int y = y_lo; y <= y_hi; y += kPilG) {
    const int ng = min(kPilG, y_hi - y + 1);

    // ---- load: the footprint bytes of rows y .. y + ng - 1, global -> LDS ----
    for (int it = tid; it < ng * ndw; it += kThreads) {
      const int g = it / ndw, j = it - g * ndw;
      const uint8_t* rowp = seg0 - m + (int64_t)(y + g) * sstride;
      const int b0 = 4 * j;
      uint32_t v = 0;
      if (dwords && b0 >= m && b0 + 4 <= m + nbytes) {
        v = *reinterpret_cast<const uint32_t*>(rowp + b0);
      } else {
#pragma unroll
        for (int b = 0; b < 4; b++)
          if (b0 + b >= m && b0 + b < m + nbytes) v |= (uint32_t)rowp[b0 + b] << (8 * b);
      }
      srcw[g * (seg >> 2) + j] = v;
    }
    __syncthreads();  // (also: the V pass of the group before is done with the ring)

    // ---- H pass: LDS bytes -> bytes of the ring ----
    {
      const int g = tid >> 6, xl = tid & (kPilTX - 1);
      if (g < ng && xl < tw) {
        const int32_t* xi = xinf + xl * xs;
        const uint8_t* sr = srcb + g * seg + xi[0];
        const int cnt = xi[1];
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = 1 << (kPilPrecisionShift - 1);
        for (int k = 0; k < cnt; k++) {
          const int w = xi[kTapHeader + k];
#pragma unroll
          for (int c = 0; c < C; c++) acc[c] += __mul24((int)sr[k * C + c], w);
        }
        uint8_t* rr = ring + ((y + g - y_lo) % ring_rows) * kPitch + xl * C;
#pragma unroll
        for (int c = 0; c < C; c++) rr[c] = (uint8_t)clip8(acc[c]);
      }
    }
    __syncthreads();

    // ---- V pass: the output rows whose last tap row is in the ring now ----
    const int y_end = y + ng - 1;
    int nready = 0;
    while (oy + nready < oy1) {
      const int32_t* e = ytab + (size_t)(oy + nready) * ystride;
      if (e[0] + e[1] - 1 > y_end) break;
      nready++;
    }
    for (int r = wave; r < nready; r += kThreads / kWave) {
      const int row = oy + r;
      const int32_t* e = ytab + (size_t)row * ystride;
      const int first = e[0], cnt = e[1];
      if (lane >= nq) continue;
      int acc[4];
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = 1 << (kPilPrecisionShift - 1);
      int slot = (first - y_lo) % ring_rows;
      for (int k = 0; k < cnt; k++) {
        const int w = e[kTapHeader + k];
        const uint32_t q = ringw[slot * (kPitch >> 2) + lane];
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] += __mul24((int)((q >> (8 * j)) & 0xffu), w);
        slot = slot + 1 == ring_rows ? 0 : slot + 1;
      }
      int res[4];
#pragma unroll
      for (int j = 0; j < 4; j++) res[j] = clip8(acc[j]);
      const int64_t drow = (int64_t)row * im.dst_stride;
      const int o0 = ox0 * C + 4 * lane;
      const bool full = 4 * lane + 4 <= nout;
      if constexpr (F32) {
        float* d = reinterpret_cast<float*>(reinterpret_cast<char*>(im.dst) + drow) + o0;
        const float f[4] = {div255((float)res[0]), div255((float)res[1]), div255((float)res[2]), div255((float)res[3])};
        if (full && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
          *reinterpret_cast<float4*>(d) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
          for (int j = 0; j < 4 && 4 * lane + j < nout; j++) d[j] = f[j];
        }
      } else {
        uint8_t* d = reinterpret_cast<uint8_t*>(im.dst) + drow + o0;
        if (full && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
          *reinterpret_cast<uint32_t*>(d) =
              (uint32_t)res[0] | ((uint32_t)res[1] << 8) | ((uint32_t)res[2] << 16) | ((uint32_t)res[3] << 24);
        } else {
          for (int j = 0; j < 4 && 4 * lane + j < nout; j++) d[j] = (uint8_t)res[j];
        }
      }
    }
    oy += nready;
  }
}

template <int C, bool F32>
int launch_t(const PilCfg& cfg, const ImgDev* imgs, hipStream_t s) {
  hipLaunchKernelGGL((pil_resize_rows<C, F32>), dim3(cfg.ntiles), dim3(kThreads), pil_resize_smem_bytes(cfg), s, imgs,
                     cfg.nimgs, kTapHeader + cfg.max_xw, cfg.seg_bytes, cfg.max_yw + kPilG);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

int pil_resize_smem_bytes(const PilCfg& cfg) {
  return kPilTX * (kTapHeader + cfg.max_xw) * 4 + kPilG * cfg.seg_bytes + (cfg.max_yw + kPilG) * pil_ring_pitch(cfg.channels);
}

int launch_pil_resize(const PilCfg& cfg, const ImgDev* imgs, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (cfg.ntiles <= 0 || (cfg.seg_bytes & 3) != 0) return -2;
  switch (cfg.channels * 2 + (cfg.f32 ? 1 : 0)) {
    case 2: return launch_t<1, false>(cfg, imgs, s);
    case 3: return launch_t<1, true>(cfg, imgs, s);
    case 6: return launch_t<3, false>(cfg, imgs, s);
    case 7: return launch_t<3, true>(cfg, imgs, s);
    default: return -2;
  }
}

}  // namespace mxd
