// pilblur.hip -- Pillow's ImageFilter.GaussianBlur / BoxBlur of the enhance
// stage (resample.h): the images of an enhance call whose op is
// MXD_ENHANCE_PIL_GAUSSIAN_BLUR or MXD_ENHANCE_PIL_BOX_BLUR.  pilblur_rows runs
// in the enhance stage's slot of the chain, behind enhance_rows and blur_rows
// on the same stream, reads and writes the rows that stage does (the images'
// own EnhanceRowDev entries) and takes the images neither of the two has a
// unit for.  One launch covers every such image of a call; no workgroup waits
// on another.
//
// The blur is P = 3 (Gaussian) or 1 (box) passes of an extended box filter
// along the rows, then P along the columns, each pass on the bytes the one
// before it wrote: out = (ww * box + fw * (the two pixels beyond the box)
// + 2^23) >> 24 with the box 2R + 1 pixels wide and every index clamped at the
// image's edge (mxd_amd.h).  A pass reaches rho = R + 1
// pixels.  The arithmetic is uint32, so every summation order gives the same
// bits: the horizontal box is a difference of two prefix sums and the vertical
// one a running sum, and a pixel costs the same at every radius.
//
// pilblur_rows  a row-streaming column strip.  A workgroup of 256 lanes (four
//               waves of 64) owns a strip of kBlurStripW = 64 output pixels
//               (192 channel columns) times a segment of seg_rows output rows
//               y0..y1-1 of one image, and walks down the source rows
//               y0 - P rho .. y1 - 1 + P rho clipped to the image, kStep = 4
//               rows a step, one row a wave:
//
//               stage  the step's rows of 64 + 2 P rho pixels, clipped to the
//                      image (never padded: every pass clamps its own indices
//                      at the image's edge, none at the strip's), go from the
//                      scratch rows into LDS as the aligned dwords that cover
//                      their bytes (the bytes then start `shift` = 0..3 bytes
//                      into the staged row).  A lane's dwords are the same
//                      columns in every step; the loads of step t + 1 are
//                      issued into registers before the passes of step t.
//                      Every address is clamped into the image's own
//                      stride x h bytes, enhance_rows' rule.
//               H      wave v takes staged row v; lane l takes its pixels
//                      3l..3l+2, nine channel columns held in registers through
//                      all P passes.  A pass: the lane sums its three pixels per
//                      channel, a wave-level inclusive scan (shuffles) turns
//                      the lane sums into offsets, and the lane writes its nine
//                      prefix sums to the wave's LDS prefix row; then every
//                      output is read back as differences of that row -- the
//                      box from two prefixes 2R + 1 apart, each pixel beyond it
//                      from two adjacent ones -- with an index below the
//                      image's first pixel or above its last replaced by that
//                      pixel times its count.  Every lane computes every pass;
//                      what a pass computes more than rho pixels inside the
//                      staged span's cut ends is wrong and is never read by a
//                      valid pixel of the next pass (the valid span shrinks by
//                      rho a side and a pass, except at the image's edge), and
//                      in modular uint32 it cancels out of the differences.
//                      The last pass writes the strip's 192 columns as a byte
//                      row into the first V ring.
//               V      a cascade of P stages, lane c < 192 owning channel
//                      column c in all of them: the column's bytes never cross
//                      lanes, so the cascade needs no barrier.  Stage j keeps
//                      its input rows in an LDS ring of byte rows (2R + 3 rows
//                      are live; kRing = 40 leaves room for a step's rows) and
//                      the box of its next output row as one uint32 running sum
//                      in a register: per output row, add the entering row,
//                      subtract the leaving one, ww * sum + fw * (the two rows
//                      beyond), round, and hand the byte to stage j + 1's ring.
//                      An output row is due when input row min(y + rho, h - 1)
//                      has arrived, so the image's last row releases several;
//                      row indices clamp at the image's top and bottom per
//                      stage, and the first output row of a segment builds its
//                      sum directly.  The last stage gathers four bytes from
//                      four lanes into a dword and stores the dword where the
//                      destination base and stride are 4-byte aligned; row
//                      tails and misaligned destinations take element stores
//                      (blur_rows' rule).
//
//               R, ww, fw and P are uniform per workgroup: the image's record
//               is read through a uniform (scalar) address and every loop has a
//               uniform trip count; no lane leaves the walk early.  The only
//               redundant work is the P rho warm-up rows (and columns) at both
//               ends of a segment (strip).
//
// Matrix instructions do not fit this kernel: a box of equal weights is a
// difference of running sums, two additions a pixel, where an MFMA would spend
// a (2R + 1)-wide product on it; and every pass ends in a shift and a byte
// rounding that the next pass reads, so the passes cannot be merged into one
// product either.  The accumulation order is free (integers); the byte
// rounding after every pass is not.  The CPU statement is enhance.cpp's; the
// two share no code.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "resample.h"

namespace mxd {
namespace {

constexpr int kThreads = 256;
constexpr int kStep = 4;                                 // source rows a step: one a wave
constexpr int kCols = kBlurStripW * 3;                   // channel columns of a strip
constexpr int kMaxP = 3;                                 // passes per axis
constexpr int kMaxPix = kBlurStripW + 2 * kMaxP * kBlurMaxR;  // pixels of a staged row: 160
constexpr int kLanePix = 3;                              // pixels a lane holds in the H passes
constexpr int kStageWords = (kMaxPix * 3 + 3 + 3) / 4;   // a staged row: its bytes behind a shift of up to 3
constexpr int kStageItems = (kStep * kStageWords + kThreads - 1) / kThreads;
constexpr int kPreWords = (1 + 64 * kLanePix) * 3;       // a prefix row: a zero pixel, then every lane's three
constexpr int kRing = 40;                                // byte rows of a V ring: >= 2 (kBlurMaxR - 1) + 3 + kStep - 1
static_assert(64 * kLanePix >= kMaxPix, "a wave holds a staged row");
static_assert(kThreads / 64 == kStep, "one staged row a wave");
static_assert(kRing >= 2 * (kBlurMaxR - 1) + 3 + kStep - 1, "the ring holds a stage's live rows and a step's new ones");
static_assert(kCols % 4 == 0 && kCols % 64 == 0, "a dword's four lanes share a wave; a strip starts at a dword");

using EnhRowK = const __attribute__((address_space(4))) EnhanceRowDev;
using PilRecK = const __attribute__((address_space(4))) PilBlurRecDev;

// What is uniform in a workgroup and the V cascade's state.
struct Walk {
  int h, R, rho, P, r0;
  uint32_t ww, fw;
  int olo[kMaxP], ohi[kMaxP];  // the output rows stage j owes: [olo, ohi)
  int yo[kMaxP];               // its next one
  uint32_t acc[kMaxP];         // the box sum of output row yo - 1 (this lane's column)
  // the last stage's stores
  uint8_t* dst;
  int64_t dstride;
  int ncols;
  bool wide;
};

__device__ __forceinline__ int ring_at(const Walk& k, int row, int col) {
  const int y = min(max(row, 0), k.h - 1);
  return ((y - k.r0) % kRing) * kCols + col;
}

// Input row yi of stage J has arrived in ring J (column `col` of it, for this
// lane): emit the output rows that are due.
template <int J>
__device__ __forceinline__ void advance(Walk& k, uint8_t (*rings)[kRing * kCols], int col, int yi) {
  uint8_t* const in = rings[J];
  while (k.yo[J] < k.ohi[J] && min(k.yo[J] + k.rho, k.h - 1) <= yi) {
    const int y = k.yo[J];
    const uint32_t below = in[ring_at(k, y - k.rho, col)], above = in[ring_at(k, y + k.rho, col)];
    if (y == k.olo[J]) {
      uint32_t a = 0;
      for (int d = -k.R; d <= k.R; d++) a += in[ring_at(k, y + d, col)];
      k.acc[J] = a;
    } else {
      k.acc[J] += (uint32_t)in[ring_at(k, y + k.R, col)] - below;  // (below is also the row that leaves)
    }
    const uint32_t v = (k.ww * k.acc[J] + k.fw * (below + above) + (1u << 23)) >> 24;
    k.yo[J] = y + 1;
    bool last = true;
    if constexpr (J + 1 < kMaxP) {
      if (J + 1 < k.P) {
        last = false;
        rings[J + 1][ring_at(k, y, col)] = (uint8_t)v;
        advance<J + 1>(k, rings, col, y);
      }
    }
    if (last) {
      // four lanes' bytes to the lane of the dword's first column
      const uint32_t out = v | (uint32_t)__shfl_down((int)v, 1) << 8 | (uint32_t)__shfl_down((int)v, 2) << 16 |
                           (uint32_t)__shfl_down((int)v, 3) << 24;
      if ((col & 3) == 0 && col < k.ncols) {
        uint8_t* const d = k.dst + (int64_t)y * k.dstride + col;
        if (k.wide && col + 4 <= k.ncols) {
          *reinterpret_cast<uint32_t*>(d) = out;
        } else {
#pragma unroll
          for (int b = 0; b < 4; b++)
            if (col + b < k.ncols) d[b] = (uint8_t)(out >> (8 * b));
        }
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void pilblur_rows(const void* __restrict__ rows, const void* __restrict__ recs,
                                                         int nrecs) {
  __shared__ uint32_t stage[kStep * kStageWords];
  __shared__ uint32_t pre[kStep][kPreWords];
  __shared__ __attribute__((aligned(4))) uint8_t rings[kMaxP][kRing * kCols];

  PilRecK* bk = (PilRecK*)recs;
  const int blk = blockIdx.x;
  int lo = 0, hi = nrecs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bk[mid].unit_begin <= blk) lo = mid; else hi = mid - 1;
  }
  PilRecK& rec = bk[lo];
  EnhRowK& e = ((EnhRowK*)rows)[rec.entry];
  const int w = e.w, h = e.h;
  const int R = min(max(rec.R, 0), kBlurMaxR - 1), rho = R + 1;
  const int P = rec.passes == 1 ? 1 : kMaxP;
  const uint32_t ww = rec.ww, fw = rec.fw;
  const int unit = blk - rec.unit_begin;
  const int seg = unit / rec.strips, strip = unit - seg * rec.strips;
  const int x0 = strip * kBlurStripW;
  const int y0 = seg * rec.seg_rows, y1 = min(y0 + rec.seg_rows, h);
  const uint8_t* const src = e.src;
  const int64_t sstride = e.src_stride;
  const int64_t limit = sstride * h;
  const int lane = (int)threadIdx.x;
  const int wv = lane >> 6, wl = lane & 63;

  // The staged row: image pixels sx0 .. sx1 - 1, n of them, `shift` bytes into the row.
  const int sx0 = max(0, x0 - P * rho), sx1 = min(w, x0 + kBlurStripW + P * rho);
  const int n = sx1 - sx0;
  const int shift = (sx0 * 3) & 3;
  const int nw = (shift + n * 3 + 3) >> 2;
  // The source rows of the walk: r0 .. r1 - 1.
  const int r0 = max(0, y0 - P * rho), r1 = min(h, y1 + P * rho);
  // The lane's staged dwords: the same columns in every step.
  int srow[kStageItems], scol[kStageItems];
#pragma unroll
  for (int j = 0; j < kStageItems; j++) {
    const int i = lane + kThreads * j;
    srow[j] = i / kStageWords;
    scol[j] = i - srow[j] * kStageWords;
    if (srow[j] >= kStep || scol[j] >= nw) srow[j] = -1;
  }
  uint32_t held[kStageItems];
  auto prefetch = [&](int lb) {  // the lane's dwords of the step whose first row is lb
#pragma unroll
    for (int j = 0; j < kStageItems; j++) {
      held[j] = 0;
      if (srow[j] < 0) continue;
      const int64_t o = (int64_t)min(lb + srow[j], h - 1) * sstride + (sx0 * 3 - shift + 4 * scol[j]);
      held[j] = *reinterpret_cast<const uint32_t*>(src + min(max(o, (int64_t)0), limit - 4));
    }
  };

  Walk k;
  k.h = h, k.R = R, k.rho = rho, k.P = P, k.r0 = r0, k.ww = ww, k.fw = fw;
#pragma unroll
  for (int j = 0; j < kMaxP; j++) {
    const int reach = max(P - 1 - j, 0) * rho;
    k.olo[j] = max(0, y0 - reach), k.ohi[j] = min(h, y1 + reach);
    k.yo[j] = k.olo[j];
    k.acc[j] = 0;
  }
  k.ncols = 3 * min(kBlurStripW, w - x0);  // the strip's columns inside the image
  k.dst = e.dst + 3 * (int64_t)x0;
  k.dstride = e.dst_stride;
  k.wide = ((reinterpret_cast<uint64_t>(e.dst) | (uint64_t)e.dst_stride) & 3) == 0;

  const uint8_t* const sbytes = reinterpret_cast<const uint8_t*>(stage) + wv * (kStageWords * 4) + shift;
  uint32_t* const mypre = pre[wv];
  if (wl < 3) mypre[wl] = 0;  // the zero pixel in front: the prefix below the staged row's first pixel
  // prefix(i, c): the sum of channel c over the staged pixels 0..i, i clamped to -1..n-1
  auto prefix = [&](int i, int c) { return mypre[3 * (1 + min(max(i, -1), n - 1)) + c]; };

  const int nsteps = (r1 - r0 + kStep - 1) / kStep;
  int lb = r0;  // the step's first row
  prefetch(lb);
  for (int t = 0; t < nsteps; t++) {
#pragma unroll
    for (int j = 0; j < kStageItems; j++)
      if (srow[j] >= 0) stage[srow[j] * kStageWords + scol[j]] = held[j];
    __syncthreads();
    if (t + 1 < nsteps) prefetch(lb + kStep);

    // H: wave wv's staged row through P passes, nine columns a lane in registers
    uint32_t px[kLanePix][3];
#pragma unroll
    for (int i = 0; i < kLanePix; i++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int q = kLanePix * wl + i;
        px[i][c] = q < n ? sbytes[3 * q + c] : 0;
      }
    for (int pass = 0; pass < P; pass++) {
      // the lane's inclusive prefixes, then the wave's
      uint32_t run[kLanePix][3], tot[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        run[0][c] = px[0][c];
#pragma unroll
        for (int i = 1; i < kLanePix; i++) run[i][c] = run[i - 1][c] + px[i][c];
        uint32_t s = run[kLanePix - 1][c];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t up = (uint32_t)__shfl_up((int)s, d);
          if (wl >= d) s += up;
        }
        tot[c] = s - run[kLanePix - 1][c];  // the lanes below
      }
#pragma unroll
      for (int i = 0; i < kLanePix; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) mypre[3 * (1 + kLanePix * wl + i) + c] = tot[c] + run[i][c];
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const uint32_t first = prefix(0, c), last = prefix(n - 1, c) - prefix(n - 2, c);
#pragma unroll
        for (int i = 0; i < kLanePix; i++) {
          const int q = kLanePix * wl + i;     // the staged pixel
          const int a = sx0 + q - R, b = sx0 + q + R;  // the box in image pixels
          const uint32_t under = (uint32_t)max(0, -a), over = (uint32_t)max(0, b - (w - 1));
          const uint32_t pa1 = prefix(q - R - 1, c), pb = prefix(q + R, c);
          const uint32_t box = pb - pa1 + under * first + over * last;
          const uint32_t below = a - 1 < 0 ? first : pa1 - prefix(q - R - 2, c);
          const uint32_t above = b + 1 > w - 1 ? last : prefix(q + R + 1, c) - pb;
          px[i][c] = ((ww * box + fw * (below + above) + (1u << 23)) >> 24) & 0xffu;
        }
      }
      __syncthreads();  // (the next pass, or the next step, overwrites the prefix row)
    }
    // the strip's columns of the row into the first ring
    {
      const int y = lb + wv;
      if (y < r1) {
        uint8_t* const out = rings[0] + ((y - r0) % kRing) * kCols;
#pragma unroll
        for (int i = 0; i < kLanePix; i++) {
          const int xs = sx0 + kLanePix * wl + i - x0;  // the pixel's place in the strip
          if (xs >= 0 && xs < kBlurStripW) {
#pragma unroll
            for (int c = 0; c < 3; c++) out[3 * xs + c] = (uint8_t)px[i][c];
          }
        }
      }
    }
    __syncthreads();

    // V: the step's rows enter the cascade in order
    if (lane < kCols) {
      for (int r = 0; r < kStep; r++)
        if (lb + r < r1) advance<0>(k, rings, lane, lb + r);
    }
    lb += kStep;
  }
}

}  // namespace

int launch_pilblur(const EnhanceRowDev* rows, const PilBlurRecDev* recs, int nrecs, int nunits, void* stream) {
  if (nrecs <= 0 || nunits <= 0) return 0;
  hipLaunchKernelGGL(pilblur_rows, dim3(nunits), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const void*>(rows), static_cast<const void*>(recs), nrecs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
