// blur.hip -- the Gaussian blur of the enhance stage (resample.h): the images
// of an enhance call whose op is MXD_ENHANCE_GAUSSIAN_BLUR.  blur_rows runs in
// the enhance stage's slot of the chain, behind enhance_rows on the same
// stream, reads and writes the rows that stage does (the images' own
// EnhanceRowDev entries) and takes the images enhance_rows has no tile for.
// One launch covers every blurred image of a call; no kernel waits on another
// workgroup.
//
// blur_rows<S>  a row-streaming column strip.  A workgroup of 256 lanes (four
//               waves of 64) owns a strip of kBlurStripW = 64 output pixels
//               (192 channel columns) times a segment of seg_rows output rows
//               y0..y1-1 of one image, and walks down the logical source rows
//               y0 - R .. y1 - 1 + R (reflected into the image), S rows a step:
//
//               stage  the step's S rows of 64 + 2R pixels go from the scratch
//                      rows into an LDS byte staging area.  An interior strip
//                      loads the aligned dwords that cover its bytes (the
//                      bytes then start `shift` = 0..3 bytes into the staged
//                      row); an edge strip gathers each staged dword from four
//                      reflected element addresses.  A lane's dwords are the
//                      same columns in every step, so their offsets into a row
//                      are computed once, and the loads of step t + 1 are
//                      issued into registers before the passes of step t.
//                      Every address is clamped into the image's own
//                      stride x h bytes, enhance_rows' rule.
//               H      lane i takes channel column i % 192 of staged row
//                      i / 192 (S * 192 / 256 items a lane, interleaved under
//                      one tap loop) and writes the float32 result into an LDS
//                      ring of float32 rows, 192 floats each.  The ring holds
//                      2 * 16 + S rows: the 2R + S a step's output rows read.
//               V      once the ring holds the window of an output row, lane
//                      i takes four adjacent columns (one ds_read_b128 a tap
//                      row: consecutive lanes read consecutive 16 bytes, no
//                      bank conflict) of output row i / 48, rounds, packs four
//                      bytes a dword and stores the dword where the
//                      destination base and stride are 4-byte aligned; row
//                      tails and misaligned destinations take element stores.
//
//               Two barriers a step (stage -> H, H -> V); no lane leaves the
//               walk early.  R and the weights are uniform per workgroup: the
//               image's record is read through a uniform (scalar) address and
//               the tap loops have a uniform trip count.  The only redundant
//               work is the 2R H-pass rows at the top and bottom of a segment.
//
// Matrix instructions do not fit this kernel: the accumulation order of both
// passes is part of the contract -- centre tap first,
// then the pairs d = 1..R, each product and each sum rounded to float32 -- and
// an MFMA's internal order and precision are not that.  For the same reason
// nothing is fused: this file is compiled with -ffp-contract=off and says so
// again below.  The CPU statement is enhance.cpp's; the two share no code.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "resample.h"

#pragma clang fp contract(off)

namespace mxd {
namespace {

constexpr int kThreads = 256;
constexpr int kCols = kBlurStripW * 3;                                   // channel columns of a strip
constexpr int kStageWords = ((kBlurStripW + 2 * kBlurMaxR) * 3 + 3 + 3) / 4;  // a staged row: its bytes behind a shift of up to 3
constexpr int kGroups = kCols / 4;                                       // V-pass lanes per output row
static_assert(kCols % 4 == 0, "a strip starts at a dword of the destination row");

using EnhRowK = const __attribute__((address_space(4))) EnhanceRowDev;
using BlurRecK = const __attribute__((address_space(4))) BlurRecDev;

// torch / NumPy "reflect" of i into 0..n-1: period 2 (n - 1), 0 for n == 1.
__device__ __forceinline__ int reflect(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

__device__ __forceinline__ uint32_t round_byte(float a) { return (uint32_t)(int)fminf(fmaxf(rintf(a), 0.0f), 255.0f); }

template <int S>
__global__ __launch_bounds__(kThreads) void blur_rows(const void* __restrict__ rows, const void* __restrict__ recs,
                                                      int nrecs) {
  constexpr int kRing = 2 * kBlurMaxR + S;
  constexpr int kStageItems = (S * kStageWords + kThreads - 1) / kThreads;
  constexpr int kHItems = S * kCols / kThreads;
  constexpr int kVItems = (S * kGroups + kThreads - 1) / kThreads;
  static_assert(S * kCols % kThreads == 0, "the H pass fills every lane");
  __shared__ uint32_t stage[S * kStageWords];
  __shared__ __attribute__((aligned(16))) float ring[kRing * kCols];

  BlurRecK* bk = (BlurRecK*)recs;
  const int blk = blockIdx.x;
  int lo = 0, hi = nrecs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bk[mid].unit_begin <= blk) lo = mid; else hi = mid - 1;
  }
  BlurRecK& rec = bk[lo];
  EnhRowK& e = ((EnhRowK*)rows)[rec.entry];
  const int w = e.w, h = e.h;
  const int R = (rec.k - 1) >> 1;
  const int unit = blk - rec.unit_begin;
  const int seg = unit / rec.strips, strip = unit - seg * rec.strips;
  const int x0 = strip * kBlurStripW;
  const int y0 = seg * rec.seg_rows, y1 = min(y0 + rec.seg_rows, h);
  const uint8_t* const src = e.src;
  const int64_t sstride = e.src_stride;
  const int64_t limit = sstride * h;
  const int lane = (int)threadIdx.x;

  // The staged row: nb bytes from pixel x0 - R on, `shift` bytes into the row.
  const int nb = (kBlurStripW + 2 * R) * 3;
  const bool interior = x0 - R >= 0 && x0 + kBlurStripW + R <= w;
  const int shift = interior ? ((x0 - R) * 3) & 3 : 0;
  const int nw = (shift + nb + 3) >> 2;
  // The lane's staged dwords: the same columns in every step.
  int srow[kStageItems], scol[kStageItems];
  int soff[kStageItems][4];  // interior: [0], the dword's offset into a source row; edge: its four bytes'
#pragma unroll
  for (int j = 0; j < kStageItems; j++) {
    const int i = lane + kThreads * j;
    srow[j] = i / kStageWords;
    scol[j] = i - srow[j] * kStageWords;
    if (srow[j] >= S || scol[j] >= nw) srow[j] = -1;
    if (interior) {
      soff[j][0] = (x0 - R) * 3 - shift + 4 * scol[j];
    } else {
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int k = min(4 * scol[j] + b, nb - 1);
        const int px = k / 3;
        soff[j][b] = 3 * reflect(x0 - R + px, w) + (k - 3 * px);
      }
    }
  }
  uint32_t pre[kStageItems];
  auto prefetch = [&](int lb) {  // the lane's dwords of the step whose first logical row is lb
#pragma unroll
    for (int j = 0; j < kStageItems; j++) {
      pre[j] = 0;
      if (srow[j] < 0) continue;
      const int64_t ro = (int64_t)reflect(lb + srow[j], h) * sstride;
      if (interior) {
        pre[j] = *reinterpret_cast<const uint32_t*>(src + min(max(ro + soff[j][0], (int64_t)0), limit - 4));
      } else {
#pragma unroll
        for (int b = 0; b < 4; b++)
          pre[j] |= (uint32_t)src[min(max(ro + soff[j][b], (int64_t)0), limit - 1)] << (8 * b);
      }
    }
  };

  const float w0 = rec.w[0];
  const int ncols = 3 * min(kBlurStripW, w - x0);  // the strip's columns inside the image
  uint8_t* const dst = e.dst;
  const int64_t dstride = e.dst_stride;
  const bool wide = ((reinterpret_cast<uint64_t>(dst) | (uint64_t)dstride) & 3) == 0;
  const uint8_t* const sbytes = reinterpret_cast<const uint8_t*>(stage);

  const int nsteps = (y1 - y0 + 2 * R + S - 1) / S;
  int lb = y0 - R;  // the step's first logical row
  int sb = 0;       // its ring slot
  prefetch(lb);
  for (int t = 0; t < nsteps; t++) {
#pragma unroll
    for (int j = 0; j < kStageItems; j++)
      if (srow[j] >= 0) stage[srow[j] * kStageWords + scol[j]] = pre[j];
    __syncthreads();
    if (t + 1 < nsteps) prefetch(lb + S);

    // H: staged bytes -> the ring's float32 rows sb .. sb + S - 1
    {
      int pos[kHItems];
      float a[kHItems];
#pragma unroll
      for (int j = 0; j < kHItems; j++) {
        const int i = lane + kThreads * j;
        const int r = i / kCols, c = i - r * kCols;
        pos[j] = r * (kStageWords * 4) + shift + 3 * R + c;
        a[j] = w0 * (float)sbytes[pos[j]];
      }
      for (int d = 1; d <= R; d++) {
        const float wd = rec.w[d];
#pragma unroll
        for (int j = 0; j < kHItems; j++) {
          const int q = (int)sbytes[pos[j] - 3 * d] + (int)sbytes[pos[j] + 3 * d];
          const float p = wd * (float)q;
          a[j] = a[j] + p;
        }
      }
#pragma unroll
      for (int j = 0; j < kHItems; j++) {
        const int i = lane + kThreads * j;
        const int r = i / kCols, c = i - r * kCols;
        int s = sb + r;
        if (s >= kRing) s -= kRing;
        ring[s * kCols + c] = a[j];
      }
    }
    __syncthreads();

    // V: the output rows lb - R .. lb + S - 1 - R that lie in the segment
#pragma unroll
    for (int j = 0; j < kVItems; j++) {
      const int i = lane + kThreads * j;
      const int yr = i / kGroups, g = i - yr * kGroups;
      const int y = lb - R + yr;
      if (yr >= S || y < y0 || y >= y1 || 4 * g >= ncols) continue;
      int sc = sb + yr - R;
      if (sc < 0) sc += kRing;
      const float4 c4 = *reinterpret_cast<const float4*>(&ring[sc * kCols + 4 * g]);
      float a[4] = {w0 * c4.x, w0 * c4.y, w0 * c4.z, w0 * c4.w};
      for (int d = 1; d <= R; d++) {
        const float wd = rec.w[d];
        int sm = sc - d, sp = sc + d;
        if (sm < 0) sm += kRing;
        if (sp >= kRing) sp -= kRing;
        const float4 m = *reinterpret_cast<const float4*>(&ring[sm * kCols + 4 * g]);
        const float4 p = *reinterpret_cast<const float4*>(&ring[sp * kCols + 4 * g]);
        const float s0 = m.x + p.x, s1 = m.y + p.y, s2 = m.z + p.z, s3 = m.w + p.w;
        const float p0 = wd * s0, p1 = wd * s1, p2 = wd * s2, p3 = wd * s3;
        a[0] = a[0] + p0;
        a[1] = a[1] + p1;
        a[2] = a[2] + p2;
        a[3] = a[3] + p3;
      }
      const uint32_t out = round_byte(a[0]) | round_byte(a[1]) << 8 | round_byte(a[2]) << 16 | round_byte(a[3]) << 24;
      uint8_t* const d = dst + (int64_t)y * dstride + 3 * (int64_t)x0 + 4 * g;
      if (wide && 4 * g + 4 <= ncols) {
        *reinterpret_cast<uint32_t*>(d) = out;
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (4 * g + k < ncols) d[k] = (uint8_t)(out >> (8 * k));
      }
    }
    lb += S;
    sb += S;
    if (sb >= kRing) sb -= kRing;
  }
}

}  // namespace

int launch_blur(const EnhanceRowDev* rows, const BlurRecDev* recs, int nrecs, int nunits, int step, void* stream) {
  if (nrecs <= 0 || nunits <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (step == 4)
    hipLaunchKernelGGL(blur_rows<4>, dim3(nunits), dim3(kThreads), 0, s, static_cast<const void*>(rows),
                       static_cast<const void*>(recs), nrecs);
  else if (step == 8)
    hipLaunchKernelGGL(blur_rows<8>, dim3(nunits), dim3(kThreads), 0, s, static_cast<const void*>(rows),
                       static_cast<const void*>(recs), nrecs);
  else
    return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
