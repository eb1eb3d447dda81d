// format_rows.hip -- u8 rows -> formatted rows (mxd_out_format): the second
// pass of the images a formatted call resizes on the band and general
// kernels (their stores are tuned for u8 / f32 rows and stay as they are; the
// wave kernels write the format themselves, wave_fmt.hip).  One launch covers
// all such images of a call: a workgroup takes kRows rows of one image, copies
// the format's table (mxd_out_format_table's output, channels x 256 elements)
// into LDS and looks every byte up, so the elements equal the table by
// construction -- the same values the wave kernels store.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "resample.h"

namespace mxd {
namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void format_rows(const FmtRowDev* __restrict__ rows, int nimgs, OutFmtDev fmt) {
  __shared__ uint32_t tab[4 * 256];
  const int blk = blockIdx.x;
  int lo = 0, hi = nimgs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].blk_begin <= blk) lo = mid; else hi = mid - 1;
  }
  const FmtRowDev& im = rows[lo];
  const int c = im.channels, w = im.crop_w, h = im.crop_h;
  const int e16 = fmt.elem16, chw = fmt.chw;
  for (int i = threadIdx.x; i < c * 256; i += kThreads)
    tab[i] = e16 ? (uint32_t)static_cast<const uint16_t*>(fmt.table)[i] : static_cast<const uint32_t*>(fmt.table)[i];
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

}  // namespace

int launch_format_rows(const FmtRowDev* rows, int nimgs, int nblocks, const OutFmtDev& fmt, void* stream) {
  if (nimgs <= 0 || nblocks <= 0) return 0;
  hipLaunchKernelGGL(format_rows, dim3(nblocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), rows, nimgs,
                     fmt);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
