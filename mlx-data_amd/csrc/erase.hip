// erase.hip -- the erase launch (resample.h): Random Erasing on the output
// elements of an erase call, behind the stage that wrote them.  Write-only,
// with work proportional to the erased area; one launch covers every box of
// every image of the call.
//
// erase_boxes  a workgroup of 256 lanes takes one unit: 256 consecutive items
//              of one box's quad grid (rows y0..y1 times the image-aligned
//              x-quads, x >> 2 in the window's coordinates, so a quad is both
//              the Philox counter's first word and -- for a destination whose
//              base and strides allow -- one aligned vector store).  The
//              unit's record is found by binary search over unit_begin and
//              read through a uniform (scalar) address.  A lane owns one item:
//              (row, quad) = item / nq, item % nq through the record's
//              reciprocal (a mulhi and one correction, no integer division).
//              Per channel it makes one Philox4x32-10 call and four normals in
//              registers (erase_noise.h), or takes the record's constant.
//              CHW: the four elements of a channel are adjacent in one plane,
//              one 16-byte (f32), 8-byte (16-bit) or 4-byte (u8) store each.
//              HWC: the 3 x 4 values, transposed in registers, are twelve
//              adjacent elements: 3 x 16 bytes, 16 + 8 bytes, or 3 x 4 bytes.
//              Vector stores are nontemporal and need a full quad and a base,
//              stride and plane stride that keep them aligned (tested once per
//              workgroup: uniform).  The partial quads at a box's left and
//              right edges, quads a later box cuts, and misaligned
//              destinations take masked element stores.
//
// Overlap: an element that one of the image's later boxes contains is not
// written here -- that box's own record writes it -- so every element has one
// writer and neither launch nor workgroup order matters.  Bounds: a lane
// stores only elements with x0 <= x < x1 and y0 <= y < y1 of its box, which
// the host checked against the crop window.  No LDS: nothing is reused.  The
// kernel waits on no other workgroup.
//
// Arithmetic: erase_noise.h, shared with the CPU statement (mxd_erase_apply);
// compiled with -ffp-contract=off, said again below.
#include <hip/hip_runtime.h>

#include "devutil.h"
#include "erase_noise.h"
#include "resample.h"

#pragma clang fp contract(off)

namespace mxd {
namespace {

constexpr int kThreads = kEraseItems;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4a8 __attribute__((aligned(8)));

using EraseRecK = const __attribute__((address_space(4))) EraseRecDev;

template <class T>
__device__ __forceinline__ void nt(char* p, T v) {
  __builtin_nontemporal_store(v, MXD_GLOBAL_PTR(T, p));
}

// The record of unit u: the last of nrecs whose first unit is <= u.
__device__ __forceinline__ int record_of_unit(EraseRecK* recs, int nrecs, int u) {
  int lo = 0, hi = nrecs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (recs[mid].unit_begin <= u) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One element of ES bytes.
template <int ES>
__device__ __forceinline__ void store_elem(char* p, uint32_t v) {
  if constexpr (ES == 4) nt<uint32_t>(p, v);
  else if constexpr (ES == 2) nt<uint16_t>(p, (uint16_t)v);
  else nt<uint8_t>(p, (uint8_t)v);
}

// ELEM: noise::Elem; CHW: channel planes.
template <int ELEM, bool CHW>
__global__ __launch_bounds__(kThreads) void erase_boxes(const EraseRecDev* __restrict__ recs, int nrecs) {
  constexpr int ES = ELEM == noise::kElemU8 ? 1 : ELEM == noise::kElemF32 ? 4 : 2;
  const int unit = blockIdx.x;
  EraseRecK* rk = (EraseRecK*)recs;
  EraseRecK& rec = rk[record_of_unit(rk, nrecs, unit)];
  const uint32_t item = (uint32_t)(unit - rec.unit_begin) * kEraseItems + threadIdx.x;
  if (item >= (uint32_t)rec.items) return;
  const uint32_t nq = (uint32_t)rec.nq;
  uint32_t row = __umulhi(item, rec.nq_recip);
  uint32_t rem = item - row * nq;
  if (rem >= nq) row += 1, rem -= nq;
  const int x0 = rec.x0, x1 = rec.x1;
  const int y = rec.y0 + (int)row;
  const int xq = (x0 >> 2) + (int)rem;
  const int xb = 4 * xq;
  // which of the quad's elements this box writes
  uint32_t mask = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int x = xb + k;
    bool in = x >= x0 && x < x1;
#pragma unroll
    for (int l = 0; l < 3; l++)
      in = in && !(x >= rec.later[l][0] && x < rec.later[l][2] && y >= rec.later[l][1] && y < rec.later[l][3]);
    mask |= in ? 1u << k : 0u;
  }
  if (mask == 0) return;

  uint32_t v[3][4];
  bool noise = false;
  if constexpr (ELEM != noise::kElemU8) noise = rec.pixel != 0;
  if (noise) {
    if constexpr (ELEM != noise::kElemU8) {
      const uint32_t s0 = rec.seed[0], s1 = rec.seed[1], b = rec.box_no;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        float z[4];
        noise::pixel_normals(s0, s1, b, (uint32_t)c, (uint32_t)y, (uint32_t)xq, z);
#pragma unroll
        for (int k = 0; k < 4; k++) v[c][k] = noise::elem_bits(z[k], ELEM);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int k = 0; k < 4; k++) v[c][k] = rec.fill[c];
  }

  // widest store of a lane: 16 bytes (f32), 8 (16-bit elements), 4 (u8)
  constexpr int kAlign = ES == 4 ? 16 : ES == 2 ? 8 : 4;
  const int64_t dstride = rec.dst_stride, pstride = rec.plane_stride;
  const uint64_t bits = reinterpret_cast<uint64_t>(rec.dst) | (uint64_t)dstride | (CHW ? (uint64_t)pstride : 0);
  const bool wide = (bits & (kAlign - 1)) == 0 && mask == 0xfu;
  char* const drow = static_cast<char*>(rec.dst) + (int64_t)y * dstride;
  if constexpr (CHW) {
    char* const d = drow + (int64_t)xb * ES;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      char* p = d + c * pstride;
      if (wide) {
        if constexpr (ES == 4) nt<u32x4>(p, u32x4{v[c][0], v[c][1], v[c][2], v[c][3]});
        else if constexpr (ES == 2) nt<u32x2>(p, u32x2{v[c][0] | v[c][1] << 16, v[c][2] | v[c][3] << 16});
        else nt<uint32_t>(p, v[c][0] | v[c][1] << 8 | v[c][2] << 16 | v[c][3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (mask >> k & 1u) store_elem<ES>(p + k * ES, v[c][k]);
      }
    }
  } else {
    char* const d = drow + (int64_t)xb * 3 * ES;
    // e[j]: element j of the quad's twelve, channel j % 3 of pixel j / 3
    uint32_t e[12];
#pragma unroll
    for (int j = 0; j < 12; j++) e[j] = v[j % 3][j / 3];
    if (wide) {
      if constexpr (ES == 4) {
#pragma unroll
        for (int k = 0; k < 3; k++) nt<u32x4>(d + 16 * k, u32x4{e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3]});
      } else if constexpr (ES == 2) {
        nt<u32x4a8>(d, u32x4a8{e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16});
        nt<u32x2>(d + 16, u32x2{e[8] | e[9] << 16, e[10] | e[11] << 16});
      } else {
#pragma unroll
        for (int k = 0; k < 3; k++)
          nt<uint32_t>(d + 4 * k, e[4 * k] | e[4 * k + 1] << 8 | e[4 * k + 2] << 16 | e[4 * k + 3] << 24);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 12; j++)
        if (mask >> (j / 3) & 1u) store_elem<ES>(d + j * ES, e[j]);
    }
  }
}

}  // namespace

int launch_erase(const EraseRecDev* recs, int nrecs, int nunits, int elem, bool chw, void* stream) {
  if (nrecs <= 0 || nunits <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(nunits), block(kThreads);
#define MXD_ERASE_CASE(E)                                                                  \
  case E:                                                                                  \
    if (chw) hipLaunchKernelGGL((erase_boxes<E, true>), grid, block, 0, s, recs, nrecs);   \
    else hipLaunchKernelGGL((erase_boxes<E, false>), grid, block, 0, s, recs, nrecs);      \
    break
  switch (elem) {
    MXD_ERASE_CASE(noise::kElemU8);
    MXD_ERASE_CASE(noise::kElemF32);
    MXD_ERASE_CASE(noise::kElemF16);
    MXD_ERASE_CASE(noise::kElemBF16);
    default:
      return -1;
  }
#undef MXD_ERASE_CASE
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mxd
