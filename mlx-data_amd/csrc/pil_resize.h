// pil_resize.h -- what the host planner and pil_resize.hip share: the shape of
// pil_resize_rows, the kernel of Pillow's 8-bit resize (mxd_filter 16..18).
#pragma once

#include <cstdint>

#include "resample.h"

namespace mxd {

// One workgroup takes a tile of kPilTX output columns x kPilTY output rows of
// one image and streams the tile's source rows through LDS kPilG at a time.
constexpr int kPilTX = 64, kPilTY = 32, kPilG = 4;
// Most taps per axis.  A 16 : 1 Lanczos downscale has 97; the limit bounds the
// LDS of the staged horizontal taps and of the ring of H-resampled rows.
constexpr int kPilMaxTaps = 128;
// Fraction bits of a coefficient (taps.h kPilPrecisionBits; Pillow's PRECISION_BITS).
constexpr int kPilPrecisionShift = 22;
// Bytes per ring row: kPilTX pixels, padded by a dword against bank conflicts.
constexpr int pil_ring_pitch(int channels) { return kPilTX * channels + 4; }

// A launch over ImgDev descriptors as general_group lays them out (tile_begin,
// nstrips, tx = kPilTX, ty = kPilTY; xtab / ytab entries hold int32 8.22
// coefficients in their weight words).
struct PilCfg {
  int32_t channels;  // 1 or 3
  int32_t f32;       // output f32 q / 255, else u8
  int32_t nimgs, ntiles;
  int32_t max_xw, max_yw;  // most taps of any image's horizontal / vertical table
  int32_t seg_bytes;       // LDS bytes per source row: the widest tile footprint plus its dword phase, a multiple of 4
};

// Dynamic LDS bytes of a launch.
int pil_resize_smem_bytes(const PilCfg& cfg);
// Enqueues pil_resize_rows; imgs is a device pointer to cfg.nimgs entries.
int launch_pil_resize(const PilCfg& cfg, const ImgDev* imgs, void* stream);

}  // namespace mxd
