// resample.h -- device-side descriptors shared by capi.cpp and resample.hip.
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace mxd {

// One entry of a per-axis tap table in device memory: the first input index
// and tap count stored as int bits, then `width` f32 weights, zero padded to
// at least kMinTabWidth so the wave and band kernels can read T <=
// kMinTabWidth weights of any entry unconditionally (both read up to their
// largest tap bucket / class, 32).
constexpr int kTapHeader = 2;
constexpr int kMinTabWidth = 32;

// Per-image parameters, resolved by the host (geometry already validated).
// Each image is cut into nbands x nstrips tiles of ty output rows x tx output
// columns; tiles of all images are numbered consecutively from tile_begin.
struct ImgDev {
  const uint8_t* src;
  int64_t src_stride;
  void* dst;
  int64_t dst_stride;
  const float* ytab;  // crop_h entries of (kTapHeader + ywidth) floats
  const float* xtab;  // crop_w entries of (kTapHeader + xwidth) floats
  int32_t ywidth, xwidth;
  int32_t crop_w, crop_h;
  int32_t flip;  // bit 0: mirror; wave path: bits 8.. = byte offset of the
                 // source window past the 4-byte aligned `src` (0..3)
  int32_t tile_begin;
  int32_t nstrips, ty, tx, group;
  int32_t src_w, src_h;  // src_h: rows stored at src (the whole image, or a staged footprint)
  int32_t src_x0, src_y0;  // source pixel at src (0, 0 unless only a footprint is stored)
  const struct YccDev* ycc;  // wave kernels: the source is JPEG sample planes, not RGB (null: RGB at src)
};
static_assert(sizeof(ImgDev) == 112, "ImgDev layout");

// A JPEG image's sample planes as a wave kernel's source (the fused decode
// finish): 4:2:0 YCbCr as jpeg_idct writes them; the kernel
// makes the RGB pixels of the rows it reads in registers, by jpeg_color's
// rules (h2v2 fancy upsampling, jdcolor's fixed-point YCbCr -> RGB).
// ImgDev::src is the Y plane's first byte; the source image is the window
// from (win_x, win_y) (win_x a multiple of 4) of win_w x win_h =
// ImgDev::src_w x src_h pixels.
struct YccDev {
  int64_t cb, cr;          // Cb / Cr plane: byte offset from the Y plane
  int32_t ystride, cstride;
  int32_t dw, dh;          // chroma plane samples per row / rows (jdsample's downsampled size)
  int32_t win_x, win_y;
  int32_t records;         // bytes from the Y plane to the Cr plane's end (the buffer's range)
  int32_t pad;
};
static_assert(sizeof(YccDev) == 48, "YccDev layout");

struct LaunchCfg {
  int32_t vec;        // bytes per thread per source row: 16 (16-byte aligned rows) or 1
  int32_t channels;   // 1..4
  int32_t alpha;      // channels == 4: STBIR_RGBA alpha weighting
  int32_t f32;        // output f32 /255
  int32_t nimgs;
  int32_t ntiles;
  int32_t max_tx, max_ty, max_xw, max_yw, max_vw, max_group;
};

// Wave-per-unit fast paths (wave.hip): source rows 4-byte aligned (a window
// may start at any byte: ImgDev::flip bits 8.. hold the base's misalignment),
// f32 outputs 4-byte aligned, every strip's source window <= wave_window_px()
// pixels (start aligned to wave_window_align()), strip_cols <= 64 q, taps <=
// 17.  Units are numbered through ImgDev::tile_begin exactly like tiles; ty =
// band rows, tx = strip columns.  kind: 0 = gather, 2 = scatter (ImgDev::ytab
// is the schedule, ywidth its words per band, group the offset of its
// iteration entries).  taps = horizontal (and, for gather, vertical) tap
// bucket; s / dmax = scatter shape; q = output pixels per lane; shift = some
// image of the launch has a misaligned base.
struct WaveCfg {
  int32_t channels;
  int32_t f32;  // output mode: 0 u8, 1 f32 q/255, 2 formatted (OutFmtDev; launch_wave_fmt)
  int32_t taps, nimgs, nunits;
  int32_t kind;
  int32_t s, dmax;
  int32_t q, shift;
  int32_t p;  // source pixels per lane (wave_default_p, or 8 for wide RGB windows; RGB 16 = byte lanes)
  int32_t per_img = 0;  // units of every image when all images of the launch have the same count, else 0
  int32_t prio = 1;     // progress-based wave priority (off for the concurrent launches of a mixed batch)
  int32_t ycc = 0;      // sources are JPEG sample planes (ImgDev::ycc; scatter, p = 4, no shift)
  int32_t nt = 0;       // streaming (nt) source loads (scatter kernels; wave.hip LAUX)
};

// A formatted output (mxd_out_format) as the kernels see it: a launch
// argument, never part of the per-image descriptors (a cached descriptor slot
// serves any format).  table: the device copy of mxd_out_format_table's
// output for the launch's channel count, channels x 256 elements.
struct OutFmtDev {
  const void* table;
  int64_t plane_stride;  // CHW: bytes between the channel planes of an image
  int32_t elem16;        // elements are 2 bytes (f16 / bf16), else 4 (f32)
  int32_t chw;           // channel planes, else pixel interleaved
};
constexpr int kWaveOutFmt = 2;  // WaveCfg::f32 of the formatted kernels

// Scatter schedule geometry, shared by the kernel and the host builder:
// register ring slots for DMAX iterations per group, groups per unrolled
// block (a multiple of S whose iterations are a multiple of the ring), words
// per iteration entry (row + S weights).
constexpr int scatter_gcd(int a, int b) { return b ? scatter_gcd(b, a % b) : a; }
// Ring target: 6 (4 slots at DMAX 4) keeps the C2 kernel at 118 VGPRs, i.e.
// 4 waves per SIMD; 12 (166 VGPRs, 3 waves) measured 3 % slower on C2 and
// 1-2 % on C4/C5 (tools/ab.sh, profiles/r02/ring_ab.txt).  Tuning builds
// override it with -DMXD_RING=<n> (kernel and host together).
#ifndef MXD_RING
#define MXD_RING 6
#endif
// Past DMAX 9 (large downscale ratios) a ring of DMAX slots would hold 12-16
// rows of registers: the ring is the smallest size in [MXD_RING, 2 MXD_RING]
// that divides two groups (the block then stays S = 2 groups long).
// Tuning builds: -DMXD_RING_FIXED=<n> uses n slots at every DMAX >= 2.
#ifndef MXD_RING_FIXED
#define MXD_RING_FIXED 0
#endif
// DMAX 5 (1080p / 4K -> 512, C5) takes 4 slots: its RGB u8 kernel then fits
// 124 VGPRs (4 waves per SIMD instead of 3 at 5 slots), C5 0.3244 -> 0.3204 ms
// per launch (profiles/r03/ring_variants.jsonl, variant ring4).
// (Narrow-lane rings of 4 / 3 slots at DMAX 2 / 3, 8 waves per SIMD, were
// measured in round 4 and lost: 480p 0.0935 vs 0.0903 ms per launch, C4
// 0.0236 vs 0.0227, profiles/r04/ring_pack_b.jsonl.)
// JPEG plane sources (wave.hip YccSrc) hold 9 dwords per ring slot: their
// ring is the smallest that keeps the unrolled block at S = 2 groups (3 slots
// at DMAX 1, 4 at DMAX 2, DMAX up to 6, then 6 or 4).
constexpr int kYccLaneBytes = 36;
constexpr int scatter_ring_slots(int dmax, int lane_bytes = 0) {
  if (lane_bytes == kYccLaneBytes)
    return dmax == 1 ? 3 : dmax == 2 ? 4 : dmax <= 6 ? dmax : (2 * dmax) % 6 == 0 ? 6 : 4;
  if (MXD_RING_FIXED > 0 && dmax >= 2) return MXD_RING_FIXED;
  if (dmax == 5 && MXD_RING == 6) return 4;
  if (MXD_RING % dmax == 0) return MXD_RING;
  if (2 * dmax <= MXD_RING) return 2 * dmax;
  if (dmax > 9)
    for (int r = MXD_RING; r <= 2 * MXD_RING; r++)
      if ((2 * dmax) % r == 0) return r;
  return dmax;
}
constexpr int scatter_block_groups(int s, int dmax, int lane_bytes = 0) {
  return scatter_ring_slots(dmax, lane_bytes) / scatter_gcd(scatter_ring_slots(dmax, lane_bytes), s * dmax) * s;
}
constexpr int scatter_entry_words(int s) { return s <= 2 ? 4 : 8; }  // prefetch row, row, s weights

int wave_taps_bucket(int taps);            // supported padded tap count >= taps, or -1
int wave_default_p(int channels);          // source pixels per lane of the gather kernels
int wave_window_px(int channels, int p);   // source pixels one wave covers per row
int wave_window_align(int channels);       // window start alignment (pixels)
// RGB with p = 16: byte lanes (16 bytes per lane, a wave_byte_window()-byte
// window starting at a 16-byte boundary past the 4-byte aligned base).
bool wave_byte_lanes(int channels, int p);
int wave_byte_window();
int wave_plane_floats(int channels, int p);  // LDS floats per wave
int wave_lanes();
int launch_wave(const WaveCfg& cfg, const ImgDev* imgs, void* stream);
// Whether cfg's kernel exists, in its output mode (formatted: wave_fmt.hip)
// and with its load policy (cfg.nt).
bool wave_has_kernel(const WaveCfg& cfg);
// The scatter shapes of the cubic filters (wave_cubic.hip: S = 4, RGB, u8 and
// f32 modes, default load policy): the kernel of cfg (a WaveKernel), or null.
// wave_has_kernel / launch_wave / wave_capacity look there after wave.hip's own.
void* wave_cubic_kernel(const WaveCfg& cfg);
// The formatted-output kernels (wave_fmt.hip; cfg.f32 == kWaveOutFmt): every
// shape wave.hip itself has in the other two modes (not wave_cubic.hip's: a
// formatted call resizes those images into u8 scratch rows and formats them
// with format_rows); wave_capacity() forwards to wave_fmt_capacity().
int launch_wave_fmt(const WaveCfg& cfg, const ImgDev* imgs, const OutFmtDev& fmt, void* stream);
int wave_fmt_capacity(const WaveCfg& cfg, int device);
bool wave_fmt_has_kernel(const WaveCfg& cfg);
// The row stage (row_stage.hip): the second pass behind the resize launches
// of a formatted, colour or tone call, over u8 scratch rows.  One entry per
// image of the pass; a workgroup takes a fixed number of rows of one image,
// workgroups numbered through blk_begin like units through ImgDev::tile_begin.
// The three entry types nest: FmtRowDev is the head of all of them, a colour
// entry adds the image's matrix, a tone entry the image's op on top of that.
//
// u8 rows -> formatted rows (format_rows): the images the band and general
// kernels resize in a formatted call, 1-4 channels, one workgroup per
// kFmtRows rows.
constexpr int kFmtRows = 8;
struct FmtRowDev {
  const uint8_t* src;  // u8 rows, src_stride apart (pixel_rows: 16-byte aligned base, stride a multiple of 16)
  void* dst;
  int64_t src_stride, dst_stride;
  int32_t crop_w, crop_h, channels;
  int32_t blk_begin;   // first of the image's workgroups among the launch's
};
static_assert(sizeof(FmtRowDev) == 48, "FmtRowDev layout");
int launch_format_rows(const FmtRowDev* rows, int nimgs, int nblocks, const OutFmtDev& fmt, void* stream);
// u8 RGB rows -> (per-image byte table) -> (per-image matrix) -> any output
// form (pixel_rows): the second pass of a colour call (mxd_color) and of a
// tone call (mxd_tone), whose every image is resized into u8 scratch rows.
// One workgroup per kPixelRows rows of an image.  fmt.table == nullptr: u8
// output (HWC); else the table's elements, as format_rows writes them.
constexpr int kPixelRows = 8;
// A colour call's entry: the matrix is part of the uploaded bytes, so a
// cached descriptor slot serves the same matrices only.
struct ColorRowDev {
  FmtRowDev head;
  float m[12];  // mxd_color::m, row-major
};
static_assert(sizeof(ColorRowDev) == 96, "ColorRowDev layout");
int launch_color_rows(const ColorRowDev* rows, int nimgs, int nblocks, const OutFmtDev& fmt, void* stream);
// A tone call: three launches on the call's stream.  tone_hist adds the
// histograms of the images whose op needs statistics into the workspace (one
// workgroup per kToneHistRows rows, numbered through hist_begin; none for the
// other images), tone_lut turns every image's statistics and parameters into
// its 3 x 256 byte table (one workgroup per image), pixel_rows looks every
// byte up, applies the matrix and writes the destinations.  An entry says
// where the image's statistics and table lie in the workspace (byte offsets).
// The statistics of an image are kToneStatWords uint32: the histograms of q0,
// q1, q2 and, used by MXD_TONE_CONTRAST only, of the luma byte; they must be
// zero when tone_hist starts.
constexpr int kToneHistRows = 16;
constexpr int kToneStatWords = 4 * 256;
constexpr int kToneLutBytes = 3 * 256;
struct ToneRowDev {
  ColorRowDev color;   // m: the identity without colours
  int32_t op, arg;     // mxd_tone::op, ::arg
  float factor;        // mxd_tone::factor
  int32_t hist_begin;  // first of the image's tone_hist workgroups (the next image's when it has none)
  int32_t stat_off;    // the image's statistics in the workspace, -1: the op needs none
  int32_t lut_off;     // the image's table in the workspace
  int32_t pad[2];
};
static_assert(sizeof(ToneRowDev) == 128, "ToneRowDev layout");
static_assert(std::is_standard_layout<ToneRowDev>::value, "an entry is addressed through its head");
// ws: the workspace's device address; matrix: some image has a colour matrix
// (else the entries hold the identity and the step is skipped).
int launch_tone(const ToneRowDev* rows, int nimgs, int hist_blocks, int row_blocks, const OutFmtDev& fmt, uint8_t* ws,
                bool matrix, void* stream);
// Whether op reads the image's statistics.
inline bool tone_needs_stats(int op) { return op >= 3; }
// The warp stage (warp.hip): between the resize launches and the second pass
// of a warp call (mxd_warp), over u8 RGB scratch rows.  One entry per image; a
// workgroup takes one kWarpTileW x kWarpTileH output tile of one image, tiles
// numbered through tile_begin.  warp_tab (one workgroup per image of path
// kWarpTable, launched only when there is one) first writes the index tables
// xt[w], yt[h] (int32) at tab_off in the workspace.
constexpr int kWarpTileW = 64, kWarpTileH = 16;
// An image's code path: its bytes copied, 16.16 fixed point, double bilinear, table lookup.
enum WarpPath : int32_t { kWarpCopy = 0, kWarpFixed = 1, kWarpBilinear = 2, kWarpTable = 3 };
struct WarpRowDev {
  const uint8_t* src;  // u8 rows (16-byte aligned base, stride a multiple of 16)
  uint8_t* dst;        // scratch rows like src, or the caller's u8 destination (any alignment)
  int64_t src_stride, dst_stride;
  int32_t w, h;
  int32_t tile_begin;  // first of the image's workgroups among the launch's
  int32_t tiles_x;     // tiles per tile row
  int32_t path;        // WarpPath
  uint32_t fill;       // r | g << 8 | b << 16
  int32_t tab_off;     // kWarpTable: the image's tables in the workspace (bytes)
  int32_t tab_index;   // kWarpTable: its warp_tab workgroup; -1 otherwise
  double m[6];         // mxd_warp::m
};
static_assert(sizeof(WarpRowDev) == 112, "WarpRowDev layout");
// tab_rows: how many entries take the table path; ws: the tables' workspace.
int launch_warp(const WarpRowDev* rows, int nimgs, int ntiles, int tab_rows, uint8_t* ws, void* stream);
// The enhance stage (enhance.hip): behind the resize launches (and the warp
// stage) and before the second pass of an enhance call (mxd_enhance), over u8
// RGB scratch rows.  One entry per image; a workgroup takes one kEnhTileW x
// kEnhTileH output tile of one image, tiles numbered through tile_begin.  The
// stage cannot run in place: src and dst are different rows.
constexpr int kEnhTileW = 64, kEnhTileH = 16;
// mxd_enhance_op's values.
enum EnhanceOp : int32_t { kEnhNone = 0, kEnhSharpness = 1, kEnhColor = 2, kEnhBrightness = 3 };
struct EnhanceRowDev {
  const uint8_t* src;  // u8 rows (16-byte aligned base, stride a multiple of 16)
  uint8_t* dst;        // scratch rows like src, or the caller's u8 destination (any alignment)
  int64_t src_stride, dst_stride;
  int32_t w, h;
  int32_t tile_begin;  // first of the image's workgroups among the launch's
  int32_t tiles_x;     // tiles per tile row
  int32_t op;          // EnhanceOp
  float factor;        // mxd_enhance::factor (0 for MXD_ENHANCE_NONE)
};
static_assert(sizeof(EnhanceRowDev) == 56, "EnhanceRowDev layout");
int launch_enhance(const EnhanceRowDev* rows, int nimgs, int ntiles, void* stream);
// The mix stage (mix.hip): the last stage of a mix call (mxd_mix), over u8 RGB
// scratch rows.  One entry per image; a workgroup takes kMixRows rows of one
// image, workgroups numbered through blk_begin.  It reads the image's rows
// and, unless the op is NONE, its partner's rows -- both written by the stage
// before it, so no image reads a mixed byte -- and writes the destinations in
// the call's output form (fmt as pixel_rows takes it: table == nullptr is u8).
constexpr int kMixRows = 8;
// mxd_mix_op's values.
enum MixOp : int32_t { kMixNone = 0, kMixMixup = 1, kMixCutmix = 2 };
struct MixRowDev {
  const uint8_t* src;  // u8 rows (16-byte aligned base, stride a multiple of 16)
  void* dst;           // the caller's destination (any alignment)
  int64_t src_stride, dst_stride;
  int32_t w, h;
  const uint8_t* psrc;  // the partner's rows among those the stage reads (null for kMixNone)
  int64_t psrc_stride;
  int32_t blk_begin;    // first of the image's workgroups among the launch's
  int32_t op;           // MixOp
  float w_self, w_other;   // kMixMixup (0 otherwise)
  int32_t x0, y0, x1, y1;  // kMixCutmix (0 otherwise)
  int32_t pad[2];
};
static_assert(sizeof(MixRowDev) == 96, "MixRowDev layout");
int launch_mix(const MixRowDev* rows, int nimgs, int nblocks, const OutFmtDev& fmt, void* stream);
// What the entries of every stage behind the resize begin with: the rows the
// stage reads and writes.  The host places them by one rule for all stages
// (capi_internal.h, the stage chain); the rest of an entry is its stage's own.
struct RowHead {
  const uint8_t* src;
  void* dst;
  int64_t src_stride, dst_stride;
  int32_t w, h;
};
#define MXD_ROW_HEAD(T, W, H)                                                                                   \
  static_assert(offsetof(T, src) == offsetof(RowHead, src) && offsetof(T, dst) == offsetof(RowHead, dst) &&     \
                    offsetof(T, src_stride) == offsetof(RowHead, src_stride) &&                                 \
                    offsetof(T, dst_stride) == offsetof(RowHead, dst_stride) &&                                 \
                    offsetof(T, W) == offsetof(RowHead, w) && offsetof(T, H) == offsetof(RowHead, h) &&         \
                    sizeof(((T*)nullptr)->dst) == sizeof(void*),                                                \
                #T " begins with a RowHead")
MXD_ROW_HEAD(FmtRowDev, crop_w, crop_h);
MXD_ROW_HEAD(WarpRowDev, w, h);
MXD_ROW_HEAD(EnhanceRowDev, w, h);
MXD_ROW_HEAD(MixRowDev, w, h);
#undef MXD_ROW_HEAD
// Waves of this configuration the device runs at once (occupancy x CUs), 0 if unknown.
int wave_capacity(const WaveCfg& cfg, int device);
// Diagnostics: the occupancy API's blocks per CU, the kernel's VGPRs and LDS
// bytes per block; returns waves per block (-1: no kernel / error).
int wave_kernel_info(const WaveCfg& cfg, int device, int* api_blocks, int* vgprs, int* lds);
// policy: 0 default (16-B loads / stores per thread), 1 nt, 2 nt sc1 (buffer forms)
int launch_copy(const void* src, void* dst, size_t bytes, void* stream, int policy = 0);

// Dynamic LDS bytes the kernel needs for cfg.
int resample_smem_bytes(const LaunchCfg& cfg);

// Enqueues the fused kernel; imgs is a device pointer to cfg.nimgs entries.
int launch_resample(const LaunchCfg& cfg, const ImgDev* imgs, void* stream);

}  // namespace mxd
