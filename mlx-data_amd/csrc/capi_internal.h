// capi_internal.h -- what the translation units of the C ABI share:
// capi.cpp (extern "C" entry points, pixel maps, process-wide state),
// plan.cpp (tap tables, kernel planning, the schedule cache),
// batch_layout.cpp (build_layout: a batch's descriptors, launch groups and
// launch order, built without a device), batch.cpp (descriptor workspaces,
// run_batch: uploads a layout and launches it, one fused launch per kernel
// shape) and hostpath.cpp / hostjpeg.cpp (host-resident and JPEG batches staged through
// page-locked memory; hostpath.h).  Host only.
#pragma once
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <array>
#include <numeric>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "mxd_amd.h"
#include "band.h"
#include "band_plan.h"
#include "jpeg.h"
#include "jpegdev.h"
#include "jpeghuff.h"
#include "pixmap.h"
#include "resample.h"
#include "taps.h"



#define MXD_HIP(expr)                                                                                    \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return fail(MXD_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace mxd {
namespace capi {

using mxd::ImgDev;
using mxd::LaunchCfg;

// Error message of the calling thread's last failed entry point.
extern thread_local std::string g_error;
int fail(int code, const std::string& msg);
// Every entry point that takes a device ordinal refuses one that does not exist.
int check_device(int32_t device);

// Restores the calling thread's current device on scope exit.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};


// Kernel policy (mxd_set_kernel_policy) and tuning knobs (mxd_set_tuning).
extern std::atomic<int32_t> g_policy;
extern std::atomic<int32_t> g_tune[MXD_TUNE_COUNT];

// ---------------------------------------------------------------------------
// Device tap tables: one per (device, in_size, out_size, filter), covering every
// output pixel of the axis, so any crop window is a pointer offset into it.
struct DevTable {
  float* ptr = nullptr;
  int32_t width = 0;     // max taps of any output
  int32_t padded = 0;    // weights per entry in device memory (>= kMinTabWidth)
  int32_t filter = 0;    // mxd_filter the weights were built with (0 for an identity axis)
  std::vector<int32_t> first, count;  // host copy for tiling decisions
  std::vector<float> w;               // host copy of the weights, `width` per output (scatter schedules)
};

class TableCache {
 public:
  // upload = false: host copies only (ptr stays null), for planning without a device.
  explicit TableCache(bool upload = true) : upload_(upload) {}
  int get(int32_t device, int32_t in, int32_t out, const DevTable** out_tab, int32_t filter = 0) {
    if (filter < 0 || filter >= mxd::kFilterCount)
      return fail(MXD_ERR_INVALID, "mxd: unknown filter " + std::to_string(filter));
    if (in == out) filter = 0;  // the identity for every filter: one table
    std::lock_guard<std::mutex> lock(mu_);
    auto key = std::make_tuple(device, in, out, filter);
    auto it = map_.find(key);
    if (it != map_.end()) {
      *out_tab = it->second.get();
      return MXD_OK;
    }
    mxd::AxisTaps taps;
    if (!mxd::build_axis_taps(in, out, 0, out, &taps, filter))
      return fail(MXD_ERR_INVALID, "image: cannot create image with 0 or negative dimension");
    const int32_t padded = std::max<int32_t>(taps.width, mxd::kMinTabWidth);
    const int32_t stride = mxd::kTapHeader + padded;
    std::vector<float> host((size_t)out * stride, 0.0f);
    for (int32_t i = 0; i < out; i++) {
      float* e = &host[(size_t)i * stride];
      std::memcpy(&e[0], &taps.first[i], 4);
      std::memcpy(&e[1], &taps.count[i], 4);
      std::memcpy(&e[2], &taps.weight[(size_t)i * taps.width], sizeof(float) * taps.width);
    }
    auto tab = std::make_unique<DevTable>();
    tab->width = taps.width;
    tab->padded = padded;
    tab->filter = filter;
    tab->first = taps.first;
    tab->count = taps.count;
    tab->w = taps.weight;
    if (upload_) {
      DeviceGuard g(device);
      MXD_HIP(hipMalloc(&tab->ptr, host.size() * sizeof(float)));
      MXD_HIP(hipMemcpy(tab->ptr, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    *out_tab = tab.get();
    map_[key] = std::move(tab);
    return MXD_OK;
  }

 private:
  bool upload_;
  std::mutex mu_;
  std::map<std::tuple<int32_t, int32_t, int32_t, int32_t>, std::unique_ptr<DevTable>> map_;
};

TableCache& tables();
TableCache& host_tables();  // host copies only (planning without a device)

// ---------------------------------------------------------------------------
// Tiling.
constexpr int32_t kTileRows = 32;          // output rows per tile
constexpr int32_t kStripBytes = 1536;      // target source-footprint bytes per strip row
constexpr int32_t kLdsBudget = 40 * 1024;  // bytes of LDS for the f32 row group
constexpr int32_t kBandMaxRows = 16;       // band kernel: most output rows per unit (short units keep the
                                           // device on few images at a time; the stream makes them cheap)


int32_t strip_chunks(const DevTable& xt, int32_t crop_x, int32_t crop_w, int32_t ox0, int32_t ox1, bool flip,
                     int32_t c, int32_t vec);
int validate(const mxd_image& im, int32_t i);

// ---------------------------------------------------------------------------
// Planning (plan.cpp).
struct ImgPlan {
  const DevTable* xt = nullptr;
  const DevTable* yt = nullptr;
  bool band = false;     // runs on the band kernel (band.hip)
  mxd::BandPlan bp;      // its plan
  bool wave = false;     // runs on a wave kernel (wave.hip), else the general tile kernel
  int32_t bucket = -1;   // wave kernel tap bucket
  int32_t kind = 0;      // wave kernel: 0 gather, 2 scatter
  int32_t s = 0, dmax = 0, p = 0;  // scatter shape (ScatterShape)
  int32_t nstrips = 0, tx = 0, q = 0, shift = 0;
  int32_t pp = 0;  // source pixels per lane
  bool ycc = false;  // reads JPEG sample planes (Stored::ycc)
};

// Shape of the scatter schedule for crop rows [off, off+len) of a vertical
// table, valid for bands starting at any row: dmax = most source rows that are
// new for one output row (after the previous row's last tap), p = prologue
// groups (the first output of a band needs all its taps), s = most output rows
// a source row's weights must reach from its group (accumulator slots).
// s = 0: taps not monotone (not a geometry the scatter kernel handles).
struct ScatterShape {
  int32_t s = 0, dmax = 0, p = 0;
  int32_t lane_bytes = 0;  // of the kernel that runs it (its ring: resample.h scatter_ring_slots)
};
ScatterShape scatter_shape(const DevTable& t, int32_t off, int32_t len);

// The wave kernels' scatter schedule (layout: wave.hip) for crop rows
// [crop_y, crop_y + crop_h) in bands of ty rows: `band_words` words per band,
// the iteration entries `entry_off` words into each.  Returns false if the
// rows do not fit the shape.  (The band kernel's: band_plan.h band_schedule.)
bool scatter_schedule_words(const DevTable& yt, int32_t crop_y, int32_t crop_h, int32_t ty, const ScatterShape& sh,
                            std::vector<int32_t>* words, int32_t* band_words, int32_t* entry_off);

// A schedule in device memory.
struct DevSched {
  int32_t* ptr = nullptr;
  int32_t band_words = 0;  // words per band
  int32_t entry_off = 0;   // word offset of the iteration entries in a band (band kernel: 0)
};
// Both kernels' schedules, built once per (kind, device, vertical geometry,
// crop rows, band height, shape or class) and cached (plan.cpp).
class SchedCache;
SchedCache& schedules();
SchedCache& host_schedules();  // built and checked but never uploaded (ptr stays null)
int scatter_schedule(SchedCache& cache, int32_t device, const DevTable& yt, int32_t src_h, int32_t resize_h,
                     int32_t crop_y, int32_t crop_h, int32_t ty, const ScatterShape& sh, const DevSched** out);
int band_schedule_dev(SchedCache& cache, int32_t device, const DevTable& yt, int32_t src_h, int32_t resize_h,
                      int32_t crop_y, int32_t crop_h, int32_t ty, int32_t db, int32_t s, int32_t min_groups,
                      const DevSched** out);
mxd::AxisView axis_view(const DevTable& t);

bool wave_strips(const DevTable& xt, const mxd_image& im, int32_t pp, int32_t* nstrips, int32_t* tx, int32_t* q);
int32_t band_rows(const std::vector<std::pair<int32_t, int32_t>>& strips, int32_t capacity, int32_t kMaxBand = 64);
int32_t band_capacity_cached(const mxd::BandCfg& cfg, int32_t device);
int32_t wave_capacity_cached(const mxd::WaveCfg& cfg, int32_t device);

// Where an image's source bytes live: the whole image at mxd_image::src, or
// (host path) only its staged footprint: `rows` rows from source row y0 and
// columns from source pixel x0 at base, `stride` bytes apart.
// ycc: a JPEG image's sample planes instead (base = its Y plane; wave.hip
// YccSrc): only a scatter wave kernel with RGB pixel lanes runs it.
struct Stored {
  const uint8_t* base;
  int64_t stride;
  int32_t x0, y0, rows;
  const mxd::YccDev* ycc = nullptr;
};

Stored whole(const mxd_image& im);
bool wave_layout_ok(const mxd_image& im, const Stored& st, int32_t out_dtype);
void plan_band(const mxd_image& im, const Stored& st, int32_t out_dtype, ImgPlan& p);
void plan_wave(const mxd_image& im, const Stored& st, int32_t out_dtype, ImgPlan& p);
// Whether run_batch would resize image im from the JPEG planes st.ycc
// describes (a scatter wave kernel with RGB pixel lanes takes it).
bool ycc_plan_ok(const mxd_image& im, const Stored& st, int32_t out_dtype, int32_t device);

// What a plan depends on: geometry, the stored region's layout and the
// alignments of source and destination.
struct PlanKey {
  int32_t v[21];
  bool operator==(const PlanKey& o) const { return std::memcmp(v, o.v, sizeof v) == 0; }
};
struct PlanKeyHash {
  size_t operator()(const PlanKey& k) const {
    uint64_t h = 1469598103934665603ull;  // FNV-1a over the words
    for (int32_t x : k.v) h = (h ^ (uint32_t)x) * 1099511628211ull;
    return (size_t)h;
  }
};
PlanKey plan_key(const mxd_image& im, const Stored& st);

// ---------------------------------------------------------------------------
// Batch layout (batch_layout.cpp): what one launchable batch (one channel
// count, one alpha mode) uploads and launches, as a plain value.  Building it
// makes no device call of its own: what it needs from a device reaches it
// through a LayoutEnv, whose host form (host_env) plans without one.  There
// the device pointers in the descriptors are null plus their offsets;
// everything else is what the device form builds.
struct LayoutEnv {
  TableCache* tables;
  SchedCache* scheds;
  int32_t band_capacity, wave_capacity;  // workgroups / waves the device runs at once; < 0: ask the device
};
LayoutEnv device_env();
LayoutEnv host_env(int32_t band_capacity, int32_t wave_capacity);

// What follows the resize of a call, as every layer below the entry points
// passes it on.  fmt: a formatted output (mxd_out_format).  colors: a colour
// call, colors[i] belongs to images[i].  tones: a tone call, tones[i] belongs
// to images[i]; colors may be null then (no matrix).  warps: a warp call,
// warps[i] belongs to images[i]; every other member may be null then.
// enhances: an enhance call, enhances[i] belongs to images[i]; every other
// member may be null then.  mixes: a mix call, mixes[i] belongs to images[i] and
// names its partner among the call's images; every other member may be null
// then.
//
// The stage chain.  Behind its resize kernels such a call launches at most
// four stages, in this order: the warp stage (warp.hip; a warp call), the
// enhance stage (enhance.hip; an enhance call), the second pass
// (row_stage.hip: format_rows for the images of a formatted call that no wave
// kernel takes; pixel_rows for every image of a colour or tone call, and,
// with identity matrices, of a warp or enhance call with a format alone), the
// mix stage (mix.hip; a mix call).  The mix stage is always the last and
// writes the output form itself: in a mix call the resize kernels run in
// their u8 mode, a second pass exists only with tones or colours and is
// pixel_rows in its u8 form, and a format alone makes no second pass.
// One rule places their rows.  The resize kernels write u8 scratch rows A.
// Every stage reads the rows the stage before it wrote.  The rows alternate
// A, B, A, B (A is dead once the second stage has read B).  The last stage
// writes the caller's destinations.  Rows B, as large as A, exist when at
// least two stages follow the resize.
enum class SecondPass : int32_t { None, Format, Color, Tone };
enum class StageKind : int32_t { Warp, Enhance, Pass, Mix };
enum class Rows : int32_t { A, B, Dst };
struct PostOps {
  const mxd_out_format* fmt = nullptr;
  const mxd_color* colors = nullptr;
  const mxd_tone* tones = nullptr;
  const mxd_warp* warps = nullptr;
  const mxd_enhance* enhances = nullptr;
  const mxd_mix* mixes = nullptr;
  // (a format alone, or nullptr, converts: a formatted / plain call)
  PostOps(const mxd_out_format* f = nullptr, const mxd_color* c = nullptr, const mxd_tone* t = nullptr,
          const mxd_warp* w = nullptr, const mxd_enhance* e = nullptr, const mxd_mix* m = nullptr)
      : fmt(f), colors(c), tones(t), warps(w), enhances(e), mixes(m) {}
  bool any() const { return fmt || colors || tones || warps || enhances || mixes; }
  bool per_image() const { return colors || tones || warps || enhances || mixes; }  // a colour, tone, warp, enhance or mix call
  SecondPass pass() const {
    // (a warp or enhance call with a format alone: pixel_rows with the identity, which is exact;
    // a mix call: the mix stage writes the format, so tones and colours alone make a second pass)
    return tones                                            ? SecondPass::Tone
           : colors || ((warps || enhances) && fmt && !mixes) ? SecondPass::Color
           : fmt && !mixes                                  ? SecondPass::Format
                                                            : SecondPass::None;
  }
  // The resize kernels write the format themselves (wave kernels in their
  // formatted mode).  A colour or tone call's run in their u8 mode into
  // scratch rows: the output form is pixel_rows' alone.
  bool resize_formats() const { return pass() == SecondPass::Format; }
  // The call's share for the images from `first` on (a host-path chunk).
  PostOps at(int32_t first) const {
    return PostOps{fmt, colors ? colors + first : nullptr, tones ? tones + first : nullptr,
                   warps ? warps + first : nullptr, enhances ? enhances + first : nullptr,
                   mixes ? mixes + first : nullptr};  // (a mix call is one chunk: partners index from `first` = 0)
  }
};

struct BatchLayout {
  struct BandGroup {
    int32_t first, count, units;  // first descriptor, images, units
    mxd::BandCfg cfg;
    int32_t table = -1;  // word offset of its unit -> image table among the tables (per_img == 0)
  };
  struct WaveGroup {
    int32_t first, count, units, ty;
    mxd::WaveCfg cfg;
  };
  struct Launch {
    int64_t units;  // a band unit (a workgroup) counts as 4 wave units
    int32_t kind;   // 0 band, 1 wave, 2 general
    int32_t group;
  };
  int32_t n = 0;
  std::vector<ImgPlan> plans;     // by batch index
  std::vector<int32_t> image_of;  // batch index of descriptor k < n: band, then wave, then general images
  // One upload, in ImgDev-sized blocks: the n descriptors, the unit -> image
  // tables from tables_at, the stages' entries from fmt_at (Stage::at each).
  // fmt_at is where the tables end, with or without stages; the second pass,
  // whose entries come first, has at == fmt_at.
  std::vector<ImgDev> descs;
  size_t tables_at = 0, fmt_at = 0;
  std::vector<BandGroup> bands;
  std::vector<WaveGroup> waves;
  int32_t general_at = 0;  // first descriptor of the general kernel
  LaunchCfg general{};     // nimgs == 0: no general launch
  std::vector<Launch> launches;  // largest first
  // What follows the resize: the stage chain (the rule above PostOps), in
  // launch order.  A stage's entries lie in the upload from block `at`:
  // `count` entries of `entry_size` bytes, all beginning with the RowHead that
  // head() returns (resample.h).  Their src, and their dst unless the stage
  // writes the destinations, are offsets into a scratch of scratch_bytes
  // until add_scratch() makes them addresses.
  struct Stage {
    StageKind kind;
    Rows reads, writes;
    size_t at = 0, entry_size = 0;
    int32_t count = 0;
    int32_t blocks = 0;      // workgroups of its kernel over the entries
    int32_t pre_blocks = 0;  // of the kernel in front of it: warp_tab (the table-path images), tone_hist
  };
  Stage chain[4];
  int32_t nstages = 0;
  Stage* stage(StageKind k) {
    for (int32_t s = 0; s < nstages; s++)
      if (chain[s].kind == k) return &chain[s];
    return nullptr;
  }
  const Stage* stage(StageKind k) const { return const_cast<BatchLayout*>(this)->stage(k); }
  uint8_t* head(const Stage& st, int32_t j) { return reinterpret_cast<uint8_t*>(descs.data() + st.at) + (size_t)j * st.entry_size; }
  // The scratch: rows A from 0 (the resize kernels' destinations, 256-byte
  // aligned each), rows B the same rows b_at (a multiple of 256; 0 without B)
  // further on, the warp stage's index tables (w + h int32 per table-path
  // image) from warp_tab_at, a tone call's workspace from tone_ws_at (a
  // multiple of 256): tone_stat_bytes of statistics (one block per image whose
  // op needs them; zeroed for every call), then one table per image.
  // warp_tab, tone_ws: their addresses once add_scratch() knows the scratch.
  // The second pass reads, in a formatted call, the images no wave kernel
  // takes; in a colour or tone call every image (wave kernels in their u8 mode
  // included), entries in batch order.  The other stages have one entry
  // per image in batch order.
  SecondPass pass = SecondPass::None;  // the second pass's kernel
  bool matrix = false;  // pixel_rows applies the entries' matrices (a tone call without colours: the identity, skipped)
  std::vector<mxd_image> images;  // the batch with the destinations the resize kernels write
  size_t scratch_bytes = 0, b_at = 0, warp_tab_at = 0, tone_ws_at = 0, tone_stat_bytes = 0;
  uint8_t* warp_tab = nullptr;
  uint8_t* tone_ws = nullptr;
  // The chain by its members' names (0 / false for a stage the call has not).
  bool warped() const { return stage(StageKind::Warp) != nullptr; }
  bool enhanced() const { return stage(StageKind::Enhance) != nullptr; }
  size_t warp_at() const { return warped() ? stage(StageKind::Warp)->at : 0; }
  size_t enhance_at() const { return enhanced() ? stage(StageKind::Enhance)->at : 0; }
  int32_t warp_tiles() const { return warped() ? stage(StageKind::Warp)->blocks : 0; }
  int32_t warp_tab_count() const { return warped() ? stage(StageKind::Warp)->pre_blocks : 0; }
  int32_t enhance_tiles() const { return enhanced() ? stage(StageKind::Enhance)->blocks : 0; }
  bool mixed() const { return stage(StageKind::Mix) != nullptr; }
  size_t mix_at() const { return mixed() ? stage(StageKind::Mix)->at : 0; }
  int32_t mix_blocks() const { return mixed() ? stage(StageKind::Mix)->blocks : 0; }
  const Stage* second() const { return stage(StageKind::Pass); }
  size_t entry_size() const { return second() ? second()->entry_size : 0; }
  int32_t fmt_count() const { return second() ? second()->count : 0; }
  int32_t fmt_blocks() const { return second() ? second()->blocks : 0; }
  int32_t tone_hist_blocks() const { return second() ? second()->pre_blocks : 0; }
  mxd::FmtRowDev& entry(int32_t j) { return *reinterpret_cast<mxd::FmtRowDev*>(head(*second(), j)); }
  mxd::WarpRowDev& warp_entry(int32_t i) { return *reinterpret_cast<mxd::WarpRowDev*>(head(*stage(StageKind::Warp), i)); }
  mxd::EnhanceRowDev& enhance_entry(int32_t i) {
    return *reinterpret_cast<mxd::EnhanceRowDev*>(head(*stage(StageKind::Enhance), i));
  }
  mxd::MixRowDev& mix_entry(int32_t i) { return *reinterpret_cast<mxd::MixRowDev*>(head(*stage(StageKind::Mix), i)); }
  const int32_t* unit_tables() const { return reinterpret_cast<const int32_t*>(descs.data() + tables_at); }
  void add_scratch(uint8_t* base);
};
// ops.fmt: out_dtype is not read; the format's values are launch arguments,
// not part of the layout.  A colour or tone call is planned as a u8 call into
// scratch whatever ops.fmt and out_dtype say.
int build_layout(const LayoutEnv& env, int32_t device, const mxd_image* images, int32_t n, const Stored* stored,
                 int32_t out_dtype, const PostOps& ops, BatchLayout* out);

// The images of a batch for which pred holds, in batch order, with their
// stored entries.
struct SubBatch {
  std::vector<mxd_image> images;
  std::vector<Stored> stored;
};
template <class Pred>
SubBatch partition(const mxd_image* images, int32_t n, const Stored* stored, Pred pred) {
  SubBatch s;
  for (int32_t i = 0; i < n; i++)
    if (pred(images[i])) {
      s.images.push_back(images[i]);
      if (stored) s.stored.push_back(stored[i]);
    }
  return s;
}
// The launchable sub-batches of a batch, in launch order: by channel count,
// RGBA with weighted alpha first.  Empty: the batch is launchable as it is.
std::vector<SubBatch> split_batch(const mxd_image* images, int32_t n, const Stored* stored);

// ---------------------------------------------------------------------------
// Batches (batch.cpp): one fused launch per kernel shape over a batch whose
// sources are in device memory (or, from the host path, staged: stored[i]):
// validation, split_batch, build_layout, then upload and launches.
// ops.fmt alone: a formatted output (out_dtype is not read).  Images a wave
// kernel takes are written in that form by the resize launch; the others are
// resized into a per-(device, stream) u8 scratch and formatted by one
// format_rows launch that follows on the stream.
// ops.colors / ops.tones: a colour / tone call; ops.fmt == nullptr then means
// out_dtype's form (MXD_U8 / MXD_F32_DIV255).  Every image is resized into the
// scratch in u8 and the row stage (a tone call: tone_hist, tone_lut, then
// pixel_rows) writes the destinations.
int run_batch(const mxd_image* images, int32_t n, int32_t out_dtype, int32_t device, void* stream,
              const Stored* stored = nullptr, PostOps ops = {});
// The head of every colour and tone call (nothing to do for the others):
// validates the warps, the enhances, the tones, then the matrices, makes ops->fmt the format pixel_rows
// writes (f32_fmt, the q / 255 table, for MXD_F32_DIV255; null stays null for
// MXD_U8) and *out_dtype the form the kernels are planned in.
int prepare_post_ops(const mxd_image* images, int32_t n, PostOps* ops, int32_t* out_dtype, mxd_out_format* f32_fmt);

// ---------------------------------------------------------------------------
// Colour transform (color.cpp).
// An entry as the kernels and the CPU statement use it: |m| < 2^-100 is zero.
float color_entry(float m);
// colors[i] against images[i] (images may be null: the matrices alone).
int color_validate(const mxd_image* images, const mxd_color* colors, int32_t n);

// ---------------------------------------------------------------------------
// Tone operations (tone.cpp).
// tones[i] against images[i] (images may be null: the tones alone).
int tone_validate(const mxd_image* images, const mxd_tone* tones, int32_t n);

// ---------------------------------------------------------------------------
// Affine warps (warp.cpp).
// warps[i] against images[i] (its crop window's size).
int warp_validate(const mxd_image* images, const mxd_warp* warps, int32_t n);
// One warp against a w x h image.
int warp_validate_one(const mxd_warp& warp, int32_t w, int32_t h);

// ---------------------------------------------------------------------------
// Enhance operations (enhance.cpp).
// enhances[i] against images[i] (images may be null: the entries alone).
int enhance_validate(const mxd_image* images, const mxd_enhance* enhances, int32_t n);

// ---------------------------------------------------------------------------
// MixUp / CutMix (mix.cpp).
// mixes[i] against images[i] and its partner's (images may be null: the entries alone).
int mix_validate(const mxd_image* images, const mxd_mix* mixes, int32_t n);

// ---------------------------------------------------------------------------
// Formatted outputs (outfmt.cpp).
int32_t fmt_elem_size(const mxd_out_format& fmt);
// The format itself (null, elem, layout; mean / std of the first `channels` channels).
int fmt_validate(const mxd_out_format* fmt, int32_t channels);
// The destinations of a call against it (alignment, strides, one channel count under CHW).
int fmt_validate_images(const mxd_image* images, int32_t n, const mxd_out_format& fmt);
// channels x 256 elements: what each result byte of each channel becomes.
void fmt_table(const mxd_out_format& fmt, int32_t channels, void* table);
// Its cached device copy.
int fmt_device_table(int32_t device, const mxd_out_format& fmt, int32_t channels, const void** out);

// ---------------------------------------------------------------------------
// Host-resident batches (hostpath.cpp; JPEG batches: hostjpeg.cpp; what
// those two share is in hostpath.h).
// ops (device destinations only): every chunk's launch writes ops.fmt, and is
// a colour / tone call with the chunk's slice of the matrices / tones.
int host_path(const mxd_image* images, int32_t n, int32_t out_dtype, int32_t device, bool dst_device,
              const mxd_jpeg_image* jpeg = nullptr, PostOps ops = {});
int jpeg_path(const mxd_jpeg_image* jimg, int32_t n, int32_t out_dtype, int32_t device, bool dst_device,
              PostOps ops = {});
// mxd_host_stats counters: host-path calls, images, wall ns, device-wait ns,
// coefficient parses, parse ns
extern std::atomic<int64_t> g_host_stats[6];
extern std::atomic<int64_t> g_device_stats[2];  // mxd_device_stats: timed chunks, device ns
int64_t now_ns();
extern std::atomic<int64_t> g_plane_sources;  // images resized from their JPEG sample planes (mxd_jpeg_plane_sources)
extern std::atomic<int64_t> g_narrow_images;  // f32 results returned to the host as u8 (mxd_narrow_returns)
const mxd::jpeg::Coefs* coefs_of(const mxd_jpeg_coefs* c);
// Frees the buffers of every idle host-path context (mxd_release_host_buffers).
void host_trim();

// ---------------------------------------------------------------------------
// Pixel maps (capi.cpp; host images: hostpath.cpp).
int pix_validate(const mxd_pixmap& im, int32_t op, int32_t i);
int run_pixmap(const mxd_pixmap* images, int32_t n, int32_t op, int32_t device, void* stream);
int pixmap_host(const mxd_pixmap* images, int32_t n, int32_t op, int32_t device);

}  // namespace capi
}  // namespace mxd
