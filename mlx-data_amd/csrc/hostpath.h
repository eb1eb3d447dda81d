// hostpath.h -- what the two translation units of the host path share:
// hostpath.cpp (context pool, helper threads, the chunk driver, the raw-image
// source, the output side) and hostjpeg.cpp (the JPEG source: chunk layout,
// staging, the decode launches).  Host only.
#pragma once
#include "capi_internal.h"

#include <array>
#include <functional>

namespace mxd {
namespace capi {

// ---------------------------------------------------------------------------
// Each call borrows a context from its device's pool (a bounded number, so
// pinned / device memory is bounded no matter how many threads call), and
// runs the batch in chunks over the context's two slots: while the GPU copies
// in, computes and copies out chunk k on one slot's stream, the calling
// thread stages chunk k+1 into the other slot's pinned buffer and copies
// chunk k-1's results out.
struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  uint8_t* pin_in = nullptr;
  size_t pin_in_cap = 0;
  uint8_t* pin_out = nullptr;
  size_t pin_out_cap = 0;
  uint8_t* dev_in = nullptr;
  size_t dev_in_cap = 0;
  uint8_t* dev_out = nullptr;
  size_t dev_out_cap = 0;
  uint8_t* dev_mid = nullptr;  // JPEG chunks: IDCT samples + decoded RGB images
  size_t dev_mid_cap = 0;
  int32_t* huff_err = nullptr;  // page-locked: the entropy decode's error word, copied back with the chunk
  // MXD_TUNE_DEVICE_TIMING: events around the chunk's kernels (timed: this
  // chunk recorded them)
  hipEvent_t k0 = nullptr, k1 = nullptr;
  bool timed = false;
};

struct HostCtx {
  Slot slot[2];
};

// Per image: the staged footprint (columns from x0, 16-byte aligned so both
// kernel families read it as they would the whole image) and its offsets.
struct Stage {
  int32_t x0, y0, rows;
  int64_t pitch, copy, in_off, out_off, out_row;
  int64_t stage_row;            // an output row as staged (u8 for a narrow return)
  bool narrow = false;          // f32 results returned as u8, expanded on the host
  int64_t in_size;              // staged bytes (footprint rows, or a JPEG's coefficients)
  bool src_pinned, dst_pinned;  // page-locked host memory: DMA'd directly, no staging copy
  bool pending = false;         // JPEG whose entropy decode runs on the device (nothing staged at in_off)
  const uint8_t* src_dev;       // zero copy: the kernel reads the page-locked source in place
  uint8_t* dst_dev;             // zero copy: the kernel writes the page-locked destination in place
  std::array<int32_t, 4> foot;  // JPEG: the resize footprint (x0, x1, y0, y1, inclusive, in image pixels)
};

struct ChunkRange {
  int32_t first, end;  // images [first, end)
};

// Chunk tables of a JPEG chunk (device-side finish, jpegdev.h): where the
// coefficients, descriptors and quantisation tables sit in the staged input,
// and the decoded images in the slot's dev_mid buffer.
struct JpegChunk {
  std::vector<mxd::JpegPlaneDev> planes;
  std::vector<mxd::JpegImgDev> imgs;
  std::vector<uint16_t> qtabs;
  std::vector<mxd::YccDev> ycc;  // per image: its planes as a resize source (used when JpegImgDev::skip)
  int64_t planes_off = 0, imgs_off = 0, q_off = 0, ycc_off = 0, end = 0;  // in the staged input
  int64_t samples = 0, rgb_off = 0, mid_bytes = 0;             // in dev_mid
  int64_t nblocks = 0, max_quad_rows = 0;  // max_quad_rows: the colour kernel's threads per image (8 pixels each)
  // Device entropy decode of the chunk's pending images (jpeghuff.h): their
  // unstuffed segments (words_off..), tables, image / segment / job records in
  // the staged input; their coefficients in dev_in past the staged bytes
  // ([coef_off, dev_end), written by the decode, never copied).
  std::vector<mxd::HuffDev> htabs;
  struct TableSet {
    std::array<uint64_t, 8> key;  // device_table serials
    int n;
    int32_t first;                // in htabs
  };
  std::vector<TableSet> table_sets;
  std::vector<mxd::HuffImgDev> himgs;
  std::vector<mxd::HuffSegDev> hsegs;
  std::vector<mxd::HuffJobDev> hjobs;
  struct Raw {
    const uint8_t *b, *e;  // raw segment bytes
    int64_t at;            // staged byte offset (relative to words_off)
  };
  std::vector<Raw> raw;              // per staged segment (hsegs entries)
  std::vector<int32_t> seg_first;    // per chunk image: its first raw entry (-1: not pending)
  std::vector<int32_t> seg_count;    // and their number
  std::vector<int64_t> pend_rel;     // per chunk image: its coefficients relative to coef_off (-1: not pending)
  int64_t words_off = 0, words_bytes = 0, htabs_off = 0, himgs_off = 0, hsegs_off = 0, hjobs_off = 0;
  int64_t coef_off = 0, coef_bytes = 0, dev_end = 0;
  int64_t pub_off = 0;  // the jobs' publication records + launch control, zeroed with the coefficients
  int32_t huff_threads = 0;
  int64_t huff_lds = 0;  // the largest job's dynamic LDS (its words included when they fit)
  bool huff_search = false;  // some table needs the searching kernel (HuffDev::search)
};

// Lays out the chunk `r` of a JPEG batch whose host-decoded coefficients are
// staged at st[i].in_off; the tables follow at `tables_at`.  Host arithmetic
// only (tests/native/jpeg_layout.cpp pins it without a device).
void jpeg_chunk(const mxd_jpeg_image* jimg, const Stage* st, ChunkRange r, int64_t tables_at, JpegChunk* out);

// One host_path() call: its arguments, the per-image plan, and the chunk the
// driver is building on slot `sl`.
struct HostCall {
  const mxd_image* images;
  int32_t n, out_dtype, device;
  bool dst_device;
  const mxd_jpeg_image* jpeg;  // not null: images[i] is jpeg[i]'s window (hostjpeg.cpp)
  // ops.fmt: every chunk's launch writes this format into the (device)
  // destinations; out_dtype is then MXD_U8, the form the kernels are planned
  // in.  A colour or tone call: a chunk's launch gets ops.at(its first image).
  PostOps ops;
  std::vector<Stage> st;
  std::vector<ChunkRange> chunks;
  HostCtx* ctx = nullptr;
  int pending[2] = {-1, -1};  // chunk in flight on each slot
  // the chunk being built
  ChunkRange cur{0, 0};
  Slot* sl = nullptr;
  int64_t in_bytes = 0, in_staged = 0;  // of pin_in / dev_in: all inputs, and those the staged copy covers
  int64_t dev_in_bytes = 0;             // device-only bytes past them
  int64_t out_bytes = 0, out_staged = 0;
  bool zero_copy = false;               // the kernels read / write the slot's page-locked buffers in place
  const uint8_t* pin_in_dev = nullptr;  // zero copy through the staging buffers: their device-side addresses
  uint8_t* pin_out_dev = nullptr;
  std::vector<mxd_image> dev_imgs;  // the chunk's images as run_batch gets them
  std::vector<Stored> where;
  JpegChunk jc;

  int32_t launch_dtype(int32_t i) const { return st[i].narrow ? MXD_U8 : out_dtype; }
};

// The JPEG source (hostjpeg.cpp), step by step as host_path() calls it.
int jpeg_plan_input(HostCall& c, int32_t i);  // coefficient size, pending, the resize footprint
int jpeg_lay_out(HostCall& c);                // staged offsets + the chunk's tables; grows dev_mid
void jpeg_stage(HostCall& c, int32_t i);      // coefficients, or unstuffed segments (helper threads)
int jpeg_bind(HostCall& c);                   // RGB frame or planes per image; the chunk's tables into pin_in
int jpeg_enqueue(HostCall& c);                // decode, IDCT, colour

// Helpers of both.
int grow_pinned(uint8_t** p, size_t* cap, size_t need);
int grow_device(uint8_t** p, size_t* cap, size_t need);
// Page-locked host memory of this HIP runtime (hipHostMalloc'd or
// registered): the DMA engines can read / write it in place.
bool host_pinned(const void* p);
// The device-side address of page-locked host memory (kernels read it over
// PCIe), or null when the runtime gives none.
const uint8_t* host_device_ptr(const void* p);
// Source footprint of an image's crop window (rows [y_lo, y_hi], pixels
// [x_lo, x_hi]): taps are monotone, so the window's ends bound it.
void footprint(const DevTable& xt, const DevTable& yt, const mxd_image& im, int32_t* x_lo, int32_t* x_hi,
               int32_t* y_lo, int32_t* y_hi);
// f(i) for i in [first, end), split over helper threads when `bytes` of host
// memory traffic are worth it.
void parallel_items(int32_t first, int32_t end, int64_t bytes, const std::function<void(int32_t)>& f);

}  // namespace capi
}  // namespace mxd
