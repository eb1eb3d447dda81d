// batch.cpp -- run_batch (capi_internal.h): per-stream descriptor
// workspaces and the fused launches of one batch's layout (batch_layout.cpp:
// band, wave and general kernels, forked over helper streams when a batch
// needs several).
#include <atomic>
#include <deque>

#include "capi_internal.h"

namespace mxd {
namespace capi {
namespace {

struct Workspace {
  std::mutex mu;
  // Descriptor slots: each launch reads its descriptors from one slot.  A
  // batch whose descriptors a slot holds reuses it; a new one takes the least
  // recently used slot once the launches that read it are done.
  // Reuse is fenced without an event per launch (an event between kernels
  // costs the GPU a few microseconds): batches are numbered in stream order,
  // every slot remembers the last batch that read it, and one event is
  // recorded every kFenceEvery batches; reusing a slot waits on the first
  // fence recorded after its last batch (recording one then if none is).
  // With 16 slots the fence a reuse needs was recorded >= 8 batches earlier
  // and has normally completed.
  static constexpr int kSlots = 16;
  static constexpr uint64_t kFenceEvery = 8;
  static constexpr size_t kMaxFences = 8;
  struct Slot {
    ImgDev* host = nullptr;  // pageable copy (cache key; copy modes' source)
    ImgDev* dev = nullptr;
    ImgDev* zc = nullptr;          // pinned, read by the kernels in place (zero-copy modes)
    bool zc_nc = false;            // zc allocated non-coherent
    const ImgDev* launch = nullptr;  // what the batch's kernels read (dev or zc)
    size_t cap = 0, count = 0;
    hipEvent_t copied = nullptr;   // mode 1: the copy-stream upload landed
    uint64_t last_use = 0;         // LRU clock
    uint64_t last_batch = 0;       // the last batch that read it (0: none)
  } slot[kSlots];
  int cur = -1;
  uint64_t clock = 0;
  uint64_t batch = 0;    // batches launched on this stream
  uint64_t written = 0;  // of them, batches that wrote a slot
  struct Fence {
    hipEvent_t ev;
    uint64_t covers;  // every batch <= covers has finished once ev has
  };
  std::deque<Fence> fences;
  std::vector<hipEvent_t> spare;
  hipStream_t copy = nullptr;
  // Fork/join helpers: the launches of a mixed batch (one per kernel shape)
  // run concurrently on these streams, so one launch's tail overlaps the
  // next instead of idling the CUs between serialized launches.
  static constexpr int kHelpers = 3;
  hipStream_t helper[kHelpers] = {};
  hipEvent_t fork = nullptr, join[kHelpers] = {};
};

// Records a fence covering every batch launched so far on the stream.
int record_fence(Workspace* ws, hipStream_t s) {
  hipEvent_t ev = nullptr;
  if (!ws->spare.empty()) {
    ev = ws->spare.back();
    ws->spare.pop_back();
  } else {
    MXD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  MXD_HIP(hipEventRecord(ev, s));
  ws->fences.push_back({ev, ws->batch});
  while (ws->fences.size() > Workspace::kMaxFences) {
    // a later fence covers everything the oldest did
    ws->spare.push_back(ws->fences.front().ev);
    ws->fences.pop_front();
  }
  return MXD_OK;
}

// Blocks until batch `b` of the stream has finished.
int wait_batch(Workspace* ws, uint64_t b, hipStream_t s) {
  if (b == 0) return MXD_OK;
  for (const Workspace::Fence& f : ws->fences)
    if (f.covers >= b) {
      MXD_HIP(hipEventSynchronize(f.ev));
      return MXD_OK;
    }
  if (int rc = record_fence(ws, s)) return rc;
  MXD_HIP(hipEventSynchronize(ws->fences.back().ev));
  return MXD_OK;
}

class WorkspacePool {
 public:
  Workspace* get(int32_t device, void* stream) {
    std::lock_guard<std::mutex> lock(mu_);
    auto& w = map_[std::make_pair(device, stream)];
    if (!w) w = std::make_unique<Workspace>();
    return w.get();
  }

 private:
  std::mutex mu_;
  std::map<std::pair<int32_t, void*>, std::unique_ptr<Workspace>> map_;
};

WorkspacePool& workspaces() {
  static WorkspacePool* p = new WorkspacePool();
  return *p;
}

// The u8 scratch of a formatted call's two-pass images, one per (device,
// stream) like the descriptor slots: the band / general kernels write it and
// format_rows reads it later on the same stream, so it must outlive the call.
// It only grows; growing first drains the stream that may still read it.  A
// call holds `mu` from taking the scratch until its last launch is enqueued,
// so two threads on one stream cannot interleave writers and readers.
struct FmtScratch {
  std::mutex mu;
  uint8_t* ptr = nullptr;
  size_t cap = 0;
};

FmtScratch* fmt_scratch(int32_t device, void* stream) {
  static std::mutex mu;
  static auto* map = new std::map<std::pair<int32_t, void*>, std::unique_ptr<FmtScratch>>();
  std::lock_guard<std::mutex> lock(mu);
  auto& s = (*map)[std::make_pair(device, stream)];
  if (!s) s = std::make_unique<FmtScratch>();
  return s.get();
}

int grow_scratch(FmtScratch* sc, size_t need, void* stream) {
  if (need <= sc->cap) return MXD_OK;
  if (sc->ptr) {
    MXD_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    MXD_HIP(hipFree(sc->ptr));
    sc->ptr = nullptr;
    sc->cap = 0;
  }
  const size_t cap = std::max<size_t>(need + need / 4, (size_t)1 << 20);
  MXD_HIP(hipMalloc(reinterpret_cast<void**>(&sc->ptr), cap));
  sc->cap = cap;
  return MXD_OK;
}

}  // namespace

int32_t strip_chunks(const DevTable& xt, int32_t crop_x, int32_t crop_w, int32_t ox0, int32_t ox1, bool flip,
                     int32_t c, int32_t vec) {
  const int32_t xa = flip ? crop_w - ox1 : ox0;
  const int32_t xb = flip ? crop_w - 1 - ox0 : ox1 - 1;
  const int32_t lo = xt.first[crop_x + xa];
  const int32_t hi = xt.first[crop_x + xb] + xt.count[crop_x + xb] - 1;
  const int32_t fb0 = (lo * c) & ~(vec - 1);
  return ((hi + 1) * c - fb0 + vec - 1) / vec;
}

int validate(const mxd_image& im, int32_t i) {
  // the message is built only on failure (this runs for every image of every batch)
  auto at = [i](const char* msg) { return fail(MXD_ERR_INVALID, std::string(msg) + " (image " + std::to_string(i) + ")"); };
  if (!im.src || !im.dst) return at("mxd: null src/dst pointer");
  if (im.src_w <= 0 || im.src_h <= 0) return at("image: cannot create image with 0 or negative dimension");
  if (im.channels <= 0 || im.channels > 4) return at("verifyImage: channels must be 0 <= c <= 4");
  if (im.resize_w <= 0 || im.resize_h <= 0 || im.crop_w <= 0 || im.crop_h <= 0)
    return at("image: cannot create image with 0 or negative dimension");
  if (im.crop_x < 0 || im.crop_y < 0 || im.crop_x >= im.resize_w || im.crop_y >= im.resize_h)
    return at("Array: sub: offset out of bound");
  if (im.crop_x + im.crop_w > im.resize_w || im.crop_y + im.crop_h > im.resize_h)
    return at("Array: sub: shape out of bound");
  if (im.src_stride < (int64_t)im.src_w * im.channels) return at("mxd: src_stride smaller than a row");
  if (im.filter < 0 || im.filter >= mxd::kFilterCount) return at("mxd: unknown filter");
  return MXD_OK;
}

// Whether the host can store into the device's memory directly (large PCI
// BAR: the whole HBM mapped for the CPU), cached per device.
bool large_bar(int32_t device) {
  static std::mutex mu;
  static std::map<int32_t, bool> known;
  std::lock_guard<std::mutex> lock(mu);
  auto it = known.find(device);
  if (it != known.end()) return it->second;
  hipDeviceProp_t prop{};
  const bool ok = hipGetDeviceProperties(&prop, device) == hipSuccess && prop.isLargeBar != 0;
  known[device] = ok;
  return ok;
}

// Uploads descs to the stream's workspace (skipped when unchanged) and returns
// the device copy.
int upload_descs(const std::vector<ImgDev>& descs, int32_t device, void* stream, ImgDev** dev_out,
                 std::unique_lock<std::mutex>* hold, Workspace** ws_out = nullptr, bool* hit = nullptr) {
  if (hit) *hit = false;
  Workspace* ws = workspaces().get(device, stream);
  if (ws_out) *ws_out = ws;
  *hold = std::unique_lock<std::mutex>(ws->mu);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t n = descs.size();
  const size_t bytes = sizeof(ImgDev) * n;
  // A batch whose descriptors a slot already holds (a loop over fixed device
  // buffers) launches from that slot's device copy: no upload, no
  // cross-stream wait once the copy has landed.  Slots are immutable while
  // cached, so concurrent readers are safe.
  if (!(g_policy.load() & MXD_POLICY_NO_DESC_CACHE))
    for (int k = 0; k < Workspace::kSlots; k++) {
      Workspace::Slot& c = ws->slot[k];
      if (c.count == n && c.host && std::memcmp(c.host, descs.data(), bytes) == 0) {
        ws->cur = k;
        c.last_use = ++ws->clock;
        c.last_batch = ws->batch + 1;  // the batch about to launch
        if (c.copied && hipEventQuery(c.copied) != hipSuccess) MXD_HIP(hipStreamWaitEvent(s, c.copied, 0));
        *dev_out = const_cast<ImgDev*>(c.launch);
        if (hit) *hit = true;
        return MXD_OK;
      }
    }
  if (!ws->copy) MXD_HIP(hipStreamCreateWithFlags(&ws->copy, hipStreamNonBlocking));
  // the least recently used slot takes the new batch
  int victim = 0;
  for (int k = 1; k < Workspace::kSlots; k++)
    if (ws->slot[k].last_use < ws->slot[victim].last_use) victim = k;
  ws->cur = victim;
  ws->slot[victim].last_use = ++ws->clock;
  Workspace::Slot& c = ws->slot[ws->cur];
  // Host-side wait: the launches that read this slot are done.  (Ordering
  // the upload after them on the GPU instead, with a wait of the copy stream
  // on the compute stream, measured ms-long stalls.)
  if (int rc = wait_batch(ws, c.last_batch, s)) return rc;
  c.last_batch = ws->batch + 1;
  if (n > c.cap) {
    // empty first: a failed allocation below leaves an empty slot (cap 0),
    // never a stale capacity over null buffers
    c.cap = c.count = 0;
    c.launch = nullptr;
    if (c.dev) MXD_HIP(hipFree(c.dev));
    std::free(c.host);
    if (c.zc) MXD_HIP(hipHostFree(c.zc));
    c.dev = nullptr;
    c.host = nullptr;
    c.zc = nullptr;
    const size_t cap = std::max<size_t>(n, 64);
    MXD_HIP(hipMalloc(reinterpret_cast<void**>(&c.dev), sizeof(ImgDev) * cap));
    // the host copy only answers "does a slot hold these descriptors" (and is
    // the source of the copy modes 1 / 2): pageable, so 16 slots per stream
    // cost no page-locked allocations
    c.host = static_cast<ImgDev*>(std::malloc(sizeof(ImgDev) * cap));
    if (!c.host) {
      c.cap = c.count = 0;
      return fail(MXD_ERR_NOMEM, "mxd: out of host memory for descriptors");
    }
    c.cap = cap;
  }
  std::memcpy(c.host, descs.data(), bytes);
  c.count = n;
  // Upload modes (MXD_TUNE_DESC): 1 = copy stream + cross-stream wait, 2 =
  // copy on the launch stream, 3 / 4 = the kernels read the pinned slot in
  // place (coherent / non-coherent allocation), 6 = the host stores into the
  // device slot through the large PCI BAR.  Default 6 (4 without a large
  // BAR): no copy, no cross-stream wait, and the kernels read their
  // descriptors from HBM like a cached batch.  With slot reuse fenced every 4
  // written batches (8 slots), fresh batches cost C2 +0.2-1.5 % and C4
  // -3..+1.5 % over cached descriptors in mode 6, C2 +1.3 % and C4 +3..18 %
  // in mode 4 (profiles/r03/desc_host_d.jsonl, three repetitions); with 16
  // slots fenced every 8, C2 -1.5..0 % and C4 -3..+4.6 %
  // (profiles/r03/fresh_slots16.jsonl); against +3.9 % / +5 %
  // with an event per launch (desc_host.jsonl) and +6.5 % / +31 % for the
  // round-2 copy stream.  A copy kernel on the launch stream bringing the slot
  // into HBM (mode 5 of profiles/r03/desc_host_b.jsonl) measured no better and
  // was dropped.
  int32_t mode = g_tune[MXD_TUNE_DESC].load() > 0 ? g_tune[MXD_TUNE_DESC].load() : 6;
  if (mode == 6 && !large_bar(device)) mode = 4;
  if (mode == 6) {
    // the host stores the array straight into the device slot through the
    // large PCI BAR (~1 us for 13 KB); the fence drains the write-combining
    // buffers before the launch's doorbell, and the kernel-start acquire
    // drops the slot's lines from the L2s.  Kernels read HBM, no PCIe trip.
    std::memcpy(c.dev, descs.data(), bytes);
    std::atomic_thread_fence(std::memory_order_seq_cst);
    c.launch = c.dev;
  } else if (mode >= 3) {
    const bool nc = mode == 4;
    if (!c.zc || c.zc_nc != nc || n > c.cap) {
      if (c.zc) MXD_HIP(hipHostFree(c.zc));
      MXD_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.zc), sizeof(ImgDev) * c.cap,
                            nc ? hipHostMallocNonCoherent : hipHostMallocDefault));
      c.zc_nc = nc;
    }
    std::memcpy(c.zc, descs.data(), bytes);
    c.launch = c.zc;
  } else if (mode == 2) {
    MXD_HIP(hipMemcpyAsync(c.dev, c.host, bytes, hipMemcpyHostToDevice, s));
    c.launch = c.dev;
  } else {
    if (!c.copied) MXD_HIP(hipEventCreateWithFlags(&c.copied, hipEventDisableTiming));
    MXD_HIP(hipMemcpyAsync(c.dev, c.host, bytes, hipMemcpyHostToDevice, ws->copy));
    MXD_HIP(hipEventRecord(c.copied, ws->copy));
    MXD_HIP(hipStreamWaitEvent(s, c.copied, 0));
    c.launch = c.dev;
  }
  *dev_out = const_cast<ImgDev*>(c.launch);
  return MXD_OK;
}

// After the launches of a batch: count it, and every kFenceEvery batches that
// wrote a slot record a fence for slot reuse (a loop of cache hits records
// none: an eviction after it records its fence on demand).
int release_descs(Workspace* ws, void* stream, bool hit) {
  ws->batch++;
  if (!hit && ++ws->written % Workspace::kFenceEvery == 0)
    return record_fence(ws, reinterpret_cast<hipStream_t>(stream));
  return MXD_OK;
}

namespace {

// The call as a whole.  *out_dtype becomes the form the kernels are planned in.
int validate_batch(const mxd_image* images, int32_t n, int32_t* out_dtype, int32_t device, const mxd_out_format* fmt) {
  if (n < 0 || (n > 0 && !images)) return fail(MXD_ERR_INVALID, "mxd: bad image array");
  if (fmt) *out_dtype = MXD_U8;  // the form the kernels of a formatted call are planned in
  if (*out_dtype != MXD_U8 && *out_dtype != MXD_F32_DIV255) return fail(MXD_ERR_INVALID, "mxd: bad out_dtype");
  if (n == 0) return MXD_OK;
  const int64_t elem = *out_dtype == MXD_F32_DIV255 ? 4 : 1;
  for (int32_t i = 0; i < n; i++) {
    if (int rc = validate(images[i], i)) return rc;
    if (!fmt && images[i].dst_stride < (int64_t)images[i].crop_w * images[i].channels * elem)
      return fail(MXD_ERR_INVALID, "mxd: dst_stride smaller than an output row");
  }
  if (fmt)
    if (int rc = fmt_validate_images(images, n, *fmt)) return rc;
  return check_device(device);
}

// Formatted call: the format as the kernels see it and, when some image takes
// two passes, the stream's scratch (held until the last launch is enqueued)
// with the layout's scratch offsets made addresses in it.  fmt == nullptr (a
// colour call with u8 output): no table.
int take_scratch(BatchLayout& L, const mxd_out_format* fmt, int32_t device, void* stream, mxd::OutFmtDev* ofd,
                 std::unique_lock<std::mutex>* hold) {
  if (fmt) {
    ofd->plane_stride = fmt->plane_stride;
    ofd->elem16 = fmt_elem_size(*fmt) == 2 ? 1 : 0;
    ofd->chw = fmt->layout == MXD_LAYOUT_CHW ? 1 : 0;
    if (int rc = fmt_device_table(device, *fmt, L.images[0].channels, &ofd->table)) return rc;
  }
  if (L.scratch_bytes == 0) return MXD_OK;
  FmtScratch* sc = fmt_scratch(device, stream);
  *hold = std::unique_lock<std::mutex>(sc->mu);
  if (int rc = grow_scratch(sc, L.scratch_bytes, stream)) return rc;
  L.add_scratch(sc->ptr);
  return MXD_OK;
}

// Several launches: fork them over the caller's stream and the workspace's
// helper streams (largest first), join back before return, so one launch's
// tail overlaps the next.
int launch_all(const BatchLayout& L, const ImgDev* dev, Workspace* ws, const mxd::OutFmtDev* ofd, void* stream) {
  // Streams: the caller's and one helper by default.  C3's six launches
  // measured 0.465 ms on one stream, 0.429 on two and 0.455 on four
  // (profiles/r03/c3_sizing.jsonl); MXD_TUNE_STREAMS overrides.
  const int32_t knob_streams = g_tune[MXD_TUNE_STREAMS].load();
  const int32_t nstreams = knob_streams > 0 ? knob_streams : 2;
  const int nfork = std::min<int>({(int)L.launches.size() - 1, nstreams - 1, Workspace::kHelpers});
  if (nfork > 0) {
    if (!ws->fork) {
      MXD_HIP(hipEventCreateWithFlags(&ws->fork, hipEventDisableTiming));
      for (int h = 0; h < Workspace::kHelpers; h++) {
        MXD_HIP(hipStreamCreateWithFlags(&ws->helper[h], hipStreamNonBlocking));
        MXD_HIP(hipEventCreateWithFlags(&ws->join[h], hipEventDisableTiming));
      }
    }
    MXD_HIP(hipEventRecord(ws->fork, reinterpret_cast<hipStream_t>(stream)));
    for (int h = 0; h < nfork; h++) MXD_HIP(hipStreamWaitEvent(ws->helper[h], ws->fork, 0));
  }
  const int32_t* tables_dev = reinterpret_cast<const int32_t*>(dev + L.tables_at);
  int launch_rc = MXD_OK;
  for (size_t k = 0; k < L.launches.size(); k++) {
    const int lane = nfork > 0 ? (int)(k % (size_t)(nfork + 1)) : 0;
    void* s = lane == 0 ? stream : reinterpret_cast<void*>(ws->helper[lane - 1]);
    int rc = 0;
    if (L.launches[k].kind == 0) {
      const BatchLayout::BandGroup& g = L.bands[L.launches[k].group];
      rc = mxd::launch_band(g.cfg, dev + g.first, g.table >= 0 ? tables_dev + g.table : nullptr, s);
    } else if (L.launches[k].kind == 1) {
      const BatchLayout::WaveGroup& g = L.waves[L.launches[k].group];
      mxd::WaveCfg cfg = g.cfg;
      cfg.prio = nfork == 0 ? 1 : 0;  // priorities only where launches never overlap
      rc = ofd ? mxd::launch_wave_fmt(cfg, dev + g.first, *ofd, s) : mxd::launch_wave(cfg, dev + g.first, s);
    } else {
      rc = mxd::launch_resample(L.general, dev + L.general_at, s);
    }
    if (rc) {
      launch_rc = fail(MXD_ERR_DEVICE, std::string("resample launch failed: ") + hipGetErrorString(hipGetLastError()) +
                                           " rc=" + std::to_string(rc));
      break;
    }
  }
  // Every helper stream that may hold kernels of this batch joins the
  // caller's stream -- on a failed launch too, so the slot's fence covers the
  // kernels already queued and a caller syncing its own stream waits for
  // their writes.
  for (int h = 0; h < nfork; h++) {
    if (hipEventRecord(ws->join[h], ws->helper[h]) != hipSuccess ||
        hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), ws->join[h], 0) != hipSuccess)
      if (launch_rc == MXD_OK) launch_rc = fail(MXD_ERR_DEVICE, "mxd: joining helper streams failed");
  }
  return launch_rc;
}

// One stage of the chain over its entries in the uploaded copy.
int launch_stage(const BatchLayout& L, const BatchLayout::Stage& st, const ImgDev* dev, const mxd::OutFmtDev& form,
                 void* stream) {
  if (st.count == 0) return MXD_OK;  // (a formatted call whose every image a wave kernel took)
  const void* entries = dev + st.at;
  // The output form is the last stage's: a second pass in front of the mix
  // stage writes u8 scratch rows (pixel_rows without a table).
  const mxd::OutFmtDev ofd = st.writes == Rows::Dst ? form : mxd::OutFmtDev{};
  // (only a mix call has a second pass that is not the last stage: anywhere else it would drop its format)
  if (st.kind == StageKind::Pass && st.writes != Rows::Dst && !L.mixed())
    return fail(MXD_ERR_DEVICE, "mxd: a second pass that does not write the destinations outside a mix call");
  const char* what = "format_rows launch failed: ";
  int rc = 0;
  if (st.kind == StageKind::Warp) {
    what = "warp launch failed: ";
    rc = mxd::launch_warp(static_cast<const mxd::WarpRowDev*>(entries), st.count, st.blocks, st.pre_blocks, L.warp_tab, stream);
  } else if (st.kind == StageKind::Enhance) {
    what = "enhance launch failed: ";
    rc = mxd::launch_enhance(static_cast<const mxd::EnhanceRowDev*>(entries), st.count, st.blocks, stream);
  } else if (st.kind == StageKind::Mix) {
    what = "mix launch failed: ";
    rc = mxd::launch_mix(static_cast<const mxd::MixRowDev*>(entries), st.count, st.blocks, ofd, stream);
  } else if (L.pass == SecondPass::Tone) {
    // this call's statistics start from zero, whatever the stream's last call left
    if (L.tone_stat_bytes > 0 &&
        hipMemsetAsync(L.tone_ws, 0, L.tone_stat_bytes, reinterpret_cast<hipStream_t>(stream)) != hipSuccess)
      return fail(MXD_ERR_DEVICE, std::string("tone workspace memset failed: ") + hipGetErrorString(hipGetLastError()));
    what = "tone launch failed: ";
    rc = mxd::launch_tone(static_cast<const mxd::ToneRowDev*>(entries), st.count, st.pre_blocks, st.blocks, ofd, L.tone_ws,
                          L.matrix, stream);
  } else if (L.pass == SecondPass::Color) {
    what = "color_rows launch failed: ";
    rc = mxd::launch_color_rows(static_cast<const mxd::ColorRowDev*>(entries), st.count, st.blocks, ofd, stream);
  } else {
    rc = mxd::launch_format_rows(static_cast<const mxd::FmtRowDev*>(entries), st.count, st.blocks, ofd, stream);
  }
  if (rc) return fail(MXD_ERR_DEVICE, std::string(what) + hipGetErrorString(hipGetLastError()));
  return MXD_OK;
}

// One launchable batch: its layout, the upload, the launches.
int run_launchable(const mxd_image* images, int32_t n, int32_t out_dtype, int32_t device, void* stream,
                   const Stored* stored, const PostOps& ops) {
  DeviceGuard guard(device);
  BatchLayout L;
  if (int rc = build_layout(device_env(), device, images, n, stored, out_dtype, ops, &L)) return rc;
  mxd::OutFmtDev ofd{};
  std::unique_lock<std::mutex> scratch_hold;
  if (ops.any())
    if (int rc = take_scratch(L, ops.fmt, device, stream, &ofd, &scratch_hold)) return rc;
  ImgDev* dev = nullptr;
  std::unique_lock<std::mutex> hold;
  Workspace* ws = nullptr;
  bool hit = false;
  if (int rc = upload_descs(L.descs, device, stream, &dev, &hold, &ws, &hit)) return rc;
  int launch_rc = launch_all(L, dev, ws, ops.resize_formats() ? &ofd : nullptr, stream);
  // The chain, behind the joins: every resize kernel that wrote scratch rows
  // is ordered before it on the caller's stream.
  for (int32_t s = 0; s < L.nstages && launch_rc == MXD_OK; s++) launch_rc = launch_stage(L, L.chain[s], dev, ofd, stream);
  // The batch is counted on a failed launch too (see launch_all).
  const int rel = release_descs(ws, stream, hit);
  return launch_rc != MXD_OK ? launch_rc : rel;
}

}  // namespace

int prepare_post_ops(const mxd_image* images, int32_t n, PostOps* ops, int32_t* out_dtype, mxd_out_format* f32_fmt) {
  if (!ops->per_image()) return MXD_OK;
  if (n < 0 || (n > 0 && !images)) return fail(MXD_ERR_INVALID, "mxd: bad image array");
  if (ops->warps)
    if (int rc = warp_validate(images, ops->warps, n)) return rc;
  if (ops->enhances)
    if (int rc = enhance_validate(images, ops->enhances, n)) return rc;
  if (ops->tones)
    if (int rc = tone_validate(images, ops->tones, n)) return rc;
  if (ops->colors)
    if (int rc = color_validate(images, ops->colors, n)) return rc;
  if (ops->mixes)
    if (int rc = mix_validate(images, ops->mixes, n)) return rc;
  if (!ops->fmt) {
    if (*out_dtype != MXD_U8 && *out_dtype != MXD_F32_DIV255) return fail(MXD_ERR_INVALID, "mxd: bad out_dtype");
    if (*out_dtype == MXD_F32_DIV255) {
      // the table of {F32, HWC, normalize 0}: q / 255 bit for bit
      *f32_fmt = mxd_out_format{};
      f32_fmt->elem = MXD_ELEM_F32;
      f32_fmt->layout = MXD_LAYOUT_HWC;
      ops->fmt = f32_fmt;
    }
  }
  *out_dtype = MXD_U8;  // the form every image is resized in
  return MXD_OK;
}

// One channel count per launch, and one alpha mode per general-kernel launch.
std::vector<SubBatch> split_batch(const mxd_image* images, int32_t n, const Stored* stored) {
  // launch classes in order: 1, 2, 3 channels, RGBA weighted, RGBA not (the flag means nothing below four channels)
  auto cls = [](const mxd_image& im) { return 2 * im.channels - (im.channels == 4 && im.rgba_weighted ? 1 : 0); };
  std::vector<SubBatch> subs;
  bool mixed = false;
  for (int32_t i = 1; i < n; i++) mixed = mixed || cls(images[i]) != cls(images[0]);
  for (int32_t c = 2; mixed && c <= 8; c++) {
    SubBatch s = partition(images, n, stored, [&](const mxd_image& im) { return cls(im) == c; });
    if (!s.images.empty()) subs.push_back(std::move(s));
  }
  return subs;
}

int run_batch(const mxd_image* images, int32_t n, int32_t out_dtype, int32_t device, void* stream,
              const Stored* stored, PostOps ops) {
  mxd_out_format f32_fmt;
  if (int rc = prepare_post_ops(images, n, &ops, &out_dtype, &f32_fmt)) return rc;
  if (int rc = validate_batch(images, n, &out_dtype, device, ops.fmt)) return rc;
  if (n == 0) return MXD_OK;
  // (a colour or tone call's images all have three channels: one launchable
  // batch, so colors[i] and tones[i] stay beside images[i])
  const std::vector<SubBatch> subs = ops.per_image() ? std::vector<SubBatch>{} : split_batch(images, n, stored);
  if (subs.empty()) return run_launchable(images, n, out_dtype, device, stream, stored, ops);
  for (const SubBatch& s : subs)
    if (int rc = run_launchable(s.images.data(), (int32_t)s.images.size(), out_dtype, device, stream,
                                stored ? s.stored.data() : nullptr, ops))
      return rc;
  return MXD_OK;
}

}  // namespace capi
}  // namespace mxd

