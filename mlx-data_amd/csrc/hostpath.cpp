// hostpath.cpp -- host-resident batches (hostpath.h): the context pool, the
// helper threads, the chunk driver (host_path), the raw-image source (sources
// staged through page-locked memory, or read in place over PCIe) and the
// output side (results copied out, or written to device destinations).  The
// JPEG source is hostjpeg.cpp.
#include "hostpath.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>

#include <immintrin.h>
#include <sched.h>

namespace mxd {
namespace capi {

std::atomic<int64_t> g_plane_sources{0};
std::atomic<int64_t> g_narrow_images{0};
std::atomic<int64_t> g_host_stats[6] = {};
std::atomic<int64_t> g_device_stats[2] = {};
int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

int grow_pinned(uint8_t** p, size_t* cap, size_t need) {
  if (need <= *cap) return MXD_OK;
  if (*p) MXD_HIP(hipHostFree(*p));
  *p = nullptr;
  *cap = 0;
  const size_t c = (need + (1 << 20) - 1) & ~(size_t)((1 << 20) - 1);
  MXD_HIP(hipHostMalloc(reinterpret_cast<void**>(p), c, hipHostMallocDefault));
  *cap = c;
  return MXD_OK;
}

int grow_device(uint8_t** p, size_t* cap, size_t need) {
  if (need <= *cap) return MXD_OK;
  if (*p) MXD_HIP(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  const size_t c = (need + (1 << 20) - 1) & ~(size_t)((1 << 20) - 1);
  MXD_HIP(hipMalloc(reinterpret_cast<void**>(p), c));
  *cap = c;
  return MXD_OK;
}

bool host_pinned(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory is not an error here
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

const uint8_t* host_device_ptr(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeHost || !a.devicePointer) {
    (void)hipGetLastError();
    return nullptr;
  }
  return static_cast<const uint8_t*>(a.devicePointer);
}

void footprint(const DevTable& xt, const DevTable& yt, const mxd_image& im, int32_t* x_lo, int32_t* x_hi,
               int32_t* y_lo, int32_t* y_hi) {
  const int32_t xa = im.crop_x, xb = im.crop_x + im.crop_w - 1;
  const int32_t ya = im.crop_y, yb = im.crop_y + im.crop_h - 1;
  *x_lo = xt.first[xa];
  *x_hi = xt.first[xb] + xt.count[xb] - 1;
  *y_lo = yt.first[ya];
  *y_hi = yt.first[yb] + yt.count[yb] - 1;
}

namespace {

void free_slot_buffers(Slot& s) {
  if (s.pin_in) (void)hipHostFree(s.pin_in);
  if (s.pin_out) (void)hipHostFree(s.pin_out);
  if (s.dev_in) (void)hipFree(s.dev_in);
  if (s.dev_out) (void)hipFree(s.dev_out);
  if (s.dev_mid) (void)hipFree(s.dev_mid);
  if (s.huff_err) (void)hipHostFree(s.huff_err);
  s.huff_err = nullptr;
  s.pin_in = s.pin_out = s.dev_in = s.dev_out = s.dev_mid = nullptr;
  s.pin_in_cap = s.pin_out_cap = s.dev_in_cap = s.dev_out_cap = s.dev_mid_cap = 0;
}

// Concurrent host-path calls per device (each context holds its staging
// buffers): enough for the 16 prefetch workers of the largest measured
// pipeline, which 4 contexts serialised.
constexpr int kCtxPerDevice = 16;

// Host-side byte moves of the host path (footprint staging into pinned
// memory, copy-out of results) are bound by one core's memory bandwidth;
// they are split over helper threads, fewer when several host-path calls run
// at once (prefetch workers already spread the work).
std::atomic<int> g_host_calls{0};

// Persistent helper threads for parallel_items: starting and joining up to 7
// std::threads, ~20 us each, for every ~24 MB chunk measured slower.
class Helpers {
 public:
  static Helpers& get() {
    static Helpers* h = new Helpers();  // leaked on purpose: its threads live until exit
    return *h;
  }
  // Runs `work` on the calling thread and on up to `extra` helpers; returns
  // once every helper that took part has finished it (helpers that had not
  // started by then never will).
  void run(int extra, const std::function<void()>& work) {
    auto job = std::make_shared<Job>();
    job->work = &work;
    job->pending = extra;
    {
      // the pool grows to the helpers every call in flight asks for (capped),
      // so concurrent calls (prefetch workers, split devices) each get theirs
      std::lock_guard<std::mutex> lk(mu_);
      outstanding_ += extra;
      while ((int)threads_.size() < std::min(outstanding_, kMaxHelpers)) threads_.emplace_back([this] { loop(); });
      for (int k = 0; k < extra; k++) queue_.push_back(job);
    }
    cv_.notify_all();
    work();
    int unclaimed = 0;
    {
      std::lock_guard<std::mutex> lk(mu_);
      outstanding_ -= extra;
      for (auto it = queue_.begin(); it != queue_.end();)
        if (*it == job) {
          it = queue_.erase(it);
          unclaimed++;
        } else {
          ++it;
        }
    }
    std::unique_lock<std::mutex> lk(job->mu);
    job->pending -= unclaimed;
    job->cv.wait(lk, [&] { return job->pending == 0; });
  }

 private:
  static constexpr int kMaxHelpers = 16;
  struct Job {
    const std::function<void()>* work = nullptr;
    int pending = 0;
    std::mutex mu;
    std::condition_variable cv;
  };
  void loop() {
    for (;;) {
      std::shared_ptr<Job> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !queue_.empty(); });
        job = queue_.front();
        queue_.pop_front();
      }
      (*job->work)();
      std::lock_guard<std::mutex> lk(job->mu);
      if (--job->pending == 0) job->cv.notify_all();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::shared_ptr<Job>> queue_;
  std::vector<std::thread> threads_;
  int outstanding_ = 0;  // helpers asked for by the calls in flight
};

// The CPUs this process may keep busy: the affinity mask, capped by a cgroup
// CPU quota (v2 cpu.max, v1 cpu.cfs_quota_us) -- a container's share, which
// the mask does not show: the GPU boxes give every process the whole
// machine's mask and a 16-CPU quota, and sizing helpers by the mask put
// 16 prefetch workers x 8 staging threads on 16 CPUs -- and by
// OMP_NUM_THREADS when the environment sets it above 1 (the boxes' per-GPU
// share; torchrun and similar launchers export 1 to every rank by default,
// which says nothing about the host's CPUs and is ignored).
// MXD_HOST_CPUS overrides all of it (tuning knobs).
int host_cpu_budget() {
  if (const char* e = std::getenv("MXD_HOST_CPUS"))
    if (std::atoi(e) > 0) return std::atoi(e);
  int n = (int)std::thread::hardware_concurrency();
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  auto cap = [&](double quota, double period) {
    if (quota > 0 && period > 0) n = std::min(n, std::max(1, (int)std::ceil(quota / period)));
  };
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    double period = 0;
    if (std::fscanf(f, "%31s %lf", q, &period) == 2 && std::strcmp(q, "max") != 0) cap(std::atof(q), period);
    std::fclose(f);
  } else if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
    double quota = -1, period = 0;
    if (std::fscanf(g, "%lf", &quota) != 1) quota = -1;
    std::fclose(g);
    if (FILE* h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (std::fscanf(h, "%lf", &period) != 1) period = 0;
      std::fclose(h);
    }
    cap(quota, period);
  }
  if (const char* e = std::getenv("OMP_NUM_THREADS")) {
    const int k = std::atoi(e);
    if (k > 1) n = std::min(n, k);
  }
  return std::max(1, n);
}

// dst[j] = src[j] / 255 in f32 (IEEE division: the bytes of the kernels'
// MXD_F32_DIV255 output and of the reference's astype(float32) / 255 for the
// same u8 value; multiplying by 1/255 differs for 126 of the 256 values).
// The f32 rows are written with streaming (non-temporal) stores from the
// first 32-byte boundary on: the batch is written once here and read by the
// consumer later, and ordinary stores would first read every destination
// line into the cache (the pass is bound by host memory traffic).
__attribute__((target("avx2"))) void div255_avx2(const uint8_t* src, float* dst, int64_t n) {
  const __m256 k = _mm256_set1_ps(255.0f);
  int64_t j = 0;
  for (; j < n && (reinterpret_cast<uintptr_t>(dst + j) & 31) != 0; j++) dst[j] = (float)src[j] / 255.0f;
  for (; j + 16 <= n; j += 16) {
    const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + j));
    _mm256_stream_ps(dst + j, _mm256_div_ps(_mm256_cvtepi32_ps(_mm256_cvtepu8_epi32(b)), k));
    _mm256_stream_ps(dst + j + 8, _mm256_div_ps(_mm256_cvtepi32_ps(_mm256_cvtepu8_epi32(_mm_srli_si128(b, 8))), k));
  }
  for (; j < n; j++) dst[j] = (float)src[j] / 255.0f;
}

void div255_row(const uint8_t* src, float* dst, int64_t n) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2) return div255_avx2(src, dst, n);
  for (int64_t j = 0; j < n; j++) dst[j] = (float)src[j] / 255.0f;
}

}  // namespace

void parallel_items(int32_t first, int32_t end, int64_t bytes, const std::function<void(int32_t)>& f) {
  const int32_t n = end - first;
  static const int hw = host_cpu_budget();
  int t = std::min<int64_t>({8, hw / std::max(1, g_host_calls.load()), n, bytes >> 20});
  if (t <= 1) {
    for (int32_t i = first; i < end; i++) f(i);
    return;
  }
  std::atomic<int32_t> next{first};
  const std::function<void()> work = [&] {
    for (int32_t i; (i = next.fetch_add(1)) < end;) f(i);
  };
  Helpers::get().run(t - 1, work);
}

namespace {

class HostPool {
 public:
  HostCtx* acquire(int32_t device) {
    std::unique_lock<std::mutex> lk(mu_);
    Dev& d = devs_[device];
    cv_.wait(lk, [&] { return !d.idle.empty() || (int)d.all.size() < kCtxPerDevice; });
    if (!d.idle.empty()) {
      HostCtx* c = d.idle.back();
      d.idle.pop_back();
      return c;
    }
    d.all.push_back(std::make_unique<HostCtx>());
    return d.all.back().get();
  }
  void release(int32_t device, HostCtx* c) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      devs_[device].idle.push_back(c);
    }
    cv_.notify_one();
  }
  // Frees the buffers of every idle context (streams stay).
  void trim() {
    std::lock_guard<std::mutex> lk(mu_);
    for (auto& kv : devs_) {
      DeviceGuard g(kv.first);
      for (HostCtx* c : kv.second.idle)
        for (Slot& s : c->slot) free_slot_buffers(s);
    }
  }

 private:
  struct Dev {
    std::vector<std::unique_ptr<HostCtx>> all;
    std::vector<HostCtx*> idle;
  };
  std::mutex mu_;
  std::condition_variable cv_;
  std::map<int32_t, Dev> devs_;
};

HostPool& host_pool() {
  static HostPool* p = new HostPool();
  return *p;
}

// Borrowed context, returned to the pool on scope exit.
struct CtxLease {
  int32_t device;
  HostCtx* ctx;
  explicit CtxLease(int32_t d) : device(d), ctx(host_pool().acquire(d)) {}
  ~CtxLease() { host_pool().release(device, ctx); }
};

// MXD_TUNE_HOST_STREAMS > 0: host-path slots share that many library
// streams per device (round robin as slots are first set up) instead of
// owning one each, so 16 prefetch workers do not spread their device calls
// over 32 streams when HIP maps a process's streams onto fewer hardware
// queues (GPU_MAX_HW_QUEUES, 4 by default).  Read when a slot is first set up.
int shared_stream(hipStream_t* out, int32_t n) {
  static std::mutex mu;
  static std::map<int, std::pair<std::vector<hipStream_t>, int64_t>> pools;
  int dev = 0;
  MXD_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto& pl = pools[dev];
  if ((int32_t)pl.first.size() < n) {
    hipStream_t st = nullptr;
    MXD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    pl.first.push_back(st);
    *out = st;
    return MXD_OK;
  }
  *out = pl.first[(size_t)(pl.second++ % (int64_t)pl.first.size())];
  return MXD_OK;
}

int init_slot(Slot& s) {
  if (!s.stream) {
    const int32_t shared = g_tune[MXD_TUNE_HOST_STREAMS].load();
    if (shared > 0) {
      if (int rc = shared_stream(&s.stream, shared)) return rc;
    } else {
      MXD_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    }
  }
  // the calling thread sleeps on the chunk's event instead of polling
  // (MXD_TUNE_HOST_WAIT 2: polling): with 16 prefetch workers on 16 cores the
  // polling waits took the cores the other workers' parsing and staging need
  // (JPEG device batch at 16 workers, C4 137 k -> 156-161 k img/s, C1
  // 176-192 k -> 205-208 k; profiles/r04/host_wait_ab.jsonl)
  if (!s.done)
    MXD_HIP(hipEventCreateWithFlags(
        &s.done, hipEventDisableTiming | (g_tune[MXD_TUNE_HOST_WAIT].load() == 2 ? 0 : hipEventBlockingSync)));
  return MXD_OK;
}

// Counts the call in (the helpers' share of the CPUs) and, on exit, into
// mxd_host_stats.
struct CallCount {
  int64_t n, t0 = now_ns();
  explicit CallCount(int64_t images) : n(images) { g_host_calls.fetch_add(1); }
  ~CallCount() {
    g_host_calls.fetch_sub(1);
    g_host_stats[0].fetch_add(1, std::memory_order_relaxed);
    g_host_stats[1].fetch_add(n, std::memory_order_relaxed);
    g_host_stats[2].fetch_add(now_ns() - t0, std::memory_order_relaxed);
  }
};

void waited(int64_t t0) { g_host_stats[3].fetch_add(now_ns() - t0, std::memory_order_relaxed); }

// On every exit (an error return included) the context goes back to the
// pool idle: no kernel of this call may still read its slot buffers or
// write the caller's destinations once the call has returned.
struct Drain {
  HostCtx& c;
  ~Drain() {
    const int64_t t0 = now_ns();
    for (Slot& sl : c.slot)
      if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    waited(t0);
  }
};

// Planning, per image.

// Raw source: the footprint of the crop window, staged or read in place.
int raw_plan_input(HostCall& c, int32_t i) {
  const mxd_image& im = c.images[i];
  const DevTable *xt = nullptr, *yt = nullptr;
  if (int rc = tables().get(c.device, im.src_w, im.resize_w, &xt, im.filter)) return rc;
  if (int rc = tables().get(c.device, im.src_h, im.resize_h, &yt, im.filter)) return rc;
  int32_t xl, xh, yl, yh;
  footprint(*xt, *yt, im, &xl, &xh, &yl, &yh);
  const int32_t ch = im.channels;
  const int32_t m = 16 / std::gcd(ch, 16);  // x0 * ch is a multiple of 16
  Stage& s = c.st[i];
  s.x0 = xl - xl % m;
  s.y0 = yl;
  s.rows = yh - yl + 1;
  const int64_t want = (int64_t)(xh + 1 - s.x0) * ch + 32;  // + the kernels' read-ahead inside a row
  s.copy = std::min<int64_t>((int64_t)(im.src_w - s.x0) * ch, want);
  s.pitch = (want + 15) & ~(int64_t)15;
  s.in_size = s.pitch * s.rows;
  s.src_pinned = host_pinned(im.src);
  // Page-locked sources are read in place by the kernel (PCIe reads): 2-D
  // DMA of short footprint rows measured 3.4x slower than one contiguous
  // copy of the same bytes (tools/pcie_probe.py).
  s.src_dev = s.src_pinned && !(g_policy.load() & MXD_POLICY_NO_ZERO_COPY) ? host_device_ptr(im.src) : nullptr;
  return MXD_OK;
}

// Where image i's result goes.  narrow_pct: the share of the images whose
// f32 results return narrow (host_path).  The host expands a narrow result
// with aligned f32 stores, so only an image whose destination and row stride
// are both 4-byte aligned is narrowed; any other returns f32 over the link.
int plan_output(HostCall& c, int32_t i, int32_t narrow_pct) {
  const mxd_image& im = c.images[i];
  Stage& s = c.st[i];
  s.out_row = (int64_t)im.crop_w * im.channels * (c.out_dtype == MXD_F32_DIV255 ? 4 : 1);
  s.dst_pinned = !c.dst_device && host_pinned(im.dst);
  s.dst_dev = s.dst_pinned && !(g_policy.load() & MXD_POLICY_NO_ZERO_COPY)
                  ? const_cast<uint8_t*>(host_device_ptr(im.dst)) : nullptr;
  s.narrow = c.out_dtype == MXD_F32_DIV255 && !c.dst_device && narrow_pct > 0 &&
             (narrow_pct == 100 || (i * narrow_pct) % 100 < narrow_pct) &&
             ((reinterpret_cast<uintptr_t>(im.dst) | (uintptr_t)im.dst_stride) & 3) == 0;
  if (s.narrow) s.dst_pinned = false, s.dst_dev = nullptr;  // staged, then expanded into place
  s.stage_row = s.narrow ? s.out_row / 4 : s.out_row;
  if (!c.dst_device && im.dst_stride < s.out_row)
    return fail(MXD_ERR_INVALID, "mxd: dst_stride smaller than an output row");
  return MXD_OK;
}

// Chunks of about kChunk staged bytes (at least one image each).  A JPEG
// whose entropy decode runs on the device stages only its compressed
// segments, and counts an eighth of its coefficient bytes (device memory):
// ~300 ImageNet-size files a chunk, so a 128-file batch is one entropy
// launch over the whole GPU rather than three of ~40 files on ~80 CUs
// (round 5).
// (at most 65535 images a chunk: the JPEG colour kernel puts one image per grid row)
constexpr int32_t kChunkImages = 65535;
// A mix call's one chunk stages every source of the call at once -- page-locked
// host memory, the device input and the u8 scratch rows of the whole call --
// so its staged bytes are bounded instead of cut.
constexpr int64_t kMixChunk = (int64_t)1 << 30;

int cut_chunks(HostCall& c) {
  constexpr int64_t kChunk = 24 << 20;
  auto size = [&](int32_t q) { return c.st[q].pending ? c.st[q].in_size / 8 : c.st[q].in_size; };
  // A mix call is one chunk: an image's partner must be on the device with it.
  // Its staging then overlaps no compute.
  if (c.ops.mixes) {
    int64_t bytes = 0;
    for (int32_t q = 0; q < c.n; q++) bytes += size(q);
    if (c.n > kChunkImages || bytes > kMixChunk)
      return fail(MXD_ERR_UNSUPPORTED, "mxd: a mix call from host sources is one chunk: at most " +
                                           std::to_string(kChunkImages) + " images and " +
                                           std::to_string(kMixChunk >> 20) + " MiB of staged sources (this call: " +
                                           std::to_string(c.n) + " images, " + std::to_string(bytes >> 20) + " MiB)");
    c.chunks.push_back({0, c.n});
    return MXD_OK;
  }
  for (int32_t i = 0; i < c.n;) {
    int32_t j = i;
    int64_t bytes = 0;
    while (j < c.n && j - i < kChunkImages && (j == i || bytes + size(j) <= kChunk)) {
      bytes += size(j);
      j++;
    }
    c.chunks.push_back({i, j});
    i = j;
  }
  return MXD_OK;
}

// The output side.

// Waits for chunk k and copies its staged results into place.
int copy_out(HostCall& c, int k) {
  Slot& sl = c.ctx->slot[k & 1];
  const int64_t t0 = now_ns();
  MXD_HIP(hipEventSynchronize(sl.done));
  waited(t0);
  c.pending[k & 1] = -1;
  if (sl.timed) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, sl.k0, sl.k1) == hipSuccess && ms > 0.0f) {
      g_device_stats[0].fetch_add(1, std::memory_order_relaxed);
      g_device_stats[1].fetch_add((int64_t)((double)ms * 1e6), std::memory_order_relaxed);
    }
    sl.timed = false;
  }
  if (sl.huff_err && *sl.huff_err) {
    *sl.huff_err = 0;
    return fail(MXD_ERR_DEVICE, "jpeg entropy decode: a job never received its predecessor's state");
  }
  if (c.dst_device) return MXD_OK;  // the kernel wrote the destinations
  const ChunkRange of = c.chunks[k];
  int64_t bytes = 0;
  for (int32_t i = of.first; i < of.end; i++) bytes += c.st[i].out_row * c.images[i].crop_h;
  parallel_items(of.first, of.end, bytes, [&](int32_t i) {
    const Stage& s = c.st[i];
    if (s.dst_pinned) return;  // DMA'd straight into place
    const mxd_image& im = c.images[i];
    uint8_t* d = static_cast<uint8_t*>(im.dst);
    const uint8_t* src = sl.pin_out + s.out_off;
    if (s.narrow) {
      for (int32_t r = 0; r < im.crop_h; r++)
        div255_row(src + (size_t)r * s.stage_row, reinterpret_cast<float*>(d + (size_t)r * im.dst_stride), s.stage_row);
      _mm_sfence();  // the streaming stores are visible before the call returns
    } else if (im.dst_stride == s.out_row) {
      std::memcpy(d, src, (size_t)s.out_row * im.crop_h);
    } else {
      for (int32_t r = 0; r < im.crop_h; r++)
        std::memcpy(d + (size_t)r * im.dst_stride, src + (size_t)r * s.out_row, s.out_row);
    }
  });
  return MXD_OK;
}

// Output offsets of the chunk (staged images first: one D2H covers them;
// directly DMA'd ones after them), then the slot's buffers, grown to the
// chunk.  c.zero_copy: the kernels read the staged inputs from the
// page-locked slot buffer and write results into its page-locked output
// buffer (no H2D / D2H DMA step in between).
int lay_out_outputs(HostCall& c) {
  Slot& sl = *c.sl;
  c.out_bytes = c.out_staged = 0;
  for (int pass = 0; pass < 2; pass++)
    for (int32_t i = c.cur.first; i < c.cur.end; i++) {
      Stage& s = c.st[i];
      if (s.dst_pinned != (pass == 1) || s.dst_dev) continue;
      s.out_off = c.out_bytes;
      // page-locked destinations back to back (one copy per contiguous run)
      const int64_t b = s.stage_row * c.images[i].crop_h;
      c.out_bytes += pass == 1 && (s.stage_row & 3) == 0 ? b : (b + 255) & ~(int64_t)255;
      if (pass == 0) c.out_staged = s.out_off + b;
    }
  if (int rc = grow_pinned(&sl.pin_in, &sl.pin_in_cap, c.in_bytes)) return rc;
  if (int rc = grow_device(&sl.dev_in, &sl.dev_in_cap, std::max(c.in_bytes, c.dev_in_bytes))) return rc;
  if (!c.dst_device) {
    if (int rc = grow_pinned(&sl.pin_out, &sl.pin_out_cap, c.out_bytes)) return rc;
    if (int rc = grow_device(&sl.dev_out, &sl.dev_out_cap, c.out_bytes)) return rc;
  }
  c.pin_in_dev = c.zero_copy ? host_device_ptr(sl.pin_in) : nullptr;
  c.pin_out_dev =
      c.zero_copy && !c.dst_device && sl.pin_out ? const_cast<uint8_t*>(host_device_ptr(sl.pin_out)) : nullptr;
  return MXD_OK;
}

// Each image's destination as the kernels see it: in place over PCIe, the
// slot's output buffer, or (device destinations) the caller's own.
void bind_destinations(HostCall& c) {
  uint8_t* out = c.pin_out_dev ? c.pin_out_dev : c.sl->dev_out;
  for (int32_t i = c.cur.first; i < c.cur.end; i++) {
    const Stage& s = c.st[i];
    mxd_image& d = c.dev_imgs[i - c.cur.first];
    if (s.dst_dev) {
      d.dst = s.dst_dev;
    } else if (!c.dst_device) {
      d.dst = out + s.out_off;
      d.dst_stride = s.stage_row;
    }
  }
}

// One resize launch per output dtype (a chunk mixes them only when a share
// of its images is narrowed).
int resize(HostCall& c) {
  const int32_t first = c.cur.first, cn = c.cur.end - first;
  bool mixed = false;
  for (int32_t i = first + 1; i < c.cur.end; i++) mixed = mixed || c.st[i].narrow != c.st[first].narrow;
  if (!mixed)
    return run_batch(c.dev_imgs.data(), cn, c.launch_dtype(first), c.device, c.sl->stream, c.where.data(),
                     c.ops.at(first));
  // (narrowing needs host destinations, a format, a colour or a tone device ones: never both)
  if (c.ops.any()) return fail(MXD_ERR_UNSUPPORTED, "mxd: narrow return within a formatted call");
  int rc = MXD_OK;
  for (int part = 0; part < 2 && rc == MXD_OK; part++) {
    std::vector<mxd_image> pi;
    std::vector<Stored> pw;
    for (int32_t j = 0; j < cn; j++)
      if (c.st[first + j].narrow == (part == 0)) {
        pi.push_back(c.dev_imgs[j]);
        pw.push_back(c.where[j]);
      }
    if (!pi.empty())
      rc = run_batch(pi.data(), (int32_t)pi.size(), part == 0 ? MXD_U8 : c.out_dtype, c.device, c.sl->stream, pw.data());
  }
  return rc;
}

// The chunk's results back to the host: the staged ones in one copy;
// page-locked destinations straight from the device.  Images packed back to
// back both here and in the destination (a batch tensor) go as one copy;
// strided ones as 2-D copies.
int enqueue_outputs(HostCall& c) {
  const Slot& sl = *c.sl;
  if (c.out_staged > 0 && !c.pin_out_dev)
    MXD_HIP(hipMemcpyAsync(sl.pin_out, sl.dev_out, c.out_staged, hipMemcpyDeviceToHost, sl.stream));
  for (int32_t i = c.cur.first; i < c.cur.end;) {
    const Stage& s = c.st[i];
    const mxd_image& im = c.images[i];
    if (!s.dst_pinned || s.dst_dev) {
      i++;
      continue;
    }
    if (im.dst_stride != s.out_row) {
      MXD_HIP(hipMemcpy2DAsync(im.dst, im.dst_stride, sl.dev_out + s.out_off, s.out_row, s.out_row, im.crop_h,
                               hipMemcpyDeviceToHost, sl.stream));
      i++;
      continue;
    }
    int32_t j = i + 1;
    int64_t run = s.out_row * im.crop_h;
    while (j < c.cur.end && c.st[j].dst_pinned && c.images[j].dst_stride == c.st[j].out_row &&
           static_cast<uint8_t*>(c.images[j].dst) == static_cast<uint8_t*>(im.dst) + run &&
           c.st[j].out_off == s.out_off + run) {
      run += c.st[j].out_row * c.images[j].crop_h;
      j++;
    }
    MXD_HIP(hipMemcpyAsync(im.dst, sl.dev_out + s.out_off, run, hipMemcpyDeviceToHost, sl.stream));
    i = j;
  }
  return MXD_OK;
}

// The raw-image source.

// Staged images first (one H2D covers them), page-locked ones that are
// DMA'd row by row after them.
void raw_lay_out(HostCall& c) {
  c.in_bytes = c.in_staged = c.dev_in_bytes = 0;
  for (int pass = 0; pass < 2; pass++)
    for (int32_t i = c.cur.first; i < c.cur.end; i++) {
      Stage& s = c.st[i];
      if (s.src_pinned != (pass == 1) || s.src_dev) continue;
      s.in_off = c.in_bytes;
      c.in_bytes += (s.in_size + 255) & ~(int64_t)255;
      if (pass == 0) c.in_staged = s.in_off + s.in_size;
    }
  c.zero_copy = !(g_policy.load() & MXD_POLICY_NO_ZERO_COPY);
}

void raw_stage(HostCall& c, int32_t i) {
  const mxd_image& im = c.images[i];
  const Stage& s = c.st[i];
  if (s.src_pinned) return;
  uint8_t* stage = c.sl->pin_in + s.in_off;
  const uint8_t* from = im.src + (int64_t)s.y0 * im.src_stride + (int64_t)s.x0 * im.channels;
  for (int32_t r = 0; r < s.rows; r++) std::memcpy(stage + r * s.pitch, from + (int64_t)r * im.src_stride, s.copy);
}

void raw_bind(HostCall& c) {
  const uint8_t* in = c.pin_in_dev ? c.pin_in_dev : c.sl->dev_in;
  for (int32_t i = c.cur.first; i < c.cur.end; i++) {
    const mxd_image& im = c.images[i];
    const Stage& s = c.st[i];
    mxd_image& d = c.dev_imgs[i - c.cur.first];
    if (s.src_dev) {
      // zero copy: the footprint rows in place in the page-locked source
      d.src = s.src_dev + (int64_t)s.y0 * im.src_stride + (int64_t)s.x0 * im.channels;
      c.where[i - c.cur.first] = Stored{d.src, im.src_stride, s.x0, s.y0, s.rows};
    } else {
      d.src = in + s.in_off;  // checked by validate() only; `where` says what is stored
      c.where[i - c.cur.first] = Stored{d.src, s.pitch, s.x0, s.y0, s.rows};
    }
    d.src_stride = std::max<int64_t>(s.pitch, (int64_t)im.src_w * im.channels);
  }
}

// 2-D copies of the page-locked sources that are not read in place.
int raw_enqueue_copies(HostCall& c) {
  for (int32_t i = c.cur.first; i < c.cur.end; i++) {
    const Stage& s = c.st[i];
    if (!s.src_pinned || s.src_dev) continue;
    const mxd_image& im = c.images[i];
    const uint8_t* from = im.src + (int64_t)s.y0 * im.src_stride + (int64_t)s.x0 * im.channels;
    MXD_HIP(hipMemcpy2DAsync(c.sl->dev_in + s.in_off, s.pitch, from, im.src_stride, s.copy, s.rows,
                             hipMemcpyHostToDevice, c.sl->stream));
  }
  return MXD_OK;
}

}  // namespace

// The host path: host sources, results to host (dst_device false: D2H +
// copy-out) or straight into device destinations (dst_device true).
// jpeg != nullptr: images[i] is jpeg[i] as an mxd_image (3 channels, the
// window as the source); its "source" is the image's coefficients, and the
// chunk's kernels first decode them into dev_mid.  Every step is common to
// both sources unless it picks a raw_* or a jpeg_* function.
int host_path(const mxd_image* images, int32_t n, int32_t out_dtype, int32_t device, bool dst_device,
              const mxd_jpeg_image* jpeg, PostOps ops) {
  if (n < 0 || (n > 0 && !images)) return fail(MXD_ERR_INVALID, "mxd: bad image array");
  // the stages behind the resize write device destinations only
  const char* const call = ops.mixes      ? "mix"
                           : ops.warps    ? "warp"
                           : ops.enhances ? "enhance"
                           : ops.tones    ? "tone"
                                          : "colour";
  if (!dst_device && ops.per_image())
    return fail(MXD_ERR_UNSUPPORTED, std::string("mxd: ") + call + " calls need device destinations");
  mxd_out_format f32_fmt;
  if (int rc = prepare_post_ops(images, n, &ops, &out_dtype, &f32_fmt)) return rc;
  const mxd_out_format* const fmt = ops.fmt;
  if (fmt) {
    // formatted results go to device destinations only; the launches are planned as u8 ones
    if (!dst_device) return fail(MXD_ERR_UNSUPPORTED, "mxd: formatted outputs need device destinations");
    out_dtype = MXD_U8;
  }
  if (out_dtype != MXD_U8 && out_dtype != MXD_F32_DIV255) return fail(MXD_ERR_INVALID, "mxd: bad out_dtype");
  if (n == 0) return MXD_OK;
  for (int32_t i = 0; i < n; i++)
    if (int rc = validate(images[i], i)) return rc;
  if (fmt)
    if (int rc = fmt_validate_images(images, n, *fmt)) return rc;
  if (int rc = check_device(device)) return rc;
  // Narrow return (round 6): f32 results bound for host memory cross the link
  // as the u8 bytes the same kernels compute before their exact /255 (the
  // f32 output is LUT[u8] bit for bit), and the host expands them while it
  // copies them into place -- a quarter of the link bytes (150 instead of 602
  // KB per 224x224 RGB image), for page-locked destinations too (instead of
  // the kernels writing f32 into them over PCIe: the pipeline's host batches
  // are page-locked, and that write was the host-ending C4 bound, 43 GB/s).
  // MXD_TUNE_F32_LINK 1: the f32 results cross the link; 2..99: that
  // percentage of the images is narrowed, spread evenly, the rest cross the
  // link as f32 (the link and the host's writes share the work).
  const int32_t link_knob = g_tune[MXD_TUNE_F32_LINK].load();
  const int32_t narrow_pct = link_knob == 1 ? 0 : link_knob >= 2 && link_knob < 100 ? link_knob : 100;
  DeviceGuard g(device);
  CallCount call_count(n);
  HostCall c;
  c.images = images, c.n = n, c.out_dtype = out_dtype, c.device = device, c.dst_device = dst_device, c.jpeg = jpeg;
  c.ops = ops;

  // Plan: inputs and outputs per image, then the chunks.
  c.st.resize(n);
  int64_t nnarrow = 0;
  for (int32_t i = 0; i < n; i++) {
    if (int rc = jpeg ? jpeg_plan_input(c, i) : raw_plan_input(c, i)) return rc;
    if (int rc = plan_output(c, i, narrow_pct)) return rc;
    nnarrow += c.st[i].narrow ? 1 : 0;
  }
  if (nnarrow) g_narrow_images.fetch_add(nnarrow, std::memory_order_relaxed);
  if (int rc = cut_chunks(c)) return rc;

  CtxLease lease(device);
  c.ctx = lease.ctx;
  Drain drain{*c.ctx};
  for (Slot& sl : c.ctx->slot)
    if (int rc = init_slot(sl)) return rc;

  for (int k = 0; k < (int)c.chunks.size(); k++) {
    c.cur = c.chunks[k];
    c.sl = &c.ctx->slot[k & 1];
    Slot& sl = *c.sl;
    if (c.pending[k & 1] >= 0)
      if (int rc = copy_out(c, c.pending[k & 1])) return rc;

    // Lay out the chunk in the slot's buffers, stage it, bind every image.
    if (jpeg) {
      if (int rc = jpeg_lay_out(c)) return rc;
    } else {
      raw_lay_out(c);
    }
    if (int rc = lay_out_outputs(c)) return rc;
    c.dev_imgs.assign(images + c.cur.first, images + c.cur.end);
    c.where.assign(c.cur.end - c.cur.first, Stored{});
    parallel_items(c.cur.first, c.cur.end, c.in_staged, [&](int32_t i) { jpeg ? jpeg_stage(c, i) : raw_stage(c, i); });
    bind_destinations(c);
    if (jpeg) {
      if (int rc = jpeg_bind(c)) return rc;
    } else {
      raw_bind(c);
    }

    // Enqueue: input copies, the source's kernels (k0 in front of the first
    // kernel when timed), the resize, k1, output copies, done.
    if (c.in_staged > 0 && !c.pin_in_dev)
      MXD_HIP(hipMemcpyAsync(sl.dev_in, sl.pin_in, c.in_staged, hipMemcpyHostToDevice, sl.stream));
    sl.timed = g_tune[MXD_TUNE_DEVICE_TIMING].load() == 1;
    if (sl.timed && !sl.k0) MXD_HIP(hipEventCreate(&sl.k0));
    if (sl.timed && !sl.k1) MXD_HIP(hipEventCreate(&sl.k1));
    if (!jpeg)
      if (int rc = raw_enqueue_copies(c)) return rc;
    if (sl.timed) MXD_HIP(hipEventRecord(sl.k0, sl.stream));
    if (jpeg)
      if (int rc = jpeg_enqueue(c)) return rc;
    if (int rc = resize(c)) {
      sl.timed = false;  // (k1 not recorded for this chunk)
      return rc;
    }
    if (sl.timed) MXD_HIP(hipEventRecord(sl.k1, sl.stream));
    if (!dst_device)
      if (int rc = enqueue_outputs(c)) return rc;
    MXD_HIP(hipEventRecord(sl.done, sl.stream));
    c.pending[k & 1] = k;

    // results of the previous chunk, while this one runs
    const int prev = c.pending[(k + 1) & 1];
    if (prev >= 0)
      if (int rc = copy_out(c, prev)) return rc;
  }
  for (int k = 0; k < 2; k++)
    if (c.pending[k] >= 0)
      if (int rc = copy_out(c, c.pending[k])) return rc;
  return MXD_OK;
}

void host_trim() { host_pool().trim(); }

// Pixel maps of host images through a borrowed context (mxd_pixmap_host).
int pixmap_host(const mxd_pixmap* images, int32_t n, int32_t op, int32_t device) {
  if (n < 0 || (n > 0 && !images)) return fail(MXD_ERR_INVALID, "mxd: bad image array");
  if (n == 0) return MXD_OK;
  for (int32_t i = 0; i < n; i++)
    if (int rc = pix_validate(images[i], op, i)) return rc;
  if (int rc = check_device(device)) return rc;
  DeviceGuard g(device);
  CtxLease lease(device);
  Slot& ctx = lease.ctx->slot[0];
  if (int rc = init_slot(ctx)) return rc;
  std::vector<size_t> in_off(n), out_off(n);
  std::vector<int64_t> in_pitch(n), out_pitch(n);
  size_t in_bytes = 0, out_bytes = 0;
  for (int32_t i = 0; i < n; i++) {
    const mxd_pixmap& im = images[i];
    const int64_t oc = op == MXD_AFFINE ? im.channels : 1;
    in_pitch[i] = ((int64_t)im.src_w * im.channels + 15) & ~(int64_t)15;
    out_pitch[i] = ((int64_t)im.dst_w * oc + 15) & ~(int64_t)15;
    in_off[i] = in_bytes;
    in_bytes += ((size_t)in_pitch[i] * im.src_h + 255) & ~(size_t)255;
    out_off[i] = out_bytes;
    out_bytes += ((size_t)out_pitch[i] * im.dst_h + 255) & ~(size_t)255;
  }
  if (int rc = grow_pinned(&ctx.pin_in, &ctx.pin_in_cap, in_bytes)) return rc;
  if (int rc = grow_pinned(&ctx.pin_out, &ctx.pin_out_cap, out_bytes)) return rc;
  if (int rc = grow_device(&ctx.dev_in, &ctx.dev_in_cap, in_bytes)) return rc;
  if (int rc = grow_device(&ctx.dev_out, &ctx.dev_out_cap, out_bytes)) return rc;
  std::vector<mxd_pixmap> dev_imgs(images, images + n);
  for (int32_t i = 0; i < n; i++) {
    const mxd_pixmap& im = images[i];
    const size_t row = (size_t)im.src_w * im.channels;
    uint8_t* stage = ctx.pin_in + in_off[i];
    for (int32_t r = 0; r < im.src_h; r++)
      std::memcpy(stage + (size_t)r * in_pitch[i], im.src + (size_t)r * im.src_stride, row);
    dev_imgs[i].src = ctx.dev_in + in_off[i];
    dev_imgs[i].src_stride = in_pitch[i];
    dev_imgs[i].dst = ctx.dev_out + out_off[i];
    dev_imgs[i].dst_stride = out_pitch[i];
  }
  MXD_HIP(hipMemcpyAsync(ctx.dev_in, ctx.pin_in, in_bytes, hipMemcpyHostToDevice, ctx.stream));
  if (int rc = run_pixmap(dev_imgs.data(), n, op, device, ctx.stream)) return rc;
  MXD_HIP(hipMemcpyAsync(ctx.pin_out, ctx.dev_out, out_bytes, hipMemcpyDeviceToHost, ctx.stream));
  MXD_HIP(hipStreamSynchronize(ctx.stream));
  for (int32_t i = 0; i < n; i++) {
    const mxd_pixmap& im = images[i];
    const size_t row = (size_t)im.dst_w * (op == MXD_AFFINE ? im.channels : 1);
    uint8_t* d = static_cast<uint8_t*>(im.dst);
    const uint8_t* s = ctx.pin_out + out_off[i];
    for (int32_t r = 0; r < im.dst_h; r++) std::memcpy(d + (size_t)r * im.dst_stride, s + (size_t)r * out_pitch[i], row);
  }
  return MXD_OK;
}


}  // namespace capi
}  // namespace mxd
