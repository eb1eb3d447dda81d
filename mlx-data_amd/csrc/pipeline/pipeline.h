// pipeline.h -- the mlx-data Buffer/Stream operator surface for the image
// path, with the pixel work of image_resize_smallest_side / image_resize /
// image_center_crop / image_random_crop / image_random_h_flip deferred to the
// batch and executed by the fused gfx950 kernel through the C ABI
// (include/mxd_amd.h).
//
// Mirrors (semantics, error conditions, RNG draw order) of mlx-data 0.2.0:
//   Array / batch         mlx/data/Array.{h,cpp} (batch :465-498, sub :544-583)
//   Sample, check_key     mlx/data/Sample.{h,cpp}:13,18-29
//   Op / KeyTransformOp   mlx/data/op/{Op,KeyTransform}.{h,cpp}
//   image ops             mlx/data/op/ImageTransform.cpp:22-158,317-332
//   LoadImage             mlx/data/op/LoadImage.cpp:23-48
//   buffers               mlx/data/buffer/{FromVector,Perm,Shuffle,Transform,Batch}.cpp
//   streams               mlx/data/stream/{FromBuffer,Transform,Batch,Prefetch,OrderedPrefetch}.cpp
//   state                 mlx/data/core/State.cpp:9-22
//   merge_batch           mlx/data/core/Utils.cpp:209-252, BatchShape.cpp:26-66
#pragma once

#include <array>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <queue>
#include <random>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "mxd_amd.h"

namespace mxd {
namespace pipe {

// Same order as mlx::data::ArrayType; Float16 and BFloat16 (image_normalize's
// outputs) are appended, so the reference's order stays a prefix.
enum class DType { Any, UInt8, Int8, Int32, Int64, Float, Double, Float16, BFloat16 };
int64_t itemsize(DType t);

class Array;

// An entropy-decoded JPEG (mxd_jpeg_coefs_decode): load_image's output when
// the device finish is on (set_device_decode).  Its pixels come from the host
// finish on first direct access, or from the GPU finish inside the batch
// launch that resizes / crops it (mxd_jpeg_resize_crop_*); the bytes are the
// same either way.
struct JpegSource;

// image_normalize's output format (mxd_out_format without the strides): for a
// result byte q of channel c the element is ((float)q / 255 - mean[c]) /
// std[c] in float32 operations (q / 255 alone when !normalize), converted to
// `elem` (round to nearest even), written pixel-interleaved or as channel
// planes.
struct OutFormat {
  int32_t elem = 0;    // mxd_elem: 0 float32, 1 float16, 2 bfloat16
  int32_t layout = 0;  // mxd_layout: 0 HWC, 1 CHW
  bool normalize = false;
  std::array<float, 4> mean{{0, 0, 0, 0}}, std{{1, 1, 1, 1}};
  bool operator==(const OutFormat& o) const {
    return elem == o.elem && layout == o.layout && normalize == o.normalize &&
           (!normalize || (mean == o.mean && std == o.std));
  }
  bool operator!=(const OutFormat& o) const { return !(*this == o); }
  DType type() const { return elem == 0 ? DType::Float : elem == 1 ? DType::Float16 : DType::BFloat16; }
  bool chw() const { return layout == 1; }
};

// Pixel work that has not run yet: take the window (sx, sy, sw, sh) of `src`,
// resize it to resize_w x resize_h (identity when equal), keep the crop window
// of that, mirror it if `flip`.  The output is `crop_h x crop_w x C` uint8.
// It materialises on the GPU -- one launch for a whole batch when the batch
// node sees plans, one launch per image when something reads it directly.
struct ImagePlan {
  std::shared_ptr<Array> src;  // (H, W, C) uint8, materialised
  int64_t sx = 0, sy = 0, sw = 0, sh = 0;
  int64_t resize_w = 0, resize_h = 0;
  int64_t crop_x = 0, crop_y = 0, crop_w = 0, crop_h = 0;
  bool flip = false;
  // Went through core::image::resize (stbir): 4-channel images are then
  // alpha-weighted (STBIR_RGBA); crops and mirrors alone never are.
  bool resampled = false;
  // mxd_filter of the pending resize (0 = triangle, the reference's).  One
  // plan holds one resize: a second one materialises the first.
  int filter = 0;
  // image_to_float: the kernel writes float32 q / 255 (MXD_F32_DIV255)
  // instead of the uint8 q; the array's type is then Float.
  bool f32 = false;
  // image_normalize: the launch writes `out`'s elements instead
  // (mxd_*_to_device_fmt); the array's type is out.type() and, with CHW, its
  // shape (C, crop_h, crop_w).
  bool formatted = false;
  OutFormat out;
  // image_color_twist / image_color_matrix / image_random_color_twist: the
  // launch maps every result pixel through mxd_color `color` (row-major 3 x 4,
  // offsets in byte units) before the output form above.  A pointwise map:
  // crops and mirrors still compose on the plan; a resize or a second colour
  // op materialises the first.
  bool colored = false;
  std::array<float, 12> color{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  // image_posterize / _solarize / _autocontrast / _equalize / _contrast: the
  // launch looks every result byte up in the table of mxd_tone {tone_op,
  // tone_arg, tone_factor} before the colour map and the output form above.
  // Mirrors compose after every tone op; crops after the pointwise ones
  // (posterize, solarize) only: the others' statistics are those of the
  // window the op saw, so a crop materialises them first, as a resize or a
  // second tone op (or a tone op on a coloured plan: tone runs before colour)
  // materialises any.
  bool toned = false;
  int32_t tone_op = 0, tone_arg = 0;
  float tone_factor = 0.0f;
  // image_affine / _shear / _translate / _affine_rotate and their random
  // forms: the launch warps the u8 RGB result of the geometry above (mxd_warp
  // {warp_mode, warp_fill, warp_m}: Pillow's Image.transform(AFFINE)) before
  // the tone op, the colour map and the output form, which compose after it.
  // A warp op on a plan already warped, toned or coloured materialises it
  // first, as any crop, flip, resize or image_rotate after a warp does.
  bool warped = false;
  int32_t warp_mode = 0;
  std::array<uint8_t, 4> warp_fill{{0, 0, 0, 0}};
  std::array<double, 6> warp_m{{1, 0, 0, 0, 1, 0}};
  // image_sharpness / _color / _brightness and their random forms: the launch
  // applies mxd_enhance {enhance_op, enhance_factor} (Pillow's ImageEnhance)
  // to the u8 RGB result of the geometry and the warp above, before the tone
  // op, the colour map and the output form, which compose after it.  A flip
  // composes after every enhance op and a crop after COLOR and BRIGHTNESS (they
  // are pointwise, and SMOOTH is symmetric); a crop after SHARPNESS, whose
  // copied ring is the uncropped window's, a resize, image_rotate, a warp op
  // or a second enhance op materialises the plan first, as an enhance op on a
  // plan already toned or coloured does.
  bool enhanced = false;
  int32_t enhance_op = 0;
  float enhance_factor = 1.0f;
  int64_t channels() const;
};

class Array {
 public:
  Array(DType type, std::vector<int64_t> shape);                      // zero-initialised storage
  Array(DType type, std::vector<int64_t> shape, std::shared_ptr<void> data);
  // Device-resident storage (a batch made with batch(..., device=d)):
  // data() is then a device pointer on `device`.
  Array(DType type, std::vector<int64_t> shape, std::shared_ptr<void> data, int device);
  explicit Array(std::shared_ptr<const ImagePlan> plan);              // lazy image
  Array(std::shared_ptr<const JpegSource> jpeg, int64_t height, int64_t width);  // lazy decode, (H, W, 3)

  DType type() const { return type_; }
  const std::vector<int64_t>& shape() const { return shape_; }
  int64_t shape(int d) const;
  int ndim() const { return (int)shape_.size(); }
  int64_t size() const;
  int64_t nbytes() const { return size() * itemsize(type_); }
  // Materialises a pending image plan (one GPU launch) on first use.
  void* data() const;
  const std::shared_ptr<const ImagePlan>& plan() const { return plan_; }
  bool pending() const;
  // The entropy-decoded JPEG of a lazy decode not materialised yet, else null.
  std::shared_ptr<const JpegSource> jpeg() const;
  // -1: host memory; else the HIP device holding data().
  int device() const { return device_; }

 private:
  DType type_;
  std::vector<int64_t> shape_;
  mutable std::shared_ptr<void> data_;
  std::shared_ptr<const ImagePlan> plan_;
  mutable std::shared_ptr<const JpegSource> jpeg_;
  int device_ = -1;
  mutable std::mutex mu_;
};

using Sample = std::unordered_map<std::string, std::shared_ptr<Array>>;

std::shared_ptr<Array> check_key(const Sample& s, const std::string& key);

// Devices the fused kernel may use (default: all visible).  With several,
// one batch is split into contiguous slices, one per device, each launched
// from its own host thread (the reference's shard / partition analogue,
// op/Shard.cpp:11-20, stream/Partition.cpp:23-35); outputs land at the same
// offsets, so the batch is identical to a single-device one.
void set_devices(const std::vector<int>& devices);
std::vector<int> devices();
// How run_host splits a batch of n images over ndev devices (pipeline.cpp).
constexpr int64_t kMinSliceImages = 64;
struct Slice {
  int64_t device;      // index into devices()
  int64_t begin, end;  // images [begin, end) of the batch
};
std::vector<Slice> split_batch(int64_t n, int64_t ndev, uint64_t first);

// load_image's JPEG route: on (the default when a device is visible), only
// the entropy decode runs in load_image and the GPU finishes the decode inside
// the batch launch; off, load_image decodes whole on the
// host.  Identical bytes either way.
void set_device_decode(bool on);
// With the device decode on: the Huffman decode too runs on the GPU for the
// files it covers (mxd_jpeg_coefs_parse; default on).  Off: the host
// entropy-decodes every file (round 3's split).
void set_device_entropy(bool on);
bool device_entropy();
bool device_decode();
// Bytes the device batch pool holds for `device` (idle and pending blocks).
size_t device_pool_bytes(int device);
// Per-device batch calls made (fused launches, one per device slice) and the
// JPEG images they carried since the last reset (diagnostics, tests).
std::pair<int64_t, int64_t> run_on_stats(bool reset);
std::vector<int64_t> pipe_stats(bool reset);  // diagnostics: see pipeline.cpp g_pipe_ns

// ---------------------------------------------------------------- state
struct State {
  std::mt19937 gen;
  int64_t version = 0;
};
void set_state(int64_t seed);
std::shared_ptr<State> get_state();

// ---------------------------------------------------------------- ops
class Op {
 public:
  virtual ~Op() = default;
  virtual Sample apply(const Sample& sample) const = 0;
};

class KeyTransformOp : public Op {
 public:
  KeyTransformOp(std::string ikey, std::string okey) : ikey_(std::move(ikey)), okey_(std::move(okey)) {}
  Sample apply(const Sample& sample) const override;
  virtual std::shared_ptr<Array> apply_key(const std::shared_ptr<Array>& x) const = 0;

 protected:
  std::string ikey_, okey_;
};

class KeyTransform : public KeyTransformOp {
 public:
  using Fn = std::function<std::shared_ptr<Array>(const std::shared_ptr<Array>&)>;
  KeyTransform(std::string ikey, Fn fn, std::string okey) : KeyTransformOp(std::move(ikey), std::move(okey)), fn_(std::move(fn)) {}
  std::shared_ptr<Array> apply_key(const std::shared_ptr<Array>& x) const override { return fn_(x); }

 private:
  Fn fn_;
};

class ImageOp : public KeyTransformOp {
 public:
  using KeyTransformOp::KeyTransformOp;
  std::shared_ptr<Array> apply_key(const std::shared_ptr<Array>& x) const override;
  virtual std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const = 0;
  // (F, H, W, C) video: op/ImageTransform.cpp:33-70 -- apply_image per frame,
  // every frame the size of the first; pending frame plans run as one batched
  // launch writing straight into the result.
  virtual std::shared_ptr<Array> apply_video(const std::shared_ptr<Array>& video) const;
};

// Frame i of a materialised (F, H, W, C) video, sharing its storage.
std::shared_ptr<Array> video_frame(const std::shared_ptr<Array>& video, int64_t i);
// Stacks per-frame results (pending plans in one launch) into (F, h, w, c).
std::shared_ptr<Array> stack_frames(const std::vector<std::shared_ptr<Array>>& frames);

// The resize ops' `filter` argument: "triangle" (the reference's, the
// default), "catmullrom" (PIL BICUBIC / torch bicubic), "mitchell",
// "cubicbspline" -> mxd_filter.  Any other name: std::invalid_argument
// (Python: ValueError) naming the four.
int parse_filter(const std::string& name);
const char* filter_name(int filter);

class ImageResizeSmallestSide : public ImageOp {
 public:
  ImageResizeSmallestSide(std::string ikey, int64_t size, std::string okey, int filter = 0)
      : ImageOp(std::move(ikey), std::move(okey)), size_(size), filter_(filter) {}
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;

 private:
  int64_t size_;
  int filter_;
};

class ImageResize : public ImageOp {
 public:
  ImageResize(std::string ikey, int64_t w, int64_t h, std::string okey, int filter = 0)
      : ImageOp(std::move(ikey), std::move(okey)), w_(w), h_(h), filter_(filter) {}
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;

 private:
  int64_t w_, h_;
  int filter_;
};

class ImageCenterCrop : public ImageOp {
 public:
  ImageCenterCrop(std::string ikey, int64_t w, int64_t h, std::string okey)
      : ImageOp(std::move(ikey), std::move(okey)), w_(w), h_(h) {}
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;

 private:
  int64_t w_, h_;
};

class ImageRandomCrop : public ImageOp {
 public:
  ImageRandomCrop(std::string ikey, int64_t w, int64_t h, std::string okey)
      : ImageOp(std::move(ikey), std::move(okey)), w_(w), h_(h) {}
  std::shared_ptr<Array> apply_video(const std::shared_ptr<Array>& video) const override;
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;

 private:
  int64_t w_, h_;
};

class ImageRandomHFlip : public ImageOp {
 public:
  ImageRandomHFlip(std::string ikey, float prob, std::string okey)
      : ImageOp(std::move(ikey), std::move(okey)), prob_(prob) {}
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;
  std::shared_ptr<Array> apply_video(const std::shared_ptr<Array>& video) const override;

 private:
  float prob_;
};

// Fused normalize: the reference's post-batch
// `key_transform(key, lambda x: x.astype("float32") / 255)`
// (benchmarks/comparative/caltech101/mlx_data.py:34,46) as an image op ahead
// of batch.  A pending image (resize / crop / mirror not run yet) only
// records it, so batch writes the float32 tensor from the same launch; a
// materialised uint8 image is converted by one identity launch.  Values are
// exactly float(q) / 255.0f.  UInt8 input only ("image must be of type
// UInt8", core/image/ImageTransform.cpp:17-21).
class ImageToFloat : public ImageOp {
 public:
  ImageToFloat(std::string ikey, std::string okey) : ImageOp(std::move(ikey), std::move(okey)) {}
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;
};

// Fused normalise / cast / layout (an addition to the reference's surface,
// like ImageToFloat): the reference's post-batch
// `((x.astype("float32") / 255) - mean) / std`, cast to float16 / bfloat16 and
// transposed to channels-first if asked, as an image op ahead of batch.  It
// only marks the pending plan; batch then writes the final tensor from the
// resize launch.  mean / std: empty (q / 255 only), one value, or one per
// channel (checked against the image when the op is applied).  (F, H, W, C)
// videos work with HWC; CHW on one throws.
class ImageNormalize : public ImageOp {
 public:
  ImageNormalize(std::string ikey, std::vector<float> mean, std::vector<float> std, const std::string& dtype,
                 const std::string& layout, std::string okey);
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;
  std::shared_ptr<Array> apply_video(const std::shared_ptr<Array>& video) const override;

 private:
  std::vector<float> mean_, std_;
  OutFormat fmt_;
};

// Per-image colour transform (an addition to the reference's surface): a
// 3 x 4 affine map of the RGB result bytes, rounded and clamped back to bytes
// (DESIGN.md section 2), fused into the batch launch.  The op only marks the
// pending plan.  RGB images only: "image_color_twist: image must have 3
// channels" otherwise.  `matrix`: row-major 3 x 4, offsets in byte units.
class ImageColorMatrix : public ImageOp {
 public:
  ImageColorMatrix(std::string ikey, const std::array<float, 12>& matrix, std::string okey);
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;

 private:
  std::array<float, 12> m_;
};

// brightness, fixed-centre (0.5) contrast, saturation, hue (degrees):
// mxd_color_twist_matrix's matrix.  Negative or non-finite factors throw
// std::invalid_argument.
std::array<float, 12> color_twist(double brightness, double contrast, double saturation, double hue);

// Each factor drawn per image from its (lo, hi) range with one
// std::uniform_real_distribution<double> draw from the thread's State
// generator, in the order brightness, contrast, saturation, hue; a factor
// without a range draws nothing and stays at its default.  A video draws once
// for all its frames.
class ImageRandomColorTwist : public ImageOp {
 public:
  using Range = std::pair<double, double>;
  // has[k]: range[k] is given (k: brightness, contrast, saturation, hue)
  ImageRandomColorTwist(std::string ikey, const std::array<bool, 4>& has, const std::array<Range, 4>& range,
                        std::string okey);
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;
  std::shared_ptr<Array> apply_video(const std::shared_ptr<Array>& video) const override;

 private:
  std::array<float, 12> draw() const;
  std::array<bool, 4> has_;
  std::array<Range, 4> range_;
};

// Per-image tone operations (an addition to the reference's surface):
// Pillow's posterize, solarize, autocontrast, equalize and mean-grey contrast
// of the RGB result bytes, bit for bit, fused into the
// batch launch.  The op only marks the pending plan.  RGB images only:
// "image_equalize: image must have 3 channels, not N" otherwise.  Bad
// arguments throw std::invalid_argument from the constructor.
class ImageTone : public ImageOp {
 public:
  // op: mxd_tone_op; arg: posterize's bits / solarize's threshold; factor: contrast's
  ImageTone(std::string ikey, int32_t op, int64_t arg, double factor, std::string okey);
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;

 private:
  int32_t op_, arg_;
  float factor_;
};
// "posterize", ... of an mxd_tone_op (the op is image_<name>).
const char* tone_name(int32_t op);

// Per-image affine warps (an addition to the reference's surface): Pillow's
// Image.transform(size, AFFINE, matrix, resample, fillcolor=fill) and
// Image.rotate(angle, resample, fillcolor=fill) of the RGB result bytes, bit
// for bit, fused into the batch launch.  The op only
// marks the pending plan; the rotate matrix needs the image's size and is
// made when the op is applied.  RGB images only: "image_shear: image must
// have 3 channels, not N" otherwise.  Bad arguments throw
// std::invalid_argument from the constructors; a matrix outside the bound of
// the C calls throws their message when the op is applied.
class ImageAffine : public ImageOp {
 public:
  enum Kind { kMatrix = 0, kShear = 1, kTranslate = 2, kRotate = 3 };
  using Range = std::pair<double, double>;
  // v: the six entries (kMatrix), x and y (kShear, kTranslate: pixels), the
  // angle in degrees (kRotate).  mode: mxd_warp_mode.  fill: r, g, b in 0..255.
  ImageAffine(std::string ikey, Kind kind, const std::vector<double>& v, int32_t mode,
              const std::array<int64_t, 3>& fill, std::string okey);
  // The random forms: one uniform double per given range from the thread's
  // generator, x then y (kRotate: has[0] and range[0], the angle); a range
  // that is not given draws nothing and leaves 0.  A video draws once.
  ImageAffine(std::string ikey, Kind kind, const std::array<bool, 2>& has, const std::array<Range, 2>& range,
              int32_t mode, const std::array<int64_t, 3>& fill, std::string okey);
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;
  std::shared_ptr<Array> apply_video(const std::shared_ptr<Array>& video) const override;

 private:
  std::string name() const;
  std::vector<double> params() const;  // the fixed ones, or a draw
  std::shared_ptr<Array> mark(const std::shared_ptr<Array>& img, const std::vector<double>& v) const;
  Kind kind_;
  bool random_;
  std::vector<double> v_;
  std::array<bool, 2> has_{{false, false}};
  std::array<Range, 2> range_{};
  int32_t mode_;
  std::array<uint8_t, 4> fill_{{0, 0, 0, 0}};
};
// "nearest" / "bilinear" -> mxd_warp_mode (std::invalid_argument otherwise) and back.
int32_t parse_resample(const std::string& op, const std::string& name);
const char* resample_name(int32_t mode);
// Pillow's Image.rotate matrix for expand=False about (w / 2, h / 2).
std::array<double, 6> affine_rotate_matrix(int64_t w, int64_t h, double angle);

// Per-image enhance operations (an addition to the reference's surface):
// Pillow's ImageEnhance.Sharpness / Color / Brightness of the RGB result
// bytes, bit for bit, fused into the batch launch.  The
// op only marks the pending plan.  RGB images only: "image_sharpness: image
// must have 3 channels, not N" otherwise.  Bad arguments throw
// std::invalid_argument from the constructors.
class ImageEnhance : public ImageOp {
 public:
  // op: mxd_enhance_op (not NONE); factor: finite, 0 <= factor <= 1e6.
  ImageEnhance(std::string ikey, int32_t op, double factor, std::string okey);
  // The random forms: one uniform double in [lo, hi] from the thread's
  // generator per image; a video draws once for all its frames.
  ImageEnhance(std::string ikey, int32_t op, std::pair<double, double> range, std::string okey);
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;
  std::shared_ptr<Array> apply_video(const std::shared_ptr<Array>& video) const override;

 private:
  std::string name() const;
  double factor() const;  // the fixed one, or a draw
  std::shared_ptr<Array> mark(const std::shared_ptr<Array>& img, double factor) const;
  int32_t op_;
  bool random_;
  double lo_, hi_;
};
// "sharpness", "color", "brightness" of an mxd_enhance_op (the op is image_<name>).
const char* enhance_name(int32_t op);

// op/ImageTransform.h:139-152 ImageRotate: nearest-pixel rotation about the
// centre (core::image::rotate -> affine), one GPU pixel-map launch.
class ImageRotate : public ImageOp {
 public:
  ImageRotate(std::string ikey, double angle, bool crop, std::string okey)
      : ImageOp(std::move(ikey), std::move(okey)), angle_(angle), crop_(crop) {}
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;

 private:
  double angle_;
  bool crop_;
};

// op/ImageTransform.h:154-167 ImageChannelReduction: RGB -> (H, W, 1) gray in
// 16.16 fixed point with a named preset; unknown presets throw at construction.
class ImageChannelReduction : public ImageOp {
 public:
  ImageChannelReduction(std::string ikey, const std::string& preset, std::string okey);
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;

 private:
  float params_[4];  // bias, m0, m1, m2
};

// op/ImageTransform.h ImageRandomAreaCrop: a crop whose area and aspect ratio
// are drawn by rejection sampling (Inception-style); the image unchanged when
// no trial meets the constraints.
class ImageRandomAreaCrop : public ImageOp {
 public:
  ImageRandomAreaCrop(std::string ikey, std::pair<float, float> area_range, std::pair<float, float> aspect_ratio_range,
                      int num_trial, std::string okey);
  std::shared_ptr<Array> apply_image(const std::shared_ptr<Array>& img) const override;
  std::shared_ptr<Array> apply_video(const std::shared_ptr<Array>& video) const override;
  // (x, y, w, h) of the crop for a w x h image, all 0 when none was found.
  std::array<int64_t, 4> draw(int64_t w, int64_t h) const;

 private:
  std::pair<float, float> area_, aspect_;
  int trials_;
};

// Decoder hook: (path or encoded bytes, from_memory) -> (H, W, 3) uint8, or
// nullptr when the image cannot be decoded.  Installed by the binding.
using ImageDecoder = std::function<std::shared_ptr<Array>(const std::string& path, const std::shared_ptr<Array>& bytes,
                                                          bool from_memory, bool info)>;
void set_image_decoder(ImageDecoder dec);

class LoadImage : public KeyTransformOp {
 public:
  LoadImage(std::string ikey, std::string prefix, bool info, std::string format, bool from_memory, std::string okey);
  std::shared_ptr<Array> apply_key(const std::shared_ptr<Array>& x) const override;

 private:
  std::string prefix_;
  bool info_;
  std::string format_;
  bool from_memory_;
};

// ---------------------------------------------------------------- batching
// array::batch semantics (pad with pad_value to the max shape; optional
// concatenation dim).  Pending image plans of one key become one fused launch.
// device >= 0: the batch is made in that device's memory:
// pending images are written there by the kernel (host sources staged, no
// D2H); anything else is batched on the host and uploaded once.
std::shared_ptr<Array> batch_arrays(const std::vector<std::shared_ptr<Array>>& arrs, double pad_value, int dim,
                                    bool has_dim, int device = -1);

// Where merge_batch puts each key: device < 0 everything on the host; else
// the listed keys on `device`, or (empty list) every key with a pending image.
struct DeviceOut {
  int device = -1;
  std::vector<std::string> keys;
};
// batch_mix: MixUp / CutMix across the images of `key` in a batch (timm's
// FastCollateMixup).  The partner of image i of n is
// n - 1 - i.  mode: one draw set per batch, per pair (i < ceil(n / 2), shared by
// both members) or per image.
enum class MixMode : int { Batch = 0, Pair = 1, Elem = 2 };
struct MixSpec {
  std::string key, lam_key = "mix_lam", partner_key = "mix_partner";
  double mixup_alpha = 0.0, cutmix_alpha = 0.0, prob = 1.0, switch_prob = 0.5;
  MixMode mode = MixMode::Batch;
};
// Throws std::invalid_argument (the op's ValueError) for a spec no batch could run.
void check_mix_spec(const MixSpec& spec);
// What one image of a batch gets: the C ABI's entry and the weight of its own label.
struct MixDraw {
  mxd_mix mix;
  float lam;  // 1 for MXD_MIX_NONE; CutMix: 1 - box area / (h w)
};
// The entries of a batch of n images of h x w pixels, drawn from the calling
// thread's State.  Per draw set, with freshly constructed distributions:
// uniform_real<double>(0, 1), the set is applied iff it is < prob (nothing more
// is drawn otherwise); with both alphas > 0 one more, CutMix iff it is <
// switch_prob; lam, one uniform_real<double>(0, 1) for alpha == 1, else
// g1 / (g1 + g2) of two gamma_distribution<double>(alpha, 1) draws; for CutMix
// timm's rand_bbox without margin: cy = uniform_int<int>(0, h - 1), then cx.
std::vector<MixDraw> batch_mix_draws(int64_t n, int64_t h, int64_t w, const MixSpec& spec);

// mix: the arrays of mix->key are mixed (batch_mix) and the sample gains
// mix->lam_key (float32 (B,)) and mix->partner_key (int64 (B,)).
Sample merge_batch(const std::vector<Sample>& samples, const std::unordered_map<std::string, double>& pad,
                   const std::unordered_map<std::string, int>& dims, const DeviceOut& out = {},
                   const MixSpec* mix = nullptr);

// ---------------------------------------------------------------- threads
// Workers share the queue state with the pool, so the pool may be destroyed
// from one of its own workers: a finished task's result can hold the last
// reference to the pipeline that owns the pool (an exception carrying a
// Python traceback, released on the worker).  That worker is detached
// instead of joined and leaves its loop through the shared state.
class ThreadPool {
 public:
  explicit ThreadPool(int n);
  ~ThreadPool();
  std::future<Sample> enqueue(std::function<Sample()> fn);
  // Whether the calling thread is one of this pool's workers.
  bool on_worker() const;

 private:
  struct State {
    std::queue<std::packaged_task<Sample()>> tasks;
    std::mutex mu;
    std::condition_variable cv;
    bool stop = false;
  };
  std::shared_ptr<State> st_;
  std::vector<std::thread> workers_;
};

// ---------------------------------------------------------------- buffers
class Buffer {
 public:
  virtual ~Buffer() = default;
  virtual int64_t size() const = 0;
  virtual Sample get(int64_t idx) const = 0;
};

class FromVector : public Buffer {
 public:
  explicit FromVector(std::vector<Sample> data) : data_(std::move(data)) {}
  int64_t size() const override { return (int64_t)data_.size(); }
  Sample get(int64_t idx) const override;

 private:
  std::vector<Sample> data_;
};

class Perm : public Buffer {
 public:
  Perm(std::shared_ptr<Buffer> b, std::vector<int64_t> perm);
  int64_t size() const override { return (int64_t)perm_.size(); }
  Sample get(int64_t idx) const override;

 private:
  std::shared_ptr<Buffer> b_;
  std::vector<int64_t> perm_;
};
std::shared_ptr<Buffer> shuffle_buffer(const std::shared_ptr<Buffer>& b);

class BufferTransform : public Buffer {
 public:
  BufferTransform(std::shared_ptr<Buffer> b, std::shared_ptr<Op> op) : b_(std::move(b)), op_(std::move(op)) {}
  int64_t size() const override { return b_->size(); }
  Sample get(int64_t idx) const override;

 private:
  std::shared_ptr<Buffer> b_;
  std::shared_ptr<Op> op_;
};

class BufferBatch : public Buffer {
 public:
  BufferBatch(std::shared_ptr<Buffer> b, int64_t batch_size, std::unordered_map<std::string, double> pad,
              std::unordered_map<std::string, int> dims, DeviceOut out = {}, std::shared_ptr<const MixSpec> mix = nullptr);
  int64_t size() const override { return size_; }
  Sample get(int64_t idx) const override;

 private:
  std::shared_ptr<Buffer> b_;
  int64_t bs_, size_;
  std::unordered_map<std::string, double> pad_;
  std::unordered_map<std::string, int> dims_;
  DeviceOut out_;
  std::shared_ptr<const MixSpec> mix_;  // batch_mix
};

// ---------------------------------------------------------------- streams
class Stream {
 public:
  virtual ~Stream() = default;
  virtual Sample next() const = 0;
  virtual void reset() = 0;
};

class FromBuffer : public Stream {
 public:
  explicit FromBuffer(std::shared_ptr<Buffer> b) : b_(std::move(b)) {}
  Sample next() const override;
  void reset() override;

 private:
  std::shared_ptr<Buffer> b_;
  mutable std::mutex mu_;
  mutable int64_t idx_ = 0;
};

class StreamTransform : public Stream {
 public:
  StreamTransform(std::shared_ptr<Stream> s, std::shared_ptr<Op> op) : s_(std::move(s)), op_(std::move(op)) {}
  Sample next() const override;
  void reset() override { s_->reset(); }

 private:
  std::shared_ptr<Stream> s_;
  std::shared_ptr<Op> op_;
};

class StreamBatch : public Stream {
 public:
  StreamBatch(std::shared_ptr<Stream> s, int64_t batch_size, std::unordered_map<std::string, double> pad,
              std::unordered_map<std::string, int> dims, DeviceOut out = {}, std::shared_ptr<const MixSpec> mix = nullptr);
  Sample next() const override;
  void reset() override { s_->reset(); }

 private:
  std::shared_ptr<Stream> s_;
  int64_t bs_;
  std::unordered_map<std::string, double> pad_;
  std::unordered_map<std::string, int> dims_;
  DeviceOut out_;
  std::shared_ptr<const MixSpec> mix_;  // batch_mix
};

class Prefetch : public Stream {
 public:
  Prefetch(std::shared_ptr<Stream> s, int prefetch_size, int num_threads);
  ~Prefetch() override;
  Sample next() const override;
  void reset() override;

 private:
  std::shared_ptr<Stream> s_;
  std::unique_ptr<ThreadPool> pool_;
  int size_;
  mutable std::mutex mu_;
  mutable std::queue<std::future<Sample>> cache_;
};

class OrderedPrefetch : public Stream {
 public:
  OrderedPrefetch(std::shared_ptr<Buffer> b, int prefetch_size, int num_threads);
  ~OrderedPrefetch() override;
  Sample next() const override;
  void reset() override;

 private:
  std::shared_ptr<Buffer> b_;
  std::unique_ptr<ThreadPool> pool_;
  int size_;
  mutable std::mutex mu_;
  mutable std::vector<std::future<Sample>> cache_;
  mutable int64_t idx_ = 0;
};

}  // namespace pipe
}  // namespace mxd
