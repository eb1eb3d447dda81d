// module.cpp -- pybind11 binding of the pipeline (csrc/pipeline) with the
// mlx.data Python surface for the image path: names and keyword arguments of
// python/src/wrap_dataset.h:83-110,305-332,364-402,746-777,
// wrap_stream.cpp:123-129,340-377, wrap_buffer.cpp:93,250,342,358,373 and
// the numpy conversions of wrap.cpp:27-222.  The GIL is released around every
// get()/next(), so prefetch workers (and the GPU launches they issue) run in
// parallel; Python callbacks (key_transform functions, the image decoder)
// re-acquire it.
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <sstream>

#include "../pipeline/pipeline.h"
#include "mxd_amd.h"

namespace py = pybind11;
using namespace mxd::pipe;

namespace {

// ------------------------------------------------------------ numpy -> Array
std::shared_ptr<Array> to_array(py::handle obj);

std::shared_ptr<Array> from_numpy(py::array a) {
  if (!(a.flags() & py::detail::npy_api::constants::NPY_ARRAY_C_CONTIGUOUS_))
    throw std::runtime_error("[to_array] Contiguous array expected -- use numpy.ascontiguousarray()");
  std::vector<int64_t> shape(a.ndim());
  for (int i = 0; i < a.ndim(); i++) shape[i] = a.shape(i);
  // Zero copy: the Array keeps a reference to the numpy object, dropped under
  // the GIL (wrap.cpp:97-105).  Read-only arrays are fine: the pipeline never
  // writes into an input.
  auto handle = a.inc_ref();
  std::shared_ptr<void> data(const_cast<void*>(a.data()), [handle](void*) {
    py::gil_scoped_acquire gil;
    handle.dec_ref();
  });
  DType t;
  switch (a.dtype().char_()) {
    case 'f': t = DType::Float; break;
    case 'e': t = DType::Float16; break;
    case 'd': t = DType::Double; break;
    case 'i': t = DType::Int32; break;
    case 'l':
    case 'q': t = DType::Int64; break;
    case 'b': t = DType::Int8; break;
    case 'B': t = DType::UInt8; break;
    case 'S':
      shape.push_back(a.itemsize());
      t = DType::Int8;
      break;
    default: {
      std::ostringstream msg;
      msg << "[to_array] Unsupported array type '" << a.dtype().char_() << "'";
      throw std::invalid_argument(msg.str());
    }
  }
  return std::make_shared<Array>(t, shape, data);
}

std::shared_ptr<Array> scalar_i64(int64_t v) {
  auto buf = std::shared_ptr<void>(new int64_t(v), [](void* p) { delete static_cast<int64_t*>(p); });
  return std::make_shared<Array>(DType::Int64, std::vector<int64_t>{}, buf);
}

std::shared_ptr<Array> scalar_f64(double v) {
  auto buf = std::shared_ptr<void>(new double(v), [](void* p) { delete static_cast<double*>(p); });
  return std::make_shared<Array>(DType::Double, std::vector<int64_t>{}, buf);
}

std::shared_ptr<Array> from_bytes(const char* p, size_t n) {
  auto a = std::make_shared<Array>(DType::Int8, std::vector<int64_t>{(int64_t)n});
  if (n) std::memcpy(a->data(), p, n);
  return a;
}

struct DeviceArray;
std::shared_ptr<Array> device_array_of(py::handle obj);

std::shared_ptr<Array> to_array(py::handle obj) {
  if (py::isinstance<py::array>(obj)) return from_numpy(obj.cast<py::array>());
  if (auto d = device_array_of(obj)) return d;
  if (py::isinstance<py::bool_>(obj) || py::isinstance<py::int_>(obj)) return scalar_i64(obj.cast<int64_t>());
  if (py::isinstance<py::float_>(obj)) return scalar_f64(obj.cast<double>());
  if (py::isinstance<py::bytes>(obj)) {
    char* p;
    Py_ssize_t n;
    PyBytes_AsStringAndSize(obj.ptr(), &p, &n);
    return from_bytes(p, (size_t)n);
  }
  if (py::isinstance<py::str>(obj))
    throw std::invalid_argument("[to_array] Cannot convert strings to arrays. Please encode them as bytes first.");
  // A Python buffer (bytearray, array.array, memoryview ...) is copied: it
  // may be mutable and is not ours to alias (wrap.cpp:159-163, to_array(py::buffer)).
  if (py::isinstance<py::buffer>(obj)) {
    py::buffer_info info = obj.cast<py::buffer>().request();
    int64_t expect = info.itemsize;
    bool contiguous = true;
    for (int d = info.ndim - 1; d >= 0; d--) {
      if (info.shape[d] > 1 && info.strides[d] != expect) contiguous = false;
      expect *= info.shape[d];
    }
    if (!contiguous) throw std::invalid_argument("[to_array] Contiguous buffer expected -- maybe cast to np.array");
    py::array a = py::array::ensure(obj);
    if (!a) throw std::invalid_argument("[to_array] Unsupported buffer type '" + info.format + "'");
    return from_numpy(a.attr("copy")().cast<py::array>());
  }
  // Anything else with the array interface (wrap.cpp:165-175).
  try {
    return from_numpy(py::array::ensure(obj));
  } catch (const std::exception&) {
  }
  std::ostringstream msg;
  msg << "[to_array] Cannot convert type " << py::str(py::type::of(obj)).cast<std::string>()
      << " to an array. Use a numpy array, a python buffer or scalar.";
  throw std::invalid_argument(msg.str());
}

// ------------------------------------------------------------ Array -> numpy
py::dtype np_dtype(DType t) {
  switch (t) {
    case DType::Int8: return py::dtype("b");
    case DType::UInt8: return py::dtype("B");
    case DType::Int32: return py::dtype("i4");
    case DType::Int64: return py::dtype("i8");
    case DType::Float: return py::dtype("f");
    case DType::Double: return py::dtype("d");
    case DType::Float16: return py::dtype("e");
    case DType::BFloat16:
      throw std::runtime_error(
          "bfloat16 has no NumPy type: build the batch in device memory (batch(..., device=d)) and take it "
          "through DLPack (torch.from_dlpack)");
    default: throw std::runtime_error("internal error: unknown type");
  }
}

py::array to_numpy(const std::shared_ptr<Array>& a) {
  py::dtype dt = np_dtype(a->type());  // (bfloat16 raises before any GPU work)
  void* data;
  {
    // May run the pending GPU work of this array.
    py::gil_scoped_release nogil;
    data = a->data();
  }
  auto* keep = new std::shared_ptr<Array>(a);
  py::capsule owner(keep, [](void* p) { delete static_cast<std::shared_ptr<Array>*>(p); });
  std::vector<int64_t> shape = a->shape(), strides(shape.size());
  int64_t s = itemsize(a->type());
  for (int d = (int)shape.size() - 1; d >= 0; d--) {
    strides[d] = s;
    s *= shape[d];
  }
  return py::array(dt, shape, strides, data, owner);
}

// ------------------------------------------------------------ device arrays
// DLPack (v0.8 ABI, dlpack.h): a device batch is handed to consumers
// (torch.from_dlpack, ...) without a copy.  Only the layout is restated here.
struct DLDevice {
  int32_t device_type;  // kDLROCM = 10
  int32_t device_id;
};
struct DLDataType {
  uint8_t code;  // kDLInt 0, kDLUInt 1, kDLFloat 2, kDLBfloat 4
  uint8_t bits;
  uint16_t lanes;
};
struct DLTensor {
  void* data;
  DLDevice device;
  int32_t ndim;
  DLDataType dtype;
  int64_t* shape;
  int64_t* strides;
  uint64_t byte_offset;
};
struct DLManagedTensor {
  DLTensor dl_tensor;
  void* manager_ctx;
  void (*deleter)(DLManagedTensor*);
};
constexpr int32_t kDLROCM = 10;

DLDataType dl_dtype(DType t) {
  switch (t) {
    case DType::UInt8: return {1, 8, 1};
    case DType::Int8: return {0, 8, 1};
    case DType::Int32: return {0, 32, 1};
    case DType::Int64: return {0, 64, 1};
    case DType::Float: return {2, 32, 1};
    case DType::Double: return {2, 64, 1};
    case DType::Float16: return {2, 16, 1};
    case DType::BFloat16: return {4, 16, 1};
    default: throw std::runtime_error("internal error: unknown type");
  }
}

// The Python face of a device-resident Array.
struct DeviceArray {
  std::shared_ptr<Array> a;
};

struct DLHolder {
  std::shared_ptr<Array> a;
  std::vector<int64_t> shape;
  DLManagedTensor t{};
};

py::capsule to_dlpack(const std::shared_ptr<Array>& a) {
  auto* h = new DLHolder{a, a->shape(), {}};
  h->t.dl_tensor.data = a->data();
  h->t.dl_tensor.device = {kDLROCM, a->device()};
  h->t.dl_tensor.ndim = a->ndim();
  h->t.dl_tensor.dtype = dl_dtype(a->type());
  h->t.dl_tensor.shape = h->shape.data();
  h->t.dl_tensor.strides = nullptr;  // compact row-major
  h->t.manager_ctx = h;
  h->t.deleter = [](DLManagedTensor* t) { delete static_cast<DLHolder*>(t->manager_ctx); };
  // A capsule never consumed ("dltensor" still its name) frees the tensor.
  return py::capsule(&h->t, "dltensor", [](PyObject* cap) {
    if (PyCapsule_IsValid(cap, "dltensor")) {
      auto* t = static_cast<DLManagedTensor*>(PyCapsule_GetPointer(cap, "dltensor"));
      if (t && t->deleter) t->deleter(t);
    }
  });
}

py::array device_to_numpy(const std::shared_ptr<Array>& a) {
  py::array host = to_numpy(std::make_shared<Array>(a->type(), a->shape()));
  {
    py::gil_scoped_release nogil;
    if (a->nbytes() > 0 && mxd_memcpy_d2h(host.mutable_data(), a->data(), (size_t)a->nbytes(), a->device()) != MXD_OK)
      throw std::runtime_error(mxd_last_error());
  }
  return host;
}

py::object to_py(const std::shared_ptr<Array>& a) {
  if (a->device() >= 0) return py::cast(DeviceArray{a});
  return to_numpy(a);
}

py::dict to_dict(const Sample& s) {
  py::dict d;
  for (const auto& kv : s) d[py::str(kv.first)] = to_py(kv.second);
  return d;
}

Sample to_sample(py::handle obj) {
  if (!py::isinstance<py::dict>(obj)) throw std::invalid_argument("Sample: dict expected");
  Sample s;
  for (auto kv : obj.cast<py::dict>()) s[kv.first.cast<std::string>()] = to_array(kv.second);
  return s;
}

// A Python callable that may be destroyed from a worker thread.
std::shared_ptr<py::function> hold(py::function f) {
  return std::shared_ptr<py::function>(new py::function(std::move(f)), [](py::function* p) {
    if (_Py_IsFinalizing()) return;  // the interpreter is going: taking the GIL would block forever
    py::gil_scoped_acquire gil;
    delete p;
  });
}

// A prefetching stream or buffer whose last Python reference goes away joins
// its worker threads, and those may be waiting for the GIL (a Python
// key_transform, the image decoder): destroy it with the GIL released.  At
// interpreter exit the workers can no longer take the GIL at all, so the
// object is left to the process teardown.
template <class T>
std::shared_ptr<T> nogil_owned(T* obj) {
  return std::shared_ptr<T>(obj, [](T* o) {
    if (_Py_IsFinalizing()) return;
    if (PyGILState_Check()) {
      py::gil_scoped_release nogil;
      delete o;
    } else {
      delete o;
    }
  });
}

// image_normalize's mean / std: None, a scalar, or one value per channel.
std::vector<float> channel_values(const py::object& v, const char* what) {
  if (v.is_none()) return {};
  if (py::isinstance<py::float_>(v) || py::isinstance<py::int_>(v)) return {v.cast<float>()};
  if (!py::isinstance<py::str>(v) && !py::isinstance<py::bytes>(v)) {
    try {
      auto out = v.cast<std::vector<float>>();
      if (!out.empty()) return out;
    } catch (const py::cast_error&) {
    }
  }
  throw std::invalid_argument(std::string("image_normalize: ") + what + " must be None, a number or a sequence of numbers");
}

// image_color_matrix's matrix: a 3 x 3 or 3 x 4 nested sequence or array, for
// [r g b 1] in [0, 1] units -> row-major 3 x 4 with the offsets scaled to byte
// units (x 255, in float32).
std::array<float, 12> color_matrix(const py::object& v) {
  std::vector<std::vector<float>> rows;
  try {
    rows = v.cast<std::vector<std::vector<float>>>();
  } catch (const py::cast_error&) {
    throw std::invalid_argument("image_color_matrix: matrix must be a 3x3 or 3x4 nested sequence or array of numbers");
  }
  if (rows.size() != 3 || (rows[0].size() != 3 && rows[0].size() != 4) || rows[1].size() != rows[0].size() ||
      rows[2].size() != rows[0].size())
    throw std::invalid_argument("image_color_matrix: matrix must be 3x3 or 3x4");
  std::array<float, 12> m{};
  for (int r = 0; r < 3; r++)
    for (size_t k = 0; k < rows[r].size(); k++) {
      if (!std::isfinite(rows[r][k])) throw std::invalid_argument("image_color_matrix: entries must be finite");
      m[4 * r + k] = k == 3 ? rows[r][k] * 255.0f : rows[r][k];
    }
  return m;
}

// image_random_color_twist's arguments: None or a (lo, hi) pair each.
void color_range(const py::object& v, const char* what, int k, std::array<bool, 4>& has,
                 std::array<ImageRandomColorTwist::Range, 4>& range) {
  has[k] = !v.is_none();
  if (!has[k]) return;
  try {
    range[k] = v.cast<std::pair<double, double>>();
  } catch (const py::cast_error&) {
    throw std::invalid_argument(std::string("image_random_color_twist: ") + what + " must be None or a (lo, hi) pair");
  }
}

// The affine ops' fill: a scalar or an (r, g, b) sequence of integers.
std::array<int64_t, 3> warp_fill_arg(const std::string& op, const py::object& v) {
  try {
    if (py::isinstance<py::int_>(v)) {
      const int64_t f = v.cast<int64_t>();
      return {{f, f, f}};
    }
    const auto rgb = v.cast<std::vector<int64_t>>();
    if (rgb.size() == 3) return {{rgb[0], rgb[1], rgb[2]}};
  } catch (const py::cast_error&) {
  }
  throw std::invalid_argument(op + ": fill must be an integer or an (r, g, b) sequence of integers");
}

// The random affine ops' arguments: None or a (lo, hi) pair each.
void warp_range(const std::string& op, const py::object& v, const char* what, int k, std::array<bool, 2>& has,
                std::array<ImageAffine::Range, 2>& range) {
  has[k] = !v.is_none();
  if (!has[k]) return;
  try {
    range[k] = v.cast<std::pair<double, double>>();
  } catch (const py::cast_error&) {
    throw std::invalid_argument(op + ": " + what + " must be None or a (lo, hi) pair");
  }
}

std::shared_ptr<ImageAffine> affine_op(const char* op, const std::string& key, ImageAffine::Kind kind,
                                       const std::vector<double>& v, const std::string& resample, const py::object& fill,
                                       const std::string& output_key) {
  return std::make_shared<ImageAffine>(key, kind, v, parse_resample(op, resample), warp_fill_arg(op, fill), output_key);
}

std::shared_ptr<ImageAffine> random_affine_op(const char* op, const std::string& key, ImageAffine::Kind kind,
                                              const py::object& a, const char* a_name, const py::object& b,
                                              const std::string& resample, const py::object& fill,
                                              const std::string& output_key) {
  std::array<bool, 2> has{};
  std::array<ImageAffine::Range, 2> range{};
  warp_range(op, a, a_name, 0, has, range);
  if (kind != ImageAffine::kRotate) warp_range(op, b, "y", 1, has, range);
  return std::make_shared<ImageAffine>(key, kind, has, range, parse_resample(op, resample), warp_fill_arg(op, fill),
                                       output_key);
}

// The random enhance ops' factor: a (lo, hi) pair.
std::pair<double, double> enhance_range(const std::string& op, const py::object& v) {
  try {
    return v.cast<std::pair<double, double>>();
  } catch (const py::cast_error&) {
    throw std::invalid_argument(op + ": factor must be a (lo, hi) pair");
  }
}

// ------------------------------------------------------------ dataset ops
// The ops every Dataset (Buffer and Stream) carries (wrap_dataset.h).
template <class D, class Wrap>
void dataset_ops(py::class_<D, std::shared_ptr<D>>& cls, Wrap wrap) {
  using Self = std::shared_ptr<D>;
  cls.def(
         "key_transform",
         [wrap](const Self& self, const std::string& key, py::function func, const std::string& output_key) {
           auto fn = hold(std::move(func));
           auto op = std::make_shared<KeyTransform>(
               key,
               [fn](const std::shared_ptr<Array>& x) {
                 py::gil_scoped_acquire gil;
                 return to_array((*fn)(to_py(x)));
               },
               output_key);
           return wrap(self, op);
         },
         py::arg("key"), py::arg("func"), py::arg("output_key") = "")
      .def(
          "load_image",
          [wrap](const Self& self, const std::string& key, const std::string& prefix, bool info,
                 const std::string& format, bool from_memory, const std::string& output_key) {
            return wrap(self, std::make_shared<LoadImage>(key, prefix, info, format, from_memory, output_key));
          },
          py::arg("key"), py::arg("prefix") = "", py::arg("info") = false, py::arg("format") = "RGB",
          py::arg("from_memory") = false, py::arg("output_key") = "")
      .def(
          "image_resize_smallest_side",
          [wrap](const Self& self, const std::string& key, int64_t size, const std::string& output_key,
                 const std::string& filter) {
            return wrap(self, std::make_shared<ImageResizeSmallestSide>(key, size, output_key, parse_filter(filter)));
          },
          py::arg("key"), py::arg("size"), py::arg("output_key") = "", py::kw_only(), py::arg("filter") = "triangle")
      .def(
          "image_resize",
          [wrap](const Self& self, const std::string& key, int64_t w, int64_t h, const std::string& output_key,
                 const std::string& filter) {
            return wrap(self, std::make_shared<ImageResize>(key, w, h, output_key, parse_filter(filter)));
          },
          py::arg("key"), py::arg("w"), py::arg("h"), py::arg("output_key") = "", py::kw_only(),
          py::arg("filter") = "triangle")
      .def(
          "image_center_crop",
          [wrap](const Self& self, const std::string& key, int64_t w, int64_t h, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageCenterCrop>(key, w, h, output_key));
          },
          py::arg("key"), py::arg("w"), py::arg("h"), py::arg("output_key") = "")
      .def(
          "image_random_crop",
          [wrap](const Self& self, const std::string& key, int64_t w, int64_t h, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageRandomCrop>(key, w, h, output_key));
          },
          py::arg("key"), py::arg("w"), py::arg("h"), py::arg("output_key") = "")
      .def(
          "image_random_h_flip",
          [wrap](const Self& self, const std::string& key, float prob, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageRandomHFlip>(key, prob, output_key));
          },
          py::arg("key"), py::arg("prob"), py::arg("output_key") = "")
      .def(
          "image_random_area_crop",
          [wrap](const Self& self, const std::string& key, std::pair<float, float> area_range,
                 std::pair<float, float> aspect_ratio_range, int num_trial, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageRandomAreaCrop>(key, area_range, aspect_ratio_range, num_trial,
                                                                    output_key));
          },
          py::arg("key"), py::arg("area_range"), py::arg("aspect_ratio_range"), py::arg("num_trial") = 10,
          py::arg("output_key") = "")
      .def(
          "image_rotate",
          [wrap](const Self& self, const std::string& key, double angle, bool crop, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageRotate>(key, angle, crop, output_key));
          },
          py::arg("key"), py::arg("angle"), py::arg("crop") = false, py::arg("output_key") = "")
      .def(
          "image_channel_reduction",
          [wrap](const Self& self, const std::string& key, const std::string& preset, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageChannelReduction>(key, preset, output_key));
          },
          py::arg("key"), py::arg("preset") = "default", py::arg("output_key") = "")
      .def(
          "image_to_float",
          [wrap](const Self& self, const std::string& key, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageToFloat>(key, output_key));
          },
          py::arg("key"), py::arg("output_key") = "")
      .def(
          "image_normalize",
          [wrap](const Self& self, const std::string& key, const py::object& mean, const py::object& std,
                 const std::string& dtype, const std::string& layout, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageNormalize>(key, channel_values(mean, "mean"),
                                                               channel_values(std, "std"), dtype, layout, output_key));
          },
          py::arg("key"), py::arg("mean") = py::none(), py::arg("std") = py::none(), py::arg("dtype") = "float32",
          py::arg("layout") = "hwc", py::arg("output_key") = "")
      .def(
          "image_color_twist",
          [wrap](const Self& self, const std::string& key, double brightness, double contrast, double saturation,
                 double hue, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageColorMatrix>(
                                  key, color_twist(brightness, contrast, saturation, hue), output_key));
          },
          py::arg("key"), py::arg("brightness") = 1.0, py::arg("contrast") = 1.0, py::arg("saturation") = 1.0,
          py::arg("hue") = 0.0, py::arg("output_key") = "")
      .def(
          "image_color_matrix",
          [wrap](const Self& self, const std::string& key, const py::object& matrix, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageColorMatrix>(key, color_matrix(matrix), output_key));
          },
          py::arg("key"), py::arg("matrix"), py::arg("output_key") = "")
      .def(
          "image_random_color_twist",
          [wrap](const Self& self, const std::string& key, const py::object& brightness, const py::object& contrast,
                 const py::object& saturation, const py::object& hue, const std::string& output_key) {
            std::array<bool, 4> has{};
            std::array<ImageRandomColorTwist::Range, 4> range{};
            color_range(brightness, "brightness", 0, has, range);
            color_range(contrast, "contrast", 1, has, range);
            color_range(saturation, "saturation", 2, has, range);
            color_range(hue, "hue", 3, has, range);
            return wrap(self, std::make_shared<ImageRandomColorTwist>(key, has, range, output_key));
          },
          py::arg("key"), py::arg("brightness") = py::none(), py::arg("contrast") = py::none(),
          py::arg("saturation") = py::none(), py::arg("hue") = py::none(), py::arg("output_key") = "")
      .def(
          "image_posterize",
          [wrap](const Self& self, const std::string& key, int64_t bits, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageTone>(key, MXD_TONE_POSTERIZE, bits, 0.0, output_key));
          },
          py::arg("key"), py::arg("bits"), py::arg("output_key") = "")
      .def(
          "image_solarize",
          [wrap](const Self& self, const std::string& key, int64_t threshold, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageTone>(key, MXD_TONE_SOLARIZE, threshold, 0.0, output_key));
          },
          py::arg("key"), py::arg("threshold") = 128, py::arg("output_key") = "")
      .def(
          "image_autocontrast",
          [wrap](const Self& self, const std::string& key, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageTone>(key, MXD_TONE_AUTOCONTRAST, 0, 0.0, output_key));
          },
          py::arg("key"), py::arg("output_key") = "")
      .def(
          "image_equalize",
          [wrap](const Self& self, const std::string& key, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageTone>(key, MXD_TONE_EQUALIZE, 0, 0.0, output_key));
          },
          py::arg("key"), py::arg("output_key") = "")
      .def(
          "image_contrast",
          [wrap](const Self& self, const std::string& key, double factor, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageTone>(key, MXD_TONE_CONTRAST, 0, factor, output_key));
          },
          py::arg("key"), py::arg("factor"), py::arg("output_key") = "")
      .def(
          "image_affine",
          [wrap](const Self& self, const std::string& key, const py::object& matrix, const std::string& resample,
                 const py::object& fill, const std::string& output_key) {
            std::vector<double> m;
            try {
              m = matrix.cast<std::vector<double>>();
            } catch (const py::cast_error&) {
              throw std::invalid_argument("image_affine: matrix must be a sequence of 6 numbers");
            }
            if (m.size() != 6) throw std::invalid_argument("image_affine: matrix must be a sequence of 6 numbers");
            return wrap(self, affine_op("image_affine", key, ImageAffine::kMatrix, m, resample, fill, output_key));
          },
          py::arg("key"), py::arg("matrix"), py::arg("resample") = "nearest", py::arg("fill") = 0,
          py::arg("output_key") = "")
      .def(
          "image_shear",
          [wrap](const Self& self, const std::string& key, double x, double y, const std::string& resample,
                 const py::object& fill, const std::string& output_key) {
            return wrap(self, affine_op("image_shear", key, ImageAffine::kShear, {x, y}, resample, fill, output_key));
          },
          py::arg("key"), py::arg("x") = 0.0, py::arg("y") = 0.0, py::arg("resample") = "nearest", py::arg("fill") = 0,
          py::arg("output_key") = "")
      .def(
          "image_translate",
          [wrap](const Self& self, const std::string& key, double x, double y, const std::string& resample,
                 const py::object& fill, const std::string& output_key) {
            return wrap(self,
                        affine_op("image_translate", key, ImageAffine::kTranslate, {x, y}, resample, fill, output_key));
          },
          py::arg("key"), py::arg("x") = 0.0, py::arg("y") = 0.0, py::arg("resample") = "nearest", py::arg("fill") = 0,
          py::arg("output_key") = "")
      .def(
          "image_affine_rotate",
          [wrap](const Self& self, const std::string& key, double angle, const std::string& resample,
                 const py::object& fill, const std::string& output_key) {
            return wrap(self,
                        affine_op("image_affine_rotate", key, ImageAffine::kRotate, {angle}, resample, fill, output_key));
          },
          py::arg("key"), py::arg("angle"), py::arg("resample") = "nearest", py::arg("fill") = 0,
          py::arg("output_key") = "")
      .def(
          "image_random_shear",
          [wrap](const Self& self, const std::string& key, const py::object& x, const py::object& y,
                 const std::string& resample, const py::object& fill, const std::string& output_key) {
            return wrap(self, random_affine_op("image_random_shear", key, ImageAffine::kShear, x, "x", y, resample, fill,
                                               output_key));
          },
          py::arg("key"), py::arg("x") = py::none(), py::arg("y") = py::none(), py::arg("resample") = "nearest",
          py::arg("fill") = 0, py::arg("output_key") = "")
      .def(
          "image_random_translate",
          [wrap](const Self& self, const std::string& key, const py::object& x, const py::object& y,
                 const std::string& resample, const py::object& fill, const std::string& output_key) {
            return wrap(self, random_affine_op("image_random_translate", key, ImageAffine::kTranslate, x, "x", y, resample,
                                               fill, output_key));
          },
          py::arg("key"), py::arg("x") = py::none(), py::arg("y") = py::none(), py::arg("resample") = "nearest",
          py::arg("fill") = 0, py::arg("output_key") = "")
      .def(
          "image_random_affine_rotate",
          [wrap](const Self& self, const std::string& key, const py::object& angle, const std::string& resample,
                 const py::object& fill, const std::string& output_key) {
            if (angle.is_none()) throw std::invalid_argument("image_random_affine_rotate: angle must be a (lo, hi) pair");
            return wrap(self, random_affine_op("image_random_affine_rotate", key, ImageAffine::kRotate, angle, "angle",
                                               py::none(), resample, fill, output_key));
          },
          py::arg("key"), py::arg("angle"), py::arg("resample") = "nearest", py::arg("fill") = 0,
          py::arg("output_key") = "")
      .def(
          "image_sharpness",
          [wrap](const Self& self, const std::string& key, double factor, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageEnhance>(key, MXD_ENHANCE_SHARPNESS, factor, output_key));
          },
          py::arg("key"), py::arg("factor"), py::arg("output_key") = "")
      .def(
          "image_random_sharpness",
          [wrap](const Self& self, const std::string& key, const py::object& factor, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageEnhance>(key, MXD_ENHANCE_SHARPNESS, enhance_range("image_random_sharpness", factor),
                                                             output_key));
          },
          py::arg("key"), py::arg("factor"), py::arg("output_key") = "")
      .def(
          "image_color",
          [wrap](const Self& self, const std::string& key, double factor, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageEnhance>(key, MXD_ENHANCE_COLOR, factor, output_key));
          },
          py::arg("key"), py::arg("factor"), py::arg("output_key") = "")
      .def(
          "image_random_color",
          [wrap](const Self& self, const std::string& key, const py::object& factor, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageEnhance>(key, MXD_ENHANCE_COLOR, enhance_range("image_random_color", factor),
                                                             output_key));
          },
          py::arg("key"), py::arg("factor"), py::arg("output_key") = "")
      .def(
          "image_brightness",
          [wrap](const Self& self, const std::string& key, double factor, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageEnhance>(key, MXD_ENHANCE_BRIGHTNESS, factor, output_key));
          },
          py::arg("key"), py::arg("factor"), py::arg("output_key") = "")
      .def(
          "image_random_brightness",
          [wrap](const Self& self, const std::string& key, const py::object& factor, const std::string& output_key) {
            return wrap(self, std::make_shared<ImageEnhance>(key, MXD_ENHANCE_BRIGHTNESS, enhance_range("image_random_brightness", factor),
                                                             output_key));
          },
          py::arg("key"), py::arg("factor"), py::arg("output_key") = "");
}

using PadMap = std::unordered_map<std::string, double>;
using DimMap = std::unordered_map<std::string, int>;

std::shared_ptr<Array> device_array_of(py::handle obj) {
  if (!py::isinstance<DeviceArray>(obj)) return nullptr;
  return obj.cast<const DeviceArray&>().a;
}

// batch(..., device=None | int, device_keys=None | [str])
DeviceOut device_out(const py::object& device, const py::object& keys) {
  DeviceOut o;
  if (!device.is_none()) {
    o.device = device.cast<int>();
    if (o.device < 0) throw std::invalid_argument("batch: device must be a device index >= 0");
  }
  if (!keys.is_none()) o.keys = keys.cast<std::vector<std::string>>();
  if (!o.keys.empty() && o.device < 0) throw std::invalid_argument("batch: device_keys needs device");
  return o;
}

// batch_mix's keyword arguments as a checked MixSpec (ValueError when the op is made).
std::shared_ptr<const MixSpec> mix_spec(const std::string& key, double mixup_alpha, double cutmix_alpha, double prob,
                                        double switch_prob, const std::string& mode, const std::string& lam_key,
                                        const std::string& partner_key) {
  auto s = std::make_shared<MixSpec>();
  s->key = key, s->lam_key = lam_key, s->partner_key = partner_key;
  s->mixup_alpha = mixup_alpha, s->cutmix_alpha = cutmix_alpha, s->prob = prob, s->switch_prob = switch_prob;
  if (mode == "batch") s->mode = MixMode::Batch;
  else if (mode == "pair") s->mode = MixMode::Pair;
  else if (mode == "elem") s->mode = MixMode::Elem;
  else throw std::invalid_argument("batch_mix: unknown mode '" + mode + "' (batch, pair, elem)");
  check_mix_spec(*s);
  return s;
}

}  // namespace

PYBIND11_MODULE(_pipeline, m) {
  m.doc() = "mlx.data image-path operator surface over the gfx950 resize/crop kernels";

  py::class_<DeviceArray>(m, "DeviceArray",
                          "A batch tensor in device memory (batch(..., device=d)): DLPack producer "
                          "(__dlpack__ / __dlpack_device__, kDLROCM), numpy() copies it to the host.")
      .def_property_readonly("shape", [](const DeviceArray& d) { return py::tuple(py::cast(d.a->shape())); })
      .def_property_readonly("dtype",
                             [](const DeviceArray& d) -> py::object {
                               // bfloat16 has no NumPy dtype: its name instead
                               if (d.a->type() == DType::BFloat16) return py::str("bfloat16");
                               return np_dtype(d.a->type());
                             })
      .def_property_readonly("device", [](const DeviceArray& d) { return d.a->device(); })
      .def_property_readonly("data_ptr", [](const DeviceArray& d) { return reinterpret_cast<uintptr_t>(d.a->data()); })
      .def_property_readonly("nbytes", [](const DeviceArray& d) { return d.a->nbytes(); })
      .def("__dlpack__", [](const DeviceArray& d, py::kwargs) { return to_dlpack(d.a); })
      .def("__dlpack_device__", [](const DeviceArray& d) { return py::make_tuple(kDLROCM, d.a->device()); })
      .def("numpy", [](const DeviceArray& d) { return device_to_numpy(d.a); })
      .def("__array__", [](const DeviceArray& d, py::args, py::kwargs) { return device_to_numpy(d.a); })
      .def("__len__", [](const DeviceArray& d) { return d.a->ndim() ? d.a->shape(0) : 0; })
      .def("__repr__", [](const DeviceArray& d) {
        std::ostringstream o;
        o << "DeviceArray(shape=(";
        for (int i = 0; i < d.a->ndim(); i++) o << (i ? ", " : "") << d.a->shape(i);
        o << (d.a->ndim() == 1 ? ",)" : ")") << ", device=" << d.a->device() << ")";
        return o.str();
      });

  py::class_<Buffer, std::shared_ptr<Buffer>> buffer(m, "Buffer");
  py::class_<Stream, std::shared_ptr<Stream>> stream(m, "Stream");

  dataset_ops(buffer, [](const std::shared_ptr<Buffer>& b, std::shared_ptr<Op> op) -> std::shared_ptr<Buffer> {
    return std::make_shared<BufferTransform>(b, std::move(op));
  });
  dataset_ops(stream, [](const std::shared_ptr<Stream>& s, std::shared_ptr<Op> op) -> std::shared_ptr<Stream> {
    return std::make_shared<StreamTransform>(s, std::move(op));
  });

  buffer.def("size", &Buffer::size)
      .def("__len__", &Buffer::size)
      .def("__getitem__",
           [](const std::shared_ptr<Buffer>& b, int64_t idx) {
             Sample s;
             {
               py::gil_scoped_release nogil;
               idx = idx < 0 ? idx + b->size() : idx;  // wrap_buffer.cpp:62
               s = b->get(idx);
             }
             return to_dict(s);
           })
      .def("shuffle", [](const std::shared_ptr<Buffer>& b) { return shuffle_buffer(b); })
      .def("perm",
           [](const std::shared_ptr<Buffer>& b, std::vector<int64_t> perm) -> std::shared_ptr<Buffer> {
             return std::make_shared<Perm>(b, std::move(perm));
           })
      .def("to_stream", [](const std::shared_ptr<Buffer>& b) -> std::shared_ptr<Stream> {
        return std::make_shared<FromBuffer>(b);
      })
      .def(
          "batch",
          [](const std::shared_ptr<Buffer>& b, int64_t batch_size, PadMap pad, DimMap dim, py::object device,
             py::object device_keys) -> std::shared_ptr<Buffer> {
            return std::make_shared<BufferBatch>(b, batch_size, std::move(pad), std::move(dim),
                                                 device_out(device, device_keys));
          },
          py::arg("batch_size"), py::arg("pad") = PadMap{}, py::arg("dim") = DimMap{}, py::arg("device") = py::none(),
          py::arg("device_keys") = py::none())
      .def(
          "batch_mix",
          [](const std::shared_ptr<Buffer>& b, int64_t batch_size, const std::string& key, double mixup_alpha,
             double cutmix_alpha, double prob, double switch_prob, const std::string& mode, const std::string& lam_key,
             const std::string& partner_key, PadMap pad, DimMap dim, py::object device,
             py::object device_keys) -> std::shared_ptr<Buffer> {
            auto spec = mix_spec(key, mixup_alpha, cutmix_alpha, prob, switch_prob, mode, lam_key, partner_key);
            return std::make_shared<BufferBatch>(b, batch_size, std::move(pad), std::move(dim),
                                                 device_out(device, device_keys), std::move(spec));
          },
          py::arg("batch_size"), py::arg("key"), py::kw_only(), py::arg("mixup_alpha") = 0.0,
          py::arg("cutmix_alpha") = 0.0, py::arg("prob") = 1.0, py::arg("switch_prob") = 0.5, py::arg("mode") = "batch",
          py::arg("lam_key") = "mix_lam", py::arg("partner_key") = "mix_partner", py::arg("pad") = PadMap{},
          py::arg("dim") = DimMap{}, py::arg("device") = py::none(), py::arg("device_keys") = py::none())
      .def(
          "ordered_prefetch",
          [](const std::shared_ptr<Buffer>& b, int prefetch_size, int num_threads) -> std::shared_ptr<Stream> {
            return nogil_owned<Stream>(new OrderedPrefetch(b, prefetch_size, num_threads));
          },
          py::arg("prefetch_size"), py::arg("num_threads"));

  stream
      .def("next",
           [](const std::shared_ptr<Stream>& s) {
             Sample x;
             {
               py::gil_scoped_release nogil;
               x = s->next();
             }
             return to_dict(x);
           })
      .def("reset",
           [](const std::shared_ptr<Stream>& s) {
             py::gil_scoped_release nogil;
             s->reset();
           })
      .def(
          "batch",
          [](const std::shared_ptr<Stream>& s, int64_t batch_size, PadMap pad, DimMap dim, py::object device,
             py::object device_keys) -> std::shared_ptr<Stream> {
            return std::make_shared<StreamBatch>(s, batch_size, std::move(pad), std::move(dim),
                                                 device_out(device, device_keys));
          },
          py::arg("batch_size"), py::arg("pad") = PadMap{}, py::arg("dim") = DimMap{}, py::arg("device") = py::none(),
          py::arg("device_keys") = py::none())
      .def(
          "batch_mix",
          [](const std::shared_ptr<Stream>& s, int64_t batch_size, const std::string& key, double mixup_alpha,
             double cutmix_alpha, double prob, double switch_prob, const std::string& mode, const std::string& lam_key,
             const std::string& partner_key, PadMap pad, DimMap dim, py::object device,
             py::object device_keys) -> std::shared_ptr<Stream> {
            auto spec = mix_spec(key, mixup_alpha, cutmix_alpha, prob, switch_prob, mode, lam_key, partner_key);
            return std::make_shared<StreamBatch>(s, batch_size, std::move(pad), std::move(dim),
                                                 device_out(device, device_keys), std::move(spec));
          },
          py::arg("batch_size"), py::arg("key"), py::kw_only(), py::arg("mixup_alpha") = 0.0,
          py::arg("cutmix_alpha") = 0.0, py::arg("prob") = 1.0, py::arg("switch_prob") = 0.5, py::arg("mode") = "batch",
          py::arg("lam_key") = "mix_lam", py::arg("partner_key") = "mix_partner", py::arg("pad") = PadMap{},
          py::arg("dim") = DimMap{}, py::arg("device") = py::none(), py::arg("device_keys") = py::none())
      .def(
          "prefetch",
          [](const std::shared_ptr<Stream>& s, int prefetch_size, int num_threads) -> std::shared_ptr<Stream> {
            return nogil_owned<Stream>(new Prefetch(s, prefetch_size, num_threads));
          },
          py::arg("prefetch_size"), py::arg("num_threads"));

  m.def("buffer_from_vector", [](py::list data) -> std::shared_ptr<Buffer> {
    std::vector<Sample> samples;
    samples.reserve(data.size());
    for (auto item : data) {
      samples.push_back(to_sample(item));
      if (samples.back().empty()) throw std::runtime_error("FromVector: unexpected empty sample");
    }
    return std::make_shared<FromVector>(std::move(samples));
  });

  m.def("set_state", &set_state, py::arg("seed") = 1234);
  m.def("set_devices", &set_devices, py::arg("devices"));
  // diagnostics (device-free): the entries batch_mix would give a batch of n images of h x w pixels, drawn
  // from the calling thread's State: (op, partner, w_self, w_other, x0, y0, x1, y1, lam) per image
  m.def(
      "_batch_mix_draws",
      [](int64_t n, int64_t h, int64_t w, double mixup_alpha, double cutmix_alpha, double prob, double switch_prob,
         const std::string& mode) {
        auto spec = mix_spec("image", mixup_alpha, cutmix_alpha, prob, switch_prob, mode, "mix_lam", "mix_partner");
        std::vector<std::tuple<int, int, float, float, int, int, int, int, float>> out;
        for (const MixDraw& d : batch_mix_draws(n, h, w, *spec))
          out.emplace_back(d.mix.op, d.mix.partner, d.mix.w_self, d.mix.w_other, d.mix.x0, d.mix.y0, d.mix.x1, d.mix.y1,
                           d.lam);
        return out;
      },
      py::arg("n"), py::arg("h"), py::arg("w"), py::kw_only(), py::arg("mixup_alpha") = 0.0, py::arg("cutmix_alpha") = 0.0,
      py::arg("prob") = 1.0, py::arg("switch_prob") = 0.5, py::arg("mode") = "batch");
  // diagnostics: how a batch of n images is split over ndev devices
  m.def(
      "_split_batch",
      [](int64_t n, int64_t ndev, uint64_t first) {
        std::vector<std::tuple<int64_t, int64_t, int64_t>> out;
        for (const Slice& s : split_batch(n, ndev, first)) out.emplace_back(s.device, s.begin, s.end);
        return out;
      },
      py::arg("n"), py::arg("ndev"), py::arg("first") = 0);
  m.attr("_MIN_SLICE_IMAGES") = kMinSliceImages;
  m.def("devices", &devices);
  m.def("set_device_decode", &set_device_decode, py::arg("on"));
  m.def("set_device_entropy", &set_device_entropy, py::arg("on"));
  m.def("device_entropy", &device_entropy);
  m.def("device_decode", &device_decode);
  m.def("_device_pool_bytes", &device_pool_bytes, py::arg("device"));
  m.def("_run_on_stats", &run_on_stats, py::arg("reset") = false);
  m.def("_pipe_stats", &pipe_stats, py::arg("reset") = false);

  // The decoder holds a Python callable: drop it before the interpreter goes.
  py::module_::import("atexit").attr("register")(py::cpp_function([] { set_image_decoder(nullptr); }));

  // fn(path: str, data: numpy int8 | None, from_memory: bool, info: bool)
  //   -> uint8 (H, W, C) array, (w, h) for info, or None.
  m.def("set_image_decoder", [](py::function fn) {
    auto f = hold(std::move(fn));
    set_image_decoder([f](const std::string& path, const std::shared_ptr<Array>& bytes, bool from_memory,
                          bool info) -> std::shared_ptr<Array> {
      py::gil_scoped_acquire gil;
      py::object data = from_memory ? py::object(to_numpy(bytes)) : py::object(py::none());
      py::object r = (*f)(path, data, from_memory, info);
      if (r.is_none()) return nullptr;
      return to_array(r);
    });
  });

  // Test hooks: whether a sample value is still a pending GPU plan.
  m.def("_pending", [](const std::shared_ptr<Buffer>& b, int64_t idx, const std::string& key) {
    Sample s;
    {
      py::gil_scoped_release nogil;
      s = b->get(idx);
    }
    return check_key(s, key)->pending();
  });
  // Test hook: sample `idx` of each buffer merged into one batch, so a batch
  // can hold samples that went through different ops.
  m.def(
      "_merge",
      [](const std::vector<std::shared_ptr<Buffer>>& buffers, int64_t idx, py::object device) {
        DeviceOut dev;
        if (!device.is_none()) dev.device = device.cast<int>();
        Sample out;
        {
          py::gil_scoped_release nogil;
          std::vector<Sample> samples;
          for (const auto& b : buffers) samples.push_back(b->get(idx));
          out = merge_batch(samples, {}, {}, dev);
        }
        return to_dict(out);
      },
      py::arg("buffers"), py::arg("idx") = 0, py::arg("device") = py::none());
  m.def("_plan", [](const std::shared_ptr<Buffer>& b, int64_t idx, const std::string& key) -> py::object {
    Sample s;
    {
      py::gil_scoped_release nogil;
      s = b->get(idx);
    }
    auto a = check_key(s, key);
    if (!a->pending()) return py::none();
    const ImagePlan& p = *a->plan();
    py::dict d;
    d["src_shape"] = p.src->shape();
    d["window"] = py::make_tuple(p.sx, p.sy, p.sw, p.sh);
    d["resize"] = py::make_tuple(p.resize_w, p.resize_h);
    d["crop"] = py::make_tuple(p.crop_x, p.crop_y, p.crop_w, p.crop_h);
    d["flip"] = p.flip;
    d["filter"] = filter_name(p.filter);
    d["shape"] = a->shape();
    if (p.formatted) {
      static const char* const elems[] = {"float32", "float16", "bfloat16"};
      py::dict f;
      f["dtype"] = elems[p.out.elem];
      f["layout"] = p.out.chw() ? "chw" : "hwc";
      f["normalize"] = p.out.normalize;
      f["mean"] = std::vector<float>(p.out.mean.begin(), p.out.mean.end());
      f["std"] = std::vector<float>(p.out.std.begin(), p.out.std.end());
      d["format"] = f;
    } else {
      d["format"] = py::none();
    }
    // the colour matrix as mxd_color holds it: three rows of four, offsets in byte units
    if (p.colored) {
      std::vector<std::vector<float>> rows;
      for (int r = 0; r < 3; r++) rows.emplace_back(p.color.begin() + 4 * r, p.color.begin() + 4 * r + 4);
      d["color"] = rows;
    } else {
      d["color"] = py::none();
    }
    // the tone op: (name, bits / threshold / factor; None for the parameterless ones)
    if (p.toned) {
      py::object arg = py::none();
      if (p.tone_op == MXD_TONE_POSTERIZE || p.tone_op == MXD_TONE_SOLARIZE) arg = py::int_(p.tone_arg);
      else if (p.tone_op == MXD_TONE_CONTRAST) arg = py::float_(p.tone_factor);
      d["tone"] = py::make_tuple(tone_name(p.tone_op), arg);
    } else {
      d["tone"] = py::none();
    }
    // the warp: (resample, (r, g, b), the six entries)
    if (p.warped) {
      d["warp"] = py::make_tuple(resample_name(p.warp_mode), py::make_tuple(p.warp_fill[0], p.warp_fill[1], p.warp_fill[2]),
                                 py::make_tuple(p.warp_m[0], p.warp_m[1], p.warp_m[2], p.warp_m[3], p.warp_m[4], p.warp_m[5]));
    } else {
      d["warp"] = py::none();
    }
    // the enhance op: (name, factor)
    if (p.enhanced) d["enhance"] = py::make_tuple(enhance_name(p.enhance_op), py::float_(p.enhance_factor));
    else d["enhance"] = py::none();
    return d;
  });
}
