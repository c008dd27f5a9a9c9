// tensor.cc -- the non-template parts of the tensor unit: tensors from numpy and from foreign device memory, the class bindings.
#include "tensor.h"

namespace i8ie_py {

// float32 ndarray in pinned host memory: i8ie.tensor() of it (or of a slice of it) uploads asynchronously
py::array_t<float> pinned_empty(std::vector<ssize_t> shape) {
  size_t n = 1;
  for (ssize_t d : shape) {
    if (d < 0) throw std::runtime_error("i8ie: pinned_empty: negative dimension");
    n *= (size_t)d;
  }
  void* p = nullptr;
  check(i8ie_host_malloc(ctx(), std::max<size_t>(n * sizeof(float), 4), &p));
  ppool().user_blocks += 1;
  py::capsule owner(p, [](void* q) {
    if (rt().ctx) i8ie_host_free(rt().ctx, q);
    ppool().user_blocks -= 1;
  });
  return py::array_t<float>(shape, static_cast<float*>(p), owner);
}

Tensor<float> tensor_from_numpy(F32Array a) {
  Tensor<float> t;  // include/tensor.h:40-47: copies the ndarray
  t.shape.assign(a.shape(), a.shape() + a.ndim());
  t.size = a.size();
  t.st = std::make_shared<Storage>();
  t.st->bytes = (size_t)t.size * sizeof(float);
  int pinned = 0;
  if (ppool().user_blocks > 0 && t.st->bytes > 0)
    check(i8ie_host_is_pinned(ctx(), a.data(), t.st->bytes, &pinned));
  if (pinned) {
    // The copy the reference makes at construction becomes an asynchronous upload on the transfer
    // stream; the ndarray must stay unchanged until wait_upload() (or the first read-back) returns.
    Storage& st = *t.st;
    auto& uc = upload_cache()[st.bytes];
    if (!uc.empty()) {
      UploadSlot slot = uc.back();
      uc.pop_back();
      check(i8ie_stream_wait_event(ctx(), slot.free_ev, 1));
      event_put(slot.free_ev);
      st.dev = slot.dev;
    } else {
      check(i8ie_malloc(ctx(), st.bytes, &st.dev));
      // a block fresh from the allocator may still be read by queued compute-stream work
      i8ie_event* e = event_take();
      check(i8ie_event_record(ctx(), e, 0));
      check(i8ie_stream_wait_event(ctx(), e, 1));
      event_put(e);
    }
    st.upload_block = true;
    st.keep = a;
    check(i8ie_memcpy_h2d_async(ctx(), st.dev, a.data(), st.bytes, 1));
    st.ready_ev = event_take();
    check(i8ie_event_record(ctx(), st.ready_ev, 1));
    return t;
  }
  t.st->host.resize(t.st->bytes);
  if (t.st->bytes) std::memcpy(t.st->host.data(), a.data(), t.st->bytes);
  t.st->host_valid = true;
  return t;
}

// Zero-copy view of foreign device memory (a torch tensor's data_ptr(), any hipMalloc block): the tensor reads it
// in place; `owner` is kept alive as long as the tensor (or a reshape view of it) lives.  The memory must be
// complete on this module's stream (share the stream with use_stream(), or synchronise the producer first).
Tensor<float> tensor_from_device(uintptr_t ptr, std::vector<ssize_t> shape, py::object owner) {
  if (ptr == 0 || (ptr & 3u) != 0) throw std::runtime_error("i8ie: tensor_from_device: null or misaligned pointer");
  Tensor<float> t;
  t.shape = std::move(shape);
  t.size = 1;
  for (ssize_t d : t.shape) {
    if (d <= 0) throw std::runtime_error("i8ie: tensor_from_device: non-positive dimension");
    t.size *= d;
  }
  (void)ctx();
  t.st = std::make_shared<Storage>();
  t.st->bytes = (size_t)t.size * sizeof(float);
  t.st->dev = reinterpret_cast<void*>(ptr);
  t.st->external = true;
  t.st->keep = std::move(owner);
  return t;
}

template <typename T>
void bind_tensor(py::module_& m, const char* name) {
  using Fut = typename Tensor<T>::HostFuture;
  py::class_<Fut, std::shared_ptr<Fut>>(m, (std::string(name) + "_HostFuture").c_str())
      .def("done", &Fut::done)
      .def("result", &Fut::result);
  py::class_<Tensor<T>>(m, name)
      .def(py::init<>())
      .def("numpy", &Tensor<T>::numpy)
      .def("numpy_async", &Tensor<T>::numpy_async)
      .def("wait_upload", [](Tensor<T>& t) { if (t.st) t.st->wait_upload_on_host(); })
      .def("zero_point", [](const Tensor<T>& t) { return t.zero_point; })
      .def("scale", [](const Tensor<T>& t) { return t.scale; })
      .def("sum",
           [](Tensor<T>& t) {  // src/pybind11.cc:18-25: sequential fp32 sum
             py::array_t<T> a = t.numpy();
             const T* p = a.data();
             float s = 0;
             for (ssize_t i = 0; i < t.size; ++i) s += p[i];
             return s;
           })
      .def("ref_count",
           [](Tensor<T>& t) {
             t.realize();
             return t.st ? (long)t.st.use_count() : 0L;
           })
      .def("reshape", [](Tensor<T>& t, std::vector<ssize_t> shape) { return t.reshape(std::move(shape)); })
      .def("layout", [](Tensor<T>& t) { t.realize(); return t.st ? t.st->layout : 0; })
      .def("prefetch", [](Tensor<T>& t) { (void)t.dptr(); })
      // device address of the (launched, NCHW-ordered) contents: for __cuda_array_interface__ exports
      .def("data_ptr", [](Tensor<T>& t) { return (uintptr_t)t.dptr(); })
      .def("shape", [](const Tensor<T>& t) { return t.shape; })
      .def("nbytes", [](const Tensor<T>& t) { return (size_t)t.size * sizeof(T); });
}

Tensor<u8_t> pending_u8(std::vector<ssize_t> shape, float scale, u8_t zp) {
  Tensor<u8_t> t;
  t.shape = std::move(shape);
  t.size = 1;
  for (ssize_t d : t.shape) t.size *= d;
  t.scale = scale;
  t.zero_point = zp;
  return t;
}

void bind_tensors(py::module_& m) {
  // the reference registers Tensor<T> under typeid(...).name() (src/pybind11.cc:12)
  bind_tensor<float>(m, "6TensorIfE");
  bind_tensor<u8_t>(m, "6TensorIhE");
  bind_tensor<s8_t>(m, "6TensorIcE");
  py::class_<Tensor<int32_t>>(m, "6TensorIiE").def("numpy", &Tensor<int32_t>::numpy);

  m.def("tensor", &tensor_from_numpy);  // src/pybind11.cc:38-40
  m.def("tensor_from_device", &tensor_from_device);
  // additive (the reference can only default-construct its s8 tensors from Python): an s8 tensor from an ndarray,
  // so that the s8 overloads of relu / max_pool2d can be exercised
  m.def("tensor_s8", [](S8Array a, float scale, int zp) {
    Tensor<s8_t> t(std::vector<ssize_t>(a.shape(), a.shape() + a.ndim()));
    t.scale = scale;
    t.zero_point = (u8_t)zp;
    if (t.size > 0) {
      py::gil_scoped_release nogil;
      check(i8ie_memcpy_h2d(ctx(), t.dptr(), a.data(), (size_t)t.size));
    }
    return t;
  }, py::arg("array"), py::arg("scale") = 1.0f, py::arg("zero_point") = 0);
}

}  // namespace i8ie_py
