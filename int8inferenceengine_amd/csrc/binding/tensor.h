// tensor.h -- PendNode, a recorded launch that every holder shares, and Tensor<T> with its numpy traffic.
#pragma once
#include "runtime.h"

namespace i8ie_py {

using F32Array = py::array_t<float, py::array::c_style | py::array::forcecast>;
using S8Array = py::array_t<s8_t, py::array::c_style | py::array::forcecast>;

// A recorded (not yet launched) operation.  Every holder -- python-side copies of the tensor, relu(y) made from y,
// the closures of consumers that captured their input -- shares ONE node, and the node remembers what it has
// produced: a producer observed twice, or consumed by two ops, launches once per distinct (relu, border) request,
// and its upstream chain (whose nodes cache in the same way) is never launched again.
struct PendNode {
  // arguments: fuse relu; physical border wanted by the consumer; consumer reads re-biased bytes (both honoured for NHWC
  // results of layers whose kernel can; what came out is in the Storage)
  std::function<std::shared_ptr<Storage>(bool, int, bool)> fn;
  // a conv layer whose kernel can fold a following max_pool2d into its epilogue (i8ie_layer_fuses_pool): arguments
  // relu, border of the POOLED result, pool kernel_size, stride; returns null when this launch cannot (the caller
  // then pools the unfused result)
  std::function<std::shared_ptr<Storage>(bool, int, bool, int, int)> fn_pool;
  struct Made {
    bool relu;
    int border;
    std::shared_ptr<Storage> st;
  };
  std::vector<Made> made;
  std::shared_ptr<Storage> get(bool relu, int border, bool s8 = false) {
    for (const Made& m : made)
      if (m.relu == relu && m.border == border && m.st) {
        if (m.st->s8 && !s8) continue;  // (a plain reader does not take the re-biased copy)
        // a bordered NHWC result that was since converted in place (to_nchw) no longer has the border asked for
        if (border > 0 && (m.st->layout != I8IE_LAYOUT_NHWC || m.st->border != border)) continue;
        return m.st;
      }
    std::shared_ptr<Storage> st = fn(relu, border, s8);
    made.push_back(Made{relu, border, st});
    return st;
  }
  // a result already produced for this relu, whatever border / re-bias it was asked with: for a consumer that reads its
  // operand as it lies (add), so that a producer launched for another consumer is not launched a second time
  std::shared_ptr<Storage> find_any(bool relu) const {
    for (const Made& m : made)
      if (m.relu == relu && m.st) return m.st;
    return nullptr;
  }
  // the pending producers this node reads (none once they have launched): lets a two-operand consumer launch the operand
  // that is downstream of the other one first
  std::vector<std::weak_ptr<PendNode>> inputs;
  bool reads(const PendNode* target) const {
    for (const auto& w : inputs)
      if (auto n = w.lock()) {
        if (n.get() == target) return true;
        if (n->made.empty() && n->reads(target)) return true;
      }
    return false;
  }
};
template <typename F>
std::shared_ptr<PendNode> make_pend(F&& f, std::initializer_list<std::shared_ptr<PendNode>> inputs = {}) {
  auto n = std::make_shared<PendNode>();
  n->fn = std::forward<F>(f);
  for (const auto& i : inputs)
    if (i) n->inputs.push_back(i);
  return n;
}

// ----------------------------------------------------------------- tensor ----
template <typename T>
struct Tensor {
  std::shared_ptr<Storage> st;
  std::vector<ssize_t> shape;
  ssize_t size = 0;
  float scale = 1;      // include/tensor.h:153
  u8_t zero_point = 0;  // include/tensor.h:154
  // A layer forward that has been recorded but not launched yet: lets a following relu
  // fold into the epilogue.  Launching is observationally identical to the eager call.
  // arguments: fuse relu; physical border wanted by the consumer (honoured for NHWC results)
  std::shared_ptr<PendNode> pend;
  bool pend_relu = false;
  // a pending small Linear layer can also produce dequantize(layer(x)) directly (argument: fuse relu)
  std::shared_ptr<std::function<std::shared_ptr<Storage>(bool)>> pend_f32;
  // set while this tensor is a not-yet-launched quantize(x, scale, zp): lets the first conv read x directly
  std::shared_ptr<Storage> qsrc;
  float qscale = 0;
  u8_t qzp = 0;

  void adopt(std::shared_ptr<Storage> s) {  // takes a launched result: nothing is pending on this tensor any more
    st = std::move(s);
    pend.reset();
    pend_f32.reset();
    qsrc.reset();
  }
  void realize(int border = 0, bool s8 = false) {
    if (pend) adopt(pend->get(pend_relu, border, s8));
  }

  Tensor() = default;
  explicit Tensor(std::vector<ssize_t> shp) : shape(std::move(shp)) {
    size = 1;
    for (ssize_t d : shape) size *= d;
    st = device_storage((size_t)size * sizeof(T));
  }
  T* dptr() {  // NCHW / row-major bytes, as the reference lays them out
    realize();
    if (!st) throw std::runtime_error("i8ie: empty tensor");
    st->to_nchw();
    return static_cast<T*>(st->device_ptr());
  }
  T* dptr_any() {  // whatever layout the storage is in (see st->layout), plain bytes
    realize();
    if (!st) throw std::runtime_error("i8ie: empty tensor");
    T* p = static_cast<T*>(st->device_ptr());
    st->unbias();
    return p;
  }
  T* dptr_raw() {  // ... as it is, re-biased or not (st->s8): for consumers that take I8IE_LAYOUT_NHWC_S8
    if (!st) throw std::runtime_error("i8ie: empty tensor");
    return static_cast<T*>(st->device_ptr());
  }
  py::array_t<T> numpy() {
    realize();
    py::array_t<T> out(shape);
    if (st && size > 0) {
      st->to_nchw();
      st->read_back(out.mutable_data());
    }
    return out;
  }
  struct HostFuture;
  std::shared_ptr<HostFuture> numpy_async();
  // include/tensor.h:106-133: at most one -1, no zeros, sizes must match
  Tensor<T> reshape(std::vector<ssize_t> shp) {
    realize();
    // Views are defined on the reference's element order, so the buffer goes back to NCHW here -- except for the
    // flatten x.reshape(n, -1) of a border-free NHWC activation: that view is converted only if its bytes are
    // observed (dptr() / numpy()); a Linear layer reads it as it lies (K walked in (h, w, c) order).  Any other
    // new shape would disagree with the storage's logical dims for the layout-aware consumers.
    const bool flatten = st && st->layout == I8IE_LAYOUT_NHWC && st->border == 0 && shp.size() == 2 &&
                         (shp[0] == st->dn || (shp[0] < 0 && shp[1] == (ssize_t)st->dc * st->dh * st->dw) ||
                          (shp[1] < 0 && shp[0] == st->dn));
    if (st && !flatten) st->to_nchw();
    ssize_t midx = -1, sz = 1;
    for (size_t i = 0; i < shp.size(); ++i) {
      if (shp[i] < 0) {
        if (midx != -1) throw std::runtime_error("i8ie: reshape: more than one negative dimension");
        midx = (ssize_t)i;
      } else if (shp[i] == 0) {
        throw std::runtime_error("i8ie: reshape: zero dimension");
      } else {
        sz *= shp[i];
      }
    }
    if (midx >= 0) {
      if (size % sz != 0) throw std::runtime_error("i8ie: reshape: size is not divisible");
      shp[midx] = size / sz;
      sz *= shp[midx];
    }
    if (sz != size) throw std::runtime_error("i8ie: reshape: element count differs");
    Tensor<T> v;
    v.st = st;
    v.shape = std::move(shp);
    v.size = size;
    v.scale = scale;
    v.zero_point = zero_point;
    return v;
  }
};

// numpy() split in two: the device->host copy is queued behind the tensor's kernels into pinned staging
// memory and result() waits for it, so the caller can launch the next batch in between.
template <typename T>
struct Tensor<T>::HostFuture {
  std::vector<ssize_t> shape;
  size_t bytes = 0, cap = 0;
  void* buf = nullptr;
  i8ie_event* ev = nullptr;
  py::object ready;  // already on the host
  HostFuture() = default;
  HostFuture(const HostFuture&) = delete;
  HostFuture& operator=(const HostFuture&) = delete;
  bool done() {
    if (!ev) return true;
    int d = 0;
    check(i8ie_event_query(ev, &d));
    return d != 0;
  }
  py::object result() {
    if (ready) return ready;
    if (ev) {
      py::gil_scoped_release nogil;
      check(i8ie_event_synchronize(ev));
    }
    py::array_t<T> out(shape);
    if (bytes) std::memcpy(out.mutable_data(), buf, bytes);
    release();
    ready = out;
    return ready;
  }
  void release() {
    if (ev) event_put(ev);
    if (buf) pinned_put(buf, cap);
    ev = nullptr;
    buf = nullptr;
  }
  ~HostFuture() {
    if (!rt().ctx) return;
    if (ev) i8ie_event_synchronize(ev);  // the copy may still be writing the staging block
    release();
  }
};
template <typename T>
std::shared_ptr<typename Tensor<T>::HostFuture> Tensor<T>::numpy_async() {
  realize();
  auto f = std::make_shared<HostFuture>();
  f->shape = shape;
  if (!st || size == 0 || st->host_valid) {
    f->ready = numpy();
    return f;
  }
  st->to_nchw();
  f->bytes = (size_t)size * sizeof(T);
  f->cap = pinned_capacity(f->bytes);
  f->buf = pinned_take(f->cap);
  check(i8ie_memcpy_d2h_async(ctx(), f->buf, st->device_ptr(), f->bytes, 0));
  f->ev = event_take();
  check(i8ie_event_record(ctx(), f->ev, 0));
  return f;
}

// A u8 result that is still to be produced (recorded, or written by the caller): shape, element count and quantisation
// parameters, no storage yet.
Tensor<u8_t> pending_u8(std::vector<ssize_t> shape, float scale, u8_t zp);
// float32 ndarray in pinned host memory: i8ie.tensor() of it (or of a slice of it) uploads asynchronously
py::array_t<float> pinned_empty(std::vector<ssize_t> shape);
void bind_tensors(py::module_& m);  // the four tensor classes, tensor, tensor_from_device, tensor_s8

}  // namespace i8ie_py
