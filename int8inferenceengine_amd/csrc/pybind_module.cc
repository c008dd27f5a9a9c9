// pybind_module.cc -- the rebuilt extension module `_CXX_i8ie`.
//
// Same Python-visible surface as the reference's module (src/pybind11.cc:37-55,
// declare_linear src/fully_connected.cc:54-72, declare_conv2d
// src/conv2d.cc:144-165, declare_tensor_funcs src/functional.cc:66-82), but
// every tensor lives in MI355X HBM and every op is a HIP kernel reached through
// the C-ABI of libi8ie_hip.so (include/i8ie_hip.h).  This file contains no HIP
// code and no arithmetic of the hot path: only ownership, shapes, the
// prepare/convert state machine (src/layer.cc:28-54) and the calibrator
// (src/calibrator.cc).  There is no CPU fallback: if the library or a GPU is
// missing, calls raise RuntimeError.
//
// Additive API (not in the reference; needed for parity tests and benchmarks):
//   layer.set_output_qparams(scale, zp) / output_qparams() / q_weight() /
//   q_bias() / weight_scale() / forward_debug(u8 tensor) -> (out, int32 acc);
//   tensor.prefetch();  module: set_device, device, synchronize, memory_stats,
//   set_calibration_seed, abi_version.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "i8ie_hip.h"
#include "pybind11/numpy.h"
#include "pybind11/pybind11.h"
#include "pybind11/stl.h"

namespace py = pybind11;
using u8_t = unsigned char;
using s8_t = signed char;

namespace {

// ---------------------------------------------------------------- runtime ----
struct Runtime {
  i8ie_ctx* ctx = nullptr;
  int device = -1;
  long calib_seed = -1;  // < 0: std::random_device, as the reference (src/calibrator.cc:9-10)
  int calib_mode = 0;    // 0 auto: seeded -> the reference's mt19937 stream replayed on the host (golden-pinned),
                         // unseeded -> sampled on the device (no D2H of the layer outputs); 1 host; 2 device
};
Runtime& rt() {
  static Runtime* r = new Runtime();  // intentionally leaked: outlives every tensor at exit
  return *r;
}
void check(int rc) {
  if (rc != I8IE_OK) throw std::runtime_error(std::string("i8ie: ") + i8ie_last_error());
}
int default_device() {
  if (const char* e = std::getenv("I8IE_DEVICE")) return std::atoi(e);
  if (const char* e = std::getenv("LOCAL_RANK")) return std::atoi(e);  // one process per GPU
  return 0;
}
i8ie_ctx* ctx() {
  Runtime& r = rt();
  if (!r.ctx) {
    if (r.device < 0) r.device = default_device();
    check(i8ie_ctx_create(r.device, &r.ctx));
  }
  return r.ctx;
}

// ---------------------------------------------------------------- storage ----
// One buffer shared by a tensor and its reshape views (the role of the
// py::capsule in include/tensor.h:28,94-104).  A host mirror is kept for
// tensors that came from numpy so that small host-side round trips
// (argmax / == / sum in i8ie/__init__.py) do not touch the device.
struct Storage;
// Bordered NHWC buffers whose border bytes already hold the zero point, keyed by geometry: a network that
// runs the same shapes again gets them back and skips the border fill (kernels only write interiors).
struct BorderKey {
  size_t bytes;
  int n, c, h, w, b, zp;
  bool operator<(const BorderKey& o) const {
    return std::tie(bytes, n, c, h, w, b, zp) < std::tie(o.bytes, o.n, o.c, o.h, o.w, o.b, o.zp);
  }
};
std::map<BorderKey, std::vector<void*>>& border_cache() {
  static auto* m = new std::map<BorderKey, std::vector<void*>>();
  return *m;
}

// ---- pinned host staging, events and upload blocks (asynchronous transfers) ----
struct PinnedPool {
  std::map<size_t, std::vector<void*>> free_blocks;  // by capacity (multiples of 4 KiB)
  std::vector<i8ie_event*> events;
  size_t user_blocks = 0;  // live pinned_empty() arrays
};
PinnedPool& ppool() {
  static auto* p = new PinnedPool();
  return *p;
}
size_t pinned_capacity(size_t bytes) { return (bytes + 4095) & ~(size_t)4095; }
void* pinned_take(size_t cap) {
  auto& v = ppool().free_blocks[cap];
  if (!v.empty()) {
    void* p = v.back();
    v.pop_back();
    return p;
  }
  void* p = nullptr;
  check(i8ie_host_malloc(ctx(), cap, &p));
  return p;
}
void pinned_put(void* p, size_t cap) {
  auto& v = ppool().free_blocks[cap];
  if (v.size() < 8) v.push_back(p);
  else i8ie_host_free(ctx(), p);
}
i8ie_event* event_take() {
  auto& v = ppool().events;
  if (!v.empty()) {
    i8ie_event* e = v.back();
    v.pop_back();
    return e;
  }
  i8ie_event* e = nullptr;
  check(i8ie_event_create(ctx(), &e));
  return e;
}
void event_put(i8ie_event* e) { ppool().events.push_back(e); }
// Device blocks written by the transfer stream.  They bypass the stream-ordered allocator (whose reuse
// rule only covers the compute stream): a block comes back with an event recorded behind its last
// compute-stream reader, and the next upload into it makes the transfer stream wait for that event.
struct UploadSlot {
  void* dev;
  i8ie_event* free_ev;
};
std::map<size_t, std::vector<UploadSlot>>& upload_cache() {
  static auto* m = new std::map<size_t, std::vector<UploadSlot>>();
  return *m;
}

struct Storage {
  size_t bytes = 0;
  void* dev = nullptr;
  i8ie_event* ready_ev = nullptr;  // recorded on the transfer stream behind the upload into `dev`
  bool upload_block = false;       // `dev` belongs to upload_cache()
  bool external = false;           // `dev` is foreign HIP memory (e.g. a torch tensor's): never freed here
  py::object keep;                 // the pinned ndarray an asynchronous upload reads from / the foreign owner
  int bzp = -1;  // >= 0: bordered NHWC buffer with border bytes == bzp, the physical byte (returns to border_cache)
  std::vector<unsigned char> host;
  bool host_valid = false;
  // physical layout of a 4-D u8 activation: the engine keeps NHWC between layers and
  // converts back to the reference's NCHW only when the bytes are observed
  int layout = I8IE_LAYOUT_NCHW;
  int border = 0;                      // NHWC only: physical border (pixels) holding the zero point
  bool s8 = false;                     // NHWC only: bytes stored re-biased (^0x80, I8IE_LAYOUT_NHWC_S8; border: zp ^ 0x80)
  int dn = 0, dc = 0, dh = 0, dw = 0;  // logical NCHW dims, valid when layout == NHWC
  void set_nhwc(const std::vector<ssize_t>& shp, int b) {
    layout = I8IE_LAYOUT_NHWC;
    border = b;
    dn = (int)shp[0]; dc = (int)shp[1]; dh = (int)shp[2]; dw = (int)shp[3];
  }
  void unbias() {  // re-biased bytes -> plain u8, in place (border bytes become the zero point again)
    if (!s8 || !dev) return;
    check(i8ie_rebias_u8(ctx(), (const uint8_t*)dev, (uint8_t*)dev, (int64_t)bytes));
    s8 = false;
    if (bzp >= 0) bzp ^= 0x80;
  }
  void to_nchw() {
    if (layout == I8IE_LAYOUT_NCHW || external) return;
    unbias();
    void* fresh = nullptr;
    const size_t logical = (size_t)dn * dc * dh * dw;
    check(i8ie_malloc(ctx(), logical, &fresh));
    check(i8ie_layout_convert_u8(ctx(), (const uint8_t*)dev, (uint8_t*)fresh, dn, dc, dh, dw, 0, border, 0));
    i8ie_free(ctx(), dev);  // stream-ordered: the conversion above still reads it, reuse is queued behind
    dev = fresh;
    bytes = logical;
    layout = I8IE_LAYOUT_NCHW;
    border = 0;
    bzp = -1;
  }
  void wait_upload_on_stream() {  // the compute stream waits (device side) for the upload
    if (!ready_ev) return;
    check(i8ie_stream_wait_event(ctx(), ready_ev, 0));
    event_put(ready_ev);
    ready_ev = nullptr;
    keep = py::object();
  }
  void wait_upload_on_host() {
    if (!ready_ev) return;
    {
      py::gil_scoped_release nogil;
      check(i8ie_event_synchronize(ready_ev));
    }
    keep = py::object();  // the source may be refilled; the compute stream still has to wait on the event
  }
  ~Storage() {
    if (external) return;  // the owner object in `keep` frees it
    if (!dev || !rt().ctx) return;
    if (ready_ev) {  // never consumed: let the copy finish before the block is reused
      i8ie_stream_wait_event(rt().ctx, ready_ev, 0);
      event_put(ready_ev);
      ready_ev = nullptr;
    }
    int capturing = 0;  // a graph being captured has this address baked in: the block goes to the graph
    i8ie_ctx_is_capturing(rt().ctx, &capturing);  // (i8ie_free hands it over), never to a cache of ours
    if (upload_block && !capturing) {
      auto& slot = upload_cache()[bytes];
      if (slot.size() < 4) {
        i8ie_event* e = event_take();
        i8ie_event_record(rt().ctx, e, 0);
        slot.push_back(UploadSlot{dev, e});
        return;
      }
    }
    if (bzp >= 0 && layout == I8IE_LAYOUT_NHWC && border > 0 && !capturing) {
      auto& slot = border_cache()[BorderKey{bytes, dn, dc, dh, dw, border, bzp}];
      if (slot.size() < 4) {
        slot.push_back(dev);
        return;
      }
    }
    i8ie_free(rt().ctx, dev);
  }
  void* device_ptr() {
    if (ready_ev) wait_upload_on_stream();
    if (!dev) {
      check(i8ie_malloc(ctx(), bytes, &dev));
      if (host_valid) {
        py::gil_scoped_release nogil;
        check(i8ie_memcpy_h2d(ctx(), dev, host.data(), bytes));
      }
      if (bytes > (1u << 20)) {  // keep the mirror only for small tensors
        std::vector<unsigned char>().swap(host);
        host_valid = false;
      }
    }
    return dev;
  }
  void read_back(void* dst) {
    if (ready_ev) wait_upload_on_stream();
    if (host_valid) {
      std::memcpy(dst, host.data(), bytes);
      return;
    }
    py::gil_scoped_release nogil;
    check(i8ie_memcpy_d2h(ctx(), dst, dev, bytes));
  }
};

std::shared_ptr<Storage> device_storage(size_t bytes) {
  auto s = std::make_shared<Storage>();
  s->bytes = bytes;
  check(i8ie_malloc(ctx(), bytes, &s->dev));
  return s;
}

// NHWC u8 storage for logical shape `shp` (NCHW order) with a border of b pixels holding zp (s8: the bytes of this
// tensor are stored re-biased, I8IE_LAYOUT_NHWC_S8, so its border holds zp ^ 0x80)
std::shared_ptr<Storage> nhwc_storage(const std::vector<ssize_t>& shp, int b, int zp, bool s8 = false) {
  const size_t bytes = (size_t)shp[0] * shp[1] * (shp[2] + 2 * b) * (shp[3] + 2 * b);
  if (s8) zp ^= 0x80;
  if (b <= 0) {
    auto s = device_storage(bytes);
    s->set_nhwc(shp, 0);
    s->s8 = s8;
    return s;
  }
  auto s = std::make_shared<Storage>();
  s->bytes = bytes;
  s->set_nhwc(shp, b);
  s->s8 = s8;
  s->bzp = zp;
  auto it = border_cache().find(BorderKey{bytes, s->dn, s->dc, s->dh, s->dw, b, zp});
  if (it != border_cache().end() && !it->second.empty()) {
    s->dev = it->second.back();  // border still valid from its previous life
    it->second.pop_back();
    return s;
  }
  check(i8ie_malloc(ctx(), bytes, &s->dev));
  check(i8ie_fill_border_u8(ctx(), (uint8_t*)s->dev, s->dn, s->dc, s->dh, s->dw, b, (uint8_t)zp));
  return s;
}

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

Tensor<float> tensor_from_numpy(py::array_t<float, py::array::c_style | py::array::forcecast> a) {
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

// A u8 result that is still to be produced (recorded, or written by the caller): shape, element count and quantisation
// parameters, no storage yet.
Tensor<u8_t> pending_u8(std::vector<ssize_t> shape, float scale, u8_t zp) {
  Tensor<u8_t> t;
  t.shape = std::move(shape);
  t.size = 1;
  for (ssize_t d : t.shape) t.size *= d;
  t.scale = scale;
  t.zero_point = zp;
  return t;
}
void check_zero_point(int zp) {
  if (zp < 0 || zp > 255) throw std::runtime_error("i8ie: zero point must be in [0, 255]");
}
// the result's quantisation parameters as a caller of add / mul / cat / lut gave them
void check_out_qparams(const char* op, float scale, int zp) {
  check_zero_point(zp);
  if (!(scale > 0) || !std::isfinite(scale)) throw std::runtime_error(std::string("i8ie: ") + op + ": the output scale must be positive and finite");
}

// ------------------------------------------------------------ elementwise ----
Tensor<u8_t> quantize(Tensor<float>& in, float scale, u8_t zp) {  // src/quantize_utils.cc:44-52
  Tensor<u8_t> out = pending_u8(in.shape, scale, zp);
  (void)in.dptr();  // make sure the FP32 source is on the device
  std::shared_ptr<Storage> src = in.st;
  const ssize_t n = in.size;
  out.qsrc = src;
  out.qscale = scale;
  out.qzp = zp;
  // deferred: a first conv layer that accepts FP32 input consumes `src` directly (fused quantize)
  out.pend = make_pend(
      [src, n, scale, zp](bool relu, int, bool) {
        auto st = device_storage((size_t)n);
        check(i8ie_quantize_f32_u8(ctx(), (const float*)src->device_ptr(), (uint8_t*)st->dev, n, scale, zp));
        if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, n, zp));
        return st;
      });
  return out;
}
Tensor<float> dequantize(Tensor<u8_t>& in) {  // src/quantize_utils.cc:54-58
  if (in.pend && in.pend_f32) {  // classifier head still pending: layer + (relu) + dequantize in one launch
    Tensor<float> out;
    out.shape = in.shape;
    out.size = in.size;
    out.st = (*in.pend_f32)(in.pend_relu);
    return out;
  }
  Tensor<float> out(in.shape);
  check(i8ie_dequantize_u8_f32(ctx(), in.dptr(), out.dptr(), in.size, in.scale, in.zero_point));
  return out;
}
Tensor<u8_t> relu_u8(Tensor<u8_t>& in) {  // src/functional.cc:15-26
  if (in.pend && !in.pend_relu) {
    // `in` is a layer output that has not been launched: record layer+relu as one launch.
    // `in` itself stays pending (if it is ever observed it launches without the relu).
    Tensor<u8_t> out = pending_u8(in.shape, in.scale, in.zero_point);
    out.pend = in.pend;
    out.pend_f32 = in.pend_f32;
    out.pend_relu = true;  // (qsrc is not carried over: relu(quantize(x)) is not a plain quantize)
    return out;
  }
  const uint8_t* src = in.shape.size() == 4 ? in.dptr_any() : in.dptr();
  Tensor<u8_t> out(in.shape);
  out.scale = in.scale;
  out.zero_point = in.zero_point;
  if (in.st->layout == I8IE_LAYOUT_NHWC) {  // elementwise over the physical buffer (border bytes = zp stay zp)
    out.st = device_storage(in.st->bytes);
    out.st->set_nhwc(in.shape, in.st->border);
  }
  check(i8ie_relu_u8(ctx(), src, (uint8_t*)out.st->dev, (int64_t)in.st->bytes, in.zero_point));
  return out;
}
Tensor<float> relu_f32(Tensor<float>& in) {  // src/functional.cc:5-13
  Tensor<float> out(in.shape);
  check(i8ie_relu_f32(ctx(), in.dptr(), out.dptr(), in.size));
  return out;
}
template <typename T>
std::vector<ssize_t> pool_shape(const Tensor<T>& in, ssize_t k, ssize_t s) {
  if (in.shape.size() != 4) throw std::runtime_error("i8ie: max_pool2d expects an NCHW tensor");
  if (k <= 0 || s <= 0) throw std::runtime_error("i8ie: max_pool2d: kernel_size and stride must be positive");
  if (k > in.shape[2] || k > in.shape[3]) throw std::runtime_error("i8ie: max_pool2d: window larger than input");
  return {in.shape[0], in.shape[1], (in.shape[2] - k) / s + 1, (in.shape[3] - k) / s + 1};
}
Tensor<u8_t> max_pool2d_u8(Tensor<u8_t>& in, ssize_t k, ssize_t s) {  // src/functional.cc:36-64
  Tensor<u8_t> out = pending_u8(pool_shape(in, k, s), in.scale, in.zero_point);
  Tensor<u8_t> src = in;
  const std::vector<ssize_t> ishp = in.shape, oshp = out.shape;
  const u8_t zp = in.zero_point;
  const int kk = (int)k, ss = (int)s;
  // deferred so that a consuming conv can ask for a zero-point border around the result
  out.pend = make_pend(
      [src, ishp, oshp, zp, kk, ss](bool relu, int border, bool s8) mutable {
        if (src.pend && src.pend->fn_pool && src.pend.use_count() == 1 && src.pend->made.empty()) {
          // relu(layer(x)) still pending, nobody else holds it (no second consumer, not observable any more), and its
          // kernel pools in the epilogue: one launch, no unpooled tensor.  With another holder the layer launches once,
          // unfused, and every consumer reads that result (a recorded launch never runs twice).
          // (a relu behind the pool folds in as well: max-pool and relu commute, both are monotone)
          std::shared_ptr<Storage> st = src.pend->fn_pool(src.pend_relu || relu, border, s8, kk, ss);
          if (st) return st;
        }
        const uint8_t* ip = src.dptr_any();
        std::shared_ptr<Storage> st;
        const size_t logical = (size_t)oshp[0] * oshp[1] * oshp[2] * oshp[3];
        if (src.st->layout == I8IE_LAYOUT_NHWC && ishp[1] % 16 == 0) {
          st = nhwc_storage(oshp, border, zp);
          check(i8ie_maxpool2d_u8_nhwc(ctx(), ip, src.st->border, (uint8_t*)st->dev, border, (int)ishp[0], (int)ishp[1],
                                       (int)ishp[2], (int)ishp[3], kk, ss));
        } else {
          st = device_storage(logical);
          check(i8ie_maxpool2d_u8(ctx(), src.dptr(), (uint8_t*)st->dev, (int)ishp[0], (int)ishp[1], (int)ishp[2],
                                  (int)ishp[3], kk, ss));
        }
        if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        return st;
      }, {in.pend});
  return out;
}

// ---- add (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_add_u8) ----------------------------
Tensor<float> add_f32(Tensor<float>& a, Tensor<float>& b) {
  if (a.shape != b.shape) throw std::runtime_error("i8ie: add: shapes differ (there is no broadcasting)");
  Tensor<float> out(a.shape);
  check(i8ie_add_f32(ctx(), a.dptr(), b.dptr(), out.dptr(), a.size));
  return out;
}
// ---- the operand rules of the deferred joining ops (add, mul, cat, lut, avg_pool2d) ----------------
// The storage an operand is read from, as it lies (any layout, border, re-bias).  A producer that has launched for another
// consumer -- the skip tensor, made bordered / re-biased for the first conv of the block -- is taken from its node's results;
// one that has not launches plain.
std::shared_ptr<Storage> operand_as_it_lies(Tensor<u8_t>& t) {
  if (t.pend) {
    if (auto st = t.pend->find_any(t.pend_relu)) t.adopt(st);
    else t.realize();
  }
  if (!t.st) throw std::runtime_error("i8ie: empty tensor");
  t.st->device_ptr();  // (uploads a host-made tensor, waits for an asynchronous upload)
  return t.st;
}
// `t` must not launch before `reader`: both are pending and reader = f(t) has not launched.  Launching the reader launches t
// for f (bordered as f wants it), and t is then found among its node's results instead of launching a second time, plain.
bool waits_for(const Tensor<u8_t>& t, const Tensor<u8_t>& reader) {
  return t.pend && reader.pend && reader.pend != t.pend && reader.pend->made.empty() && reader.pend->reads(t.pend.get());
}
// The storages of k operands, as they lie: each round launches the first unresolved operand that waits for no other unresolved
// one.  Two operands: b goes first exactly when waits_for(a, b) -- a then finds waits_for(b, a) false, which a cycle alone could
// make true, and a cycle cannot be recorded -- and a goes first otherwise.
std::vector<std::shared_ptr<Storage>> resolve_operands(Tensor<u8_t>* ts, size_t k) {
  std::vector<std::shared_ptr<Storage>> ss(k);
  for (size_t round = 0; round < k; ++round) {
    size_t pick = k;
    for (size_t i = 0; i < k && pick == k; ++i) {
      if (ss[i]) continue;
      bool is_read = false;
      for (size_t j = 0; j < k && !is_read; ++j) is_read = j != i && !ss[j] && waits_for(ts[i], ts[j]);
      if (!is_read) pick = i;
    }
    if (pick == k) pick = (size_t)(std::find(ss.begin(), ss.end(), nullptr) - ss.begin());  // (a cycle cannot be recorded)
    ss[pick] = operand_as_it_lies(ts[pick]);
  }
  return ss;
}
// NCHW operands converted for one launch: (source, its NHWC copy).  Lives as long as the launch is being queued.
using NhwcCopies = std::vector<std::pair<std::shared_ptr<Storage>, std::shared_ptr<Storage>>>;
// A rank-4 operand in the engine's layout under the logical dims `shp`.  A view whose storage is NHWC under other logical dims
// goes back to the reference's order first (the view is defined on it); an NCHW tensor (user-made) takes one conversion into a
// temporary that `copies` keeps alive, and the same storage coming again gets the same copy.
std::shared_ptr<Storage> as_engine_nhwc(const std::shared_ptr<Storage>& s, const std::vector<ssize_t>& shp, NhwcCopies& copies) {
  if (s->layout == I8IE_LAYOUT_NHWC && (s->dn != shp[0] || s->dc != shp[1] || s->dh != shp[2] || s->dw != shp[3])) s->to_nchw();
  if (s->layout == I8IE_LAYOUT_NHWC) return s;
  for (const auto& c : copies)
    if (c.first == s) return c.second;
  auto tmp = device_storage((size_t)(shp[0] * shp[1] * shp[2] * shp[3]));
  tmp->set_nhwc(shp, 0);
  check(i8ie_layout_convert_u8(ctx(), (const uint8_t*)s->device_ptr(), (uint8_t*)tmp->dev, (int)shp[0], (int)shp[1], (int)shp[2],
                               (int)shp[3], 1, 0, 0));
  copies.emplace_back(s, tmp);
  return tmp;
}
// Two operands of one shape brought to one layout (add, the equal-shape mul).  Operands that agree stay as they lie: two NCHW
// tensors take the flat form.  Rank 4 otherwise: the engine keeps NHWC between layers (and a consumer that asked for a border
// reads NHWC).  Other ranks -- a flattened NHWC activation against plain rows -- both back to the reference's order.
void reconcile_pair(std::shared_ptr<Storage>& sa, std::shared_ptr<Storage>& sb, const std::vector<ssize_t>& shp, NhwcCopies& copies) {
  const bool same_dims = sa->dn == sb->dn && sa->dc == sb->dc && sa->dh == sb->dh && sa->dw == sb->dw;
  if (sa->layout == sb->layout && (sa->layout == I8IE_LAYOUT_NCHW || same_dims)) return;
  if (shp.size() == 4) {
    sa = as_engine_nhwc(sa, shp, copies);
    sb = as_engine_nhwc(sb, shp, copies);
  } else {
    sa->to_nchw();
    sb->to_nchw();
  }
}

// The deferred result of a two-operand op on operands of one shape (add, the equal-shape mul), through the op's flat and NHWC
// C entries.  Deferred like max_pool2d's result: relu(op(..)) is one launch, and a consuming conv gets its zero-point border
// and, where it reads them, re-biased bytes straight from the op's kernel.  The caller has checked its arguments.
using PairFlatFn = decltype(&i8ie_add_u8);
using PairNhwcFn = decltype(&i8ie_add_u8_nhwc);
Tensor<u8_t> equal_shape_u8(PairFlatFn flat, PairNhwcFn nhwc, Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp) {
  Tensor<u8_t> out = pending_u8(a.shape, scale, (u8_t)zp);
  std::array<Tensor<u8_t>, 2> ops{a, b};  // share the operands' storage / pending launches
  const float s_a = a.scale, s_b = b.scale;
  const u8_t zp_a = a.zero_point, zp_b = b.zero_point, zp_o = (u8_t)zp;
  const std::vector<ssize_t> shp = a.shape;
  const ssize_t n = a.size;
  out.pend = make_pend(
      [flat, nhwc, ops, s_a, s_b, zp_a, zp_b, scale, zp_o, shp, n](bool relu, int border, bool s8) mutable {
        auto ss = resolve_operands(ops.data(), 2);
        NhwcCopies copies;
        reconcile_pair(ss[0], ss[1], shp, copies);
        Storage *sa = ss[0].get(), *sb = ss[1].get();
        std::shared_ptr<Storage> st;
        if (sa->layout == I8IE_LAYOUT_NHWC) {
          st = nhwc_storage({sa->dn, sa->dc, sa->dh, sa->dw}, shp.size() == 4 ? border : 0, zp_o, s8);
          check(nhwc(ctx(), (const uint8_t*)sa->device_ptr(), sa->border, sa->s8 ? 1 : 0, (const uint8_t*)sb->device_ptr(), sb->border,
                     sb->s8 ? 1 : 0, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0, sa->dn, sa->dc, sa->dh, sa->dw, s_a, zp_a, s_b, zp_b,
                     scale, zp_o, relu ? 1 : 0));
        } else {
          st = device_storage((size_t)n);
          check(flat(ctx(), (const uint8_t*)sa->device_ptr(), (const uint8_t*)sb->device_ptr(), (uint8_t*)st->dev, (int64_t)n, s_a, zp_a,
                     s_b, zp_b, scale, zp_o, relu ? 1 : 0));
        }
        // (the operands are released with the closure's copies, as a layer's input is)
        return st;
      }, {a.pend, b.pend});
  return out;
}
Tensor<u8_t> add_u8(Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp) {
  if (a.shape != b.shape) throw std::runtime_error("i8ie: add: shapes differ (there is no broadcasting)");
  check_out_qparams("add", scale, zp);  // (add alone checks neither the operands' scales nor for an empty tensor)
  return equal_shape_u8(i8ie_add_u8, i8ie_add_u8_nhwc, a, b, scale, zp);
}
// ---- mul (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_mul_u8) ----------------------------
// b has a's shape (false), or is a gate [n, c, 1, 1] / [n, c] of a rank-4 a (true); anything else is a RuntimeError
// (before any device call).  Only the second operand broadcasts.
template <typename T>
bool mul_is_gate(const Tensor<T>& a, const Tensor<T>& b) {
  if (a.shape.size() != 2 && a.shape.size() != 4) throw std::runtime_error("i8ie: mul: the first operand must be [n, c, h, w] or [m, f]");
  for (ssize_t d : a.shape)
    if (d <= 0) throw std::runtime_error("i8ie: mul: empty tensor");
  if (a.shape == b.shape) return false;
  const bool gate = a.shape.size() == 4 && b.shape.size() >= 2 && b.shape[0] == a.shape[0] && b.shape[1] == a.shape[1] &&
                    (b.shape.size() == 2 || (b.shape.size() == 4 && b.shape[2] == 1 && b.shape[3] == 1));
  if (!gate)
    throw std::runtime_error("i8ie: mul: the second operand must have the first one's shape or be its gate [n, c, 1, 1] / [n, c] "
                             "(no other broadcasting)");
  return true;
}
Tensor<float> mul_f32(Tensor<float>& a, Tensor<float>& b) {
  const bool gate = mul_is_gate(a, b);
  Tensor<float> out(a.shape);
  check(i8ie_mul_f32(ctx(), a.dptr(), b.dptr(), out.dptr(), a.size, gate ? (int64_t)(a.shape[2] * a.shape[3]) : 0));
  return out;
}
// i8ie_mul_u8_nhwc on operands of one shape, with the add's argument list
int mul_u8_nhwc_equal(i8ie_ctx* c, const uint8_t* a, int a_border, int a_s8, const uint8_t* b, int b_border, int b_s8, uint8_t* out,
                      int out_border, int out_s8, int n, int ch, int h, int w, float s_a, uint8_t zp_a, float s_b, uint8_t zp_b,
                      float s_out, uint8_t zp_out, int relu) {
  return i8ie_mul_u8_nhwc(c, a, a_border, a_s8, b, b_border, b_s8, 0, out, out_border, out_s8, n, ch, h, w, s_a, zp_a, s_b, zp_b, s_out,
                          zp_out, relu);
}
Tensor<u8_t> mul_u8(Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp) {
  const bool gate = mul_is_gate(a, b);
  check_out_qparams("mul", scale, zp);
  if (!std::isfinite(a.scale) || !std::isfinite(b.scale)) throw std::runtime_error("i8ie: mul: an operand's scale is not finite");
  if ((!a.st && !a.pend) || (!b.st && !b.pend)) throw std::runtime_error("i8ie: empty tensor");
  if (!gate) return equal_shape_u8(i8ie_mul_u8, mul_u8_nhwc_equal, a, b, scale, zp);
  Tensor<u8_t> out = pending_u8(a.shape, scale, (u8_t)zp);
  std::array<Tensor<u8_t>, 2> ops{a, b};  // share the operands' storage / pending launches
  const float s_a = a.scale, s_b = b.scale;
  const u8_t zp_a = a.zero_point, zp_b = b.zero_point, zp_o = (u8_t)zp;
  const std::vector<ssize_t> shp = a.shape;
  // deferred like the equal-shape result
  out.pend = make_pend(
      [ops, s_a, s_b, zp_a, zp_b, scale, zp_o, shp](bool relu, int border, bool s8) mutable {
        // (the gate of a squeeze-and-excitation block is f(a), still pending: it launches first, and a is read as it lies)
        auto ss = resolve_operands(ops.data(), 2);
        NhwcCopies copies;
        std::shared_ptr<Storage> sa = as_engine_nhwc(ss[0], shp, copies);
        std::shared_ptr<Storage>& sb = ss[1];
        // the gate as its producer left it: an [n, c, 1, 1] NHWC buffer with its border and re-bias, or plain rows (an
        // NCHW [n, c, 1, 1] tensor is the same bytes)
        const bool g_nhwc = sb->layout == I8IE_LAYOUT_NHWC && sb->dn == shp[0] && sb->dc == shp[1] && sb->dh == 1 && sb->dw == 1;
        if (!g_nhwc) sb->to_nchw();
        std::shared_ptr<Storage> st = nhwc_storage(shp, border, zp_o, s8);
        check(i8ie_mul_u8_nhwc(ctx(), (const uint8_t*)sa->device_ptr(), sa->border, sa->s8 ? 1 : 0, (const uint8_t*)sb->device_ptr(),
                               g_nhwc ? sb->border : 0, g_nhwc && sb->s8 ? 1 : 0, 1, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0,
                               (int)shp[0], (int)shp[1], (int)shp[2], (int)shp[3], s_a, zp_a, s_b, zp_b, scale, zp_o, relu ? 1 : 0));
        return st;
      }, {a.pend, b.pend});
  return out;
}
// ---- matmul / softmax (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_bmm_u8, i8ie_softmax_u8) ----
// Operands are rank 3 [b, r, c], or rank 4 [n, c, h, w] counted as [n, c, h * w] (the last two dimensions merged in reference
// order).  a is [b, m, k] ([b, k, m] when transpose_a), b is [b, k, n] ([b, n, k] when transpose_b); the same b on both sides.
// The result is [b, m, n] -- or [b, m, h, w] when a was given as rank 4 [b, m, h, w], untransposed, and n == h * w.  Anything
// else is a RuntimeError (before any device call).
struct MatmulShape {
  ssize_t b = 0, m = 0, n = 0, k = 0;
  std::vector<ssize_t> out;
};
template <typename T>
MatmulShape matmul_shape(const Tensor<T>& a, const Tensor<T>& b, bool ta, bool tb) {
  auto rc = [](const Tensor<T>& t, const char* which) {
    if (t.shape.size() != 3 && t.shape.size() != 4)
      throw std::runtime_error(std::string("i8ie: matmul: the ") + which + " operand must be [b, r, c] or [n, c, h, w]");
    for (ssize_t d : t.shape)
      if (d <= 0) throw std::runtime_error("i8ie: matmul: empty tensor");
    return std::array<ssize_t, 3>{t.shape[0], t.shape[1], t.shape.size() == 4 ? t.shape[2] * t.shape[3] : t.shape[2]};
  };
  const auto A = rc(a, "first"), B = rc(b, "second");
  MatmulShape s;
  s.b = A[0];
  s.m = ta ? A[2] : A[1];
  s.k = ta ? A[1] : A[2];
  s.n = tb ? B[1] : B[2];
  if (B[0] != s.b) throw std::runtime_error("i8ie: matmul: the operands' batch sizes differ (there is no broadcasting)");
  if ((tb ? B[2] : B[1]) != s.k) throw std::runtime_error("i8ie: matmul: the operands' inner dimensions differ");
  if (s.k > 32768) throw std::runtime_error("i8ie: matmul: inner dimension above 32768");
  if (a.shape.size() == 4 && !ta && s.n == a.shape[2] * a.shape[3]) s.out = {s.b, s.m, a.shape[2], a.shape[3]};
  else s.out = {s.b, s.m, s.n};
  return s;
}
// the [rows, cols] matrix per batch item of a tensor in reference order; `transposed`: the tensor holds [cols, rows]
i8ie_bmm_mat mat_reference_order(void* ptr, ssize_t rows, ssize_t cols, bool transposed) {
  i8ie_bmm_mat m;
  m.ptr = ptr;
  m.batch_stride = (int64_t)rows * cols;
  m.row_stride = transposed ? 1 : (int64_t)cols;
  m.col_stride = transposed ? (int64_t)rows : 1;
  m.s8 = 0;
  return m;
}
Tensor<float> matmul_f32(Tensor<float>& a, Tensor<float>& b, bool ta, bool tb) {
  const MatmulShape s = matmul_shape(a, b, ta, tb);
  Tensor<float> out(s.out);
  i8ie_bmm_args g{};
  g.b = (int)s.b; g.m = (int)s.m; g.n = (int)s.n; g.k = (int)s.k;
  g.a = mat_reference_order(a.dptr(), s.m, s.k, ta);
  g.bm = mat_reference_order(b.dptr(), s.k, s.n, tb);
  g.out = mat_reference_order(out.dptr(), s.m, s.n, false);
  check(i8ie_bmm_f32(ctx(), &g));
  return out;
}
// A u8 operand as it lies.  A rank-4 tensor stored NHWC without a border is physically [n, t, c]: its [c, t] matrix has the
// channel stride 1 and is read through the strides, re-biased or not.  One that exists with a border, and a view under other
// logical dims, goes back to the reference's order first (one layout conversion).
i8ie_bmm_mat mat_of_storage(const std::shared_ptr<Storage>& s, const std::vector<ssize_t>& shp, ssize_t rows, ssize_t cols, bool transposed) {
  const bool nhwc = s->layout == I8IE_LAYOUT_NHWC && s->border == 0 && shp.size() == 4 && s->dn == shp[0] && s->dc == shp[1] &&
                    s->dh == shp[2] && s->dw == shp[3];
  if (!nhwc) {
    s->to_nchw();
    return mat_reference_order(s->device_ptr(), rows, cols, transposed);
  }
  i8ie_bmm_mat m = mat_reference_order(s->device_ptr(), rows, cols, !transposed);  // [t, c] in memory: the transpose of [c, t]
  m.s8 = s->s8 ? 1 : 0;
  return m;
}
Tensor<u8_t> matmul_u8(Tensor<u8_t>& a, Tensor<u8_t>& b, float scale, int zp, bool ta, bool tb) {
  const MatmulShape s = matmul_shape(a, b, ta, tb);
  check_out_qparams("matmul", scale, zp);
  if (!std::isfinite(a.scale) || !std::isfinite(b.scale)) throw std::runtime_error("i8ie: matmul: an operand's scale is not finite");
  if ((!a.st && !a.pend) || (!b.st && !b.pend)) throw std::runtime_error("i8ie: empty tensor");
  Tensor<u8_t> out = pending_u8(s.out, scale, (u8_t)zp);
  std::array<Tensor<u8_t>, 2> ops{a, b};  // share the operands' storage / pending launches
  const float s_a = a.scale, s_b = b.scale;
  const u8_t zp_a = a.zero_point, zp_b = b.zero_point, zp_o = (u8_t)zp;
  const std::vector<ssize_t> sha = a.shape, shb = b.shape;
  // deferred like add's result: relu(matmul(..)) is one launch, and a rank-4 result gets the border and re-bias the next conv
  // asks for straight from the kernel.  The operands' producers are asked for border 0 (operand_as_it_lies).
  out.pend = make_pend(
      [ops, s, s_a, s_b, zp_a, zp_b, scale, zp_o, sha, shb, ta, tb](bool relu, int border, bool s8) mutable {
        auto ss = resolve_operands(ops.data(), 2);
        i8ie_bmm_args g{};
        g.b = (int)s.b; g.m = (int)s.m; g.n = (int)s.n; g.k = (int)s.k;
        g.a = mat_of_storage(ss[0], sha, s.m, s.k, ta);
        g.bm = mat_of_storage(ss[1], shb, s.k, s.n, tb);
        std::shared_ptr<Storage> st;
        if (s.out.size() == 4) {  // NHWC [b, h + 2B, w + 2B, m]: the n columns are the pixels
          st = nhwc_storage(s.out, border, zp_o, s8);
          g.out.ptr = st->dev;
          g.out.batch_stride = (int64_t)s.m * (s.out[2] + 2 * st->border) * (s.out[3] + 2 * st->border);
          g.out.row_stride = 1;
          g.out.col_stride = (int64_t)s.m;
          g.out.s8 = st->s8 ? 1 : 0;
          g.out_pix_axis = 2;
          g.out_h = (int)s.out[2]; g.out_w = (int)s.out[3]; g.out_border = st->border;
        } else {
          st = device_storage((size_t)(s.b * s.m * s.n));
          g.out = mat_reference_order(st->dev, s.m, s.n, false);
        }
        g.s_a = s_a; g.s_b = s_b; g.s_out = scale;
        g.zp_a = zp_a; g.zp_b = zp_b; g.zp_out = zp_o;
        g.relu = relu ? 1 : 0;
        check(i8ie_bmm_u8(ctx(), &g));
        return st;
      }, {a.pend, b.pend});
  return out;
}
// softmax over the last axis; the u8 result always carries scale 1/256, zero point 0.  A plain flat tensor: an input that is
// not in reference order is converted first.
Tensor<float> softmax_f32(Tensor<float>& x) {
  if (x.shape.empty() || x.size <= 0) throw std::runtime_error("i8ie: softmax: empty tensor");
  Tensor<float> out(x.shape);
  check(i8ie_softmax_f32(ctx(), x.dptr(), out.dptr(), (int64_t)(x.size / x.shape.back()), (int)x.shape.back()));
  return out;
}
Tensor<u8_t> softmax_u8(Tensor<u8_t>& x) {
  if (x.shape.empty() || x.size <= 0) throw std::runtime_error("i8ie: softmax: empty tensor");
  if (x.shape.back() > 65535) throw std::runtime_error("i8ie: softmax: rows of more than 65535 values");
  if (!std::isfinite(x.scale) || x.scale < 0) throw std::runtime_error("i8ie: softmax: the input scale must be finite and not negative");
  const uint8_t* src = x.dptr();
  Tensor<u8_t> out(x.shape);
  out.scale = 1.0f / 256.0f;
  out.zero_point = 0;
  check(i8ie_softmax_u8(ctx(), src, out.dptr(), (int64_t)(x.size / x.shape.back()), (int)x.shape.back(), x.scale));
  return out;
}
// ---- attention (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_attention_u8) -----------------------
// Operands are rank 3 [b, t, c], or rank 4 [n, c, h, w] counted as [n, h * w, c] (the engine's NHWC storage as it lies).  q is
// [b, tq, c], k and v are [b, tk, c], c = heads * d; or one packed tensor with 3 * heads * d channels (k == v == nullptr): q, k, v
// are then its channels [0, c), [c, 2c), [2c, 3c).  The result has q's rank: [b, tq, c] or [n, c, h, w].  Anything else is a
// RuntimeError (before any device call).
struct AttnShape {
  ssize_t b = 0, heads = 0, d = 0, c = 0, tq = 0, tk = 0;
  bool packed = false;
  std::vector<ssize_t> out;
};
template <typename T>
AttnShape attention_shape(const Tensor<T>& q, const Tensor<T>* k, const Tensor<T>* v, ssize_t heads) {
  auto btc = [](const Tensor<T>& t, const char* which) {
    if (t.shape.size() != 3 && t.shape.size() != 4)
      throw std::runtime_error(std::string("i8ie: attention: ") + which + " must be [b, t, c] or [n, c, h, w]");
    for (ssize_t d : t.shape)
      if (d <= 0) throw std::runtime_error("i8ie: attention: empty tensor");
    if (t.shape.size() == 4) return std::array<ssize_t, 3>{t.shape[0], t.shape[2] * t.shape[3], t.shape[1]};
    return std::array<ssize_t, 3>{t.shape[0], t.shape[1], t.shape[2]};
  };
  if ((k == nullptr) != (v == nullptr)) throw std::runtime_error("i8ie: attention takes q, k and v, or one packed qkv tensor");
  if (heads < 1) throw std::runtime_error("i8ie: attention: heads must be >= 1");
  AttnShape s;
  s.heads = heads;
  s.packed = k == nullptr;
  const auto Q = btc(q, s.packed ? "qkv" : "q");
  s.b = Q[0];
  s.tq = s.tk = Q[1];
  if (s.packed) {
    if (Q[2] % (3 * heads) != 0) throw std::runtime_error("i8ie: attention: a packed qkv tensor needs 3 * heads * d channels");
    s.c = Q[2] / 3;
  } else {
    const auto K = btc(*k, "k"), V = btc(*v, "v");
    if (K[0] != s.b || V[0] != s.b) throw std::runtime_error("i8ie: attention: the operands' batch sizes differ (there is no broadcasting)");
    if (K[2] != Q[2] || V[2] != Q[2]) throw std::runtime_error("i8ie: attention: q, k and v must have the same channel count");
    if (K[1] != V[1]) throw std::runtime_error("i8ie: attention: k and v must have the same token count");
    if (Q[2] % heads != 0) throw std::runtime_error("i8ie: attention: the channel count is not heads * d");
    s.c = Q[2];
    s.tk = K[1];
  }
  s.d = s.c / heads;
  if (s.tk > 32768) throw std::runtime_error("i8ie: attention: more than 32768 key tokens");
  if (q.shape.size() == 4) s.out = {s.b, s.c, q.shape[2], q.shape[3]};
  else s.out = {s.b, s.tq, s.c};
  return s;
}
// FP32: the composition i8ie_bmm_f32, i8ie_softmax_f32, i8ie_bmm_f32 per head.  Rank-3 operands go through
// i8ie_attention_f32; an FP32 rank-4 tensor is NCHW, its token matrix has the token stride 1, so the same three entries are
// driven through strides here (the bits are the same: i8ie_bmm_f32 adds in ascending k whatever the strides are).  `scores`:
// null, or a [b, heads, tq, tk] tensor that receives the scores before the softmax (what the calibrator samples).
Tensor<float> attention_f32(Tensor<float>& q, Tensor<float>* k, Tensor<float>* v, ssize_t heads, Tensor<float>* scores) {
  const AttnShape s = attention_shape(q, k, v, heads);
  Tensor<float> out(s.out);
  Tensor<float>* ts[3] = {&q, s.packed ? &q : k, s.packed ? &q : v};
  const ssize_t C = s.packed ? 3 * s.c : s.c;
  const bool flat = q.shape.size() == 3 && ts[1]->shape.size() == 3 && ts[2]->shape.size() == 3;
  if (flat) {
    i8ie_attention_args g{};
    g.b = (int)s.b; g.heads = (int)s.heads; g.d = (int)s.d; g.tq = (int)s.tq; g.tk = (int)s.tk;
    i8ie_attn_mat* ms[3] = {&g.q, &g.k, &g.v};
    for (int i = 0; i < 3; ++i) {
      const ssize_t t = i == 0 ? s.tq : s.tk;
      *ms[i] = i8ie_attn_mat{ts[i]->dptr() + (s.packed ? i * s.c : 0), (int64_t)t * C, (int64_t)C, 0};
    }
    g.out = i8ie_attn_mat{out.dptr(), (int64_t)s.tq * s.c, (int64_t)s.c, 0};
    g.scores_out_dev = scores ? scores->dptr() : nullptr;
    check(i8ie_attention_f32(ctx(), &g));
    return out;
  }
  // element (batch, token, column) of a tensor with `ch` channels, channel offset `off`: [b, t, ch] or NCHW [b, ch, t]
  auto mat = [](Tensor<float>& t, ssize_t tokens, ssize_t ch, ssize_t off, bool tokens_are_rows) {
    const bool nchw = t.shape.size() == 4;
    i8ie_bmm_mat m;
    m.ptr = t.dptr() + (nchw ? off * tokens : off);
    m.batch_stride = (int64_t)tokens * ch;
    const int64_t tok = nchw ? 1 : (int64_t)ch, col = nchw ? (int64_t)tokens : 1;
    m.row_stride = tokens_are_rows ? tok : col;
    m.col_stride = tokens_are_rows ? col : tok;
    m.s8 = 0;
    return m;
  };
  const ssize_t per_head = s.tq * s.tk;
  Tensor<float> ws({s.b, s.tq, s.tk});
  for (ssize_t h = 0; h < s.heads; ++h) {
    i8ie_bmm_args a{};
    a.b = (int)s.b; a.m = (int)s.tq; a.n = (int)s.tk; a.k = (int)s.d;
    a.a = mat(*ts[0], s.tq, C, h * s.d, true);
    a.bm = mat(*ts[1], s.tk, C, (s.packed ? s.c : 0) + h * s.d, false);
    a.out = i8ie_bmm_mat{ws.dptr(), (int64_t)per_head, (int64_t)s.tk, 1, 0};
    check(i8ie_bmm_f32(ctx(), &a));
    if (scores) {
      a.out = i8ie_bmm_mat{scores->dptr() + h * per_head, (int64_t)(s.heads * per_head), (int64_t)s.tk, 1, 0};
      check(i8ie_bmm_f32(ctx(), &a));
    }
    check(i8ie_softmax_f32(ctx(), ws.dptr(), ws.dptr(), (int64_t)(s.b * s.tq), (int)s.tk));
    i8ie_bmm_args o{};
    o.b = (int)s.b; o.m = (int)s.tq; o.n = (int)s.d; o.k = (int)s.tk;
    o.a = i8ie_bmm_mat{ws.dptr(), (int64_t)per_head, (int64_t)s.tk, 1, 0};
    o.bm = mat(*ts[2], s.tk, C, (s.packed ? 2 * s.c : 0) + h * s.d, true);
    o.out = mat(out, s.tq, s.c, h * s.d, true);
    check(i8ie_bmm_f32(ctx(), &o));
  }
  return out;
}
// A u8 operand as it lies.  A rank-4 tensor stored NHWC without a border is physically [n, t, ch]: read in place, re-biased or
// not.  One that exists with a border, a view under other logical dims and an NCHW tensor take a layout conversion into a
// border-free NHWC buffer (`copies` keeps a temporary alive); a rank-3 tensor is read in the reference's order.
i8ie_attn_mat attn_operand(std::shared_ptr<Storage> s, const std::vector<ssize_t>& shp, ssize_t tokens, ssize_t ch, ssize_t off,
                           NhwcCopies& copies) {
  i8ie_attn_mat m{};
  if (shp.size() == 4) {
    if (s->layout == I8IE_LAYOUT_NHWC && s->border != 0) s->to_nchw();
    s = as_engine_nhwc(s, shp, copies);
    m.s8 = s->s8 ? 1 : 0;
  } else {
    s->to_nchw();
  }
  m.ptr = (uint8_t*)s->device_ptr() + off;
  m.batch_stride = (int64_t)tokens * ch;
  m.token_stride = (int64_t)ch;
  return m;
}
Tensor<u8_t> attention_u8(Tensor<u8_t>& q, Tensor<u8_t>* k, Tensor<u8_t>* v, ssize_t heads, float s_s, int zp_s, float scale, int zp) {
  const AttnShape s = attention_shape(q, k, v, heads);
  check_out_qparams("attention", scale, zp);
  check_out_qparams("attention (scores)", s_s, zp_s);
  std::vector<Tensor<u8_t>> ops{q};  // share the operands' storage / pending launches
  if (!s.packed) {
    ops.push_back(*k);
    ops.push_back(*v);
  }
  for (const auto& t : ops) {
    if (!std::isfinite(t.scale)) throw std::runtime_error("i8ie: attention: an operand's scale is not finite");
    if (!t.st && !t.pend) throw std::runtime_error("i8ie: empty tensor");
  }
  Tensor<u8_t> out = pending_u8(s.out, scale, (u8_t)zp);
  const u8_t zp_o = (u8_t)zp, zs = (u8_t)zp_s;
  // deferred like matmul's result: relu(attention(..)) is one launch, and a rank-4 result gets the border and re-bias the next
  // conv asks for straight from the kernel.  The operands' producers are asked for border 0 (operand_as_it_lies).
  auto run = [ops, s, s_s, zs, scale, zp_o](bool relu, int border, bool s8) mutable {
    auto ss = resolve_operands(ops.data(), ops.size());
    NhwcCopies copies;
    i8ie_attention_args g{};
    g.b = (int)s.b; g.heads = (int)s.heads; g.d = (int)s.d; g.tq = (int)s.tq; g.tk = (int)s.tk;
    const ssize_t C = s.packed ? 3 * s.c : s.c;
    const Tensor<u8_t>&tq = ops[0], &tk = ops[s.packed ? 0 : 1], &tv = ops[s.packed ? 0 : 2];
    g.q = attn_operand(ss[0], tq.shape, s.tq, C, 0, copies);
    g.k = attn_operand(ss[s.packed ? 0 : 1], tk.shape, s.tk, C, s.packed ? s.c : 0, copies);
    g.v = attn_operand(ss[s.packed ? 0 : 2], tv.shape, s.tk, C, s.packed ? 2 * s.c : 0, copies);
    g.s_q = tq.scale; g.s_k = tk.scale; g.s_v = tv.scale; g.s_s = s_s; g.s_o = scale;
    g.zp_q = tq.zero_point; g.zp_k = tk.zero_point; g.zp_v = tv.zero_point; g.zp_s = zs; g.zp_o = zp_o;
    g.relu = relu ? 1 : 0;
    std::shared_ptr<Storage> st;
    if (s.out.size() == 4) {  // NHWC [b, h + 2B, w + 2B, c]: the tq tokens are the pixels
      st = nhwc_storage(s.out, border, zp_o, s8);
      g.out = i8ie_attn_mat{st->dev, (int64_t)s.c * (s.out[2] + 2 * st->border) * (s.out[3] + 2 * st->border), (int64_t)s.c, st->s8 ? 1 : 0};
      g.out_h = (int)s.out[2]; g.out_w = (int)s.out[3]; g.out_border = st->border;
    } else {
      st = device_storage((size_t)(s.b * s.tq * s.c));
      g.out = i8ie_attn_mat{st->dev, (int64_t)s.tq * s.c, (int64_t)s.c, 0};
    }
    check(i8ie_attention_u8(ctx(), &g));
    return st;
  };
  if (s.packed) out.pend = make_pend(run, {q.pend});
  else out.pend = make_pend(run, {q.pend, k->pend, v->pend});
  return out;
}
// ---- layer_norm (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_layernorm_u8) ---------------------
// [n, c, h, w] is normalised over c per pixel, [m, f] and [b, t, f] over the last axis: (rows, inner) of the FP32 entry, or
// a RuntimeError (before any device call)
template <typename T>
std::pair<int64_t, int64_t> layer_norm_rows(const Tensor<T>& x, ssize_t channels) {
  const size_t r = x.shape.size();
  if (x.size <= 0 || (r != 2 && r != 3 && r != 4)) throw std::runtime_error("i8ie: layer_norm expects [n, c, h, w], [m, f] or [b, t, f]");
  if ((r == 4 ? x.shape[1] : x.shape.back()) != channels)
    throw std::runtime_error("i8ie: layer_norm: the normalised axis has " + std::to_string(r == 4 ? x.shape[1] : x.shape.back()) +
                             " values, the layer " + std::to_string(channels));
  if (channels > 16384) throw std::runtime_error("i8ie: layer_norm: rows of more than 16384 values");
  return {(int64_t)(x.size / channels), r == 4 ? (int64_t)(x.shape[2] * x.shape[3]) : 1};
}
std::shared_ptr<Storage> upload_f32(const std::vector<float>& v) {
  auto s = device_storage(v.size() * sizeof(float));
  check(i8ie_memcpy_h2d(ctx(), s->dev, v.data(), v.size() * sizeof(float)));
  return s;
}
Tensor<float> layer_norm_f32(Tensor<float>& x, const std::shared_ptr<Storage>& gamma, const std::shared_ptr<Storage>& beta, ssize_t channels,
                             float eps) {
  const auto ri = layer_norm_rows(x, channels);
  if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: layer_norm: eps must be positive and finite");
  Tensor<float> out(x.shape);
  check(i8ie_layernorm_f32(ctx(), x.dptr(), out.dptr(), ri.first, (int)channels, (const float*)gamma->dev, (const float*)beta->dev, eps,
                           ri.second));
  return out;
}
// g, b: the device arrays of i8ie_layernorm_affine for (scale, zp), kept alive by the recorded launch
Tensor<u8_t> layer_norm_u8(Tensor<u8_t>& in, const std::shared_ptr<Storage>& g, const std::shared_ptr<Storage>& b, ssize_t channels, float eps,
                           float scale, int zp) {
  check_out_qparams("layer_norm", scale, zp);
  if (!in.st && !in.pend) throw std::runtime_error("i8ie: empty tensor");
  const int64_t rows = layer_norm_rows(in, channels).first;
  if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: layer_norm: eps must be positive and finite");
  if (!(in.scale > 0) || !std::isfinite(in.scale)) throw std::runtime_error("i8ie: layer_norm: the input scale must be positive and finite");
  Tensor<u8_t> out = pending_u8(in.shape, scale, (u8_t)zp);
  Tensor<u8_t> src = in;
  const std::vector<ssize_t> shp = in.shape;
  const float s_in = in.scale;
  const u8_t zp_o = (u8_t)zp;
  const int C = (int)channels;
  // deferred like add's and the activations' results: relu(ln(..)) is one launch, a consuming conv gets its zero-point border
  // and, where it reads them, re-biased bytes straight from the kernel, and several consumers share one launch (PendNode)
  out.pend = make_pend(
      [src, g, b, shp, rows, s_in, eps, zp_o, C](bool relu, int border, bool s8) mutable {
        std::shared_ptr<Storage> si = operand_as_it_lies(src);
        std::shared_ptr<Storage> st;
        if (shp.size() == 4) {
          NhwcCopies copies;
          si = as_engine_nhwc(si, shp, copies);
          st = nhwc_storage(shp, border, zp_o, s8);
          check(i8ie_layernorm_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                       st->s8 ? 1 : 0, (int)shp[0], C, (int)shp[2], (int)shp[3], (const float*)g->dev, (const float*)b->dev,
                                       s_in, eps, relu ? 1 : 0, zp_o));
        } else {  // rows (a flattened NHWC activation goes back to the reference's order; one pixel per image is in it already)
          if (si->layout == I8IE_LAYOUT_NHWC && si->dh * si->dw == 1 && si->border == 0) si->unbias();
          else si->to_nchw();
          st = device_storage((size_t)rows * C);
          check(i8ie_layernorm_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, rows, C, (const float*)g->dev,
                                  (const float*)b->dev, s_in, eps, relu ? 1 : 0, zp_o));
        }
        return st;
      }, {in.pend});
  return out;
}
using F32Array = py::array_t<float, py::array::c_style | py::array::forcecast>;
std::vector<float> layer_norm_param(const py::object& a, ssize_t channels, float fill, const char* what) {
  if (a.is_none()) return std::vector<float>((size_t)channels, fill);
  F32Array v = F32Array::ensure(a);
  if (!v || v.ndim() != 1 || v.shape(0) != channels)
    throw std::runtime_error(std::string("i8ie: layer_norm: ") + what + " must hold one float per normalised value");
  return std::vector<float>(v.data(), v.data() + v.size());
}
// (g, b) of i8ie_layernorm_affine on the device
std::pair<std::shared_ptr<Storage>, std::shared_ptr<Storage>> layer_norm_affine(const std::vector<float>& gamma, const std::vector<float>& beta,
                                                                                 float scale, int zp) {
  std::vector<float> g(gamma.size()), b(gamma.size());
  check(i8ie_layernorm_affine(gamma.data(), beta.data(), (int)gamma.size(), scale, (uint8_t)zp, g.data(), b.data()));
  return {upload_f32(g), upload_f32(b)};
}
template <typename T>
ssize_t layer_norm_axis(const Tensor<T>& x) {
  if (x.shape.size() < 2) throw std::runtime_error("i8ie: layer_norm expects [n, c, h, w], [m, f] or [b, t, f]");
  return x.shape.size() == 4 ? x.shape[1] : x.shape.back();
}
// ---- cat (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_concat_u8) --------------------------
// axis 1 of k rank-4 [n, c_i, h, w] or k rank-2 [m, f_i] tensors: the result's shape, or a RuntimeError (before any device call)
template <typename T>
std::vector<ssize_t> cat_shape(const std::vector<Tensor<T>>& ts) {
  if (ts.empty() || ts.size() > I8IE_CONCAT_MAX_INPUTS) throw std::runtime_error("i8ie: cat: between 1 and 8 tensors");
  std::vector<ssize_t> shp = ts[0].shape;
  if (shp.size() != 2 && shp.size() != 4) throw std::runtime_error("i8ie: cat: tensors must be [n, c, h, w] or [m, f] (joined along axis 1)");
  for (size_t i = 1; i < ts.size(); ++i) {
    const std::vector<ssize_t>& s = ts[i].shape;
    if (s.size() != shp.size()) throw std::runtime_error("i8ie: cat: ranks differ");
    for (size_t d = 0; d < s.size(); ++d)
      if (d != 1 && s[d] != ts[0].shape[d]) throw std::runtime_error("i8ie: cat: shapes differ outside axis 1");
    shp[1] += s[1];
  }
  for (const auto& t : ts)
    for (ssize_t d : t.shape)
      if (d <= 0) throw std::runtime_error("i8ie: cat: empty tensor");
  return shp;
}
// a Python list of tensors of one dtype; anything else (a mix included) is a RuntimeError
template <typename T>
std::vector<Tensor<T>> cat_list(const py::list& l) {
  std::vector<Tensor<T>> ts;
  for (const py::handle& h : l) {
    if (!py::isinstance<Tensor<T>>(h)) throw std::runtime_error("i8ie: cat: every tensor must have the same dtype (float32, or uint8 with scale and zero_point)");
    ts.push_back(h.cast<Tensor<T>&>());
  }
  return ts;
}
template <typename T>
ssize_t cat_run_len(const Tensor<T>& t) { return t.shape.size() == 4 ? t.shape[1] * t.shape[2] * t.shape[3] : t.shape[1]; }
Tensor<float> cat_f32(std::vector<Tensor<float>> ts) {
  Tensor<float> out(cat_shape(ts));
  const float* in[I8IE_CONCAT_MAX_INPUTS];
  int64_t len[I8IE_CONCAT_MAX_INPUTS];
  for (size_t i = 0; i < ts.size(); ++i) {
    in[i] = ts[i].dptr();
    len[i] = (int64_t)cat_run_len(ts[i]);
  }
  check(i8ie_concat_f32(ctx(), (int)ts.size(), in, len, out.dptr(), (int64_t)out.shape[0]));
  return out;
}
Tensor<u8_t> cat_u8(std::vector<Tensor<u8_t>> ts, float scale, int zp) {
  const std::vector<ssize_t> shp = cat_shape(ts);
  check_out_qparams("cat", scale, zp);
  for (const auto& t : ts)
    if (!std::isfinite(t.scale)) throw std::runtime_error("i8ie: cat: an input's scale is not finite");
  Tensor<u8_t> out = pending_u8(shp, scale, (u8_t)zp);
  const u8_t zp_o = (u8_t)zp;
  const ssize_t total = out.size;
  // deferred like add's result: relu(cat(..)) is one launch, and a consuming conv gets its zero-point border and, where it
  // reads them, re-biased bytes straight from the concat kernel.  (the closure's copies share the inputs' storage / launches)
  auto node = make_pend([ts, scale, zp_o, shp, total](bool relu, int border, bool s8) mutable {
    const int k = (int)ts.size();
    auto ss = resolve_operands(ts.data(), ts.size());
    bool any_nhwc = false;
    for (int i = 0; i < k; ++i) any_nhwc = any_nhwc || ss[i]->layout == I8IE_LAYOUT_NHWC;
    const uint8_t* in[I8IE_CONCAT_MAX_INPUTS];
    float s_in[I8IE_CONCAT_MAX_INPUTS];
    uint8_t zp_in[I8IE_CONCAT_MAX_INPUTS];
    for (int i = 0; i < k; ++i) {
      s_in[i] = ts[i].scale;
      zp_in[i] = ts[i].zero_point;
    }
    std::shared_ptr<Storage> st;
    if (shp.size() == 4 && any_nhwc) {  // the engine keeps NHWC between layers (and a consumer that asked for a border reads NHWC)
      int c_in[I8IE_CONCAT_MAX_INPUTS], b_in[I8IE_CONCAT_MAX_INPUTS], x_in[I8IE_CONCAT_MAX_INPUTS];
      NhwcCopies copies;  // (the same tensor again takes its conversion too)
      for (int i = 0; i < k; ++i) {
        ss[i] = as_engine_nhwc(ss[i], ts[i].shape, copies);
        in[i] = (const uint8_t*)ss[i]->device_ptr();
        c_in[i] = (int)ts[i].shape[1];
        b_in[i] = ss[i]->border;
        x_in[i] = ss[i]->s8 ? 1 : 0;
      }
      st = nhwc_storage(shp, border, zp_o, s8);
      check(i8ie_concat_u8_nhwc(ctx(), k, in, c_in, b_in, x_in, s_in, zp_in, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0, (int)shp[0],
                                (int)shp[2], (int)shp[3], scale, zp_o, relu ? 1 : 0));
    } else {  // NCHW tensors and [m, f_i] rows (a flattened NHWC activation goes back to the reference's order): the run form
      int64_t len[I8IE_CONCAT_MAX_INPUTS];
      for (int i = 0; i < k; ++i) {
        ss[i]->to_nchw();
        in[i] = (const uint8_t*)ss[i]->device_ptr();
        len[i] = (int64_t)cat_run_len(ts[i]);
      }
      st = device_storage((size_t)total);
      check(i8ie_concat_u8(ctx(), k, in, len, s_in, zp_in, (uint8_t*)st->dev, (int64_t)shp[0], scale, zp_o, relu ? 1 : 0));
    }
    // (the inputs are released with the closure's copies, as a layer's input is)
    return st;
  });
  for (const auto& t : ts)
    if (t.pend) node->inputs.push_back(t.pend);
  out.pend = node;
  return out;
}
// ---- avg_pool2d / global_avg_pool2d (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_avgpool2d_u8) ---
// kh x kw window; the global pool is the whole image at stride 1
template <typename T>
std::vector<ssize_t> avg_pool_shape(const Tensor<T>& in, ssize_t kh, ssize_t kw, ssize_t s, bool global) {
  const std::string what = global ? "i8ie: global_avg_pool2d" : "i8ie: avg_pool2d";
  if (in.shape.size() != 4) throw std::runtime_error(what + " expects an NCHW tensor");
  if (global) {
    kh = in.shape[2];
    kw = in.shape[3];
  }
  if (kh <= 0 || kw <= 0 || s <= 0) throw std::runtime_error(what + ": kernel_size and stride must be positive");
  if (kh > in.shape[2] || kw > in.shape[3]) throw std::runtime_error(what + ": window larger than input");
  if (kh * kw > 65536) throw std::runtime_error(what + ": window of more than 65536 elements");
  return {in.shape[0], in.shape[1], (in.shape[2] - kh) / s + 1, (in.shape[3] - kw) / s + 1};
}
Tensor<float> avg_pool_f32(Tensor<float>& in, ssize_t k, ssize_t s, bool global) {
  Tensor<float> out(avg_pool_shape(in, k, k, s, global));
  const ssize_t kh = global ? in.shape[2] : k, kw = global ? in.shape[3] : k;
  check(i8ie_avgpool2d_f32(ctx(), in.dptr(), out.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3],
                           (int)kh, (int)kw, (int)s));
  return out;
}
Tensor<u8_t> avg_pool_u8(Tensor<u8_t>& in, ssize_t k, ssize_t s, bool global) {
  Tensor<u8_t> out = pending_u8(avg_pool_shape(in, k, k, s, global), in.scale, in.zero_point);  // (as max_pool2d: the input's qparams)
  Tensor<u8_t> src = in;
  const std::vector<ssize_t> ishp = in.shape, oshp = out.shape;
  const u8_t zp = in.zero_point;
  const int kh = (int)(global ? in.shape[2] : k), kw = (int)(global ? in.shape[3] : k), ss = (int)s;
  // deferred like max_pool2d's and add's results: relu(avg_pool2d(..)) is one launch, and a consuming conv gets its
  // zero-point border and, where it reads them, re-biased bytes straight from the pool kernel
  out.pend = make_pend(
      [src, ishp, oshp, zp, kh, kw, ss](bool relu, int border, bool s8) mutable {
        std::shared_ptr<Storage> si = operand_as_it_lies(src);
        const size_t logical = (size_t)oshp[0] * oshp[1] * oshp[2] * oshp[3];
        std::shared_ptr<Storage> st;
        if (si->layout == I8IE_LAYOUT_NHWC) {
          // a plain border-free [n, c, 1, 1] result is the same bytes in both orders: it is labelled NCHW, so that its
          // reshape to [n, c] reaches a Linear layer (or the host) without a layout conversion
          const bool both_orders = oshp[2] == 1 && oshp[3] == 1 && border == 0 && !s8;
          st = both_orders ? device_storage(logical) : nhwc_storage(oshp, border, zp, s8);
          check(i8ie_avgpool2d_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev,
                                       st->border, st->s8 ? 1 : 0, (int)ishp[0], (int)ishp[1], (int)ishp[2], (int)ishp[3], kh, kw, ss,
                                       relu ? 1 : 0, zp));
        } else {  // an NCHW operand (a user-made tensor)
          st = device_storage(logical);
          check(i8ie_avgpool2d_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, (int)ishp[0], (int)ishp[1], (int)ishp[2],
                                  (int)ishp[3], kh, kw, ss));
          if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        }
        return st;
      }, {in.pend});
  return out;
}
// ---- upsample (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_upsample2d_u8) -----------------------
template <typename T>
std::vector<ssize_t> upsample_shape(const Tensor<T>& in, ssize_t fh, ssize_t fw, int mode) {
  if (in.shape.size() != 4) throw std::runtime_error("i8ie: upsample expects an NCHW tensor");
  for (ssize_t d : in.shape)
    if (d <= 0) throw std::runtime_error("i8ie: upsample: empty tensor");
  if (fh < 1 || fh > 8 || fw < 1 || fw > 8) throw std::runtime_error("i8ie: upsample: scale factors must be integers in 1..8");
  if (mode != I8IE_UPSAMPLE_NEAREST && mode != I8IE_UPSAMPLE_BILINEAR) throw std::runtime_error("i8ie: upsample: unknown mode");
  return {in.shape[0], in.shape[1], in.shape[2] * fh, in.shape[3] * fw};
}
Tensor<float> upsample_f32(Tensor<float>& in, ssize_t fh, ssize_t fw, int mode) {
  Tensor<float> out(upsample_shape(in, fh, fw, mode));
  check(i8ie_upsample2d_f32(ctx(), in.dptr(), out.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3],
                            (int)fh, (int)fw, mode));
  return out;
}
Tensor<u8_t> upsample_u8(Tensor<u8_t>& in, ssize_t fh, ssize_t fw, int mode) {
  Tensor<u8_t> out = pending_u8(upsample_shape(in, fh, fw, mode), in.scale, in.zero_point);  // (as the pools: the input's qparams)
  if (!in.st && !in.pend) throw std::runtime_error("i8ie: empty tensor");
  Tensor<u8_t> src = in;
  const std::vector<ssize_t> ishp = in.shape, oshp = out.shape;
  const u8_t zp = in.zero_point;
  const int f_h = (int)fh, f_w = (int)fw;
  // deferred like avg_pool2d's result: relu(upsample(..)) is one launch, and a consuming conv gets its zero-point border
  // and, where it reads them, re-biased bytes straight from the upsample kernel
  out.pend = make_pend(
      [src, ishp, oshp, zp, f_h, f_w, mode](bool relu, int border, bool s8) mutable {
        std::shared_ptr<Storage> si = operand_as_it_lies(src);
        // (a view whose storage is NHWC under other logical dims goes back to the reference's order: the view is defined on it)
        if (si->layout == I8IE_LAYOUT_NHWC && (si->dn != ishp[0] || si->dc != ishp[1] || si->dh != ishp[2] || si->dw != ishp[3])) si->to_nchw();
        std::shared_ptr<Storage> st;
        if (si->layout == I8IE_LAYOUT_NHWC) {
          st = nhwc_storage(oshp, border, zp, s8);
          check(i8ie_upsample2d_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                        st->s8 ? 1 : 0, (int)ishp[0], (int)ishp[1], (int)ishp[2], (int)ishp[3], f_h, f_w, mode,
                                        relu ? 1 : 0, zp));
        } else {  // an NCHW operand (a user-made tensor)
          st = device_storage((size_t)oshp[0] * oshp[1] * oshp[2] * oshp[3]);
          check(i8ie_upsample2d_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, (int)ishp[0], (int)ishp[1], (int)ishp[2],
                                   (int)ishp[3], f_h, f_w, mode));
          if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        }
        return st;
      }, {in.pend});
  return out;
}
// ---- activation / lut (no counterpart in the reference; arithmetic: include/i8ie_hip.h, i8ie_activation_table) -------
using LutBytes = std::array<u8_t, 256>;
Tensor<float> activation_f32(Tensor<float>& in, int kind, float param) {
  Tensor<float> out(in.shape);
  check(i8ie_activation_f32(ctx(), kind, param, in.dptr(), out.dptr(), in.size));
  return out;
}
// out = table[in] with the result's (scale, zp): table maps plain bytes to plain bytes
Tensor<u8_t> lut_u8(Tensor<u8_t>& in, const LutBytes& table, float scale, int zp) {
  check_out_qparams("lut", scale, zp);
  if (!in.st && !in.pend) throw std::runtime_error("i8ie: empty tensor");
  Tensor<u8_t> out = pending_u8(in.shape, scale, (u8_t)zp);
  Tensor<u8_t> src = in;
  const std::vector<ssize_t> shp = in.shape;
  const ssize_t total = in.size;
  const u8_t zp_o = (u8_t)zp;
  // deferred like add's and cat's results: relu(act(..)) is one launch (the relu is max(table[a], zp) on the host), and a
  // consuming conv gets its zero-point border and, where it reads them, re-biased bytes straight from the lookup kernel
  out.pend = make_pend(
      [src, table, zp_o, shp, total](bool relu, int border, bool s8) mutable {
        std::shared_ptr<Storage> si = operand_as_it_lies(src);
        LutBytes t = table;
        if (relu)
          for (u8_t& b : t) b = std::max(b, zp_o);
        std::shared_ptr<Storage> st;
        if (shp.size() == 4) {  // the engine keeps NHWC between layers (and a consumer that asked for a border reads NHWC)
          NhwcCopies copies;
          si = as_engine_nhwc(si, shp, copies);
          st = nhwc_storage(shp, border, zp_o, s8);
          check(i8ie_lut_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                 st->s8 ? 1 : 0, (int)shp[0], (int)shp[1], (int)shp[2], (int)shp[3], t.data()));
        } else {  // rows and other ranks (a flattened NHWC activation goes back to the reference's order): the flat form
          si->to_nchw();
          st = device_storage((size_t)total);
          check(i8ie_lut_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, (int64_t)total, t.data()));
        }
        return st;
      }, {in.pend});
  return out;
}
Tensor<u8_t> activation_u8(Tensor<u8_t>& in, int kind, float param, float scale, int zp) {
  check_zero_point(zp);
  LutBytes table;
  check(i8ie_activation_table(kind, param, in.scale, in.zero_point, scale, (uint8_t)zp, table.data()));
  return lut_u8(in, table, scale, zp);
}
LutBytes lut_from_array(const py::array_t<uint8_t, py::array::c_style>& a) {
  if (a.size() != 256) throw std::runtime_error("i8ie: lut: the table must hold 256 uint8 entries");
  LutBytes t;
  std::memcpy(t.data(), a.data(), 256);
  return t;
}
// the s8 instantiations of the generic templates (src/functional.cc:5-13, 36-64, registered at :78-82)
Tensor<s8_t> relu_s8(Tensor<s8_t>& in) {
  if (!in.st) return Tensor<s8_t>();  // default-constructed: nothing to do
  Tensor<s8_t> out(in.shape);  // (the generic relu does not carry scale / zero point over: src/functional.cc:7)
  if (in.size > 0) check(i8ie_relu_s8(ctx(), (const int8_t*)in.dptr(), (int8_t*)out.dptr(), in.size));
  return out;
}
Tensor<s8_t> max_pool2d_s8(Tensor<s8_t>& in, ssize_t k, ssize_t s) {
  Tensor<s8_t> out(pool_shape(in, k, s));
  out.scale = in.scale;  // src/functional.cc:43-44
  out.zero_point = in.zero_point;
  check(i8ie_maxpool2d_s8(ctx(), (const int8_t*)in.dptr(), (int8_t*)out.dptr(), (int)in.shape[0], (int)in.shape[1],
                          (int)in.shape[2], (int)in.shape[3], (int)k, (int)s));
  return out;
}
Tensor<float> max_pool2d_f32(Tensor<float>& in, ssize_t k, ssize_t s) {
  Tensor<float> out(pool_shape(in, k, s));
  check(i8ie_maxpool2d_f32(ctx(), in.dptr(), out.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2],
                           (int)in.shape[3], (int)k, (int)s));
  return out;
}

// -------------------------------------------------------------- calibrator ----
// src/calibrator.cc:6-37, include/calibrator.h:4-14
constexpr ssize_t kNumSamples = 1000;
struct Calibrator {
  std::array<float, kNumSamples> samples{};  // value-initialised (make_unique<Calibrator>(), src/layer.cc:33)
  ssize_t cnt = 0;
  // device-side sampling (i8ie_calib_sample_f32): the 1000 slots live on the GPU until get_range()
  float* samples_dev = nullptr;
  int* scratch_dev = nullptr;
  int64_t seen = 0;
  uint64_t dev_seed = 0;
  Calibrator() = default;
  Calibrator(const Calibrator&) = delete;
  Calibrator& operator=(const Calibrator&) = delete;
  ~Calibrator() {
    if (samples_dev) i8ie_free(rt().ctx, samples_dev);
    if (scratch_dev) i8ie_free(rt().ctx, scratch_dev);
  }
  static bool on_device() { return rt().calib_mode == 2 || (rt().calib_mode == 0 && rt().calib_seed < 0); }
  void sample_device(const float* dptr, ssize_t n) {
    if (!samples_dev) {
      check(i8ie_malloc(rt().ctx, kNumSamples * sizeof(float), (void**)&samples_dev));
      check(i8ie_malloc(rt().ctx, kNumSamples * sizeof(int), (void**)&scratch_dev));
      check(i8ie_memset(rt().ctx, samples_dev, 0, kNumSamples * sizeof(float)));
      if (rt().calib_seed >= 0) {
        dev_seed = (uint64_t)rt().calib_seed;
      } else {
        std::random_device rd;
        dev_seed = ((uint64_t)rd() << 32) | rd();
      }
    }
    check(i8ie_calib_sample_f32(rt().ctx, dptr, (int64_t)n, seen, dev_seed, samples_dev, scratch_dev));
    seen += n;
    cnt = seen < kNumSamples ? (ssize_t)seen : kNumSamples;
  }
  void sample(const float* data, ssize_t n) {
    std::mt19937 rng;
    if (rt().calib_seed >= 0) {
      rng.seed((unsigned)rt().calib_seed);
    } else {
      std::random_device rd;
      rng.seed(rd());
    }
    std::uniform_int_distribution<ssize_t> dist(0, kNumSamples * 2);  // about half get sampled
    for (ssize_t i = 0; i < n; ++i) {
      if (cnt < kNumSamples) {
        samples[cnt++] = data[i];
      } else {
        ssize_t idx = dist(rng);
        if (idx < kNumSamples) samples[idx] = data[i];
      }
    }
  }
  std::tuple<float, u8_t> get_range(float quantile) {
    if (samples_dev) check(i8ie_memcpy_d2h(rt().ctx, samples.data(), samples_dev, kNumSamples * sizeof(float)));
    std::sort(samples.begin(), samples.end());
    float out_min = samples[(size_t)((1.0 - quantile) * cnt)];
    float out_max = samples[(size_t)(quantile * (cnt - 1))];
    out_min = std::fmin(out_min, 0.);
    out_max = std::fmax(out_max, 0.);
    u8_t zp = (u8_t)(255 * (0 - out_min) / (out_max - out_min + 1e-09));
    float scale = (zp == 0) ? (out_max - out_min) / 255 : (0 - out_min) / zp;
    if (scale == 0) scale = 1;
    return std::make_tuple(scale, zp);
  }
};

// what a preparing layer (or Add) does with its FP32 result: src/conv2d.cc:94-96, src/fully_connected.cc:17-19
void calib_sample(Calibrator& cal, Tensor<float>& out) {
  if (Calibrator::on_device()) {  // no copy of the layer output to the host
    cal.sample_device(out.dptr(), out.size);
    return;
  }
  py::array_t<float> a = out.numpy();
  cal.sample(a.data(), out.size);
}

// ------------------------------------------------------------------ layers ----
// The prepare / convert state machine of src/layer.cc:28-54 around a layer's output (scale, zero_point): what the layers with
// weights and those without share.
class QuantState {
 public:
  QuantState() = default;
  QuantState(const QuantState&) = delete;
  QuantState& operator=(const QuantState&) = delete;
  void prepare() {  // src/layer.cc:28-35
    if (is_quantized_) {
      std::cerr << "already quantized" << std::endl;
      return;
    }
    cal_ = std::make_unique<Calibrator>();
    is_preparing_ = true;
  }
  void set_output_qparams(float s, int zp) {  // additive: inject what calibration would produce
    check_zero_point(zp);
    scale_ = s;
    zero_point_ = (u8_t)zp;
    qparams_overridden_ = true;
    output_qparams_changed();
  }
  std::tuple<float, int> output_qparams() const { return std::make_tuple(scale_, (int)zero_point_); }
  bool is_quantized() const { return is_quantized_; }

 protected:
  ~QuantState() = default;
  virtual void output_qparams_changed() {}  // (a layer with a live handle pushes them into it)
  // the calibration half of convert() (src/layer.cc:36-47): false when the layer is quantized already
  bool convert_qparams() {
    if (is_quantized_) {
      std::cerr << "already quantized" << std::endl;
      return false;
    }
    if (!is_preparing_) {
      if (!qparams_overridden_) std::cerr << "No prepared, use default config" << std::endl;
    } else {
      float s;
      u8_t z;
      std::tie(s, z) = cal_->get_range(1);
      if (!qparams_overridden_) {
        scale_ = s;
        zero_point_ = z;
      }
      cal_.reset();
    }
    return true;
  }
  void set_quantized() {
    cal_.reset();
    is_preparing_ = false;
    is_quantized_ = true;
  }
  void maybe_sample(Tensor<float>& out) {  // src/conv2d.cc:94-96, src/fully_connected.cc:17-19
    if (is_preparing_) calib_sample(*cal_, out);
  }

  std::unique_ptr<Calibrator> cal_;
  bool is_preparing_ = false;
  bool is_quantized_ = false;
  bool qparams_overridden_ = false;
  float scale_ = 1;       // include/layer.h:46
  u8_t zero_point_ = 0;   // include/layer.h:47
};

// x.reshape(n, -1) of a border-free NHWC activation of m images that still lies as its conv left it: its storage (a Linear
// layer then walks K in (h, w, c) order instead of asking for the reference's order), or null
const Storage* flattened_nhwc(const Tensor<u8_t>& t, int m) {
  const Storage* s = t.st.get();
  const bool yes = s && s->layout == I8IE_LAYOUT_NHWC && s->border == 0 && s->dn == m && s->dh * s->dw > 1 &&
                   (ssize_t)s->dn * s->dc * s->dh * s->dw == t.size;
  return yes ? s : nullptr;
}

class BaseLayer : public QuantState {
 public:
  BaseLayer(std::vector<ssize_t> wshape, ssize_t out_channel) : wshape_(std::move(wshape)) {
    ssize_t n = 1;
    for (ssize_t d : wshape_) n *= d;
    w_.assign((size_t)n, 0.0f);
    b_.assign((size_t)out_channel, 0.0f);
    has_fp32_ = true;
  }
  BaseLayer(py::array_t<float, py::array::c_style | py::array::forcecast> w,
            py::array_t<float, py::array::c_style | py::array::forcecast> b) {
    has_fp32_ = true;
    load_weight(w);
    load_bias(b);
  }
  virtual ~BaseLayer() { release_fp32_dev(); }

  void load_weight(py::array_t<float, py::array::c_style | py::array::forcecast> w) {  // include/layer.h:15-20
    if (!has_fp32_) throw std::runtime_error("i8ie: load_weight: layer is already converted");
    check_weight_shape(std::vector<ssize_t>(w.shape(), w.shape() + w.ndim()), "load_weight");
    wshape_.assign(w.shape(), w.shape() + w.ndim());
    w_.assign(w.data(), w.data() + w.size());
    release_fp32_dev();
  }
  void load_bias(py::array_t<float, py::array::c_style | py::array::forcecast> b) {  // include/layer.h:21-26
    if (!has_fp32_) throw std::runtime_error("i8ie: load_bias: layer is already converted");
    b_.assign(b.data(), b.data() + b.size());
    release_fp32_dev();
  }
  void convert(bool per_channel = false) {  // src/layer.cc:36-54 (per_channel: the opt-in per-output-channel rule)
    if (!convert_qparams()) return;
    check_shapes();
    const ssize_t n = (ssize_t)b_.size();
    qw_.resize(w_.size());
    qb_.resize(b_.size());
    per_channel_ = per_channel;
    if (per_channel) {
      w_scales_.assign((size_t)n, 0.0f);
      check(i8ie_quantize_weight_per_channel(w_.data(), (int)n, (int64_t)(w_.size() / n), b_.data(),
                                             reinterpret_cast<int8_t*>(qw_.data()), reinterpret_cast<int8_t*>(qb_.data()),
                                             w_scales_.data()));
      w_scale_ = 1;
    } else {
      check(i8ie_quantize_weight(w_.data(), (int64_t)w_.size(), b_.data(), (int64_t)b_.size(),
                                 reinterpret_cast<int8_t*>(qw_.data()), reinterpret_cast<int8_t*>(qb_.data()),
                                 &w_scale_));
    }
    install_handle();
  }
  // additive: restore a converted layer from saved INT8 weights (what convert() would have produced)
  // w_scale: a number (per-tensor layer) or an array of one scale per output feature (per-channel layer)
  void load_quantized(py::array_t<s8_t, py::array::c_style | py::array::forcecast> qw,
                      py::array_t<s8_t, py::array::c_style | py::array::forcecast> qb, py::object w_scale, float s_out,
                      int zp_out) {
    check_zero_point(zp_out);
    std::vector<ssize_t> shp(qw.shape(), qw.shape() + qw.ndim());
    if (shp.size() != wshape_.size()) throw std::runtime_error("i8ie: load_quantized: weight rank mismatch");
    check_weight_shape(shp, "load_quantized");
    wshape_ = shp;
    if (qb.size() != wshape_[0]) throw std::runtime_error("i8ie: load_quantized: bias size mismatch");
    const bool pc = py::isinstance<py::array>(w_scale) ? py::array(w_scale).ndim() > 0
                                                        : (py::isinstance<py::list>(w_scale) || py::isinstance<py::tuple>(w_scale));
    std::vector<float> scales;
    if (pc) {
      auto a = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(w_scale);
      if (!a || a.ndim() != 1 || a.size() != wshape_[0])
        throw std::runtime_error("i8ie: load_quantized: weight_scale array must hold one scale per output feature");
      scales.assign(a.data(), a.data() + a.size());
    }
    qw_.assign(qw.data(), qw.data() + qw.size());
    qb_.assign(qb.data(), qb.data() + qb.size());
    per_channel_ = pc;
    w_scales_ = scales;
    w_scale_ = pc ? 1.0f : w_scale.cast<float>();
    scale_ = s_out;
    zero_point_ = (u8_t)zp_out;
    qparams_overridden_ = true;
    install_handle();
  }
  py::array_t<s8_t> q_weight() const {
    need_quantized();
    py::array_t<s8_t> a(wshape_);
    std::memcpy(a.mutable_data(), qw_.data(), qw_.size());
    return a;
  }
  py::array_t<s8_t> q_bias() const {
    need_quantized();
    py::array_t<s8_t> a((ssize_t)qb_.size());
    std::memcpy(a.mutable_data(), qb_.data(), qb_.size());
    return a;
  }
  float weight_scale() const {
    need_quantized();
    if (per_channel_) throw std::runtime_error("i8ie: weight_scale: per-channel layer (use weight_scales())");
    return w_scale_;
  }
  py::array_t<float> weight_scales() const {  // float32 [out] in both modes (i8ie_layer_weight_scales)
    need_quantized();
    py::array_t<float> a((ssize_t)qb_.size());
    int pc = 0;
    check(i8ie_layer_weight_scales(q_.get(), a.mutable_data(), (int)qb_.size(), &pc));
    return a;
  }
  bool is_per_channel() const { return is_quantized_ && per_channel_; }

 protected:
  void output_qparams_changed() override {
    if (q_) check(i8ie_layer_set_output_qparams(q_.get(), scale_, zero_point_));
  }
  // the tail convert() and load_quantized() share: the library's layer from the INT8 weights, the output qparams into it,
  // the FP32 weights released (src/layer.cc:52-53), the state flipped
  void install_handle() {
    i8ie_layer* raw = make_handle((ssize_t)qb_.size());
    q_ = std::shared_ptr<i8ie_layer>(raw, [](i8ie_layer* l) { i8ie_layer_destroy(l); });
    check(i8ie_layer_set_output_qparams(q_.get(), scale_, zero_point_));
    set_quantized();
    std::vector<float>().swap(w_);
    std::vector<float>().swap(b_);
    has_fp32_ = false;
    release_fp32_dev();
  }
  virtual void check_shapes() const = 0;
  // a layer that was given its channel counts refuses a weight of another shape (Conv2d with groups: [out, in/groups, k, k])
  virtual void check_weight_shape(const std::vector<ssize_t>&, const char*) const {}
  virtual i8ie_layer* make_handle(ssize_t n) = 0;
  // Deferred INT8 forward: returns a tensor whose launch happens when it is first needed.
  Tensor<u8_t> defer(Tensor<u8_t>& in, std::vector<ssize_t> oshape, int m, int h, int w, bool spatial) {
    Tensor<u8_t> out = pending_u8(std::move(oshape), scale_, zero_point_);
    std::shared_ptr<i8ie_layer> handle = q_;
    Tensor<u8_t> src = in;  // shares the input's storage / pending launch
    const float s_in = in.scale;
    const u8_t zp_in = in.zero_point;
    const int zp_out = zero_point_;
    const std::vector<ssize_t> oshp = out.shape;
    const size_t obytes = (size_t)out.size;
    // One recorded conv / linear forward, with or without a max-pool folded in behind it (pk > 1).  Negotiates the
    // layouts at both ends with the library: a conv whose kernel reads re-biased bytes asks its producer for them, and
    // stores re-biased itself when its consumer asked and its kernel can (i8ie_layer_rebiased_io).
    auto run = [handle, s_in, zp_in, zp_out, m, spatial, oshp, obytes](Tensor<u8_t>& src, int h, int w, bool relu, int border, bool s8,
                                                                        int pk, int ps) -> std::shared_ptr<Storage> {
      int out_layout = I8IE_LAYOUT_NCHW, pad = 0;
      if (spatial) {
        check(i8ie_layer_preferred_layout(handle.get(), &out_layout));
        check(i8ie_layer_padding(handle.get(), &pad));
      }
      const bool pool = pk > 1 || (pk == 1 && ps > 1);  // (a subsampling 1 x 1 window is a pool: the library runs it unfused)
      if (pool && out_layout != I8IE_LAYOUT_NHWC) return nullptr;  // (the caller pools the unfused result)
      std::vector<ssize_t> rshp = oshp;
      if (pool) {
        rshp[2] = (oshp[2] - pk) / ps + 1;
        rshp[3] = (oshp[3] - pk) / ps + 1;
      }
      int reads = 0, stores = 0;
      if (spatial && out_layout == I8IE_LAYOUT_NHWC) check(i8ie_layer_rebiased_io(handle.get(), m, h, w, pool ? pk : 0, ps, &reads, &stores));
      const bool st_s8 = s8 && stores;
      if (spatial && out_layout == I8IE_LAYOUT_NHWC && src.pend && src.qsrc && !src.pend_relu) {
        int yes = 0;
        check(i8ie_layer_accepts_f32_input(handle.get(), h, w, &yes));
        if (yes) {  // quantize + conv (+ relu) (+ max-pool) in one kernel, reading the FP32 input
          auto st = nhwc_storage(rshp, border, zp_out, st_s8);
          check(i8ie_layer_forward_f32_input_pool(handle.get(), (const float*)src.qsrc->device_ptr(), m, h, w, src.qscale, src.qzp,
                                                  relu ? 1 : 0, pool ? pk : 0, ps, (uint8_t*)st->dev,
                                                  st_s8 ? I8IE_LAYOUT_NHWC_S8 : I8IE_LAYOUT_NHWC, border, nullptr));
          return st;
        }
      }
      const uint8_t* ip;
      if (spatial) {
        // ask a still-pending producer for a zero-point border that covers this conv's padding (and for re-biased bytes
        // when this layer's kernel reads them as they are)
        src.realize(out_layout == I8IE_LAYOUT_NHWC ? pad : 0, reads != 0);
        ip = (src.st && src.st->s8 && reads) ? src.dptr_raw() : src.dptr_any();
      } else {
        src.realize(0);
        if (const Storage* s = flattened_nhwc(src, m)) {
          ip = src.dptr_any();
          h = s->dh;
          w = s->dw;
        } else {
          ip = src.dptr();
        }
      }
      const int in_layout = src.st->s8 ? I8IE_LAYOUT_NHWC_S8 : src.st->layout, in_border = src.st->border;
      const int ob = out_layout == I8IE_LAYOUT_NHWC ? border : 0;
      auto st = out_layout == I8IE_LAYOUT_NHWC ? nhwc_storage(rshp, ob, zp_out, st_s8) : device_storage(obytes);
      const int ol = st_s8 ? I8IE_LAYOUT_NHWC_S8 : out_layout;
      if (pool)
        check(i8ie_layer_forward_pool(handle.get(), ip, in_layout, in_border, m, h, w, s_in, zp_in, relu ? 1 : 0, pk, ps,
                                      (uint8_t*)st->dev, ol, ob, nullptr));
      else
        check(i8ie_layer_forward_fused(handle.get(), ip, in_layout, in_border, m, h, w, s_in, zp_in, relu ? 1 : 0,
                                       (uint8_t*)st->dev, ol, ob, nullptr));
      // (the input is released when the last tensor holding this closure lets go of it: right after the
      // launch in `x = relu(layer(x))`, later if the un-fused result is observed as well)
      return st;
    };
    out.pend = make_pend([run, src, h, w](bool relu, int border, bool s8) mutable { return run(src, h, w, relu, border, s8, 0, 0); },
                         {in.pend});
    if (spatial) {
      // max_pool2d right behind this (relu'd) conv: one call of the library, which folds the pool into the convolution's
      // epilogue where a kernel of its can and runs the max-pool kernel behind it otherwise
      Tensor<u8_t> srcp = in;
      out.pend->fn_pool = [run, srcp, h, w](bool relu, int border, bool s8, int pk, int ps) mutable {
        return run(srcp, h, w, relu, border, s8, pk, ps);
      };
    }
    if (!spatial && out.shape.size() == 2 && out.shape[1] <= 16) {
      // dequantize(layer(x)) of a classifier head: one fused launch (i8ie_layer_forward_dequant)
      Tensor<u8_t> src2 = in;
      out.pend_f32 = std::make_shared<std::function<std::shared_ptr<Storage>(bool)>>(
          [handle, src2, s_in, zp_in, m, obytes](bool relu) mutable {
            src2.realize(0);
            const uint8_t* ip;
            int lay = I8IE_LAYOUT_NCHW, hh = 0, ww = 0;
            if (const Storage* s = flattened_nhwc(src2, m)) {
              ip = src2.dptr_any();
              lay = I8IE_LAYOUT_NHWC;
              hh = s->dh;
              ww = s->dw;
            } else {
              ip = src2.dptr();
            }
            auto f = device_storage(obytes * sizeof(float));
            auto q = device_storage(obytes);  // u8 side output: only written when the fused kernel does not apply
            check(i8ie_layer_forward_dequant(handle.get(), ip, lay, m, hh, ww, s_in, zp_in, relu ? 1 : 0,
                                             (uint8_t*)q->dev, (float*)f->dev));
            return f;
          });
    }
    return out;
  }
  // forward_debug: the eager forward in the reference's order, with the int32 accumulators (shape `ashape`) beside the result
  std::tuple<Tensor<u8_t>, py::object> forward_acc(Tensor<u8_t>& in, std::vector<ssize_t> oshape, std::vector<ssize_t> ashape, int m, int h,
                                                   int w) {
    Tensor<u8_t> out = pending_u8(std::move(oshape), scale_, zero_point_);
    out.st = device_storage((size_t)out.size);
    Tensor<int32_t> acc(std::move(ashape));
    check(i8ie_layer_forward(q_.get(), in.dptr(), m, h, w, in.scale, in.zero_point, out.dptr(), acc.dptr()));
    py::object acc_np = acc.numpy();
    return std::make_tuple(std::move(out), acc_np);
  }
  // Conv2d / ConvTranspose2d on a u8 tensor: recorded, or the debug forward
  std::tuple<Tensor<u8_t>, py::object> forward_spatial_u8(Tensor<u8_t>& in, std::vector<ssize_t> oshape, bool want_acc) {
    const int n = (int)in.shape[0], h = (int)in.shape[2], w = (int)in.shape[3];
    if (!want_acc) return std::make_tuple(defer(in, oshape, n, h, w, true), py::object(py::none()));
    return forward_acc(in, oshape, {oshape[0], oshape[2] * oshape[3], oshape[1]}, n, h, w);
  }
  void need_quantized() const {
    if (!is_quantized_) throw std::runtime_error("i8ie: layer is not converted (call convert() first)");
  }
  void need_fp32() const {
    if (!has_fp32_)
      throw std::runtime_error("i8ie: FP32 input given to a converted layer (its FP32 weights were released)");
  }
  void upload_fp32() {
    if (w_dev_) return;
    check(i8ie_malloc(ctx(), w_.size() * 4, (void**)&w_dev_));
    check(i8ie_malloc(ctx(), b_.size() * 4, (void**)&b_dev_));
    check(i8ie_memcpy_h2d(ctx(), w_dev_, w_.data(), w_.size() * 4));
    check(i8ie_memcpy_h2d(ctx(), b_dev_, b_.data(), b_.size() * 4));
  }
  void release_fp32_dev() {
    if (rt().ctx) {
      if (w_dev_) i8ie_free(rt().ctx, w_dev_);
      if (b_dev_) i8ie_free(rt().ctx, b_dev_);
    }
    w_dev_ = b_dev_ = nullptr;
  }

  std::vector<ssize_t> wshape_;
  std::vector<float> w_, b_;
  bool has_fp32_ = false;
  float* w_dev_ = nullptr;
  float* b_dev_ = nullptr;
  std::vector<s8_t> qw_, qb_;
  float w_scale_ = 1;
  bool per_channel_ = false;
  std::vector<float> w_scales_;  // per-channel layers: s_w[j]
  std::shared_ptr<i8ie_layer> q_;
};

class Linear : public BaseLayer {
 public:
  Linear(ssize_t in_channel, ssize_t out_channel) : BaseLayer({out_channel, in_channel}, out_channel) {}
  using BaseLayer::BaseLayer;

  Tensor<float> forward_f32(Tensor<float>& in) {  // src/fully_connected.cc:5-21
    need_fp32();
    check_shapes();
    const ssize_t n = wshape_[0], k = wshape_[1];
    if (in.shape.empty() || in.size % k != 0 || in.shape.back() != k)
      throw std::runtime_error("i8ie: Linear: input's last dimension must equal in_features");
    const ssize_t m = in.size / k;
    upload_fp32();
    Tensor<float> out({m, n});
    check(i8ie_linear_f32(ctx(), in.dptr(), (int)m, (int)k, w_dev_, b_dev_, (int)n, out.dptr()));
    maybe_sample(out);
    return out;
  }
  std::tuple<Tensor<u8_t>, py::object> forward_u8(Tensor<u8_t>& in, bool want_acc) {  // src/fully_connected.cc:22-52
    need_quantized();
    const ssize_t n = wshape_[0], k = wshape_[1];
    if (in.shape.empty() || in.shape.back() != k)
      throw std::runtime_error("i8ie: Linear: input's last dimension must equal in_features");
    const ssize_t m = in.size / k;
    if (!want_acc) return std::make_tuple(defer(in, {m, n}, (int)m, 0, 0, false), py::object(py::none()));
    return forward_acc(in, {m, n}, {m, n}, (int)m, 0, 0);
  }

 protected:
  void check_shapes() const override {
    if (wshape_.size() != 2) throw std::runtime_error("i8ie: Linear weight must be [out_features, in_features]");
    if (has_fp32_ && (ssize_t)b_.size() != wshape_[0]) throw std::runtime_error("i8ie: Linear bias size mismatch");
  }
  i8ie_layer* make_handle(ssize_t n) override {
    i8ie_layer* l = nullptr;
    if (per_channel_)
      check(i8ie_linear_create_per_channel(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                           reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)wshape_[1],
                                           w_scales_.data(), &l));
    else
      check(i8ie_linear_create(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                               reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)wshape_[1], w_scale_, &l));
    return l;
  }
};

class Conv2d : public BaseLayer {
 public:
  // groups: not in the reference (src/conv2d.cc:100-142 per group); the weight is [out, in / groups, k, k]
  // dilation: not in the reference either (torch.nn.Conv2d's dilation=, one integer)
  Conv2d(ssize_t in_channel, ssize_t out_channel, ssize_t kernel_size, ssize_t stride, ssize_t padding, ssize_t groups = 1,
         ssize_t dilation = 1)
      : BaseLayer({out_channel, checked_cg(in_channel, out_channel, groups), kernel_size, kernel_size}, out_channel),
        stride_(stride), padding_(padding), groups_(groups), dilation_(dilation), in_channels_(in_channel) {
    if (dilation < 1) throw std::runtime_error("i8ie: Conv2d: dilation must be >= 1");
    if (stride == 0) throw std::runtime_error("i8ie: Conv2d: stride must not be 0");  // include/conv2d.h:12-14
    if (stride < 0 || padding < 0) throw std::runtime_error("i8ie: Conv2d: negative stride/padding");
  }
  // include/conv2d.h:16-17 leaves stride_/padding_ uninitialised for these two
  // constructors; they are 1 / 0 here.
  Conv2d(py::array_t<float, py::array::c_style | py::array::forcecast> w,
         py::array_t<float, py::array::c_style | py::array::forcecast> b)
      : BaseLayer(w, b) {}

  std::vector<ssize_t> out_shape(const std::vector<ssize_t>& s) const {
    if (s.size() != 4) throw std::runtime_error("i8ie: Conv2d expects an NCHW tensor");
    if (s[1] != in_channels()) throw std::runtime_error("i8ie: Conv2d: input channels do not match the weight");
    const ssize_t kh = dilation_ * (wshape_[2] - 1) + 1, kw = dilation_ * (wshape_[3] - 1) + 1;  // the kernel's extent
    if (s[2] - kh + 2 * padding_ < 0 || s[3] - kw + 2 * padding_ < 0)
      throw std::runtime_error(dilation_ > 1 ? "i8ie: Conv2d: dilated kernel larger than the padded input"
                                             : "i8ie: Conv2d: kernel larger than the padded input");
    return {s[0], wshape_[0], (s[2] - kh + 2 * padding_) / stride_ + 1, (s[3] - kw + 2 * padding_) / stride_ + 1};
  }
  Tensor<float> forward_f32(Tensor<float>& in) {  // src/conv2d.cc:63-98
    need_fp32();
    check_shapes();
    Tensor<float> out(out_shape(in.shape));
    upload_fp32();
    check(i8ie_conv2d_f32_dilated(ctx(), in.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3],
                                  w_dev_, b_dev_, (int)wshape_[0], (int)wshape_[2], (int)wshape_[3], (int)stride_,
                                  (int)padding_, (int)groups_, (int)dilation_, out.dptr()));
    maybe_sample(out);
    return out;
  }
  std::tuple<Tensor<u8_t>, py::object> forward_u8(Tensor<u8_t>& in, bool want_acc) {  // src/conv2d.cc:100-142
    need_quantized();
    return forward_spatial_u8(in, out_shape(in.shape), want_acc);
  }

 protected:
  void check_shapes() const override {
    if (wshape_.size() != 4) throw std::runtime_error("i8ie: Conv2d weight must be [out, in, kh, kw]");
    if (has_fp32_ && (ssize_t)b_.size() != wshape_[0]) throw std::runtime_error("i8ie: Conv2d bias size mismatch");
  }
  void check_weight_shape(const std::vector<ssize_t>& shp, const char* what) const override {
    if (in_channels_ <= 0) return;  // (built from arrays: the weight defines the layer)
    if (shp.size() != 4 || shp[0] != wshape_[0] || shp[1] != in_channels_ / groups_ || shp[2] != wshape_[2] || shp[3] != wshape_[3])
      throw std::runtime_error(std::string("i8ie: Conv2d: ") + what + ": weight must be [out, in / groups, k, k]");
  }
  i8ie_layer* make_handle(ssize_t n) override {
    i8ie_layer* l = nullptr;
    if (per_channel_)
      check(i8ie_conv2d_create_dilated_per_channel(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                                   reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)in_channels(),
                                                   (int)wshape_[2], (int)wshape_[3], (int)stride_, (int)padding_,
                                                   (int)groups_, (int)dilation_, w_scales_.data(), &l));
    else
      check(i8ie_conv2d_create_dilated(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                       reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)in_channels(),
                                       (int)wshape_[2], (int)wshape_[3], (int)stride_, (int)padding_, (int)groups_,
                                       (int)dilation_, w_scale_, &l));
    return l;
  }

 public:
  ssize_t groups() const { return groups_; }
  ssize_t dilation() const { return dilation_; }

 private:
  static ssize_t checked_cg(ssize_t in_channel, ssize_t out_channel, ssize_t groups) {
    if (groups < 1) throw std::runtime_error("i8ie: Conv2d: groups must be >= 1");
    if (in_channel % groups != 0 || out_channel % groups != 0)
      throw std::runtime_error("i8ie: Conv2d: groups must divide in_channels and out_channels");
    return in_channel / groups;
  }
  ssize_t in_channels() const { return wshape_[1] * groups_; }
  ssize_t stride_ = 1;
  ssize_t padding_ = 0;
  ssize_t groups_ = 1;
  ssize_t dilation_ = 1;
  ssize_t in_channels_ = 0;  // as constructed from sizes (0: constructed from arrays)
};

// ConvTranspose2d (additive, not in the reference): torch.nn.ConvTranspose2d with a square kernel, groups = 1, dilation = 1.
// The layer is the reference convolution of the equivalent zero-inserted problem (include/i8ie_hip.h,
// i8ie_conv_transpose2d_create), so the weights are held as the equivalent kernel W~ [out, in, k, k],
// W~[oc][ic][ky][kx] = W[ic][oc][k-1-ky][k-1-kx]: convert() quantises W~ by the layers' own rules (per tensor over weight and
// bias; per row of W~ with row_len = in*k*k).  load_weight / load_quantized take and q_weight gives torch's [in, out, k, k].
class ConvTranspose2d : public BaseLayer {
 public:
  ConvTranspose2d(ssize_t in_channel, ssize_t out_channel, ssize_t kernel_size, ssize_t stride, ssize_t padding, ssize_t output_padding)
      : BaseLayer({checked(out_channel, in_channel, kernel_size, stride, padding, output_padding), in_channel, kernel_size, kernel_size},
                  out_channel),
        stride_(stride), padding_(padding), opad_(output_padding) {}

  // torch's [in, out, k, k] <-> the equivalent [out, in, k, k] (the same map both ways round, with the outer sizes swapped)
  template <typename T>
  static std::vector<T> swap_flip(const T* src, ssize_t a, ssize_t b, ssize_t k) {  // src [a][b][k][k] -> [b][a][k][k], flipped
    std::vector<T> dst((size_t)(a * b * k * k));
    for (ssize_t i = 0; i < a; ++i)
      for (ssize_t j = 0; j < b; ++j)
        for (ssize_t y = 0; y < k; ++y)
          for (ssize_t x = 0; x < k; ++x)
            dst[(size_t)(((j * a + i) * k + (k - 1 - y)) * k + (k - 1 - x))] = src[(size_t)(((i * b + j) * k + y) * k + x)];
    return dst;
  }
  void check_torch_shape(const std::vector<ssize_t>& shp, const char* what) const {
    if (shp.size() != 4 || shp[0] != wshape_[1] || shp[1] != wshape_[0] || shp[2] != wshape_[2] || shp[3] != wshape_[3])
      throw std::runtime_error(std::string("i8ie: ConvTranspose2d: ") + what + ": weight must be [in, out, k, k]");
  }
  void load_weight(py::array_t<float, py::array::c_style | py::array::forcecast> w) {
    if (!has_fp32_) throw std::runtime_error("i8ie: load_weight: layer is already converted");
    check_torch_shape(std::vector<ssize_t>(w.shape(), w.shape() + w.ndim()), "load_weight");
    w_ = swap_flip<float>(w.data(), wshape_[1], wshape_[0], wshape_[2]);
    wt_.assign(w.data(), w.data() + w.size());
    release_fp32_dev();
  }
  void load_quantized(py::array_t<s8_t, py::array::c_style | py::array::forcecast> qw,
                      py::array_t<s8_t, py::array::c_style | py::array::forcecast> qb, py::object w_scale, float s_out, int zp_out) {
    check_torch_shape(std::vector<ssize_t>(qw.shape(), qw.shape() + qw.ndim()), "load_quantized");
    std::vector<s8_t> eq = swap_flip<s8_t>(qw.data(), wshape_[1], wshape_[0], wshape_[2]);
    py::array_t<s8_t> a(wshape_);
    std::memcpy(a.mutable_data(), eq.data(), eq.size());
    BaseLayer::load_quantized(a, qb, w_scale, s_out, zp_out);
    std::vector<float>().swap(wt_);
  }
  void convert(bool per_channel = false) {
    BaseLayer::convert(per_channel);
    if (is_quantized_) std::vector<float>().swap(wt_);
  }
  py::array_t<s8_t> q_weight() const {
    need_quantized();
    std::vector<s8_t> t = swap_flip<s8_t>(qw_.data(), wshape_[0], wshape_[1], wshape_[2]);
    py::array_t<s8_t> a(std::vector<ssize_t>{wshape_[1], wshape_[0], wshape_[2], wshape_[3]});
    std::memcpy(a.mutable_data(), t.data(), t.size());
    return a;
  }

  std::vector<ssize_t> out_shape(const std::vector<ssize_t>& s) const {
    if (s.size() != 4) throw std::runtime_error("i8ie: ConvTranspose2d expects an NCHW tensor");
    if (s[1] != wshape_[1]) throw std::runtime_error("i8ie: ConvTranspose2d: input channels do not match the weight");
    const ssize_t k = wshape_[2];
    const ssize_t oh = (s[2] - 1) * stride_ - 2 * padding_ + k + opad_, ow = (s[3] - 1) * stride_ - 2 * padding_ + k + opad_;
    if (s[2] < 1 || s[3] < 1 || oh < 1 || ow < 1) throw std::runtime_error("i8ie: ConvTranspose2d: empty output");
    return {s[0], wshape_[0], oh, ow};
  }
  Tensor<float> forward_f32(Tensor<float>& in) {
    need_fp32();
    Tensor<float> out(out_shape(in.shape));
    if (!w_dev_) {  // (the FP32 kernel reads torch's layout)
      if (wt_.empty()) wt_ = swap_flip<float>(w_.data(), wshape_[0], wshape_[1], wshape_[2]);
      check(i8ie_malloc(ctx(), wt_.size() * 4, (void**)&w_dev_));
      check(i8ie_malloc(ctx(), b_.size() * 4, (void**)&b_dev_));
      check(i8ie_memcpy_h2d(ctx(), w_dev_, wt_.data(), wt_.size() * 4));
      check(i8ie_memcpy_h2d(ctx(), b_dev_, b_.data(), b_.size() * 4));
    }
    check(i8ie_conv_transpose2d_f32(ctx(), in.dptr(), (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3],
                                    w_dev_, b_dev_, (int)wshape_[0], (int)wshape_[2], (int)stride_, (int)padding_, (int)opad_,
                                    out.dptr()));
    maybe_sample(out);
    return out;
  }
  std::tuple<Tensor<u8_t>, py::object> forward_u8(Tensor<u8_t>& in, bool want_acc) {
    need_quantized();
    return forward_spatial_u8(in, out_shape(in.shape), want_acc);
  }

 protected:
  void check_shapes() const override {
    if (wshape_.size() != 4) throw std::runtime_error("i8ie: ConvTranspose2d weight must be [in, out, k, k]");
    if (has_fp32_ && (ssize_t)b_.size() != wshape_[0]) throw std::runtime_error("i8ie: ConvTranspose2d bias size mismatch");
  }
  i8ie_layer* make_handle(ssize_t n) override {
    i8ie_layer* l = nullptr;
    if (per_channel_)
      check(i8ie_conv_transpose2d_create_per_channel(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                                     reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)wshape_[1],
                                                     (int)wshape_[2], (int)stride_, (int)padding_, (int)opad_,
                                                     w_scales_.data(), &l));
    else
      check(i8ie_conv_transpose2d_create(ctx(), reinterpret_cast<const int8_t*>(qw_.data()),
                                         reinterpret_cast<const int8_t*>(qb_.data()), (int)n, (int)wshape_[1], (int)wshape_[2],
                                         (int)stride_, (int)padding_, (int)opad_, w_scale_, &l));
    return l;
  }

 private:
  // the rules of the C entries (I8IE_ERR_ARG there), raised where Conv2d raises for bad groups
  static ssize_t checked(ssize_t out_channel, ssize_t in_channel, ssize_t k, ssize_t stride, ssize_t padding, ssize_t opad) {
    if (in_channel < 1 || out_channel < 1 || k < 1) throw std::runtime_error("i8ie: ConvTranspose2d: non-positive size");
    if (stride < 1) throw std::runtime_error("i8ie: ConvTranspose2d: stride must be >= 1");
    if (padding < 0 || padding > k - 1) throw std::runtime_error("i8ie: ConvTranspose2d: padding must be in [0, kernel_size - 1]");
    if (opad < 0 || opad >= stride) throw std::runtime_error("i8ie: ConvTranspose2d: output_padding must be in [0, stride)");
    return out_channel;
  }
  ssize_t stride_ = 1, padding_ = 0, opad_ = 0;
  std::vector<float> wt_;  // the FP32 weight as loaded (torch's layout), for the FP32 kernel
};

// A layer without weights (the residual Add, the channel Concat): the layers' prepare / convert state machine
// (src/layer.cc:28-54) around its output (scale, zero_point); FP32 tensors join in FP32 (and are sampled while preparing),
// u8 tensors after convert().
class Weightless : public QuantState {
 public:
  void convert(bool /*per_channel: there are no weights*/ = false) {
    if (convert_qparams()) set_quantized();
  }
  void load_quantized(float s_out, int zp_out) {  // what convert() would have left behind
    set_output_qparams(s_out, zp_out);
    set_quantized();
  }

 protected:
  Tensor<float> sampled(Tensor<float> out) {  // what a preparing layer does with its FP32 result
    maybe_sample(out);
    return out;
  }
  void need_quantized(const char* what) const {
    if (!is_quantized_) throw std::runtime_error(std::string("i8ie: ") + what + " is not converted (call convert() first)");
  }
};
class Add : public Weightless {
 public:
  Tensor<float> forward_f32(Tensor<float>& a, Tensor<float>& b) { return sampled(add_f32(a, b)); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& a, Tensor<u8_t>& b) {
    need_quantized("Add");
    return add_u8(a, b, scale_, zero_point_);
  }
};
// a * b; b has a's shape or is a's gate [n, c, 1, 1] / [n, c]
class Mul : public Weightless {
 public:
  Tensor<float> forward_f32(Tensor<float>& a, Tensor<float>& b) { return sampled(mul_f32(a, b)); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& a, Tensor<u8_t>& b) {
    mul_is_gate(a, b);
    need_quantized("Mul");
    return mul_u8(a, b, scale_, zero_point_);
  }
};
// a . b of two activation tensors (matmul_shape's rules), each optionally given transposed
class MatMul : public Weightless {
 public:
  MatMul(bool transpose_a, bool transpose_b) : ta_(transpose_a), tb_(transpose_b) {}
  Tensor<float> forward_f32(Tensor<float>& a, Tensor<float>& b) { return sampled(matmul_f32(a, b, ta_, tb_)); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& a, Tensor<u8_t>& b) {
    matmul_shape(a, b, ta_, tb_);
    need_quantized("MatMul");
    return matmul_u8(a, b, scale_, zero_point_, ta_, tb_);
  }
  bool transpose_a() const { return ta_; }
  bool transpose_b() const { return tb_; }

 private:
  bool ta_, tb_;
};
// multi-head attention of q, k, v (or one packed qkv tensor; attention_shape's rules): two calibrated parameter sets, the
// scores' (scale, zero_point) beside the output's.  While preparing, the FP32 scores are sampled by a calibrator of their own.
class Attention : public Weightless {
 public:
  explicit Attention(ssize_t heads) : heads_(heads) {
    if (heads < 1) throw std::runtime_error("i8ie: Attention: heads must be >= 1");
  }
  void prepare() {
    if (!is_quantized_) score_cal_ = std::make_unique<Calibrator>();
    QuantState::prepare();
  }
  void convert(bool /*per_channel: there are no weights*/ = false) {
    if (!is_quantized_ && is_preparing_ && score_cal_ && score_cal_->cnt > 0) {
      float s;
      u8_t z;
      std::tie(s, z) = score_cal_->get_range(1);
      if (!score_overridden_) {
        score_scale_ = s;
        score_zp_ = z;
      }
    }
    score_cal_.reset();
    Weightless::convert();
  }
  void set_score_qparams(float s, int zp) {  // inject what calibration would produce
    check_zero_point(zp);
    score_scale_ = s;
    score_zp_ = (u8_t)zp;
    score_overridden_ = true;
  }
  std::tuple<float, int> score_qparams() const { return std::make_tuple(score_scale_, (int)score_zp_); }
  void load_quantized(float s_out, int zp_out, float s_score, int zp_score) {  // what convert() would have left behind
    set_score_qparams(s_score, zp_score);
    Weightless::load_quantized(s_out, zp_out);
  }
  Tensor<float> forward_f32(Tensor<float>& q, Tensor<float>& k, Tensor<float>& v) { return run_f32(q, &k, &v); }
  Tensor<float> forward_f32_packed(Tensor<float>& qkv) { return run_f32(qkv, nullptr, nullptr); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& q, Tensor<u8_t>& k, Tensor<u8_t>& v) { return run_u8(q, &k, &v); }
  Tensor<u8_t> forward_u8_packed(Tensor<u8_t>& qkv) { return run_u8(qkv, nullptr, nullptr); }
  ssize_t heads() const { return heads_; }

 private:
  Tensor<float> run_f32(Tensor<float>& q, Tensor<float>* k, Tensor<float>* v) {
    if (!is_preparing_ || !score_cal_) return attention_f32(q, k, v, heads_, nullptr);
    const AttnShape s = attention_shape(q, k, v, heads_);
    Tensor<float> scores(std::vector<ssize_t>{s.b, s.heads, s.tq, s.tk});
    Tensor<float> out = attention_f32(q, k, v, heads_, &scores);
    calib_sample(*score_cal_, scores);
    return sampled(out);
  }
  Tensor<u8_t> run_u8(Tensor<u8_t>& q, Tensor<u8_t>* k, Tensor<u8_t>* v) {
    attention_shape(q, k, v, heads_);
    need_quantized("Attention");
    return attention_u8(q, k, v, heads_, score_scale_, score_zp_, scale_, zero_point_);
  }
  ssize_t heads_;
  std::unique_ptr<Calibrator> score_cal_;
  float score_scale_ = 1;
  u8_t score_zp_ = 0;
  bool score_overridden_ = false;
};
// cat along axis 1: a list of FP32 tensors before convert(), of u8 tensors after it
class Concat : public Weightless {
 public:
  py::object forward(const py::list& tensors) {
    if (!tensors.empty() && py::isinstance<Tensor<u8_t>>(tensors[0])) {
      std::vector<Tensor<u8_t>> ts = cat_list<u8_t>(tensors);
      cat_shape(ts);
      need_quantized("Concat");
      return py::cast(cat_u8(std::move(ts), scale_, zero_point_));
    }
    return py::cast(sampled(cat_f32(cat_list<float>(tensors))));
  }
};
// a table-driven activation (I8IE_ACT_*): f in FP32 before convert(), one table lookup from the input tensor's
// (scale, zero_point) to this layer's own output qparams after it
class Activation : public Weightless {
 public:
  Activation(int kind, float param) : kind_(kind), param_(param) {
    LutBytes probe;  // (an unknown kind or a slope that is not finite is refused here)
    check(i8ie_activation_table(kind, param, 1.0f, 0, 1.0f, 0, probe.data()));
  }
  Tensor<float> forward_f32(Tensor<float>& x) { return sampled(activation_f32(x, kind_, param_)); }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& x) {
    need_quantized("Activation");
    return activation_u8(x, kind_, param_, scale_, zero_point_);
  }
  int kind() const { return kind_; }
  float param() const { return param_; }

 private:
  int kind_;
  float param_;
};
// LayerNorm over the channel axis of [n, c, h, w] or the last axis of [m, f] / [b, t, f]: a layer with fp32 weight (gamma) and
// bias (beta) and the layers' prepare / convert state machine around its output (scale, zero_point).  There are no INT8
// weights: convert() computes g = gamma / s_out and b = beta / s_out + zp_out (i8ie_layernorm_affine) and uploads them once.
class LayerNorm : public QuantState {
 public:
  LayerNorm(ssize_t channels, float eps) : channels_(channels), eps_(eps) {
    if (channels < 1 || channels > 16384) throw std::runtime_error("i8ie: LayerNorm: channels must be in 1..16384");
    if (!(eps > 0) || !std::isfinite(eps)) throw std::runtime_error("i8ie: LayerNorm: eps must be positive and finite");
    gamma_.assign((size_t)channels, 1.0f);
    beta_.assign((size_t)channels, 0.0f);
  }
  void load_weight(const py::object& w) { gamma_ = layer_norm_param(w, channels_, 1.0f, "weight"); params_changed(); }
  void load_bias(const py::object& b) { beta_ = layer_norm_param(b, channels_, 0.0f, "bias"); params_changed(); }
  void convert(bool /*per_channel: there are no INT8 weights*/ = false) {
    if (!convert_qparams()) return;
    install();
  }
  void load_quantized(const py::object& w, const py::object& b, float s_out, int zp_out) {  // what convert() would have left behind
    check_zero_point(zp_out);
    gamma_ = layer_norm_param(w, channels_, 1.0f, "weight");
    beta_ = layer_norm_param(b, channels_, 0.0f, "bias");
    scale_ = s_out;
    zero_point_ = (u8_t)zp_out;
    qparams_overridden_ = true;
    install();
  }
  Tensor<float> forward_f32(Tensor<float>& x) {
    layer_norm_rows(x, channels_);
    if (!gamma_dev_) {
      gamma_dev_ = upload_f32(gamma_);
      beta_dev_ = upload_f32(beta_);
    }
    Tensor<float> out = layer_norm_f32(x, gamma_dev_, beta_dev_, channels_, eps_);
    maybe_sample(out);
    return out;
  }
  Tensor<u8_t> forward_u8(Tensor<u8_t>& x) {
    layer_norm_rows(x, channels_);
    if (!is_quantized_) throw std::runtime_error("i8ie: LayerNorm is not converted (call convert() first)");
    return layer_norm_u8(x, g_dev_, b_dev_, channels_, eps_, scale_, zero_point_);
  }
  py::array_t<float> weight() const { return py::array_t<float>((ssize_t)gamma_.size(), gamma_.data()); }
  py::array_t<float> bias() const { return py::array_t<float>((ssize_t)beta_.size(), beta_.data()); }
  ssize_t channels() const { return channels_; }
  float eps() const { return eps_; }

 protected:
  void output_qparams_changed() override {
    if (is_quantized_) install();
  }

 private:
  void params_changed() {
    gamma_dev_.reset();
    beta_dev_.reset();
    if (is_quantized_) install();
  }
  void install() {
    if (!(scale_ > 0) || !std::isfinite(scale_)) throw std::runtime_error("i8ie: LayerNorm: the output scale must be positive and finite");
    std::tie(g_dev_, b_dev_) = layer_norm_affine(gamma_, beta_, scale_, zero_point_);
    set_quantized();
  }
  ssize_t channels_;
  float eps_;
  std::vector<float> gamma_, beta_;
  std::shared_ptr<Storage> gamma_dev_, beta_dev_;  // FP32 path
  std::shared_ptr<Storage> g_dev_, b_dev_;         // after convert()
};
template <typename L>
void bind_weightless_state(py::class_<L>& c) {
  c.def("prepare", &L::prepare)
      .def("convert", &L::convert, py::arg("per_channel") = false)
      .def("set_output_qparams", &L::set_output_qparams, py::arg("scale"), py::arg("zero_point"))
      .def("output_qparams", &L::output_qparams)
      .def("load_quantized", &L::load_quantized, py::arg("out_scale"), py::arg("out_zero_point"))
      .def("is_quantized", &L::is_quantized);
}
template <typename L>
void bind_weightless_common(py::class_<L>& c) {
  c.def(py::init<>());
  bind_weightless_state(c);
}

template <typename L>
void bind_layer_common(py::class_<L>& c) {
  c.def("load_weight", &L::load_weight)
      .def("load_bias", &L::load_bias)
      .def("prepare", &L::prepare)
      .def("convert", &L::convert, py::arg("per_channel") = false)
      .def("__call__", [](L& l, Tensor<float>& x) { return l.forward_f32(x); })
      .def("__call__", [](L& l, Tensor<u8_t>& x) { return std::get<0>(l.forward_u8(x, false)); })
      .def("forward_debug", [](L& l, Tensor<u8_t>& x) { return l.forward_u8(x, true); })
      .def("set_output_qparams", &L::set_output_qparams, py::arg("scale"), py::arg("zero_point"))
      .def("output_qparams", &L::output_qparams)
      .def("load_quantized", &L::load_quantized, py::arg("q_weight"), py::arg("q_bias"), py::arg("weight_scale"),
           py::arg("out_scale"), py::arg("out_zero_point"))
      .def("q_weight", &L::q_weight)
      .def("q_bias", &L::q_bias)
      .def("weight_scale", &L::weight_scale)
      .def("weight_scales", &L::weight_scales)
      .def("is_per_channel", &L::is_per_channel)
      .def("is_quantized", &L::is_quantized);
}

}  // namespace

PYBIND11_MODULE(_CXX_i8ie, m) {
  m.doc() = "i8ie extension module: MI355X (gfx950) HIP backend behind include/i8ie_hip.h";

  // the reference registers Tensor<T> under typeid(...).name() (src/pybind11.cc:12)
  bind_tensor<float>(m, "6TensorIfE");
  bind_tensor<u8_t>(m, "6TensorIhE");
  bind_tensor<s8_t>(m, "6TensorIcE");
  py::class_<Tensor<int32_t>>(m, "6TensorIiE").def("numpy", &Tensor<int32_t>::numpy);

  m.def("tensor", &tensor_from_numpy);  // src/pybind11.cc:38-40
  m.def("tensor_from_device", &tensor_from_device);
  // additive (the reference can only default-construct its s8 tensors from Python): an s8 tensor from an ndarray,
  // so that the s8 overloads of relu / max_pool2d can be exercised
  m.def("tensor_s8", [](py::array_t<s8_t, py::array::c_style | py::array::forcecast> a, float scale, int zp) {
    Tensor<s8_t> t(std::vector<ssize_t>(a.shape(), a.shape() + a.ndim()));
    t.scale = scale;
    t.zero_point = (u8_t)zp;
    if (t.size > 0) {
      py::gil_scoped_release nogil;
      check(i8ie_memcpy_h2d(ctx(), t.dptr(), a.data(), (size_t)t.size));
    }
    return t;
  }, py::arg("array"), py::arg("scale") = 1.0f, py::arg("zero_point") = 0);
  m.def("quantize", &quantize);         // src/pybind11.cc:41-45
  m.def("dequantize", &dequantize);     // src/pybind11.cc:46-48
  m.def("relu", &relu_f32);             // src/functional.cc:73-75
  m.def("relu", &relu_u8);
  m.def("max_pool2d", &max_pool2d_f32);  // src/functional.cc:68-72
  m.def("max_pool2d", &max_pool2d_u8);
  m.def("relu", &relu_s8);               // src/functional.cc:81
  m.def("max_pool2d", &max_pool2d_s8);
  // additive (the reference joins no two tensors): a + b in FP32; the quantized Add of include/i8ie_hip.h on u8 tensors
  m.def("add", &add_f32, py::arg("a"), py::arg("b"));
  m.def("add", &add_u8, py::arg("a"), py::arg("b"), py::arg("scale"), py::arg("zero_point"));
  // additive: a * b in FP32; the quantized Mul of include/i8ie_hip.h on u8 tensors.  b has a's shape or is a's gate
  m.def("mul", &mul_f32, py::arg("a"), py::arg("b"));
  m.def("mul", &mul_u8, py::arg("a"), py::arg("b"), py::arg("scale"), py::arg("zero_point"));
  // additive: the batched matmul of two activation tensors and the softmax over the last axis (include/i8ie_hip.h,
  // i8ie_bmm_u8 / i8ie_softmax_u8); a u8 softmax result always carries scale 1/256, zero point 0
  m.def("matmul", &matmul_f32, py::arg("a"), py::arg("b"), py::arg("transpose_a") = false, py::arg("transpose_b") = false);
  m.def("matmul", &matmul_u8, py::arg("a"), py::arg("b"), py::arg("scale"), py::arg("zero_point"), py::arg("transpose_a") = false,
        py::arg("transpose_b") = false);
  m.def("softmax", &softmax_f32, py::arg("x"));
  m.def("softmax", &softmax_u8, py::arg("x"));
  // additive: fused multi-head attention (include/i8ie_hip.h, i8ie_attention_u8); k and v None: q is a packed qkv tensor
  m.def("attention", [](Tensor<float>& q, Tensor<float>* k, Tensor<float>* v, ssize_t heads) { return attention_f32(q, k, v, heads, nullptr); },
        py::arg("q"), py::arg("k").none(true), py::arg("v").none(true), py::arg("heads"));
  m.def("attention", &attention_u8, py::arg("q"), py::arg("k").none(true), py::arg("v").none(true), py::arg("heads"),
        py::arg("score_scale"), py::arg("score_zero_point"), py::arg("scale"), py::arg("zero_point"));
  // additive: LayerNorm over the channel axis of [n, c, h, w] or the last axis of [m, f] / [b, t, f] (include/i8ie_hip.h,
  // i8ie_layernorm_u8); weight / bias: float32 [channels] or None (ones / zeros); uploaded per call
  m.def("layer_norm", [](Tensor<float>& x, const py::object& w, const py::object& b, float eps) {
    const ssize_t c = layer_norm_axis(x);
    return layer_norm_f32(x, upload_f32(layer_norm_param(w, c, 1.0f, "weight")), upload_f32(layer_norm_param(b, c, 0.0f, "bias")), c, eps);
  }, py::arg("x"), py::arg("weight"), py::arg("bias"), py::arg("eps"));
  m.def("layer_norm", [](Tensor<u8_t>& x, const py::object& w, const py::object& b, float eps, float scale, int zp) {
    check_out_qparams("layer_norm", scale, zp);
    const ssize_t c = layer_norm_axis(x);
    if (c > 16384) throw std::runtime_error("i8ie: layer_norm: rows of more than 16384 values");
    auto gb = layer_norm_affine(layer_norm_param(w, c, 1.0f, "weight"), layer_norm_param(b, c, 0.0f, "bias"), scale, zp);
    return layer_norm_u8(x, gb.first, gb.second, c, eps, scale, zp);
  }, py::arg("x"), py::arg("weight"), py::arg("bias"), py::arg("eps"), py::arg("scale"), py::arg("zero_point"));
  // additive: cat along axis 1 of up to 8 tensors, a copy in FP32; the quantized concat of include/i8ie_hip.h on u8 tensors
  m.def("cat", [](const py::list& tensors) { return cat_f32(cat_list<float>(tensors)); }, py::arg("tensors"));
  m.def("cat", [](const py::list& tensors, float scale, int zp) { return cat_u8(cat_list<u8_t>(tensors), scale, zp); },
        py::arg("tensors"), py::arg("scale"), py::arg("zero_point"));
  // additive: the table-driven activations of include/i8ie_hip.h (kind: I8IE_ACT_*), f in FP32, one table lookup on u8
  // tensors; lut applies a caller's own 256-entry table
  m.def("activation", &activation_f32, py::arg("x"), py::arg("kind"), py::arg("param"));
  m.def("activation", &activation_u8, py::arg("x"), py::arg("kind"), py::arg("param"), py::arg("scale"), py::arg("zero_point"));
  m.def("lut", [](Tensor<u8_t>& x, const py::array_t<uint8_t, py::array::c_style>& table, float scale, int zp) {
    return lut_u8(x, lut_from_array(table), scale, zp);
  }, py::arg("x"), py::arg("table"), py::arg("scale"), py::arg("zero_point"));
  m.def("activation_table", [](int kind, float param, float s_in, int zp_in, float s_out, int zp_out) {
    check_zero_point(zp_in);
    check_zero_point(zp_out);
    py::array_t<uint8_t> out(256);
    check(i8ie_activation_table(kind, param, s_in, (uint8_t)zp_in, s_out, (uint8_t)zp_out, out.mutable_data()));
    return out;
  }, py::arg("kind"), py::arg("param"), py::arg("s_in"), py::arg("zp_in"), py::arg("s_out"), py::arg("zp_out"));
  // additive (the reference has no average pool): round-to-nearest integer mean on u8 tensors, fp32 sum / n on FP32 ones
  m.def("avg_pool2d", [](Tensor<float>& x, ssize_t k, ssize_t s) { return avg_pool_f32(x, k, s, false); }, py::arg("x"),
        py::arg("kernel_size"), py::arg("stride"));
  m.def("avg_pool2d", [](Tensor<u8_t>& x, ssize_t k, ssize_t s) { return avg_pool_u8(x, k, s, false); }, py::arg("x"),
        py::arg("kernel_size"), py::arg("stride"));
  m.def("global_avg_pool2d", [](Tensor<float>& x) { return avg_pool_f32(x, 0, 1, true); }, py::arg("x"));
  m.def("global_avg_pool2d", [](Tensor<u8_t>& x) { return avg_pool_u8(x, 0, 1, true); }, py::arg("x"));
  // additive (the reference has no resize op): nearest / bilinear upsampling by integer factors (mode: I8IE_UPSAMPLE_*), exact
  // integers on u8 tensors, the fp32 sequence of include/i8ie_hip.h on FP32 ones
  m.def("upsample", &upsample_f32, py::arg("x"), py::arg("factor_h"), py::arg("factor_w"), py::arg("mode"));
  m.def("upsample", &upsample_u8, py::arg("x"), py::arg("factor_h"), py::arg("factor_w"), py::arg("mode"));

  {
    py::class_<Linear> c(m, "Linear");  // src/fully_connected.cc:54-72
    c.def(py::init<py::array_t<float, py::array::c_style | py::array::forcecast>,
                   py::array_t<float, py::array::c_style | py::array::forcecast>>())
        .def(py::init([](Tensor<float>& w, Tensor<float>& b) { return new Linear(w.numpy(), b.numpy()); }))
        .def(py::init<ssize_t, ssize_t>());
    bind_layer_common(c);
  }
  {
    py::class_<Conv2d> c(m, "Conv2d");  // src/conv2d.cc:144-165
    c.def(py::init<py::array_t<float, py::array::c_style | py::array::forcecast>,
                   py::array_t<float, py::array::c_style | py::array::forcecast>>())
        .def(py::init([](Tensor<float>& w, Tensor<float>& b) { return new Conv2d(w.numpy(), b.numpy()); }))
        .def(py::init<ssize_t, ssize_t, ssize_t, ssize_t, ssize_t, ssize_t, ssize_t>(), py::arg("in_channels"),
             py::arg("out_channels"), py::arg("kernel_size"), py::arg("stride") = 1, py::arg("padding") = 0,
             py::arg("groups") = 1, py::arg("dilation") = 1)
        .def("groups", &Conv2d::groups)
        .def("dilation", &Conv2d::dilation);
    bind_layer_common(c);
  }

  {
    py::class_<ConvTranspose2d> c(m, "ConvTranspose2d");
    c.def(py::init<ssize_t, ssize_t, ssize_t, ssize_t, ssize_t, ssize_t>(), py::arg("in_channels"), py::arg("out_channels"),
          py::arg("kernel_size"), py::arg("stride") = 1, py::arg("padding") = 0, py::arg("output_padding") = 0);
    bind_layer_common(c);
  }

  {
    py::class_<Add> c(m, "Add");
    bind_weightless_common(c);
    c.def("__call__", &Add::forward_f32).def("__call__", &Add::forward_u8);
  }
  {
    py::class_<Mul> c(m, "Mul");
    bind_weightless_common(c);
    c.def("__call__", &Mul::forward_f32).def("__call__", &Mul::forward_u8);
  }
  {
    py::class_<MatMul> c(m, "MatMul");
    c.def(py::init<bool, bool>(), py::arg("transpose_a") = false, py::arg("transpose_b") = false);
    bind_weightless_state(c);
    c.def("__call__", &MatMul::forward_f32).def("__call__", &MatMul::forward_u8)
        .def("transpose_a", &MatMul::transpose_a).def("transpose_b", &MatMul::transpose_b);
  }
  {
    py::class_<Attention> c(m, "Attention");
    c.def(py::init<ssize_t>(), py::arg("heads"))
        .def("prepare", &Attention::prepare)
        .def("convert", &Attention::convert, py::arg("per_channel") = false)
        .def("set_output_qparams", &Attention::set_output_qparams, py::arg("scale"), py::arg("zero_point"))
        .def("output_qparams", &Attention::output_qparams)
        .def("set_score_qparams", &Attention::set_score_qparams, py::arg("scale"), py::arg("zero_point"))
        .def("score_qparams", &Attention::score_qparams)
        .def("load_quantized", &Attention::load_quantized, py::arg("out_scale"), py::arg("out_zero_point"), py::arg("score_scale"),
             py::arg("score_zero_point"))
        .def("is_quantized", &Attention::is_quantized)
        .def("heads", &Attention::heads)
        .def("__call__", &Attention::forward_f32).def("__call__", &Attention::forward_f32_packed)
        .def("__call__", &Attention::forward_u8).def("__call__", &Attention::forward_u8_packed);
  }
  {
    py::class_<Concat> c(m, "Concat");
    bind_weightless_common(c);
    c.def("__call__", &Concat::forward, py::arg("tensors"));
  }
  {
    py::class_<Activation> c(m, "Activation");
    c.def(py::init<int, float>(), py::arg("kind"), py::arg("param") = 0.0f);
    bind_weightless_state(c);
    c.def("__call__", &Activation::forward_f32).def("__call__", &Activation::forward_u8).def("kind", &Activation::kind).def("param", &Activation::param);
  }

  {
    py::class_<LayerNorm> c(m, "LayerNorm");
    c.def(py::init<ssize_t, float>(), py::arg("channels"), py::arg("eps") = 1e-5f)
        .def("load_weight", &LayerNorm::load_weight)
        .def("load_bias", &LayerNorm::load_bias)
        .def("prepare", &LayerNorm::prepare)
        .def("convert", &LayerNorm::convert, py::arg("per_channel") = false)
        .def("__call__", &LayerNorm::forward_f32)
        .def("__call__", &LayerNorm::forward_u8)
        .def("set_output_qparams", &LayerNorm::set_output_qparams, py::arg("scale"), py::arg("zero_point"))
        .def("output_qparams", &LayerNorm::output_qparams)
        .def("load_quantized", &LayerNorm::load_quantized, py::arg("weight"), py::arg("bias"), py::arg("out_scale"),
             py::arg("out_zero_point"))
        .def("weight", &LayerNorm::weight)
        .def("bias", &LayerNorm::bias)
        .def("channels", &LayerNorm::channels)
        .def("eps", &LayerNorm::eps)
        .def("is_quantized", &LayerNorm::is_quantized);
  }

  // ---- additive runtime controls -------------------------------------------------
  m.def("abi_version", []() { return i8ie_version(); });
  m.def("device_count", []() {
    int n = 0;
    check(i8ie_device_count(&n));
    return n;
  });
  m.def("set_device", [](int d) {
    if (rt().ctx && rt().device != d) throw std::runtime_error("i8ie: set_device after the context was created");
    rt().device = d;
  });
  m.def("device", []() {
    (void)ctx();
    return rt().device;
  });
  m.def("synchronize", []() {
    py::gil_scoped_release nogil;
    check(i8ie_sync(ctx()));
  });
  m.def("stream", []() { return (uintptr_t)i8ie_ctx_stream(ctx()); });
  m.def("memory_stats", []() {
    size_t live = 0, cached = 0, allocs = 0;
    check(i8ie_memory_stats(ctx(), &live, &cached, &allocs));
    return py::make_tuple(live, cached, allocs);
  });
  m.def("pinned_empty", &pinned_empty);
  m.def("trim", []() {
    for (auto& kv : border_cache())
      for (void* p : kv.second) i8ie_free(ctx(), p);
    border_cache().clear();
    for (auto& kv : upload_cache())
      for (UploadSlot& u : kv.second) {
        check(i8ie_stream_wait_event(ctx(), u.free_ev, 0));  // order the reuse behind the recorded reader
        event_put(u.free_ev);
        i8ie_free(ctx(), u.dev);
      }
    upload_cache().clear();
    for (auto& kv : ppool().free_blocks)
      for (void* p : kv.second) i8ie_host_free(ctx(), p);
    ppool().free_blocks.clear();
    check(i8ie_trim(ctx()));
  });
  m.def("force_fallback", [](bool on) { check(i8ie_ctx_set_option(ctx(), I8IE_OPT_FORCE_FALLBACK, on ? 1 : 0)); });
  m.def("profile_start",
        [](bool mfma_only, int stride) {
          check(i8ie_ctx_set_option(ctx(), I8IE_OPT_PROFILE_STRIDE, stride));
          check(i8ie_profile_start(ctx(), mfma_only ? 1 : 0));
        },
        py::arg("mfma_only") = false, py::arg("stride") = 1);
  m.def("profile_stop", []() {
    std::vector<i8ie_profile_entry> e(64);
    int n = 0;
    {
      py::gil_scoped_release nogil;
      check(i8ie_profile_stop(ctx(), e.data(), (int)e.size(), &n));
    }
    py::dict out;
    for (int i = 0; i < n && i < (int)e.size(); ++i)
      out[py::str(e[i].name)] = py::make_tuple(e[i].launches, e[i].total_ms, e[i].total_ops, e[i].total_bytes);
    return out;
  });
  // run on a borrowed hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); call before the first op
  m.def("use_stream", [](uintptr_t stream, int device) {
    if (rt().ctx) throw std::runtime_error("i8ie: use_stream after the context was created");
    rt().device = device;
    check(i8ie_ctx_create_on_stream(device, (void*)stream, &rt().ctx));
  });
  m.def("set_calibration_seed", [](long seed) { rt().calib_seed = seed; });
  // where Calibrator::sample runs: "auto" (seeded: host replay of the reference's mt19937 stream; unseeded: on the
  // device), "host", "device" (seeded or not: counter-based draws, reproducible for a given seed)
  m.def("set_calibration_mode", [](const std::string& mode) {
    if (mode == "auto") rt().calib_mode = 0;
    else if (mode == "host") rt().calib_mode = 1;
    else if (mode == "device") rt().calib_mode = 2;
    else throw std::invalid_argument("set_calibration_mode: auto | host | device");
  });
  m.def("calibration_mode", []() { return std::string(rt().calib_mode == 0 ? "auto" : rt().calib_mode == 1 ? "host" : "device"); });
  // the device sampler on its own: feed chunks (device tensors), then the 1000 slots and get_range()
  m.def("calibrator_device_samples", [](std::vector<py::array_t<float, py::array::c_style | py::array::forcecast>> chunks, long seed) {
    const long keep_seed = rt().calib_seed;
    rt().calib_seed = seed;
    Calibrator cal;
    try {
      for (auto& c : chunks) {
        float* d = nullptr;
        check(i8ie_malloc(ctx(), (size_t)c.size() * 4 + 4, (void**)&d));
        check(i8ie_memcpy_h2d(ctx(), d, c.data(), (size_t)c.size() * 4));
        cal.sample_device(d, (ssize_t)c.size());
        check(i8ie_sync(ctx()));
        i8ie_free(ctx(), d);
      }
    } catch (...) {
      rt().calib_seed = keep_seed;
      throw;
    }
    rt().calib_seed = keep_seed;
    py::array_t<float> slots(kNumSamples);
    check(i8ie_memcpy_d2h(ctx(), slots.mutable_data(), cal.samples_dev, kNumSamples * sizeof(float)));
    float s;
    u8_t z;
    std::tie(s, z) = cal.get_range(1);
    return py::make_tuple(slots, (long)cal.cnt, s, (int)z);
  });
  // the layers' calibrator on its own (host code, no GPU): feed chunks through sample(), then get_range()
  m.def("calibrator_range",
        [](std::vector<py::array_t<float, py::array::c_style | py::array::forcecast>> chunks, float quantile) {
          Calibrator cal;
          for (auto& c : chunks) cal.sample(c.data(), c.size());
          auto [scale, zp] = cal.get_range(quantile);
          return py::make_tuple(scale, (int)zp);
        });
  // ---- whole-forward replay as one HIP graph (include/i8ie_hip.h, i8ie_graph_*) ----------------------------
  struct Graph {
    i8ie_graph* g = nullptr;
    ~Graph() { if (g) i8ie_graph_destroy(g); }
  };
  py::class_<Graph, std::shared_ptr<Graph>>(m, "Graph")
      .def("launch", [](Graph& gr) { check(i8ie_graph_launch(gr.g)); })
      .def("nodes", [](Graph& gr) {
        int k = 0, n = 0;
        check(i8ie_graph_nodes(gr.g, &k, &n));
        return py::make_tuple(k, n);
      });
  m.def("graph_begin", []() { check(i8ie_graph_begin(ctx())); });
  m.def("graph_end", []() {
    auto gr = std::make_shared<Graph>();
    check(i8ie_graph_end(ctx(), &gr->g));
    return gr;
  });
  // overwrite a resident FP32 tensor's device buffer (the input a captured graph reads) from host memory
  m.def("upload_into", [](Tensor<float>& t, py::array_t<float, py::array::c_style | py::array::forcecast> a) {
    if ((size_t)a.size() != (size_t)t.size) throw std::invalid_argument("upload_into: size mismatch");
    check(i8ie_memcpy_h2d(ctx(), t.dptr(), a.data(), (size_t)t.size * 4));
    if (t.st) {  // a host mirror of the old values (small tensors made from an ndarray) is stale now
      t.st->host_valid = false;
      std::vector<unsigned char>().swap(t.st->host);
    }
  });

  // raw device copy into / out of foreign HIP memory (e.g. a torch tensor's data_ptr) for the
  // multi-GPU logits gather; both sides must be used on this module's stream or synchronised.
  m.def("copy_to_ptr", [](Tensor<float>& t, uintptr_t dst) {
    check(i8ie_memcpy_d2d(ctx(), (void*)dst, t.dptr(), (size_t)t.size * 4));
  });
  m.def("copy_to_ptr", [](Tensor<u8_t>& t, uintptr_t dst) {
    check(i8ie_memcpy_d2d(ctx(), (void*)dst, t.dptr(), (size_t)t.size));
  });
}
