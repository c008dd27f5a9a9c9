// runtime.h -- the device runtime under the binding: the context, pinned staging memory and events, the caches of bordered
// and upload blocks, and Storage, the buffer tensors share.  Each piece of state is a function-local static of runtime.cc.
#pragma once
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

namespace i8ie_py {

// ---------------------------------------------------------------- runtime ----
struct Runtime {
  i8ie_ctx* ctx = nullptr;
  int device = -1;
  long calib_seed = -1;  // < 0: std::random_device, as the reference (src/calibrator.cc:9-10)
  int calib_mode = 0;    // 0 auto: seeded -> the reference's mt19937 stream replayed on the host (golden-pinned),
                         // unseeded -> sampled on the device (no D2H of the layer outputs); 1 host; 2 device
  // the observer a prepare() gives its calibrator, and how a histogram becomes a range at convert() (include/i8ie_hip.h,
  // "Histogram calibration"); calib_mode above belongs to the reservoir alone
  bool calib_histogram = false;           // false: the reference's 1000-slot reservoir
  int calib_method = I8IE_CALIB_MINMAX;   // I8IE_CALIB_*, read at convert()
  double calib_param = 99.99;             // the percentile of I8IE_CALIB_PERCENTILE
};
Runtime& rt();  // one instance, intentionally leaked: outlives every tensor at exit
inline void check(int rc) {
  if (rc != I8IE_OK) throw std::runtime_error(std::string("i8ie: ") + i8ie_last_error());
}
int default_device();
inline i8ie_ctx* ctx() {
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
std::map<BorderKey, std::vector<void*>>& border_cache();

// ---- pinned host staging, events and upload blocks (asynchronous transfers) ----
struct PinnedPool {
  std::map<size_t, std::vector<void*>> free_blocks;  // by capacity (multiples of 4 KiB)
  std::vector<i8ie_event*> events;
  size_t user_blocks = 0;  // live pinned_empty() arrays
};
PinnedPool& ppool();
inline size_t pinned_capacity(size_t bytes) { return (bytes + 4095) & ~(size_t)4095; }
void* pinned_take(size_t cap);
void pinned_put(void* p, size_t cap);
i8ie_event* event_take();
void event_put(i8ie_event* e);
// Device blocks written by the transfer stream.  They bypass the stream-ordered allocator (whose reuse
// rule only covers the compute stream): a block comes back with an event recorded behind its last
// compute-stream reader, and the next upload into it makes the transfer stream wait for that event.
struct UploadSlot {
  void* dev;
  i8ie_event* free_ev;
};
std::map<size_t, std::vector<UploadSlot>>& upload_cache();

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

std::shared_ptr<Storage> device_storage(size_t bytes);
// NHWC u8 storage for logical shape `shp` (NCHW order) with a border of b pixels holding zp (s8: the bytes of this
// tensor are stored re-biased, I8IE_LAYOUT_NHWC_S8, so its border holds zp ^ 0x80)
std::shared_ptr<Storage> nhwc_storage(const std::vector<ssize_t>& shp, int b, int zp, bool s8 = false);
std::shared_ptr<Storage> upload_f32(const std::vector<float>& v);

}  // namespace i8ie_py
