// runtime.cc -- the one instance of each piece of runtime state (function-local statics, never destroyed) and the allocators over them.
#include "runtime.h"

namespace i8ie_py {

Runtime& rt() {
  static Runtime* r = new Runtime();  // intentionally leaked: outlives every tensor at exit
  return *r;
}
int default_device() {
  if (const char* e = std::getenv("I8IE_DEVICE")) return std::atoi(e);
  if (const char* e = std::getenv("LOCAL_RANK")) return std::atoi(e);  // one process per GPU
  return 0;
}
std::map<BorderKey, std::vector<void*>>& border_cache() {
  static auto* m = new std::map<BorderKey, std::vector<void*>>();
  return *m;
}
PinnedPool& ppool() {
  static auto* p = new PinnedPool();
  return *p;
}
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
std::map<size_t, std::vector<UploadSlot>>& upload_cache() {
  static auto* m = new std::map<size_t, std::vector<UploadSlot>>();
  return *m;
}
std::shared_ptr<Storage> device_storage(size_t bytes) {
  auto s = std::make_shared<Storage>();
  s->bytes = bytes;
  check(i8ie_malloc(ctx(), bytes, &s->dev));
  return s;
}

std::shared_ptr<Storage> nhwc_storage(const std::vector<ssize_t>& shp, int b, int zp, bool s8) {
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
std::shared_ptr<Storage> upload_f32(const std::vector<float>& v) {
  auto s = device_storage(v.size() * sizeof(float));
  check(i8ie_memcpy_h2d(ctx(), s->dev, v.data(), v.size() * sizeof(float)));
  return s;
}

}  // namespace i8ie_py
