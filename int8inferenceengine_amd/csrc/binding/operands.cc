// operands.cc -- see operands.h
#include "operands.h"

namespace i8ie_py {

void check_zero_point(int zp) {
  if (zp < 0 || zp > 255) throw std::runtime_error("i8ie: zero point must be in [0, 255]");
}
void check_out_qparams(const char* op, float scale, int zp) {
  check_zero_point(zp);
  if (!(scale > 0) || !std::isfinite(scale)) throw std::runtime_error(std::string("i8ie: ") + op + ": the output scale must be positive and finite");
}
std::shared_ptr<Storage> operand_as_it_lies(Tensor<u8_t>& t) {
  if (t.pend) {
    if (auto st = t.pend->find_any(t.pend_relu)) t.adopt(st);
    else t.realize();
  }
  if (!t.st) throw std::runtime_error("i8ie: empty tensor");
  t.st->device_ptr();  // (uploads a host-made tensor, waits for an asynchronous upload)
  return t.st;
}
bool waits_for(const Tensor<u8_t>& t, const Tensor<u8_t>& reader) {
  return t.pend && reader.pend && reader.pend != t.pend && reader.pend->made.empty() && reader.pend->reads(t.pend.get());
}
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

}  // namespace i8ie_py
