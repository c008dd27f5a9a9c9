// ops_rearrange.cc -- narrow / channel_shuffle / pixel_shuffle / pixel_unshuffle (no counterpart in the reference; the index
// maps: include/i8ie_hip.h, i8ie_rearrange_u8_nhwc) and bind_rearrange.  The entries are private to the i8ie package
// (tests/golden/binding_surface.json stays as it is; tests/golden/binding_surface_rearrange.json records them).
#include "ops.h"

namespace i8ie_py {

namespace {

struct Rearrange {
  int kind, p0, p1;
  std::vector<ssize_t> ishp;  // the operand as [n, c, h, w] ([m, f] rows: h = w = 1)
  std::vector<ssize_t> oshp;  // the result in the operand's rank
  int on, oc, oh, ow;
};
// the checked arguments of one call and the result's shape: a RuntimeError that names the op, before any device call
template <typename T>
Rearrange rearrange_args(const Tensor<T>& in, const char* name, int kind, ssize_t p0, ssize_t p1) {
  const std::string what = std::string("i8ie: ") + name;
  const size_t rank = in.shape.size();
  if (kind == I8IE_REARRANGE_NARROW ? (rank != 2 && rank != 4) : rank != 4)
    throw std::runtime_error(what + (kind == I8IE_REARRANGE_NARROW ? " expects [n, c, h, w] or [m, f]" : " expects an NCHW tensor"));
  for (ssize_t d : in.shape)
    if (d <= 0 || d > 0x7FFFFFFF) throw std::runtime_error(what + ": empty tensor");
  if (p0 < -0x7FFFFFFF || p0 > 0x7FFFFFFF || p1 < -0x7FFFFFFF || p1 > 0x7FFFFFFF) throw std::runtime_error(what + ": argument out of range");
  Rearrange g{kind, (int)p0, (int)p1, {in.shape[0], in.shape[1], rank == 4 ? in.shape[2] : 1, rank == 4 ? in.shape[3] : 1}, {}, 0, 0, 0, 0};
  int d[4];
  if (i8ie_rearrange_output_shape(kind, g.p0, g.p1, (int)g.ishp[0], (int)g.ishp[1], (int)g.ishp[2], (int)g.ishp[3], d) != I8IE_OK)
    throw std::runtime_error(std::string("i8ie: ") + i8ie_last_error());
  g.on = d[0]; g.oc = d[1]; g.oh = d[2]; g.ow = d[3];
  if (rank == 4) g.oshp = {d[0], d[1], d[2], d[3]};
  else g.oshp = {d[0], d[1]};
  return g;
}
Tensor<float> rearrange_f32(Tensor<float>& in, const Rearrange& g) {
  Tensor<float> out(g.oshp);
  check(i8ie_rearrange_f32(ctx(), in.dptr(), out.dptr(), (int)g.ishp[0], (int)g.ishp[1], (int)g.ishp[2], (int)g.ishp[3], g.kind, g.p0, g.p1));
  return out;
}
Tensor<u8_t> rearrange_u8(Tensor<u8_t>& in, const Rearrange& g) {
  need_contents(in);
  const u8_t zp = in.zero_point;
  const bool rank4 = in.shape.size() == 4;
  // deferred like upsample's result: relu(op(..)) is one launch, and a consuming conv gets its zero-point border and, where it
  // reads them, re-biased bytes straight from the kernel; a part of a split that nobody consumes launches nothing
  return deferred_one_input(  // (as the pools: the input's qparams)
      in, g.oshp, in.scale, zp, [g, zp, rank4](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        const int n = (int)g.ishp[0], c = (int)g.ishp[1], h = (int)g.ishp[2], w = (int)g.ishp[3];
        // (a view whose storage is NHWC under other logical dims goes back to the reference's order: the view is defined on it)
        if (si->layout == I8IE_LAYOUT_NHWC && (!rank4 || si->dn != n || si->dc != c || si->dh != h || si->dw != w)) si->to_nchw();
        std::shared_ptr<Storage> st;
        if (si->layout == I8IE_LAYOUT_NHWC) {
          st = nhwc_storage({g.on, g.oc, g.oh, g.ow}, border, zp, s8);
          check(i8ie_rearrange_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                       st->s8 ? 1 : 0, n, c, h, w, g.kind, g.p0, g.p1, relu ? 1 : 0, zp));
        } else {  // an NCHW operand (a user-made tensor) and rows
          st = device_storage((size_t)g.on * g.oc * g.oh * g.ow);
          check(i8ie_rearrange_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, n, c, h, w, g.kind, g.p0, g.p1));
          if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        }
        return st;
      });
}
[[noreturn]] void refuse_s8(const char* name) {
  throw std::runtime_error(std::string("i8ie: ") + name + ": int8 (s8) tensors are not supported (uint8 and FP32 tensors are)");
}

// one private entry: f32 first, then u8, then the s8 overload that refuses
template <typename... P, typename Args>
void def_entry(py::module_& m, const char* entry, const char* name, int kind, Args args) {
  std::apply([&](auto... a) {
    m.def(entry, [name, kind](Tensor<float>& x, P... p) {
      const ssize_t v[4] = {(ssize_t)p..., 0, 0};  // (p1 = 0 where the op has one parameter)
      return rearrange_f32(x, rearrange_args(x, name, kind, v[0], v[1]));
    }, py::arg("x"), a...);
    m.def(entry, [name, kind](Tensor<u8_t>& x, P... p) {
      const ssize_t v[4] = {(ssize_t)p..., 0, 0};  // (p1 = 0 where the op has one parameter)
      return rearrange_u8(x, rearrange_args(x, name, kind, v[0], v[1]));
    }, py::arg("x"), a...);
    m.def(entry, [name](Tensor<s8_t>&, P...) -> Tensor<s8_t> { refuse_s8(name); }, py::arg("x"), a...);
  }, args);
}

}  // namespace

void bind_rearrange(py::module_& m) {
  def_entry<ssize_t, ssize_t>(m, "_narrow", "narrow", I8IE_REARRANGE_NARROW, std::make_tuple(py::arg("start"), py::arg("length")));
  def_entry<ssize_t>(m, "_channel_shuffle", "channel_shuffle", I8IE_REARRANGE_CHANNEL_SHUFFLE, std::make_tuple(py::arg("groups")));
  def_entry<ssize_t>(m, "_pixel_shuffle", "pixel_shuffle", I8IE_REARRANGE_PIXEL_SHUFFLE, std::make_tuple(py::arg("upscale_factor")));
  def_entry<ssize_t>(m, "_pixel_unshuffle", "pixel_unshuffle", I8IE_REARRANGE_PIXEL_UNSHUFFLE, std::make_tuple(py::arg("downscale_factor")));
}

}  // namespace i8ie_py
