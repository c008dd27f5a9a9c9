// ops_pad.cc -- pad (constant, reflect, replicate, circular; negative amounts crop) on the last two axes (no counterpart in the
// reference; the index rule: include/i8ie_hip.h, "Spatial padding") and bind_pad.  The entry is private to the i8ie package
// (tests/golden/binding_surface.json stays as it is; tests/golden/binding_surface_pad.json records it): i8ie.pad / i8ie.crop
// come here with checked integers.
#include <cmath>

#include "ops.h"

namespace i8ie_py {

namespace {

struct Pad {
  int mode, left, right, top, bottom;
  int n, c, h, w, oh, ow;
  std::vector<ssize_t> oshp;
};
// the checked arguments of one call and the result's shape: a RuntimeError that names the op, before any device call
template <typename T>
Pad pad_args(const Tensor<T>& in, ssize_t left, ssize_t right, ssize_t top, ssize_t bottom, int mode) {
  if (in.shape.size() != 4) throw std::runtime_error("i8ie: pad expects an NCHW tensor");
  for (ssize_t d : in.shape)
    if (d <= 0 || d > 0x7FFFFFFF) throw std::runtime_error("i8ie: pad: empty tensor");
  for (ssize_t a : {left, right, top, bottom})
    if (a < -65535 || a > 65535) throw std::runtime_error("i8ie: pad: an amount beyond +-65535");
  Pad g{mode, (int)left, (int)right, (int)top, (int)bottom, (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3], 0, 0, {}};
  int d[4];
  if (i8ie_pad_output_shape(mode, g.left, g.right, g.top, g.bottom, g.n, g.c, g.h, g.w, d) != I8IE_OK)
    throw std::runtime_error(std::string("i8ie: ") + i8ie_last_error());
  g.oh = d[2]; g.ow = d[3];
  g.oshp = {d[0], d[1], d[2], d[3]};
  return g;
}
// the byte quantize gives `value` at (scale, zp): (u8)(value / scale + zp), fp32 divide, add, truncate, low 8 bits (no clamp;
// include/i8ie_hip.h, i8ie_quantize_f32_u8).  The device's float -> int conversion saturates and turns NaN into 0; so does this.
u8_t fill_byte(float value, float scale, u8_t zp) {
  const volatile float q = value / scale;  // (two roundings: no contraction, whatever the host compiler's flags)
  const float t = q + (float)zp;
  int32_t i;
  if (std::isnan(t)) i = 0;
  else if (t >= 2147483648.0f) i = 0x7FFFFFFF;
  else if (t <= -2147483648.0f) i = (int32_t)0x80000000u;
  else i = (int32_t)t;
  return (u8_t)((uint32_t)i & 0xFFu);
}
Tensor<float> pad_f32(Tensor<float>& in, const Pad& g, float value) {
  Tensor<float> out(g.oshp);
  check(i8ie_pad2d_f32(ctx(), in.dptr(), out.dptr(), g.n, g.c, g.h, g.w, g.mode, g.left, g.right, g.top, g.bottom, value));
  return out;
}
Tensor<u8_t> pad_u8(Tensor<u8_t>& in, const Pad& g, float value) {
  need_contents(in);
  const u8_t zp = in.zero_point;
  const u8_t fill = g.mode == I8IE_PAD_CONSTANT ? fill_byte(value, in.scale, zp) : zp;
  // deferred like the rearrangements' results: relu(pad(..)) is one launch, and a consuming conv gets its zero-point border and,
  // where it reads them, re-biased bytes straight from the kernel; a result that nobody consumes launches nothing
  return deferred_one_input(  // (as the pools: the input's qparams)
      in, g.oshp, in.scale, zp, [g, zp, fill](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        // (a view whose storage is NHWC under other logical dims goes back to the reference's order: the view is defined on it)
        if (si->layout == I8IE_LAYOUT_NHWC && (si->dn != g.n || si->dc != g.c || si->dh != g.h || si->dw != g.w)) si->to_nchw();
        std::shared_ptr<Storage> st;
        if (si->layout == I8IE_LAYOUT_NHWC) {
          st = nhwc_storage(g.oshp, border, zp, s8);
          check(i8ie_pad2d_u8_nhwc(ctx(), (const uint8_t*)si->device_ptr(), si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border,
                                   st->s8 ? 1 : 0, g.n, g.c, g.h, g.w, g.mode, g.left, g.right, g.top, g.bottom, fill, relu ? 1 : 0, zp));
        } else {  // an NCHW operand (a user-made tensor, or a producer that hands over NCHW): the flat entry, in place
          st = device_storage((size_t)g.n * g.c * g.oh * g.ow);
          check(i8ie_pad2d_u8(ctx(), (const uint8_t*)si->device_ptr(), (uint8_t*)st->dev, g.n, g.c, g.h, g.w, g.mode, g.left, g.right, g.top,
                              g.bottom, fill));
          if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        }
        return st;
      });
}

}  // namespace

void bind_pad(py::module_& m) {
  // f32 first, then u8, then the s8 overload that refuses
  m.def("_pad", [](Tensor<float>& x, ssize_t left, ssize_t right, ssize_t top, ssize_t bottom, int mode, float value) {
    return pad_f32(x, pad_args(x, left, right, top, bottom, mode), value);
  }, py::arg("x"), py::arg("left"), py::arg("right"), py::arg("top"), py::arg("bottom"), py::arg("mode"), py::arg("value"));
  m.def("_pad", [](Tensor<u8_t>& x, ssize_t left, ssize_t right, ssize_t top, ssize_t bottom, int mode, float value) {
    return pad_u8(x, pad_args(x, left, right, top, bottom, mode), value);
  }, py::arg("x"), py::arg("left"), py::arg("right"), py::arg("top"), py::arg("bottom"), py::arg("mode"), py::arg("value"));
  m.def("_pad", [](Tensor<s8_t>&, ssize_t, ssize_t, ssize_t, ssize_t, int, float) -> Tensor<s8_t> {
    throw std::runtime_error("i8ie: pad: int8 (s8) tensors are not supported (uint8 and FP32 tensors are)");
  }, py::arg("x"), py::arg("left"), py::arg("right"), py::arg("top"), py::arg("bottom"), py::arg("mode"), py::arg("value"));
}

}  // namespace i8ie_py
