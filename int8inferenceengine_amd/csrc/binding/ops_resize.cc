// ops_resize.cc -- interpolate to any size and adaptive_avg_pool2d (no counterpart in the reference; the arithmetic:
// include/i8ie_hip.h, i8ie_resize2d_u8 / i8ie_adaptive_avgpool2d_u8) and bind_resize.  The entries are private to the i8ie
// package (tests/golden/binding_surface.json stays as it is): i8ie.interpolate / i8ie.adaptive_avg_pool2d come here only where
// the geometry is not one that upsample, avg_pool2d or global_avg_pool2d already express.
#include "ops.h"

namespace i8ie_py {

namespace {

// mode: I8IE_RESIZE_* for the resize, -1 for the adaptive pool
struct Resize {
  int mode;
  int n, c, h, w, oh, ow;
  std::vector<ssize_t> oshp;
};
// the checked arguments of one call and the result's shape: a RuntimeError that names the op, before any device call
template <typename T>
Resize resize_args(const Tensor<T>& in, const char* name, ssize_t oh, ssize_t ow, int mode) {
  const std::string what = std::string("i8ie: ") + name;
  if (in.shape.size() != 4) throw std::runtime_error(what + " expects an NCHW tensor");
  for (ssize_t d : in.shape)
    if (d <= 0 || d > 0x7FFFFFFF) throw std::runtime_error(what + ": empty tensor");
  if (oh < 1 || ow < 1 || oh > 0x7FFFFFFF || ow > 0x7FFFFFFF) throw std::runtime_error(what + ": the output size must be at least 1 x 1");
  if (mode >= 0) {
    if (mode != I8IE_RESIZE_NEAREST && mode != I8IE_RESIZE_BILINEAR && mode != I8IE_RESIZE_BILINEAR_ALIGNED)
      throw std::runtime_error(what + ": unknown mode");
    const int64_t dy = mode == I8IE_RESIZE_BILINEAR ? 2 * (int64_t)oh : (oh > 1 ? oh - 1 : 1);
    const int64_t dx = mode == I8IE_RESIZE_BILINEAR ? 2 * (int64_t)ow : (ow > 1 ? ow - 1 : 1);
    if (mode != I8IE_RESIZE_NEAREST && dy * dx > (int64_t)1 << 22)
      throw std::runtime_error(what + ": the output is too large for the exact blend (den_y * den_x above 2^22)");
  } else {
    auto longest = [](int64_t L, int64_t O) {  // the longest window [floor(i L / O), ceil((i + 1) L / O)) of an axis
      int64_t m = 0;
      for (int64_t i = 0; i < O; ++i) m = std::max(m, ((i + 1) * L + O - 1) / O - (i * L) / O);
      return m;
    };
    if (longest(in.shape[2], oh) * longest(in.shape[3], ow) > 65536) throw std::runtime_error(what + ": window of more than 65536 elements");
  }
  return Resize{mode, (int)in.shape[0], (int)in.shape[1], (int)in.shape[2], (int)in.shape[3], (int)oh, (int)ow,
                {in.shape[0], in.shape[1], oh, ow}};
}
Tensor<float> resize_f32(Tensor<float>& in, const Resize& g) {
  Tensor<float> out(g.oshp);
  if (g.mode >= 0) check(i8ie_resize2d_f32(ctx(), in.dptr(), out.dptr(), g.n, g.c, g.h, g.w, g.oh, g.ow, g.mode));
  else check(i8ie_adaptive_avgpool2d_f32(ctx(), in.dptr(), out.dptr(), g.n, g.c, g.h, g.w, g.oh, g.ow));
  return out;
}
Tensor<u8_t> resize_u8(Tensor<u8_t>& in, const Resize& g) {
  need_contents(in);
  const u8_t zp = in.zero_point;
  // deferred like upsample's result: relu(op(..)) is one launch, and a consuming conv gets its zero-point border and, where it
  // reads them, re-biased bytes straight from the kernel
  return deferred_one_input(  // (as the pools: the input's qparams)
      in, g.oshp, in.scale, zp, [g, zp](std::shared_ptr<Storage> si, bool relu, int border, bool s8) {
        // (a view whose storage is NHWC under other logical dims goes back to the reference's order: the view is defined on it)
        if (si->layout == I8IE_LAYOUT_NHWC && (si->dn != g.n || si->dc != g.c || si->dh != g.h || si->dw != g.w)) si->to_nchw();
        std::shared_ptr<Storage> st;
        if (si->layout == I8IE_LAYOUT_NHWC) {
          st = nhwc_storage(g.oshp, border, zp, s8);
          const uint8_t* ip = (const uint8_t*)si->device_ptr();
          if (g.mode >= 0)
            check(i8ie_resize2d_u8_nhwc(ctx(), ip, si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0, g.n, g.c, g.h,
                                        g.w, g.oh, g.ow, g.mode, relu ? 1 : 0, zp));
          else
            check(i8ie_adaptive_avgpool2d_u8_nhwc(ctx(), ip, si->border, si->s8 ? 1 : 0, (uint8_t*)st->dev, st->border, st->s8 ? 1 : 0, g.n,
                                                  g.c, g.h, g.w, g.oh, g.ow, relu ? 1 : 0, zp));
        } else {  // an NCHW operand (a user-made tensor)
          st = device_storage((size_t)g.n * g.c * g.oh * g.ow);
          const uint8_t* ip = (const uint8_t*)si->device_ptr();
          if (g.mode >= 0) check(i8ie_resize2d_u8(ctx(), ip, (uint8_t*)st->dev, g.n, g.c, g.h, g.w, g.oh, g.ow, g.mode));
          else check(i8ie_adaptive_avgpool2d_u8(ctx(), ip, (uint8_t*)st->dev, g.n, g.c, g.h, g.w, g.oh, g.ow));
          if (relu) check(i8ie_relu_u8(ctx(), (const uint8_t*)st->dev, (uint8_t*)st->dev, (int64_t)st->bytes, zp));
        }
        return st;
      });
}
[[noreturn]] void refuse_s8(const char* name) {
  throw std::runtime_error(std::string("i8ie: ") + name + ": int8 (s8) tensors are not supported (uint8 and FP32 tensors are)");
}

}  // namespace

void bind_resize(py::module_& m) {
  m.def("_interpolate", [](Tensor<float>& x, ssize_t oh, ssize_t ow, int mode) {
    if (mode < 0) throw std::runtime_error("i8ie: interpolate: unknown mode");
    return resize_f32(x, resize_args(x, "interpolate", oh, ow, mode));
  }, py::arg("x"), py::arg("out_h"), py::arg("out_w"), py::arg("mode"));
  m.def("_interpolate", [](Tensor<u8_t>& x, ssize_t oh, ssize_t ow, int mode) {
    if (mode < 0) throw std::runtime_error("i8ie: interpolate: unknown mode");
    return resize_u8(x, resize_args(x, "interpolate", oh, ow, mode));
  }, py::arg("x"), py::arg("out_h"), py::arg("out_w"), py::arg("mode"));
  m.def("_interpolate", [](Tensor<s8_t>&, ssize_t, ssize_t, int) -> Tensor<s8_t> { refuse_s8("interpolate"); }, py::arg("x"),
        py::arg("out_h"), py::arg("out_w"), py::arg("mode"));
  m.def("_adaptive_avg_pool2d", [](Tensor<float>& x, ssize_t oh, ssize_t ow) {
    return resize_f32(x, resize_args(x, "adaptive_avg_pool2d", oh, ow, -1));
  }, py::arg("x"), py::arg("out_h"), py::arg("out_w"));
  m.def("_adaptive_avg_pool2d", [](Tensor<u8_t>& x, ssize_t oh, ssize_t ow) {
    return resize_u8(x, resize_args(x, "adaptive_avg_pool2d", oh, ow, -1));
  }, py::arg("x"), py::arg("out_h"), py::arg("out_w"));
  m.def("_adaptive_avg_pool2d", [](Tensor<s8_t>&, ssize_t, ssize_t) -> Tensor<s8_t> { refuse_s8("adaptive_avg_pool2d"); }, py::arg("x"),
        py::arg("out_h"), py::arg("out_w"));
}

}  // namespace i8ie_py
