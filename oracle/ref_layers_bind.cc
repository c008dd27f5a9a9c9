// ref_layers_bind.cc -- our own pybind11 module (_i8ie_ref_layers) around the reference's LAYER code:
//     src/layer.cc            (quantize_weight, BaseLayer::convert)
//     src/conv2d.cc           (Conv2d::forward_prop, both overloads; im2col, transpose)
//     src/fully_connected.cc  (Linear::forward_prop, both overloads)
// together with src/quantize_utils.cc, src/functional.cc and src/calibrator.cc, which they call.  All of them
// are compiled WHERE THEY LIE by oracle/Makefile (target `ref_layers`) into oracle/_ref/ (git-ignored); nothing
// of the reference is copied into this repository.  include/layer.h includes mkl.h: oracle/mkl_stub/mkl.h
// stands in for it (declarations only), and the two CBLAS entry points the layers call are defined by
// oracle/gemm_provider.c, which is linked in instead of libmkl_rt and is itself held to committed MKL results.
//
// The module has a name of its own so that it can never be taken for the product's _CXX_i8ie; its classes are
// module-local so that it can live beside _i8ie_ref_partial in one process.
//
// TEST INFRASTRUCTURE ONLY: used by tests/golden/make_golden_layers.py to produce the fixtures
// tests/golden/ref_{quantize_weight,conv2d_u8,linear_u8,layers_f32,networks}.npz and ref_alexnet_digests.json,
// and by the one live test of tests/test_ref_layers_golden.py.
#include <omp.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "pybind11/numpy.h"
#include "pybind11/pybind11.h"
#include "pybind11/stl.h"
#include "conv2d.h"           // reference header (include/conv2d.h)
#include "fully_connected.h"  // reference header (include/fully_connected.h)
#include "quantize_utils.h"   // reference header (include/quantize_utils.h)
#include "tensor.h"           // reference header (include/tensor.h)

namespace py = pybind11;

void declare_tensor_funcs(py::module&);  // reference src/functional.cc:78
// reference src/layer.cc:6-26 (a free function no header declares)
void quantize_weight(Tensor<s8_t>& q_weight, Tensor<s8_t>& q_bias, Tensor<float>& weight, Tensor<float>& bias);

extern "C" {
typedef void (*gp_hook_fn)(int m, int n, int k, const int32_t* c, int ldc, const int32_t* oc, const void* a);
void gp_set_hook(gp_hook_fn fn);  // oracle/gemm_provider.c
}
#include "mkl.h"  // oracle/mkl_stub/mkl.h (already seen through layer.h)

namespace {

using f32_array = py::array_t<float, py::array::c_style | py::array::forcecast>;

inline std::vector<ssize_t> shape_of(const py::array& a) {
  return std::vector<ssize_t>(a.shape(), a.shape() + a.ndim());
}

template <typename T>
py::array_t<T> copy_out(Tensor<T>& t) {
  py::array_t<T> a(t.shape());
  std::memcpy(a.mutable_data(), t.data(), sizeof(T) * (size_t)t.size());
  return a;
}

template <typename T>
void bind_tensor(py::module& m, const char* name) {
  py::class_<Tensor<T>>(m, name, py::module_local())
      .def("numpy", [](Tensor<T>& t) { return py::array(t.shape(), t.data(), t.cap()); })
      .def("scale", [](Tensor<T>& t) { return (float)t.scale(); })
      .def("zero_point", [](Tensor<T>& t) { return (int)t.zero_point(); })
      // reference include/tensor.h:106-133 (Tensor::reshape, the call of i8ie/tensor.py)
      .def("reshape", [](Tensor<T>& t, std::vector<ssize_t> shape) -> Tensor<T>&& {
        return std::move(t.reshape(shape));
      });
}

// scale_ / zero_point_ are protected and the reference sets them only through its unseeded calibrator; a
// derived struct may name them, so a case can fix its output qparams.
template <typename L>
struct Open : L {
  using L::L;
  using BaseLayer::q_bias_;
  using BaseLayer::q_weight_;
  using BaseLayer::scale_;
  using BaseLayer::zero_point_;
};

template <typename L, typename C>
void bind_layer_common(C& cls) {
  cls.def("load_weight", [](Open<L>& l, py::array_t<float> w) { l.load_weight(w); })
      .def("load_bias", [](Open<L>& l, py::array_t<float> b) { l.load_bias(b); })
      .def("convert", [](Open<L>& l) { l.convert(); })  // src/layer.cc:36-54 (never prepared: default qparams)
      .def("set_output_qparams",
           [](Open<L>& l, float scale, int zp) {
             l.scale_ = scale;
             l.zero_point_ = (u8_t)zp;
           })
      .def("forward_f32", [](Open<L>& l, Tensor<float>& x) -> Tensor<float>&& {
        return std::move(l.forward_prop(std::move(x)));
      })
      .def("forward_u8", [](Open<L>& l, Tensor<u8_t>& x) -> Tensor<u8_t>&& {
        return std::move(l.forward_prop(std::move(x)));
      })
      .def("q_weight", [](Open<L>& l) { return copy_out(*l.q_weight_).template cast<py::array>(); })
      .def("q_bias", [](Open<L>& l) { return copy_out(*l.q_bias_).template cast<py::array>(); })
      .def("weight_scale", [](Open<L>& l) { return py::make_tuple(l.q_weight_->scale(), l.q_bias_->scale()); });
}

// ---- recorder behind the provider's hook: C and oc of every integer GEMM call ------------------------------
struct Rec {
  int tid, m, n, k;
  long seq;
  std::vector<int32_t> c, oc;
};
std::mutex g_mu;
std::vector<Rec> g_recs;
long g_seq = 0;

void on_gemm(int m, int n, int k, const int32_t* c, int ldc, const int32_t* oc, const void*) {
  Rec r;
  r.tid = omp_get_thread_num();
  r.m = m, r.n = n, r.k = k;
  r.c.resize((size_t)m * n);
  for (int i = 0; i < m; ++i) std::memcpy(&r.c[(size_t)i * n], c + (size_t)i * ldc, sizeof(int32_t) * (size_t)n);
  r.oc.assign(oc, oc + n);
  std::lock_guard<std::mutex> lock(g_mu);
  r.seq = g_seq++;
  g_recs.push_back(std::move(r));
}

}  // namespace

PYBIND11_MODULE(_i8ie_ref_layers, m) {
  m.doc() = "reference layer.cc + conv2d.cc + fully_connected.cc (+ quantize_utils, functional), compiled in place";
  bind_tensor<float>(m, "RefTensorF32");
  bind_tensor<u8_t>(m, "RefTensorU8");
  bind_tensor<s8_t>(m, "RefTensorS8");

  m.def("f32", [](f32_array a) { return new Tensor<float>(a); }, py::return_value_policy::take_ownership);
  m.def("u8", [](py::array_t<u8_t, py::array::c_style | py::array::forcecast> a, float scale, int zp) {
    auto* t = new Tensor<u8_t>(shape_of(a));
    std::memcpy(t->data(), a.data(), (size_t)a.size());
    t->scale() = scale;
    t->zero_point() = (u8_t)zp;
    return t;
  }, py::return_value_policy::take_ownership);

  // reference src/quantize_utils.cc:44-58
  m.def("quantize", [](Tensor<float>& in, float scale, int zp) -> Tensor<u8_t>&& {
    return std::move(quantize(in, scale, (u8_t)zp));
  });
  m.def("dequantize", [](Tensor<u8_t>& in) -> Tensor<float>&& { return std::move(dequantize(in)); });
  // reference src/functional.cc:66-82: relu(T), max_pool2d(T, kernel_size, strides)
  declare_tensor_funcs(m);

  // reference src/layer.cc:6-26, called directly: (q_w, q_b, scale of q_w, scale of q_b)
  m.def("quantize_weight", [](f32_array w, f32_array b) {
    Tensor<float> tw(w), tb(b);
    Tensor<s8_t> qw(shape_of(w)), qb(shape_of(b));
    quantize_weight(qw, qb, tw, tb);
    return py::make_tuple(copy_out(qw).cast<py::array>(), copy_out(qb).cast<py::array>(), (float)qw.scale(),
                          (float)qb.scale());
  });

  py::class_<Open<Conv2d>> conv(m, "Conv2d", py::module_local());
  conv.def(py::init<ssize_t, ssize_t, ssize_t, ssize_t, ssize_t>(), py::arg("in_channels"),
           py::arg("out_channels"), py::arg("kernel_size"), py::arg("stride") = 1, py::arg("padding") = 0);
  bind_layer_common<Conv2d>(conv);
  py::class_<Open<Linear>> lin(m, "Linear", py::module_local());
  lin.def(py::init<ssize_t, ssize_t>());
  bind_layer_common<Linear>(lin);

  // every cblas_gemm_s8u8s32 call between record_begin() and record_end(): (thread, sequence, C [m, n], oc [n]).
  // Conv2d issues one call per image from an OpenMP loop, so the caller orders them (or runs one thread).
  m.def("record_begin", [] {
    std::lock_guard<std::mutex> lock(g_mu);
    g_recs.clear();
    g_seq = 0;
    gp_set_hook(on_gemm);
  });
  m.def("record_end", [] {
    gp_set_hook(nullptr);
    std::lock_guard<std::mutex> lock(g_mu);
    py::list out;
    for (auto& r : g_recs) {
      py::array_t<int32_t> c({(ssize_t)r.m, (ssize_t)r.n});
      std::memcpy(c.mutable_data(), r.c.data(), sizeof(int32_t) * r.c.size());
      py::array_t<int32_t> oc((ssize_t)r.n);
      std::memcpy(oc.mutable_data(), r.oc.data(), sizeof(int32_t) * r.oc.size());
      out.append(py::make_tuple(r.tid, r.seq, c, oc, r.k));
    }
    g_recs.clear();
    return out;
  });
  // the provider as it is linked into THIS module, with the reference's argument pattern: the generator holds it
  // to the committed MKL results before it generates anything
  m.def("gemm_s8u8s32", [](py::array_t<u8_t, py::array::c_style | py::array::forcecast> a,
                           py::array_t<int8_t, py::array::c_style | py::array::forcecast> b,
                           py::array_t<int32_t, py::array::c_style | py::array::forcecast> oc) {
    const int M = (int)a.shape(0), K = (int)a.shape(1), N = (int)b.shape(0);
    py::array_t<int32_t> c({(ssize_t)M, (ssize_t)N});
    cblas_gemm_s8u8s32(CblasRowMajor, CblasNoTrans, CblasTrans, CblasRowOffset, M, N, K, 1, a.data(), K, 0, b.data(), K,
                       0, 0, c.mutable_data(), N, oc.data());
    return c;
  });
  m.def("set_num_threads", [](int n) { omp_set_num_threads(n); });
  m.def("compiler", [] { return std::string("g++ " __VERSION__); });
}
