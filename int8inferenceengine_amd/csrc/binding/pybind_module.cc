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
//
// The binding is split by concern ("The binding's layout"): runtime, tensor, operands, ops, calibrator, layers.
// This file registers them and holds the runtime controls.
#include "layers.h"

using namespace i8ie_py;

PYBIND11_MODULE(_CXX_i8ie, m) {
  m.doc() = "i8ie extension module: MI355X (gfx950) HIP backend behind include/i8ie_hip.h";

  bind_tensors(m);
  bind_ops(m);
  bind_rearrange(m);
  bind_resize(m);
  bind_pad(m);
  bind_posembed(m);
  bind_layers(m);
  bind_calibration(m);

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
  m.def("upload_into", [](Tensor<float>& t, F32Array a) {
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
