// calibrator.cc -- sampling a layer's FP32 result, and the calibration controls of the module.
#include "calibrator.h"

namespace i8ie_py {

void calib_sample(Calibrator& cal, Tensor<float>& out) {
  if (Calibrator::on_device()) {  // no copy of the layer output to the host
    cal.sample_device(out.dptr(), out.size);
    return;
  }
  py::array_t<float> a = out.numpy();
  cal.sample(a.data(), out.size);
}

void bind_calibration(py::module_& m) {
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
  m.def("calibrator_device_samples", [](std::vector<F32Array> chunks, long seed) {
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
  m.def("calibrator_range", [](std::vector<F32Array> chunks, float quantile) {
    Calibrator cal;
    for (auto& c : chunks) cal.sample(c.data(), c.size());
    auto [scale, zp] = cal.get_range(quantile);
    return py::make_tuple(scale, (int)zp);
  });
}

}  // namespace i8ie_py
