// calibrator.cc -- sampling a layer's FP32 result, and the calibration controls of the module.
#include "calibrator.h"

namespace i8ie_py {

int calib_method_code(const std::string& method, double param) {
  if (!(param > 50.0 && param <= 100.0)) throw std::invalid_argument("calibration: the percentile must lie in (50, 100]");
  if (method == "minmax") return I8IE_CALIB_MINMAX;
  if (method == "percentile") return I8IE_CALIB_PERCENTILE;
  if (method == "mse") return I8IE_CALIB_MSE;
  throw std::invalid_argument("calibration: the range method is minmax | percentile | mse");
}
static const char* calib_method_name(int code) { return code == I8IE_CALIB_MINMAX ? "minmax" : code == I8IE_CALIB_PERCENTILE ? "percentile" : "mse"; }
static void need_histogram(Calibrator* cal, bool preparing) {
  if (!preparing || !cal) throw std::runtime_error("i8ie: the layer is not preparing: there is no calibration histogram");
  if (!cal->histogram) throw std::runtime_error("i8ie: the layer prepared under the reservoir (set_calibration before prepare())");
}
py::dict histogram_dict(Calibrator* cal, bool preparing) {
  need_histogram(cal, preparing);
  i8ie_calib_hist_header h;
  std::vector<uint64_t> counts;
  cal->read_histogram(h, counts);
  py::array_t<uint64_t> a((ssize_t)counts.size());
  std::memcpy(a.mutable_data(), counts.data(), counts.size() * sizeof(uint64_t));
  py::dict d;
  d["exponent"] = (int)h.exponent;
  d["counts"] = a;
  d["min"] = h.min;
  d["max"] = h.max;
  d["nonfinite"] = (uint64_t)h.nonfinite;
  return d;
}
py::tuple histogram_range_tuple(Calibrator* cal, bool preparing, const std::string& method, double param) {
  const int code = calib_method_code(method, param);
  need_histogram(cal, preparing);
  auto [s, z, lo, hi] = cal->histogram_range(code, param);
  return py::make_tuple(s, (int)z, lo, hi);
}

void calib_sample(Calibrator& cal, Tensor<float>& out) {
  if (cal.histogram) {  // whatever set_calibration_mode says: that mode belongs to the reservoir
    cal.observe(out.dptr(), out.size);
    return;
  }
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
  // the observer prepare() hands out from now on and the range method convert() uses: "reservoir" (the reference's), or a
  // histogram observer read as "minmax" | "percentile" (param: the percentile) | "mse" (include/i8ie_hip.h)
  m.def("_set_calibration", [](const std::string& method, double param) {
    if (method == "reservoir") {
      if (!(param > 50.0 && param <= 100.0)) throw std::invalid_argument("calibration: the percentile must lie in (50, 100]");
      rt().calib_histogram = false;
    } else {
      rt().calib_method = calib_method_code(method, param);
      rt().calib_histogram = true;
    }
    rt().calib_param = param;
  }, py::arg("method"), py::arg("param") = 99.99);
  m.def("_calibration", []() {
    return py::make_tuple(std::string(rt().calib_histogram ? calib_method_name(rt().calib_method) : "reservoir"), rt().calib_param);
  });
  // i8ie_calib_hist_range + i8ie_calib_range_qparams on a histogram given from the host (no GPU): header = (exponent, min,
  // max), hist = uint64[2048]; returns (scale, zero_point, lo, hi)
  m.def("_calib_hist_range", [](std::tuple<int, float, float> header, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> hist,
                                const std::string& method, double param) {
    if (hist.size() != I8IE_CALIB_HIST_BINS) throw std::invalid_argument("_calib_hist_range: hist holds 2048 counters");
    i8ie_calib_hist_header h{};
    h.exponent = std::get<0>(header);
    h.min = std::get<1>(header);
    h.max = std::get<2>(header);
    float lo, hi, scale;
    u8_t zp;
    check(i8ie_calib_hist_range(&h, hist.data(), calib_method_code(method, param), param, &lo, &hi));
    i8ie_calib_range_qparams(lo, hi, &scale, &zp);
    return py::make_tuple(scale, (int)zp, lo, hi);
  }, py::arg("header"), py::arg("hist"), py::arg("method"), py::arg("param") = 99.99);
  // the layers' calibrator on its own (host code, no GPU): feed chunks through sample(), then get_range()
  m.def("calibrator_range", [](std::vector<F32Array> chunks, float quantile) {
    Calibrator cal;
    for (auto& c : chunks) cal.sample(c.data(), c.size());
    auto [scale, zp] = cal.get_range(quantile);
    return py::make_tuple(scale, (int)zp);
  });
}

}  // namespace i8ie_py
