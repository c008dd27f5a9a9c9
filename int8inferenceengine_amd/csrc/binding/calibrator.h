// calibrator.h -- the calibrator and the prepare / convert state machine around a layer's output (scale, zero_point).
#pragma once
#include "operands.h"

namespace i8ie_py {

// src/calibrator.cc:6-37, include/calibrator.h:4-14
constexpr ssize_t kNumSamples = 1000;
struct Calibrator {
  std::array<float, kNumSamples> samples{};  // value-initialised (make_unique<Calibrator>(), src/layer.cc:33)
  ssize_t cnt = 0;
  // device-side sampling (i8ie_calib_sample_f32): the 1000 slots live on the GPU until get_range()
  float* samples_dev = nullptr;
  int* scratch_dev = nullptr;
  int64_t seen = 0;
  uint64_t dev_seed = 0;
  // the histogram observer (i8ie_calib_hist_*): every value is seen on the device, the state is read back once, at get_range()
  const bool histogram = false;
  void* hist_dev = nullptr;
  Calibrator() = default;
  explicit Calibrator(bool histogram_observer) : histogram(histogram_observer) {}
  Calibrator(const Calibrator&) = delete;
  Calibrator& operator=(const Calibrator&) = delete;
  ~Calibrator() {
    if (samples_dev) i8ie_free(rt().ctx, samples_dev);
    if (scratch_dev) i8ie_free(rt().ctx, scratch_dev);
    if (hist_dev) i8ie_free(rt().ctx, hist_dev);
  }
  static bool on_device() { return rt().calib_mode == 2 || (rt().calib_mode == 0 && rt().calib_seed < 0); }
  void sample_device(const float* dptr, ssize_t n) {
    if (!samples_dev) {
      check(i8ie_malloc(rt().ctx, kNumSamples * sizeof(float), (void**)&samples_dev));
      check(i8ie_malloc(rt().ctx, kNumSamples * sizeof(int), (void**)&scratch_dev));
      check(i8ie_memset(rt().ctx, samples_dev, 0, kNumSamples * sizeof(float)));
      if (rt().calib_seed >= 0) {
        dev_seed = (uint64_t)rt().calib_seed;
      } else {
        std::random_device rd;
        dev_seed = ((uint64_t)rd() << 32) | rd();
      }
    }
    check(i8ie_calib_sample_f32(rt().ctx, dptr, (int64_t)n, seen, dev_seed, samples_dev, scratch_dev));
    seen += n;
    cnt = seen < kNumSamples ? (ssize_t)seen : kNumSamples;
  }
  void observe(const float* dptr, ssize_t n) {  // asynchronous: nothing here waits for the device
    if (!hist_dev) {
      check(i8ie_malloc(ctx(), i8ie_calib_hist_state_bytes(), &hist_dev));
      check(i8ie_calib_hist_reset(ctx(), hist_dev));
    }
    check(i8ie_calib_hist_observe_f32(ctx(), dptr, (int64_t)n, hist_dev));
    seen += n;
    cnt = seen < kNumSamples ? (ssize_t)seen : kNumSamples;
  }
  // the state as it stands (an observer that has seen nothing: the reset state, without a device call)
  void read_histogram(i8ie_calib_hist_header& h, std::vector<uint64_t>& counts) {
    counts.assign(I8IE_CALIB_HIST_BINS, 0);
    if (hist_dev) {
      check(i8ie_calib_hist_read(ctx(), hist_dev, &h, counts.data()));
      return;
    }
    h = i8ie_calib_hist_header{};
    h.min = INFINITY;
    h.max = -INFINITY;
    h.exponent = -100;
  }
  // (scale, zero_point, lo, hi) of the histogram under one range method
  std::tuple<float, u8_t, float, float> histogram_range(int method, double param) {
    i8ie_calib_hist_header h;
    std::vector<uint64_t> counts;
    read_histogram(h, counts);
    float lo, hi, scale;
    u8_t zp;
    check(i8ie_calib_hist_range(&h, counts.data(), method, param, &lo, &hi));
    i8ie_calib_range_qparams(lo, hi, &scale, &zp);
    return std::make_tuple(scale, zp, lo, hi);
  }
  void sample(const float* data, ssize_t n) {
    std::mt19937 rng;
    if (rt().calib_seed >= 0) {
      rng.seed((unsigned)rt().calib_seed);
    } else {
      std::random_device rd;
      rng.seed(rd());
    }
    std::uniform_int_distribution<ssize_t> dist(0, kNumSamples * 2);  // about half get sampled
    for (ssize_t i = 0; i < n; ++i) {
      if (cnt < kNumSamples) {
        samples[cnt++] = data[i];
      } else {
        ssize_t idx = dist(rng);
        if (idx < kNumSamples) samples[idx] = data[i];
      }
    }
  }
  std::tuple<float, u8_t> get_range(float quantile) {
    if (histogram) {  // the method in force now, at convert()
      auto [s, z, lo, hi] = histogram_range(rt().calib_method, rt().calib_param);
      (void)lo, (void)hi;
      return std::make_tuple(s, z);
    }
    if (samples_dev) check(i8ie_memcpy_d2h(rt().ctx, samples.data(), samples_dev, kNumSamples * sizeof(float)));
    std::sort(samples.begin(), samples.end());
    float out_min = samples[(size_t)((1.0 - quantile) * cnt)];
    float out_max = samples[(size_t)(quantile * (cnt - 1))];
    float scale;
    u8_t zp;
    i8ie_calib_range_qparams(out_min, out_max, &scale, &zp);
    return std::make_tuple(scale, zp);
  }
};

// what a preparing layer (or Add) does with its FP32 result: src/conv2d.cc:94-96, src/fully_connected.cc:17-19
void calib_sample(Calibrator& cal, Tensor<float>& out);

// "minmax" | "percentile" | "mse" -> I8IE_CALIB_* (std::invalid_argument otherwise, and for a percentile outside (50, 100])
int calib_method_code(const std::string& method, double param);
// what _calib_histogram / _calib_range (and Attention's two for its scores) return; RuntimeError unless `cal` is the histogram
// observer of a layer that is preparing
py::dict histogram_dict(Calibrator* cal, bool preparing);
py::tuple histogram_range_tuple(Calibrator* cal, bool preparing, const std::string& method, double param);

// The prepare / convert state machine of src/layer.cc:28-54 around a layer's output (scale, zero_point): what the layers with
// weights and those without share.
class QuantState {
 public:
  QuantState() = default;
  QuantState(const QuantState&) = delete;
  QuantState& operator=(const QuantState&) = delete;
  void prepare() {  // src/layer.cc:28-35
    if (is_quantized_) {
      std::cerr << "already quantized" << std::endl;
      return;
    }
    cal_ = std::make_unique<Calibrator>(rt().calib_histogram);
    is_preparing_ = true;
  }
  // the live histogram of a layer that is preparing with a histogram observer, and a range from it without converting
  py::dict calib_histogram() { return histogram_dict(cal_.get(), is_preparing_); }
  py::tuple calib_range(const std::string& method, double param) { return histogram_range_tuple(cal_.get(), is_preparing_, method, param); }
  void set_output_qparams(float s, int zp) {  // additive: inject what calibration would produce
    check_zero_point(zp);
    scale_ = s;
    zero_point_ = (u8_t)zp;
    qparams_overridden_ = true;
    output_qparams_changed();
  }
  std::tuple<float, int> output_qparams() const { return std::make_tuple(scale_, (int)zero_point_); }
  bool is_quantized() const { return is_quantized_; }
  bool is_preparing() const { return is_preparing_; }

 protected:
  ~QuantState() = default;
  virtual void output_qparams_changed() {}  // (a layer with a live handle pushes them into it)
  // the calibration half of convert() (src/layer.cc:36-47): false when the layer is quantized already
  bool convert_qparams() {
    if (is_quantized_) {
      std::cerr << "already quantized" << std::endl;
      return false;
    }
    if (!is_preparing_) {
      if (!qparams_overridden_) std::cerr << "No prepared, use default config" << std::endl;
    } else {
      float s;
      u8_t z;
      std::tie(s, z) = cal_->get_range(1);
      if (!qparams_overridden_) {
        scale_ = s;
        zero_point_ = z;
      }
      cal_.reset();
    }
    return true;
  }
  void set_quantized() {
    cal_.reset();
    is_preparing_ = false;
    is_quantized_ = true;
  }
  void maybe_sample(Tensor<float>& out) {  // src/conv2d.cc:94-96, src/fully_connected.cc:17-19
    if (is_preparing_) calib_sample(*cal_, out);
  }

  std::unique_ptr<Calibrator> cal_;
  bool is_preparing_ = false;
  bool is_quantized_ = false;
  bool qparams_overridden_ = false;
  float scale_ = 1;       // include/layer.h:46
  u8_t zero_point_ = 0;   // include/layer.h:47
};
// the state machine's methods as every layer class exposes them (load_quantized differs per class and stays with it)
template <typename C>
void bind_quant_state(C& c) {
  using L = typename C::type;
  c.def("prepare", &L::prepare)
      .def("convert", &L::convert, py::arg("per_channel") = false)
      .def("set_output_qparams", &L::set_output_qparams, py::arg("scale"), py::arg("zero_point"))
      .def("output_qparams", &L::output_qparams)
      .def("is_quantized", &L::is_quantized)
      .def("_calib_histogram", &L::calib_histogram)
      .def("_calib_range", &L::calib_range, py::arg("method"), py::arg("param") = 99.99);
}

void bind_calibration(py::module_& m);  // set_calibration_seed ... calibrator_range, _set_calibration ... _calib_hist_range

}  // namespace i8ie_py
