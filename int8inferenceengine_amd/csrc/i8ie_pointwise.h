// i8ie_pointwise.h -- host helpers the pointwise units share (i8ie_elementwise, i8ie_add, i8ie_mul, i8ie_concat, i8ie_lut,
// i8ie_avgpool): the launch constants and grid rule, the alignment test, i8ie_requant.h's "ordinary scale" rule, the
// three-scale argument check of the two-operand ops and the geometry of a bordered NHWC buffer.  Everything here has internal
// linkage (an unnamed namespace per including unit): no call crosses a translation unit through this header.
// i8ie_gconv.hip and i8ie_deconv.hip include it for aligned_to alone.
#pragma once

#include <cmath>
#include <cstdint>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;

// blocks of kThreads for `work_items` grid-stride items: at least one, at most kMaxBlocks
inline int grid_for(int64_t work_items) {
  int64_t b = (work_items + kThreads - 1) / kThreads;
  if (b < 1) b = 1;
  return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}
inline bool aligned_to(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// a scale the guarded estimate may be used with (i8ie_requant.h's rule): not zero, denormal or huge
inline bool ordinary(float s) { return s > 1e-30f && s < 1e30f; }

// the argument check of a two-operand op (add, mul)
inline bool scales_ok(float s_a, float s_b, float s_out) {
  return std::isfinite(s_a) && std::isfinite(s_b) && std::isfinite(s_out) && s_out > 0.0f;
}

// A bordered NHWC buffer [n][h + 2b][w + 2b][c], each buffer of a launch with its own b.
struct NhwcGeom {
  int64_t img;  // bytes per image: (h + 2b) * (w + 2b) * c
  int64_t row;  // bytes per physical row: (w + 2b) * c
  int64_t org;  // offset of interior pixel (0, 0): b * row + b * c
};
inline NhwcGeom buf_geom(int c, int h, int w, int border) {
  NhwcGeom g;
  g.row = (int64_t)(w + 2 * border) * c;
  g.img = (int64_t)(h + 2 * border) * g.row;
  g.org = (int64_t)border * g.row + (int64_t)border * c;
  return g;
}

}  // namespace
