// i8ie_pointwise.h -- helpers the pointwise units share (i8ie_elementwise, i8ie_binary, i8ie_concat, i8ie_lut, i8ie_avgpool).
// Host: the launch constants and grid rule, the alignment test and the item width it allows, the pixel walk of the kernels that keep per-channel values in registers, i8ie_requant.h's "ordinary scale"
// rule, the three-scale argument check of the two-operand ops and the geometry of a bordered NHWC buffer.  Device: the walk of
// a bordered NHWC buffer by row items.  Everything here has internal linkage (an unnamed namespace per including unit): no
// call crosses a translation unit through this header.  i8ie_gconv.hip and i8ie_deconv.hip include it for aligned_to alone.
#pragma once

#include <cmath>
#include <cstdint>
#include <initializer_list>

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
// items of 16 / 4 / 1 bytes: the widest that divides every one of `sizes` (the run of bytes an item must not straddle, and
// whatever else must stay item-aligned) and to which every one of `bufs` is aligned
inline int item_width(std::initializer_list<int64_t> sizes, std::initializer_list<const void*> bufs) {
  for (int v = 16; v > 1; v >>= 2) {
    bool ok = true;
    for (int64_t s : sizes) ok = ok && s % v == 0;
    for (const void* p : bufs) ok = ok && aligned_to(p, (unsigned)v);
    if (ok) return v;
  }
  return 1;
}

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

// The pixel walk of the kernels that keep per-channel values in registers (Mul's gate form, i8ie_binary.hip; the BatchNorm,
// i8ie_batchnorm.hip).  An item is VEC bytes of one pixel's channels.  A block holds `rows` whole pixels of `lanes_c` items each
// (rows * lanes_c <= kThreads; consecutive lanes take consecutive channel items of one pixel, then the next pixel, so a wave's
// accesses are contiguous), and every lane walks `walk` pixels of one image, `rows` pixels apart: its channel item never changes.
// Blocks stride over (image, channel chunk, pixel tile) units up to kMaxBlocks.  a: the buffer read, o: the buffer written.
struct PixelWalk {
  int64_t units;           // n * chunks * tiles
  int cpv;                 // items per pixel: c / VEC
  int lanes_c, rows;       // a block's shape: lanes_c = min(cpv, 256) items by rows = 256 / lanes_c pixels
  int chunks, tiles;       // channel chunks of lanes_c items per pixel; tiles of rows * walk pixels per image
  int hw, w, c;
  int step_x;              // rows % w: how far a lane's column moves per step (its row moves by rows / w, +1 where the column wraps)
  int64_t a_step, a_wrap;  // ... and its byte offset in a: rows / w physical rows + step_x pixels; the extra 2 * border pixels of a wrap
  int64_t o_step, o_wrap;
};
inline void pixel_walk_init(PixelWalk& t, int vec, int walk, int n, int c, int h, int w, const NhwcGeom& ga, const NhwcGeom& go) {
  t.cpv = c / vec;
  t.lanes_c = t.cpv < kThreads ? t.cpv : kThreads;
  t.rows = kThreads / t.lanes_c;
  t.chunks = (t.cpv + t.lanes_c - 1) / t.lanes_c;
  t.hw = h * w;
  t.w = w;
  t.c = c;
  t.tiles = (t.hw + t.rows * walk - 1) / (t.rows * walk);
  t.units = (int64_t)n * t.chunks * t.tiles;
  const int step_y = t.rows / w;
  t.step_x = t.rows % w;
  t.a_step = step_y * ga.row + (int64_t)t.step_x * c;
  t.a_wrap = ga.row - (int64_t)w * c;
  t.o_step = step_y * go.row + (int64_t)t.step_x * c;
  t.o_wrap = go.row - (int64_t)w * c;
}
inline int pixel_walk_blocks(const PixelWalk& t) { return (int)(t.units > kMaxBlocks ? kMaxBlocks : t.units); }

#if defined(__HIPCC__)
// The interior of a bordered NHWC buffer walked by row items.  The w * c interior bytes of an image row are the contiguous
// unit; an item is VEC bytes of one row (c % VEC == 0 and VEC-aligned buffers: every row start is then VEC-aligned in every
// buffer, whatever its border).  A launch covers items = n * h * per_row of them, per_row = w * c / VEC; Idx is uint32_t while
// items fits, int64_t beyond.
template <typename Idx>
struct RowItem {
  Idx img;
  int64_t y, col;  // interior row, byte column in it
};
template <int VEC, typename Idx>
__device__ __forceinline__ RowItem<Idx> row_item(Idx v, Idx per_row, Idx h) {
  const Idx r = v / per_row;
  const int64_t col = (int64_t)(v - r * per_row) * VEC;
  const Idx img = r / h;
  return {img, (int64_t)(r - img * h), col};
}
template <typename Idx>
__device__ __forceinline__ int64_t nhwc_at(const NhwcGeom& g, const RowItem<Idx>& it) {
  return (int64_t)it.img * g.img + g.org + it.y * g.row + it.col;
}
#endif

}  // namespace
