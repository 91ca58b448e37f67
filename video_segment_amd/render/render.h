// render.h -- launchers of the two render kernels (render.hip), called by render_capi.cpp.
#ifndef VSG_RENDER_RENDER_H_
#define VSG_RENDER_RENDER_H_

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace vsg_render_impl {

// One scan interval to paint: pixels [left_x, right_x] of row y get `value` (a packed colour
// c0 | c1 << 8 | c2 << 16, or a region id).  The host has checked it against the frame.
struct Interval {
  int32_t y, left_x, right_x;
  uint32_t value;
};
static_assert(sizeof(Interval) == 16, "uploaded as int4");

enum ComposeMode { COMPOSE_RENDER = 0, COMPOSE_BLEND = 1, COMPOSE_CONCAT = 2 };

// Row pitch (in uint32) of the colour plane of a W-wide frame: a multiple of 4 with at least four
// spare columns, so that k_render_compose may load the uint4 of its last column group and that
// group's right neighbour without leaving the row.
inline int PlanePitch(int width) { return (width + 3) / 4 * 4 + 4; }

// plane[y * pitch + x] = value for every pixel of every interval.  No launch when n == 0.
void LaunchFill(const Interval* intervals, int64_t n, uint32_t* plane, int pitch, hipStream_t stream);

// Edge rule + blend / concatenation from the filled plane into BGR24 rows.  src may be null for
// COMPOSE_RENDER.  out has H rows (2 * H for COMPOSE_CONCAT) of out_stride bytes.
void LaunchCompose(const uint32_t* plane, int pitch, int width, int height, const uint8_t* src,
                   size_t src_stride, uint8_t* out, size_t out_stride, int highlight_edges, int mode,
                   float alpha, hipStream_t stream);

}  // namespace vsg_render_impl

#endif  // VSG_RENDER_RENDER_H_
