// render_capi.cpp -- the one host translation unit of libvsg_render.so: every extern "C" entry point declared
// in include/vsg_render.h.
//
// ../common/capi_support.h keeps Throw, Guard, the thread's last error text, Block and StageClock in an unnamed
// namespace, so that the libraries loaded into one process do not share them.  vsg_render_last_error() and the
// entry points share that thread-local only inside one translation unit: the parts below are included here, in
// dependency order, and are not compiled on their own.
//
//   render_scan.h          the scans over segment heads the entry points call, with their head functors: the one
//                          place where this unit instantiates device code (the library's scan kernels)
//   render_desc.h          the proto reader, the hierarchy lookup, the polygon lines of a vector-only desc;
//                          host only, no HIP call
//   render_handle.h        struct vsg_render, the families' state, the stage enums, the helpers the families share
//   capi_level.inc         ingest, the id plane, runs, components, the level plane of the later families;
//                          vsg_render_level_regions, vsg_render_level_components
//   capi_frame.inc         create, destroy, options, vsg_render_frame, vsg_render_id_image, vsg_render_rasterize
//   capi_boundaries.inc    vsg_render_level_boundaries
//   capi_adjacency.inc     vsg_render_level_adjacency
//   capi_overlap.inc       vsg_render_level_overlap
//   capi_persistence.inc   vsg_render_persistence_image, _frame, _graph
//   capi_tree_cut.inc      vsg_render_tree_cut, _tuning
//   capi_colors.inc        vsg_render_level_colors, vsg_render_mean_frame
//   capi_pool.inc          vsg_render_level_pool, vsg_render_level_unpool
//   capi_volume.inc        vsg_render_volume_begin, _add, _table
//   capi_contours.inc      vsg_render_level_contours, vsg_render_level_mesh
//   capi_simplify.inc      vsg_render_level_mesh_simplified
//   capi_distance.inc      vsg_render_boundary_distance, vsg_render_boundary_benchmark
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/vsg_render.h"
#include "render.h"
#include "render_scan.h"
#include "persistence_table.h"
#include "../common/capi_support.h"

#include "render_desc.h"
#include "render_handle.h"
#include "capi_level.inc"
#include "capi_frame.inc"
#include "capi_boundaries.inc"
#include "capi_adjacency.inc"
#include "capi_overlap.inc"
#include "capi_persistence.inc"
#include "capi_tree_cut.inc"
#include "capi_colors.inc"
#include "capi_pool.inc"
#include "capi_volume.inc"
#include "capi_contours.inc"
#include "capi_simplify.inc"
#include "capi_distance.inc"
