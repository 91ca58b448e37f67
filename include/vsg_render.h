/*
 * vsg_render.h -- C ABI of the segmentation renderer (libvsg_render.so).
 *
 * Mirrors the reference's SegmentationRenderUnit (segmentation/segmentation_unit.cpp:478-655,
 * segment_util/segmentation_render.{h,cpp}) and SegmentationDescToIdImage
 * (segment_util/segmentation_util.cpp:741-770) on an MI355X: a serialized SegmentationDesc goes in,
 * a BGR24 picture of its regions at a hierarchy level (or an int32 image of their ids at a level)
 * comes out, in host or in device memory.  The library is independent of libvsg_hip.so; it reads the
 * few proto fields it needs (region.id, region.raster.scan_inter,
 * region.vectorization.polygon{coord_idx, hole}, vector_mesh.coord, rasterization_removed,
 * hierarchy[l].region{id,parent_id}, frame_width, frame_height) with a reader of its own.
 *
 * Vector-only descs.  The reference's result files carry no rasters: its writer strips them, sets
 * rasterization_removed and keeps Region2D.vectorization and the vector_mesh, and every consumer
 * rebuilds the scan intervals with RasterVectorization (segment_util/segmentation_util.cpp:1103-1246).
 * A desc with rasterization_removed = true and a vector_mesh is rendered from its polygons: the
 * scan conversion runs on the device (three stages: edge walk, radix sort by region and row, pairing)
 * with the reference's f32 arithmetic, operation for operation, and hands the same interval list to
 * the same two kernels.  Such a desc may have another frame size than the handle: its mesh is then
 * scaled to the handle's size as ScaleVectorization does (:1248-1267).  A desc without that flag is
 * handled as before, from its rasters, and has to have the handle's size.
 * A vectorization with a row the reference does not define is refused with VSG_ERR_INVALID: an odd
 * number of active edges; edges its comparator cannot order (three crossings chained within its
 * eps of 1e-3, or two it cannot tell apart at different x); an interval with left_x outside [0, W]
 * or right_x outside [-1, W - 1]; a coord_idx outside the mesh; a line outside rows [0, H].
 *
 * Conventions are those of vsg.h: every function returns VSG_OK (0) or a negative status,
 * vsg_render_last_error() is a thread-local message of the last failure, a handle is
 * thread-compatible and owns one HIP stream, and there is NO CPU fallback: without a usable HIP
 * device vsg_render_create fails with VSG_ERR_DEVICE.  Every call returns after its work on the
 * handle's stream has finished, so an output in device memory is complete on return; inputs in
 * device memory have to be complete when the call is made.
 *
 * Not offered (the reference has them): draw_shape_descriptors, and the two cv::putText overlays
 * ("Frame #...", "Change to chunk id ...") -- the Hershey glyphs are OpenCV's data.  A rendered
 * frame therefore equals the reference's up to those text pixels.  The inputs of
 * draw_shape_descriptors are available, though: vsg_render_level_regions returns every region of a
 * level with its merged rasterization, its area and its shape moments; the ellipse's axes and angle
 * (GetShapeDescriptorFromShapeMoments) and the drawing itself are left to the caller.  A region of a
 * level above 0 is usually several blobs in one frame; vsg_render_level_components returns the same
 * per connected component, and vsg_render_level_boundaries the boundary point lists of either: the
 * reference's GetBoundary (segment_util/segmentation_boundary.{h,cpp}), the N4 inner or outer boundary
 * pixels of a rasterization in row-major order.  Contour tracing at a level (BoundaryComputation,
 * segmentation/boundary.cpp) is offered by vsg_render_level_contours: the closed outlines of every region or
 * component as ordered vertex lists.  The reference's shared-segment mesh (segments cut at junctions and
 * shared by the two regions they separate) is offered by vsg_render_level_mesh, at any level and for
 * components, and the approxPolyDP simplification of its segments by vsg_render_level_mesh_simplified.  The
 * reference's polygon assembly on top of it (min_hole_length, its unordered_map hole order, the vector_mesh
 * numbering) is still not offered.
 * Which regions or components of a level touch in a frame, and along how many pixel sides, is what
 * vsg_render_level_adjacency returns; the reference has no per-frame counterpart
 * (CompoundRegion.neighbor_id covers a chunk in 3-D).  Scores
 * against ground truth and correspondence between frames are not offered either, but the table they are
 * all functions of is: vsg_render_level_overlap relates a level to a ground-truth label image or to the id
 * image of another frame.  Boundary scores over a whole hierarchy are not offered; the ultrametric contour
 * map they are functions of is: vsg_render_persistence_image, vsg_render_persistence_frame and
 * vsg_render_persistence_graph return, for every pixel side and for every pair of touching level-0
 * regions, the number of hierarchy levels at which the two sides are still different regions.
 * What a boundary benchmark counts within a distance tolerance is offered as integers:
 * vsg_render_boundary_distance is the exact squared distance transform of a level's edges, and
 * vsg_render_boundary_benchmark the matched boundary pixels of every level against a ground-truth label
 * image; the quotients (precision, recall, F) are left to the caller.
 * Appearance descriptors (Lab histograms, the hierarchical stage's) are not offered; the exact colour sums
 * of every group of a level and the mean-colour picture are: vsg_render_level_colors and
 * vsg_render_mean_frame.  Appearance beyond the 8-bit picture is the caller's own per-pixel data: a float
 * feature map of C channels (activations, flow, depth, logits) is pooled by the groups of a level, and group
 * values are painted back into feature planes, by vsg_render_level_pool and vsg_render_level_unpool; what is
 * derived from the pooled sums (means, variances, histograms, any colour space) is left to the caller.
 * All of the above is per frame; what a region id sums up to over the frames of a video
 * (life span, volume, trajectory, colour sums, overlap with ground-truth labels: the inputs of the 3-D
 * supervoxel scores) is accumulated on the device by a volume session: vsg_render_volume_begin, _add, _table.
 *
 * A well-formed SegmentationDesc rasterizes a partition of the frame: scan intervals do not
 * overlap.  Where they do, which region a pixel shows is unspecified (the reference paints in
 * region order).  Intervals outside the frame are refused with VSG_ERR_INVALID.
 */
#ifndef VSG_RENDER_H_
#define VSG_RENDER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef VSG_OK
#define VSG_OK 0
#define VSG_ERR_INVALID -1
#define VSG_ERR_DEVICE -2
#define VSG_ERR_STATE -3
#define VSG_ERR_INTERNAL -4
#define VSG_MEM_HOST 0
#define VSG_MEM_DEVICE 1
#endif

typedef struct vsg_render vsg_render;

/* SegmentationRenderUnitOptions (segmentation_unit.h) without the stream names. */
typedef struct vsg_render_options {
  float blend_alpha;       /* 0.5f; weight of the render over the source frame                    */
  float hierarchy_level;   /* 0; a value with a fractional part is a fraction of the hierarchy's
                            * height, resolved on the first frame (segmentation_unit.cpp:567-580)  */
  int highlight_edges;     /* 1; region boundaries in black                                       */
  int concat_with_source;  /* 0; 1 = output of 2*H rows, render on top, source frame below        */
  int has_video;           /* 1; 0 = no source frame: blend_alpha is forced to 1                  */
  int device;              /* -1 = the caller's current HIP device                                */
} vsg_render_options;

/* What the last vsg_render_frame / vsg_render_id_image call of a handle did.  Device times are HIP
 * events on the handle's stream around the kernels; host times are wall clock. */
typedef struct vsg_render_stats {
  double decode_ms;            /* proto decode, hierarchy lookup, colour table, interval list (host) */
  double upload_ms;            /* interval list to the device, frame to the device when it is host
                                * memory (host wall clock until the copies are enqueued)              */
  float clear_us, fill_us, compose_us;   /* plane clear, k_render_fill, k_render_compose            */
  int launches;                /* kernels + memsets + copies enqueued by the call                   */
  int64_t intervals;           /* scan intervals painted                                            */
  int64_t distinct_ids;        /* distinct mapped ids of the frame                                  */
  int64_t device_allocations;  /* hipMalloc / hipHostMalloc calls of the handle since creation      */
} vsg_render_stats;

const char* vsg_render_last_error(void);
void vsg_render_default_options(vsg_render_options* o);

/* concat_with_source without has_video is VSG_ERR_INVALID (the reference CHECK-fails,
 * segmentation_unit.cpp:613). */
int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** h);
void vsg_render_destroy(vsg_render* h);

/* Renders one frame.  seg: serialized SegmentationDesc (host).  bgr: the BGR24 source frame of
 * `stride` bytes per row in mem_in memory (ignored without has_video, required with it).  out: H
 * (or 2*H) rows of out_stride bytes in mem_out memory; out_stride 0 = vsg_render_default_stride.
 * Only the first 3*W bytes of each output row are written.
 * The first frame's desc is kept as the hierarchy and resolves the level; every later desc that
 * carries a hierarchy replaces the kept one (segmentation_unit.cpp:567-591). */
int vsg_render_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr,
                     size_t stride, int mem_in, uint8_t* out, size_t out_stride, int mem_out);

/* SegmentationDescToIdImage(level, ...): W*H int32, the id at `level` of the region covering each
 * pixel, -1 where none does.  The hierarchy is the desc's own when it carries one (it then also
 * replaces the handle's kept one), else the kept one.  level < 0, or level > 0 and not below the
 * hierarchy's height, is VSG_ERR_INVALID (the reference's clamp at segmentation_util.cpp:748
 * would index past the last level there). */
int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level,
                        int32_t* out_int32, int mem_out);

/* The level the handle resolved on its first rendered frame (-1 for an over-segmentation without
 * hierarchy, which renders as level 0); VSG_ERR_STATE before the first frame. */
int vsg_render_level(vsg_render* h, int* level);

/* 3*W rounded up to a multiple of 4 (segmentation_unit.cpp:526-529). */
size_t vsg_render_default_stride(int width);

int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s);

/* ReplaceRasterizationFromVectorization (segmentation_util.cpp:1238-1246) as a service: the scan
 * intervals of every region's vectorization, scaled to the handle's frame size, as int32 quadruples
 * {y, left_x, right_x, region_id} in the reference's order: regions in the desc's order, rows
 * upwards, left to right.  The empty intervals the reference emits where two edges start at one
 * vertex (left_x = right_x + 1) are included.  The desc needs a vector_mesh; rasterization_removed
 * is not looked at, rasters are ignored, and the handle's kept hierarchy is left alone.
 * *count is the number of intervals of the frame; when capacity_intervals is smaller the call
 * fails with VSG_ERR_INVALID, *count set and out untouched.  out: mem_out memory.
 * out == NULL with capacity_intervals == 0 asks for the count only: the desc is decoded and its lines
 * are checked on the host, nothing runs on the device, and the call returns VSG_OK with *count. */
int vsg_render_rasterize(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* out,
                         size_t capacity_intervals, size_t* count, int mem_out);

/* What the vector path of the handle's last call did (all zero after a call on a desc with
 * rasters).  Device times are HIP events around the stages. */
typedef struct vsg_render_vector_stats {
  int64_t lines;           /* polygon lines kept (|dy| >= 1e-3)                                    */
  int64_t crossings;       /* line x row crossings = 2 * intervals                                 */
  int64_t groups;          /* (region, row) pairs with at least one crossing                       */
  int64_t largest_group;   /* most crossings of one region in one row                              */
  float walk_us, sort_us, pairs_us;   /* k_vec_walk, the radix sort, k_vec_pairs                   */
  int launches;            /* enqueued by the vector stages; the radix sort counts as one          */
} vsg_render_vector_stats;

int vsg_render_last_vector_stats(vsg_render* h, vsg_render_vector_stats* s);

/* One region of a hierarchy level, as vsg_render_level_regions returns it. */
typedef struct vsg_render_level_region {      /* 56 bytes, no padding */
  int32_t id;                /* region id at `level` (GetParentId(overseg_id, 0, level))            */
  int32_t first_interval;    /* index of its first interval in the interval list                    */
  int32_t num_intervals;
  int32_t area;              /* RasterizationArea of the merged rasterization                       */
  int32_t min_x, min_y, max_x, max_y;          /* bounding box, inclusive                           */
  float size, mean_x, mean_y, moment_xx, moment_xy, moment_yy;   /* ShapeMomentsFromRasterization   */
} vsg_render_level_region;

/* The regions of hierarchy level `level` with their rasterizations, areas and shape moments: what
 * GetParentMap + GetCompoundRegionRasterizations (segment_util/segmentation_util.cpp:199-213,
 * 592-605), RasterizationArea (:644-650) and ShapeMomentsFromRasterization (:652-693) give, computed
 * on the device from the id plane of vsg_render_id_image.
 * regions: ordered by ascending id.  intervals: int32 quadruples {y, left_x, right_x, region_id} as
 * vsg_render_rasterize writes them, grouped by region in the order of the region list, within a
 * region in ScanIntervalComparator order (y, then left_x).  Both in mem_out memory.
 * Level and hierarchy are those of vsg_render_id_image: the desc's own hierarchy when it carries one
 * (it then replaces the kept one), else the kept one; level 0 needs none; level < 0, or level > 0
 * and not below the hierarchy's height, an unsorted level or an id missing from one is
 * VSG_ERR_INVALID.  A vector-only desc (rasterization_removed) is scan converted on the device
 * first, at the handle's size.  Region ids have to be non-negative.
 *
 * A region's rasterization is the set of maximal runs of its id per row of the id plane; pixels
 * without a region (-1) belong to no run and a run ends with its row.  Where no region has two
 * touching intervals in one row (left_x = right_x + 1 of its neighbour) this is exactly what
 * MergeRasterizations returns, whatever the order of the children; every desc this project or the
 * reference's dense unit writes is of that kind.  Where one region does have touching intervals, the
 * reference joins them only in rows that a second child shares (MergeRasterization copies a row
 * only one side has), so its result depends on the children; this call returns the maximal runs.
 * Overlapping intervals are unspecified, as for the picture.
 * The moments are ShapeMomentsFromRasterization applied to that list in its order, f32 operation
 * for operation: every sum is accumulated interval by interval, so the bits are the reference's.
 *
 * *num_regions and *num_intervals are always set on VSG_OK and when a capacity is too small; in
 * that case the call fails with VSG_ERR_INVALID and neither output is touched.  regions == NULL and
 * intervals == NULL with both capacities 0 asks for the counts only (VSG_OK); the counts come from
 * the plane, so this needs the device too.  A null handle or a null count pointer is
 * VSG_ERR_INVALID and touches no device. */
int vsg_render_level_regions(vsg_render* h, const uint8_t* seg, size_t seg_len, int level,
                             vsg_render_level_region* regions, size_t capacity_regions, size_t* num_regions,
                             int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int mem_out);

/* What the last vsg_render_level_regions call of the handle did.  Device times are HIP events around
 * the stages: k_level_runs; the radix sort; the scan and k_level_table; k_level_moments (not run,
 * like largest_region_intervals not known, in a count-only call). */
typedef struct vsg_render_level_stats {
  int64_t runs, regions, largest_region_intervals;
  float runs_us, sort_us, table_us, moments_us;
  int launches;
} vsg_render_level_stats;
int vsg_render_last_level_stats(vsg_render* h, vsg_render_level_stats* s);

#define VSG_RENDER_CONNECT_N4 1   /* SegmentationDesc::N4_CONNECT */
#define VSG_RENDER_CONNECT_N8 2   /* SegmentationDesc::N8_CONNECT */

/* One connected component of a region of a hierarchy level, as vsg_render_level_components returns
 * it. */
typedef struct vsg_render_level_component {   /* 64 bytes, no padding */
  int32_t id;                 /* region id at `level` */
  int32_t component;          /* 0-based index among its region's components, reference order */
  int32_t region_components;  /* how many components that region has */
  int32_t first_interval, num_intervals;
  int32_t area;
  int32_t min_x, min_y, max_x, max_y;
  float size, mean_x, mean_y, moment_xx, moment_xy, moment_yy;
} vsg_render_level_component;

/* The connected components of every region of hierarchy level `level`: ConnectedComponents
 * (segment_util/segmentation_util.cpp:1007-1101) applied to each region's rasterization, with
 * RasterizationArea and ShapeMomentsFromRasterization of every component, computed on the device.
 *
 * Input is the id plane of vsg_render_id_image at `level`; decode, hierarchy rules, refusals and the
 * handling of vector-only descs are those of vsg_render_level_regions, region ids have to be
 * non-negative, and pixels without a region (-1) belong to no component.  A region's rasterization is
 * the list vsg_render_level_regions returns: its maximal runs per row in (y, left_x) order.
 * Two runs of one region are neighbours as in ScanIntervalsNeighbored: |dy| <= 1 and, for
 * VSG_RENDER_CONNECT_N4, max(left_x) <= min(right_x); for VSG_RENDER_CONNECT_N8,
 * max(left_x) - min(right_x) <= 1.  Maximal runs never touch within a row, so only runs of adjacent
 * rows are neighbours, and the components are exactly the 4-connected (8-connected) components of
 * the pixels of each id.  Any other connectedness is VSG_ERR_INVALID.
 * Order is that of ConnectedComponents' second loop: a region's components are ordered by the first
 * appearance of their intervals in the region's list, that is by their first pixel in row-major
 * order, and a component keeps its intervals in list order.  Regions are ordered by ascending id.
 * area, bounding box and moments are RasterizationArea and ShapeMomentsFromRasterization applied to
 * the component's interval list in that order, f32 operation for operation, by the kernel that
 * computes them for vsg_render_level_regions.
 *
 * components: ordered by (id, component).  intervals: int32 quadruples {y, left_x, right_x,
 * region_id}, grouped by component in the order of the component list.  label_image: NULL, or W*H
 * int32 that receive the index of each pixel's component in the component list, -1 where there is
 * none.  All in mem_out memory.
 * *num_components and *num_intervals are always set on VSG_OK and when a capacity is too small; in
 * that case the call fails with VSG_ERR_INVALID and no output is touched, the label image included.
 * components == NULL, intervals == NULL and label_image == NULL with both capacities 0 asks for the
 * counts only (VSG_OK; needs the device).  A null handle, a null count pointer or a bad connectedness
 * is VSG_ERR_INVALID and touches no device. */
int vsg_render_level_components(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                                vsg_render_level_component* components, size_t capacity_components, size_t* num_components,
                                int32_t* intervals, size_t capacity_intervals, size_t* num_intervals,
                                int32_t* label_image, int mem_out);

/* What the last vsg_render_level_components call of the handle did.  links: neighbour pairs found
 * between adjacent rows (fewer than 2 * runs).  Device times are HIP events around the stages:
 * k_level_runs; the radix sort, the scan and k_level_table of the runs; the union-find (k_comp_init,
 * k_comp_link, k_comp_flatten); the radix sort by component, the scan, k_comp_table and
 * k_comp_finish; the moments; the label image's clear and fill.  The time the stream idles while the
 * host reads the number of components is in none of them.  The last two are not run, and
 * largest_component_intervals is not known, in a count-only or refused call. */
typedef struct vsg_render_component_stats {
  int64_t runs, regions, components, links, largest_component_intervals;
  float runs_us, sort_us, link_us, order_us, moments_us, label_us;
  int launches;
} vsg_render_component_stats;
int vsg_render_last_component_stats(vsg_render* h, vsg_render_component_stats* s);

#define VSG_RENDER_BOUNDARY_INNER 0
#define VSG_RENDER_BOUNDARY_OUTER 1

/* One boundary, as vsg_render_level_boundaries returns it. */
typedef struct vsg_render_level_boundary {   /* 16 bytes, no padding */
  int32_t id;           /* region id at `level` */
  int32_t component;    /* index among its region's components; -1 with connectedness 0 */
  int32_t first_point, num_points;
} vsg_render_level_boundary;

/* The N4 boundary pixels of every region of hierarchy level `level`, or of every connected component
 * of its regions: GetBoundary (segment_util/segmentation_boundary.cpp:78-179) applied to each of their
 * rasterizations, computed on the device.
 *
 * Let P be an int32 plane of W x H, -1 where nothing covers the pixel; positions outside the frame
 * count as -1.  A group g >= 0 is a value of P.
 *   inner(g): the positions (x, y) with P = g and at least one of the four neighbours != g.  The frame
 *     edge therefore always bounds a region.  This is the reference's result exactly.
 *   outer(g): the positions (x, y) of [-1, W] x [-1, H] with P != g and at least one of the four
 *     neighbours = g.  Positions outside the frame and uncovered pixels are included, a pixel of another
 *     group is an outer point of g, and a position is an outer point of up to four groups; it is listed
 *     once per group, however many of its neighbours belong to that group.
 * Within a group the points are ordered by y, then by x: the order of the reference's loops.
 * connectedness 0: P is the id plane of vsg_render_id_image at `level`; one boundary per region,
 * regions in ascending id, record k belonging to record k of vsg_render_level_regions.
 * VSG_RENDER_CONNECT_N4 / _N8: P is the label image of vsg_render_level_components with that
 * connectedness; one boundary per component in the component list's order, record k belonging to
 * record k of that call (which is made internally: vsg_render_last_component_stats then describes it).
 * Every group has at least one inner and at least one outer point, so the lists align one to one.
 *
 * Two things differ from the reference's outer mode, on purpose:
 *  1. The reference reports every outer point with x one too large: its row pointers start at
 *     min_range - shift while its x starts at min_range (segmentation_boundary.cpp:148-154), so
 *     reference_x = x + 1 throughout, y being right.  This call returns the true position x.
 *  2. The reference's outer mode reads one byte before the first row of the caller's buffer (the left
 *     neighbour of position -1 of its first row) and, with a buffer of the advertised size
 *     3 * (frame_width + 2), one byte past the last row.  This call treats those positions as not in
 *     the region, which is what the reference computes whenever the bytes it happens to read are zero.
 *
 * boundaries: one record per group.  points: int32 pairs {x, y}, grouped by boundary in list order;
 * x is in [-1, W] and y in [-1, H] for outer points.  Both in mem_out memory.
 * Decode, hierarchy rules, refusals, the non-negative ids and the handling of vector-only descs are
 * those of vsg_render_level_regions.
 * *num_boundaries and *num_points are always set on VSG_OK and when a capacity is too small; in that
 * case the call fails with VSG_ERR_INVALID and neither output is touched.  boundaries == NULL and
 * points == NULL with both capacities 0 asks for the counts only (VSG_OK; needs the device).  A null
 * handle, a null count pointer, a connectedness other than 0, VSG_RENDER_CONNECT_N4 and
 * VSG_RENDER_CONNECT_N8 or a `which` other than the two above is VSG_ERR_INVALID and touches no
 * device. */
int vsg_render_level_boundaries(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                                int which, vsg_render_level_boundary* boundaries, size_t capacity_boundaries,
                                size_t* num_boundaries, int32_t* points, size_t capacity_points,
                                size_t* num_points, int mem_out);

/* What the last vsg_render_level_boundaries call of the handle did.  Device times are HIP events
 * around the stages: making the plane (the id plane's clear and fill; with a connectedness, also every
 * stage of the internal vsg_render_level_components call up to its label image); the count pass of
 * k_bound_classify; its emit pass; the radix sort; the scan, k_bound_table and k_bound_finish.  The
 * last three are not run, and boundaries and largest_boundary_points are 0, when there is no point. */
typedef struct vsg_render_boundary_stats {
  int64_t points, boundaries, largest_boundary_points;
  float plane_us, count_us, emit_us, sort_us, table_us;
  int launches;
} vsg_render_boundary_stats;
int vsg_render_last_boundary_stats(vsg_render* h, vsg_render_boundary_stats* s);

#define VSG_RENDER_ADJACENT_N4 1   /* pixel sides only */
#define VSG_RENDER_ADJACENT_N8 2   /* pixel sides and diagonal contacts */

/* One node of the adjacency graph, as vsg_render_level_adjacency returns it. */
typedef struct vsg_render_level_node {   /* 28 bytes, no padding */
  int32_t id;                /* region id at `level` */
  int32_t component;         /* index among its region's components; -1 with connectedness 0 */
  int32_t first_edge, num_edges;
  int32_t border_frame;      /* pixel sides of the group on the frame edge */
  int32_t border_uncovered;  /* pixel sides next to an uncovered (-1) pixel inside the frame */
  int32_t border_shared;     /* pixel sides next to another group = sum of shared_n4 of its edges */
} vsg_render_level_node;

/* One directed edge of the adjacency graph. */
typedef struct vsg_render_level_edge {   /* 16 bytes, no padding */
  int32_t neighbour;         /* index of the neighbour in the node list */
  int32_t neighbour_id;      /* its region id (equal to the node's own id for two components of one region) */
  int32_t shared_n4;         /* pixel sides the two groups share */
  int32_t shared_diagonal;   /* diagonal contacts; 0 with VSG_RENDER_ADJACENT_N4 */
} vsg_render_level_edge;

/* The region adjacency graph of hierarchy level `level`: which regions, or which connected components
 * of its regions, touch which, and along how much border.  Computed on the device.
 *
 * The plane.  P is the plane of vsg_render_level_boundaries: the id plane of vsg_render_id_image at
 * `level` for connectedness 0, or the label image of vsg_render_level_components for
 * VSG_RENDER_CONNECT_N4 / _N8 (that call is made internally: vsg_render_last_component_stats then
 * describes it).  Positions outside the frame are not pixels.  A group g >= 0 is a value of P.
 *
 * Sides.  Every pixel of g has four sides, each classified by what lies across it:
 *   outside the frame:           the side counts to border_frame;
 *   an in-frame pixel with -1:   the side counts to border_uncovered;
 *   a pixel of another group b:  the side counts to border_shared of g and to shared_n4 of the edge g -> b;
 *   a pixel of g:                the side counts to nothing.
 * So border_frame + border_uncovered + border_shared is the group's perimeter in pixel sides.
 *
 * Diagonal contacts.  With VSG_RENDER_ADJACENT_N8, every pair of in-frame positions {(x, y), (x+1, y+1)}
 * or {(x+1, y), (x, y+1)} with different non-negative values a, b adds 1 to shared_diagonal of a -> b and
 * of b -> a; the other two pixels of that 2 x 2 block do not matter.  An edge exists when
 * shared_n4 + shared_diagonal > 0.  With VSG_RENDER_ADJACENT_N4 only sides make edges, and
 * shared_diagonal is 0.
 *
 * Nodes.  One node per group; every group has at least one bordering side, so no group is lost.  The
 * order is that of the sibling calls: ascending id for connectedness 0, record k belonging to record k
 * of vsg_render_level_regions; the component list's order otherwise, record k belonging to record k of
 * vsg_render_level_components.
 *
 * Edges.  Grouped by node in node order, and within a node by ascending `neighbour`.  The graph is
 * symmetric: a -> b is listed iff b -> a is, with equal counts.  Under N4 components two components of
 * one region can touch diagonally; that is an edge with neighbour_id equal to the node's own id.
 *
 * Decode, hierarchy rules (the desc's own hierarchy replaces the kept one), refusals, the non-negative
 * ids and the handling of vector-only descs are those of vsg_render_level_regions.
 * *num_nodes and *num_edges are always set on VSG_OK and when a capacity is too small; in that case the
 * call fails with VSG_ERR_INVALID and neither output is touched.  nodes == NULL and edges == NULL with
 * both capacities 0 asks for the counts only (VSG_OK; needs the device).  A null handle, a null count
 * pointer, a connectedness other than 0, VSG_RENDER_CONNECT_N4 and VSG_RENDER_CONNECT_N8 or a
 * neighbourhood other than the two above is VSG_ERR_INVALID and touches no device.  A frame with no
 * covered pixel returns zero nodes and zero edges.  Both lists in mem_out memory. */
int vsg_render_level_adjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                               int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes,
                               size_t* num_nodes, vsg_render_level_edge* edges, size_t capacity_edges,
                               size_t* num_edges, int mem_out);

/* What the last vsg_render_level_adjacency call of the handle did.  sides: the sum over the nodes of
 * the three border fields plus the sum over the edges of shared_diagonal, a property of the plane.
 * keys: what the radix sort saw; equal to sides, since equal keys are not combined before the sort.
 * Device times are HIP events around the stages: making the plane (as in vsg_render_boundary_stats);
 * the count pass of k_adj_classify; its emit pass; the radix sort; the clears, the scan, k_adj_table,
 * k_adj_finish and k_adj_resolve.  The last three are not run, and nodes, edges and largest_node_edges
 * are 0, when there is no key. */
typedef struct vsg_render_adjacency_stats {
  int64_t sides, keys, nodes, edges, largest_node_edges;
  float plane_us, count_us, emit_us, sort_us, table_us;
  int launches;
} vsg_render_adjacency_stats;
int vsg_render_last_adjacency_stats(vsg_render* h, vsg_render_adjacency_stats* s);

/* One row of the overlap table, as vsg_render_level_overlap returns it: a group of the level. */
typedef struct vsg_render_overlap_row {    /* 32 bytes, no padding */
  int32_t id;            /* region id at `level` */
  int32_t component;     /* index among its region's components; -1 with connectedness 0 */
  int32_t first_pair, num_pairs;
  int32_t area;          /* pixels of the group */
  int32_t unlabelled;    /* of those, pixels where the other plane is negative */
  int32_t best_label;    /* label with the largest count; ties: the smallest label; -1 when num_pairs == 0 */
  int32_t best_count;    /* its count; 0 when num_pairs == 0 */
} vsg_render_overlap_row;

/* One column of the overlap table: a label of the other plane. */
typedef struct vsg_render_overlap_col {    /* 24 bytes, no padding */
  int32_t label;         /* a non-negative value of the other plane */
  int32_t area;          /* pixels of the frame with that label */
  int32_t uncovered;     /* of those, pixels where P is -1 */
  int32_t num_pairs;     /* groups it overlaps */
  int32_t best_row;      /* index in the row list of the group with the largest count; ties: the smallest
                            index; -1 when num_pairs == 0 */
  int32_t best_count;
} vsg_render_overlap_col;

/* One non-empty cell of the overlap table. */
typedef struct vsg_render_overlap_pair {   /* 16 bytes, no padding */
  int32_t row, col;      /* indices into the two lists */
  int32_t label;         /* cols[col].label */
  int32_t count;         /* pixels with P = the row's group and other = label; > 0 */
} vsg_render_overlap_pair;

/* The overlap (contingency) table of hierarchy level `level` and a plane of labels: for every (group of
 * the level, label of the other plane) the number of pixels where both hold, with the marginals of either
 * side.  Every score of a segmentation against ground truth (undersegmentation error, achievable
 * segmentation accuracy, the Rand-type scores) and the correspondence of a level between two frames are
 * functions of it.  Computed on the device, in integers throughout.
 *
 * The planes.  P is the plane of vsg_render_level_boundaries: the id plane of vsg_render_id_image at
 * `level` for connectedness 0, or the label image of vsg_render_level_components for
 * VSG_RENDER_CONNECT_N4 / _N8 (that call is made internally: vsg_render_last_component_stats then
 * describes it).  B is `other`: H rows of other_pitch int32 in mem_other memory, host or device,
 * independent of mem_out; other_pitch 0 means W, and only the first W values of a row are read.  Every
 * int32 is a legal value of B, and every negative value means "no label" (ground-truth void): no label
 * value is refused.  B is read only; it may be memory that an earlier vsg_render_id_image or
 * vsg_render_level_components of the same handle wrote.
 *
 * Rows.  One row per group of P, in the order of the sibling calls: record k belongs to record k of
 * vsg_render_level_regions for connectedness 0, of vsg_render_level_components otherwise.  area is the
 * pixels of the group, unlabelled those of them with B < 0, so area - unlabelled is the sum of the counts
 * of its pairs.
 *
 * Cols.  One column per distinct non-negative value of B inside the frame, ascending; values covered by no
 * group are included.  area - uncovered is the sum of the counts of its pairs.
 *
 * Pairs.  One pair per (group, label) with at least one common pixel, grouped by row in row order and
 * within a row by ascending label, which is ascending col.
 *
 * Decode, hierarchy rules (the desc's own hierarchy replaces the kept one), level refusals, the
 * non-negative ids and the handling of vector-only descs are those of vsg_render_level_regions.
 * *num_rows, *num_cols and *num_pairs are always set on VSG_OK and when a capacity is too small; in that
 * case the call fails with VSG_ERR_INVALID and no output is touched.  All three outputs NULL with all three
 * capacities 0 asks for the counts only (VSG_OK; needs the device).  A null handle, a null count pointer, a
 * null `other`, a mem_other that is not one of the two memory kinds, an other_pitch that is neither 0 nor
 * >= W, or a connectedness other than 0, VSG_RENDER_CONNECT_N4 and VSG_RENDER_CONNECT_N8 is
 * VSG_ERR_INVALID and touches no device; all but the pitch, which is compared with the handle's width, are
 * answered before the handle is dereferenced.  A frame with no covered pixel returns zero rows and zero
 * pairs, and still every column.  A B without a label returns zero cols and zero pairs, and still every
 * row.  All three lists in mem_out memory. */
int vsg_render_level_overlap(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                             const int32_t* other, size_t other_pitch, int mem_other,
                             vsg_render_overlap_row* rows, size_t capacity_rows, size_t* num_rows,
                             vsg_render_overlap_col* cols, size_t capacity_cols, size_t* num_cols,
                             vsg_render_overlap_pair* pairs, size_t capacity_pairs, size_t* num_pairs,
                             int mem_out);

/* What the last vsg_render_level_overlap call of the handle did.  covered: pixels with P >= 0; labelled:
 * pixels with B >= 0; both: the sum of all counts.  runs: what the radix sort saw, the maximal runs, per
 * frame row, of constant (P, B) with at least one of the two non-negative; a run ends with its row.
 * Device times are HIP events around the stages: making the plane (as in vsg_render_boundary_stats) and
 * bringing a host B to the device; the count pass of k_overlap_runs with k_overlap_totals; its emit pass;
 * the radix sort of the runs; everything after it (the scans, k_overlap_table, k_overlap_pairs,
 * k_overlap_rows, the sort of the distinct keys by label, k_overlap_col_heads, k_overlap_cols).  The last
 * three are not run, and rows, cols, pairs and largest_row_pairs are 0, when there is no run. */
typedef struct vsg_render_overlap_stats {
  int64_t covered, labelled, both, runs, rows, cols, pairs, largest_row_pairs;
  float plane_us, count_us, emit_us, sort_us, table_us;
  int launches;
} vsg_render_overlap_stats;
int vsg_render_last_overlap_stats(vsg_render* h, vsg_render_overlap_stats* s);

/* ---- Boundary persistence: the edges of all hierarchy levels in one pass ----
 *
 * Hierarchy.  The desc's own hierarchy when it carries one, else the handle's kept one.  A desc's own
 * hierarchy replaces the kept one, exactly as in vsg_render_id_image.
 * Height.  L = max(1, number of levels of that hierarchy).  L > 65535 is VSG_ERR_INVALID.
 * Ancestors.  A_l(r) = GetParentId(r, 0, l) for l in [0, L), with A_0(r) = r.  The lookups and refusals
 * are exactly those of vsg_render_id_image at level L - 1: an unsorted level or an id missing from a level
 * is VSG_ERR_INVALID, and so is a negative region id, as in vsg_render_level_regions.  Only regions that
 * paint at least one pixel (that have a scan interval or, in a vector-only desc, a polygon) are looked up.
 * Persistence of two region ids.  pers(a, b) is the number of l in [0, L) with A_l(a) != A_l(b).  So
 * pers(a, a) = 0, and pers(a, b) is in [1, L] for a != b.  "No region" (-1) against a region is L; -1
 * against -1 is 0.  A_{l+1} is a function of A_l, so "differ at l" is monotone in l; the device finds the
 * count by bisection over a table of ancestors.
 * The persistence plane Q, W x H int32, with P0 the level-0 id image:
 *   Q(x, y) = max( pers(P0(x,y), P0(x+1,y)) if x+1 < W,  pers(P0(x,y), P0(x,y+1)) if y+1 < H ),
 * and 0 when neither neighbour exists.  This is the reference's edge rule (segmentation_render.h:159-182:
 * right and below, in frame), as vsg_render_frame applies it.  Consequence: for every l in [0, L), Q > l
 * holds exactly where vsg_render_id_image(level = l) differs from its in-frame right or below neighbour,
 * -1 counting as a value; so Q > l is the set of pixels highlight_edges blackens at level l.
 * The persistence picture, H rows of BGR24: every byte is (s * (L - Q) + L / 2) / L in unsigned integer
 * arithmetic, s being the source frame's byte with has_video and 255 without.  Only the first 3 * W bytes
 * of a row are written; out_stride 0 means vsg_render_default_stride.  blend_alpha, highlight_edges,
 * hierarchy_level and concat_with_source are not looked at.  There are no floats in it.
 * The persistence graph.  Nodes and edges are byte for byte those of
 * vsg_render_level_adjacency(level 0, connectedness 0, neighbourhood).  persistence[e] = pers(the id of
 * the node edge e belongs to, its neighbour_id) for every directed edge e; it is symmetric.  level_sides[l]
 * for l in [0, L) is an int64: the number of unordered pairs of in-frame, side-adjacent pixels whose ids at
 * level l are both >= 0 and differ.  Equivalently, level_sides[l] = 1/2 of the sum of shared_n4 over the
 * edges with persistence > l, and 1/2 of the sum of border_shared over the nodes of
 * vsg_render_level_adjacency at level l.  With VSG_RENDER_ADJACENT_N8, an edge that is diagonal-only
 * (shared_n4 = 0) still gets its persistence.
 *
 * vsg_render_persistence_image writes Q (W * H int32, rows W apart) to out_int32 in mem_out memory and L to
 * *num_levels.  vsg_render_persistence_frame writes the picture to `out` and L to *num_levels; bgr, stride
 * and mem_in are those of vsg_render_frame: bgr is required with has_video and ignored without.
 * vsg_render_persistence_graph runs the adjacency pipeline at level 0 internally
 * (vsg_render_last_adjacency_stats then describes it), then one kernel over the edges and one small
 * reduction.  The number of launches of each call does not depend on L.
 *
 * *num_nodes, *num_edges and *num_levels are always set on VSG_OK and when a capacity is too small (the
 * persistence list has capacity_edges entries); in that case the call fails with VSG_ERR_INVALID and no
 * output is touched.  All four outputs NULL with all three capacities 0 asks for the counts only (VSG_OK;
 * needs the device).  A null handle, a null output of the image and frame calls, a null count pointer,
 * an unknown memory kind or a neighbourhood other than VSG_RENDER_ADJACENT_N4 and
 * VSG_RENDER_ADJACENT_N8 is VSG_ERR_INVALID, answered before the handle is dereferenced, and touches no
 * device.  Vector-only descs are scan converted at the handle's size first.  Every call returns after its
 * stream work has finished. */
int vsg_render_persistence_image(vsg_render* h, const uint8_t* seg, size_t seg_len,
                                 int32_t* out_int32, int* num_levels, int mem_out);
int vsg_render_persistence_frame(vsg_render* h, const uint8_t* seg, size_t seg_len,
                                 const uint8_t* bgr, size_t stride, int mem_in,
                                 uint8_t* out, size_t out_stride, int mem_out, int* num_levels);
int vsg_render_persistence_graph(vsg_render* h, const uint8_t* seg, size_t seg_len, int neighbourhood,
                                 vsg_render_level_node* nodes, size_t capacity_nodes, size_t* num_nodes,
                                 vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges,
                                 int32_t* persistence,            /* capacity_edges entries */
                                 int64_t* level_sides, size_t capacity_levels, size_t* num_levels,
                                 int mem_out);

/* What the last persistence call of the handle did; fields that a call does not compute are 0.  levels: L.
 * regions: the columns of the ancestor table, the distinct ids of the regions that paint.  edge_pixels and
 * top_pixels (image and frame calls): pixels with Q > 0 and with Q == L.  nodes and edges (graph call).
 * Device times are HIP events around the stages: plane_us, making the level-0 plane (clear and fill);
 * persist_us, k_persist_plane, or k_persist_edges with k_persist_sides; compose_us, k_persist_compose;
 * graph_us, the count, emit, sort and table stages of the internal adjacency call. */
typedef struct vsg_render_persistence_stats {
  int64_t levels, regions, edge_pixels /* Q > 0 */, top_pixels /* Q == L */, nodes, edges;
  float plane_us, persist_us, compose_us, graph_us;
  int launches;
} vsg_render_persistence_stats;
int vsg_render_last_persistence_stats(vsg_render* h, vsg_render_persistence_stats* s);

/* ---- Level colours: per-group colour sums and the mean-colour picture ----
 *
 * One record of the colour table, as vsg_render_level_colors returns it. */
typedef struct vsg_render_level_color {   /* 72 bytes, no padding */
  int32_t id;            /* region id at `level` */
  int32_t component;     /* index among its region's components; -1 with connectedness 0 */
  int32_t area;          /* pixels of the group */
  uint8_t mean[3];       /* B, G, R: (2 * sum[c] + area) / (2 * area), integer division */
  uint8_t reserved0;     /* written as 0 */
  int64_t sum[3];        /* B, G, R over the group's pixels */
  int64_t sum_sq[3];     /* squares of the same bytes */
  uint8_t min[3], max[3];
  uint8_t reserved1[2];  /* written as 0 */
} vsg_render_level_color;

/* What every group of hierarchy level `level` looks like in the frame: the sums, the sums of squares, the
 * minima and the maxima of the three 8-bit channels over the group's pixels, and the picture of the level
 * painted in mean colours.  Computed on the device, in integers throughout: there are no floats, no colour
 * conversion and no histogram in it.
 *
 * The planes.  P is the plane of vsg_render_level_overlap: the id plane of vsg_render_id_image at `level`
 * for connectedness 0, or the label image of vsg_render_level_components for VSG_RENDER_CONNECT_N4 / _N8
 * (that call is made internally: vsg_render_last_component_stats then describes it).  F is `bgr`: H rows
 * of `stride` bytes of BGR24 in mem_in memory, host or device, independent of mem_out.  Only the first
 * 3 * W bytes of a row are read; a stride below 3 * W is VSG_ERR_INVALID.  F is required whatever the
 * handle's has_video.  It is read once per call; a host frame is copied to the device first, as in
 * vsg_render_frame.
 *
 * The table.  One record per group of P, in the order of the sibling calls: record k belongs to record k of
 * vsg_render_level_regions for connectedness 0, of vsg_render_level_components otherwise, with the same id,
 * component and area.  Pixels with P < 0 enter no record.  sum[c], sum_sq[c], min[c] and max[c] are over
 * the bytes F(x, y)[c] of the group's pixels, c = 0, 1, 2 being B, G, R.  mean[c] is sum[c] / area rounded
 * half up, in integers: (2 * sum[c] + area) / (2 * area).  Nothing else is derived on the device: the
 * variance of a channel is sum_sq / area - (sum / area)^2, left to the caller.
 *
 * The picture.  C(x, y) is the packed mean (B | G << 8 | R << 16) of the group at (x, y), and 0 (black)
 * where P < 0, exactly as the cleared plane of vsg_render_frame.  vsg_render_mean_frame writes what
 * vsg_render_frame makes of that colour plane with the handle's own options: the edge rule on colours
 * (highlight_edges: a pixel is black where its colour differs from its in-frame right or below neighbour's,
 * so two touching groups with equal means show no edge between them, and a group whose mean is black shows
 * none against uncovered pixels), the blend with blend_alpha (forced to 1 without has_video),
 * concat_with_source, out_stride 0 = vsg_render_default_stride, and only the first 3 * W bytes of each
 * output row written.  The picture is made by the two kernels of vsg_render_frame, unchanged.  The call
 * neither resolves nor changes the level the handle keeps for vsg_render_frame (vsg_render_level).
 *
 * Decode, hierarchy rules (the desc's own hierarchy replaces the kept one), level refusals, the
 * non-negative ids and the handling of vector-only descs are those of vsg_render_level_regions.
 * *num_colors is always set on VSG_OK and when the capacity is too small; in that case the call fails with
 * VSG_ERR_INVALID and nothing is written.  colors == NULL with capacity 0 asks for the count only (VSG_OK;
 * needs the device).  A null handle, a null count pointer, a null bgr, a null out, a memory kind other than
 * the two, or a connectedness other than 0, VSG_RENDER_CONNECT_N4 and VSG_RENDER_CONNECT_N8 is
 * VSG_ERR_INVALID, answered before the handle is dereferenced, and touches no device.  The stride is the
 * exception: it is compared with the handle's width, so it is answered after the handle is read.  A frame
 * with no covered pixel returns zero records, and a picture that is black before the blend.  The table in
 * mem_out memory. */
int vsg_render_level_colors(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                            const uint8_t* bgr, size_t stride, int mem_in,
                            vsg_render_level_color* colors, size_t capacity_colors, size_t* num_colors,
                            int mem_out);

int vsg_render_mean_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                          const uint8_t* bgr, size_t stride, int mem_in,
                          uint8_t* out, size_t out_stride, int mem_out);

/* What the last vsg_render_level_colors or vsg_render_mean_frame call of the handle did.  groups: the
 * records.  intervals: the maximal runs of P, the entries of the interval list.  covered: pixels with
 * P >= 0, the sum of the areas.  largest_group_intervals: most intervals of one group.  Device times are
 * HIP events around the stages: plane_us, everything that makes the interval list (the id plane's clear and
 * fill, the runs, the sort and the table; with a connectedness, every stage of the internal
 * vsg_render_level_components call) and bringing a host F to the device; sums_us, k_color_runs; table_us,
 * the clear, k_color_table and k_color_finish; paint_us (vsg_render_mean_frame), k_color_intervals, the
 * plane's clear, k_render_fill and k_render_compose.  launches does not depend on H, on the number of
 * groups or on the number of intervals. */
typedef struct vsg_render_color_stats {
  int64_t groups, intervals, covered, largest_group_intervals;
  float plane_us, sums_us, table_us, paint_us;
  int launches;
} vsg_render_color_stats;                 /* 56 bytes with the tail padding */
int vsg_render_last_color_stats(vsg_render* h, vsg_render_color_stats* s);

/* ---- Level pooling: float feature planes pooled by group, group values painted back ----
 *
 * One group of the pooled table, as vsg_render_level_pool returns it. */
typedef struct vsg_render_pool_group {   /* 16 bytes, no padding */
  int32_t id;            /* region id at `level` */
  int32_t component;     /* index among its region's components; -1 with connectedness 0 */
  int32_t area;          /* pixels of the group */
  int32_t reserved;      /* written as 0 */
} vsg_render_pool_group;

#define VSG_POOL_F32 0    /* IEEE binary32 */
#define VSG_POOL_F16 1    /* IEEE binary16 */
#define VSG_POOL_BF16 2   /* bfloat16: the upper 16 bits of a binary32 */

/* A float feature map of C channels pooled by the groups of hierarchy level `level`, the float, C-channel
 * sibling of vsg_render_level_colors, and its inverse, which paints one value per group and channel back into
 * feature planes.  Computed on the device.
 *
 * The plane.  P is the plane of vsg_render_level_overlap, exactly as for vsg_render_level_colors: the id plane
 * of the level for connectedness 0, the component label image for VSG_RENDER_CONNECT_N4 / _N8 (that call is
 * made internally).  Pixels with P < 0 enter no group, and their feature values are never read.
 *
 * The features.  `dtype` is one of VSG_POOL_F32, VSG_POOL_F16, VSG_POOL_BF16; `features` has to be aligned to
 * its element size.  Strides are in elements: element (c, y, x) is at
 * features[c * chan_stride + y * row_stride + x * pixel_stride], in mem_in memory, independent of mem_out.  Two
 * layouts are accepted.  Planar: pixel_stride == 1, with any row and channel stride that keep rows and planes
 * disjoint (row_stride >= W; the planes behind one another or interleaved row by row).  Channels-last:
 * chan_stride == 1 and pixel_stride >= channels (row_stride >= (W - 1) * pixel_stride + channels).  A layout that
 * is both (one channel) is read as planar.  Anything else, and any negative stride, is VSG_ERR_INVALID.
 * 1 <= channels <= 65535.  A host map is copied to the device first, through a block of the handle that only
 * grows, with its strides and its address modulo 16 kept.
 *
 * The table.  One group per group of P, in the order of the sibling calls: groups[k] has the id, component and
 * area of record k of vsg_render_level_regions (connectedness 0) or vsg_render_level_components.  sum, sum_sq,
 * min and max are dense row-major [capacity_groups][channels] matrices in mem_out memory; each may be NULL,
 * which means not wanted, and a statistic that is not wanted is not computed.  groups may be NULL likewise.
 * Every element is first widened exactly to f64.  sum[k][c] is the f64 sum of the group's values of channel c,
 * sum_sq[k][c] the f64 sum of their squares (the square of an f32, f16 or bf16 value is exact in f64).  Both are
 * accumulated in f64 in an order that is a function of the interval list and the layout only (the strides and
 * the address modulo 16), never of the scheduling: there are no floating-point atomics anywhere, and the same
 * call returns the same bits; a host map and a device copy of it do when their addresses agree modulo 16 (a
 * sliced view copied to another offset may differ in the last bits of a sum).  min[k][c] and max[k][c] are the extreme non-NaN values as f32, +inf and -inf when
 * the group has none.  A NaN in a group's channel makes that channel's sum and sum_sq NaN and touches nothing
 * else.  Nothing else is derived on the device: mean and variance are left to the caller.
 *
 * Decode, hierarchy rules, level refusals, the non-negative ids and the handling of vector-only descs are those
 * of vsg_render_level_regions.  *num_groups is always set on VSG_OK and when the capacity is too small; in that
 * case the call fails with VSG_ERR_INVALID and nothing is written.  Every output NULL with capacity 0 asks for
 * the count only (VSG_OK; needs the device).  A null handle, a null count pointer, null features, a dtype other
 * than the three, channels outside [1, 65535], strides that are neither layout, a negative stride, a memory kind
 * other than the two, or a connectedness other than 0, VSG_RENDER_CONNECT_N4 and VSG_RENDER_CONNECT_N8 is
 * VSG_ERR_INVALID, answered before the handle is dereferenced, and touches no device.  Disjointness is the
 * exception: it is compared with the handle's size, so it is answered after the handle is read.  A frame with
 * no covered pixel returns zero groups.  The call neither resolves nor changes the level the handle keeps for
 * vsg_render_frame (vsg_render_level). */
int vsg_render_level_pool(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                          const void* features, int dtype, int channels,
                          ptrdiff_t chan_stride, ptrdiff_t row_stride, ptrdiff_t pixel_stride, int mem_in,
                          vsg_render_pool_group* groups, double* sum, double* sum_sq, float* min, float* max,
                          size_t capacity_groups, size_t* num_groups, int mem_out);

/* Unpool.  values is [num_values][channels] f32, dense, in mem_in memory; num_values has to equal the number of
 * groups of the level, otherwise the call fails with VSG_ERR_INVALID and out stays untouched.
 * out(c, y, x) = values[record(P(y, x))][c], converted to `dtype` with round-to-nearest-even; where P < 0 the
 * output is `fill`, converted likewise.  out accepts the same two layouts, in mem_out memory.  Only the W
 * elements of a row (planar) or the `channels` elements of a pixel (channels-last) are written: padding is
 * never touched.  A host output goes through a block of the handle: the span from its first to its last element
 * is copied to the device as it is, written into there and copied back whole, so what lies between the map's
 * elements is rewritten with its own bytes.  The
 * refusals are those of vsg_render_level_pool, with out for features and values for the count pointer. */
int vsg_render_level_unpool(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                            const float* values, size_t num_values, int channels, int mem_in, float fill,
                            void* out, int dtype, ptrdiff_t chan_stride, ptrdiff_t row_stride,
                            ptrdiff_t pixel_stride, int mem_out);

/* What the last vsg_render_level_pool or vsg_render_level_unpool call of the handle did.  groups, intervals,
 * covered, largest_group_intervals: as in vsg_render_color_stats.  feature_bytes: the bytes of features the
 * sums stage read, covered * channels * the element size (0 when no statistic was wanted).  Device times are
 * HIP events around the stages: plane_us, everything that makes the interval list and bringing a host input
 * to the device; sums_us, k_pool_sums_planar or k_pool_sums_last; table_us, k_pool_combine, the clear,
 * k_pool_count and k_pool_finish; paint_us (unpool), k_pool_intervals, the plane's clear, k_render_fill and
 * k_pool_gather_planar or k_pool_gather_last.  launches does not depend on H, on the number of groups, on the
 * number of intervals or on the number of channels. */
typedef struct vsg_render_pool_stats {
  int64_t groups, intervals, covered, largest_group_intervals, feature_bytes;
  float plane_us, sums_us, table_us, paint_us;
  int launches;
} vsg_render_pool_stats;                  /* 64 bytes with the tail padding */
int vsg_render_last_pool_stats(vsg_render* h, vsg_render_pool_stats* s);

/* ---- Volume session: a level's supervoxels accumulated over frames ----
 *
 * One row of the volume table, as vsg_render_volume_table returns it: a region id of the session's level, that
 * is a supervoxel, over every frame added so far. */
typedef struct vsg_render_volume_row {    /* 152 bytes, no padding */
  int32_t id, first_frame, last_frame, frames;   /* the smallest and the largest `frame` in which it painted a
                                                    pixel, and the number of adds in which it did */
  int32_t min_x, min_y, max_x, max_y;            /* bounding box over all frames, inclusive */
  int32_t first_pair, num_pairs, best_label, reserved0;   /* its slice of the pairs; the label with the largest
                                                    count, ties: the smallest label, -1 when num_pairs == 0;
                                                    reserved0 is written as 0 */
  int64_t volume, unlabelled, best_count;        /* voxels; of those, voxels where B is negative; the count of
                                                    best_label, 0 when num_pairs == 0 */
  int64_t sum_x, sum_y, sum_t;                   /* over its voxels, with t = `frame` */
  int64_t sum[3], sum_sq[3];                     /* B, G, R over its voxels, and the squares of the same bytes */
  uint8_t min[3], max[3], reserved1[2];          /* reserved1 is written as 0 */
} vsg_render_volume_row;

/* One column of the volume table: a label of the `other` planes. */
typedef struct vsg_render_volume_col {    /* 48 bytes, no padding */
  int32_t label, num_pairs, best_row, first_frame, last_frame, frames;   /* best_row: index in the row list of
                                                    the supervoxel with the largest count; ties: the smallest
                                                    index; -1 when num_pairs == 0 */
  int64_t volume, uncovered, best_count;         /* voxels with that label; of those, voxels where P is -1 */
} vsg_render_volume_col;

/* One non-empty cell of the volume table. */
typedef struct vsg_render_volume_pair {   /* 24 bytes, no padding */
  int32_t row, col, label, frames;        /* indices into the two lists; cols[col].label; the number of adds in
                                             which the two shared a pixel */
  int64_t count;                          /* voxels with P = the row's id and B = label; > 0 */
} vsg_render_volume_pair;

/* What the volume session of the handle holds and what its last calls did.  frames, rows, cols, pairs: of the
 * session.  new_rows, new_cols, new_pairs: keys the last add brought; resorts: the tables (0 to 3) it sorted
 * again because of them.  covered, labelled, both: voxels with P >= 0, with B >= 0 and with both, over the
 * session (labelled and both are 0 without with_labels).  Device times are HIP events: frame_us, the internal
 * per-frame stages of the last add (the stages of the internal vsg_render_level_overlap and
 * vsg_render_level_colors calls, or of the level's interval list alone); geometry_us, k_volume_geometry;
 * merge_us, the three merge kernels; sort_us, the radix sorts and gathers of the re-sorted tables (0 when the
 * add brought no key; the wait for the status words between the merge and the sorts is in no stage); table_us,
 * everything the last vsg_render_volume_table call ran.  launches: of the last add, the internal calls'
 * included; it does not depend on H, on the number of groups or on the frames added so far, only on which
 * tables had to be sorted again. */
typedef struct vsg_render_volume_stats {
  int64_t frames, rows, cols, pairs;
  int64_t new_rows, new_cols, new_pairs, resorts;
  int64_t covered, labelled, both;
  float frame_us, geometry_us, merge_us, sort_us, table_us;
  int launches;
} vsg_render_volume_stats;                /* 112 bytes */

/* A volume session is a device-resident table that every added frame is merged into and that can be read out at
 * any time: how long a supervoxel lives, its volume, its trajectory, its colour sums and its overlap with the
 * labels of a ground truth, without a per-frame table leaving the device.  Everything in it is an integer.
 *
 * The groups are the regions of one hierarchy level, keyed by region id.  Connected components are not offered
 * as groups: their indices mean nothing across frames.
 *
 * vsg_render_volume_begin starts, or restarts and empties, the session and fixes `level` (>= 0) and the two
 * flags (0 or 1) for all of it.  A null handle, a negative level or a flag other than 0 and 1 is
 * VSG_ERR_INVALID, answered before the handle is dereferenced; the call touches no device.
 *
 * vsg_render_volume_add adds one frame.  `frame` >= 0 is the caller's frame index, in any order; adding an
 * index twice counts it twice (unchecked).  Decode, hierarchy rules (the desc's own hierarchy replaces the kept
 * one, so a chunk's later frames use the hierarchy its first frame brought), level refusals, the non-negative
 * ids and the handling of vector-only descs are those of vsg_render_level_regions; the level is checked by the
 * add.  bgr, stride and mem_in are those of vsg_render_level_colors: required with with_colors, not looked at
 * without.  other, other_pitch and mem_other are those of vsg_render_level_overlap: required with with_labels,
 * not looked at without.  Without a session the call returns VSG_ERR_STATE.  A null handle or a negative frame
 * is VSG_ERR_INVALID, answered before the handle is dereferenced; a required plane that is null and an unknown
 * memory kind of a required plane are VSG_ERR_INVALID too, answered once the session's flags are read, and
 * touch no device; stride and pitch are compared with the handle's width.  A failed add leaves the session as
 * it was before the call: the per-frame stages run, and are checked, before anything is merged.  The one exception
 * is a failure of the device or of an allocation once the merge has begun (VSG_ERR_DEVICE, VSG_ERR_INTERNAL): it
 * ends the session, every later add or table call returns VSG_ERR_STATE until the next vsg_render_volume_begin.
 * The per-frame stages are internal calls: with with_labels vsg_render_level_overlap (connectedness 0), with
 * with_colors vsg_render_level_colors (connectedness 0); they overwrite vsg_render_last_overlap_stats and
 * vsg_render_last_color_stats, and every add overwrites vsg_render_last_stats.  Other calls on the handle
 * between two adds do not disturb the session.
 *
 * vsg_render_volume_table may be called at any time of a session and does not end it (VSG_ERR_STATE without
 * one).  Rows.  One row per region id that painted at least one pixel in any added frame, ascending by id.
 * Cols.  One column per distinct non-negative value of any added `other`, ascending by label.  Pairs.  One pair
 * per (id, label) with a common voxel, grouped by row in row order and within a row by ascending label.
 * first_pair of a row without a pair is the number of pairs of the rows before it.
 * Without with_labels: unlabelled = 0, best_label = -1, best_count = 0, first_pair = num_pairs = 0, and there
 * are no cols and no pairs.  Without with_colors: the colour fields are 0.
 * volume - unlabelled is the sum of the counts of the row's pairs, volume - uncovered the sum of the counts of
 * the column's pairs.  The table equals the field-wise sum (minimum and maximum for the extrema) over the added
 * frames of what vsg_render_level_regions, vsg_render_level_colors and vsg_render_level_overlap
 * (connectedness 0) return for each frame.
 * *num_rows, *num_cols and *num_pairs are always set on VSG_OK and when a capacity is too small; in that case
 * the call fails with VSG_ERR_INVALID and no output is touched.  All three outputs NULL with all three
 * capacities 0 asks for the counts only.  A null handle, a null count pointer or an unknown mem_out is
 * VSG_ERR_INVALID, answered before the handle is dereferenced.  All three lists in mem_out memory. */
int vsg_render_volume_begin(vsg_render* h, int level, int with_colors, int with_labels);
int vsg_render_volume_add(vsg_render* h, const uint8_t* seg, size_t seg_len, int frame,
                          const uint8_t* bgr, size_t stride, int mem_in,
                          const int32_t* other, size_t other_pitch, int mem_other);
int vsg_render_volume_table(vsg_render* h,
                            vsg_render_volume_row* rows, size_t capacity_rows, size_t* num_rows,
                            vsg_render_volume_col* cols, size_t capacity_cols, size_t* num_cols,
                            vsg_render_volume_pair* pairs, size_t capacity_pairs, size_t* num_pairs,
                            int mem_out);
int vsg_render_last_volume_stats(vsg_render* h, vsg_render_volume_stats* s);

/* ---- Level contours: the traced closed outlines of every group of a level ----
 *
 * One contour, as vsg_render_level_contours returns it. */
typedef struct vsg_render_level_contour {   /* 48 bytes, no padding */
  int32_t id;             /* region id of the group */
  int32_t component;      /* index among its region's components; -1 with connectedness 0 */
  int32_t group;          /* index k of the group in the sibling list */
  int32_t first_vertex;   /* offset of the contour's first vertex in `vertices`, in vertices */
  int32_t num_vertices;   /* even, at least 4 */
  int32_t length;         /* number of cracks, in pixel sides */
  int32_t min_x, min_y, max_x, max_y;   /* bounding box in corner coordinates */
  int64_t area2;          /* sum of x[i] * y[i + 1] - x[i + 1] * y[i]: twice the area, negative for a hole */
} vsg_render_level_contour;

/* The outlines of every region of hierarchy level `level`, or of every connected component of its regions,
 * as ordered closed polylines on the corner lattice.  Traced on the device; everything is an integer and
 * nothing depends on the order of execution.
 *
 * The plane.  P is the plane of vsg_render_level_boundaries: the id plane of vsg_render_id_image at `level`
 * for connectedness 0, or the label image of vsg_render_level_components for VSG_RENDER_CONNECT_N4 / _N8
 * (that call is made internally: vsg_render_last_component_stats then describes it).  Positions outside the
 * frame count as -1.  A group g >= 0 is a value of P; group index k is record k of the sibling call,
 * vsg_render_level_regions for connectedness 0 and vsg_render_level_components otherwise.
 *
 * Cracks.  Every pixel (x, y) of g has four sides: 0 top, 1 right, 2 bottom, 3 left.  A side is a crack of g
 * when the pixel across it is not g: outside the frame, uncovered, or of another group.  These are exactly
 * the sides the three border_* fields of vsg_render_level_adjacency count.  A crack is directed clockwise on
 * screen around its own pixel, on the corner lattice [0, W] x [0, H]: top from (x, y) to (x + 1, y), right
 * from (x + 1, y) to (x + 1, y + 1), bottom from (x + 1, y + 1) to (x, y + 1), left from (x, y + 1) to
 * (x, y), so that g is always on the right hand of the direction of travel.  key = 4 * (y * W + x) + side
 * identifies a crack.
 *
 * Successor.  At the corner where a crack ends the contour continues with the first crack of g, among those
 * that start at that corner, in the order right turn (the next side of the same pixel), straight on (the
 * same side of the next pixel of g), left turn (the side of the diagonal pixel of g); two reads of P decide
 * it.  At a saddle corner (two diagonal pixels of g, the other two not g) the contour therefore stays with
 * its own pixel, whatever the connectedness: positive contours bound N4-connected sets of g, holes bound
 * N8-connected sets of the complement, and an N8 component made of two diagonal pixels has two positive
 * contours.  The successor map is a permutation of the cracks; its cycles are the contours.
 *
 * Vertices.  A crack is a turn crack when its predecessor has another direction.  A contour's vertex list is
 * the start corners of its turn cracks in travel order, beginning with the turn crack of smallest key (the
 * crack of smallest key alone is not always a turn: under a hole two or more pixels wide it is not).
 * Collinear corners are never listed; every contour has an even number of at least 4 vertices; a corner can
 * occur twice in one list, at saddles.
 *
 * Order.  Contours are ordered by group, within a group by the key of their first turn crack: the first
 * contour of every group is positive and starts at the top-left corner of the group's first pixel in
 * row-major order.  vertices: int32 pairs {x, y}, grouped by contour in list order; capacity_vertices and
 * *num_vertices count pairs.
 *
 * Decode, hierarchy rules (the desc's own hierarchy replaces the kept one), level refusals, the
 * non-negative ids and the handling of vector-only descs are those of vsg_render_level_regions.
 * *num_contours and *num_vertices are always set on VSG_OK and when a capacity is too small; in that case
 * the call fails with VSG_ERR_INVALID and neither output is touched.  contours == NULL and vertices == NULL
 * with both capacities 0 asks for the counts only (VSG_OK; needs the device).  A null handle, a null count
 * pointer, a memory kind other than the two, or a connectedness other than 0, VSG_RENDER_CONNECT_N4 and
 * VSG_RENDER_CONNECT_N8 is VSG_ERR_INVALID, answered before the handle is dereferenced.  A frame with no
 * covered pixel returns zero contours and zero vertices.  The call neither resolves nor changes the level
 * the handle keeps for vsg_render_frame (vsg_render_level).  Counts are 32-bit like the siblings': a handle
 * whose crack keys would not fit (4 * W * H above 2^31) is refused with VSG_ERR_INVALID, and there are never
 * more cracks than keys.  Both lists in mem_out memory. */
int vsg_render_level_contours(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                              vsg_render_level_contour* contours, size_t capacity_contours,
                              size_t* num_contours, int32_t* vertices, size_t capacity_vertices,
                              size_t* num_vertices, int mem_out);

/* What the last vsg_render_level_contours call of the handle did.  cracks: the sides between a group and
 * anything else, each counted for its own group; vertices and contours: the lengths of the two lists; holes:
 * contours with area2 < 0; largest_contour_cracks: the longest `length`.  Device times are HIP events around
 * the stages: plane_us, making the plane (as in vsg_render_boundary_stats); classify_us, the count pass (the
 * crack masks and their scan) and the emit pass; trace_us, everything from the crack list to the ordered
 * vertices (both doublings, the contours' sort and scans, the vertex scatter); table_us, the records, their
 * lengths, boxes and areas, and the copies.  rounds: the pointer doubling rounds run, twice
 * ceil(log2 cracks) made even (a launch does two rounds).  launches is a function of the connectedness, of ceil(log2 cracks), of where the outputs
 * go and of how the plane is made (a vector-only desc adds its scan conversion), not of the plane's content.
 * The stages after the count pass are not run, and everything but cracks is 0, when there is no crack. */
typedef struct vsg_render_contour_stats {
  int64_t cracks, vertices, contours, holes, largest_contour_cracks;
  float plane_us, classify_us, trace_us, table_us;
  int rounds, launches;
} vsg_render_contour_stats;               /* 64 bytes */
int vsg_render_last_contour_stats(vsg_render* h, vsg_render_contour_stats* s);

/* ---- Level mesh: the contours of a level cut at the junctions into segments shared by two groups ----
 *
 * vsg_render_level_contours gives every group its own closed polygons, so the border between two groups is
 * stored twice.  The mesh stores it once: every contour is a list of references to segments, and a segment
 * between two groups is referenced by both, by one of them backwards.
 *
 * The plane P, groups, group index k, cracks, crack keys, direction of travel and the successor rule are those
 * of vsg_render_level_contours for the same (level, connectedness).  Positions outside the frame count as -1,
 * and so do uncovered pixels.
 *
 * Sides at a corner.  Lattice corner (cx, cy) is surrounded clockwise by the pixels (cx-1, cy-1), (cx, cy-1),
 * (cx, cy), (cx-1, cy).  sides(cx, cy) is the number of cyclically adjacent pairs among these four with
 * different values of P.  It is 0, 2, 3 or 4.  A corner with sides >= 3 is a junction.  Junctions include the
 * saddle a, b, a, b and a region border arriving at the frame edge (a, b, -1).  The four frame corners and a
 * -1/-1 contact are not junctions.
 *
 * Halves.  Every contour is a cycle of cracks.  It is cut at every crack whose start corner is a junction.
 * The pieces are the contour's halves.  A contour without a junction is one closed half that begins at its
 * leader, the turn crack of smallest key, as in the contours call.  All cracks of a half have the same value
 * across them.  This value is the half's other side, a group or -1.
 *
 * Segments.  A half is an owner when the group index of its other side is smaller than its own.  -1 counts
 * as smaller than every group.  Every half whose other side is a group has exactly one twin.  The twin is the
 * half of that group made of the opposite sides (pixel across, side + 2) in reverse order.  Exactly one of
 * the two is the owner.  A segment is an owner half.  Segments are listed in (right group index, key of the
 * half's first crack) order.
 *
 * The vertex list of an open segment, in the owner's direction of travel, holds the start corner of its first
 * crack, the start corners of its later turn cracks, and the end corner of its last crack.  Both end corners
 * are always listed, including where the curve runs straight through the junction.  Interior collinear
 * corners are never listed.  A closed segment lists exactly its contour's vertices and repeats none.  A half
 * that starts and ends at the same junction is open, not closed; an island that touches another island
 * diagonally is such a case.
 *
 * Loops and refs.  Loop c is contour c of the sibling contours call, with the same count and the same order.
 * Its refs are its halves in travel order.  The list begins with the half that contains the contour's leader
 * crack.  An owner half is written as its segment index s.  The other half is written as ~s: the same
 * segment travelled backwards. */
typedef struct vsg_render_mesh_segment {   /* 32 bytes, no padding */
  int32_t right, left;            /* group index on the right hand (the owner) and on the left hand; left = -1: none */
  int32_t first_vertex, num_vertices;   /* slice of `vertices`; open: >= 2, closed: even and >= 4 */
  int32_t length;                 /* cracks */
  int32_t closed;                 /* 1: a contour without a junction */
  int32_t start_sides, end_sides; /* sides() at the first and last corner: 3 or 4; both 0 when closed */
} vsg_render_mesh_segment;
typedef struct vsg_render_mesh_loop {      /* 16 bytes, no padding */
  int32_t group, first_ref, num_refs, length;   /* length = the contour's = the sum over its refs */
} vsg_render_mesh_loop;

/* vertices: int32 pairs {x, y}, grouped by segment in list order; capacity_vertices and *num_vertices count
 * pairs.  refs: int32, grouped by loop in list order.
 *
 * Decode, hierarchy rules (the desc's own hierarchy replaces the kept one), level refusals, the non-negative
 * ids and the handling of vector-only descs are those of vsg_render_level_regions.  *num_segments,
 * *num_vertices, *num_loops and *num_refs are always set on VSG_OK and when a capacity is too small; in that
 * case the call fails with VSG_ERR_INVALID and no output is touched.  All four outputs NULL with all four
 * capacities 0 asks for the counts only (VSG_OK; needs the device).  A null handle, a null count pointer, a
 * memory kind other than the two, or a connectedness other than 0, VSG_RENDER_CONNECT_N4 and
 * VSG_RENDER_CONNECT_N8 is VSG_ERR_INVALID, answered before the handle is dereferenced.  A frame with no
 * covered pixel returns four zero counts.  The call neither resolves nor changes the level the handle keeps
 * for vsg_render_frame (vsg_render_level).  Counts are 32-bit like the siblings': a handle whose crack keys
 * would not fit (4 * W * H above 2^31) is refused with VSG_ERR_INVALID.  All four lists in mem_out memory.
 *
 * The call runs the stages of vsg_render_level_contours internally, as a count-only call: afterwards
 * vsg_render_last_contour_stats (and, for N4 / N8, vsg_render_last_component_stats) describe that run. */
int vsg_render_level_mesh(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                          vsg_render_mesh_segment* segments, size_t capacity_segments, size_t* num_segments,
                          int32_t* vertices, size_t capacity_vertices, size_t* num_vertices,
                          vsg_render_mesh_loop* loops, size_t capacity_loops, size_t* num_loops,
                          int32_t* refs, size_t capacity_refs, size_t* num_refs, int mem_out);

/* What the last vsg_render_level_mesh call of the handle did.  cracks: as in vsg_render_contour_stats;
 * segments, vertices, loops, refs: the lengths of the four lists; closed_segments: segments with closed = 1;
 * shared_segments: segments with left >= 0; junctions: corners with sides >= 3; longest_segment_cracks: the
 * longest `length`.  Device times are HIP events around the stages: plane_us and classify_us, those of the
 * contour stages; trace_us, the contour stages' trace_us + table_us; split_us, the junction bits, the third
 * pointer doubling and the halves; table_us, the segments' sort, the vertices, the records, loops, refs,
 * lengths and the copies.  rounds: the rounds of all three doublings, three times ceil(log2 cracks) made even.
 * launches, those of the contour stages included, is a function of the connectedness, of ceil(log2 cracks),
 * of where the outputs go and of how the plane is made, not of the plane's content.  Everything but cracks
 * is 0 when there is no crack. */
typedef struct vsg_render_mesh_stats {
  int64_t cracks, segments, closed_segments, shared_segments, vertices, loops, refs, junctions,
      longest_segment_cracks;
  float plane_us, classify_us, trace_us, split_us, table_us;
  int rounds, launches;
} vsg_render_mesh_stats;                  /* 104 bytes with 4 bytes of tail padding */
int vsg_render_last_mesh_stats(vsg_render* h, vsg_render_mesh_stats* s);

/* ---- Simplified level mesh: the segments of the level mesh after Douglas-Peucker, on the device ----
 *
 * The reference's result files hold its borders after cv::approxPolyDP at max_error 1.0
 * (ComputeVectorization, segmentation/boundary.cpp).  vsg_render_level_mesh_simplified applies that step to
 * every segment of vsg_render_level_mesh.  A shared segment is simplified once, so the two groups it separates
 * still meet along the same polyline.
 *
 * Segments, their order, right, left, length (cracks), closed, start_sides, end_sides, loops and refs are
 * exactly those of vsg_render_level_mesh for the same (level, connectedness).  Only `vertices`, and each
 * record's first_vertex and num_vertices, change.
 *
 * The point list.  Q(s) holds every lattice corner segment s passes, in the owner's direction of travel.  An
 * open segment has length + 1 points, both end corners included.  A closed segment has length points.  It
 * begins at the first vertex the mesh call lists for it, and none is repeated.
 *
 * Collapse rule.  Let t = max(3, min_segment_points) if min_segment_points > 0, else 0.  An open segment with
 * length + 1 < t becomes {first corner, last corner}.  The reference's call uses 4.
 *
 * Otherwise the new list is ApproxPolyDP(Q, (double)max_error, closed = record.closed): OpenCV 2.4's
 * approxPolyDP for integer points as this project restates it (video_segment_amd/csrc/boundary.cpp,
 * tests/boundary_oracle.py).  It has three parts.  The three farthest-point sweeps choose the start of a
 * closed curve.  The recursion splits a slice at its farthest point (dist > max_dist: the first index wins a
 * tie) unless max_dist * max_dist <= eps * (dx * dx + dy * dy), with eps = max_error * max_error in double.
 * The final in-place pass drops points on almost straight joints, the wrap-around read of a closed list
 * included.  An open segment whose two end corners coincide goes in as closed = false, as the mesh records it;
 * the function's own start_pt == end_pt branch handles it.
 *
 * An open segment always keeps both end corners (num_vertices >= 2).  A closed segment may come back with 1
 * vertex or more.  Its vertex count need not be even.  It is generally a rotation of the list, because the
 * sweeps choose the start.  max_error = 0 with min_segment_points = 0 returns every open segment's corner list
 * unchanged, and every closed segment's list as a cyclic rotation.
 *
 * The stages work on the corner lists the mesh stages leave on the device, not on Q: along a straight run the
 * distance to a chord is linear and the distance to a sweep's start is strictly convex, so every maximum falls
 * on a corner.  Every double expression of the host function is evaluated operation for operation, without
 * contraction.
 *
 * max_error has to be finite and >= 0, min_segment_points >= 0.  Both are checked together with the null
 * handle, the null count pointers, mem_out and connectedness, before the handle is dereferenced; the refusal is
 * VSG_ERR_INVALID with the argument's name in the last-error text.  Capacities, count-only calls, "no output is
 * touched", level and vector-only rules and the 32-bit key limit are those of vsg_render_level_mesh:
 * *num_segments, *num_vertices, *num_loops and *num_refs are always set on VSG_OK and when a capacity is too
 * small; in that case the call fails with VSG_ERR_INVALID and no output is touched.  All four outputs NULL with
 * all four capacities 0 asks for the counts only (VSG_OK; needs the device).  A frame with no covered pixel
 * returns four zero counts.  The call neither resolves nor changes the level the handle keeps for
 * vsg_render_frame.  All four lists in mem_out memory.
 *
 * The call runs the contour and mesh stages internally, as a count-only mesh call: afterwards
 * vsg_render_last_contour_stats and vsg_render_last_mesh_stats describe that run. */
int vsg_render_level_mesh_simplified(vsg_render* h, const uint8_t* seg, size_t seg_len, int level,
                                     int connectedness, float max_error, int min_segment_points,
                                     vsg_render_mesh_segment* segments, size_t capacity_segments,
                                     size_t* num_segments, int32_t* vertices, size_t capacity_vertices,
                                     size_t* num_vertices, vsg_render_mesh_loop* loops, size_t capacity_loops,
                                     size_t* num_loops, int32_t* refs, size_t capacity_refs, size_t* num_refs,
                                     int mem_out);

/* What the last vsg_render_level_mesh_simplified call of the handle did.  segments: the mesh's;
 * collapsed_segments: open segments the collapse rule replaced by their end corners; vertices_in: the mesh's
 * vertices; vertices_kept: vertices after the recursion (2 for a collapsed segment); vertices_out: after the
 * joint pass, the length of `vertices`; single_vertex_closed: closed segments that came back as one vertex;
 * longest_segment_vertices_in: the most vertices a segment of the mesh has; max_rounds: the most refinement
 * rounds any segment took, a round being one level of the recursion in which a vertex was kept.  Device times
 * are HIP events around the stages: dp_us, the collapse rule, the sweeps and the rounds; clean_us, the joint
 * pass; table_us, the scan, the compaction, the records and the copies.  launches, those of the contour and
 * mesh stages included, is a function of the connectedness, of ceil(log2 cracks), of where the outputs go and
 * of how the plane is made, not of the plane's content, max_error or min_segment_points: no launch happens
 * per round.  Everything is 0 when there is no crack, but launches. */
typedef struct vsg_render_simplify_stats {
  int64_t segments, collapsed_segments, vertices_in, vertices_kept, vertices_out, single_vertex_closed,
      longest_segment_vertices_in;
  float dp_us, clean_us, table_us;
  int max_rounds, launches;
} vsg_render_simplify_stats;              /* 80 bytes with 4 bytes of tail padding */
int vsg_render_last_simplify_stats(vsg_render* h, vsg_render_simplify_stats* s);

/* ---- Boundary distance: the exact distance transform of a level's edges, boundary scores of all levels ----
 *
 * Boundary precision and recall over all levels are functions of the persistence plane only at tolerance zero;
 * every published benchmark matches boundaries within a distance.  These calls give the distance, and the
 * matched counts of every hierarchy level at a tolerance, in integers.
 *
 * Edge set of a plane.  E(P) = { (x, y) : P(x, y) != P(x+1, y) with x+1 < W, or P(x, y) != P(x, y+1) with
 * y+1 < H }, -1 counting as a value: the reference's edge rule, the pixels highlight_edges blackens.
 * The squared distance.  D(x, y) = min over (u, v) in E of (x - u)^2 + (y - v)^2, an int32; it is 0 exactly on
 * E.  D is VSG_RENDER_DISTANCE_NONE everywhere when E is empty.  A handle is at most 32768 x 32768, so every
 * finite D is at most 2 * 32767^2 = 2147352578, below VSG_RENDER_DISTANCE_NONE.  There are no floats in it
 * and no approximation: D is the exact Euclidean distance transform, squared.
 *
 * vsg_render_boundary_distance.  P is the plane of vsg_render_id_image(level): the same decode, hierarchy
 * bookkeeping, level rules, refusals and vector-only handling.  E = E(P), which is exactly Q > level of the
 * persistence plane.  D is written as W * H int32 with rows W apart to out_int32 in mem_out memory.  A null
 * handle, a null output or an unknown memory kind is VSG_ERR_INVALID, answered before the handle is
 * dereferenced.  On every refusal the output is untouched.
 *
 * vsg_render_boundary_benchmark.  `other` is a label plane B with the rules of vsg_render_level_overlap: H
 * rows of W int32 in mem_other memory, other_pitch values apart (0 means W), every int32 legal.
 * B' = max(B, -1): all negative values are one "void" value.  G = E(B').  L, the hierarchy and Q are those of
 * the persistence calls, the L > 65535 refusal and the ancestor table's refusals included.  With
 * T = tolerance_sq the call returns one record per l in [0, L):
 *   seg_edges[l]   = #{ p : Q(p) > l }                        the edge pixels of level l
 *   seg_matched[l] = #{ p : Q(p) > l and D_G(p) <= T }        of those, the ones within sqrt(T) of G
 *   gt_edges[l]    = |G|                                      the same at every level
 *   gt_matched[l]  = #{ p in G : D_l(p) <= T }                D_l the distance to { Q > l }
 * so that precision = seg_matched / seg_edges and recall = gt_matched / gt_edges.  Two identities make the
 * work independent of L: seg_matched[l] counts Q > l over the pixels with D_G <= T, one distance transform and
 * one histogram of Q; and D_l(p) <= T holds exactly when M(p) > l with M(p) = max{ Q(q) : |p - q|^2 <= T },
 * the disc maximum of Q, taken at the pixels of G only.  The number of launches of a call does not depend on L.
 * tolerance_sq outside [0, VSG_RENDER_MAX_TOLERANCE_SQ] is VSG_ERR_INVALID, answered without a device.
 * *num_levels is always set on VSG_OK and when capacity_levels is too small; in that case the call fails with
 * VSG_ERR_INVALID and touches no output.  scores == NULL with capacity_levels 0 asks for the count only
 * (VSG_OK; needs the device).  A null handle, a null count pointer, a null `other`, an unknown memory kind or
 * a pitch below W is VSG_ERR_INVALID, answered before the handle is used for device work.  The call paints
 * the persistence plane internally: vsg_render_last_persistence_stats then describes that.
 *
 * When an edge set is empty the call stops after counting it: D is filled with VSG_RENDER_DISTANCE_NONE, or
 * both matched counts are 0.  Vector-only descs are scan converted at the handle's size first.  Every call
 * returns after its stream work has finished. */
#define VSG_RENDER_DISTANCE_NONE 0x7fffffff
#define VSG_RENDER_MAX_TOLERANCE_SQ 4096
int vsg_render_boundary_distance(vsg_render* h, const uint8_t* seg, size_t seg_len, int level,
                                 int32_t* out_int32, int mem_out);

typedef struct vsg_render_boundary_score {   /* 32 bytes, no padding */
  int64_t seg_edges;     /* pixels with Q > l                                                          */
  int64_t seg_matched;   /* of those, pixels whose squared distance to the nearest pixel of G is
                          * <= tolerance_sq                                                            */
  int64_t gt_edges;      /* |G|; the same at every level                                               */
  int64_t gt_matched;    /* pixels of G whose squared distance to the nearest pixel with Q > l is
                          * <= tolerance_sq                                                            */
} vsg_render_boundary_score;
int vsg_render_boundary_benchmark(vsg_render* h, const uint8_t* seg, size_t seg_len,
                                  const int32_t* other, size_t other_pitch, int mem_other, int tolerance_sq,
                                  vsg_render_boundary_score* scores, size_t capacity_levels, size_t* num_levels,
                                  int mem_out);

/* What the last boundary distance or boundary benchmark call of the handle did.  levels: L for the benchmark
 * call, 0 for the distance call.  edge_pixels: |E| for the distance call, #{Q > 0} for the benchmark call.
 * other_edge_pixels: |G|, or 0.  max_distance: the largest finite D the distance call wrote, or 0.  Device
 * times are HIP events around the stages, and a stage that did not run reports 0: plane_us, making the plane
 * (clear and fill; with the persistence plane and the upload of a host B for the benchmark call);
 * classify_us, k_dist_classify; columns_us, k_dist_columns; rows_us, k_dist_rows; match_us, k_dist_match,
 * k_dist_disc and k_dist_scores.  launches is a function of where the buffers are, of how the plane is made
 * and of whether the classified edge set is empty, not of L. */
typedef struct vsg_render_distance_stats {
  int64_t levels, edge_pixels, other_edge_pixels, max_distance;
  float plane_us, classify_us, columns_us, rows_us, match_us;
  int launches;
} vsg_render_distance_stats;                /* 56 bytes */
int vsg_render_last_distance_stats(vsg_render* h, vsg_render_distance_stats* s);

/* ---- Tree cut: the best non-horizontal cut of the hierarchy ----
 *
 * Every other call looks at the hierarchy one horizontal level at a time.  This one chooses, region by
 * region, the level at which to stop: a coarse node where a gain says so, fine nodes elsewhere.
 *
 * Hierarchy, height L, ancestors A_l(r).  Exactly those of the persistence calls: the desc's own hierarchy
 * replaces the kept one; L = max(1, levels); L > 65535 is VSG_ERR_INVALID; the lookups and refusals are those
 * of vsg_render_id_image at level L - 1; a negative region id is refused; only regions that paint are looked
 * up.
 * Nodes.  A node is a pair (l, id) with id = A_l(r) for a region r of the level-0 id image.  Its pixels are
 * those whose level-0 region r has A_l(r) = id, its leaves those regions, its children the distinct nodes
 * (l - 1, A_{l-1}(r)) of its leaves; a node of level 0 has none.  A node with one child has that child's
 * pixels.
 * Gain g(n), int64.  Exactly one of two sources is given; both, or neither, is VSG_ERR_INVALID.
 *   Labels (labels != NULL).  B is a label plane as in vsg_render_level_overlap: any int32, negative means no
 *   label, host or device memory, labels_pitch 0 means W.  best(n) is the largest number of pixels n shares
 *   with one label >= 0, ties go to the smallest label; without a labelled pixel best_label is -1 and
 *   best_count 0.  g(n) = best(n) - penalty, 0 <= penalty <= 2^32; any other penalty is refused before the
 *   handle is dereferenced, with either source.
 *   Gain table (gains != NULL; num_gains may be 0).  vsg_render_cut_gain entries in host or device memory,
 *   strictly ascending by (level, id), |gain| <= 2^32.  A table out of order, a duplicate or a gain out of
 *   range is VSG_ERR_INVALID; the check runs on the device, and no output is touched.  Entries that name no
 *   node of this frame are ignored; nodes not listed have gain 0.  best_label is -1 and best_count 0 in every
 *   record.
 * The cut.  Bottom-up: opt(n) = g(n) at level 0.  Above, S(n) is the sum of opt(c) over the children,
 * keep(n) <=> g(n) >= S(n) -- a tie keeps the coarser node -- and opt(n) = max(g(n), S(n)).  Leaves always
 * keep.  The selected node of a region r is (l*, A_{l*}(r)) with l* = max { l : keep(A_l(r)) }: the first kept
 * node met when descending from the top.  The selected nodes partition the covered pixels, and the cut
 * maximises the sum of g over all partitions into nodes.  total is that sum; it equals the sum of opt over the
 * top-level nodes.  Everything fits in int64.
 * Consequences.  With labels and penalty 0 the sum of best_count over the cut equals that of the level-0 rows
 * of vsg_render_level_overlap, and the cut is the coarsest partition that reaches it.  With a penalty above
 * every best(n) the cut is the top level.  As the penalty grows the number of nodes never increases and no
 * region's l* decreases: the cuts are nested.
 *
 * nodes: one record per selected node, ascending by (level, id).  area: its pixels; leaves, children: as
 * defined above; split_value = S(n), 0 where children == 0; reserved is 0.  plane (optional): W * H int32,
 * rows W apart; each pixel holds the index of the record that covers it, -1 where the level-0 id image is
 * -1; NULL means not wanted and not painted.  nodes and plane are in mem_out memory.
 * *num_nodes and *total are set on VSG_OK and when the capacity is too small; in that case the call fails
 * with VSG_ERR_INVALID and nothing is touched.  nodes == NULL and plane == NULL with capacity 0 asks for the
 * count and the total only.  Vector-only descs are scan converted first.  The call returns after its stream
 * work has finished.
 * Size.  With R the regions of the level-0 image and P its (region, label) pairs (0 with a gain table),
 * L * R + L * P > 2^27 is VSG_ERR_INVALID; the message names L, R and P.  The refusal comes once the counts
 * are known, with nothing written.
 * With labels the level-0 table is made by vsg_render_level_overlap's pipeline (vsg_render_last_overlap_stats
 * then describes it), with a gain table by vsg_render_level_regions' (vsg_render_last_level_stats).
 * A null handle, a null count or total pointer, an unknown memory kind, a pitch below W, both or neither
 * source, or a penalty out of range is VSG_ERR_INVALID. */
typedef struct vsg_render_cut_gain {   /* 16 bytes, no padding */
  int32_t level, id;
  int64_t gain;
} vsg_render_cut_gain;

typedef struct vsg_render_cut_node {   /* 48 bytes, no padding */
  int32_t level, id, area, leaves, children, best_label, best_count, reserved;
  int64_t gain, split_value;
} vsg_render_cut_node;

int vsg_render_tree_cut(vsg_render* h, const uint8_t* seg, size_t seg_len,
                        const int32_t* labels, size_t labels_pitch, int mem_labels, int64_t penalty,
                        const vsg_render_cut_gain* gains, size_t num_gains, int mem_gains,
                        vsg_render_cut_node* nodes, size_t capacity_nodes, size_t* num_nodes,
                        int32_t* plane, int64_t* total, int mem_out);

/* Two DP paths.  With tree_nodes <= block_nodes one workgroup walks all levels in one launch; above it the
 * levels are launched one by one.  0: always per level.  INT64_MAX: always one workgroup.  -1: the default
 * (32768).  Any other negative value is VSG_ERR_INVALID.  The bytes of both paths are the same. */
int vsg_render_tree_cut_tuning(vsg_render* h, int64_t block_nodes);

/* What the last vsg_render_tree_cut of the handle did.  levels: L.  leaves: R.  tree_nodes: nodes of all
 * levels.  pairs: P.  entries: the keys the two sorts saw, L * R + L * P.  cut_nodes, covered (pixels of the
 * selected nodes), total.  block_nodes: the threshold in force.  Device times are HIP events around the
 * stages: plane_us, the level-0 plane; table_us, the level-0 table of the sibling call; lift_us, the node
 * keys, their sort, the node table and the gains; dp_us, the dynamic programme; paint_us, k_cut_select, the
 * scan, k_cut_records and k_cut_paint.  dp_path: 0 not run (no node), 1 one workgroup, 2 per level.
 * dp_launches: 1 on the one-workgroup path, L on the per-level path.  launches: everything the call enqueued;
 * on the one-workgroup path it does not depend on L, on the per-level path it is that number + L - 1. */
typedef struct vsg_render_cut_stats {
  int64_t levels, leaves, tree_nodes, pairs, entries, cut_nodes, covered, total, block_nodes;
  float plane_us, table_us, lift_us, dp_us, paint_us;
  int dp_path, dp_launches, launches;
} vsg_render_cut_stats;
int vsg_render_last_cut_stats(vsg_render* h, vsg_render_cut_stats* s);

/* srand(region_id); c[k] = rand() % 255 (segmentation_render.cpp:66-69) with glibc's generator
 * restated, so that process-global state stays untouched.  Host only; needs no device. */
void vsg_render_color(int region_id, uint8_t c[3]);

#ifdef __cplusplus
}
#endif

#endif /* VSG_RENDER_H_ */
