"""Python host layer of the segmentation renderer (C ABI: include/vsg_render.h, libvsg_render.so).

``SegmentationRenderer`` mirrors the reference's SegmentationRenderUnit (segmentation_unit.cpp:478-655)
without its stream plumbing: serialized ``SegmentationDesc`` bytes and, optionally, the BGR24 source
frame go in, the rendered frame (or the id image of a hierarchy level) comes out.  Frames and outputs
may be numpy arrays (host memory) or torch CUDA tensors (device memory); the output lives where the
frame does, or where ``out=`` says.  All per-pixel work happens in the HIP library; there is no
Python or CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _capi, _lib
from ._lib import VSG_MEM_DEVICE, VSG_MEM_HOST, VSG_OK, VsgError  # noqa: F401 (part of the module)

LIB_PATH = _capi.lib_path("vsg_render")


class VsgRenderOptions(_capi.Structure):
    _fields_ = [
        ("blend_alpha", C.c_float),
        ("hierarchy_level", C.c_float),
        ("highlight_edges", C.c_int),
        ("concat_with_source", C.c_int),
        ("has_video", C.c_int),
        ("device", C.c_int),
    ]


class VsgRenderStats(_capi.Structure):
    _fields_ = [
        ("decode_ms", C.c_double), ("upload_ms", C.c_double),
        ("clear_us", C.c_float), ("fill_us", C.c_float), ("compose_us", C.c_float),
        ("launches", C.c_int),
        ("intervals", C.c_int64), ("distinct_ids", C.c_int64), ("device_allocations", C.c_int64),
    ]


class VsgRenderVectorStats(_capi.Structure):
    _fields_ = [
        ("lines", C.c_int64), ("crossings", C.c_int64), ("groups", C.c_int64), ("largest_group", C.c_int64),
        ("walk_us", C.c_float), ("sort_us", C.c_float), ("pairs_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderLevelStats(_capi.Structure):
    _fields_ = [
        ("runs", C.c_int64), ("regions", C.c_int64), ("largest_region_intervals", C.c_int64),
        ("runs_us", C.c_float), ("sort_us", C.c_float), ("table_us", C.c_float), ("moments_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderComponentStats(_capi.Structure):
    _fields_ = [
        ("runs", C.c_int64), ("regions", C.c_int64), ("components", C.c_int64), ("links", C.c_int64),
        ("largest_component_intervals", C.c_int64),
        ("runs_us", C.c_float), ("sort_us", C.c_float), ("link_us", C.c_float), ("order_us", C.c_float),
        ("moments_us", C.c_float), ("label_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderBoundaryStats(_capi.Structure):
    _fields_ = [
        ("points", C.c_int64), ("boundaries", C.c_int64), ("largest_boundary_points", C.c_int64),
        ("plane_us", C.c_float), ("count_us", C.c_float), ("emit_us", C.c_float), ("sort_us", C.c_float),
        ("table_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderAdjacencyStats(_capi.Structure):
    _fields_ = [
        ("sides", C.c_int64), ("keys", C.c_int64), ("nodes", C.c_int64), ("edges", C.c_int64),
        ("largest_node_edges", C.c_int64),
        ("plane_us", C.c_float), ("count_us", C.c_float), ("emit_us", C.c_float), ("sort_us", C.c_float),
        ("table_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderOverlapStats(_capi.Structure):
    _fields_ = [
        ("covered", C.c_int64), ("labelled", C.c_int64), ("both", C.c_int64), ("runs", C.c_int64),
        ("rows", C.c_int64), ("cols", C.c_int64), ("pairs", C.c_int64), ("largest_row_pairs", C.c_int64),
        ("plane_us", C.c_float), ("count_us", C.c_float), ("emit_us", C.c_float), ("sort_us", C.c_float),
        ("table_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderPersistenceStats(_capi.Structure):
    _fields_ = [
        ("levels", C.c_int64), ("regions", C.c_int64), ("edge_pixels", C.c_int64), ("top_pixels", C.c_int64),
        ("nodes", C.c_int64), ("edges", C.c_int64),
        ("plane_us", C.c_float), ("persist_us", C.c_float), ("compose_us", C.c_float), ("graph_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderCutStats(_capi.Structure):
    _fields_ = [
        ("levels", C.c_int64), ("leaves", C.c_int64), ("tree_nodes", C.c_int64), ("pairs", C.c_int64),
        ("entries", C.c_int64), ("cut_nodes", C.c_int64), ("covered", C.c_int64), ("total", C.c_int64),
        ("block_nodes", C.c_int64),
        ("plane_us", C.c_float), ("table_us", C.c_float), ("lift_us", C.c_float), ("dp_us", C.c_float),
        ("paint_us", C.c_float),
        ("dp_path", C.c_int), ("dp_launches", C.c_int), ("launches", C.c_int),
    ]


class VsgRenderColorStats(_capi.Structure):
    _fields_ = [
        ("groups", C.c_int64), ("intervals", C.c_int64), ("covered", C.c_int64),
        ("largest_group_intervals", C.c_int64),
        ("plane_us", C.c_float), ("sums_us", C.c_float), ("table_us", C.c_float), ("paint_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderPoolStats(_capi.Structure):
    _fields_ = [
        ("groups", C.c_int64), ("intervals", C.c_int64), ("covered", C.c_int64),
        ("largest_group_intervals", C.c_int64), ("feature_bytes", C.c_int64),
        ("plane_us", C.c_float), ("sums_us", C.c_float), ("table_us", C.c_float), ("paint_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderVolumeStats(_capi.Structure):
    _fields_ = [
        ("frames", C.c_int64), ("rows", C.c_int64), ("cols", C.c_int64), ("pairs", C.c_int64),
        ("new_rows", C.c_int64), ("new_cols", C.c_int64), ("new_pairs", C.c_int64), ("resorts", C.c_int64),
        ("covered", C.c_int64), ("labelled", C.c_int64), ("both", C.c_int64),
        ("frame_us", C.c_float), ("geometry_us", C.c_float), ("merge_us", C.c_float), ("sort_us", C.c_float),
        ("table_us", C.c_float),
        ("launches", C.c_int),
    ]


class VsgRenderContourStats(_capi.Structure):
    _fields_ = [
        ("cracks", C.c_int64), ("vertices", C.c_int64), ("contours", C.c_int64), ("holes", C.c_int64),
        ("largest_contour_cracks", C.c_int64),
        ("plane_us", C.c_float), ("classify_us", C.c_float), ("trace_us", C.c_float), ("table_us", C.c_float),
        ("rounds", C.c_int), ("launches", C.c_int),
    ]


class VsgRenderMeshStats(_capi.Structure):
    _fields_ = [
        ("cracks", C.c_int64), ("segments", C.c_int64), ("closed_segments", C.c_int64),
        ("shared_segments", C.c_int64), ("vertices", C.c_int64), ("loops", C.c_int64), ("refs", C.c_int64),
        ("junctions", C.c_int64), ("longest_segment_cracks", C.c_int64),
        ("plane_us", C.c_float), ("classify_us", C.c_float), ("trace_us", C.c_float), ("split_us", C.c_float),
        ("table_us", C.c_float),
        ("rounds", C.c_int), ("launches", C.c_int),
    ]


class VsgRenderSimplifyStats(_capi.Structure):
    _fields_ = [
        ("segments", C.c_int64), ("collapsed_segments", C.c_int64), ("vertices_in", C.c_int64),
        ("vertices_kept", C.c_int64), ("vertices_out", C.c_int64), ("single_vertex_closed", C.c_int64),
        ("longest_segment_vertices_in", C.c_int64),
        ("dp_us", C.c_float), ("clean_us", C.c_float), ("table_us", C.c_float),
        ("max_rounds", C.c_int), ("launches", C.c_int),
    ]


class VsgRenderDistanceStats(_capi.Structure):
    _fields_ = [
        ("levels", C.c_int64), ("edge_pixels", C.c_int64), ("other_edge_pixels", C.c_int64),
        ("max_distance", C.c_int64),
        ("plane_us", C.c_float), ("classify_us", C.c_float), ("columns_us", C.c_float), ("rows_us", C.c_float),
        ("match_us", C.c_float),
        ("launches", C.c_int),
    ]


# vsg_render_level_region: 56 bytes, no padding
LEVEL_REGION_DTYPE = np.dtype([
    ("id", np.int32), ("first_interval", np.int32), ("num_intervals", np.int32), ("area", np.int32),
    ("min_x", np.int32), ("min_y", np.int32), ("max_x", np.int32), ("max_y", np.int32),
    ("size", np.float32), ("mean_x", np.float32), ("mean_y", np.float32),
    ("moment_xx", np.float32), ("moment_xy", np.float32), ("moment_yy", np.float32),
])
assert LEVEL_REGION_DTYPE.itemsize == 56
LEVEL_REGION_WORDS = 14

# vsg_render_level_component: 64 bytes, no padding
LEVEL_COMPONENT_DTYPE = np.dtype([
    ("id", np.int32), ("component", np.int32), ("region_components", np.int32),
    ("first_interval", np.int32), ("num_intervals", np.int32), ("area", np.int32),
    ("min_x", np.int32), ("min_y", np.int32), ("max_x", np.int32), ("max_y", np.int32),
    ("size", np.float32), ("mean_x", np.float32), ("mean_y", np.float32),
    ("moment_xx", np.float32), ("moment_xy", np.float32), ("moment_yy", np.float32),
])
assert LEVEL_COMPONENT_DTYPE.itemsize == 64
LEVEL_COMPONENT_WORDS = 16

# vsg_render_level_boundary: 16 bytes, no padding
LEVEL_BOUNDARY_DTYPE = np.dtype([
    ("id", np.int32), ("component", np.int32), ("first_point", np.int32), ("num_points", np.int32),
])
assert LEVEL_BOUNDARY_DTYPE.itemsize == 16
LEVEL_BOUNDARY_WORDS = 4

# VSG_RENDER_BOUNDARY_INNER / _OUTER
BOUNDARY_INNER = 0
BOUNDARY_OUTER = 1

# vsg_render_level_node: 28 bytes, no padding
LEVEL_NODE_DTYPE = np.dtype([
    ("id", np.int32), ("component", np.int32), ("first_edge", np.int32), ("num_edges", np.int32),
    ("border_frame", np.int32), ("border_uncovered", np.int32), ("border_shared", np.int32),
])
assert LEVEL_NODE_DTYPE.itemsize == 28
LEVEL_NODE_WORDS = 7

# vsg_render_level_edge: 16 bytes, no padding
LEVEL_EDGE_DTYPE = np.dtype([
    ("neighbour", np.int32), ("neighbour_id", np.int32), ("shared_n4", np.int32), ("shared_diagonal", np.int32),
])
assert LEVEL_EDGE_DTYPE.itemsize == 16
LEVEL_EDGE_WORDS = 4

# VSG_RENDER_ADJACENT_N4 / _N8
ADJACENT_N4 = 1
ADJACENT_N8 = 2

# vsg_render_overlap_row: 32 bytes, no padding
OVERLAP_ROW_DTYPE = np.dtype([
    ("id", np.int32), ("component", np.int32), ("first_pair", np.int32), ("num_pairs", np.int32),
    ("area", np.int32), ("unlabelled", np.int32), ("best_label", np.int32), ("best_count", np.int32),
])
assert OVERLAP_ROW_DTYPE.itemsize == 32
OVERLAP_ROW_WORDS = 8

# vsg_render_overlap_col: 24 bytes, no padding
OVERLAP_COL_DTYPE = np.dtype([
    ("label", np.int32), ("area", np.int32), ("uncovered", np.int32), ("num_pairs", np.int32),
    ("best_row", np.int32), ("best_count", np.int32),
])
assert OVERLAP_COL_DTYPE.itemsize == 24
OVERLAP_COL_WORDS = 6

# vsg_render_overlap_pair: 16 bytes, no padding
OVERLAP_PAIR_DTYPE = np.dtype([("row", np.int32), ("col", np.int32), ("label", np.int32), ("count", np.int32)])
assert OVERLAP_PAIR_DTYPE.itemsize == 16
OVERLAP_PAIR_WORDS = 4

# vsg_render_level_color: 72 bytes, no padding
LEVEL_COLOR_DTYPE = np.dtype([
    ("id", np.int32), ("component", np.int32), ("area", np.int32),
    ("mean", np.uint8, (3,)), ("reserved0", np.uint8),
    ("sum", np.int64, (3,)), ("sum_sq", np.int64, (3,)),
    ("min", np.uint8, (3,)), ("max", np.uint8, (3,)), ("reserved1", np.uint8, (2,)),
])
assert LEVEL_COLOR_DTYPE.itemsize == 72
LEVEL_COLOR_WORDS = 18

# vsg_render_pool_group: 16 bytes, no padding
POOL_GROUP_DTYPE = np.dtype([("id", np.int32), ("component", np.int32), ("area", np.int32), ("reserved", np.int32)])
assert POOL_GROUP_DTYPE.itemsize == 16
POOL_GROUP_WORDS = 4

# VSG_POOL_F32 / _F16 / _BF16, and the statistics of level_pool in the order of the C arguments
POOL_F32, POOL_F16, POOL_BF16 = 0, 1, 2
POOL_STATS = ("sum", "sum_sq", "min", "max")
_POOL_DTYPES = {"float32": POOL_F32, "float16": POOL_F16, "bfloat16": POOL_BF16, "bf16": POOL_BF16}

# vsg_render_volume_row: 152 bytes, no padding
VOLUME_ROW_DTYPE = np.dtype([
    ("id", np.int32), ("first_frame", np.int32), ("last_frame", np.int32), ("frames", np.int32),
    ("min_x", np.int32), ("min_y", np.int32), ("max_x", np.int32), ("max_y", np.int32),
    ("first_pair", np.int32), ("num_pairs", np.int32), ("best_label", np.int32), ("reserved0", np.int32),
    ("volume", np.int64), ("unlabelled", np.int64), ("best_count", np.int64),
    ("sum_x", np.int64), ("sum_y", np.int64), ("sum_t", np.int64),
    ("sum", np.int64, (3,)), ("sum_sq", np.int64, (3,)),
    ("min", np.uint8, (3,)), ("max", np.uint8, (3,)), ("reserved1", np.uint8, (2,)),
])
assert VOLUME_ROW_DTYPE.itemsize == 152
VOLUME_ROW_WORDS = 38

# vsg_render_volume_col: 48 bytes, no padding
VOLUME_COL_DTYPE = np.dtype([
    ("label", np.int32), ("num_pairs", np.int32), ("best_row", np.int32),
    ("first_frame", np.int32), ("last_frame", np.int32), ("frames", np.int32),
    ("volume", np.int64), ("uncovered", np.int64), ("best_count", np.int64),
])
assert VOLUME_COL_DTYPE.itemsize == 48
VOLUME_COL_WORDS = 12

# vsg_render_volume_pair: 24 bytes, no padding
VOLUME_PAIR_DTYPE = np.dtype([
    ("row", np.int32), ("col", np.int32), ("label", np.int32), ("frames", np.int32), ("count", np.int64),
])
assert VOLUME_PAIR_DTYPE.itemsize == 24
VOLUME_PAIR_WORDS = 6

# vsg_render_level_contour: 48 bytes, no padding
LEVEL_CONTOUR_DTYPE = np.dtype([
    ("id", np.int32), ("component", np.int32), ("group", np.int32),
    ("first_vertex", np.int32), ("num_vertices", np.int32), ("length", np.int32),
    ("min_x", np.int32), ("min_y", np.int32), ("max_x", np.int32), ("max_y", np.int32),
    ("area2", np.int64),
])
assert LEVEL_CONTOUR_DTYPE.itemsize == 48
LEVEL_CONTOUR_WORDS = 12

# vsg_render_mesh_segment: 32 bytes, no padding
MESH_SEGMENT_DTYPE = np.dtype([
    ("right", np.int32), ("left", np.int32), ("first_vertex", np.int32), ("num_vertices", np.int32),
    ("length", np.int32), ("closed", np.int32), ("start_sides", np.int32), ("end_sides", np.int32),
])
assert MESH_SEGMENT_DTYPE.itemsize == 32
MESH_SEGMENT_WORDS = 8

# vsg_render_mesh_loop: 16 bytes, no padding
MESH_LOOP_DTYPE = np.dtype([
    ("group", np.int32), ("first_ref", np.int32), ("num_refs", np.int32), ("length", np.int32),
])
assert MESH_LOOP_DTYPE.itemsize == 16
MESH_LOOP_WORDS = 4

# vsg_render_boundary_score: 32 bytes, no padding
BOUNDARY_SCORE_DTYPE = np.dtype([
    ("seg_edges", np.int64), ("seg_matched", np.int64), ("gt_edges", np.int64), ("gt_matched", np.int64),
])
assert BOUNDARY_SCORE_DTYPE.itemsize == 32
BOUNDARY_SCORE_WORDS = 4

# vsg_render_cut_node (48 bytes) and vsg_render_cut_gain (16 bytes); as int32 words in torch tensors
CUT_NODE_DTYPE = np.dtype([
    ("level", np.int32), ("id", np.int32), ("area", np.int32), ("leaves", np.int32), ("children", np.int32),
    ("best_label", np.int32), ("best_count", np.int32), ("reserved", np.int32),
    ("gain", np.int64), ("split_value", np.int64)])
assert CUT_NODE_DTYPE.itemsize == 48
CUT_NODE_WORDS = 12
CUT_GAIN_DTYPE = np.dtype([("level", np.int32), ("id", np.int32), ("gain", np.int64)])
assert CUT_GAIN_DTYPE.itemsize == 16
CUT_GAIN_WORDS = 4
CUT_MAX_PENALTY = 1 << 32
CUT_BLOCK_ALWAYS = (1 << 63) - 1   # tree_cut_tuning: always one workgroup

# VSG_RENDER_DISTANCE_NONE, VSG_RENDER_MAX_TOLERANCE_SQ
DISTANCE_NONE = 0x7fffffff
MAX_TOLERANCE_SQ = 4096

# VSG_RENDER_CONNECT_N4 / _N8 (SegmentationDesc::N4_CONNECT / N8_CONNECT)
N4 = 1
N8 = 2


# Every symbol include/vsg_render.h declares.
EXPORTED_SYMBOLS = [
    "vsg_render_last_error", "vsg_render_default_options", "vsg_render_create", "vsg_render_destroy",
    "vsg_render_frame", "vsg_render_id_image", "vsg_render_level", "vsg_render_default_stride",
    "vsg_render_last_stats", "vsg_render_color", "vsg_render_rasterize", "vsg_render_last_vector_stats",
    "vsg_render_level_regions", "vsg_render_last_level_stats",
    "vsg_render_level_components", "vsg_render_last_component_stats",
    "vsg_render_level_boundaries", "vsg_render_last_boundary_stats",
    "vsg_render_level_adjacency", "vsg_render_last_adjacency_stats",
    "vsg_render_level_overlap", "vsg_render_last_overlap_stats",
    "vsg_render_persistence_image", "vsg_render_persistence_frame", "vsg_render_persistence_graph",
    "vsg_render_last_persistence_stats",
    "vsg_render_tree_cut", "vsg_render_tree_cut_tuning", "vsg_render_last_cut_stats",
    "vsg_render_level_colors", "vsg_render_mean_frame", "vsg_render_last_color_stats",
    "vsg_render_volume_begin", "vsg_render_volume_add", "vsg_render_volume_table", "vsg_render_last_volume_stats",
    "vsg_render_level_pool", "vsg_render_level_unpool", "vsg_render_last_pool_stats",
    "vsg_render_level_contours", "vsg_render_last_contour_stats",
    "vsg_render_level_mesh", "vsg_render_last_mesh_stats",
    "vsg_render_level_mesh_simplified", "vsg_render_last_simplify_stats",
    "vsg_render_boundary_distance", "vsg_render_boundary_benchmark", "vsg_render_last_distance_stats",
]


def build(force=False):
    """Compiles libvsg_render.so in-tree (hipcc --offload-arch=gfx950); make decides what is stale."""
    _capi.make("render", force)
    return LIB_PATH


_handle = None


def lib():
    global _handle
    if _handle is not None:
        return _handle
    L = _capi.load(LIB_PATH, "libvsg_render.so")
    vp = C.c_void_p
    L.vsg_render_last_error.restype = C.c_char_p
    L.vsg_render_default_options.argtypes = [C.POINTER(VsgRenderOptions)]
    L.vsg_render_default_options.restype = None
    L.vsg_render_create.argtypes = [C.POINTER(VsgRenderOptions), C.c_int, C.c_int, C.POINTER(vp)]
    L.vsg_render_destroy.argtypes = [vp]
    L.vsg_render_destroy.restype = None
    L.vsg_render_frame.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_int]
    L.vsg_render_id_image.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, vp, C.c_int]
    L.vsg_render_level.argtypes = [vp, C.POINTER(C.c_int)]
    L.vsg_render_default_stride.argtypes = [C.c_int]
    L.vsg_render_default_stride.restype = C.c_size_t
    L.vsg_render_last_stats.argtypes = [vp, C.POINTER(VsgRenderStats)]
    L.vsg_render_color.argtypes = [C.c_int, C.POINTER(C.c_uint8 * 3)]
    L.vsg_render_color.restype = None
    L.vsg_render_rasterize.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_vector_stats.argtypes = [vp, C.POINTER(VsgRenderVectorStats)]
    L.vsg_render_level_regions.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t),
                                           vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_level_stats.argtypes = [vp, C.POINTER(VsgRenderLevelStats)]
    L.vsg_render_level_components.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t,
                                              C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), vp,
                                              C.c_int]
    L.vsg_render_last_component_stats.argtypes = [vp, C.POINTER(VsgRenderComponentStats)]
    L.vsg_render_level_boundaries.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_size_t,
                                              C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_boundary_stats.argtypes = [vp, C.POINTER(VsgRenderBoundaryStats)]
    L.vsg_render_level_adjacency.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_size_t,
                                             C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_adjacency_stats.argtypes = [vp, C.POINTER(VsgRenderAdjacencyStats)]
    L.vsg_render_level_overlap.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, C.c_int,
                                           vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t,
                                           C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_overlap_stats.argtypes = [vp, C.POINTER(VsgRenderOverlapStats)]
    L.vsg_render_persistence_image.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.POINTER(C.c_int), C.c_int]
    L.vsg_render_persistence_frame.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_int, vp, C.c_size_t,
                                               C.c_int, C.POINTER(C.c_int)]
    L.vsg_render_persistence_graph.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, vp, C.c_size_t,
                                               C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp,
                                               C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_persistence_stats.argtypes = [vp, C.POINTER(VsgRenderPersistenceStats)]
    L.vsg_render_level_colors.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, vp,
                                          C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_mean_frame.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, vp,
                                        C.c_size_t, C.c_int]
    L.vsg_render_last_color_stats.argtypes = [vp, C.POINTER(VsgRenderColorStats)]
    L.vsg_render_level_pool.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                                        C.c_ssize_t, C.c_ssize_t, C.c_ssize_t, C.c_int, vp, vp, vp, vp, vp,
                                        C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_level_unpool.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, C.c_int,
                                          C.c_int, C.c_float, vp, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_ssize_t,
                                          C.c_int]
    L.vsg_render_last_pool_stats.argtypes = [vp, C.POINTER(VsgRenderPoolStats)]
    L.vsg_render_volume_begin.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.vsg_render_volume_add.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_int, vp, C.c_size_t,
                                        C.c_int]
    L.vsg_render_volume_table.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t,
                                          C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_volume_stats.argtypes = [vp, C.POINTER(VsgRenderVolumeStats)]
    L.vsg_render_level_contours.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t,
                                            C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_contour_stats.argtypes = [vp, C.POINTER(VsgRenderContourStats)]
    L.vsg_render_level_mesh.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int,
                                        vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t),
                                        vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t),
                                        C.c_int]
    L.vsg_render_last_mesh_stats.argtypes = [vp, C.POINTER(VsgRenderMeshStats)]
    L.vsg_render_level_mesh_simplified.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_float, C.c_int,
                                                   vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t,
                                                   C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t),
                                                   vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_simplify_stats.argtypes = [vp, C.POINTER(VsgRenderSimplifyStats)]
    L.vsg_render_boundary_distance.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, vp, C.c_int]
    L.vsg_render_boundary_benchmark.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, vp,
                                                C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.vsg_render_last_distance_stats.argtypes = [vp, C.POINTER(VsgRenderDistanceStats)]
    L.vsg_render_tree_cut.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int64, vp, C.c_size_t,
                                      C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.POINTER(C.c_int64),
                                      C.c_int]
    L.vsg_render_tree_cut_tuning.argtypes = [vp, C.c_int64]
    L.vsg_render_last_cut_stats.argtypes = [vp, C.POINTER(VsgRenderCutStats)]
    _handle = L
    return L


check = _capi.checker("vsg_render", lambda: lib().vsg_render_last_error())


def default_render_options(**kw):
    return _capi.default_options(VsgRenderOptions, lib().vsg_render_default_options, "render", **kw)


def render_color(region_id):
    """(c0, c1, c2) = srand(region_id); rand() % 255 three times, the colour the reference paints a
    region id with (bytes 0, 1, 2 of the pixel).  Host only."""
    c = (C.c_uint8 * 3)()
    # srand takes the id as unsigned; any Python int is reduced to the 32 bits the C int carries
    rid = ((int(region_id) + (1 << 31)) % (1 << 32)) - (1 << 31)
    lib().vsg_render_color(rid, C.byref(c))
    return tuple(c)


def default_stride(width):
    return (3 * width + 3) // 4 * 4


def _frame_ptr(x, rows, width, what):
    return _capi.frame_ptr(x, rows, width, 3, what, unpacked="pixels have to be packed BGR24")


class SegmentationRenderer(_capi.Handle):
    """Renders SegmentationDesc messages at a hierarchy level on one MI355X.

    options: blend_alpha (0.5), hierarchy_level (0; fractional = fraction of the hierarchy's height),
    highlight_edges (True), concat_with_source (False), has_video (True), device (-1)."""

    def __init__(self, width, height, **options):
        self.W, self.H = width, height
        self.opts = default_render_options(**{k: (int(v) if isinstance(v, bool) else v) for k, v in options.items()})
        h = C.c_void_p()
        check(lib().vsg_render_create(C.byref(self.opts), width, height, C.byref(h)))
        self.h = h
        self._destroy = lib().vsg_render_destroy

    @property
    def out_rows(self):
        return self.H * (2 if self.opts.concat_with_source else 1)

    @property
    def level(self):
        """The level resolved on the first rendered frame (None before it)."""
        v = C.c_int()
        rc = lib().vsg_render_level(self.h, C.byref(v))
        if rc == _lib.VSG_ERR_STATE:
            return None
        check(rc)
        return v.value

    def render(self, seg_bytes, bgr=None, out=None):
        """Returns the rendered out_rows x W x 3 uint8 frame: a numpy array, or a torch CUDA tensor
        when bgr is one.  out: a caller's buffer instead (rows x W x 3 view; its rows may be wider
        than 3 * W bytes, the bytes between them are left alone)."""
        p_bgr, stride, mem_in = None, 0, VSG_MEM_HOST
        if self.opts.has_video:
            if bgr is None:
                raise ValueError("the renderer was created with has_video: pass the source frame")
            p_bgr, stride, mem_in = _frame_ptr(bgr, self.H, self.W, "bgr")
        if out is None:
            if bgr is not None and self.opts.has_video and _capi.is_torch(bgr) and bgr.is_cuda:
                import torch
                out = torch.empty((self.out_rows, self.W, 3), dtype=torch.uint8, device=bgr.device)
            else:
                out = np.empty((self.out_rows, self.W, 3), np.uint8)
        p_out, out_stride, mem_out = _frame_ptr(out, self.out_rows, self.W, "out")
        seg_bytes = bytes(seg_bytes)
        check(lib().vsg_render_frame(self.h, seg_bytes, len(seg_bytes), p_bgr, stride, mem_in, p_out, out_stride,
                                     mem_out))
        return out

    def id_image(self, seg_bytes, level=0, out=None):
        """H x W int32 ids at `level` (-1 where no region covers a pixel).  out: a contiguous int32
        numpy array or torch CUDA tensor to fill instead of a new numpy array."""
        if out is None:
            out = np.empty((self.H, self.W), np.int32)
        if tuple(out.shape) != (self.H, self.W) or str(out.dtype).replace("torch.", "") != "int32":
            raise ValueError("out has to be %d x %d int32" % (self.H, self.W))
        p, mem = _capi.contiguous_ptr(out)
        seg_bytes = bytes(seg_bytes)
        check(lib().vsg_render_id_image(self.h, seg_bytes, len(seg_bytes), int(level), p, mem))
        return out

    def rasterize(self, seg_bytes, out=None):
        """The scan intervals of a desc's vectorization at the renderer's frame size (the reference's
        ReplaceRasterizationFromVectorization): an (n, 4) int32 array of {y, left_x, right_x,
        region id} in the reference's order, its empty intervals included.  out: a contiguous
        (capacity, 4) int32 numpy array or torch CUDA tensor to fill instead; the first n rows of it
        are returned."""
        seg_bytes = bytes(seg_bytes)
        n = C.c_size_t()
        if out is None:
            # the count first (host work only, done again by the call below), then a buffer of that size
            check(lib().vsg_render_rasterize(self.h, seg_bytes, len(seg_bytes), None, 0, C.byref(n), VSG_MEM_HOST))
            out = np.empty((n.value, 4), np.int32)
            if n.value == 0:
                return out
        if len(out.shape) != 2 or out.shape[1] != 4 or str(out.dtype).replace("torch.", "") != "int32":
            raise ValueError("out has to be (capacity, 4) int32")
        p, mem = _capi.contiguous_ptr(out)
        check(lib().vsg_render_rasterize(self.h, seg_bytes, len(seg_bytes), p, out.shape[0], C.byref(n), mem))
        return out[:n.value]

    def level_regions(self, seg_bytes, level=0, regions_out=None, intervals_out=None):
        """The regions of hierarchy level `level` (GetCompoundRegionRasterizations, RasterizationArea,
        ShapeMomentsFromRasterization): (regions, intervals).  regions: a LEVEL_REGION_DTYPE array
        ordered by id; intervals: (n, 4) int32 {y, left_x, right_x, region id}, grouped by region in
        that order.  Without outputs the counts are asked for first and both arrays are allocated
        exactly.  regions_out / intervals_out: buffers to fill instead, both numpy (a LEVEL_REGION_DTYPE
        array and a (capacity, 4) int32 array) or both torch CUDA tensors ((capacity, 14) int32, the
        float fields as bit views, and (capacity, 4) int32); the filled parts of them are returned."""
        seg_bytes = bytes(seg_bytes)
        nr, ni = C.c_size_t(), C.c_size_t()
        if (regions_out is None) != (intervals_out is None):
            raise ValueError("pass both outputs or neither")
        if regions_out is None:
            check(lib().vsg_render_level_regions(self.h, seg_bytes, len(seg_bytes), int(level), None, 0, C.byref(nr),
                                                 None, 0, C.byref(ni), VSG_MEM_HOST))
            regions_out = np.empty(nr.value, LEVEL_REGION_DTYPE)
            intervals_out = np.empty((ni.value, 4), np.int32)
        if _capi.is_torch(regions_out) != _capi.is_torch(intervals_out):
            raise ValueError("both outputs have to be numpy arrays or both torch tensors")
        if _capi.is_torch(regions_out):
            if (regions_out.dim() != 2 or regions_out.shape[1] != LEVEL_REGION_WORDS
                    or str(regions_out.dtype) != "torch.int32"):
                raise ValueError("regions_out has to be (capacity, %d) int32" % LEVEL_REGION_WORDS)
        elif regions_out.dtype != LEVEL_REGION_DTYPE or regions_out.ndim != 1:
            raise ValueError("regions_out has to be a one-dimensional LEVEL_REGION_DTYPE array")
        if (len(intervals_out.shape) != 2 or intervals_out.shape[1] != 4
                or str(intervals_out.dtype).replace("torch.", "") != "int32"):
            raise ValueError("intervals_out has to be (capacity, 4) int32")
        pr, mem = _capi.contiguous_ptr(regions_out)
        pi, mem_i = _capi.contiguous_ptr(intervals_out)
        if mem != mem_i:
            raise ValueError("both outputs have to be in the same kind of memory")
        check(lib().vsg_render_level_regions(self.h, seg_bytes, len(seg_bytes), int(level), pr, regions_out.shape[0],
                                             C.byref(nr), pi, intervals_out.shape[0], C.byref(ni), mem))
        return regions_out[:nr.value], intervals_out[:ni.value]

    def last_level_stats(self):
        """vsg_render_last_level_stats of the last level_regions call, as a dict."""
        s = VsgRenderLevelStats()
        check(lib().vsg_render_last_level_stats(self.h, C.byref(s)))
        return s.as_dict()

    def level_components(self, seg_bytes, level=0, connectedness=N4, label_image=False, components_out=None,
                         intervals_out=None, labels_out=None):
        """The connected components (N4 or N8) of every region of hierarchy level `level`, in the
        reference's ConnectedComponents order: (components, intervals), or (components, intervals,
        labels) with label_image=True or a labels_out.  components: a LEVEL_COMPONENT_DTYPE array ordered
        by (id, component); intervals: (n, 4) int32 {y, left_x, right_x, region id} grouped by component
        in that order; labels: H x W int32, the index of each pixel's component in `components`, -1
        where there is none.  Without outputs the counts are asked for first and the arrays are
        allocated exactly.  components_out / intervals_out (both or neither) and labels_out: buffers to
        fill instead, all numpy (a LEVEL_COMPONENT_DTYPE array, a (capacity, 4) int32 array, an H x W
        int32 array) or all torch CUDA tensors ((capacity, 16) int32 with the float fields as bit views,
        (capacity, 4) int32, H x W int32); the filled parts are returned."""
        seg_bytes = bytes(seg_bytes)
        nc, ni = C.c_size_t(), C.c_size_t()
        if (components_out is None) != (intervals_out is None):
            raise ValueError("pass both list outputs or neither")
        if components_out is None:
            if labels_out is not None and _capi.is_torch(labels_out):
                raise ValueError("a torch labels_out needs torch components_out and intervals_out")
            check(lib().vsg_render_level_components(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                                    None, 0, C.byref(nc), None, 0, C.byref(ni), None, VSG_MEM_HOST))
            components_out = np.empty(nc.value, LEVEL_COMPONENT_DTYPE)
            intervals_out = np.empty((ni.value, 4), np.int32)
        torch_out = _capi.is_torch(components_out)
        if torch_out != _capi.is_torch(intervals_out):
            raise ValueError("both list outputs have to be numpy arrays or both torch tensors")
        if torch_out:
            if (components_out.dim() != 2 or components_out.shape[1] != LEVEL_COMPONENT_WORDS
                    or str(components_out.dtype) != "torch.int32"):
                raise ValueError("components_out has to be (capacity, %d) int32" % LEVEL_COMPONENT_WORDS)
        elif components_out.dtype != LEVEL_COMPONENT_DTYPE or components_out.ndim != 1:
            raise ValueError("components_out has to be a one-dimensional LEVEL_COMPONENT_DTYPE array")
        if (len(intervals_out.shape) != 2 or intervals_out.shape[1] != 4
                or str(intervals_out.dtype).replace("torch.", "") != "int32"):
            raise ValueError("intervals_out has to be (capacity, 4) int32")
        pc, mem = _capi.contiguous_ptr(components_out)
        pi, mem_i = _capi.contiguous_ptr(intervals_out)
        if mem != mem_i:
            raise ValueError("all outputs have to be in the same kind of memory")
        pl = None
        if labels_out is None and label_image:
            if torch_out:
                import torch
                labels_out = torch.empty((self.H, self.W), dtype=torch.int32, device=components_out.device)
            else:
                labels_out = np.empty((self.H, self.W), np.int32)
        if labels_out is not None:
            if (tuple(labels_out.shape) != (self.H, self.W)
                    or str(labels_out.dtype).replace("torch.", "") != "int32"):
                raise ValueError("labels_out has to be %d x %d int32" % (self.H, self.W))
            pl, mem_l = _capi.contiguous_ptr(labels_out)
            if mem_l != mem:
                raise ValueError("all outputs have to be in the same kind of memory")
        check(lib().vsg_render_level_components(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                                pc, components_out.shape[0], C.byref(nc), pi, intervals_out.shape[0],
                                                C.byref(ni), pl, mem))
        if labels_out is None:
            return components_out[:nc.value], intervals_out[:ni.value]
        return components_out[:nc.value], intervals_out[:ni.value], labels_out

    def last_component_stats(self):
        """vsg_render_last_component_stats of the last level_components call, as a dict."""
        s = VsgRenderComponentStats()
        check(lib().vsg_render_last_component_stats(self.h, C.byref(s)))
        return s.as_dict()

    def level_boundaries(self, seg_bytes, level=0, connectedness=0, outer=False, boundaries_out=None,
                         points_out=None):
        """The N4 boundary pixels (the reference's GetBoundary) of every region of hierarchy level `level`
        (connectedness 0) or of every connected component of its regions (N4 or N8): (records, points).
        records: a LEVEL_BOUNDARY_DTYPE array, record k belonging to record k of level_regions
        (level_components); points: (n, 2) int32 {x, y}, grouped by boundary in that order, within a boundary
        by y, then x.  outer=False: the pixels of a group with a 4-neighbour outside it; True: the positions
        of [-1, W] x [-1, H] outside a group with a 4-neighbour in it, at their true x (the reference
        reports x + 1).  Without outputs the counts are asked for first and both arrays are allocated
        exactly.  boundaries_out / points_out: buffers to fill instead, both numpy (a LEVEL_BOUNDARY_DTYPE
        array and a (capacity, 2) int32 array) or both torch CUDA tensors ((capacity, 4) int32 and
        (capacity, 2) int32); the filled parts of them are returned."""
        seg_bytes = bytes(seg_bytes)
        which = BOUNDARY_OUTER if outer else BOUNDARY_INNER
        nb, npts = C.c_size_t(), C.c_size_t()
        if (boundaries_out is None) != (points_out is None):
            raise ValueError("pass both outputs or neither")
        if boundaries_out is None:
            check(lib().vsg_render_level_boundaries(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                                    which, None, 0, C.byref(nb), None, 0, C.byref(npts), VSG_MEM_HOST))
            boundaries_out = np.empty(nb.value, LEVEL_BOUNDARY_DTYPE)
            points_out = np.empty((npts.value, 2), np.int32)
        if _capi.is_torch(boundaries_out) != _capi.is_torch(points_out):
            raise ValueError("both outputs have to be numpy arrays or both torch tensors")
        if _capi.is_torch(boundaries_out):
            if (boundaries_out.dim() != 2 or boundaries_out.shape[1] != LEVEL_BOUNDARY_WORDS
                    or str(boundaries_out.dtype) != "torch.int32"):
                raise ValueError("boundaries_out has to be (capacity, %d) int32" % LEVEL_BOUNDARY_WORDS)
        elif boundaries_out.dtype != LEVEL_BOUNDARY_DTYPE or boundaries_out.ndim != 1:
            raise ValueError("boundaries_out has to be a one-dimensional LEVEL_BOUNDARY_DTYPE array")
        if (len(points_out.shape) != 2 or points_out.shape[1] != 2
                or str(points_out.dtype).replace("torch.", "") != "int32"):
            raise ValueError("points_out has to be (capacity, 2) int32")
        pb, mem = _capi.contiguous_ptr(boundaries_out)
        pp, mem_p = _capi.contiguous_ptr(points_out)
        if mem != mem_p:
            raise ValueError("both outputs have to be in the same kind of memory")
        check(lib().vsg_render_level_boundaries(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                                which, pb, boundaries_out.shape[0], C.byref(nb), pp,
                                                points_out.shape[0], C.byref(npts), mem))
        return boundaries_out[:nb.value], points_out[:npts.value]

    def last_boundary_stats(self):
        """vsg_render_last_boundary_stats of the last level_boundaries call, as a dict."""
        s = VsgRenderBoundaryStats()
        check(lib().vsg_render_last_boundary_stats(self.h, C.byref(s)))
        return s.as_dict()

    def level_adjacency(self, seg_bytes, level=0, connectedness=0, neighbourhood=ADJACENT_N4, nodes_out=None,
                        edges_out=None):
        """The region adjacency graph of hierarchy level `level`: one node per region (connectedness 0) or per
        connected component of its regions (N4 or N8), and one directed edge per pair of nodes that touch:
        (nodes, edges).  nodes: a LEVEL_NODE_DTYPE array, record k belonging to record k of level_regions
        (level_components), with the node's slice of `edges` and its perimeter split into sides on the frame
        edge, next to uncovered pixels and next to other groups; edges: a LEVEL_EDGE_DTYPE array, grouped by
        node, within a node by ascending neighbour, with the shared pixel sides and, for
        neighbourhood=ADJACENT_N8, the diagonal contacts.  Without outputs the counts are asked for first
        and both arrays are allocated exactly.  nodes_out / edges_out: buffers to fill instead, both numpy
        (a LEVEL_NODE_DTYPE and a LEVEL_EDGE_DTYPE array) or both torch CUDA tensors ((capacity, 7) int32 and
        (capacity, 4) int32); the filled parts of them are returned."""
        seg_bytes = bytes(seg_bytes)
        nn, ne = C.c_size_t(), C.c_size_t()
        if (nodes_out is None) != (edges_out is None):
            raise ValueError("pass both outputs or neither")
        if nodes_out is None:
            check(lib().vsg_render_level_adjacency(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                                   int(neighbourhood), None, 0, C.byref(nn), None, 0, C.byref(ne),
                                                   VSG_MEM_HOST))
            nodes_out = np.empty(nn.value, LEVEL_NODE_DTYPE)
            edges_out = np.empty(ne.value, LEVEL_EDGE_DTYPE)
            if nn.value == 0:
                return nodes_out, edges_out
        if _capi.is_torch(nodes_out) != _capi.is_torch(edges_out):
            raise ValueError("both outputs have to be numpy arrays or both torch tensors")
        if _capi.is_torch(nodes_out):
            if nodes_out.dim() != 2 or nodes_out.shape[1] != LEVEL_NODE_WORDS or str(nodes_out.dtype) != "torch.int32":
                raise ValueError("nodes_out has to be (capacity, %d) int32" % LEVEL_NODE_WORDS)
            if edges_out.dim() != 2 or edges_out.shape[1] != LEVEL_EDGE_WORDS or str(edges_out.dtype) != "torch.int32":
                raise ValueError("edges_out has to be (capacity, %d) int32" % LEVEL_EDGE_WORDS)
        else:
            if nodes_out.dtype != LEVEL_NODE_DTYPE or nodes_out.ndim != 1:
                raise ValueError("nodes_out has to be a one-dimensional LEVEL_NODE_DTYPE array")
            if edges_out.dtype != LEVEL_EDGE_DTYPE or edges_out.ndim != 1:
                raise ValueError("edges_out has to be a one-dimensional LEVEL_EDGE_DTYPE array")
        pn, mem = _capi.contiguous_ptr(nodes_out)
        pe, mem_e = _capi.contiguous_ptr(edges_out)
        if mem != mem_e:
            raise ValueError("both outputs have to be in the same kind of memory")
        check(lib().vsg_render_level_adjacency(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                               int(neighbourhood), pn, nodes_out.shape[0], C.byref(nn), pe,
                                               edges_out.shape[0], C.byref(ne), mem))
        return nodes_out[:nn.value], edges_out[:ne.value]

    def last_adjacency_stats(self):
        """vsg_render_last_adjacency_stats of the last level_adjacency call, as a dict."""
        s = VsgRenderAdjacencyStats()
        check(lib().vsg_render_last_adjacency_stats(self.h, C.byref(s)))
        return s.as_dict()

    def _other_ptr(self, other):
        """(pointer, row pitch in int32, mem kind) of the H x W int32 plane `other`: a numpy array or a torch
        tensor whose rows are contiguous and may be further apart than W values."""
        if tuple(other.shape) != (self.H, self.W) or str(other.dtype).replace("torch.", "") != "int32":
            raise ValueError("other has to be %d x %d int32" % (self.H, self.W))
        ptr, strides, mem = _capi._memory(other)
        unit = 1 if _capi.is_torch(other) else 4        # torch strides count elements, numpy's bytes
        if strides[1] != unit and self.W > 1:
            raise ValueError("other: the values of a row have to be contiguous")
        pitch = self.W
        if self.H > 1:
            if strides[0] % unit or strides[0] // unit < self.W:
                raise ValueError("other: rows have to be at least W int32 apart")
            pitch = strides[0] // unit
        _capi._drain(other)
        return C.c_void_p(ptr), pitch, mem

    def level_overlap(self, seg_bytes, level=0, other=None, connectedness=0, rows_out=None, cols_out=None,
                      pairs_out=None):
        """The overlap (contingency) table of hierarchy level `level` and the label plane `other`: (rows, cols,
        pairs).  other: an H x W int32 numpy array or torch CUDA tensor with contiguous rows (its row stride
        becomes the pitch); a negative value is "no label".  rows: an OVERLAP_ROW_DTYPE array, record k
        belonging to record k of level_regions (connectedness 0) or level_components (N4 or N8), with the
        group's area, how much of it is unlabelled, its slice of `pairs` and the label it overlaps most;
        cols: an OVERLAP_COL_DTYPE array, one per distinct label by ascending label, with the label's area,
        how much of it no group covers and the row that overlaps it most; pairs: an OVERLAP_PAIR_DTYPE array,
        one per (group, label) with a common pixel, grouped by row, within a row by ascending label.
        Without outputs the counts are asked for first and the arrays are allocated exactly.  rows_out /
        cols_out / pairs_out (all or none): buffers to fill instead, all numpy (arrays of the three dtypes) or
        all torch CUDA tensors ((capacity, 8), (capacity, 6) and (capacity, 4) int32); the filled parts of
        them are returned."""
        if other is None:
            raise ValueError("other is needed")
        seg_bytes = bytes(seg_bytes)
        po, pitch, mem_other = self._other_ptr(other)
        nr, nc, npairs = C.c_size_t(), C.c_size_t(), C.c_size_t()
        outs = (rows_out, cols_out, pairs_out)
        if any(o is None for o in outs) and not all(o is None for o in outs):
            raise ValueError("pass all three outputs or none")
        if rows_out is None:
            check(lib().vsg_render_level_overlap(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                                 po, pitch, mem_other, None, 0, C.byref(nr), None, 0, C.byref(nc),
                                                 None, 0, C.byref(npairs), VSG_MEM_HOST))
            rows_out = np.empty(nr.value, OVERLAP_ROW_DTYPE)
            cols_out = np.empty(nc.value, OVERLAP_COL_DTYPE)
            pairs_out = np.empty(npairs.value, OVERLAP_PAIR_DTYPE)
            if nr.value == 0 and nc.value == 0:
                return rows_out, cols_out, pairs_out
        outs = (rows_out, cols_out, pairs_out)
        if len({_capi.is_torch(o) for o in outs}) != 1:
            raise ValueError("all outputs have to be numpy arrays or all torch tensors")
        specs = (("rows_out", OVERLAP_ROW_DTYPE, OVERLAP_ROW_WORDS), ("cols_out", OVERLAP_COL_DTYPE, OVERLAP_COL_WORDS),
                 ("pairs_out", OVERLAP_PAIR_DTYPE, OVERLAP_PAIR_WORDS))
        for o, (name, dtype, words) in zip(outs, specs):
            if _capi.is_torch(o):
                if o.dim() != 2 or o.shape[1] != words or str(o.dtype) != "torch.int32":
                    raise ValueError("%s has to be (capacity, %d) int32" % (name, words))
            elif o.dtype != dtype or o.ndim != 1:
                raise ValueError("%s has to be a one-dimensional array of its dtype" % name)
        ptrs = [_capi.contiguous_ptr(o) for o in outs]
        if len({mem for _, mem in ptrs}) != 1:
            raise ValueError("all outputs have to be in the same kind of memory")
        check(lib().vsg_render_level_overlap(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness), po,
                                             pitch, mem_other, ptrs[0][0], rows_out.shape[0], C.byref(nr),
                                             ptrs[1][0], cols_out.shape[0], C.byref(nc), ptrs[2][0],
                                             pairs_out.shape[0], C.byref(npairs), ptrs[0][1]))
        return rows_out[:nr.value], cols_out[:nc.value], pairs_out[:npairs.value]

    def last_overlap_stats(self):
        """vsg_render_last_overlap_stats of the last level_overlap call, as a dict."""
        s = VsgRenderOverlapStats()
        check(lib().vsg_render_last_overlap_stats(self.h, C.byref(s)))
        return s.as_dict()

    def persistence_image(self, seg_bytes, out=None):
        """The boundary persistence plane of the desc's hierarchy: (plane, levels).  plane: H x W int32, for
        every pixel the number of hierarchy levels at which it still differs from its right or its below
        neighbour (0: inside a level-0 region; levels: a boundary no level removes), so that plane > l is
        the edge mask of level l; levels: the hierarchy's height L.  out: a contiguous int32 numpy array or
        torch CUDA tensor to fill instead of a new numpy array."""
        if out is None:
            out = np.empty((self.H, self.W), np.int32)
        if tuple(out.shape) != (self.H, self.W) or str(out.dtype).replace("torch.", "") != "int32":
            raise ValueError("out has to be %d x %d int32" % (self.H, self.W))
        p, mem = _capi.contiguous_ptr(out)
        seg_bytes = bytes(seg_bytes)
        levels = C.c_int()
        check(lib().vsg_render_persistence_image(self.h, seg_bytes, len(seg_bytes), p, C.byref(levels), mem))
        return out, levels.value

    def persistence_frame(self, seg_bytes, bgr=None, out=None):
        """The persistence plane as a picture, H x W x 3 uint8: the source frame (white without has_video)
        darkened by (L - Q) / L, so that a boundary is the darker the more levels it survives.  A numpy array,
        or a torch CUDA tensor when bgr is one.  out: a caller's buffer instead, as in render()."""
        p_bgr, stride, mem_in = None, 0, VSG_MEM_HOST
        if self.opts.has_video:
            if bgr is None:
                raise ValueError("the renderer was created with has_video: pass the source frame")
            p_bgr, stride, mem_in = _frame_ptr(bgr, self.H, self.W, "bgr")
        if out is None:
            if bgr is not None and self.opts.has_video and _capi.is_torch(bgr) and bgr.is_cuda:
                import torch
                out = torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=bgr.device)
            else:
                out = np.empty((self.H, self.W, 3), np.uint8)
        p_out, out_stride, mem_out = _frame_ptr(out, self.H, self.W, "out")
        seg_bytes = bytes(seg_bytes)
        levels = C.c_int()
        check(lib().vsg_render_persistence_frame(self.h, seg_bytes, len(seg_bytes), p_bgr, stride, mem_in, p_out,
                                                 out_stride, mem_out, C.byref(levels)))
        return out

    def persistence_graph(self, seg_bytes, neighbourhood=ADJACENT_N4, nodes_out=None, edges_out=None,
                          persistence_out=None, level_sides_out=None):
        """The level-0 adjacency graph with the level at which every pair of touching regions merges: (nodes,
        edges, persistence, level_sides).  nodes, edges: those of level_adjacency(seg, 0, 0, neighbourhood);
        persistence: int32 per directed edge, the number of levels at which its two regions differ (levels:
        never merged); level_sides: int64 per level, the pixel sides between different regions of that level.
        Without outputs the counts are asked for first and the arrays are allocated exactly.  The four outputs
        (all or none): buffers to fill instead, all numpy (LEVEL_NODE_DTYPE, LEVEL_EDGE_DTYPE, int32 and int64
        arrays) or all torch CUDA tensors ((capacity, 7) int32, (capacity, 4) int32, int32 with at least the
        edges' capacity, int64); the filled parts of them are returned."""
        seg_bytes = bytes(seg_bytes)
        hood = int(neighbourhood)
        nn, ne, nl = C.c_size_t(), C.c_size_t(), C.c_size_t()
        outs = (nodes_out, edges_out, persistence_out, level_sides_out)
        if any(o is None for o in outs) and not all(o is None for o in outs):
            raise ValueError("pass all four outputs or none")
        if nodes_out is None:
            check(lib().vsg_render_persistence_graph(self.h, seg_bytes, len(seg_bytes), hood, None, 0, C.byref(nn),
                                                     None, 0, C.byref(ne), None, None, 0, C.byref(nl), VSG_MEM_HOST))
            nodes_out = np.empty(nn.value, LEVEL_NODE_DTYPE)
            edges_out = np.empty(ne.value, LEVEL_EDGE_DTYPE)
            persistence_out = np.empty(ne.value, np.int32)
            level_sides_out = np.empty(nl.value, np.int64)
        outs = (nodes_out, edges_out, persistence_out, level_sides_out)
        if len({_capi.is_torch(o) for o in outs}) != 1:
            raise ValueError("all outputs have to be numpy arrays or all torch tensors")
        if _capi.is_torch(nodes_out):
            if nodes_out.dim() != 2 or nodes_out.shape[1] != LEVEL_NODE_WORDS or str(nodes_out.dtype) != "torch.int32":
                raise ValueError("nodes_out has to be (capacity, %d) int32" % LEVEL_NODE_WORDS)
            if edges_out.dim() != 2 or edges_out.shape[1] != LEVEL_EDGE_WORDS or str(edges_out.dtype) != "torch.int32":
                raise ValueError("edges_out has to be (capacity, %d) int32" % LEVEL_EDGE_WORDS)
        else:
            if nodes_out.dtype != LEVEL_NODE_DTYPE or nodes_out.ndim != 1:
                raise ValueError("nodes_out has to be a one-dimensional LEVEL_NODE_DTYPE array")
            if edges_out.dtype != LEVEL_EDGE_DTYPE or edges_out.ndim != 1:
                raise ValueError("edges_out has to be a one-dimensional LEVEL_EDGE_DTYPE array")
        if len(persistence_out.shape) != 1 or str(persistence_out.dtype).replace("torch.", "") != "int32":
            raise ValueError("persistence_out has to be one-dimensional int32")
        if len(level_sides_out.shape) != 1 or str(level_sides_out.dtype).replace("torch.", "") != "int64":
            raise ValueError("level_sides_out has to be one-dimensional int64")
        if persistence_out.shape[0] < edges_out.shape[0]:
            raise ValueError("persistence_out has to hold as many entries as edges_out")
        ptrs = [_capi.contiguous_ptr(o) for o in outs]
        if len({mem for _, mem in ptrs}) != 1:
            raise ValueError("all outputs have to be in the same kind of memory")
        check(lib().vsg_render_persistence_graph(self.h, seg_bytes, len(seg_bytes), hood, ptrs[0][0],
                                                 nodes_out.shape[0], C.byref(nn), ptrs[1][0], edges_out.shape[0],
                                                 C.byref(ne), ptrs[2][0], ptrs[3][0], level_sides_out.shape[0],
                                                 C.byref(nl), ptrs[0][1]))
        return nodes_out[:nn.value], edges_out[:ne.value], persistence_out[:ne.value], level_sides_out[:nl.value]

    def last_persistence_stats(self):
        """vsg_render_last_persistence_stats of the last persistence call, as a dict."""
        s = VsgRenderPersistenceStats()
        check(lib().vsg_render_last_persistence_stats(self.h, C.byref(s)))
        return s.as_dict()

    def level_colors(self, seg_bytes, level=0, frame=None, connectedness=0, colors_out=None):
        """What every group of hierarchy level `level` looks like in `frame`: a LEVEL_COLOR_DTYPE array, record
        k belonging to record k of level_regions (connectedness 0) or level_components (N4 or N8), with the
        group's area and, per channel in B, G, R order, the sum, the sum of squares, the minimum, the maximum
        and the mean rounded half up, all in integers.  frame: the H x W x 3 uint8 BGR24 frame, a numpy array
        or a torch CUDA tensor (its rows may be further apart than 3 * W bytes).  Without colors_out the count
        is asked for first and the array is allocated exactly.  colors_out: a buffer to fill instead, a
        LEVEL_COLOR_DTYPE array or a (capacity, 18) int32 torch CUDA tensor; the filled part of it is
        returned."""
        if frame is None:
            raise ValueError("frame is needed")
        seg_bytes = bytes(seg_bytes)
        p_bgr, stride, mem_in = _frame_ptr(frame, self.H, self.W, "frame")
        n = C.c_size_t()
        if colors_out is None:
            check(lib().vsg_render_level_colors(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                                p_bgr, stride, mem_in, None, 0, C.byref(n), VSG_MEM_HOST))
            colors_out = np.empty(n.value, LEVEL_COLOR_DTYPE)
            if n.value == 0:
                return colors_out
        if _capi.is_torch(colors_out):
            if (colors_out.dim() != 2 or colors_out.shape[1] != LEVEL_COLOR_WORDS
                    or str(colors_out.dtype) != "torch.int32"):
                raise ValueError("colors_out has to be (capacity, %d) int32" % LEVEL_COLOR_WORDS)
        elif colors_out.dtype != LEVEL_COLOR_DTYPE or colors_out.ndim != 1:
            raise ValueError("colors_out has to be a one-dimensional LEVEL_COLOR_DTYPE array")
        p, mem = _capi.contiguous_ptr(colors_out)
        check(lib().vsg_render_level_colors(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness), p_bgr,
                                            stride, mem_in, p, colors_out.shape[0], C.byref(n), mem))
        return colors_out[:n.value]

    def mean_frame(self, seg_bytes, level=0, frame=None, connectedness=0, out=None):
        """Hierarchy level `level` painted in the mean colours of its groups (level_colors' `mean`), then
        treated as render() treats its colour plane: edges, blend with `frame`, concatenation.  The
        out_rows x W x 3 uint8 picture: a numpy array, or a torch CUDA tensor when frame is one.  frame is
        needed whatever has_video.  out: a caller's buffer instead, as in render().  The level the renderer
        keeps for render() is neither resolved nor changed."""
        if frame is None:
            raise ValueError("frame is needed")
        p_bgr, stride, mem_in = _frame_ptr(frame, self.H, self.W, "frame")
        if out is None:
            if _capi.is_torch(frame) and frame.is_cuda:
                import torch
                out = torch.empty((self.out_rows, self.W, 3), dtype=torch.uint8, device=frame.device)
            else:
                out = np.empty((self.out_rows, self.W, 3), np.uint8)
        p_out, out_stride, mem_out = _frame_ptr(out, self.out_rows, self.W, "out")
        seg_bytes = bytes(seg_bytes)
        check(lib().vsg_render_mean_frame(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness), p_bgr,
                                          stride, mem_in, p_out, out_stride, mem_out))
        return out

    def last_color_stats(self):
        """vsg_render_last_color_stats of the last level_colors or mean_frame call, as a dict."""
        s = VsgRenderColorStats()
        check(lib().vsg_render_last_color_stats(self.h, C.byref(s)))
        return s.as_dict()

    def _feature_layout(self, x, what, dtype=None):
        """(pointer, dtype code, channels, chan_stride, row_stride, pixel_stride, mem kind) of a (C, H, W) or
        (H, W) float array or tensor, the layout read from its strides (in elements).  A ValueError for anything
        that is neither planar nor channels-last; never a copy."""
        name = str(x.dtype).replace("torch.", "")
        if dtype is not None:
            wanted = _POOL_DTYPES.get(str(dtype).replace("torch.", ""))
            if name == "uint16" and wanted == POOL_BF16:
                name = "bfloat16"
            elif wanted is None or _POOL_DTYPES.get(name) != wanted:
                raise TypeError("dtype= names the format of a uint16 array ('bf16'), or the array's own")
        if name not in _POOL_DTYPES:
            raise TypeError("%s has to be float32, float16 or bfloat16 (a uint16 array with dtype='bf16'), got %s"
                            % (what, name))
        shape = tuple(x.shape)
        if shape[-2:] != (self.H, self.W) or len(shape) not in (2, 3) or (len(shape) == 3 and shape[0] < 1):
            raise ValueError("%s has to be (C, %d, %d) or (%d, %d), got %s" % (what, self.H, self.W, self.H, self.W,
                                                                              shape))
        ptr, strides, mem = _capi._memory(x)
        if not _capi.is_torch(x):
            if any(s % x.itemsize for s in strides):
                raise ValueError("%s: strides have to be multiples of the element size" % what)
            strides = tuple(s // x.itemsize for s in strides)
        channels = shape[0] if len(shape) == 3 else 1
        cs = strides[0] if len(shape) == 3 else 0
        rs, ps = strides[-2:]
        if min(cs, rs, ps) < 0:
            raise ValueError("%s: negative strides are not accepted" % what)
        # the stride of an axis of length 1 says nothing
        if self.W == 1:
            ps = channels if (channels > 1 and cs == 1) else 1
        if channels == 1:
            cs = 1 if ps != 1 else self.H * max(rs, self.W)
        if self.H == 1:
            rs = (self.W - 1) * ps + channels if cs == 1 and ps != 1 else self.W
        if not (ps == 1 or (cs == 1 and ps >= channels)):
            raise ValueError("%s is neither planar (x stride 1) nor channels-last (channel stride 1, x stride >= C): "
                             "strides %s" % (what, (cs, rs, ps)))
        W, H = self.W, self.H
        if ps != 1:
            disjoint = H == 1 or rs >= (W - 1) * ps + channels
        else:
            disjoint = (H == 1 or rs >= W) and (channels == 1 or cs >= (H - 1) * rs + W
                                                or (cs >= W and (H == 1 or rs >= (channels - 1) * cs + W)))
        if not disjoint:
            raise ValueError("%s: rows or planes overlap or are not in (channel, row, x) order: strides %s"
                             % (what, (cs, rs, ps)))
        _capi._drain(x)
        return C.c_void_p(ptr), _POOL_DTYPES[name], channels, cs, rs, ps, mem

    def level_pool(self, seg_bytes, level=0, features=None, connectedness=0, stats=("sum",), dtype=None,
                   capacity=None):
        """A float feature map pooled by the groups of hierarchy level `level`: (groups, {name: matrix}).
        features: a (C, H, W) or (H, W) float32, float16 or bfloat16 array or tensor (numpy has no bfloat16: a
        uint16 array with dtype='bf16'), planar or channels-last as its strides say; anything else is a
        ValueError, never a silent copy.  stats: which of "sum", "sum_sq" (float64) and "min", "max" (float32)
        to compute, each an (R, C) matrix; record k belongs to record k of level_regions or level_components.
        groups: a POOL_GROUP_DTYPE array.  A torch CUDA tensor gives torch tensors on its device (groups as an
        (R, 4) int32 tensor), anything else numpy arrays.  Without capacity the count is asked for first and the
        outputs are allocated exactly; capacity: rows to allocate instead, which saves that call."""
        if features is None:
            raise ValueError("features are needed")
        stats = tuple(stats)
        if any(s not in POOL_STATS for s in stats):
            raise ValueError("stats has to be a subset of %s" % (POOL_STATS,))
        seg_bytes = bytes(seg_bytes)
        p, code, channels, cs, rs, ps, mem_in = self._feature_layout(features, "features", dtype)
        n = C.c_size_t()

        def call(groups, mats, cap, mem_out):
            check(lib().vsg_render_level_pool(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness), p,
                                              code, channels, cs, rs, ps, mem_in, groups, mats[0], mats[1], mats[2],
                                              mats[3], cap, C.byref(n), mem_out))

        if capacity is None:
            call(None, [None] * 4, 0, VSG_MEM_HOST)
            capacity = n.value
        on_device = _capi.is_torch(features) and features.is_cuda
        if on_device:
            import torch
            kinds = {"sum": torch.float64, "sum_sq": torch.float64, "min": torch.float32, "max": torch.float32}
            groups = torch.empty((capacity, POOL_GROUP_WORDS), dtype=torch.int32, device=features.device)
            out = {s: torch.empty((capacity, channels), dtype=kinds[s], device=features.device) for s in stats}
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None   # noqa: E731
            mem_out = VSG_MEM_DEVICE
        else:
            kinds = {"sum": np.float64, "sum_sq": np.float64, "min": np.float32, "max": np.float32}
            groups = np.empty(capacity, POOL_GROUP_DTYPE)
            out = {s: np.empty((capacity, channels), kinds[s]) for s in stats}
            ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None   # noqa: E731
            mem_out = VSG_MEM_HOST
        if capacity:
            call(ptr(groups), [ptr(out.get(s)) for s in POOL_STATS], capacity, mem_out)
        return groups[:n.value], {s: out[s][:n.value] for s in stats}

    def level_unpool(self, seg_bytes, level=0, values=None, connectedness=0, fill=0.0, out=None, dtype=None,
                     channels_last=False):
        """One value per group and channel painted back into feature planes: out[c, y, x] = values[k, c] for the
        group k of pixel (x, y), `fill` where there is none.  values: (R, C) float32, contiguous, numpy or torch;
        R has to be the number of groups of the level.  out: a (C, H, W) or (H, W) float32, float16 or bfloat16
        array or tensor to write, planar or channels-last as its strides say (only its own elements are written);
        without it a new one where values live: dtype "float32" (the default), "float16" or "bf16" (numpy: a
        uint16 array), channels_last choosing its memory layout.  Returns out."""
        if values is None:
            raise ValueError("values are needed")
        if len(values.shape) != 2 or str(values.dtype).replace("torch.", "") != "float32":
            raise ValueError("values has to be (R, C) float32")
        rows, channels = int(values.shape[0]), int(values.shape[1])
        p_val, mem_in = _capi.contiguous_ptr(values)
        if out is None:
            name = str(dtype or "float32").replace("torch.", "")
            if name not in _POOL_DTYPES:
                raise TypeError("dtype has to be float32, float16 or bf16")
            shape = (self.H, self.W, channels) if channels_last else (channels, self.H, self.W)
            if _capi.is_torch(values):
                import torch
                kind = {POOL_F32: torch.float32, POOL_F16: torch.float16, POOL_BF16: torch.bfloat16}[_POOL_DTYPES[name]]
                out = torch.empty(shape, dtype=kind, device=values.device)
                out = out.permute(2, 0, 1) if channels_last else out
                out_dtype = None
            else:
                kind = {POOL_F32: np.float32, POOL_F16: np.float16, POOL_BF16: np.uint16}[_POOL_DTYPES[name]]
                out = np.empty(shape, kind)
                out = out.transpose(2, 0, 1) if channels_last else out
                out_dtype = "bf16" if kind is np.uint16 else None
        else:
            out_dtype = dtype
        p_out, code, out_channels, cs, rs, ps, mem_out = self._feature_layout(out, "out", out_dtype)
        if out_channels != channels:
            raise ValueError("out has %d channels, values %d" % (out_channels, channels))
        seg_bytes = bytes(seg_bytes)
        check(lib().vsg_render_level_unpool(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                            p_val if rows else None, rows, channels, mem_in, float(fill), p_out, code,
                                            cs, rs, ps, mem_out))
        return out

    def last_pool_stats(self):
        """vsg_render_last_pool_stats of the last level_pool or level_unpool call, as a dict."""
        s = VsgRenderPoolStats()
        check(lib().vsg_render_last_pool_stats(self.h, C.byref(s)))
        return s.as_dict()

    def volume_begin(self, level=0, colors=False, labels=False):
        """Starts, or restarts and empties, the renderer's volume session: the table of the supervoxels (region ids)
        of hierarchy level `level` that volume_add merges every frame into on the device.  colors: every add
        brings the BGR24 frame and the rows carry the colour sums; labels: every add brings a label plane and
        the table has columns and pairs."""
        check(lib().vsg_render_volume_begin(self.h, int(level), int(bool(colors)), int(bool(labels))))

    def volume_add(self, seg_bytes, frame, bgr=None, other=None):
        """Adds the desc of frame index `frame` (>= 0, in any order; an index added twice counts twice) to the
        volume session.  bgr: the H x W x 3 uint8 frame as in level_colors, needed with colors; other: the
        H x W int32 label plane as in level_overlap, needed with labels.  Either is ignored when the session
        does not ask for it.  A failed add leaves the session as it was."""
        seg_bytes = bytes(seg_bytes)
        p_bgr, stride, mem_in = None, 0, VSG_MEM_HOST
        if bgr is not None:
            p_bgr, stride, mem_in = _frame_ptr(bgr, self.H, self.W, "bgr")
        po, pitch, mem_other = None, 0, VSG_MEM_HOST
        if other is not None:
            po, pitch, mem_other = self._other_ptr(other)
        check(lib().vsg_render_volume_add(self.h, seg_bytes, len(seg_bytes), int(frame), p_bgr, stride, mem_in, po,
                                          pitch, mem_other))

    def volume_table(self, rows_out=None, cols_out=None, pairs_out=None):
        """The volume session's table so far: (rows, cols, pairs).  rows: a VOLUME_ROW_DTYPE array, one per region
        id that painted a pixel in any added frame, ascending by id, with its life span, box, volume, sums of x,
        y and t, colour sums, its slice of `pairs` and the label it overlaps most; cols: a VOLUME_COL_DTYPE
        array, one per label by ascending label; pairs: a VOLUME_PAIR_DTYPE array, one per (id, label) with a
        common voxel, grouped by row, within a row by ascending label.  The session goes on.  Without outputs
        the arrays are allocated exactly.  rows_out / cols_out / pairs_out (all or none): buffers to fill
        instead, all numpy (arrays of the three dtypes) or all torch CUDA tensors ((capacity, 38), (capacity, 12)
        and (capacity, 6) int32); the filled parts of them are returned."""
        nr, nc, npairs = C.c_size_t(), C.c_size_t(), C.c_size_t()
        outs = (rows_out, cols_out, pairs_out)
        if any(o is None for o in outs) and not all(o is None for o in outs):
            raise ValueError("pass all three outputs or none")
        if rows_out is None:
            check(lib().vsg_render_volume_table(self.h, None, 0, C.byref(nr), None, 0, C.byref(nc), None, 0,
                                                C.byref(npairs), VSG_MEM_HOST))
            rows_out = np.empty(nr.value, VOLUME_ROW_DTYPE)
            cols_out = np.empty(nc.value, VOLUME_COL_DTYPE)
            pairs_out = np.empty(npairs.value, VOLUME_PAIR_DTYPE)
            if nr.value == 0 and nc.value == 0:
                return rows_out, cols_out, pairs_out
        outs = (rows_out, cols_out, pairs_out)
        if len({_capi.is_torch(o) for o in outs}) != 1:
            raise ValueError("all outputs have to be numpy arrays or all torch tensors")
        specs = (("rows_out", VOLUME_ROW_DTYPE, VOLUME_ROW_WORDS), ("cols_out", VOLUME_COL_DTYPE, VOLUME_COL_WORDS),
                 ("pairs_out", VOLUME_PAIR_DTYPE, VOLUME_PAIR_WORDS))
        for o, (name, dtype, words) in zip(outs, specs):
            if _capi.is_torch(o):
                if o.dim() != 2 or o.shape[1] != words or str(o.dtype) != "torch.int32":
                    raise ValueError("%s has to be (capacity, %d) int32" % (name, words))
            elif o.dtype != dtype or o.ndim != 1:
                raise ValueError("%s has to be a one-dimensional array of its dtype" % name)
        ptrs = [_capi.contiguous_ptr(o) for o in outs]
        if len({mem for _, mem in ptrs}) != 1:
            raise ValueError("all outputs have to be in the same kind of memory")
        check(lib().vsg_render_volume_table(self.h, ptrs[0][0], rows_out.shape[0], C.byref(nr), ptrs[1][0],
                                            cols_out.shape[0], C.byref(nc), ptrs[2][0], pairs_out.shape[0],
                                            C.byref(npairs), ptrs[0][1]))
        return rows_out[:nr.value], cols_out[:nc.value], pairs_out[:npairs.value]

    def last_volume_stats(self):
        """vsg_render_last_volume_stats: the volume session's totals and what its last add and table call did, as
        a dict."""
        s = VsgRenderVolumeStats()
        check(lib().vsg_render_last_volume_stats(self.h, C.byref(s)))
        return s.as_dict()

    def level_contours(self, seg_bytes, level=0, connectedness=0, contours_out=None, vertices_out=None):
        """The closed outlines of every region of hierarchy level `level` (connectedness 0) or of every connected
        component of its regions (N4 or N8), traced along the pixel sides: (contours, vertices).  contours: a
        LEVEL_CONTOUR_DTYPE array ordered by group, `group` being the index of the contour's region in
        level_regions (component in level_components), within a group by the key of the first turn; the first
        contour of a group is its outer one, holes have a negative area2.  vertices: (n, 2) int32 corners
        {x, y} of [0, W] x [0, H], grouped by contour in that order, clockwise on screen around the group, no
        three of them collinear.  Without outputs the counts are asked for first and both arrays are allocated
        exactly.  contours_out / vertices_out: buffers to fill instead, both numpy (a LEVEL_CONTOUR_DTYPE array
        and a (capacity, 2) int32 array) or both torch CUDA tensors ((capacity, 12) int32, area2 as two
        words, and (capacity, 2) int32); the filled parts of them are returned."""
        seg_bytes = bytes(seg_bytes)
        nc, nv = C.c_size_t(), C.c_size_t()
        if (contours_out is None) != (vertices_out is None):
            raise ValueError("pass both outputs or neither")
        if contours_out is None:
            check(lib().vsg_render_level_contours(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness),
                                                  None, 0, C.byref(nc), None, 0, C.byref(nv), VSG_MEM_HOST))
            contours_out = np.empty(nc.value, LEVEL_CONTOUR_DTYPE)
            vertices_out = np.empty((nv.value, 2), np.int32)
            if nc.value == 0:
                return contours_out, vertices_out
        if _capi.is_torch(contours_out) != _capi.is_torch(vertices_out):
            raise ValueError("both outputs have to be numpy arrays or both torch tensors")
        if _capi.is_torch(contours_out):
            if (contours_out.dim() != 2 or contours_out.shape[1] != LEVEL_CONTOUR_WORDS
                    or str(contours_out.dtype) != "torch.int32"):
                raise ValueError("contours_out has to be (capacity, %d) int32" % LEVEL_CONTOUR_WORDS)
        elif contours_out.dtype != LEVEL_CONTOUR_DTYPE or contours_out.ndim != 1:
            raise ValueError("contours_out has to be a one-dimensional LEVEL_CONTOUR_DTYPE array")
        if (len(vertices_out.shape) != 2 or vertices_out.shape[1] != 2
                or str(vertices_out.dtype).replace("torch.", "") != "int32"):
            raise ValueError("vertices_out has to be (capacity, 2) int32")
        pc, mem = _capi.contiguous_ptr(contours_out)
        pv, mem_v = _capi.contiguous_ptr(vertices_out)
        if mem != mem_v:
            raise ValueError("both outputs have to be in the same kind of memory")
        check(lib().vsg_render_level_contours(self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness), pc,
                                              contours_out.shape[0], C.byref(nc), pv, vertices_out.shape[0],
                                              C.byref(nv), mem))
        return contours_out[:nc.value], vertices_out[:nv.value]

    def last_contour_stats(self):
        """vsg_render_last_contour_stats of the last level_contours call, as a dict."""
        s = VsgRenderContourStats()
        check(lib().vsg_render_last_contour_stats(self.h, C.byref(s)))
        return s.as_dict()

    def level_mesh(self, seg_bytes, level=0, connectedness=0, segments_out=None, vertices_out=None, loops_out=None,
                   refs_out=None):
        """The shared-segment mesh of hierarchy level `level`: the contours of level_contours (same level, same
        connectedness) cut at the junction corners into segments, each stored once and shared by the two groups
        it separates: (segments, vertices, loops, refs).  segments: a MESH_SEGMENT_DTYPE array in (right, first
        crack) order, `right` and `left` being group indices as in level_contours, left = -1 for the frame and
        uncovered pixels.  vertices: (n, 2) int32 corners, grouped by segment, in the direction that has `right`
        on the right hand; open segments list both end corners.  loops: a MESH_LOOP_DTYPE array, loop c being
        contour c of level_contours.  refs: int32, grouped by loop in travel order: s is segment s forwards, ~s
        segment s backwards.  Without outputs the counts are asked for first and the arrays are allocated
        exactly.  *_out: buffers to fill instead, all four numpy (the two dtypes, (capacity, 2) int32 and
        (capacity,) int32) or all four torch CUDA int32 tensors ((capacity, 8), (capacity, 2), (capacity, 4),
        (capacity,)); the filled parts of them are returned.  See mesh_polygons and mesh_desc."""
        seg_bytes = bytes(seg_bytes)
        head = (self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness))
        return self._mesh_lists(lib().vsg_render_level_mesh, head, segments_out, vertices_out, loops_out, refs_out)

    @staticmethod
    def _mesh_lists(entry, head, segments_out, vertices_out, loops_out, refs_out):
        """The four lists of a mesh entry point: `entry(*head, <the lists>, mem_out)`."""
        ns, nv, nl, nr = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        outs = (segments_out, vertices_out, loops_out, refs_out)
        if any(o is None for o in outs) and not all(o is None for o in outs):
            raise ValueError("pass all four outputs or none")
        if segments_out is None:
            check(entry(*head, None, 0, C.byref(ns), None, 0, C.byref(nv), None, 0, C.byref(nl),
                        None, 0, C.byref(nr), VSG_MEM_HOST))
            segments_out = np.empty(ns.value, MESH_SEGMENT_DTYPE)
            vertices_out = np.empty((nv.value, 2), np.int32)
            loops_out = np.empty(nl.value, MESH_LOOP_DTYPE)
            refs_out = np.empty(nr.value, np.int32)
            if ns.value == 0:
                return segments_out, vertices_out, loops_out, refs_out
            outs = (segments_out, vertices_out, loops_out, refs_out)
        if len({_capi.is_torch(o) for o in outs}) != 1:
            raise ValueError("all outputs have to be numpy arrays or all torch tensors")
        if _capi.is_torch(segments_out):
            for o, words, name in ((segments_out, MESH_SEGMENT_WORDS, "segments_out"),
                                   (loops_out, MESH_LOOP_WORDS, "loops_out")):
                if o.dim() != 2 or o.shape[1] != words or str(o.dtype) != "torch.int32":
                    raise ValueError("%s has to be (capacity, %d) int32" % (name, words))
        else:
            if segments_out.dtype != MESH_SEGMENT_DTYPE or segments_out.ndim != 1:
                raise ValueError("segments_out has to be a one-dimensional MESH_SEGMENT_DTYPE array")
            if loops_out.dtype != MESH_LOOP_DTYPE or loops_out.ndim != 1:
                raise ValueError("loops_out has to be a one-dimensional MESH_LOOP_DTYPE array")
        if (len(vertices_out.shape) != 2 or vertices_out.shape[1] != 2
                or str(vertices_out.dtype).replace("torch.", "") != "int32"):
            raise ValueError("vertices_out has to be (capacity, 2) int32")
        if len(refs_out.shape) != 1 or str(refs_out.dtype).replace("torch.", "") != "int32":
            raise ValueError("refs_out has to be (capacity,) int32")
        ptrs = [_capi.contiguous_ptr(o) for o in outs]
        if len({mem for _, mem in ptrs}) != 1:
            raise ValueError("all outputs have to be in the same kind of memory")
        check(entry(*head, ptrs[0][0], segments_out.shape[0], C.byref(ns), ptrs[1][0], vertices_out.shape[0],
                    C.byref(nv), ptrs[2][0], loops_out.shape[0], C.byref(nl), ptrs[3][0], refs_out.shape[0],
                    C.byref(nr), ptrs[0][1]))
        return segments_out[:ns.value], vertices_out[:nv.value], loops_out[:nl.value], refs_out[:nr.value]

    def last_mesh_stats(self):
        """vsg_render_last_mesh_stats of the last level_mesh call, as a dict."""
        s = VsgRenderMeshStats()
        check(lib().vsg_render_last_mesh_stats(self.h, C.byref(s)))
        return s.as_dict()

    def level_mesh_simplified(self, seg_bytes, level=0, connectedness=0, max_error=1.0, min_segment_points=4,
                              segments_out=None, vertices_out=None, loops_out=None, refs_out=None):
        """level_mesh with every segment's vertex list simplified on the device as the reference's
        ComputeVectorization does: an open segment of fewer than max(3, min_segment_points) lattice points
        (min_segment_points = 0: none) becomes its two end corners, every other segment goes through
        Douglas-Peucker (OpenCV 2.4's approxPolyDP for integer points) at max_error.  Segments, loops and refs
        are those of level_mesh; only the vertices and the records' first_vertex / num_vertices differ.  An open
        segment keeps both end corners; a closed one may come back rotated, and as a single vertex.  Outputs as
        for level_mesh.  See mesh_polygons and simplified_mesh_desc."""
        seg_bytes = bytes(seg_bytes)
        head = (self.h, seg_bytes, len(seg_bytes), int(level), int(connectedness), float(max_error),
                int(min_segment_points))
        return self._mesh_lists(lib().vsg_render_level_mesh_simplified, head, segments_out, vertices_out, loops_out,
                                refs_out)

    def last_simplify_stats(self):
        """vsg_render_last_simplify_stats of the last level_mesh_simplified call, as a dict."""
        s = VsgRenderSimplifyStats()
        check(lib().vsg_render_last_simplify_stats(self.h, C.byref(s)))
        return s.as_dict()

    def boundary_distance(self, seg_bytes, level=0, out=None):
        """The exact squared Euclidean distance from every pixel to the nearest edge pixel of hierarchy level
        `level`: H x W int32, 0 exactly where id_image(seg, level) differs from its right or below neighbour,
        DISTANCE_NONE everywhere when the level has no edge.  out: a contiguous int32 numpy array or torch CUDA
        tensor to fill instead of a new numpy array."""
        if out is None:
            out = np.empty((self.H, self.W), np.int32)
        if tuple(out.shape) != (self.H, self.W) or str(out.dtype).replace("torch.", "") != "int32":
            raise ValueError("out has to be %d x %d int32" % (self.H, self.W))
        p, mem = _capi.contiguous_ptr(out)
        seg_bytes = bytes(seg_bytes)
        check(lib().vsg_render_boundary_distance(self.h, seg_bytes, len(seg_bytes), int(level), p, mem))
        return out

    def boundary_benchmark(self, seg_bytes, other, tolerance_sq, out=None):
        """What a boundary benchmark counts at every level of the desc's hierarchy against the label plane
        `other` (as in level_overlap; all negative values are one void label), boundaries matching within
        sqrt(tolerance_sq) pixels: a BOUNDARY_SCORE_DTYPE array with one record per level, seg_edges and
        seg_matched (the level's edge pixels, and those near an edge of `other`), gt_edges and gt_matched (the
        edge pixels of `other`, and those near an edge of the level).  tolerance_sq: an integer in
        [0, MAX_TOLERANCE_SQ].  out: a buffer to fill instead, a BOUNDARY_SCORE_DTYPE array or a (capacity, 4)
        int64 torch CUDA tensor; the filled part of it is returned.  See boundary_scores."""
        if other is None:
            raise ValueError("other is needed")
        seg_bytes = bytes(seg_bytes)
        po, pitch, mem_other = self._other_ptr(other)
        nl = C.c_size_t()
        if out is None:
            # one call when the guess holds: a call that finds its capacity too small has already painted the
            # persistence plane and classified `other`, most of its cost, and says how many levels there are
            guess = np.empty(max(getattr(self, "_benchmark_levels", 0), 32), BOUNDARY_SCORE_DTYPE)
            p, mem = _capi.contiguous_ptr(guess)
            rc = lib().vsg_render_boundary_benchmark(self.h, seg_bytes, len(seg_bytes), po, pitch, mem_other,
                                                     int(tolerance_sq), p, guess.shape[0], C.byref(nl), mem)
            if rc == VSG_OK or nl.value <= guess.shape[0]:
                check(rc)
                self._benchmark_levels = nl.value
                return guess[:nl.value].copy()
            self._benchmark_levels = nl.value
            out = np.empty(nl.value, BOUNDARY_SCORE_DTYPE)
        if _capi.is_torch(out):
            if out.dim() != 2 or out.shape[1] != BOUNDARY_SCORE_WORDS or str(out.dtype) != "torch.int64":
                raise ValueError("out has to be (capacity, %d) int64" % BOUNDARY_SCORE_WORDS)
        elif out.dtype != BOUNDARY_SCORE_DTYPE or out.ndim != 1:
            raise ValueError("out has to be a one-dimensional BOUNDARY_SCORE_DTYPE array")
        p, mem = _capi.contiguous_ptr(out)
        check(lib().vsg_render_boundary_benchmark(self.h, seg_bytes, len(seg_bytes), po, pitch, mem_other,
                                                  int(tolerance_sq), p, out.shape[0], C.byref(nl), mem))
        return out[:nl.value]

    def last_distance_stats(self):
        """vsg_render_last_distance_stats of the last boundary_distance / boundary_benchmark call, as a dict."""
        s = VsgRenderDistanceStats()
        check(lib().vsg_render_last_distance_stats(self.h, C.byref(s)))
        return s.as_dict()

    def tree_cut(self, seg_bytes, labels=None, penalty=0, gains=None, plane=True, nodes_out=None, plane_out=None):
        """The best non-horizontal cut of the desc's hierarchy: (nodes, plane, total).  Exactly one source of
        gains: labels, an H x W int32 plane as level_overlap's `other` (a node gains the pixels it shares with
        its best label, minus penalty), or gains, a CUT_GAIN_DTYPE array (or a torch CUDA (n, 4) int32 tensor
        of the same bytes) strictly ascending by (level, id).  nodes: a CUT_NODE_DTYPE array, one record per
        selected node by ascending (level, id); plane: H x W int32, the index of the record that covers each
        pixel, -1 where no region is, or None with plane=False; total: the sum of the selected nodes' gains.
        Without outputs the count is asked for first and the arrays are allocated exactly.  nodes_out (and
        plane_out when a plane is wanted): buffers to fill instead, both numpy or both torch CUDA tensors
        ((capacity, 12) int32 and H x W int32); the filled part of nodes_out is returned."""
        seg_bytes = bytes(seg_bytes)
        p_labels, pitch, mem_labels = None, 0, VSG_MEM_HOST
        if labels is not None:
            p_labels, pitch, mem_labels = self._other_ptr(labels)
        p_gains, n_gains, mem_gains = None, 0, VSG_MEM_HOST
        keep = None
        if gains is not None:
            if _capi.is_torch(gains):
                if gains.dim() != 2 or gains.shape[1] != CUT_GAIN_WORDS or str(gains.dtype) != "torch.int32":
                    raise ValueError("gains has to be (n, %d) int32" % CUT_GAIN_WORDS)
            elif gains.dtype != CUT_GAIN_DTYPE or gains.ndim != 1:
                raise ValueError("gains has to be a one-dimensional CUT_GAIN_DTYPE array")
            n_gains = int(gains.shape[0])
            if n_gains == 0:
                keep = np.zeros(1, CUT_GAIN_DTYPE)    # an empty table still says "a gain table"
                p_gains, mem_gains = _capi.contiguous_ptr(keep)
            else:
                p_gains, mem_gains = _capi.contiguous_ptr(gains)
        args = (self.h, seg_bytes, len(seg_bytes), p_labels, pitch, mem_labels, int(penalty), p_gains, n_gains,
                mem_gains)
        n, total = C.c_size_t(), C.c_int64()
        if nodes_out is None:
            if plane_out is not None:
                raise ValueError("pass nodes_out with plane_out")
            check(lib().vsg_render_tree_cut(*args, None, 0, C.byref(n), None, C.byref(total), VSG_MEM_HOST))
            nodes_out = np.empty(n.value, CUT_NODE_DTYPE)
            if plane:
                plane_out = np.empty((self.H, self.W), np.int32)
        elif plane and plane_out is None:
            raise ValueError("pass plane_out with nodes_out, or plane=False")
        if _capi.is_torch(nodes_out):
            if nodes_out.dim() != 2 or nodes_out.shape[1] != CUT_NODE_WORDS or str(nodes_out.dtype) != "torch.int32":
                raise ValueError("nodes_out has to be (capacity, %d) int32" % CUT_NODE_WORDS)
        elif nodes_out.dtype != CUT_NODE_DTYPE or nodes_out.ndim != 1:
            raise ValueError("nodes_out has to be a one-dimensional CUT_NODE_DTYPE array")
        p_nodes, mem_out = _capi.contiguous_ptr(nodes_out)
        p_plane = None
        if plane:
            if tuple(plane_out.shape) != (self.H, self.W) or str(plane_out.dtype).replace("torch.", "") != "int32":
                raise ValueError("plane_out has to be %d x %d int32" % (self.H, self.W))
            p_plane, mem_plane = _capi.contiguous_ptr(plane_out)
            if mem_plane != mem_out:
                raise ValueError("all outputs have to be in the same kind of memory")
        else:
            plane_out = None
        check(lib().vsg_render_tree_cut(*args, p_nodes, nodes_out.shape[0], C.byref(n), p_plane, C.byref(total),
                                        mem_out))
        return nodes_out[:n.value], plane_out, total.value

    def tree_cut_tuning(self, block_nodes=-1):
        """The threshold between tree_cut's two DP paths: one workgroup up to block_nodes tree nodes, a launch
        per level above.  0: always per level; CUT_BLOCK_ALWAYS: always one workgroup; -1: the default."""
        check(lib().vsg_render_tree_cut_tuning(self.h, int(block_nodes)))

    def last_cut_stats(self):
        """vsg_render_last_cut_stats of the last tree_cut call, as a dict."""
        s = VsgRenderCutStats()
        check(lib().vsg_render_last_cut_stats(self.h, C.byref(s)))
        return s.as_dict()

    def last_vector_stats(self):
        """vsg_render_last_vector_stats of the last call, as a dict."""
        s = VsgRenderVectorStats()
        check(lib().vsg_render_last_vector_stats(self.h, C.byref(s)))
        return s.as_dict()

    def last_stats(self):
        """vsg_render_last_stats of the last render / id_image call, as a dict."""
        s = VsgRenderStats()
        check(lib().vsg_render_last_stats(self.h, C.byref(s)))
        return s.as_dict()


def overlap_scores(rows, pairs):
    """The two scores every evaluation of this algorithm reports, from the host arrays of level_overlap, with
    N = the sum of pairs.count (the pixels both covered and labelled): a dict of the integers
    n, asa_sum = the sum of rows.best_count and ue_sum = the sum over the pairs of
    min(count, (row.area - row.unlabelled) - count), and the float64 quotients
    asa (achievable segmentation accuracy) = asa_sum / n and
    ue (undersegmentation error, Neubert-Protzel) = ue_sum / n; both None when n == 0.  Host numpy only."""
    rows, pairs = np.asarray(rows), np.asarray(pairs)
    count = pairs["count"].astype(np.int64)
    n = int(count.sum())
    asa_sum = int(rows["best_count"].astype(np.int64).sum())
    inside = (rows["area"].astype(np.int64) - rows["unlabelled"])[pairs["row"]]
    ue_sum = int(np.minimum(count, inside - count).sum())
    return {"n": n, "asa_sum": asa_sum, "ue_sum": ue_sum,
            "asa": asa_sum / n if n else None, "ue": ue_sum / n if n else None}


def cut_scores(nodes):
    """What a cut amounts to: {"nodes", "best_sum" (the sum of best_count: the numerator of the achievable
    segmentation accuracy of the cut), "per_level" (level -> number of selected nodes)}."""
    nodes = np.asarray(nodes)
    levels, counts = np.unique(nodes["level"], return_counts=True)
    return {"nodes": int(len(nodes)), "best_sum": int(nodes["best_count"].astype(np.int64).sum()),
            "per_level": {int(l): int(c) for l, c in zip(levels, counts)}}


def tree_cut_for_count(renderer, seg_bytes, labels, max_nodes):
    """The smallest penalty whose cut of `labels` has at most max_nodes nodes: (penalty, nodes, plane, total).
    The cuts are nested (the node count never rises with the penalty), so the penalty is found by bisection
    over [0, 2^32].  When even the top level has more nodes, that cut (penalty 2^32) is returned."""
    def count(penalty):
        nodes, _, _ = renderer.tree_cut(seg_bytes, labels=labels, penalty=penalty, plane=False)
        return len(nodes)
    lo, hi = 0, CUT_MAX_PENALTY
    if count(lo) > max_nodes:
        while hi - lo > 1:        # count(lo) > max_nodes; count(hi) <= max_nodes, or hi is the end
            mid = (lo + hi) // 2
            if count(mid) > max_nodes:
                lo = mid
            else:
                hi = mid
    else:
        hi = 0
    nodes, plane, total = renderer.tree_cut(seg_bytes, labels=labels, penalty=hi)
    return hi, nodes, plane, total


def volume_scores(rows, cols, pairs):
    """The scores supervoxel benchmarks report, from the host arrays of volume_table, as Python floats (None
    where the denominator is 0), with N = the sum of pairs.count (the voxels both covered and labelled):
    ue_3d, the 3-D undersegmentation error (Neubert-Protzel): the sum over the pairs of
    min(count, (row.volume - row.unlabelled) - count), over N;
    sa_3d, the 3-D segmentation accuracy: the mean over the columns with a pair of (the sum of the counts of its
    pairs whose row has that column's label as best_label) / (col.volume - col.uncovered);
    mean_duration: the mean over the rows of `frames`;
    explained_variation: the mean over the three channels of
    sum over rows of volume * (row mean - global mean)^2 / sum over voxels of (value - global mean)^2, from the
    colour sums (None for a session without colours or without variance).
    The integers n, ue_sum and supervoxels are returned as well.  Host numpy only."""
    rows, cols, pairs = np.asarray(rows), np.asarray(cols), np.asarray(pairs)
    count = pairs["count"].astype(np.int64)
    n = int(count.sum())
    inside = (rows["volume"] - rows["unlabelled"]).astype(np.int64)[pairs["row"]] if len(pairs) else count
    ue_sum = int(np.minimum(count, inside - count).sum())
    sa = None
    if len(pairs):
        right = rows["best_label"][pairs["row"]] == pairs["label"]
        hit = np.bincount(pairs["col"][right], weights=count[right].astype(np.float64), minlength=len(cols))
        covered = (cols["volume"] - cols["uncovered"]).astype(np.float64)
        with_pair = covered > 0
        sa = float(np.mean(hit[with_pair] / covered[with_pair])) if with_pair.any() else None
    ev = None
    volume = rows["volume"].astype(np.float64)
    total = float(volume.sum())
    if total > 0 and rows["sum_sq"].any():
        s1 = rows["sum"].astype(np.float64)
        mean = s1.sum(axis=0) / total
        between = (s1 * s1 / volume[:, None]).sum(axis=0) - total * mean * mean
        whole = rows["sum_sq"].astype(np.float64).sum(axis=0) - total * mean * mean
        ok = whole > 0
        ev = float(np.mean(between[ok] / whole[ok])) if ok.any() else None
    return {"n": n, "ue_sum": ue_sum, "supervoxels": int(len(rows)),
            "ue_3d": ue_sum / n if n else None, "sa_3d": sa,
            "mean_duration": float(rows["frames"].mean()) if len(rows) else None,
            "explained_variation": ev}


def boundary_scores(scores):
    """Boundary precision, recall and F of every level from the host array of boundary_benchmark: a dict of the
    float64 arrays precision = seg_matched / seg_edges, recall = gt_matched / gt_edges and
    f = 2 precision recall / (precision + recall), each 0 where its denominator is 0, and best_level, the
    lowest level with the largest f (None without a level).  Host numpy only."""
    scores = np.asarray(scores)

    def quotient(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        return np.divide(a, b, out=np.zeros(a.shape, np.float64), where=b != 0)

    precision = quotient(scores["seg_matched"], scores["seg_edges"])
    recall = quotient(scores["gt_matched"], scores["gt_edges"])
    f = quotient(2 * precision * recall, precision + recall)
    return {"precision": precision, "recall": recall, "f": f,
            "best_level": int(np.argmax(f)) if len(f) else None}


def color_moments(records):
    """(mean, variance) of every record of level_colors, two (n, 3) float64 arrays in B, G, R order:
    sum / area and sum_sq / area - (sum / area)^2 (the population variance; never below 0).  Host numpy only."""
    records = np.asarray(records)
    area = records["area"].astype(np.float64)[:, None]
    mean = records["sum"].astype(np.float64) / area
    variance = np.maximum(records["sum_sq"].astype(np.float64) / area - mean * mean, 0.0)
    return mean, variance


def pool_moments(groups, sum, sum_sq):
    """(mean, variance) of every group and channel of level_pool, two (R, C) float64 arrays: sum / area and
    sum_sq / area - (sum / area)^2 (the population variance; never below 0).  Host numpy only."""
    groups = np.asarray(groups)
    area = groups["area"].astype(np.float64)[:, None]
    mean = np.asarray(sum, np.float64) / area
    variance = np.maximum(np.asarray(sum_sq, np.float64) / area - mean * mean, 0.0)
    return mean, variance


def region_pool(renderer, seg_bytes, level=0, connectedness=0):
    """(pool, unpool) of one frame's segmentation at one level for use in a torch model, both differentiable:
    pool maps (C, H, W) float32 CUDA features to the (R, C) float32 means of the R groups, unpool maps (R, C)
    values to the (C, H, W) planes that hold every pixel's group value (0 where there is no group).  The
    backward of pool is the unpool of grad / area, the backward of unpool the pooled sum of grad: the two calls
    of SegmentationRenderer are all there is to it."""
    import torch
    seg_bytes = bytes(seg_bytes)

    def sums(x):
        x = x.detach()
        try:   # a gradient may be a broadcast view (a stride of 0) or anything else that is no layout: copy it
            renderer._feature_layout(x, "features")
        except ValueError:
            x = x.contiguous()
        groups, out = renderer.level_pool(seg_bytes, level, x, connectedness, ("sum",))
        return groups[:, 2:3].to(torch.float64), out["sum"]

    def paint(values):
        return renderer.level_unpool(seg_bytes, level, values.detach().contiguous(), connectedness)

    class Pool(torch.autograd.Function):
        @staticmethod
        def forward(ctx, features):
            area, total = sums(features)
            ctx.save_for_backward(area)
            return (total / area).to(torch.float32)

        @staticmethod
        def backward(ctx, grad):
            area, = ctx.saved_tensors
            return paint(grad.to(torch.float32) / area.to(torch.float32))

    class Unpool(torch.autograd.Function):
        @staticmethod
        def forward(ctx, values):
            return paint(values.to(torch.float32))

        @staticmethod
        def backward(ctx, grad):
            return sums(grad.to(torch.float32))[1].to(torch.float32)

    return Pool.apply, Unpool.apply


def contour_polygons(contours, vertices):
    """The host arrays of level_contours as polygons: a list with one entry per group, in group order, each the
    list of that group's (n, 2) int32 vertex arrays (views of `vertices`), the outer contour first.  Host
    numpy only."""
    contours, vertices = np.asarray(contours), np.asarray(vertices)
    groups = [[] for _ in range(int(contours["group"].max()) + 1 if len(contours) else 0)]
    for c in contours:
        groups[int(c["group"])].append(vertices[int(c["first_vertex"]):int(c["first_vertex"]) + int(c["num_vertices"])])
    return groups


def _loop_points(segments, vertices, loop, refs):
    """The closed vertex list of one loop as a list of (x, y): its refs joined, every joint once."""
    points = []
    for ref in refs[int(loop["first_ref"]):int(loop["first_ref"]) + int(loop["num_refs"])]:
        ref = int(ref)
        seg = segments[ref if ref >= 0 else ~ref]
        part = vertices[int(seg["first_vertex"]):int(seg["first_vertex"]) + int(seg["num_vertices"])].tolist()
        if ref < 0:
            part.reverse()
        points += part if seg["closed"] else part[:-1]      # an open segment ends where the next ref begins
    return points


def mesh_polygons(segments, vertices, loops, refs):
    """The host arrays of level_mesh as polygons: a list with one entry per group, in group order, each the list
    of that group's (n, 2) int32 vertex arrays, one per loop in loop order.  Every loop is rebuilt from its refs:
    joints listed once, collinear corners dropped, rotated to begin at the start corner of its turn crack of
    smallest key, so that the result equals contour_polygons of the level_contours call.  The arrays of
    level_mesh_simplified are taken as well: a point repeated at a joint is listed once, a point on the straight
    line between its neighbours is dropped, and an oblique edge counts as the side whose quadrant its direction
    lies in (0: x grows and y does not fall, 1: y grows and x does not grow, 2: x falls and y does not grow, 3: y
    falls and x does not fall), which for the edges of level_mesh is their side.  A loop that is left with fewer
    than three points is returned as it is.  Host numpy only."""
    segments, vertices, loops, refs = (np.asarray(a) for a in (segments, vertices, loops, refs))
    groups = [[] for _ in range(int(loops["group"].max()) + 1 if len(loops) else 0)]
    start = ((0, 0), (1, 0), (1, 1), (0, 1))

    def side_of(a, b):
        dx, dy = b[0] - a[0], b[1] - a[1]
        return 0 if dx > 0 and dy >= 0 else 1 if dy > 0 else 2 if dx < 0 else 3

    def straight(a, b, c):
        """b lies between a and c on one line."""
        return ((b[0] - a[0]) * (c[1] - b[1]) == (b[1] - a[1]) * (c[0] - b[0])
                and (b[0] - a[0]) * (c[0] - b[0]) + (b[1] - a[1]) * (c[1] - b[1]) > 0)

    for loop in loops:
        pts = _loop_points(segments, vertices, loop, refs)
        pts = [p for k, p in enumerate(pts) if len(pts) == 1 or p != pts[k - 1]]
        n = len(pts)
        if n >= 3:
            pts = [pts[k] for k in range(n) if not straight(pts[k - 1], pts[k], pts[(k + 1) % n])]
            n = len(pts)
        first = 0
        if n >= 3:
            # the crack that starts at corner k: side s of pixel corner - start[s]; keys order like (y, x, s)
            keys = []
            for k in range(n):
                s = side_of(pts[k], pts[(k + 1) % n])
                keys.append((pts[k][1] - start[s][1], pts[k][0] - start[s][0], s))
            first = keys.index(min(keys))
        groups[int(loop["group"])].append(np.asarray(pts[first:] + pts[:first], np.int32).reshape(-1, 2))
    return groups


def _varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _field(number, payload):
    """A length-delimited field."""
    return _varint(number << 3 | 2) + _varint(len(payload)) + payload


def mesh_desc(width, height, group_ids, segments, vertices, loops, refs):
    """The host arrays of level_mesh as the bytes of a vector-only SegmentationDesc of width x height:
    frame_width / frame_height, rasterization_removed, one vector_mesh in which every distinct corner occurs
    once, one Region2D per distinct id of group_ids (the region id of every group index, e.g. the `id` column
    of level_regions or level_components) in ascending id order, its vectorization holding one polygon per
    loop of its groups, the first point repeated at the end, `hole` set where the loop's area is negative.
    rasterize() of the same size scan-converts it back to the level's id plane.  Host numpy only."""
    polygons = mesh_polygons(segments, vertices, loops, refs)
    group_ids = [int(i) for i in np.asarray(group_ids).tolist()]
    if len(polygons) > len(group_ids):
        raise ValueError("group_ids has fewer entries than the loops have groups")
    index = {}
    coord = []
    by_id = {}
    for g, polys in enumerate(polygons):
        for pts in polys:
            pts = pts.tolist()
            area2 = sum(pts[k][0] * pts[(k + 1) % len(pts)][1] - pts[(k + 1) % len(pts)][0] * pts[k][1]
                        for k in range(len(pts)))
            idx = []
            for x, y in pts + pts[:1]:
                if (x, y) not in index:
                    index[(x, y)] = len(coord)
                    coord += [float(x), float(y)]
                idx.append(index[(x, y)])
            polygon = _field(1, b"".join(_varint(i) for i in idx))           # Polygon.coord_idx, packed
            if area2 < 0:
                polygon += _varint(2 << 3) + _varint(1)                       # Polygon.hole
            by_id.setdefault(group_ids[g], []).append(_field(1, polygon))    # Vectorization.polygon
    out = bytearray()
    for rid in sorted(by_id):
        region = _varint(1 << 3) + _varint(rid) + _field(6, b"".join(by_id[rid]))   # Region2D.id, .vectorization
        out += _field(2, region)                                             # SegmentationDesc.region
    out += _varint(4 << 3) + _varint(int(width)) + _varint(5 << 3) + _varint(int(height))
    out += _field(11, _field(1, np.asarray(coord, "<f4").tobytes()))         # vector_mesh.coord, packed
    out += _varint(13 << 3) + _varint(1)                                     # rasterization_removed
    return bytes(out)


def simplified_mesh_desc(width, height, group_ids, segments, vertices, loops, refs):
    """mesh_desc for the host arrays of level_mesh_simplified.  The loops whose polygon has fewer than three
    distinct vertices are dropped first (the reference drops polygon.size() == 3 && polygon[0] == polygon[2]): a
    closed segment that came back as one vertex, a loop of collapsed segments.  Then mesh_desc is called with the
    loops that are left.  For the arrays of level_mesh itself the result is mesh_desc's, byte for byte; for
    level_mesh_simplified at max_error 0 without a collapse, rasterize() of the same size gives the level's id
    plane back; at a larger max_error it gives the simplified partition.  Host numpy only."""
    segments, vertices, loops, refs = (np.asarray(a) for a in (segments, vertices, loops, refs))
    keep = [len({tuple(p) for p in _loop_points(segments, vertices, loop, refs)}) >= 3 for loop in loops]
    return mesh_desc(width, height, group_ids, segments, vertices, loops[np.asarray(keep, bool)], refs)
