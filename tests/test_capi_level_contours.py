"""The level contour additions to the renderer's C ABI: vsg_render_level_contours and
vsg_render_last_contour_stats are declared in include/vsg_render.h with the documented signatures and structs,
exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vsg_render_level_contours", "vsg_render_last_contour_stats")


@pytest.fixture(scope="module")
def raw_header():
    with open(os.path.join(ROOT, "include", "vsg_render.h")) as f:
        return f.read()


@pytest.fixture(scope="module")
def header(raw_header):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw_header, flags=re.S))


def fields_of(header, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header)
    assert m, name
    return [f.strip() for f in m.group(1).split(";") if f.strip()]


def test_header_declares_the_documented_signatures_and_structs(header):
    assert ("int vsg_render_level_contours(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, vsg_render_level_contour* contours, size_t capacity_contours, "
            "size_t* num_contours, int32_t* vertices, size_t capacity_vertices, size_t* num_vertices, "
            "int mem_out);") in header
    assert "int vsg_render_last_contour_stats(vsg_render* h, vsg_render_contour_stats* s);" in header
    assert "typedef struct vsg_render_level_contour {" in header
    assert fields_of(header, "vsg_render_level_contour") == [
        "int32_t id", "int32_t component", "int32_t group", "int32_t first_vertex", "int32_t num_vertices",
        "int32_t length", "int32_t min_x, min_y, max_x, max_y", "int64_t area2"]
    assert fields_of(header, "vsg_render_contour_stats") == [
        "int64_t cracks, vertices, contours, holes, largest_contour_cracks",
        "float plane_us, classify_us, trace_us, table_us", "int rounds, launches"]


def test_header_states_the_definition(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("The plane.", "Cracks.", "Successor.", "Vertices.", "Order.",
                   "P is the plane of vsg_render_level_boundaries",
                   "0 top, 1 right, 2 bottom, 3 left",
                   "key = 4 (y W + x) + side",
                   "g is always on the right hand of the direction of travel",
                   "right turn (the next side of the same pixel), straight on",
                   "At a saddle corner",
                   "The successor map is a permutation of the cracks; its cycles are the contours",
                   "beginning with the turn crack of smallest key",
                   "Collinear corners are never listed",
                   "an even number of at least 4 vertices",
                   "within a group by the key of their first turn crack",
                   "neither output is touched",
                   "asks for the counts only",
                   "answered before the handle is dereferenced",
                   "A frame with no covered pixel returns zero contours and zero vertices",
                   "The call neither resolves nor changes the level the handle keeps for vsg_render_frame",
                   "is refused with VSG_ERR_INVALID"):
        assert phrase in text, phrase
    # the "Not offered" paragraph names the new call and what is still missing, and keeps what earlier tests pin
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    assert "Not offered" in head and "vsg_render_level_contours" in head
    assert "shared-segment mesh" in head and "approxPolyDP" in head
    for phrase in ("Lab histograms", "ground truth", "vsg_render_level_regions", "vsg_render_level_components",
                   "vsg_render_level_boundaries", "vsg_render_level_adjacency", "vsg_render_level_overlap",
                   "vsg_render_persistence_image", "vsg_render_persistence_frame", "vsg_render_persistence_graph",
                   "vsg_render_level_colors", "vsg_render_mean_frame", "draw_shape_descriptors"):
        assert phrase in head, phrase


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** h);",
            "int vsg_render_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, "
            "size_t stride, int mem_in, uint8_t* out, size_t out_stride, int mem_out);",
            "int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);",
            "int vsg_render_level_regions(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "vsg_render_level_region* regions, size_t capacity_regions, size_t* num_regions, "
            "int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int mem_out);",
            "int vsg_render_level_components(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, vsg_render_level_component* components, size_t capacity_components, "
            "size_t* num_components, int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, "
            "int32_t* label_image, int mem_out);",
            "int vsg_render_level_boundaries(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, int which, vsg_render_level_boundary* boundaries, size_t capacity_boundaries, "
            "size_t* num_boundaries, int32_t* points, size_t capacity_points, size_t* num_points, int mem_out);",
            "int vsg_render_level_adjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes, "
            "size_t* num_nodes, vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges, "
            "int mem_out);",
            "int vsg_render_level_colors(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const uint8_t* bgr, size_t stride, int mem_in, "
            "vsg_render_level_color* colors, size_t capacity_colors, size_t* num_colors, int mem_out);",
            "int vsg_render_last_color_stats(vsg_render* h, vsg_render_color_stats* s);",
            "int vsg_render_last_boundary_stats(vsg_render* h, vsg_render_boundary_stats* s);",
            "int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s);",
            "void vsg_render_color(int region_id, uint8_t c[3]);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in NAMES:
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_level_contours.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t,
                                                    psz, vp, C.c_size_t, psz, C.c_int]
    assert L.vsg_render_last_contour_stats.argtypes == [vp, C.POINTER(render.VsgRenderContourStats)]
    for method in ("level_contours", "last_contour_stats"):
        assert hasattr(render.SegmentationRenderer, method)
    assert callable(render.contour_polygons)


def test_stats_struct_layout():
    from video_segment_amd import render
    s = render.VsgRenderContourStats
    assert [n for n, _ in s._fields_] == ["cracks", "vertices", "contours", "holes", "largest_contour_cracks",
                                          "plane_us", "classify_us", "trace_us", "table_us", "rounds", "launches"]
    assert C.sizeof(s) == 64
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]


def test_record_is_48_bytes_with_the_documented_offsets():
    from video_segment_amd import render
    import level_contours_model as tm
    d = render.LEVEL_CONTOUR_DTYPE
    assert d == tm.CONTOUR_DTYPE and d.itemsize == 48 and render.LEVEL_CONTOUR_WORDS == 12
    assert {n: d.fields[n][1] for n in d.names} == {
        "id": 0, "component": 4, "group": 8, "first_vertex": 12, "num_vertices": 16, "length": 20, "min_x": 24,
        "min_y": 28, "max_x": 32, "max_y": 36, "area2": 40}
    assert d.fields["area2"][0] == np.dtype(np.int64) and d.fields["length"][0] == np.dtype(np.int32)


def test_contour_polygons():
    from video_segment_amd import render
    import level_contours_cases as tc
    import level_contours_model as tm
    import level_regions_cases as lc
    case = {c.name: c for c in tc.all_cases()}["wide_hole"]
    records, vertices = tm.contours(lc.id_image(case.msg, 0))
    groups = render.contour_polygons(records, vertices)
    assert [len(g) for g in groups] == [3, 1]                 # region 4: outline and two holes; region 9
    assert groups[1][0].tolist() == [[3, 2], [6, 2], [6, 4], [3, 4]]
    assert groups[0][0].tolist() == [[0, 0], [9, 0], [9, 7], [0, 7]]
    assert all(g.dtype == np.int32 and g.shape[1] == 2 for group in groups for g in group)
    assert render.contour_polygons(records[:0], vertices[:0]) == []


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    n, m = C.c_size_t(77), C.c_size_t(77)

    def contours(handle, connect, count_c, count_v, mem_out=0):
        return L.vsg_render_level_contours(handle, b"", 0, 0, connect, None, 0, count_c, None, 0, count_v, mem_out)

    assert contours(None, 0, C.byref(n), C.byref(m)) == -1 and b"null" in L.vsg_render_last_error()
    # everything below is looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert contours(fake, 0, None, C.byref(m)) == -1 and b"count" in L.vsg_render_last_error()
    assert contours(fake, 0, C.byref(n), None) == -1 and b"count" in L.vsg_render_last_error()
    for connect in (0, render.N4, render.N8):
        for mem in (2, -1, 7):
            assert contours(fake, connect, C.byref(n), C.byref(m), mem) == -1
            assert b"mem_out" in L.vsg_render_last_error()
    for connect in (3, -1, 4):
        for mem in (0, 1):
            assert contours(fake, connect, C.byref(n), C.byref(m), mem) == -1
            assert b"connectedness" in L.vsg_render_last_error()
    assert L.vsg_render_last_contour_stats(None, None) == -1
    s = render.VsgRenderContourStats()
    assert L.vsg_render_last_contour_stats(None, C.byref(s)) == -1
