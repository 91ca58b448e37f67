"""The level adjacency additions to the renderer's C ABI: vsg_render_level_adjacency and
vsg_render_last_adjacency_stats are declared in include/vsg_render.h with the documented signatures, defines
and structs, exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs no
device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_header_declares_the_documented_signatures_defines_and_structs(header):
    assert ("int vsg_render_level_adjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes, "
            "size_t* num_nodes, vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges, "
            "int mem_out);") in header
    assert "int vsg_render_last_adjacency_stats(vsg_render* h, vsg_render_adjacency_stats* s);" in header
    assert "#define VSG_RENDER_ADJACENT_N4 1" in header and "#define VSG_RENDER_ADJACENT_N8 2" in header
    assert fields_of(header, "vsg_render_level_node") == [
        "int32_t id", "int32_t component", "int32_t first_edge, num_edges", "int32_t border_frame",
        "int32_t border_uncovered", "int32_t border_shared"]
    assert fields_of(header, "vsg_render_level_edge") == [
        "int32_t neighbour", "int32_t neighbour_id", "int32_t shared_n4", "int32_t shared_diagonal"]
    assert fields_of(header, "vsg_render_adjacency_stats") == [
        "int64_t sides, keys, nodes, edges, largest_node_edges",
        "float plane_us, count_us, emit_us, sort_us, table_us", "int launches"]


def test_header_states_the_definition(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("The plane.", "Sides.", "Diagonal contacts.", "Nodes.", "Edges.",
                   "border_frame + border_uncovered + border_shared is the group's perimeter",
                   "a -> b is listed iff b -> a is",
                   "A frame with no covered pixel returns zero nodes and zero edges"):
        assert phrase in text, phrase
    # the "Not offered" paragraph names the new call
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    assert "Not offered" in head and "vsg_render_level_adjacency" in head


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** h);",
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
            "size_t* num_boundaries, int32_t* points, size_t capacity_points, size_t* num_points, "
            "int mem_out);",
            "int vsg_render_last_boundary_stats(vsg_render* h, vsg_render_boundary_stats* s);",
            "int vsg_render_last_component_stats(vsg_render* h, vsg_render_component_stats* s);",
            "int vsg_render_last_level_stats(vsg_render* h, vsg_render_level_stats* s);",
            "int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s);",
            "void vsg_render_color(int region_id, uint8_t c[3]);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in ("vsg_render_level_adjacency", "vsg_render_last_adjacency_stats"):
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_level_adjacency.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, vp,
                                                     C.c_size_t, psz, vp, C.c_size_t, psz, C.c_int]
    assert L.vsg_render_last_adjacency_stats.argtypes == [vp, C.POINTER(render.VsgRenderAdjacencyStats)]
    assert (render.ADJACENT_N4, render.ADJACENT_N8) == (1, 2)
    assert hasattr(render.SegmentationRenderer, "level_adjacency")
    assert hasattr(render.SegmentationRenderer, "last_adjacency_stats")


def test_stats_struct_layout():
    from video_segment_amd import render
    s = render.VsgRenderAdjacencyStats
    assert [n for n, _ in s._fields_] == ["sides", "keys", "nodes", "edges", "largest_node_edges", "plane_us",
                                          "count_us", "emit_us", "sort_us", "table_us", "launches"]
    assert C.sizeof(s) == 5 * 8 + 5 * 4 + 4
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]


def test_node_and_edge_structs_have_no_padding():
    from video_segment_amd import render
    import level_adjacency_model as am
    d = render.LEVEL_NODE_DTYPE
    names = ["id", "component", "first_edge", "num_edges", "border_frame", "border_uncovered", "border_shared"]
    assert d.itemsize == 28 and d == am.NODE_DTYPE and list(d.names) == names
    assert [d.fields[n][1] for n in names] == [0, 4, 8, 12, 16, 20, 24]
    assert all(d.fields[n][0] == np.int32 for n in names)
    assert render.LEVEL_NODE_WORDS == 7
    d = render.LEVEL_EDGE_DTYPE
    names = ["neighbour", "neighbour_id", "shared_n4", "shared_diagonal"]
    assert d.itemsize == 16 and d == am.EDGE_DTYPE and list(d.names) == names
    assert [d.fields[n][1] for n in names] == [0, 4, 8, 12]
    assert all(d.fields[n][0] == np.int32 for n in names)
    assert render.LEVEL_EDGE_WORDS == 4
    assert (am.ADJACENT_N4, am.ADJACENT_N8) == (render.ADJACENT_N4, render.ADJACENT_N8)


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    nn, ne = C.c_size_t(), C.c_size_t()

    def call(handle, connect, hood, p_nn, p_ne):
        return L.vsg_render_level_adjacency(handle, b"", 0, 0, connect, hood, None, 0, p_nn, None, 0, p_ne, 0)

    assert call(None, 0, render.ADJACENT_N4, C.byref(nn), C.byref(ne)) == -1
    assert b"null" in L.vsg_render_last_error()
    # count pointers, connectedness and neighbourhood are looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert call(fake, 0, render.ADJACENT_N4, None, C.byref(ne)) == -1
    assert b"null" in L.vsg_render_last_error()
    assert call(fake, render.N8, render.ADJACENT_N8, C.byref(nn), None) == -1
    assert b"null" in L.vsg_render_last_error()
    for connect in (3, -1, 4):
        for hood in (render.ADJACENT_N4, render.ADJACENT_N8):
            assert call(fake, connect, hood, C.byref(nn), C.byref(ne)) == -1
            assert b"connectedness" in L.vsg_render_last_error()
    for hood in (0, 3, -1):
        for connect in (0, render.N4, render.N8):
            assert call(fake, connect, hood, C.byref(nn), C.byref(ne)) == -1
            assert b"neighbourhood" in L.vsg_render_last_error()
    assert L.vsg_render_last_adjacency_stats(None, None) == -1
    s = render.VsgRenderAdjacencyStats()
    assert L.vsg_render_last_adjacency_stats(None, C.byref(s)) == -1
