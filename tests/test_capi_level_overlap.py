"""The level overlap additions to the renderer's C ABI: vsg_render_level_overlap and
vsg_render_last_overlap_stats are declared in include/vsg_render.h with the documented signatures and structs,
exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs no device."""
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


def test_header_declares_the_documented_signatures_and_structs(header):
    assert ("int vsg_render_level_overlap(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const int32_t* other, size_t other_pitch, int mem_other, "
            "vsg_render_overlap_row* rows, size_t capacity_rows, size_t* num_rows, "
            "vsg_render_overlap_col* cols, size_t capacity_cols, size_t* num_cols, "
            "vsg_render_overlap_pair* pairs, size_t capacity_pairs, size_t* num_pairs, int mem_out);") in header
    assert "int vsg_render_last_overlap_stats(vsg_render* h, vsg_render_overlap_stats* s);" in header
    assert fields_of(header, "vsg_render_overlap_row") == [
        "int32_t id", "int32_t component", "int32_t first_pair, num_pairs", "int32_t area", "int32_t unlabelled",
        "int32_t best_label", "int32_t best_count"]
    assert fields_of(header, "vsg_render_overlap_col") == [
        "int32_t label", "int32_t area", "int32_t uncovered", "int32_t num_pairs", "int32_t best_row",
        "int32_t best_count"]
    assert fields_of(header, "vsg_render_overlap_pair") == ["int32_t row, col", "int32_t label", "int32_t count"]
    assert fields_of(header, "vsg_render_overlap_stats") == [
        "int64_t covered, labelled, both, runs, rows, cols, pairs, largest_row_pairs",
        "float plane_us, count_us, emit_us, sort_us, table_us", "int launches"]


def test_header_states_the_definition(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("The planes.", "Rows.", "Cols.", "Pairs.",
                   "every negative value means \"no label\"",
                   "area - unlabelled is the sum of the counts of its pairs",
                   "area - uncovered is the sum of the counts of its pairs",
                   "within a row by ascending label, which is ascending col",
                   "A frame with no covered pixel returns zero rows and zero pairs, and still every column",
                   "A B without a label returns zero cols and zero pairs, and still every row"):
        assert phrase in text, phrase
    # the "Not offered" paragraph names the new call
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    assert "Not offered" in head and "vsg_render_level_overlap" in head and "ground truth" in head


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
            "int vsg_render_level_adjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes, "
            "size_t* num_nodes, vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges, "
            "int mem_out);",
            "int vsg_render_last_adjacency_stats(vsg_render* h, vsg_render_adjacency_stats* s);",
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
    for name in ("vsg_render_level_overlap", "vsg_render_last_overlap_stats"):
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_level_overlap.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t,
                                                   C.c_int, vp, C.c_size_t, psz, vp, C.c_size_t, psz, vp,
                                                   C.c_size_t, psz, C.c_int]
    assert L.vsg_render_last_overlap_stats.argtypes == [vp, C.POINTER(render.VsgRenderOverlapStats)]
    assert hasattr(render.SegmentationRenderer, "level_overlap")
    assert hasattr(render.SegmentationRenderer, "last_overlap_stats")
    assert callable(render.overlap_scores)


def test_stats_struct_layout():
    from video_segment_amd import render
    s = render.VsgRenderOverlapStats
    assert [n for n, _ in s._fields_] == ["covered", "labelled", "both", "runs", "rows", "cols", "pairs",
                                          "largest_row_pairs", "plane_us", "count_us", "emit_us", "sort_us",
                                          "table_us", "launches"]
    assert C.sizeof(s) == 8 * 8 + 5 * 4 + 4
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76, 80, 84]


def test_row_col_and_pair_structs_have_no_padding():
    from video_segment_amd import render
    import level_overlap_model as om
    for d, model, names, words in (
            (render.OVERLAP_ROW_DTYPE, om.ROW_DTYPE, ["id", "component", "first_pair", "num_pairs", "area",
                                                      "unlabelled", "best_label", "best_count"],
             render.OVERLAP_ROW_WORDS),
            (render.OVERLAP_COL_DTYPE, om.COL_DTYPE, ["label", "area", "uncovered", "num_pairs", "best_row",
                                                      "best_count"], render.OVERLAP_COL_WORDS),
            (render.OVERLAP_PAIR_DTYPE, om.PAIR_DTYPE, ["row", "col", "label", "count"], render.OVERLAP_PAIR_WORDS)):
        assert d == model and list(d.names) == names and words == len(names) and d.itemsize == 4 * words
        assert [d.fields[n][1] for n in names] == [4 * k for k in range(words)]
        assert all(d.fields[n][0] == np.int32 for n in names)
    assert (render.OVERLAP_ROW_WORDS, render.OVERLAP_COL_WORDS, render.OVERLAP_PAIR_WORDS) == (8, 6, 4)


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    nr, nc, npairs = C.c_size_t(), C.c_size_t(), C.c_size_t()
    counts = (C.byref(nr), C.byref(nc), C.byref(npairs))
    plane = (C.c_int32 * 4)()

    def call(handle, connect, other, mem_other, counts, pitch=0):
        return L.vsg_render_level_overlap(handle, b"", 0, 0, connect, other, pitch, mem_other, None, 0, counts[0],
                                          None, 0, counts[1], None, 0, counts[2], 0)

    assert call(None, 0, plane, 0, counts) == -1
    assert b"null" in L.vsg_render_last_error()
    # count pointers, other, mem_other and connectedness are looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    for k in range(3):
        assert call(fake, 0, plane, 0, counts[:k] + (None,) + counts[k + 1:]) == -1
        assert b"null" in L.vsg_render_last_error()
    for connect in (0, render.N4, render.N8):
        for mem in (0, 1):
            assert call(fake, connect, None, mem, counts) == -1
            assert b"other" in L.vsg_render_last_error() and b"null" in L.vsg_render_last_error()
        for mem in (2, -1, 7):
            assert call(fake, connect, plane, mem, counts) == -1
            assert b"mem_other" in L.vsg_render_last_error()
    for connect in (3, -1, 4):
        for mem in (0, 1):
            assert call(fake, connect, plane, mem, counts) == -1
            assert b"connectedness" in L.vsg_render_last_error()
    assert L.vsg_render_last_overlap_stats(None, None) == -1
    s = render.VsgRenderOverlapStats()
    assert L.vsg_render_last_overlap_stats(None, C.byref(s)) == -1
