"""The level boundary additions to the renderer's C ABI: vsg_render_level_boundaries and
vsg_render_last_boundary_stats are declared in include/vsg_render.h with the documented signatures and
structs, exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs no
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


def test_header_declares_the_documented_signatures_and_structs(header):
    assert ("int vsg_render_level_boundaries(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, int which, vsg_render_level_boundary* boundaries, size_t capacity_boundaries, "
            "size_t* num_boundaries, int32_t* points, size_t capacity_points, size_t* num_points, "
            "int mem_out);") in header
    assert "int vsg_render_last_boundary_stats(vsg_render* h, vsg_render_boundary_stats* s);" in header
    assert "#define VSG_RENDER_BOUNDARY_INNER 0" in header and "#define VSG_RENDER_BOUNDARY_OUTER 1" in header
    assert fields_of(header, "vsg_render_level_boundary") == [
        "int32_t id", "int32_t component", "int32_t first_point, num_points"]
    assert fields_of(header, "vsg_render_boundary_stats") == [
        "int64_t points, boundaries, largest_boundary_points",
        "float plane_us, count_us, emit_us, sort_us, table_us", "int launches"]


def test_header_cites_get_boundary_where_it_is_and_states_both_findings(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    assert "segment_util/segmentation_boundary" in text
    assert "GetBoundary, segmentation/boundary.cpp" not in text
    assert "reference_x = x + 1" in text
    assert "one byte before the first row" in text and "one byte past the last row" in text


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** h);",
            "int vsg_render_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, "
            "size_t stride, int mem_in, uint8_t* out, size_t out_stride, int mem_out);",
            "int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);",
            "int vsg_render_rasterize(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* out, "
            "size_t capacity_intervals, size_t* count, int mem_out);",
            "int vsg_render_level_regions(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "vsg_render_level_region* regions, size_t capacity_regions, size_t* num_regions, "
            "int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int mem_out);",
            "int vsg_render_last_level_stats(vsg_render* h, vsg_render_level_stats* s);",
            "int vsg_render_level_components(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, vsg_render_level_component* components, size_t capacity_components, "
            "size_t* num_components, int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, "
            "int32_t* label_image, int mem_out);",
            "int vsg_render_last_component_stats(vsg_render* h, vsg_render_component_stats* s);",
            "int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s);",
            "int vsg_render_last_vector_stats(vsg_render* h, vsg_render_vector_stats* s);",
            "void vsg_render_color(int region_id, uint8_t c[3]);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in ("vsg_render_level_boundaries", "vsg_render_last_boundary_stats"):
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_level_boundaries.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, vp,
                                                      C.c_size_t, psz, vp, C.c_size_t, psz, C.c_int]
    s = render.VsgRenderBoundaryStats
    assert [n for n, _ in s._fields_] == ["points", "boundaries", "largest_boundary_points", "plane_us", "count_us",
                                          "emit_us", "sort_us", "table_us", "launches"]
    assert C.sizeof(s) == 3 * 8 + 5 * 4 + 4 and s.plane_us.offset == 24 and s.launches.offset == 44
    assert (render.BOUNDARY_INNER, render.BOUNDARY_OUTER) == (0, 1)
    assert hasattr(render.SegmentationRenderer, "level_boundaries")
    assert hasattr(render.SegmentationRenderer, "last_boundary_stats")


def test_boundary_struct_is_16_bytes_without_padding():
    from video_segment_amd import render
    import level_boundaries_model as bm
    d = render.LEVEL_BOUNDARY_DTYPE
    assert d.itemsize == 16 and d == bm.BOUNDARY_DTYPE
    names = ["id", "component", "first_point", "num_points"]
    assert list(d.names) == names
    assert [d.fields[n][1] for n in names] == [0, 4, 8, 12]
    assert all(d.fields[n][0] == np.int32 for n in names)
    assert render.LEVEL_BOUNDARY_WORDS * 4 == 16


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    nb, npts = C.c_size_t(), C.c_size_t()

    def call(handle, connect, which, p_nb, p_np):
        return L.vsg_render_level_boundaries(handle, b"", 0, 0, connect, which, None, 0, p_nb, None, 0, p_np, 0)

    assert call(None, 0, 0, C.byref(nb), C.byref(npts)) == -1
    assert b"null" in L.vsg_render_last_error()
    # count pointers, connectedness and which are looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert call(fake, 0, 0, None, C.byref(npts)) == -1
    assert call(fake, render.N8, 1, C.byref(nb), None) == -1
    for connect in (3, -1, 4):
        assert call(fake, connect, 0, C.byref(nb), C.byref(npts)) == -1
        assert b"connectedness" in L.vsg_render_last_error()
    for which in (2, -1):
        for connect in (0, render.N4, render.N8):
            assert call(fake, connect, which, C.byref(nb), C.byref(npts)) == -1
            assert b"which" in L.vsg_render_last_error()
    assert L.vsg_render_last_boundary_stats(None, None) == -1
    s = render.VsgRenderBoundaryStats()
    assert L.vsg_render_last_boundary_stats(None, C.byref(s)) == -1
