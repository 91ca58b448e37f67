"""The level component additions to the renderer's C ABI: vsg_render_level_components and
vsg_render_last_component_stats are declared in include/vsg_render.h with the documented signatures
and structs, exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs
no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "vsg_render.h")) as f:
        text = f.read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def fields_of(header, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header)
    assert m, name
    return [f.strip() for f in m.group(1).split(";") if f.strip()]


def test_header_declares_the_documented_signatures_and_structs(header):
    assert ("int vsg_render_level_components(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, vsg_render_level_component* components, size_t capacity_components, "
            "size_t* num_components, int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, "
            "int32_t* label_image, int mem_out);") in header
    assert "int vsg_render_last_component_stats(vsg_render* h, vsg_render_component_stats* s);" in header
    assert "#define VSG_RENDER_CONNECT_N4 1" in header and "#define VSG_RENDER_CONNECT_N8 2" in header
    assert fields_of(header, "vsg_render_level_component") == [
        "int32_t id", "int32_t component", "int32_t region_components", "int32_t first_interval, num_intervals",
        "int32_t area", "int32_t min_x, min_y, max_x, max_y",
        "float size, mean_x, mean_y, moment_xx, moment_xy, moment_yy"]
    assert fields_of(header, "vsg_render_component_stats") == [
        "int64_t runs, regions, components, links, largest_component_intervals",
        "float runs_us, sort_us, link_us, order_us, moments_us, label_us", "int launches"]


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
            "int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s);",
            "int vsg_render_last_vector_stats(vsg_render* h, vsg_render_vector_stats* s);",
            "void vsg_render_color(int region_id, uint8_t c[3]);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in ("vsg_render_level_components", "vsg_render_last_component_stats"):
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_level_components.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t,
                                                      psz, vp, C.c_size_t, psz, vp, C.c_int]
    s = render.VsgRenderComponentStats
    assert [n for n, _ in s._fields_] == ["runs", "regions", "components", "links", "largest_component_intervals",
                                          "runs_us", "sort_us", "link_us", "order_us", "moments_us", "label_us",
                                          "launches"]
    assert C.sizeof(s) == 5 * 8 + 6 * 4 + 4 + 4 and s.runs_us.offset == 40 and s.launches.offset == 64
    assert (render.N4, render.N8) == (1, 2)
    assert hasattr(render.SegmentationRenderer, "level_components")
    assert hasattr(render.SegmentationRenderer, "last_component_stats")


def test_component_struct_is_64_bytes_without_padding():
    from video_segment_amd import render
    import level_components_model as cm
    d = render.LEVEL_COMPONENT_DTYPE
    assert d.itemsize == 64 and d == cm.COMPONENT_DTYPE
    names = ["id", "component", "region_components", "first_interval", "num_intervals", "area", "min_x", "min_y",
             "max_x", "max_y", "size", "mean_x", "mean_y", "moment_xx", "moment_xy", "moment_yy"]
    assert list(d.names) == names
    assert [d.fields[n][1] for n in names] == [4 * k for k in range(16)]
    assert all(d.fields[n][0] == np.int32 for n in names[:10]) and all(d.fields[n][0] == np.float32 for n in names[10:])
    assert render.LEVEL_COMPONENT_WORDS * 4 == 64
    assert (cm.N4, cm.N8) == (render.N4, render.N8)


def test_null_arguments_and_a_bad_connectedness_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    nc, ni = C.c_size_t(), C.c_size_t()

    def call(handle, connect, p_nc, p_ni):
        return L.vsg_render_level_components(handle, b"", 0, 0, connect, None, 0, p_nc, None, 0, p_ni, None, 0)

    assert call(None, render.N4, C.byref(nc), C.byref(ni)) == -1
    assert b"null" in L.vsg_render_last_error()
    # count pointers and connectedness are looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert call(fake, render.N4, None, C.byref(ni)) == -1
    assert call(fake, render.N8, C.byref(nc), None) == -1
    for connect in (0, 3, -1, 4):
        assert call(fake, connect, C.byref(nc), C.byref(ni)) == -1
        assert b"connectedness" in L.vsg_render_last_error()
    assert L.vsg_render_last_component_stats(None, None) == -1
    s = render.VsgRenderComponentStats()
    assert L.vsg_render_last_component_stats(None, C.byref(s)) == -1
