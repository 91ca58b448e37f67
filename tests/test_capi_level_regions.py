"""The level region additions to the renderer's C ABI: vsg_render_level_regions and
vsg_render_last_level_stats are declared in include/vsg_render.h with the documented signatures and
structs, exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs no
device."""
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
    assert ("int vsg_render_level_regions(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "vsg_render_level_region* regions, size_t capacity_regions, size_t* num_regions, "
            "int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int mem_out);") in header
    assert "int vsg_render_last_level_stats(vsg_render* h, vsg_render_level_stats* s);" in header
    assert fields_of(header, "vsg_render_level_region") == [
        "int32_t id", "int32_t first_interval", "int32_t num_intervals", "int32_t area",
        "int32_t min_x, min_y, max_x, max_y", "float size, mean_x, mean_y, moment_xx, moment_xy, moment_yy"]
    assert fields_of(header, "vsg_render_level_stats") == [
        "int64_t runs, regions, largest_region_intervals", "float runs_us, sort_us, table_us, moments_us",
        "int launches"]


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** h);",
            "int vsg_render_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, "
            "size_t stride, int mem_in, uint8_t* out, size_t out_stride, int mem_out);",
            "int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);",
            "int vsg_render_rasterize(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* out, "
            "size_t capacity_intervals, size_t* count, int mem_out);",
            "int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s);",
            "int vsg_render_last_vector_stats(vsg_render* h, vsg_render_vector_stats* s);",
            "void vsg_render_color(int region_id, uint8_t c[3]);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in ("vsg_render_level_regions", "vsg_render_last_level_stats"):
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_level_regions.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, vp, C.c_size_t, psz,
                                                   vp, C.c_size_t, psz, C.c_int]
    s = render.VsgRenderLevelStats
    assert [n for n, _ in s._fields_] == ["runs", "regions", "largest_region_intervals", "runs_us", "sort_us",
                                          "table_us", "moments_us", "launches"]
    assert C.sizeof(s) == 3 * 8 + 4 * 4 + 4 + 4 and s.runs_us.offset == 24 and s.launches.offset == 40
    assert hasattr(render.SegmentationRenderer, "level_regions")
    assert hasattr(render.SegmentationRenderer, "last_level_stats")


def test_region_struct_is_56_bytes_without_padding():
    from video_segment_amd import render
    import level_regions_model as lm
    d = render.LEVEL_REGION_DTYPE
    assert d.itemsize == 56 and d == lm.REGION_DTYPE
    names = ["id", "first_interval", "num_intervals", "area", "min_x", "min_y", "max_x", "max_y", "size", "mean_x",
             "mean_y", "moment_xx", "moment_xy", "moment_yy"]
    assert list(d.names) == names
    assert [d.fields[n][1] for n in names] == [4 * k for k in range(14)]
    assert all(d.fields[n][0] == np.int32 for n in names[:8]) and all(d.fields[n][0] == np.float32 for n in names[8:])
    assert render.LEVEL_REGION_WORDS * 4 == 56


def test_null_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    nr, ni = C.c_size_t(), C.c_size_t()
    assert L.vsg_render_level_regions(None, b"", 0, 0, None, 0, C.byref(nr), None, 0, C.byref(ni), 0) == -1
    assert b"null" in L.vsg_render_last_error()
    # the count pointers are looked at after the handle only; a non-null handle is never dereferenced
    # before them
    fake = C.create_string_buffer(8)
    assert L.vsg_render_level_regions(C.cast(fake, C.c_void_p), b"", 0, 0, None, 0, None, None, 0, C.byref(ni), 0) == -1
    assert L.vsg_render_level_regions(C.cast(fake, C.c_void_p), b"", 0, 0, None, 0, C.byref(nr), None, 0, None, 0) == -1
    assert L.vsg_render_last_level_stats(None, None) == -1
    s = render.VsgRenderLevelStats()
    assert L.vsg_render_last_level_stats(None, C.byref(s)) == -1
